// vafc_vcf.hip -- vcf-vaf-counter on the device (vc_vcf_* of include/vafc.h):
// the reference's find_pattern (vcf-vaf-counter.c:83-92), a strcmp scan of all
// rows for every record, as one pass over the raw VCF text that joins each
// line's CHROM and POS against a hash table of the rows.
//
//   tail kernel   the block's last '\n': a non-final block is scanned up to it
//   scan kernel   tiles of 4 KB.  Every lane loads 16 aligned bytes once and
//                 compares them with '\n'; the line starts of a wave's 1 KB
//                 are ranked with ballot and popcount and listed in LDS; then
//                 each lane takes one line and reads its first five columns
//                 byte by byte from the tile's copy in LDS (with 256 bytes of
//                 the next tile; beyond those from global memory).  A line
//                 with one-byte REF and ALT is looked up; what the lane will
//                 not decide is reported with row = -1 (the device never
//                 guesses).  Reports are appended with one atomic per wave.
//   table         open addressing, linear probes, keyed by (FNV-1a of chr,
//                 start); an entry holds the first row of its (chr, start) and
//                 the offset of the chr bytes, which are compared on a hash
//                 match.  20,849 rows make 512 KB: it stays in L2.
//
//   BGZF input    (vc_vcf_count_file) is inflated on the device: compressed
//                 members go over PCIe, the inflater's kernel (vafc_bgzf.hip)
//                 writes the text into HBM and the two kernels above scan it
//                 there; see count_bgzf_device below.
//
// Every global read is bounded: text by the bytes the tail kernel allows
// (<= len; an aligned 16-byte load is issued only if it holds one of them, so
// it stays inside that byte's page), table entries by the slot mask, names by
// their stored length, the hit list by its capacity (overflow is counted, not
// written).  Nothing here decides on the CPU what the kernel should have: a
// HIP failure is returned as VC_EHIP.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "vafc.h"
#include "vafc_bgzf.h"
#include "vafc_stage.h"
#include "vafc_vcf.h"

namespace {

const int VCF_BLOCK = 256;
const int VCF_WAVES = VCF_BLOCK / 64;
const uint32_t VCF_WAVE_BYTES = 64 * 16;
typedef uint32_t vcf_u32x4 __attribute__((ext_vector_type(4)));   // 16 bytes in registers (a uint4 held across a branch goes through the stack)
const uint32_t VCF_HALO = 256;   // bytes of the next tile staged with a tile: most first-five-column reads end inside
static_assert(VCF_BLOCK * 16 == VC_VCF_TILE_BYTES, "a tile is one 16-byte load per lane");
const uint32_t VCF_EMPTY = 0xFFFFFFFFu;
const uint32_t VCF_MAX_CHR = 255;
const size_t VCF_BLOCK_BYTES = (size_t)32 << 20;
const size_t VCF_MAX_HITS = (size_t)1 << 20;
// BGZF input without $VAFC_BGZF: inflated on the device (DESIGN 15 has the measurement that decided it)
const bool VCF_BGZF_DEFAULT_DEVICE = true;

struct VcVcfArgs {
	const uint8_t *text;         // the block, any alignment
	uint64_t len;
	uint64_t file_off;
	int final_block;
	uint64_t *consumed;          // written by the tail kernel, read by the scan kernel
	const uint4 *table;          // x: FNV-1a of chr, y: start, z: first row (VCF_EMPTY: free), w: offset of the name
	uint32_t mask;               // slots - 1
	const uint8_t *names;        // at an entry's w: the length byte, then the bytes
	const uint16_t *row_ra;      // [n_rows] ref | alt << 8
	uint4 *hits;                 // x, y: offset, z: row
	uint32_t cap;
	unsigned long long *n_hits;  // lines reported, beyond cap included
};

__host__ __device__ inline uint32_t vcf_fnv_step(uint32_t h, uint32_t c) { return (h ^ c) * 16777619u; }
const uint32_t VCF_FNV0 = 2166136261u;

__host__ __device__ inline uint32_t vcf_slot(uint32_t h, int32_t start, uint32_t mask)
{
	uint32_t x = h ^ ((uint32_t)start * 0x9E3779B1u);
	x ^= x >> 15;
	x *= 0x85EBCA6Bu;
	x ^= x >> 13;
	return x & mask;
}

// Bit b set: byte b of w is '\n'.
__device__ inline uint32_t vcf_nl4(uint32_t w)
{
	const uint32_t x = w ^ 0x0A0A0A0Au;
	const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 where a byte of x is 0
	return ((t >> 7) * 0x01020408u) >> 24;
}

// The first five columns of a line that starts at p, read through rd up to
// `end`: 0 with hd filled, 1 for a line the device will not decide, 2 when
// `end` came before the fifth tab.
struct VcfHead {
	uint32_t h, clen, r0, a0;
	uint64_t pos;
	bool one_ref, one_alt;
};

template <class Idx, class Rd> __device__ __forceinline__ int vcf_head(VcfHead &hd, Idx p, Idx end, Rd rd)
{
	// CHROM
	uint32_t h = VCF_FNV0, clen = 0, c = 0;
	for (; p < end; ++p) {
		c = rd(p);
		if (c < 32) break;
		h = vcf_fnv_step(h, c);
		++clen;
	}
	if (p >= end) return 2;
	if (c != '\t' || clen == 0 || clen > VCF_MAX_CHR) return 1;
	hd.h = h;
	hd.clen = clen;
	// POS: 1..18 digits
	uint64_t pos = 0;
	uint32_t digits = 0;
	for (++p; p < end; ++p, ++digits) {
		c = rd(p);
		if (c < '0' || c > '9' || digits == 19) break;
		pos = pos * 10 + (c - '0');
	}
	if (p >= end) return 2;
	if (c != '\t' || digits == 0 || digits > 18) return 1;
	hd.pos = pos;
	// ID
	for (++p; p < end && (c = rd(p)) >= 32; ++p) {}
	if (p >= end) return 2;
	if (c != '\t') return 1;
	// REF, ALT: the first byte and whether it is the only one
	Idx s0 = ++p;
	for (; p < end && (c = rd(p)) >= 32; ++p) {}
	if (p >= end) return 2;
	if (c != '\t') return 1;
	hd.one_ref = p - s0 == 1;
	hd.r0 = p > s0 ? rd(s0) : 0;
	s0 = ++p;
	for (; p < end && (c = rd(p)) >= 32; ++p) {}
	if (p >= end) return 2;
	if (c != '\t') return 1;
	hd.one_alt = p - s0 == 1;
	hd.a0 = p > s0 ? rd(s0) : 0;
	return 0;
}

// The offset behind the block's last '\n' (0: none), or len for a final block.
__global__ void __launch_bounds__(VCF_BLOCK) vcf_tail_kernel(VcVcfArgs A)
{
	__shared__ unsigned long long found;
	if (A.final_block) {
		if (threadIdx.x == 0) *A.consumed = A.len;
		return;
	}
	if (threadIdx.x == 0) found = 0;
	__syncthreads();
	for (uint64_t hi = A.len; hi > 0;) {
		const uint64_t lo = hi > (uint64_t)VC_VCF_TILE_BYTES ? hi - VC_VCF_TILE_BYTES : 0;
		unsigned long long best = 0;
		for (uint64_t p = lo + (uint64_t)threadIdx.x * 16, e = p + 16 < hi ? p + 16 : hi; p < e; ++p)
			if (A.text[p] == '\n') best = p + 1;
		if (best) atomicMax(&found, best);
		__syncthreads();
		const unsigned long long f = found;
		__syncthreads();   // every lane has read it before the next chunk may write
		if (f) break;      // the same in every lane
		hi = lo;
	}
	if (threadIdx.x == 0) *A.consumed = found;
}

__global__ void __launch_bounds__(VCF_BLOCK) vcf_scan_kernel(VcVcfArgs A)
{
	__shared__ uint16_t starts[VCF_WAVES][VCF_WAVE_BYTES];
	__shared__ vcf_u32x4 tile_text[VCF_BLOCK + VCF_HALO / 16];   // the tile's bytes and the first of the next tile's
	const uint64_t E = *A.consumed;   // bytes [0, E) are scanned; E <= len
	if (E == 0) return;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const unsigned long long lt = ((unsigned long long)1 << lane) - 1;
	const uint64_t skew = (uint64_t)((uintptr_t)A.text & 15);
	const uint8_t *abase = A.text - skew;   // 16-byte aligned
	const uint64_t span = skew + E;         // aligned offsets [skew, span) hold the text
	const uint64_t n_tiles = (span + VC_VCF_TILE_BYTES - 1) / VC_VCF_TILE_BYTES;
	for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		const uint64_t a = tile * VC_VCF_TILE_BYTES + (uint64_t)wave * VCF_WAVE_BYTES + (uint64_t)lane * 16;
		uint32_t nl = 0, valid = 0;
		vcf_u32x4 v = {0u, 0u, 0u, 0u};
		if (threadIdx.x < VCF_HALO / 16) {
			const uint64_t ha = (tile + 1) * VC_VCF_TILE_BYTES + (uint64_t)threadIdx.x * 16;
			tile_text[VCF_BLOCK + threadIdx.x] = ha < span ? *reinterpret_cast<const vcf_u32x4 *>(abase + ha) : v;
		}
		if (a + 16 > skew && a < span) {
			v = *reinterpret_cast<const vcf_u32x4 *>(abase + a);
			nl = vcf_nl4(v.x) | vcf_nl4(v.y) << 4 | vcf_nl4(v.z) << 8 | vcf_nl4(v.w) << 12;
			const uint32_t lo = a < skew ? (uint32_t)(skew - a) : 0, hi = span - a < 16 ? (uint32_t)(span - a) : 16;
			valid = (0xFFFFu << lo) & (0xFFFFu >> (16 - hi));
			nl &= valid;
		}
		tile_text[threadIdx.x] = v;
		// a line starts at text offset 0 and behind every '\n'
		uint32_t carry = (uint32_t)__shfl_up((int)(nl >> 15), 1, 64);
		if (lane == 0) carry = (a > skew && a < span) ? (abase[a - 1] == '\n') : 0;
		uint32_t st = ((nl << 1) | carry) & valid;
		if (a <= skew && skew < a + 16) st |= 1u << (skew - a);
		// rank the wave's starts.  Lines of 16 bytes or more give a lane at most
		// one: one ballot ranks them; otherwise bit q of every lane in turn
		uint32_t total;
		if (__ballot((st & (st - 1)) != 0) == 0) {
			const unsigned long long b = __ballot(st != 0);
			if (st) starts[wave][__popcll(b & lt)] = (uint16_t)(lane * 16 + (__ffs((int)st) - 1));
			total = (uint32_t)__popcll(b);
		} else {
			total = 0;
			for (int qb = 0; qb < 16; ++qb) {
				const bool mine = (st >> qb) & 1u;
				const unsigned long long b = __ballot(mine);
				if (mine) starts[wave][total + __popcll(b & lt)] = (uint16_t)(lane * 16 + qb);
				total += (uint32_t)__popcll(b);
			}
		}
		__syncthreads();
		const uint64_t tile_a = tile * VC_VCF_TILE_BYTES;
		// the staged bytes that are text: tile-relative [.., staged_end)
		const uint32_t staged_end = span - tile_a < VC_VCF_TILE_BYTES + VCF_HALO ? (uint32_t)(span - tile_a) : VC_VCF_TILE_BYTES + VCF_HALO;
		const uint8_t *staged = reinterpret_cast<const uint8_t *>(tile_text);
		for (uint32_t base = 0; base < total; base += 64) {   // total is the same in every lane of the wave
			const uint32_t i = base + (uint32_t)lane;
			bool emit = false;
			uint32_t row = VCF_EMPTY;
			uint64_t off = 0;
			if (i < total) {
				const uint32_t ks = (uint32_t)wave * VCF_WAVE_BYTES + starts[wave][i];   // tile-relative
				off = tile_a + ks - skew;   // offset in the text
				VcfHead hd = {0u, 0u, 0u, 0u, 0ull, false, false};
				// from the tile's copy in LDS; a line that runs past it is read again from global memory
				const uint8_t *text = A.text;
				int rc = vcf_head(hd, ks, staged_end, [=](uint32_t k) -> uint32_t { return staged[k]; });
				bool in_lds = true;
				if (rc == 2 && tile_a + staged_end < span) {
					in_lds = false;
					rc = vcf_head(hd, off, E, [=](uint64_t q) -> uint32_t { return text[q]; });
				}
				const bool bad = rc != 0;
				const uint32_t h = hd.h, clen = hd.clen, r0 = hd.r0, a0 = hd.a0;
				const uint64_t pos = hd.pos;
				const uint32_t rlen = hd.one_ref ? 1 : 0, alen = hd.one_alt ? 1 : 0;
				auto rd = [=](uint64_t q) -> uint32_t { return in_lds ? staged[ks + (uint32_t)(q - off)] : text[q]; };
				if (bad) {
					emit = true;   // left to the host
				} else if (rlen == 1 && alen == 1 && a0 != '.' && a0 != ',') {
					const int32_t start = (int32_t)(uint32_t)(pos - 1);   // (int)(POS - 1)
					const uint32_t ra = r0 | a0 << 8;
					uint32_t slot = vcf_slot(h, start, A.mask);
					for (uint32_t probe = 0; probe <= A.mask; ++probe, slot = (slot + 1) & A.mask) {
						const uint4 e = A.table[slot];
						if (e.z == VCF_EMPTY) break;
						if (e.x != h || (int32_t)e.y != start) continue;
						const uint8_t *nm = A.names + e.w;
						if (nm[0] != clen) continue;
						bool same = true;
						for (uint32_t k = 0; k < clen; ++k) same = same && nm[1 + k] == rd(off + k);
						if (!same) continue;
						// the first row of this (chr, start): no other row is tried
						if (A.row_ra[e.z] == ra) {
							emit = true;
							row = e.z;
						}
						break;
					}
				}
			}
			const unsigned long long eb = __ballot(emit);
			if (eb) {   // one atomic for the wave
				unsigned long long first = 0;
				if (lane == __ffsll(eb) - 1) first = atomicAdd(A.n_hits, (unsigned long long)__popcll(eb));
				first = __shfl(first, __ffsll(eb) - 1, 64);
				const unsigned long long idx = first + (unsigned long long)__popcll(eb & lt);
				if (emit && idx < A.cap) {
					const uint64_t fo = A.file_off + off;
					A.hits[idx] = make_uint4((uint32_t)fo, (uint32_t)(fo >> 32), row, 0u);
				}
			}
		}
		__syncthreads();   // the list is rewritten by the next tile
	}
}

struct Pending {
	const uint8_t *d_text = nullptr;
	uint64_t len = 0, file_off = 0;
	int final_block = 0;
	hipStream_t st = nullptr;
	bool active = false;
};

} // namespace

struct vc_vcf : VcDevice {
	uint32_t n_rows = 0;
	VcDevBuf<uint4> d_table;
	uint32_t mask = 0;
	VcDevBuf<uint8_t> d_names;
	VcDevBuf<uint16_t> d_row_ra;
	VcDevBuf<uint4> d_hits;       // max_hits entries once a scan has run
	size_t max_hits = VCF_MAX_HITS;
	VcDevBuf<unsigned long long> d_n_hits;
	VcDevBuf<uint64_t> d_consumed;
	size_t block_bytes = VCF_BLOCK_BYTES;
	Pending pend;
	std::vector<vc_vcf_hit> acc;  // collected since the last vc_vcf_hits
	bool handed = false;          // acc was returned: the next scan starts a new list
	size_t last_consumed = 0;
	uint64_t lines_reported = 0;
	// the rows on the host, for the lines the device leaves to it
	std::unordered_map<std::string, uint32_t> first_row;   // chr + '\t' + start
	std::vector<uint16_t> row_ra;
	// BGZF input inflated on the device (created by the first such file)
	vc_bgzf *zf = nullptr;
	VcDevBuf<uint8_t> ztext[2];   // the text of two pieces in turn, each behind `zhead` bytes of room for a tail
	size_t zhead[2] = {0, 0};
	uint64_t z_device_blocks = 0, z_host_blocks = 0;   // vc_vcf_inflate_info
};

namespace {

std::string host_key(const char *chr, size_t len, int32_t start)
{
	std::string k(chr, len);
	k.push_back('\t');
	k += std::to_string(start);
	return k;
}

int launch(vc_vcf *c, const Pending &p)
{
	if (c->d_hits.cap != c->max_hits) HIPCK(c->d_hits.grow(c->max_hits));   // max_hits >= 1
	VcVcfArgs A;
	A.text = p.d_text;
	A.len = p.len;
	A.file_off = p.file_off;
	A.final_block = p.final_block;
	A.consumed = c->d_consumed;
	A.table = c->d_table;
	A.mask = c->mask;
	A.names = c->d_names;
	A.row_ra = c->d_row_ra;
	A.hits = c->d_hits;
	A.cap = (uint32_t)(c->d_hits.cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : c->d_hits.cap);
	A.n_hits = c->d_n_hits;
	HIPCK(c->d_n_hits.zero_async(p.st));
	HIPCK(c->timer.begin(p.st));
	hipLaunchKernelGGL(vcf_tail_kernel, dim3(1), dim3(VCF_BLOCK), 0, p.st, A);
	HIPCK(hipGetLastError());
	uint64_t grid = (p.len + 16 + VC_VCF_TILE_BYTES - 1) / VC_VCF_TILE_BYTES;
	if (grid > (uint64_t)c->n_cu * 8) grid = (uint64_t)c->n_cu * 8;
	hipLaunchKernelGGL(vcf_scan_kernel, dim3((unsigned)grid), dim3(VCF_BLOCK), 0, p.st, A);
	HIPCK(hipGetLastError());
	HIPCK(c->timer.end(p.st));
	return VC_OK;
}

// Wait for the pending scan and move its lines into acc; a list that was too
// short is made as long as the count says and the scan is run again.
int collect(vc_vcf *c)
{
	if (!c->pend.active) return VC_OK;
	for (;;) {
		HIPCK(hipStreamSynchronize(c->pend.st));
		unsigned long long n = 0;
		uint64_t consumed = 0;
		HIPCK(hipMemcpy(&n, c->d_n_hits, sizeof n, hipMemcpyDeviceToHost));
		HIPCK(hipMemcpy(&consumed, c->d_consumed, sizeof consumed, hipMemcpyDeviceToHost));
		if (n > c->d_hits.cap) {
			c->max_hits = (size_t)n;
			const int rc = launch(c, c->pend);
			if (rc != VC_OK) return rc;
			continue;
		}
		const size_t at = c->acc.size();
		c->acc.resize(at + (size_t)n);
		if (n) HIPCK(hipMemcpy(c->acc.data() + at, c->d_hits, (size_t)n * sizeof(uint4), hipMemcpyDeviceToHost));
		c->last_consumed = (size_t)consumed;
		c->lines_reported += n;
		break;
	}
	c->pend.active = false;
	c->stage.settle();
	return VC_OK;
}

static_assert(sizeof(vc_vcf_hit) == sizeof(uint4), "a hit is written as one 16-byte store");

// The rows of an open handle, on the host and as the device table.
int vcf_fill(vc_vcf *c, const char *const *chr, const int32_t *start, const char *ref, const char *alt, size_t n,
             size_t table_slots)
{
	c->n_rows = (uint32_t)n;

	// the first row of every distinct (chr, start), in file order
	std::vector<uint32_t> firsts;
	c->row_ra.resize(n + 1, 0);
	for (size_t i = 0; i < n; ++i) {
		c->row_ra[i] = (uint16_t)((uint8_t)ref[i] | (uint16_t)(uint8_t)alt[i] << 8);
		if (c->first_row.emplace(host_key(chr[i], strlen(chr[i]), start[i]), (uint32_t)i).second) firsts.push_back((uint32_t)i);
	}
	size_t slots = table_slots;
	if (slots == 0)
		for (slots = 16; slots < 2 * firsts.size(); slots <<= 1) {}
	if (slots < firsts.size() || slots < 1 || slots > ((size_t)1 << 31)) return VC_EINVAL;
	c->mask = (uint32_t)(slots - 1);
	std::vector<uint4> table(slots, make_uint4(0u, 0u, VCF_EMPTY, 0u));
	std::vector<uint8_t> names;
	std::unordered_map<std::string, uint32_t> name_off;
	for (uint32_t i : firsts) {
		const size_t len = strlen(chr[i]);
		auto it = name_off.find(chr[i]);
		if (it == name_off.end()) {
			it = name_off.emplace(chr[i], (uint32_t)names.size()).first;
			names.push_back((uint8_t)len);
			names.insert(names.end(), chr[i], chr[i] + len);
		}
		uint32_t h = VCF_FNV0;
		for (size_t k = 0; k < len; ++k) h = vcf_fnv_step(h, (uint8_t)chr[i][k]);
		uint32_t slot = vcf_slot(h, start[i], c->mask);
		while (table[slot].z != VCF_EMPTY) slot = (slot + 1) & c->mask;   // slots >= entries: a free one exists
		table[slot] = make_uint4(h, (uint32_t)start[i], i, it->second);
	}
	names.push_back(0);

	HIPCK(c->d_table.upload(table.data(), table.size()));
	HIPCK(c->d_names.upload(names.data(), names.size()));
	HIPCK(c->d_row_ra.upload(c->row_ra.data(), c->row_ra.size()));
	HIPCK(c->d_n_hits.alloc(1));
	HIPCK(c->d_n_hits.zero());
	HIPCK(c->d_consumed.alloc(1));
	HIPCK(c->d_consumed.zero());
	return VC_OK;
}

} // namespace

extern "C" int vc_vcf_create_raw(vc_vcf **out, const char *const *chr, const int32_t *start, const char *ref,
                                 const char *alt, size_t n, size_t table_slots, int device)
{
	if (!out || (n && (!chr || !start || !ref || !alt)) || n > 0x7FFFFFFFu) return VC_EINVAL;
	*out = nullptr;
	if (table_slots & (table_slots - 1)) return VC_EINVAL;
	for (size_t i = 0; i < n; ++i)
		if (!chr[i] || strlen(chr[i]) > VCF_MAX_CHR) return VC_EINVAL;
	vc_vcf *c = new (std::nothrow) vc_vcf;
	if (!c) return VC_ENOMEM;
	int rc = c->open(device);
	if (rc == VC_OK) rc = vcf_fill(c, chr, start, ref, alt, n, table_slots);
	if (rc != VC_OK) {
		vc_vcf_destroy(c);
		return rc;
	}
	*out = c;
	return VC_OK;
}

extern "C" int vc_vcf_create(vc_vcf **out, const vc_patterns *db, int device)
{
	if (!out || !db) return VC_EINVAL;
	*out = nullptr;
	const int n = vc_patterns_count(db);
	std::vector<const char *> chr((size_t)n);
	std::vector<int32_t> start((size_t)n);
	std::vector<char> ref((size_t)n), alt((size_t)n);
	for (int i = 0; i < n; ++i) {
		int s = 0;
		if (vc_pattern_fields(db, i, &chr[(size_t)i], &s, nullptr, &ref[(size_t)i], &alt[(size_t)i], nullptr, nullptr) != VC_OK)
			return VC_EINVAL;
		start[(size_t)i] = s;
	}
	return vc_vcf_create_raw(out, chr.data(), start.data(), ref.data(), alt.data(), (size_t)n, 0, device);
}

extern "C" void vc_vcf_destroy(vc_vcf *c)
{
	if (!c) return;
	(void)hipSetDevice(c->dev);
	if (c->pend.active && c->pend.st) (void)hipStreamSynchronize(c->pend.st);
	vc_bgzf_destroy(c->zf);
	c->close();
	delete c;
}

namespace {

// Before a new scan: the one still pending is collected, and a list that was
// handed out is dropped.
int begin_scan(vc_vcf *c)
{
	HIPCK(hipSetDevice(c->dev));
	const int rc = collect(c);
	if (rc != VC_OK) return rc;
	if (c->handed) {
		c->acc.clear();
		c->handed = false;
	}
	return VC_OK;
}

} // namespace

extern "C" int vc_vcf_scan_block(vc_vcf *c, const uint8_t *text, size_t len, uint64_t file_off, int final, size_t *consumed)
{
	if (!c || (len && !text)) return VC_EINVAL;
	size_t cons = len;
	if (!final) {
		cons = 0;
		for (size_t i = len; i > 0; --i)
			if (text[i - 1] == '\n') {
				cons = i;
				break;
			}
	}
	if (consumed) *consumed = cons;
	int rc = begin_scan(c);
	if (rc != VC_OK) return rc;
	c->last_consumed = cons;
	if (cons == 0) return VC_OK;
	VcSlot *s;
	rc = c->stage.acquire_for(cons, 1, &s);
	if (rc != VC_OK) return rc;
	memcpy(s->h_seq, text, cons);
	return c->stage.submit(cons, 1, c->st, [&](const VcSlot &sl) {
		// only the consumed bytes are shipped, so on the device this block is final
		c->pend.d_text = sl.d_seq;
		c->pend.len = cons;
		c->pend.file_off = file_off;
		c->pend.final_block = 1;
		c->pend.st = c->st;
		const int r = launch(c, c->pend);
		c->pend.active = r == VC_OK;
		return r;
	}, false);
}

extern "C" int vc_vcf_scan_device(vc_vcf *c, const uint8_t *d_text, size_t len, uint64_t file_off, int final, void *stream)
{
	if (!c || (len && !d_text)) return VC_EINVAL;
	int rc = begin_scan(c);
	if (rc != VC_OK) return rc;
	c->last_consumed = 0;
	if (len == 0) return VC_OK;
	return c->on_stream(stream, [&](hipStream_t st) {
		c->pend.d_text = d_text;
		c->pend.len = len;
		c->pend.file_off = file_off;
		c->pend.final_block = final ? 1 : 0;
		c->pend.st = st;
		const int r = launch(c, c->pend);
		c->pend.active = r == VC_OK;
		return r;
	});
}

extern "C" int vc_vcf_hits(vc_vcf *c, const vc_vcf_hit **hits, size_t *n_hits, size_t *consumed)
{
	if (!c) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	const int rc = collect(c);
	if (rc != VC_OK) return rc;
	if (c->handed) c->acc.clear();   // nothing was scanned since the last call
	std::sort(c->acc.begin(), c->acc.end(), [](const vc_vcf_hit &a, const vc_vcf_hit &b) { return a.off < b.off; });
	c->handed = true;
	if (hits) *hits = c->acc.data();
	if (n_hits) *n_hits = c->acc.size();
	if (consumed) *consumed = c->last_consumed;
	return VC_OK;
}

extern "C" int vc_vcf_set_max_hits(vc_vcf *c, size_t max_hits)
{
	if (!c || max_hits == 0 || max_hits > 0xFFFFFFFFu) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	const int rc = collect(c);
	if (rc != VC_OK) return rc;
	c->max_hits = max_hits;
	return VC_OK;
}

extern "C" int vc_vcf_set_block_bytes(vc_vcf *c, size_t bytes)
{
	if (!c || bytes == 0) return VC_EINVAL;
	c->block_bytes = bytes;
	return VC_OK;
}

extern "C" int vc_vcf_kernel_ms(vc_vcf *c, float *ms)
{
	return c ? c->timer.ms(ms) : VC_EINVAL;
}

namespace {

// The lines a scan reported, in file order, under items 2-8: `text` holds the
// scanned block from its byte `base` on, up to `consumed`; set(row, ref, alt)
// receives item 7's assignments.  VC_OK (ended: a line ended the file), an
// error of vc_vcf_eval_line, or VC_VCF_ABORTED.
template <class Set>
int eval_hits(vc_vcf *c, const vc_vcf_header *hdr, const uint8_t *text, size_t base, size_t consumed, uint64_t file_off,
              const vc_vcf_hit *hits, size_t n_hits, int sample_idx, int min_depth, bool &ended, Set &&set)
{
	int rc = VC_OK;
	const uint8_t *block = text - base;   // only bytes [base, consumed) of it are read
	for (size_t i = 0; i < n_hits && !ended; ++i) {
		const size_t lo = (size_t)(hits[i].off - file_off);
		const uint8_t *nl = (const uint8_t *)memchr(block + lo, '\n', consumed - lo);
		const size_t len = nl ? (size_t)(nl - block) - lo : consumed - lo;
		vc_vcf_verdict v;
		if ((rc = vc_vcf_eval_line(hdr, block + lo, len, sample_idx, min_depth, &v)) != VC_OK) break;
		int64_t row = hits[i].row;
		if (row < 0) {
			if (!v.head_ok) {   // item 8: the file ends here
				ended = true;
				break;
			}
			// a line after all: matched here (items 2 and 3)
			const auto it = c->first_row.find(host_key((const char *)block + lo, v.chrom_len, (int32_t)(uint32_t)(uint64_t)v.pos));
			if (it == c->first_row.end()) continue;
			if (v.n_allele != 2 || v.ref_len != 1 || v.alt_len != 1 ||
			    c->row_ra[it->second] != (uint16_t)(v.ref | (uint16_t)v.alt << 8))
				continue;
			row = it->second;
		}
		if (v.verdict == VC_VCF_ABORT) {   // item 8: the reference's process ends here
			rc = VC_VCF_ABORTED;
			break;
		}
		if (v.verdict == VC_VCF_END) ended = true;
		else if (v.verdict == VC_VCF_SET) set((size_t)row, v.ref_count, v.alt_count);
	}
	return rc;
}

// The pass with the text inflated (or read) on the host.
int count_host(vc_vcf *c, const char *path, int kind, int sample_idx, int min_depth, int n_threads, uint32_t *counts,
               vc_file_stats &st)
{
	VcVcfText in;
	if (in.open(path, kind, n_threads) != VC_OK) {
		fprintf(stderr, "Error: failed to open VCF file: %s\n", path);
		return VC_EIO;
	}
	// the header: text is read until the #CHROM line is whole
	std::vector<uint8_t> buf;
	vc_vcf_header *hdr = nullptr;
	size_t body = 0;
	bool eof = false;
	for (;;) {
		const size_t at = buf.size(), step = (size_t)1 << 16;
		buf.resize(at + step);
		const size_t got = in.read(buf.data() + at, step);
		buf.resize(at + got);
		eof = got < step;
		const int rc = vc_vcf_header_parse(buf.data(), buf.size(), eof, &hdr, &body);
		if (rc == VC_OK) break;
		if (rc != VC_VCF_MORE || eof) {
			fprintf(stderr, "Error: failed to read VCF header\n");
			return VC_EINVAL;
		}
	}
	// what is read and not yet consumed: text[head ..), at file offset file_off
	std::vector<uint8_t> text(buf.begin() + (ptrdiff_t)body, buf.end());
	buf.clear();
	buf.shrink_to_fit();
	size_t head = 0;
	uint64_t file_off = body;
	st.bases = body;

	int rc = VC_OK;
	bool ended = false;
	size_t cap = c->block_bytes;
	while (!ended) {
		// a block: up to cap bytes from a line start; one without a '\n' is a line
		// longer than the block, which grows
		if (head && (head >= text.size() / 2 || eof)) {
			text.erase(text.begin(), text.begin() + (ptrdiff_t)head);
			head = 0;
		}
		while (!eof && text.size() - head < cap) {
			const size_t at = text.size(), want = cap - (at - head);
			text.resize(at + want);
			const size_t got = in.read(text.data() + at, want);
			text.resize(at + got);
			eof = got < want;
		}
		size_t blen = text.size() - head;
		if (blen == 0) break;
		if (blen > cap) blen = cap;
		const bool final = eof && blen == text.size() - head;
		const uint8_t *block = text.data() + head;
		if (!final && !memchr(block, '\n', blen)) {
			cap *= 2;
			continue;
		}
		size_t consumed = 0;
		if ((rc = vc_vcf_scan_block(c, block, blen, file_off, final ? 1 : 0, &consumed)) != VC_OK) break;
		const vc_vcf_hit *hits = nullptr;
		size_t n_hits = 0;
		if ((rc = vc_vcf_hits(c, &hits, &n_hits, nullptr)) != VC_OK) break;
		++st.blocks;
		st.seqs += n_hits;
		rc = eval_hits(c, hdr, block, 0, consumed, file_off, hits, n_hits, sample_idx, min_depth, ended,
		               [&](size_t row, uint32_t ref, uint32_t alt) {
			               counts[2 * row] = ref;
			               counts[2 * row + 1] = alt;
		               });
		if (rc != VC_OK) break;
		st.bases += consumed;
		file_off += consumed;
		head += consumed;
	}
	vc_vcf_header_free(hdr);
	return rc;
}

// ---------------------------------------------------------------------------
// BGZF input inflated on the device.  The header's members are inflated here
// with zlib; from the member that holds the first data line on, pieces of
// whole members are read straight into the stager's pinned slots, copied to
// the device as they are and inflated there by the inflater's kernel
// (vafc_bgzf.hip) on the inflater's stream, into one of two text buffers, while
// the scan of the piece before runs on this handle's stream and its lines are
// evaluated here.  A piece's text lies behind `zhead` free bytes of its buffer;
// the unconsumed tail of the piece before is copied in front of it, so every
// scan starts at a line start and reads one contiguous range.  The lines the
// host evaluates reach it as one D2H copy of the scanned text from the first
// reported line on (none when the scan reports nothing).
//
// VCF_FALLBACK: the file cannot be finished this way (a member whose status
// is not 0, bytes that are no whole member before the end of the file, an
// ISIZE above 65,536).  Nothing has been written to counts or stderr then.
// ---------------------------------------------------------------------------
const int VCF_FALLBACK = 100;
const size_t VCF_ZHEAD = (size_t)1 << 20;         // room in front of a piece's text for the tail before it
const size_t VCF_PIECE_BLOCKS = 65536;            // members of one piece at most

// One member at the file position into dst (room for 65,536 bytes): 1 = read
// (*m describes it), 0 = clean end of file, -1 = cut, not BGZF, or ISIZE too large.
int read_member(FILE *fp, uint8_t *dst, VcBgzfMember *m)
{
	const size_t got = fread(dst, 1, VC_BGZF_HEAD, fp);
	if (got == 0) return 0;
	if (got != VC_BGZF_HEAD || !vc_bgzf_head_ok(dst)) return -1;
	const size_t xlen = vc_bgzf_xlen(dst);
	if (xlen && fread(dst + VC_BGZF_HEAD, 1, xlen, fp) != xlen) return -1;
	const size_t size = vc_bgzf_member_size(dst + VC_BGZF_HEAD, xlen);
	if (size == 0) return -1;
	const size_t rest = size - VC_BGZF_HEAD - xlen;
	if (fread(dst + VC_BGZF_HEAD + xlen, 1, rest, fp) != rest) return -1;
	if (vc_bgzf_member_at(dst, size, m) != 1 || m->isize > VC_BGZF_MAX_TEXT) return -1;
	return 1;
}

// zlib over one whole member, as the host reader checks it.
bool inflate_member_host(const uint8_t *mem, const VcBgzfMember &m, std::vector<uint8_t> &text)
{
	const size_t at = text.size();
	text.resize(at + m.isize + 1);
	z_stream zs;
	memset(&zs, 0, sizeof zs);
	if (inflateInit2(&zs, -15) != Z_OK) return false;
	zs.next_in = const_cast<uint8_t *>(mem + m.payload);
	zs.avail_in = (uInt)m.payload_len;
	zs.next_out = text.data() + at;
	zs.avail_out = m.isize + 1;
	const int rc = inflate(&zs, Z_FINISH);
	const bool ok = rc == Z_STREAM_END && zs.total_out == m.isize;
	inflateEnd(&zs);
	text.resize(at + m.isize);
	return ok && (uint32_t)crc32(crc32(0L, Z_NULL, 0), text.data() + at, m.isize) == m.crc32;
}

struct ZPiece {
	size_t n_blocks = 0;
	uint64_t text_len = 0;
	bool last = false;        // the file ended behind it
	int buf = 0;              // its text buffer
};

struct ZSet {
	uint32_t row, ref, alt;
};

int count_bgzf_device(vc_vcf *c, const char *path, int sample_idx, int min_depth, uint32_t *counts, vc_file_stats &st)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) return VCF_FALLBACK;   // the host pass reports it
	struct Closer {
		FILE *fp;
		vc_vcf_header *hdr = nullptr;
		hipEvent_t ev = nullptr;
		~Closer()
		{
			if (fp) fclose(fp);
			vc_vcf_header_free(hdr);
			if (ev) (void)hipEventDestroy(ev);
		}
	} own{fp};
	HIPCK(hipSetDevice(c->dev));
	if (!c->zf) {
		const int rc = vc_bgzf_create(&c->zf, c->dev);
		if (rc != VC_OK) return rc;
	}
	vc_bgzf *zf = c->zf;
	const hipStream_t zst = (hipStream_t)vc_bgzf_stream(zf);
	HIPCK(hipEventCreateWithFlags(&own.ev, hipEventDisableTiming));
	uint64_t host_blocks = 0, device_blocks = 0;

	// the header: members are inflated here until the #CHROM line is whole
	std::vector<uint8_t> buf, mem(65536 + 16);
	std::vector<uint64_t> toff(1, 0);   // text offset of each header member
	std::vector<long> foff;             // ... and its file offset
	size_t body = 0;
	for (;;) {
		const long at = ftell(fp);
		VcBgzfMember m;
		const int r = read_member(fp, mem.data(), &m);
		if (r < 0) return VCF_FALLBACK;
		const bool eof = r == 0;
		if (!eof) {
			if (!inflate_member_host(mem.data(), m, buf)) return VCF_FALLBACK;
			foff.push_back(at);
			toff.push_back(buf.size());
			++host_blocks;
		}
		const int rc = vc_vcf_header_parse(buf.data(), buf.size(), eof, &own.hdr, &body);
		if (rc == VC_OK) break;
		// (the host pass says why: it sees the same text)
		if (rc != VC_VCF_MORE || eof) return VCF_FALLBACK;
	}
	// the member that holds the first data line; the device starts over with it
	size_t mb = 0;
	while (mb + 1 < toff.size() && toff[mb + 1] <= body) ++mb;
	const size_t skip = body - (size_t)toff[mb];   // bytes of its text in front of the first data line
	if (mb < foff.size() && fseek(fp, foff[mb], SEEK_SET) != 0) return VCF_FALLBACK;
	buf.clear();
	buf.shrink_to_fit();

	std::vector<ZSet> sets;   // item 7's assignments, applied once the file is known to be whole
	std::vector<uint8_t> lines;
	size_t cap = c->block_bytes;
	ZPiece piece[2];
	bool file_ended = false;

	// Read the next piece into the stager's slot and send it on its way: H2D and
	// inflate on the inflater's stream, into text buffer b behind its head room.
	auto start_piece = [&](ZPiece &p, int b) -> int {
		p = ZPiece();
		p.buf = b;
		if (file_ended) {
			p.last = true;
			return VC_OK;
		}
		const size_t raw_room = cap + 65536, max_blocks = std::min(VCF_PIECE_BLOCKS, raw_room / 28 + 1);
		const size_t desc_at = (raw_room + 7) & ~(size_t)7;
		VcSlot *s;
		int rc = c->stage.acquire_for(desc_at + max_blocks * sizeof(vc_bgzf_block), 1, &s);
		if (rc != VC_OK) return rc;
		vc_bgzf_block *desc = reinterpret_cast<vc_bgzf_block *>(s->h_seq + desc_at);
		size_t raw_len = 0;
		while (p.text_len < cap && raw_len + 65536 <= raw_room && p.n_blocks < max_blocks) {
			VcBgzfMember m;
			const int r = read_member(fp, s->h_seq + raw_len, &m);
			if (r < 0) return VCF_FALLBACK;
			if (r == 0) {
				file_ended = p.last = true;
				break;
			}
			vc_bgzf_block &d = desc[p.n_blocks++];
			d.in_off = raw_len + m.payload;
			d.in_len = (uint32_t)m.payload_len;
			d.isize = m.isize;
			d.out_off = p.text_len;
			d.crc32 = m.crc32;
			d.reserved = 0;
			p.text_len += m.isize;
			raw_len += m.size;
		}
		if (p.n_blocks == 0) return VC_OK;
		// the text buffer: nobody reads it any more but the copy of its tail, which `ev` follows
		if (c->zhead[b] < VCF_ZHEAD) c->zhead[b] = VCF_ZHEAD;
		if (c->ztext[b].cap < c->zhead[b] + p.text_len) HIPCK(c->ztext[b].grow(c->zhead[b] + (size_t)p.text_len + 65536));
		HIPCK(hipStreamWaitEvent(zst, own.ev, 0));
		uint8_t *d_text = c->ztext[b] + c->zhead[b];
		const size_t nb = p.n_blocks;
		const uint64_t tl = p.text_len;
		// the descriptors travel with the compressed bytes: one copy of [0, desc_at + n * 32)
		return c->stage.submit(desc_at + nb * sizeof(vc_bgzf_block), 1, zst, [&](const VcSlot &sl) {
			return vc_bgzf_inflate_device(zf, sl.d_seq, raw_len, reinterpret_cast<const vc_bgzf_block *>(sl.d_seq + desc_at), nb,
			                              d_text, (size_t)tl, VC_STREAM_CTX);
		}, false);
	};
	// Whatever is in flight has ended before the buffers are left alone.
	auto drain = [&]() {
		(void)vc_bgzf_finish(zf, nullptr, 0, nullptr, nullptr);
		(void)hipStreamSynchronize(c->st);
		c->stage.settle();
	};

	HIPCK(hipEventRecord(own.ev, c->st));
	int rc = start_piece(piece[0], 0);
	if (rc != VC_OK) return drain(), rc;
	uint64_t file_off = body;
	st.bases = body;
	size_t tail_len = 0, tail_at = 0;   // the unconsumed text of the piece before: ztext[tail_buf][tail_at, +tail_len)
	int tail_buf = 0;
	size_t first_skip = skip;
	bool ended = false;
	for (int k = 0; !ended; ++k) {
		ZPiece &p = piece[k & 1];
		const int b = p.buf;
		if (p.n_blocks) {
			size_t n = 0, ok = 0;
			if ((rc = vc_bgzf_finish(zf, nullptr, 0, &n, &ok)) != VC_OK) break;
			if (ok != p.n_blocks) {
				rc = VCF_FALLBACK;
				break;
			}
			device_blocks += p.n_blocks;
		} else if (!p.last) {
			rc = VC_EINVAL;   // (a piece without members is the end of the file)
			break;
		}
		if (first_skip > p.text_len) {   // cannot be: the header's member is the piece's first
			rc = VCF_FALLBACK;
			break;
		}
		// the text to scan: the tail before, then this piece (the very first one from the first data line on)
		size_t text_at = c->zhead[b] + first_skip, text_len = (size_t)p.text_len - first_skip;
		first_skip = 0;
		if (p.n_blocks == 0) {
			// nothing new: what is left of the piece before is the file's last line
			if (tail_len == 0) break;
			text_at = tail_at;
			text_len = tail_len;
			p.buf = tail_buf;
		} else if (tail_len) {
			if (tail_len > c->zhead[b]) {
				// a tail longer than the room in front of the text: a buffer with more room takes both
				size_t room = c->zhead[b];
				while (room < tail_len) room *= 2;
				VcDevBuf<uint8_t> nb;
				HIPCK(nb.alloc(room + (size_t)p.text_len + 65536));
				HIPCK(hipMemcpyAsync(nb + room, c->ztext[b] + c->zhead[b], (size_t)p.text_len, hipMemcpyDeviceToDevice, c->st));
				HIPCK(hipStreamSynchronize(c->st));
				c->ztext[b] = std::move(nb);
				c->zhead[b] = room;
				text_at = room;
			}
			HIPCK(hipMemcpyAsync(c->ztext[b] + text_at - tail_len, c->ztext[tail_buf] + tail_at, tail_len, hipMemcpyDeviceToDevice,
			                     c->st));
			text_at -= tail_len;
			text_len += tail_len;
		}
		HIPCK(hipEventRecord(own.ev, c->st));   // the other buffer's tail has left it
		const int sb = p.buf;
		const bool final = p.last;
		// the text is scanned as the host pass scans it: in blocks of up to cap bytes from a line start (a block
		// without a '\n' grows), a block shorter than cap only at the end of the file
		size_t pos = 0;
		bool next_started = false;
		while (!ended && pos < text_len) {
			size_t blen = text_len - pos;
			if (blen < cap && !final) break;   // the rest waits for the next piece
			if (blen > cap) blen = cap;
			const bool final_block = final && pos + blen == text_len;
			const uint8_t *d_text = c->ztext[sb] + text_at + pos;
			if ((rc = vc_vcf_scan_device(c, d_text, blen, file_off, final_block ? 1 : 0, VC_STREAM_CTX)) != VC_OK) break;
			// the next piece is read, copied and inflated while this one is scanned and evaluated
			if (!next_started && (rc = start_piece(piece[(k + 1) & 1], sb ^ 1)) != VC_OK) break;
			next_started = true;
			const vc_vcf_hit *hits = nullptr;
			size_t n_hits = 0, consumed = 0;
			if ((rc = vc_vcf_hits(c, &hits, &n_hits, &consumed)) != VC_OK) break;
			if (consumed == 0 && !final_block) {   // no '\n': a line longer than the block
				cap *= 2;
				continue;
			}
			++st.blocks;
			st.seqs += n_hits;
			if (n_hits) {
				const size_t lo = (size_t)(hits[0].off - file_off);
				lines.resize(consumed - lo);
				HIPCK(hipMemcpy(lines.data(), d_text + lo, consumed - lo, hipMemcpyDeviceToHost));
				rc = eval_hits(c, own.hdr, lines.data(), lo, consumed, file_off, hits, n_hits, sample_idx, min_depth, ended,
				               [&](size_t row, uint32_t ref, uint32_t alt) { sets.push_back(ZSet{(uint32_t)row, ref, alt}); });
				if (rc != VC_OK) break;
			}
			st.bases += consumed;
			file_off += consumed;
			pos += consumed;
		}
		if (rc != VC_OK || ended || final) break;
		if (!next_started && (rc = start_piece(piece[(k + 1) & 1], sb ^ 1)) != VC_OK) break;
		tail_buf = sb;
		tail_at = text_at + pos;
		tail_len = text_len - pos;
	}
	drain();
	if (rc == VCF_FALLBACK || (rc != VC_OK && rc != VC_VCF_ABORTED)) return rc;
	for (const ZSet &z : sets) {
		counts[2 * (size_t)z.row] = z.ref;
		counts[2 * (size_t)z.row + 1] = z.alt;
	}
	c->z_device_blocks = device_blocks;
	c->z_host_blocks = host_blocks;
	return rc;
}

// Whole BGZF members of a file, by their headers alone.
uint64_t count_members(const char *path)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) return 0;
	uint64_t n = 0;
	uint8_t h[VC_BGZF_HEAD + 65536];
	for (;;) {
		if (fread(h, 1, VC_BGZF_HEAD, fp) != VC_BGZF_HEAD || !vc_bgzf_head_ok(h)) break;
		const size_t xlen = vc_bgzf_xlen(h);
		if (xlen && fread(h + VC_BGZF_HEAD, 1, xlen, fp) != xlen) break;
		const size_t size = vc_bgzf_member_size(h + VC_BGZF_HEAD, xlen);
		if (size == 0 || fseek(fp, (long)(size - VC_BGZF_HEAD - xlen), SEEK_CUR) != 0) break;
		++n;
	}
	fclose(fp);
	return n;
}

} // namespace

extern "C" int vc_vcf_inflate_info(const vc_vcf *c, uint64_t *device_blocks, uint64_t *host_blocks)
{
	if (!c) return VC_EINVAL;
	if (device_blocks) *device_blocks = c->z_device_blocks;
	if (host_blocks) *host_blocks = c->z_host_blocks;
	return VC_OK;
}

extern "C" int vc_vcf_count_file(vc_vcf *c, const char *path, int sample_idx, int min_depth, int n_threads, uint32_t *counts,
                                 vc_file_stats *stats)
{
	if (!c || !path || (c->n_rows && !counts)) return VC_EINVAL;
	const double t0 = vc_now();
	vc_file_stats st;
	memset(&st, 0, sizeof st);
	if (stats) *stats = st;
	c->z_device_blocks = c->z_host_blocks = 0;
	int kind = VC_VCF_OTHER;
	if (vc_vcf_probe(path, &kind) != VC_OK) {
		fprintf(stderr, "Error: failed to open VCF file: %s\n", path);
		return VC_EIO;
	}
	if (kind == VC_VCF_BCF) {
		fprintf(stderr, "Error: %s is %s; only VCF text (plain, gzip or BGZF) is read\n", path, vc_vcf_kind_name(kind));
		return VC_EINVAL;
	}
	int rc = VCF_FALLBACK;
	if (kind == VC_VCF_BGZF) {
		// $VAFC_BGZF = host | device; unset: VCF_BGZF_DEFAULT_DEVICE
		const char *e = getenv("VAFC_BGZF");
		const bool device = e && *e ? strcmp(e, "device") == 0 : VCF_BGZF_DEFAULT_DEVICE;
		if (device) rc = count_bgzf_device(c, path, sample_idx, min_depth, counts, st);
		if (rc == VCF_FALLBACK) {
			memset(&st, 0, sizeof st);
			c->z_host_blocks = count_members(path);
		}
	}
	if (rc == VCF_FALLBACK) rc = count_host(c, path, kind, sample_idx, min_depth, n_threads, counts, st);
	st.seconds = vc_now() - t0;
	if (stats) *stats = st;
	return rc;
}
