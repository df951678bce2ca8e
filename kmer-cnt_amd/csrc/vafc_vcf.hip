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
// The handle (vafc_vcf_ctx.h) is created and scanned with here; the file
// passes that feed the scans are vafc_vcf_files.cpp.
//
// Every global read is bounded: text by the bytes the tail kernel allows
// (<= len; an aligned 16-byte load is issued only if it holds one of them, so
// it stays inside that byte's page), table entries by the slot mask, names by
// their stored length, the hit list by its capacity (overflow is counted, not
// written).  Nothing here decides on the CPU what the kernel should have: a
// HIP failure is returned as VC_EHIP.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <new>

#include "vafc_vcf_ctx.h"

namespace {

const int VCF_BLOCK = 256;
const int VCF_WAVES = VCF_BLOCK / 64;
const uint32_t VCF_WAVE_BYTES = 64 * 16;
typedef uint32_t vcf_u32x4 __attribute__((ext_vector_type(4)));   // 16 bytes in registers (a uint4 held across a branch goes through the stack)
const uint32_t VCF_HALO = 256;   // bytes of the next tile staged with a tile: most first-five-column reads end inside
static_assert(VCF_BLOCK * 16 == VC_VCF_TILE_BYTES, "a tile is one 16-byte load per lane");
const uint32_t VCF_EMPTY = 0xFFFFFFFFu;
const uint32_t VCF_MAX_CHR = 255;

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

int launch(vc_vcf *c, const VcVcfPending &p)
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
		if (c->first_row.emplace(vcf_host_key(chr[i], strlen(chr[i]), start[i]), (uint32_t)i).second) firsts.push_back((uint32_t)i);
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

// Launch the scan of len device bytes on st; it is the pending one.
int start_scan(vc_vcf *c, const uint8_t *d_text, size_t len, uint64_t file_off, int final, hipStream_t st)
{
	c->pend = VcVcfPending{d_text, len, file_off, final ? 1 : 0, st, false};
	const int r = launch(c, c->pend);
	c->pend.active = r == VC_OK;
	return r;
}

} // namespace

extern "C" int vc_vcf_scan_block(vc_vcf *c, const uint8_t *text, size_t len, uint64_t file_off, int final, size_t *consumed)
{
	if (!c || (len && !text)) return VC_EINVAL;
	size_t cons = len;
	if (!final) {   // up to the last '\n'
		const uint8_t *nl = len ? (const uint8_t *)memrchr(text, '\n', len) : nullptr;
		cons = nl ? (size_t)(nl - text) + 1 : 0;
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
	// only the consumed bytes are shipped, so on the device this block is final
	return c->stage.submit(cons, 1, c->st, [&](const VcSlot &sl) { return start_scan(c, sl.d_seq, cons, file_off, 1, c->st); }, false);
}

extern "C" int vc_vcf_scan_device(vc_vcf *c, const uint8_t *d_text, size_t len, uint64_t file_off, int final, void *stream)
{
	if (!c || (len && !d_text)) return VC_EINVAL;
	int rc = begin_scan(c);
	if (rc != VC_OK) return rc;
	c->last_consumed = 0;
	if (len == 0) return VC_OK;
	return c->on_stream(stream, [&](hipStream_t st) { return start_scan(c, d_text, len, file_off, final, st); });
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
