// vafc_bam.hip -- bam-vaf-counter on the device (vc_bam_* of include/vafc.h):
// the reference's worker_check_positions / count_base_at_position
// (bam-vaf-counter.c:238-318), which tests every pattern row against every
// record, as a search in the rows sorted by (tid, pos).
//
//   rows          (tid, pos) keys ascending, beside each the row's index in
//                 the pattern file and its ref / alt bytes; small enough to
//                 stay in L2
//   short kernel  one lane per record: lower bound of (tid, pos), then one
//                 merged walk of the CIGAR and the rows, both ascending in
//                 reference position
//   long kernel   records of more CIGAR ops than the threshold are listed by
//                 the short kernel and get a wave each: 64 ops at a time, a
//                 wave-wide scan of the reference and query advances gives
//                 every lane its op's interval, and each M/=/X lane searches
//                 the rows inside its own
//   weights       item 6 of the contract: the number of merged regions a
//                 record overlaps, from two sorted key arrays
//
// Every global read is bounded: rows and regions by their counts, descriptors
// by n_recs, and a record's CIGAR and bases by data_bytes before the first of
// them is read (a descriptor that fails sets flags bit 0 and is not followed).
// CIGAR words are read as aligned dwords (offsets are multiples of 4), bases
// as bytes.
//
//   text          vc_bam_scan_text_*: records found and checked in inflated BAM
//                 text on the device (vafc_bam_text.h: guess, link, emit, check,
//                 four launches on one stream) and counted where they lie by a
//                 second instantiation of the two kernels, whose CIGAR loads are
//                 byte loads: a record starts at any offset of the text
//
// vc_bam_count_file and its device pass over BGZF members: vafc_bam_files.cpp.
//
// Nothing here counts on the CPU: any HIP failure is returned as VC_EHIP.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "vafc.h"
#include "vafc_bam.h"
#include "vafc_bam_ctx.h"
#include "vafc_bam_text.h"
#include "vafc_stage.h"

namespace {

struct VcBamArgs {
	const vc_bam_rec *recs;
	uint64_t n_recs;
	const uint32_t *n_found;     // text scans: the number of records is on the device (NULL: n_recs)
	const uint8_t *data;
	uint64_t data_bytes;
	const uint64_t *row_key;     // [n_rows] bam_key(tid, pos), ascending
	const uint2 *row_info;       // [n_rows] x: row index in the pattern file, y: ref | alt << 8
	uint32_t n_rows;
	const uint64_t *reg_s;       // [n_reg] keys of the region starts, ascending
	const uint64_t *reg_e;       // [n_reg] keys of the region ends, ascending
	uint32_t n_reg;              // 0: every weight is 1
	uint32_t long_thr;
	uint32_t *long_list;         // [n_recs] records left to the long kernel
	uint32_t *long_n;
	uint32_t *counts;
	uint32_t *flags;             // bit 0: a descriptor points outside data
};

const uint32_t BAM_SKIP_FLAGS = 0x4u | 0x200u | 0x400u;
const int BAM_BLOCK = 256;
const int64_t BAM_POS_END = (int64_t)1 << 31;   // one past the largest row position

// (tid, x) as one sortable word, tid >= 0 and x in [-2^31, 2^31].
__host__ __device__ inline uint64_t bam_key(int32_t tid, int64_t x)
{
	return ((uint64_t)(uint32_t)tid << 33) + (uint64_t)(x + BAM_POS_END);
}

__device__ inline int64_t bam_key_pos(uint64_t key) { return (int64_t)(key & (((uint64_t)1 << 33) - 1)) - BAM_POS_END; }

// First i with a[i] >= key.
__device__ inline uint32_t bam_lower(const uint64_t *a, uint32_t n, uint64_t key)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (a[mid] < key) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

__device__ inline bool bam_ref_op(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
__device__ inline bool bam_query_op(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
__device__ inline bool bam_match_op(uint32_t op) { return op == 0 || op == 7 || op == 8; }

// The record's CIGAR and bases lie inside data, on a 4-byte boundary unless
// the record lies in text (ALIGNED false).
template <bool ALIGNED> __device__ inline bool bam_in_bounds(const vc_bam_rec &r, uint64_t data_bytes)
{
	const uint64_t need = 4 * (uint64_t)r.n_cigar + (((uint64_t)r.l_seq + 1) >> 1);
	return (!ALIGNED || (r.off & 3) == 0) && r.off <= data_bytes && need <= data_bytes - r.off;
}

// CIGAR word k of the words at cig: one dword, or four bytes at any alignment.
template <bool ALIGNED> __device__ inline uint32_t bam_cig(const uint8_t *cig, uint32_t k)
{
	if (ALIGNED) return reinterpret_cast<const uint32_t *>(cig)[k];
	const uint8_t *p = cig + 4 * (size_t)k;
	return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// Item 6: merged regions [s, e) of this tid with s < end and e > pos.
__device__ inline uint32_t bam_weight(const VcBamArgs &A, int32_t tid, int64_t pos, int64_t end)
{
	if (A.n_reg == 0) return 1;
	const uint32_t starts_below = bam_lower(A.reg_s, A.n_reg, bam_key(tid, end));
	const uint32_t ends_upto = bam_lower(A.reg_e, A.n_reg, bam_key(tid, pos) + 1);
	return starts_below - ends_upto;
}

// Row j against base qi of the record: ref first, else alt.
__device__ inline void bam_hit(const VcBamArgs &A, uint32_t j, const uint8_t *seq, uint64_t qi, uint32_t l_seq, uint32_t w)
{
	if (qi >= l_seq) return;
	const uint32_t b = seq[qi >> 1];
	const uint32_t nib = (qi & 1) ? (b & 15u) : (b >> 4);
	const uint32_t base = (uint32_t)(uint8_t) "=ACMGRSVTWYHKDBN"[nib];
	const uint2 info = A.row_info[j];
	const uint32_t ref = info.y & 255u, alt = (info.y >> 8) & 255u;
	if (base == ref) atomicAdd(&A.counts[2 * (size_t)info.x], w);
	else if (base == alt) atomicAdd(&A.counts[2 * (size_t)info.x + 1], w);
}

template <bool ALIGNED> __device__ inline void bam_short_body(const VcBamArgs &A)
{
	const uint64_t i = (uint64_t)blockIdx.x * BAM_BLOCK + threadIdx.x;
	if (i >= A.n_recs || (A.n_found && i >= *A.n_found)) return;
	const vc_bam_rec r = A.recs[i];
	if (!bam_in_bounds<ALIGNED>(r, A.data_bytes)) {
		atomicOr(A.flags, 1u);
		return;
	}
	if ((r.flag & BAM_SKIP_FLAGS) || r.tid < 0 || r.n_cigar == 0) return;
	if (r.n_cigar > A.long_thr) {
		A.long_list[atomicAdd(A.long_n, 1u)] = (uint32_t)i;
		return;
	}
	const uint64_t tid_end = bam_key(r.tid, BAM_POS_END);
	uint32_t j = bam_lower(A.row_key, A.n_rows, bam_key(r.tid, r.pos));
	if (j >= A.n_rows || A.row_key[j] > tid_end) return;   // most records: no row at or after them
	const uint8_t *cig = A.data + r.off;
	const uint8_t *seq = A.data + r.off + 4 * (size_t)r.n_cigar;
	int64_t rlen = 0;
	for (uint32_t k = 0; k < r.n_cigar; ++k) {
		const uint32_t c = bam_cig<ALIGNED>(cig, k);
		if (bam_ref_op(c & 15u)) rlen += c >> 4;
	}
	int64_t end = (int64_t)r.pos + (rlen ? rlen : 1);
	if (end > BAM_POS_END) end = BAM_POS_END;
	const uint64_t end_key = bam_key(r.tid, end);
	if (A.row_key[j] >= end_key) return;
	const uint32_t w = bam_weight(A, r.tid, r.pos, end);
	if (w == 0) return;
	// the merged walk: op k covers [cur, cur + L) when it consumes the reference
	uint32_t k = 0;
	int64_t cur = r.pos;
	uint64_t rp = 0;
	for (; j < A.n_rows; ++j) {
		const uint64_t key = A.row_key[j];
		if (key >= end_key) break;
		const int64_t p = bam_key_pos(key);
		uint32_t op = 0, len = 0;
		for (; k < r.n_cigar; ++k) {
			const uint32_t c = bam_cig<ALIGNED>(cig, k);
			op = c & 15u;
			len = c >> 4;
			if (bam_ref_op(op)) {
				if (p < cur + (int64_t)len) break;
				cur += len;
			}
			if (bam_query_op(op)) rp += len;
		}
		if (k >= r.n_cigar) break;   // no op left covers this row or a later one
		if (bam_match_op(op)) bam_hit(A, j, seq, rp + (uint64_t)(p - cur), r.l_seq, w);
	}
}

__global__ void __launch_bounds__(BAM_BLOCK) bam_short_kernel(VcBamArgs A) { bam_short_body<true>(A); }
__global__ void __launch_bounds__(BAM_BLOCK) bam_short_text_kernel(VcBamArgs A) { bam_short_body<false>(A); }

// Inclusive scan over the wave's 64 lanes.
__device__ inline uint64_t bam_wave_scan(uint64_t v, int lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t u = __shfl_up((unsigned long long)v, d, 64);
		if (lane >= d) v += u;
	}
	return v;
}

template <bool ALIGNED> __device__ inline void bam_long_body(const VcBamArgs &A)
{
	const int lane = threadIdx.x & 63;
	const uint32_t waves = gridDim.x * (BAM_BLOCK / 64);
	const uint32_t n_long = *A.long_n;
	for (uint32_t e = blockIdx.x * (BAM_BLOCK / 64) + (threadIdx.x >> 6); e < n_long; e += waves) {
		const vc_bam_rec r = A.recs[A.long_list[e]];   // listed by the short kernel: in bounds, not skipped
		const uint8_t *cig = A.data + r.off;
		const uint8_t *seq = A.data + r.off + 4 * (size_t)r.n_cigar;
		uint32_t w = 1;
		if (A.n_reg) {
			uint64_t rl = 0;
			for (uint32_t k = (uint32_t)lane; k < r.n_cigar; k += 64) {
				const uint32_t c = bam_cig<ALIGNED>(cig, k);
				if (bam_ref_op(c & 15u)) rl += c >> 4;
			}
#pragma unroll
			for (int d = 32; d > 0; d >>= 1) rl += __shfl_xor((unsigned long long)rl, d, 64);
			int64_t end = (int64_t)r.pos + (rl ? (int64_t)rl : 1);
			if (end > BAM_POS_END) end = BAM_POS_END;
			w = bam_weight(A, r.tid, r.pos, end);
			if (w == 0) continue;   // the same in every lane
		}
		int64_t base_cur = r.pos;
		uint64_t base_rp = 0;
		for (uint32_t g = 0; g < r.n_cigar; g += 64) {
			const uint32_t k = g + (uint32_t)lane;
			const uint32_t c = k < r.n_cigar ? bam_cig<ALIGNED>(cig, k) : 0xFu;   // past the end: a reserved op, it does nothing
			const uint32_t op = c & 15u, len = c >> 4;
			const uint64_t radv = bam_ref_op(op) ? len : 0, qadv = bam_query_op(op) ? len : 0;
			const uint64_t rsum = bam_wave_scan(radv, lane), qsum = bam_wave_scan(qadv, lane);
			const int64_t cur = base_cur + (int64_t)(rsum - radv);
			const uint64_t rp = base_rp + (qsum - qadv);
			if (bam_match_op(op) && len > 0 && cur < BAM_POS_END) {
				int64_t hi = cur + (int64_t)len;
				if (hi > BAM_POS_END) hi = BAM_POS_END;
				const uint64_t hi_key = bam_key(r.tid, hi);
				for (uint32_t j = bam_lower(A.row_key, A.n_rows, bam_key(r.tid, cur)); j < A.n_rows; ++j) {
					const uint64_t key = A.row_key[j];
					if (key >= hi_key) break;
					bam_hit(A, j, seq, rp + (uint64_t)(bam_key_pos(key) - cur), r.l_seq, w);
				}
			}
			base_cur += (int64_t)__shfl((unsigned long long)rsum, 63, 64);
			base_rp += __shfl((unsigned long long)qsum, 63, 64);
		}
	}
}

__global__ void __launch_bounds__(BAM_BLOCK) bam_long_kernel(VcBamArgs A) { bam_long_body<true>(A); }
__global__ void __launch_bounds__(BAM_BLOCK) bam_long_text_kernel(VcBamArgs A) { bam_long_body<false>(A); }

// ---------------------------------------------------------------------------
// Records in text (vafc_bam_text.h has the method and its bounds)
// ---------------------------------------------------------------------------

struct VcBamTextArgs {
	const uint8_t *text;
	uint64_t len;
	const uint64_t *cuts;   // [n_cuts], ascending
	uint32_t n_cuts;
	int32_t n_ref;
	uint64_t entry;         // the piece's first record
	uint32_t final;
	uint32_t max_recs;      // room in offs and recs
	VbtSeg *segs;           // [n_cuts + 1]
	uint32_t *offs;         // [max_recs] record offsets, in no order
	vc_bam_rec *recs;       // [max_recs] descriptor of offs[i]
	VbtResult *res;
};

// One lane per segment: its guess and the walk from there.
__global__ void __launch_bounds__(BAM_BLOCK) bam_text_guess_kernel(VcBamTextArgs T)
{
	const uint64_t s = (uint64_t)blockIdx.x * BAM_BLOCK + threadIdx.x;
	if (s > T.n_cuts) return;
	uint64_t a, b;
	vbt_seg_range(T.cuts, T.n_cuts, T.len, (uint32_t)s, &a, &b);
	VbtSeg sg;
	sg.entry = vbt_guess(T.text, T.len, a, b, T.n_ref);
	sg.exit = 0;
	sg.count = sg.stop = 0;
	if (sg.entry != VBT_NONE) vbt_walk(T.text, T.len, sg.entry, b, &sg, nullptr, 0);
	T.segs[s] = sg;
}

// One wave, the segments in order, 64 at a time: each lane loads one segment,
// and every lane takes the same steps on the values of segment j, so a segment
// that is walked again is walked by the whole wave on the same addresses.
__global__ void __launch_bounds__(64) bam_text_link_kernel(VcBamTextArgs T)
{
	const int lane = threadIdx.x;
	const uint32_t n_seg = T.n_cuts + 1;
	uint64_t e = T.entry;
	uint32_t stop = VBT_STOP_NONE, rewalked = 0;
	for (uint32_t base = 0; base < n_seg; base += 64) {
		const uint32_t s = base + (uint32_t)lane;
		VbtSeg mine;
		mine.entry = VBT_NONE;
		mine.exit = 0;
		mine.count = mine.stop = 0;
		uint64_t a = 0, b = 0;
		if (s < n_seg) {
			mine = T.segs[s];
			vbt_seg_range(T.cuts, T.n_cuts, T.len, s, &a, &b);
		}
		const int m = n_seg - base < 64 ? (int)(n_seg - base) : 64;
		for (int j = 0; j < m; ++j) {
			VbtSeg sg;
			sg.entry = __shfl((unsigned long long)mine.entry, j, 64);
			sg.exit = __shfl((unsigned long long)mine.exit, j, 64);
			sg.count = __shfl(mine.count, j, 64);
			sg.stop = __shfl(mine.stop, j, 64);
			const uint64_t ja = __shfl((unsigned long long)a, j, 64), jb = __shfl((unsigned long long)b, j, 64);
			vbt_link_step(T.text, T.len, ja, jb, &sg, &e, &stop, &rewalked);
			if (lane == j) mine = sg;
		}
		if (s < n_seg) T.segs[s] = mine;
	}
	if (lane == 0) vbt_link_end(T.text, T.len, e, stop, T.final != 0, rewalked, T.res);
}

// One lane per segment: the offsets of its records, from its true entry, into
// slots reserved with one atomic.
__global__ void __launch_bounds__(BAM_BLOCK) bam_text_emit_kernel(VcBamTextArgs T)
{
	const uint64_t s = (uint64_t)blockIdx.x * BAM_BLOCK + threadIdx.x;
	if (s > T.n_cuts) return;
	const VbtSeg sg = T.segs[s];
	if (sg.entry == VBT_NONE || sg.count == 0) return;
	uint64_t a, b;
	vbt_seg_range(T.cuts, T.n_cuts, T.len, (uint32_t)s, &a, &b);
	const uint32_t at = atomicAdd(&T.res->n_found, sg.count);
	if ((uint64_t)at + sg.count > T.max_recs) return;   // cannot be: the records are disjoint and 36 bytes or more each
	VbtSeg again;
	vbt_walk(T.text, T.len, sg.entry, b, &again, T.offs + at, sg.count);
}

// One lane per record found: its descriptor, or the skipped one of an
// irregular record; the totals per wave.
__global__ void __launch_bounds__(BAM_BLOCK) bam_text_check_kernel(VcBamTextArgs T)
{
	const uint64_t i = (uint64_t)blockIdx.x * BAM_BLOCK + threadIdx.x;
	const uint32_t n = T.res->n_found < T.max_recs ? T.res->n_found : T.max_recs;
	unsigned long long regular = 0, bases = 0;
	if (i < n) {
		const uint64_t o = T.offs[i];
		vc_bam_rec r;
		if (vbt_check(T.text, o, &r)) {
			regular = 1;
			bases = r.l_seq;
		} else {
			vbt_skip_rec(&r);
			atomicAdd(&T.res->irr_n, 1u);
			atomicMin((unsigned long long *)&T.res->irr_off, (unsigned long long)o);
		}
		T.recs[i] = r;
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		regular += __shfl_xor(regular, d, 64);
		bases += __shfl_xor(bases, d, 64);
	}
	if ((threadIdx.x & 63) == 0 && regular) {
		atomicAdd((unsigned long long *)&T.res->records, regular);
		atomicAdd((unsigned long long *)&T.res->bases, bases);
	}
}

struct VcBamPieceArgs {
	const uint8_t *text;
	uint64_t len;
	const vc_bam_piece *pieces;   // [n_pieces]
	uint32_t n_pieces;
	uint32_t max_recs;            // room in offs
	vc_bam_piece_status *out;     // [n_pieces]
	uint32_t *offs;
	VbtResult *res;
};

const int BAM_PIECE_BLOCK = 64;

// n slots of the record list, never past its room: true and *at, the first.
__device__ inline bool bam_reserve(uint32_t *n_found, uint32_t n, uint32_t room, uint32_t *at)
{
	uint32_t seen = atomicAdd(n_found, 0u);
	for (;;) {
		if ((uint64_t)seen + n > room) return false;
		const uint32_t was = atomicCAS(n_found, seen, seen + n);
		if (was == seen) break;
		seen = was;
	}
	*at = seen;
	return true;
}

// One lane per piece, one wave per block: the walk of vbt_piece_walk to count,
// slots for the pieces that ended OK, and the same walk again into them.  The
// wave sums its lanes' counts and lane 0 reserves for all of them with one
// atomic (never past max_recs, so every slot below n_found is written); only
// a wave whose sum finds no room (the caller's pieces overlap) lets each lane
// try for itself.  A wave's lanes take as many trips as its longest piece; a
// wave per piece would leave 63 lanes idle on a chain that only one lane can
// follow.
__global__ void __launch_bounds__(BAM_PIECE_BLOCK) bam_piece_walk_kernel(VcBamPieceArgs P)
{
	const int lane = threadIdx.x;
	const uint64_t i = (uint64_t)blockIdx.x * BAM_PIECE_BLOCK + threadIdx.x;
	const bool live = i < P.n_pieces;
	vc_bam_piece p = {0, 0, 0};
	vc_bam_piece_status s;
	s.status = VC_BAM_PIECE_OK;
	s.found = s.first = s.reserved = 0;
	s.missing = 0;
	if (live) {
		p = P.pieces[i];
		s.status = vbt_piece_walk(P.text, P.len, p, &s.found, &s.missing, nullptr, 0);
	}
	const uint32_t want = s.status == VC_BAM_PIECE_OK ? s.found : 0;
	const uint64_t upto = bam_wave_scan(want, lane);
	const uint64_t total = __shfl((unsigned long long)upto, 63, 64);
	uint32_t base = 0;
	int fits = 0;
	if (lane == 0 && total && total <= P.max_recs) fits = bam_reserve(&P.res->n_found, (uint32_t)total, P.max_recs, &base) ? 1 : 0;
	fits = __shfl(fits, 0, 64);
	base = __shfl(base, 0, 64);
	if (want) {
		uint32_t at = base + (uint32_t)(upto - want);
		if (!fits && !bam_reserve(&P.res->n_found, want, P.max_recs, &at)) s.status = VC_BAM_PIECE_NOROOM;
		if (s.status == VC_BAM_PIECE_OK) {
			uint32_t again;
			uint64_t none;
			s.first = at;
			(void)vbt_piece_walk(P.text, P.len, p, &again, &none, P.offs + at, s.found);
		}
	}
	if (s.status == VC_BAM_PIECE_SHORT) atomicAdd(&P.res->n_short, 1u);
	else if (s.status == VC_BAM_PIECE_CUT) atomicAdd(&P.res->n_cut, 1u);
	else if (s.status == VC_BAM_PIECE_NOROOM) atomicAdd(&P.res->n_noroom, 1u);
	if (live) P.out[i] = s;
}

} // namespace

namespace {

// n_found: the device's count of the descriptors (a text scan: n_recs is their
// room, and the records lie at any alignment).
int launch(vc_bam *c, const vc_bam_rec *d_recs, uint64_t n_recs, const uint8_t *d_data, size_t data_bytes, hipStream_t st,
           const uint32_t *n_found = nullptr)
{
	if (n_recs == 0) return VC_OK;
	if (n_recs > 0xFFFFFFFFull || ((uintptr_t)d_recs & 7) || (!n_found && ((uintptr_t)d_data & 3))) return VC_EINVAL;
	if (n_recs > c->d_long_list.cap) HIPCK(c->d_long_list.grow(n_recs + n_recs / 4 + 1024));
	VcBamArgs A;
	A.recs = d_recs;
	A.n_recs = n_recs;
	A.n_found = n_found;
	A.data = d_data;
	A.data_bytes = data_bytes;
	A.row_key = c->d_row_key;
	A.row_info = c->d_row_info;
	A.n_rows = c->n_rows;
	A.reg_s = c->d_reg_s;
	A.reg_e = c->d_reg_e;
	A.n_reg = c->n_reg;
	A.long_thr = c->long_thr;
	A.long_list = c->d_long_list;
	A.long_n = c->d_long_n;
	A.counts = c->d_counts;
	A.flags = c->d_flags;
	HIPCK(c->d_long_n.zero_async(st));
	HIPCK(c->timer.begin(st));
	const unsigned grid = (unsigned)((n_recs + BAM_BLOCK - 1) / BAM_BLOCK);
	hipLaunchKernelGGL(n_found ? bam_short_text_kernel : bam_short_kernel, dim3(grid), dim3(BAM_BLOCK), 0, st, A);
	HIPCK(hipGetLastError());
	// the list's length is known on the device only: a fixed grid of waves walks it
	uint64_t lgrid = (uint64_t)c->n_cu * 2;
	if (lgrid > (n_recs + 3) / 4) lgrid = (n_recs + 3) / 4;
	hipLaunchKernelGGL(n_found ? bam_long_text_kernel : bam_long_kernel, dim3((unsigned)lgrid), dim3(BAM_BLOCK), 0, st, A);
	HIPCK(hipGetLastError());
	HIPCK(c->timer.end(st));
	return VC_OK;
}

// The rows and regions of an open handle, on the host and on the device.
int bam_fill(vc_bam *c, const vc_patterns *db, const char *const *ref_names, int n_refs)
{
	const int n = (int)c->n_pat;
	// create_snp_map (bam-vaf-counter.c:187-215): tids and the two warnings, in row order
	std::unordered_map<std::string, int32_t> tid_of;
	for (int i = 0; i < n_refs; ++i) tid_of.emplace(ref_names[i], i);
	struct Row {
		uint64_t key;
		uint2 info;
	};
	std::vector<Row> rows;
	std::unordered_set<uint64_t> seen;
	for (int i = 0; i < n; ++i) {
		const char *chr = nullptr;
		int start = 0;
		char ref = 0, alt = 0;
		if (vc_pattern_fields(db, i, &chr, &start, nullptr, &ref, &alt, nullptr, nullptr) != VC_OK) return VC_EINVAL;
		const auto it = tid_of.find(chr);
		if (it == tid_of.end()) {
			fprintf(stderr, "Warning: chromosome %s not found in BAM header\n", chr);
			continue;
		}
		if (!seen.insert(((uint64_t)(uint32_t)it->second << 32) | (uint32_t)start).second)
			fprintf(stderr, "Warning: duplicate SNP at %s:%d\n", chr, start);
		Row r;
		r.key = bam_key(it->second, start);
		r.info.x = (uint32_t)i;
		r.info.y = (uint32_t)(uint8_t)ref | (uint32_t)(uint8_t)alt << 8;
		rows.push_back(r);
	}
	std::stable_sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.key < b.key; });
	c->n_rows = (uint32_t)rows.size();
	std::vector<uint64_t> keys(rows.size() + 1, 0);
	std::vector<uint2> info(rows.size() + 1);
	for (size_t i = 0; i < rows.size(); ++i) {
		keys[i] = rows[i].key;
		info[i] = rows[i].info;
	}

	// build_regions (:124-175), kept by name: their tids depend on each file's header
	if (n > 0) {
		std::vector<int32_t> first((size_t)n), ends((size_t)n);
		const int nr = vc_bam_build_regions(db, first.data(), ends.data());
		for (int i = 0; i < nr; ++i) {
			const char *chr = nullptr;
			int start = 0;
			(void)vc_pattern_fields(db, first[(size_t)i], &chr, &start, nullptr, nullptr, nullptr, nullptr, nullptr);
			c->reg_chr.emplace_back(chr);
			c->reg_start.push_back(start);
			c->reg_end.push_back(ends[(size_t)i]);
		}
	}

	HIPCK(c->d_row_key.upload(keys.data(), keys.size()));
	HIPCK(c->d_row_info.upload(info.data(), info.size()));
	HIPCK(c->d_counts.alloc(2 * (size_t)n + 2));
	HIPCK(c->d_counts.zero());
	HIPCK(c->d_flags.alloc(1));
	HIPCK(c->d_flags.zero());
	HIPCK(c->d_long_n.alloc(1));
	HIPCK(c->d_long_n.zero());
	HIPCK(c->d_tres.alloc(1));
	HIPCK(c->d_tres.zero());
	HIPCK(c->text_timer.init());
	HIPCK(c->check_timer.init());
	c->n_ref = n_refs;
	return VC_OK;
}

// The four launches of a text scan and the two count kernels behind them, on
// st; d_cuts is read by them, so it stays until st has passed them.
int scan_text(vc_bam *c, const uint8_t *d_text, size_t text_bytes, uint64_t entry, const uint64_t *d_cuts, size_t n_cuts,
              int final, hipStream_t st)
{
	if (text_bytes > 0xFFFFFFF0ull || n_cuts > 0x7FFFFFFFull || entry > text_bytes) return VC_EINVAL;
	const size_t n_seg = n_cuts + 1, max_recs = text_bytes / VBT_FIXED + 1;
	if (n_seg > c->d_segs.cap) HIPCK(c->d_segs.grow(n_seg + n_seg / 4 + 64));
	if (max_recs > c->d_offs.cap) HIPCK(c->d_offs.grow(max_recs + max_recs / 4 + 1024, c->d_trecs, max_recs + max_recs / 4 + 1024));
	VcBamTextArgs T;
	T.text = d_text;
	T.len = text_bytes;
	T.cuts = d_cuts;
	T.n_cuts = (uint32_t)n_cuts;
	T.n_ref = c->n_ref;
	T.entry = entry;
	T.final = final ? 1u : 0u;
	T.max_recs = (uint32_t)max_recs;
	T.segs = c->d_segs;
	T.offs = c->d_offs;
	T.recs = c->d_trecs;
	T.res = c->d_tres;
	HIPCK(c->d_tres.zero_async(st));
	HIPCK(c->text_timer.begin(st));
	const unsigned sgrid = (unsigned)((n_seg + BAM_BLOCK - 1) / BAM_BLOCK), rgrid = (unsigned)((max_recs + BAM_BLOCK - 1) / BAM_BLOCK);
	hipLaunchKernelGGL(bam_text_guess_kernel, dim3(sgrid), dim3(BAM_BLOCK), 0, st, T);
	HIPCK(hipGetLastError());
	hipLaunchKernelGGL(bam_text_link_kernel, dim3(1), dim3(64), 0, st, T);
	HIPCK(hipGetLastError());
	hipLaunchKernelGGL(bam_text_emit_kernel, dim3(sgrid), dim3(BAM_BLOCK), 0, st, T);
	HIPCK(hipGetLastError());
	HIPCK(c->text_timer.end(st));
	HIPCK(c->check_timer.begin(st));
	hipLaunchKernelGGL(bam_text_check_kernel, dim3(rgrid), dim3(BAM_BLOCK), 0, st, T);
	HIPCK(hipGetLastError());
	HIPCK(c->check_timer.end(st));
	return launch(c, c->d_trecs, max_recs, d_text, text_bytes, st, &c->d_tres.p->n_found);
}

// The piece walk, the check of what it emitted and the two count kernels
// behind them, on st; d_pieces is read by the walk, so it stays until st has
// passed it.
int scan_pieces(vc_bam *c, const uint8_t *d_text, size_t text_bytes, const vc_bam_piece *d_pieces, size_t n_pieces, hipStream_t st)
{
	if (text_bytes > 0xFFFFFFF0ull || n_pieces > 0x7FFFFFFFull) return VC_EINVAL;
	const size_t max_recs = text_bytes / VBT_FIXED + 1;
	if (n_pieces > c->d_pstat.cap) HIPCK(c->d_pstat.grow(n_pieces + n_pieces / 4 + 64));
	if (max_recs > c->d_offs.cap) HIPCK(c->d_offs.grow(max_recs + max_recs / 4 + 1024, c->d_trecs, max_recs + max_recs / 4 + 1024));
	c->n_pieces_last = n_pieces;
	HIPCK(c->d_tres.zero_async(st));
	HIPCK(hipMemsetAsync(&c->d_tres.p->irr_off, 0xFF, sizeof(uint64_t), st));   // VBT_NONE
	if (n_pieces == 0) {
		c->text_timer.clear();
		c->check_timer.clear();
		return VC_OK;
	}
	VcBamPieceArgs P;
	P.text = d_text;
	P.len = text_bytes;
	P.pieces = d_pieces;
	P.n_pieces = (uint32_t)n_pieces;
	P.max_recs = (uint32_t)max_recs;
	P.out = c->d_pstat;
	P.offs = c->d_offs;
	P.res = c->d_tres;
	VcBamTextArgs T;
	memset(&T, 0, sizeof T);
	T.text = d_text;
	T.len = text_bytes;
	T.n_ref = c->n_ref;
	T.max_recs = (uint32_t)max_recs;
	T.offs = c->d_offs;
	T.recs = c->d_trecs;
	T.res = c->d_tres;
	HIPCK(c->text_timer.begin(st));
	const unsigned pgrid = (unsigned)((n_pieces + BAM_PIECE_BLOCK - 1) / BAM_PIECE_BLOCK);
	hipLaunchKernelGGL(bam_piece_walk_kernel, dim3(pgrid), dim3(BAM_PIECE_BLOCK), 0, st, P);
	HIPCK(hipGetLastError());
	HIPCK(c->text_timer.end(st));
	HIPCK(c->check_timer.begin(st));
	const unsigned rgrid = (unsigned)((max_recs + BAM_BLOCK - 1) / BAM_BLOCK);
	hipLaunchKernelGGL(bam_text_check_kernel, dim3(rgrid), dim3(BAM_BLOCK), 0, st, T);
	HIPCK(hipGetLastError());
	HIPCK(c->check_timer.end(st));
	return launch(c, c->d_trecs, max_recs, d_text, text_bytes, st, &c->d_tres.p->n_found);
}

} // namespace

extern "C" int vc_bam_create(vc_bam **out, const vc_patterns *db, const char *const *ref_names, int n_refs, int device)
{
	if (!out || !db || n_refs < 0 || (n_refs && !ref_names)) return VC_EINVAL;
	*out = nullptr;
	const int n = vc_patterns_count(db);
	if (n > (0x7FFFFFFF >> 1)) return VC_ETOOMANY;
	vc_bam *c = new (std::nothrow) vc_bam;
	if (!c) return VC_ENOMEM;
	c->n_pat = (uint32_t)n;
	int rc = c->open(device);
	if (rc == VC_OK) rc = bam_fill(c, db, ref_names, n_refs);
	if (rc != VC_OK) {
		vc_bam_destroy(c);
		return rc;
	}
	*out = c;
	return VC_OK;
}

extern "C" void vc_bam_destroy(vc_bam *c)
{
	if (!c) return;
	c->close();
	c->text_timer.destroy();
	c->check_timer.destroy();
	vc_bgzf_destroy(c->zf);
	delete c;
}

extern "C" int vc_bam_set_regions(vc_bam *c, const int32_t *tid, const int32_t *start, const int32_t *end, size_t n)
{
	if (!c || (n && (!tid || !start || !end)) || n > 0x7FFFFFFFu) return VC_EINVAL;
	std::vector<uint64_t> s(n), e(n);
	for (size_t i = 0; i < n; ++i) {
		if (tid[i] < 0 || start[i] >= end[i]) return VC_EINVAL;
		s[i] = bam_key(tid[i], start[i]);
		e[i] = bam_key(tid[i], end[i]);
	}
	// each array in its own order: the weight is (starts below end) - (ends up to pos)
	std::sort(s.begin(), s.end());
	std::sort(e.begin(), e.end());
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));   // earlier batches read the arrays about to change
	if (n > c->d_reg_s.cap) HIPCK(c->d_reg_s.grow(n, c->d_reg_e, n));
	if (n) {
		HIPCK(hipMemcpy(c->d_reg_s, s.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
		HIPCK(hipMemcpy(c->d_reg_e, e.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
	}
	c->n_reg = (uint32_t)n;
	return VC_OK;
}

extern "C" int vc_bam_count_block(vc_bam *c, const vc_bam_rec *recs, uint64_t n_recs, const uint8_t *data, size_t data_bytes)
{
	if (!c || (n_recs && !recs) || (data_bytes && !data)) return VC_EINVAL;
	if (n_recs == 0) return VC_OK;
	if (n_recs > 0xFFFFFFFFull) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	const size_t rec_bytes = (size_t)n_recs * sizeof(vc_bam_rec), total = rec_bytes + data_bytes;
	VcSlot *s;
	const int rc = c->stage.acquire_for(total, 1, &s);
	if (rc != VC_OK) return rc;
	// descriptors first, the data behind them: both keep their alignment
	memcpy(s->h_seq, recs, rec_bytes);
	if (data_bytes) memcpy(s->h_seq + rec_bytes, data, data_bytes);
	return c->stage.submit(total, n_recs, c->st, [&](const VcSlot &sl) {
		return launch(c, reinterpret_cast<const vc_bam_rec *>(sl.d_seq), n_recs, sl.d_seq + rec_bytes, data_bytes, c->st);
	}, false);
}

extern "C" int vc_bam_count_device(vc_bam *c, const vc_bam_rec *d_recs, uint64_t n_recs, const uint8_t *d_data,
                                   size_t data_bytes, void *stream)
{
	if (!c || (n_recs && !d_recs) || (data_bytes && !d_data)) return VC_EINVAL;
	if (n_recs == 0) return VC_OK;
	HIPCK(hipSetDevice(c->dev));
	return c->on_stream(stream, [&](hipStream_t st) { return launch(c, d_recs, n_recs, d_data, data_bytes, st); });
}

extern "C" int vc_bam_finish(vc_bam *c, uint32_t *counts)
{
	if (!c) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	c->stage.settle();
	uint32_t f = 0;
	HIPCK(hipMemcpy(&f, c->d_flags, sizeof f, hipMemcpyDeviceToHost));
	if (f & 1u) {
		fprintf(stderr, "[E::vafc] a record descriptor points outside the data buffer: counts incomplete\n");
		return VC_EINVAL;
	}
	if (counts && c->n_pat)
		HIPCK(hipMemcpy(counts, c->d_counts, 2 * (size_t)c->n_pat * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return VC_OK;
}

extern "C" int vc_bam_reset(vc_bam *c)
{
	if (!c) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(c->d_counts.zero_async(c->st));
	HIPCK(c->d_flags.zero_async(c->st));
	return VC_OK;
}

extern "C" int vc_bam_set_counts(vc_bam *c, const uint32_t *counts)
{
	if (!c || (c->n_pat && !counts)) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	if (c->n_pat) {
		// pageable source: the copy has left the caller's buffer on return
		HIPCK(hipMemcpyAsync(c->d_counts, counts, 2 * (size_t)c->n_pat * sizeof(uint32_t), hipMemcpyHostToDevice, c->st));
		HIPCK(hipStreamSynchronize(c->st));
	}
	return VC_OK;
}

extern "C" int vc_bam_set_long_threshold(vc_bam *c, uint32_t ops)
{
	if (!c) return VC_EINVAL;
	c->long_thr = ops;
	return VC_OK;
}

extern "C" int vc_bam_kernel_ms(vc_bam *c, float *ms)
{
	return c ? c->timer.ms(ms) : VC_EINVAL;
}

extern "C" int vc_bam_scan_text_device(vc_bam *c, const uint8_t *d_text, size_t text_bytes, uint64_t entry,
                                       const uint64_t *d_cuts, size_t n_cuts, int final, void *stream)
{
	if (!c || (text_bytes && !d_text) || (n_cuts && !d_cuts) || ((uintptr_t)d_cuts & 7)) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	return c->on_stream(stream, [&](hipStream_t st) { return scan_text(c, d_text, text_bytes, entry, d_cuts, n_cuts, final, st); });
}

extern "C" int vc_bam_scan_text_block(vc_bam *c, const uint8_t *text, size_t text_bytes, uint64_t entry, const uint64_t *cuts,
                                      size_t n_cuts, int final)
{
	if (!c || (text_bytes && !text) || (n_cuts && !cuts)) return VC_EINVAL;
	for (size_t i = 0; i < n_cuts; ++i)
		if (cuts[i] > text_bytes || (i && cuts[i] < cuts[i - 1])) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	// the text first, the cuts behind it on an 8-byte boundary
	const size_t cuts_at = (text_bytes + 7) & ~(size_t)7, total = cuts_at + n_cuts * sizeof(uint64_t) + 8;
	VcSlot *s;
	const int rc = c->stage.acquire_for(total, 1, &s);
	if (rc != VC_OK) return rc;
	if (text_bytes) memcpy(s->h_seq, text, text_bytes);
	if (n_cuts) memcpy(s->h_seq + cuts_at, cuts, n_cuts * sizeof(uint64_t));
	return c->stage.submit(total, 1, c->st, [&](const VcSlot &sl) {
		return scan_text(c, sl.d_seq, text_bytes, entry, reinterpret_cast<const uint64_t *>(sl.d_seq + cuts_at), n_cuts, final, c->st);
	}, false);
}

int vc_bam_scan_text_cuts(vc_bam *c, const uint8_t *d_text, size_t text_bytes, uint64_t entry, const uint64_t *cuts,
                          size_t n_cuts, int final)
{
	if (n_cuts > c->d_cuts.cap) HIPCK(c->d_cuts.grow(n_cuts + n_cuts / 4 + 64));
	// pageable source: the copy has left the caller's buffer on return
	if (n_cuts) HIPCK(hipMemcpyAsync(c->d_cuts, cuts, n_cuts * sizeof(uint64_t), hipMemcpyHostToDevice, c->st));
	return scan_text(c, d_text, text_bytes, entry, c->d_cuts, n_cuts, final, c->st);
}

extern "C" int vc_bam_scan_pieces_device(vc_bam *c, const uint8_t *d_text, size_t text_bytes, const vc_bam_piece *d_pieces,
                                         size_t n_pieces, void *stream)
{
	if (!c || (text_bytes && !d_text) || (n_pieces && !d_pieces) || ((uintptr_t)d_pieces & 7)) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	return c->on_stream(stream, [&](hipStream_t st) { return scan_pieces(c, d_text, text_bytes, d_pieces, n_pieces, st); });
}

extern "C" int vc_bam_scan_pieces_block(vc_bam *c, const uint8_t *text, size_t text_bytes, const vc_bam_piece *pieces,
                                        size_t n_pieces)
{
	if (!c || (text_bytes && !text) || (n_pieces && !pieces) || n_pieces > 0x7FFFFFFFull) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	// the text first, the pieces behind it on an 8-byte boundary
	const size_t at = (text_bytes + 7) & ~(size_t)7, total = at + n_pieces * sizeof(vc_bam_piece) + 8;
	VcSlot *s;
	const int rc = c->stage.acquire_for(total, 1, &s);
	if (rc != VC_OK) return rc;
	if (text_bytes) memcpy(s->h_seq, text, text_bytes);
	if (n_pieces) memcpy(s->h_seq + at, pieces, n_pieces * sizeof(vc_bam_piece));
	return c->stage.submit(total, 1, c->st, [&](const VcSlot &sl) {
		return scan_pieces(c, sl.d_seq, text_bytes, reinterpret_cast<const vc_bam_piece *>(sl.d_seq + at), n_pieces, c->st);
	}, false);
}

int vc_bam_scan_pieces_host(vc_bam *c, const uint8_t *d_text, size_t text_bytes, const vc_bam_piece *pieces, size_t n_pieces)
{
	if (n_pieces > c->d_pieces.cap) HIPCK(c->d_pieces.grow(n_pieces + n_pieces / 4 + 64));
	// pageable source: the copy has left the caller's buffer on return
	if (n_pieces) HIPCK(hipMemcpyAsync(c->d_pieces, pieces, n_pieces * sizeof(vc_bam_piece), hipMemcpyHostToDevice, c->st));
	return scan_pieces(c, d_text, text_bytes, c->d_pieces, n_pieces, c->st);
}

extern "C" int vc_bam_pieces_result(vc_bam *c, vc_bam_pieces_res *res, vc_bam_piece_status *status, size_t n_status,
                                    uint32_t *offs, size_t n_offs)
{
	if (!c || !res || (n_status && !status) || (n_offs && !offs)) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	VbtResult r;
	HIPCK(hipMemcpy(&r, c->d_tres, sizeof r, hipMemcpyDeviceToHost));
	res->records = r.records;
	res->bases = r.bases;
	res->irregular_off = r.irr_off;
	res->found = r.n_found;
	res->irregular = r.irr_n;
	res->n_short = r.n_short;
	res->n_cut = r.n_cut;
	res->n_noroom = r.n_noroom;
	res->n_pieces = (uint32_t)c->n_pieces_last;
	const size_t ns = std::min(n_status, c->n_pieces_last), no = std::min<size_t>(n_offs, r.n_found);
	if (ns) HIPCK(hipMemcpy(status, c->d_pstat, ns * sizeof(vc_bam_piece_status), hipMemcpyDeviceToHost));
	if (no) HIPCK(hipMemcpy(offs, c->d_offs, no * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return VC_OK;
}

extern "C" int vc_bam_text_result(vc_bam *c, vc_bam_text_res *res)
{
	if (!c || !res) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	VbtResult r;
	HIPCK(hipMemcpy(&r, c->d_tres, sizeof r, hipMemcpyDeviceToHost));
	res->consumed = r.consumed;
	res->records = r.records;
	res->bases = r.bases;
	res->irregular_off = r.irr_off;
	res->irregular = r.irr_n;
	res->rewalked = r.rewalked;
	res->short_stop = r.short_stop;
	res->found = r.n_found;
	return VC_OK;
}

extern "C" int vc_bam_text_kernel_ms(vc_bam *c, float *find_ms, float *check_ms)
{
	if (!c) return VC_EINVAL;
	float f = 0, k = 0;
	int rc = c->text_timer.ms(&f);
	if (rc == VC_OK) rc = c->check_timer.ms(&k);
	if (rc != VC_OK) return rc;
	if (find_ms) *find_ms = f;
	if (check_ms) *check_ms = k;
	return VC_OK;
}

