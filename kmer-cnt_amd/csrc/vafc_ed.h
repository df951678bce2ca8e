// vafc_ed.h -- kernel argument block and launcher of the approximate pattern
// search (ed-vaf-counter), shared by the host side (vafc_ed.cpp) and the
// kernels (vafc_ed.hip).  Not part of the public C ABI (include/vafc.h).
#ifndef VAFC_ED_H
#define VAFC_ED_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define VC_ED_CHUNK 4096       // read bytes a block stages in LDS at a time (a multiple of 4)
#define VC_ED_SEGS 64          // reads (or pieces of one long read) per chunk: one per lane of the staging wave
#define VC_ED_MAX_WAVES 4      // query groups (of 64 queries) per block
#define VC_ED_LDS_MASKS 32768  // match masks of a block are kept in LDS up to this many bytes, else read from HBM

// The three word widths: queries of 1..32, 33..64 and 65..127 bytes.
enum { VC_ED_W32 = 0, VC_ED_W64 = 1, VC_ED_W128 = 2, VC_ED_WIDTHS = 3 };
static inline int vc_ed_width_words(int width) { return width == VC_ED_W128 ? 2 : 1; }
static inline int vc_ed_width_wordbytes(int width) { return width == VC_ED_W32 ? 4 : 8; }

struct VcEdArgs {
	const uint8_t *seq;          // read bytes
	uint64_t seq_bytes;          // bounds every read of seq
	const uint64_t *offs;
	const uint32_t *lens;
	uint64_t n_reads;
	uint64_t reads_per_range;    // blockIdx.y * reads_per_range = the block's first read
	const uint8_t *cls;          // [256] byte -> symbol class
	const void *masks;           // [group][class][word][64 lanes] match masks (bit i: query byte i is of the class)
	const uint32_t *qlen;        // [group * 64 + lane] query length, 0 = no query in this lane
	const uint32_t *qout;        // [group * 64 + lane] index into counts
	uint32_t n_groups;
	uint32_t n_class;
	int max_edit;                // -e as given (negative: the query's length)
	uint32_t *counts;
	uint32_t *flags;             // bit 0: a read reached past seq_bytes
};

// ---------------------------------------------------------------------------
// The recurrence: Myers 1999 ("A fast bit-vector algorithm for approximate
// string matching based on dynamic programming"), the search form in which
// row 0 of the table is 0 everywhere, over NW words of type W.  Bit i of the
// vectors is row i + 1 of the current column: pv / mv hold the vertical
// differences +1 / -1, `score` is the last row D[m][j].  Before the first
// column the table is D[i][-1] = i: every vertical difference is +1.
// ---------------------------------------------------------------------------
#if defined(__HIPCC__)
#define VC_ED_HD __host__ __device__ __forceinline__
#else
#define VC_ED_HD inline
#endif

template <typename W, int NW> struct VcEdState {
	W pv[NW], mv[NW];
	uint32_t score;   // D[m][j] of the last column consumed
	uint32_t best;    // minimum of the scores of this read so far
	uint32_t cnt;     // columns at which it occurred
};

template <typename W, int NW> VC_ED_HD void vc_ed_begin(VcEdState<W, NW> &s, uint32_t m)
{
	for (int w = 0; w < NW; ++w) {
		s.pv[w] = ~(W)0;
		s.mv[w] = 0;
	}
	s.score = m;
	s.best = 0xFFFFFFFFu;
	s.cnt = 0;
}

// One column.  eq: the match mask of the column's symbol; hb: the bit of row
// m in the last word.  HBHI: hb >= 32 is known (one 64-bit word, m >= 33), so
// the score bit comes out of the high dword with a 32-bit shift.
template <typename W, int NW, bool HBHI> VC_ED_HD void vc_ed_step(VcEdState<W, NW> &s, const W (&eq)[NW], uint32_t hb)
{
	constexpr int B = (int)sizeof(W) * 8;
	W cadd = 0, cph = 0, cmh = 0;
#pragma unroll
	for (int w = 0; w < NW; ++w) {
		const W e = eq[w], pv = s.pv[w], mv = s.mv[w];
		const W xv = e | mv;
		const W t = e & pv;
		W sum = t + pv;
		W carry = sum < t ? 1 : 0;
		if (w > 0) {
			const W sum2 = sum + cadd;
			carry |= sum2 < sum ? 1 : 0;
			sum = sum2;
		}
		cadd = carry;
		const W xh = (sum ^ pv) | e;
		W ph = mv | ~(xh | pv);
		W mh = pv & xh;
		if (w == NW - 1) {
			uint32_t up, down;
			if (HBHI) {
				up = ((uint32_t)((uint64_t)ph >> 32) >> (hb - 32)) & 1u;
				down = ((uint32_t)((uint64_t)mh >> 32) >> (hb - 32)) & 1u;
			} else {
				up = (uint32_t)(ph >> hb) & 1u;
				down = (uint32_t)(mh >> hb) & 1u;
			}
			s.score += up;
			s.score -= down;
		}
		const W pho = ph >> (B - 1), mho = mh >> (B - 1);
		ph = (ph << 1) | cph;
		mh = (mh << 1) | cmh;
		cph = pho;
		cmh = mho;
		s.pv[w] = mh | ~(xv | ph);
		s.mv[w] = ph & xv;
	}
	const bool lt = s.score < s.best;
	s.cnt = lt ? 1u : s.cnt + (s.score == s.best ? 1u : 0u);
	s.best = lt ? s.score : s.best;
}

// The hit count of one read of n bytes (include/vafc.h, vc_ed_create): the
// candidates are the n last-row scores, plus one of value m when the bound is
// the query's length and n < pad = 64 * ceil(m / 64) - m; the count is how
// often the minimum occurs if it is within the bound kp = min(e', m).  A read
// of no bytes counts 1.
template <typename W, int NW>
VC_ED_HD uint32_t vc_ed_end(const VcEdState<W, NW> &s, uint32_t n, uint32_t m, uint32_t kp, uint32_t pad)
{
	if (n == 0) return 1;
	uint32_t c = s.cnt;
	if (kp == m && n < pad && s.best == m) ++c;   // scores never exceed m
	return s.best <= kp ? c : 0;
}

#ifdef __cplusplus
extern "C" {
#endif
// grid.x = ceil(n_groups / waves) blocks of 64 * waves threads, grid.y read
// ranges; lds_masks: the block's masks fit VC_ED_LDS_MASKS.
hipError_t vc_ed_launch(const VcEdArgs *A, int width, int waves, int lds_masks, unsigned grid_x, unsigned grid_y,
                        hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
