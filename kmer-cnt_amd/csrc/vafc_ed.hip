// vafc_ed.hip -- approximate pattern search on gfx950: every query of a panel
// against every read of a batch, with Myers' bit-vector recurrence
// (vafc_ed.h).  Replaces search_kmer_in_seq / count_fastq_kmers of the
// reference (ed-vaf-counter.c:95-154), which runs edlib once per (read, query).
//
// Layout.  One lane owns one query: a wave holds a group of 64 queries (ref
// and alt of 32 patterns, interleaved), a block 1..4 groups.  blockIdx.y picks
// a contiguous range of the batch's reads.  The block streams that range
// through LDS in chunks of VC_ED_CHUNK bytes: wave 0 lays out up to 64 reads
// per chunk (an exclusive scan of their lengths, each read starting on a
// dword), all waves copy the bytes in, translated to symbol classes, and then
// every wave walks the same chunk.  A column's class is read from LDS four at
// a time into a scalar, so the walk has no divergence, and the lane's match
// mask for the class comes from an LDS table [class][word][lane] (or from the
// same table in HBM when a block's masks exceed VC_ED_LDS_MASKS).  A read
// longer than a chunk keeps its state in registers from one chunk to the next.
// Each lane adds its reads' hit counts in a register and issues one atomicAdd
// per block.
#include <hip/hip_runtime.h>

#include "vafc_ed.h"

namespace {

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

template <typename W, int NW, bool LDSM, bool HBHI>
__global__ __launch_bounds__(64 * VC_ED_MAX_WAVES) void vc_ed_kernel(const VcEdArgs A)
{
	__shared__ uint32_t s_codes[VC_ED_CHUNK / 4];
	__shared__ uint64_t s_src[VC_ED_SEGS];    // offset in seq of the segment's first byte
	__shared__ uint32_t s_beg[VC_ED_SEGS];    // the segment's bytes in s_codes: [beg, end)
	__shared__ uint32_t s_end[VC_ED_SEGS];
	__shared__ uint32_t s_len[VC_ED_SEGS];    // length of the read the segment belongs to
	__shared__ uint32_t s_flag[VC_ED_SEGS];   // bit 0: the read starts here, bit 1: it ends here
	__shared__ uint32_t s_hdr[2];             // segments of the chunk; 1 = a piece of a read longer than a chunk
	__shared__ uint8_t s_cls[256];
	extern __shared__ __align__(16) uint8_t s_dyn[];
	W *s_mask = reinterpret_cast<W *>(s_dyn);   // [class][word][wave][lane]

	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nw = blockDim.x >> 6;
	const uint32_t nthr = blockDim.x;
	const uint32_t group = blockIdx.x * nw + wave;
	const bool active = group < A.n_groups;     // wave-uniform
	const W *gmask = reinterpret_cast<const W *>(A.masks);

	for (uint32_t i = tid; i < 256; i += nthr) s_cls[i] = A.cls[i];
	// the walk reads whole dwords of classes: the bytes between two reads must
	// hold valid classes (they index the mask table) from the first chunk on
	for (uint32_t i = tid; i < VC_ED_CHUNK / 4; i += nthr) s_codes[i] = 0;
	if (LDSM) {
		const uint32_t row = nw * 64, total = A.n_class * NW * row;
		for (uint32_t i = tid; i < total; i += nthr) {
			const uint32_t l = i % row, cw = i / row;
			const uint32_t g = blockIdx.x * nw + (l >> 6);
			s_mask[i] = g < A.n_groups ? gmask[((size_t)g * A.n_class * NW + cw) * 64 + (l & 63u)] : (W)0;
		}
	}

	uint32_t m = active ? A.qlen[(size_t)group * 64 + lane] : 0;
	const bool valid = m > 0;
	if (!valid) m = HBHI ? 33 : (NW > 1 ? 65 : 1);   // an idle lane walks a harmless query
	const uint32_t hb = (m - 1) - (uint32_t)(NW - 1) * (uint32_t)(sizeof(W) * 8);
	const uint32_t pad = 64u * ((m + 63u) / 64u) - m;
	const uint32_t kp = (A.max_edit < 0 || (uint32_t)A.max_edit > m) ? m : (uint32_t)A.max_edit;

	VcEdState<W, NW> st;
	vc_ed_begin(st, m);
	uint32_t acc = 0;
	bool bad = false;

	uint64_t r = (uint64_t)blockIdx.y * A.reads_per_range;
	uint64_t r1 = r + A.reads_per_range;
	if (r1 > A.n_reads) r1 = A.n_reads;
	uint32_t done = 0;   // bytes of read r consumed by earlier chunks

	// the masks of this lane: LDS row stride between (class, word) entries
	const uint32_t lrow = nw * 64;
	const W *lm = s_mask + wave * 64 + lane;
	const W *gm = gmask + (size_t)(active ? group : 0) * A.n_class * NW * 64 + lane;

	__syncthreads();
	while (r < r1) {
		if (wave == 0) {
			const uint64_t ri = r + lane;
			const bool have = ri < r1;
			uint32_t len = 0;
			uint64_t off = 0;
			if (have) {
				len = A.lens[ri];
				off = A.offs[ri];
			}
			uint32_t rem = len;
			if (lane == 0) {
				rem = len - done;
				off += done;
			}
			// bytes the read takes in the chunk: its start is dword-aligned
			const uint32_t take = rem > VC_ED_CHUNK ? VC_ED_CHUNK + 4u : (rem + 3u) & ~3u;
			uint32_t end = take;
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const uint32_t y = __shfl_up(end, d, 64);
				if ((int)lane >= d) end += y;
			}
			const bool fit = have && end <= VC_ED_CHUNK;
			const uint32_t g = (uint32_t)__popcll(__ballot(fit));   // lengths add up: the fitting reads are a prefix
			if (g == 0) {
				if (lane == 0) {   // a piece of a read longer than what is left of a chunk
					s_src[0] = off;
					s_beg[0] = 0;
					s_end[0] = VC_ED_CHUNK;
					s_len[0] = len;
					s_flag[0] = done == 0 ? 1u : 0u;
					s_hdr[0] = 1;
					s_hdr[1] = 1;
				}
			} else {
				if (lane < g) {
					s_src[lane] = off;
					s_beg[lane] = end - take;
					s_end[lane] = end - take + rem;
					s_len[lane] = len;
					s_flag[lane] = ((lane > 0 || done == 0) ? 1u : 0u) | 2u;
				}
				if (lane == 0) {
					s_hdr[0] = g;
					s_hdr[1] = 0;
				}
			}
		}
		__syncthreads();
		const uint32_t nseg = s_hdr[0], piece = s_hdr[1];
		for (uint32_t s = wave; s < nseg; s += nw) {
			const uint32_t b = s_beg[s], n = s_end[s] - b;
			const uint64_t src = s_src[s];
			uint8_t *dst = reinterpret_cast<uint8_t *>(s_codes) + b;
			for (uint32_t j = lane; j < n; j += 64) {
				const uint64_t a = src + j;
				uint8_t ch = 0;
				if (a < A.seq_bytes) ch = A.seq[a];
				else bad = true;
				dst[j] = s_cls[ch];
			}
		}
		__syncthreads();
		if (active) {
			for (uint32_t s = 0; s < nseg; ++s) {
				const uint32_t e = uniform(s_end[s]), fl = uniform(s_flag[s]);
				uint32_t j = uniform(s_beg[s]);
				if (fl & 1u) vc_ed_begin(st, m);
				for (; j < e; j += 4) {
					const uint32_t c4 = uniform(s_codes[j >> 2]);
					const uint32_t nj = e - j < 4 ? e - j : 4;
					W eq[4][NW];
#pragma unroll
					for (int t = 0; t < 4; ++t) {
						const uint32_t c = (c4 >> (8 * t)) & 255u;   // bytes past nj: stale classes, masks unused
#pragma unroll
						for (int w = 0; w < NW; ++w)
							eq[t][w] = LDSM ? lm[(c * NW + w) * lrow] : gm[(size_t)(c * NW + w) * 64];
					}
#pragma unroll
					for (int t = 0; t < 4; ++t)
						if ((uint32_t)t < nj) vc_ed_step<W, NW, HBHI>(st, eq[t], hb);
				}
				if (fl & 2u) {
					const uint32_t add = vc_ed_end(st, uniform(s_len[s]), m, kp, pad);
					acc += valid ? add : 0u;
				}
			}
		}
		if (piece) {
			done += VC_ED_CHUNK;
		} else {
			r += nseg;
			done = 0;
		}
		__syncthreads();   // the chunk is consumed: wave 0 may lay out the next
	}
	if (valid && acc) atomicAdd(&A.counts[A.qout[(size_t)group * 64 + lane]], acc);
	if (bad) atomicOr(A.flags, 1u);
}

template <typename W, int NW, bool HBHI>
hipError_t launch_width(const VcEdArgs &A, int waves, int lds_masks, dim3 grid, hipStream_t st)
{
	const dim3 block(64u * (unsigned)waves);
	if (lds_masks) {
		const size_t dyn = (size_t)A.n_class * NW * waves * 64 * sizeof(W);
		hipLaunchKernelGGL((vc_ed_kernel<W, NW, true, HBHI>), grid, block, dyn, st, A);
	} else {
		hipLaunchKernelGGL((vc_ed_kernel<W, NW, false, HBHI>), grid, block, 0, st, A);
	}
	return hipGetLastError();
}

} // namespace

extern "C" hipError_t vc_ed_launch(const VcEdArgs *A, int width, int waves, int lds_masks, unsigned grid_x,
                                   unsigned grid_y, hipStream_t st)
{
	if (!A || waves < 1 || waves > VC_ED_MAX_WAVES || grid_x == 0 || grid_y == 0 || grid_y > 65535u)
		return hipErrorInvalidValue;
	if (lds_masks &&
	    (size_t)A->n_class * vc_ed_width_words(width) * waves * 64 * vc_ed_width_wordbytes(width) > VC_ED_LDS_MASKS)
		return hipErrorInvalidValue;
	const dim3 grid(grid_x, grid_y);
	switch (width) {
	case VC_ED_W32: return launch_width<uint32_t, 1, false>(*A, waves, lds_masks, grid, st);
	case VC_ED_W64: return launch_width<uint64_t, 1, true>(*A, waves, lds_masks, grid, st);
	case VC_ED_W128: return launch_width<uint64_t, 2, false>(*A, waves, lds_masks, grid, st);
	}
	return hipErrorInvalidValue;
}
