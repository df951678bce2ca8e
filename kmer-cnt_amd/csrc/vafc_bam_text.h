// vafc_bam_text.h -- finding and checking BAM records in inflated text, shared
// by the kernels (vafc_bam.hip) and, with a one-lane "wave", by host programs
// (tools/bam_text_check.cpp runs this text under the sanitizers).  Not part of
// the public C ABI (include/vafc.h).
//
// A BAM text is a chain: the record at offset o has a block_size word, the next
// record is at o + 4 + block_size.  The chain is found by speculation and then
// verified, so that no heuristic reaches a count:
//
//   segments  the text is cut at `cuts` (ascending offsets): segment s is
//             [cut[s-1], cut[s]), the first starts at 0, the last ends at len
//   guess     per segment: the first offset where a plausible record starts
//             (vbt_plausible, a chain of VBT_CHAIN of them or one that leaves
//             the segment), and from there the walk to the segment's end
//   link      the segments in order, with the piece's true entry e: e at or past
//             the segment's end passes through; e equal to the guess takes the
//             guessed exit; otherwise the segment is walked again from e.  By
//             induction every segment's entry is that of the serial walk.
//   walk      the exact rule, the same in the guess and in the link: a record is
//             a block_size >= 32 that fits into the text; the walk stops at a
//             block_size < 32 (VBT_STOP_SHORT) and at a record the text cuts off
//             (VBT_STOP_FIT)
//   check     per record found: the field tests of VcBamReader::next_batch
//             (vafc_bam.cpp); a record that fails one is irregular
//   pieces    many short chains in one text, each with the entry an index gives
//             (vbt_piece_walk): no guess and no link, the same walk rule, ended
//             at the piece's stop and bounded by the piece's limit
//
// Bounds, by construction: every read of text is a byte load at a position
// tested against len before it is issued; a walk over a segment of n bytes
// takes at most n / 36 + 2 trips (every trip passes a record of 36 bytes or
// more), a guess at most n * VBT_CHAIN plausibility tests, a check at most
// n_cigar word loads inside the record's own bytes.
#ifndef VAFC_BAM_TEXT_H
#define VAFC_BAM_TEXT_H

#include <stddef.h>
#include <stdint.h>

#include "vafc.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBT_HD __host__ __device__ __forceinline__
#else
#define VBT_HD inline
#endif

enum { VBT_STOP_NONE = 0, VBT_STOP_FIT = 1, VBT_STOP_SHORT = 2 };

#define VBT_NONE (~(uint64_t)0)   // no guess; no entry
#define VBT_CHAIN 3               // plausible records in a row that make a guess
#define VBT_FIXED 36              // block_size word and the fixed fields

// What the guess leaves per segment and the link makes true: on the way out of
// the link `entry` is the segment's first record of the serial walk (VBT_NONE:
// it holds no record start) and `count` its records.
struct VbtSeg {
	uint64_t entry, exit;
	uint32_t count, stop;
};

// The outcome of one scan (vc_bam_text_res of include/vafc.h is made of it).
struct VbtResult {
	uint64_t consumed;    // where the walk ended: the text's length, or the record that stopped it
	uint64_t records;     // regular records
	uint64_t bases;       // the sum of their l_seq
	uint64_t irr_off;     // lowest offset of an irregular record (VBT_NONE: none)
	uint32_t irr_n;
	uint32_t rewalked;    // segments whose guess was not the true entry
	uint32_t short_stop;  // the walk stopped at a block_size < 32
	uint32_t n_found;     // records found, irregular ones included
	uint32_t n_short, n_cut, n_noroom, pad;   // of a piece walk: pieces that ended so
};

VBT_HD uint32_t vbt_le16(const uint8_t *t, uint64_t o) { return (uint32_t)t[o] | (uint32_t)t[o + 1] << 8; }
VBT_HD uint32_t vbt_le32(const uint8_t *t, uint64_t o) { return vbt_le16(t, o) | vbt_le16(t, o + 2) << 16; }

// Segment s of n_cuts + 1: [*a, *b), empty where the cuts do not ascend.
VBT_HD void vbt_seg_range(const uint64_t *cuts, uint32_t n_cuts, uint64_t len, uint32_t s, uint64_t *a, uint64_t *b)
{
	uint64_t lo = s == 0 ? 0 : cuts[s - 1], hi = s >= n_cuts ? len : cuts[s];
	if (lo > len) lo = len;
	if (hi > len) hi = len;
	if (hi < lo) hi = lo;
	*a = lo;
	*b = hi;
}

// The fixed fields of the record at o (o + VBT_FIXED <= len) fit its block_size
// bl >= 32: the test of next_batch before it takes the record's body.
VBT_HD bool vbt_fields_fit(const uint8_t *t, uint64_t o, uint32_t bl)
{
	const uint32_t l_qname = t[o + 12], n_cigar = vbt_le16(t, o + 16);
	const int32_t l_seq = (int32_t)vbt_le32(t, o + 20);
	if (l_seq < 0 || l_qname < 1) return false;
	const uint64_t seq_bytes = ((uint64_t)l_seq + 1) >> 1;
	return ((uint64_t)n_cigar << 2) + l_qname + seq_bytes + (uint64_t)l_seq <= (uint64_t)bl - 32;
}

// Whether a record can start at o < len, by what of it lies in the text
// (fields past the text's end are not tested); *next: where the chain goes on.
VBT_HD bool vbt_plausible(const uint8_t *t, uint64_t len, uint64_t o, int32_t n_ref, uint64_t *next)
{
	*next = len;
	if (len - o < 4) return true;
	const int32_t bl = (int32_t)vbt_le32(t, o);
	if (bl < 32) return false;
	*next = o + 4 + (uint64_t)bl;
	if (len - o < VBT_FIXED) return true;
	const int32_t tid = (int32_t)vbt_le32(t, o + 4), pos = (int32_t)vbt_le32(t, o + 8);
	const int32_t next_tid = (int32_t)vbt_le32(t, o + 24);
	if (tid < -1 || tid >= n_ref || next_tid < -1 || next_tid >= n_ref || pos < -1) return false;
	if (!vbt_fields_fit(t, o, (uint32_t)bl)) return false;
	const uint64_t nul = o + VBT_FIXED + t[o + 12] - 1;   // the name's last byte
	return nul >= len || t[nul] == 0;
}

// The first offset in [a, b) where VBT_CHAIN plausible records follow one
// another, or fewer that leave the segment; VBT_NONE without one.
VBT_HD uint64_t vbt_guess(const uint8_t *t, uint64_t len, uint64_t a, uint64_t b, int32_t n_ref)
{
	for (uint64_t o = a; o < b; ++o) {
		uint64_t p = o, nx = 0;
		bool ok = true;
		for (int k = 0; k < VBT_CHAIN; ++k) {
			if (!vbt_plausible(t, len, p, n_ref, &nx)) {
				ok = false;
				break;
			}
			if (nx >= b) break;
			p = nx;
		}
		if (ok) return o;
	}
	return VBT_NONE;
}

// The exact walk from o to the first chain offset at or past b <= len (or to
// the record that stops it); offs, when given, takes the records' offsets (at
// most max_offs of them: the count of an earlier walk from the same o).
VBT_HD void vbt_walk(const uint8_t *t, uint64_t len, uint64_t o, uint64_t b, VbtSeg *sg, uint32_t *offs, uint32_t max_offs)
{
	uint32_t count = 0, stop = VBT_STOP_NONE;
	const uint64_t trips = o < b ? (b - o) / VBT_FIXED + 2 : 0;
	for (uint64_t i = 0; i < trips && o < b; ++i) {
		if (len - o < 4) {
			stop = VBT_STOP_FIT;
			break;
		}
		const int32_t bl = (int32_t)vbt_le32(t, o);
		if (bl < 32) {
			stop = VBT_STOP_SHORT;
			break;
		}
		if ((uint64_t)bl > len - o - 4) {
			stop = VBT_STOP_FIT;
			break;
		}
		if (offs && count < max_offs) offs[count] = (uint32_t)o;
		++count;
		o += 4 + (uint64_t)bl;
	}
	sg->exit = o;
	sg->count = count;
	sg->stop = stop;
}

// One step of the link over segment [a, b), whose guess is in *sg: *e is the
// chain's entry on the way in and its exit on the way out, *stop what has ended
// the walk (no later segment is entered then).
VBT_HD void vbt_link_step(const uint8_t *t, uint64_t len, uint64_t a, uint64_t b, VbtSeg *sg, uint64_t *e, uint32_t *stop,
                          uint32_t *rewalked)
{
	(void)a;
	if (*stop != VBT_STOP_NONE || *e >= b) {   // ended, or the segment lies inside a record
		sg->entry = VBT_NONE;
		sg->count = 0;
		return;
	}
	if (*e != sg->entry) {
		vbt_walk(t, len, *e, b, sg, nullptr, 0);
		sg->entry = *e;
		++*rewalked;
	}
	*e = sg->exit;
	*stop = sg->stop;
}

// After the last segment: where the walk ended and why.  A final piece's cut
// record whose fixed fields are there and do not fit is what next_batch drops
// and reads on behind: irregular.
VBT_HD void vbt_link_end(const uint8_t *t, uint64_t len, uint64_t e, uint32_t stop, bool final, uint32_t rewalked, VbtResult *res)
{
	res->consumed = e;
	res->rewalked = rewalked;
	res->short_stop = stop == VBT_STOP_SHORT;
	res->irr_off = VBT_NONE;
	res->irr_n = 0;
	if (final && stop == VBT_STOP_FIT && len - e >= VBT_FIXED && !vbt_fields_fit(t, e, vbt_le32(t, e))) {
		res->irr_off = e;
		res->irr_n = 1;
	}
}

// A piece (vc_bam_piece of include/vafc.h): a chain whose entry is known, as
// the index gives it.  The walk takes every record that starts in [entry,
// stop) and lies whole below limit, under the rule of vbt_walk; entry and stop
// past limit, and limit past the text, are clamped, so that every read is at a
// position tested against the clamped limit and a piece of n bytes behind its
// entry takes at most n / 36 + 2 trips.  offs, when given, takes the records'
// offsets (at most max_offs: the count of an earlier walk of the same piece).
// *missing: the bytes of a cut record that lie past limit, 0 where its
// block_size word is not whole either.
VBT_HD uint32_t vbt_piece_walk(const uint8_t *t, uint64_t text_bytes, const vc_bam_piece &p, uint32_t *count, uint64_t *missing,
                               uint32_t *offs, uint32_t max_offs)
{
	const uint64_t limit = p.limit < text_bytes ? p.limit : text_bytes;
	const uint64_t stop = p.stop < limit ? p.stop : limit;
	uint64_t o = p.entry < limit ? p.entry : limit;
	uint32_t n = 0, status = VC_BAM_PIECE_OK;
	*missing = 0;
	const uint64_t trips = o < stop ? (limit - o) / VBT_FIXED + 2 : 0;
	for (uint64_t i = 0; i < trips && o < stop; ++i) {
		if (limit - o < 4) {
			status = VC_BAM_PIECE_CUT;
			break;
		}
		const int32_t bl = (int32_t)vbt_le32(t, o);
		if (bl < 32) {
			status = VC_BAM_PIECE_SHORT;
			break;
		}
		if ((uint64_t)bl > limit - o - 4) {
			status = VC_BAM_PIECE_CUT;
			*missing = (uint64_t)bl - (limit - o - 4);
			break;
		}
		if (offs && n < max_offs) offs[n] = (uint32_t)o;
		++n;
		o += 4 + (uint64_t)bl;
	}
	*count = n;
	return status;
}

// The record at o, which the walk has found whole inside the text: true and
// *r (off: where its CIGAR starts in the text) if it is regular.
VBT_HD bool vbt_check(const uint8_t *t, uint64_t o, vc_bam_rec *r)
{
	const uint32_t bl = vbt_le32(t, o);
	if (!vbt_fields_fit(t, o, bl)) return false;
	r->tid = (int32_t)vbt_le32(t, o + 4);
	r->pos = (int32_t)vbt_le32(t, o + 8);
	r->n_cigar = vbt_le16(t, o + 16);
	r->flag = vbt_le16(t, o + 18);
	r->l_seq = vbt_le32(t, o + 20);
	r->reserved = 0;
	r->off = o + VBT_FIXED + t[o + 12];
	if (r->n_cigar == 0) return true;
	// the CG:B,I long-CIGAR convention stays with the host reader: the first word
	// that announces it, and aux bytes in which the tag can lie
	const uint64_t fields = ((uint64_t)r->n_cigar << 2) + t[o + 12] + (((uint64_t)r->l_seq + 1) >> 1) + r->l_seq;
	if (vbt_le32(t, r->off) == (r->l_seq << 4 | 4u) && r->tid >= 0 && r->pos >= 0 && fields < (uint64_t)bl - 32) return false;
	if (r->l_seq == 0 || (r->flag & 4u)) return true;
	uint64_t qlen = 0;
	for (uint32_t k = 0; k < r->n_cigar; ++k) {
		const uint32_t c = vbt_le32(t, r->off + 4 * (uint64_t)k), op = c & 15u;
		if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += c >> 4;
	}
	return qlen == r->l_seq;
}

// A descriptor the count kernels pass over, in place of an irregular record.
VBT_HD void vbt_skip_rec(vc_bam_rec *r)
{
	r->tid = -1;
	r->pos = 0;
	r->flag = 0x4u;
	r->n_cigar = r->l_seq = r->reserved = 0;
	r->off = 0;
}

#endif
