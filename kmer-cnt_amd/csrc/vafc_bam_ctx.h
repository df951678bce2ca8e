// vafc_bam_ctx.h -- the bam-vaf-counter handle (vc_bam of include/vafc.h), shared
// by its device unit (vafc_bam.hip: tables, kernels, block and text entries)
// and its file passes (vafc_bam_files.cpp).  Host code of HIP units only.
#ifndef VAFC_BAM_CTX_H
#define VAFC_BAM_CTX_H

#include <string>
#include <vector>

#include "vafc.h"
#include "vafc_bam_text.h"
#include "vafc_stage.h"

struct vc_bam : VcDevice {
	uint32_t n_pat = 0, n_rows = 0;
	VcDevBuf<uint64_t> d_row_key;
	VcDevBuf<uint2> d_row_info;
	VcDevBuf<uint32_t> d_counts, d_flags;   // 2 * n_pat + 2, 1
	VcDevBuf<uint64_t> d_reg_s, d_reg_e;    // one capacity (vc_bam_set_regions)
	uint32_t n_reg = 0;
	VcDevBuf<uint32_t> d_long_list, d_long_n;
	uint32_t long_thr = 64;
	// the rows as build_regions sees them: merged regions by chromosome name
	std::vector<std::string> reg_chr;
	std::vector<int32_t> reg_start, reg_end;
	// records in text (vc_bam_scan_text_*): the lists are sized by the text
	int32_t n_ref = 0;                      // of the guess: the header's references
	VcDevBuf<VbtSeg> d_segs;
	VcDevBuf<uint64_t> d_cuts;              // of a scan whose cuts come from the host
	VcDevBuf<uint32_t> d_offs;
	VcDevBuf<vc_bam_rec> d_trecs;
	VcDevBuf<VbtResult> d_tres;             // 1
	VcTimer text_timer, check_timer;        // of the last scan: guess, link and emit (or the piece walk); check
	// pieces in text (vc_bam_scan_pieces_*): the outcomes of the last scan's pieces
	VcDevBuf<vc_bam_piece_status> d_pstat;
	VcDevBuf<vc_bam_piece> d_pieces;        // of a scan whose pieces come from the host
	size_t n_pieces_last = 0;
	// the device pass of vc_bam_count_file: inflater, two text buffers with
	// room in front of the text for the tail of the piece before
	vc_bgzf *zf = nullptr;
	VcDevBuf<uint8_t> ztext[2];
	size_t zhead[2] = {0, 0};
	uint64_t z_host_members = 0, z_device_members = 0;   // of the last file (vc_bam_inflate_info)
	vc_bam_seek_res z_seek = {0, 0, 0, 0, 0};             // of the last file (vc_bam_seek_info)
};

// vc_bam_scan_text_device on the handle's own stream with the cuts in host
// memory (they have left it on return).
int vc_bam_scan_text_cuts(vc_bam *c, const uint8_t *d_text, size_t text_bytes, uint64_t entry, const uint64_t *cuts,
                          size_t n_cuts, int final);
// vc_bam_scan_pieces_device on the handle's own stream with the pieces in host
// memory (they have left it on return).
int vc_bam_scan_pieces_host(vc_bam *c, const uint8_t *d_text, size_t text_bytes, const vc_bam_piece *pieces, size_t n_pieces);

#endif
