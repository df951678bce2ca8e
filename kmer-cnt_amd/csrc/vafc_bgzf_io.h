// vafc_bgzf_io.h -- one BGZF member at a time from a file, on the host: the
// reader of the BAM host reader (vafc_bam.cpp) and of vcf-vaf-counter's file
// passes (vafc_vcf_files.cpp).  Plain C++ over stdio and zlib, no HIP; what
// needs neither is vafc_bgzf.h.
#ifndef VAFC_BGZF_IO_H
#define VAFC_BGZF_IO_H

#include <stdio.h>
#include <zlib.h>

#include "vafc_bgzf.h"

const size_t VC_BGZF_MAX_MEMBER = 65536;   // BSIZE is 16 bits

// The 12 fixed bytes and the extra field of the member at the file position
// into dst (room for VC_BGZF_MAX_MEMBER): the member's size, 0 = clean end of
// file, -1 = cut or not BGZF.  The file position is behind the extra field.
inline long vc_bgzf_read_head(FILE *fp, uint8_t *dst)
{
	const size_t got = fread(dst, 1, VC_BGZF_HEAD, fp);
	if (got == 0) return 0;
	if (got != VC_BGZF_HEAD || !vc_bgzf_head_ok(dst)) return -1;
	const size_t xlen = vc_bgzf_xlen(dst);
	// (no member has room for a longer extra field: it is not read into dst)
	if (VC_BGZF_HEAD + xlen + VC_BGZF_TAIL > VC_BGZF_MAX_MEMBER) return -1;
	if (xlen && fread(dst + VC_BGZF_HEAD, 1, xlen, fp) != xlen) return -1;
	const size_t size = vc_bgzf_member_size(dst + VC_BGZF_HEAD, xlen);
	return size ? (long)size : -1;
}

// One whole member at the file position into dst (room for
// VC_BGZF_MAX_MEMBER): 1 = read (*m describes it), 0 = clean end of file,
// -1 = cut, not BGZF, or ISIZE above 65,536 (no member holds more text).
inline int vc_bgzf_read_member(FILE *fp, uint8_t *dst, VcBgzfMember *m)
{
	const long size = vc_bgzf_read_head(fp, dst);
	if (size <= 0) return (int)size;
	const size_t head = VC_BGZF_HEAD + vc_bgzf_xlen(dst), rest = (size_t)size - head;
	if (fread(dst + head, 1, rest, fp) != rest) return -1;
	return vc_bgzf_member_at(dst, (size_t)size, m) == 1 && m->isize <= VC_BGZF_MAX_TEXT ? 1 : -1;
}

// Inflate the whole member m at mem into out, which has room for its ISIZE;
// false unless it inflates to exactly ISIZE bytes with the CRC-32 of its
// trailer.  Nothing is allocated: it runs on the BAM reader's threads.
inline bool vc_bgzf_inflate_member(const uint8_t *mem, const VcBgzfMember &m, uint8_t *out)
{
	z_stream zs = z_stream();
	if (inflateInit2(&zs, -15) != Z_OK) return false;
	uint8_t dummy;
	zs.next_in = const_cast<uint8_t *>(mem + m.payload);
	zs.avail_in = (uInt)m.payload_len;
	zs.next_out = m.isize ? out : &dummy;
	zs.avail_out = m.isize ? m.isize : 1;   // text longer than ISIZE ends in Z_BUF_ERROR or a wrong total_out
	const int rc = inflate(&zs, Z_FINISH);
	const bool ok = rc == Z_STREAM_END && zs.total_out == m.isize;
	inflateEnd(&zs);
	return ok && (uint32_t)crc32(crc32(0L, Z_NULL, 0), out, m.isize) == m.crc32;
}

#endif
