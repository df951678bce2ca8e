// vafc_bgzf.h -- the BGZF member walk over bytes in memory, shared by the
// device inflater's index (vc_bgzf_index, vafc_bgzf.hip) and the host's member
// reader (vafc_bgzf_io.h).  Plain C++, no zlib, no HIP.
//
// A BGZF member is a gzip member with FEXTRA set whose extra field holds a
// subfield 'B' 'C' of two bytes: BSIZE, the member's whole size minus one.
// Behind the 12 fixed bytes and the extra field comes the raw deflate payload,
// then CRC-32 and ISIZE of the text, which is at most 65,536 bytes.
#ifndef VAFC_BGZF_H
#define VAFC_BGZF_H

#include <stddef.h>
#include <stdint.h>

const uint32_t VC_BGZF_MAX_TEXT = 65536;   // of one member
const size_t VC_BGZF_HEAD = 12;            // fixed bytes in front of the extra field
const size_t VC_BGZF_TAIL = 8;             // CRC-32, ISIZE

inline uint32_t vc_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t vc_le32(const uint8_t *p) { return vc_le16(p) | vc_le16(p + 2) << 16; }

// Whether 12 bytes begin a gzip member that can be BGZF: deflate, FEXTRA.
inline bool vc_bgzf_head_ok(const uint8_t *h) { return h[0] == 31 && h[1] == 139 && h[2] == 8 && (h[3] & 4); }
inline size_t vc_bgzf_xlen(const uint8_t *h) { return vc_le16(h + 10); }

// The BSIZE of a member from its extra field (xlen bytes), or -1.
inline int vc_bgzf_bsize(const uint8_t *extra, size_t xlen)
{
	for (size_t i = 0; i + 4 <= xlen;) {
		const size_t slen = vc_le16(extra + i + 2);
		if (extra[i] == 'B' && extra[i + 1] == 'C' && slen == 2 && i + 6 <= xlen) return (int)vc_le16(extra + i + 4);
		i += 4 + slen;
	}
	return -1;
}

// The size of the member with this extra field, or 0 when it names none that
// can hold its own header and trailer.
inline size_t vc_bgzf_member_size(const uint8_t *extra, size_t xlen)
{
	const int bsize = vc_bgzf_bsize(extra, xlen);
	if (bsize < 0 || (size_t)bsize + 1 < VC_BGZF_HEAD + xlen + VC_BGZF_TAIL) return 0;
	return (size_t)bsize + 1;
}

struct VcBgzfMember {
	size_t size;       // the whole member
	size_t payload;    // offset of the deflate stream inside it
	size_t payload_len;
	uint32_t crc32, isize;
};

// The member at p, of which `avail` bytes are there: 1 = whole, in *m; 0 = it
// is cut off by the end of the bytes (as far as they go they can be a member);
// -1 = not a BGZF member.
inline int vc_bgzf_member_at(const uint8_t *p, size_t avail, VcBgzfMember *m)
{
	if (avail < VC_BGZF_HEAD) {
		// what is there of the fixed bytes must fit
		static const uint8_t magic[3] = {31, 139, 8};
		for (size_t i = 0; i < avail && i < 3; ++i)
			if (p[i] != magic[i]) return -1;
		if (avail > 3 && !(p[3] & 4)) return -1;
		return 0;
	}
	if (!vc_bgzf_head_ok(p)) return -1;
	const size_t xlen = vc_bgzf_xlen(p);
	if (avail < VC_BGZF_HEAD + xlen) return 0;
	const size_t size = vc_bgzf_member_size(p + VC_BGZF_HEAD, xlen);
	if (size == 0) return -1;
	if (avail < size) return 0;
	m->size = size;
	m->payload = VC_BGZF_HEAD + xlen;
	m->payload_len = size - VC_BGZF_HEAD - xlen - VC_BGZF_TAIL;
	m->crc32 = vc_le32(p + size - 8);
	m->isize = vc_le32(p + size - 4);
	return 1;
}

#endif
