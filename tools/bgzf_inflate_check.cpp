// bgzf_inflate_check.cpp -- the device inflater's decode text
// (kmer-cnt_amd/csrc/vafc_inflate.h) compiled for the host with a one-lane
// wave, in a stand-alone program for sanitizer runs
// (tools/bgzf_inflate_asan.sh): no GPU, no libvafc.so, no zlib.  Every file
// given is a run of BGZF members (tests/bgzf_fixture.py writes the cases, the
// malformed ones included).  Each member's payload is copied into a heap block
// of exactly its size and inflated into a heap block of exactly ISIZE bytes,
// so that a read or a write outside either is seen.  One line per member:
//
//   <file> <member> <status> <isize> <adler32 of the text, 0 unless status is 0>
//
// Bytes that are no whole member end a file's walk with a line "<file> end
// <offset> <reason>".
//
//   bgzf_inflate_check file ...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vafc_bgzf.h"
#include "vafc_inflate.h"

static uint32_t adler32(const uint8_t *p, size_t n)
{
	uint32_t a = 1, b = 0;
	for (size_t i = 0; i < n; ++i) {
		a = (a + p[i]) % 65521u;
		b = (b + a) % 65521u;
	}
	return b << 16 | a;
}

int main(int argc, char **argv)
{
	if (argc < 2) {
		fprintf(stderr, "usage: bgzf_inflate_check file ...\n");
		return 2;
	}
	static VciTables tables;
	VciTables *T = &tables;
	vci_crc_table<1>(*T, 0);
	for (int a = 1; a < argc; ++a) {
		FILE *fp = fopen(argv[a], "rb");
		if (!fp) {
			fprintf(stderr, "cannot open %s\n", argv[a]);
			return 2;
		}
		std::vector<uint8_t> raw;
		uint8_t buf[65536];
		for (size_t got; (got = fread(buf, 1, sizeof buf, fp)) > 0;) raw.insert(raw.end(), buf, buf + got);
		fclose(fp);
		const char *name = strrchr(argv[a], '/') ? strrchr(argv[a], '/') + 1 : argv[a];
		size_t at = 0;
		for (int k = 0; at < raw.size(); ++k) {
			VcBgzfMember m;
			const int rc = vc_bgzf_member_at(raw.data() + at, raw.size() - at, &m);
			if (rc != 1) {
				printf("%s end %zu %s\n", name, at, rc == 0 ? "cut" : "not-a-member");
				break;
			}
			uint8_t *in = (uint8_t *)malloc(m.payload_len);
			if (m.payload_len) memcpy(in, raw.data() + at + m.payload, m.payload_len);
			// an ISIZE the decoder must refuse untouched gets no text at all
			const size_t room = m.isize > VCI_MAX_TEXT ? 0 : m.isize;
			uint8_t *out = (uint8_t *)malloc(room);
			if (room) memset(out, 0xA5, room);
			const int st = vci_inflate<1>(*T, in, (uint32_t)m.payload_len, out, m.isize, m.crc32, 0);
			printf("%s %d %d %u %u\n", name, k, st, m.isize, st == 0 ? adler32(out, room) : 0u);
			free(in);
			free(out);
			at += m.size;
		}
	}
	return 0;
}
