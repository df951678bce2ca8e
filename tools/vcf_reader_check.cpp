// vcf_reader_check.cpp -- the VCF host parser (kmer-cnt_amd/csrc/vafc_vcf.cpp)
// in a stand-alone program for sanitizer runs (tools/vcf_reader_asan.sh): no
// GPU, no libvafc.so.  For every file given it sniffs the kind, reads the text
// through the project's inflaters, parses the header and evaluates every data
// line for sample indices -1..2 and minimum depths 0 and 7, and prints one
// line with a checksum of the verdicts.  Then it does the same over every
// truncation of the file at a byte of its first 4 KB: of the text, held in a
// heap block of exactly that size so that a read past its end is seen, and,
// for a compressed file, of the file itself through a temporary copy.
//
//   vcf_reader_check tmpdir file.vcf[.gz] ...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "vafc.h"
#include "vafc_vcf.h"

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
	const uint8_t *b = (const uint8_t *)p;
	for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
	return h;
}

// Header and every line of text[0 .. len), which is its own heap block.
static uint64_t walk(const uint8_t *text, size_t len, uint64_t *lines)
{
	uint64_t h = 0xCBF29CE484222325ull;
	vc_vcf_header *hdr = nullptr;
	size_t body = 0;
	const int rc = vc_vcf_header_parse(text, len, 1, &hdr, &body);
	h = fnv(h, &rc, sizeof rc);
	if (rc != VC_OK) return h;
	const int ns = vc_vcf_header_samples(hdr), tg = vc_vcf_header_type(hdr, "GT"), ta = vc_vcf_header_type(hdr, "AD");
	h = fnv(fnv(fnv(h, &ns, sizeof ns), &tg, sizeof tg), &ta, sizeof ta);
	for (size_t p = body; p < len;) {
		const uint8_t *nl = (const uint8_t *)memchr(text + p, '\n', len - p);
		const size_t e = nl ? (size_t)(nl - text) + 1 : len;
		// the line in a block of its own size, too
		uint8_t *line = (uint8_t *)malloc(e - p ? e - p : 1);
		if (e > p) memcpy(line, text + p, e - p);
		for (int s = -1; s <= 2; ++s)
			for (int d = 0; d <= 7; d += 7) {
				vc_vcf_verdict v;
				const int r = vc_vcf_eval_line(hdr, line, e - p, s, d, &v);
				h = fnv(fnv(h, &r, sizeof r), &v, sizeof v);
			}
		free(line);
		++*lines;
		p = e;
	}
	vc_vcf_header_free(hdr);
	return h;
}

static bool slurp(const char *path, std::vector<uint8_t> *out, int *kind)
{
	out->clear();
	if (vc_vcf_probe(path, kind) != VC_OK) return false;
	if (*kind == VC_VCF_BCF) return true;
	VcVcfText in;
	if (in.open(path, *kind, 2) != VC_OK) return false;
	uint8_t buf[1 << 12];
	for (size_t n; (n = in.read(buf, sizeof buf)) > 0;) out->insert(out->end(), buf, buf + n);
	return true;
}

int main(int argc, char **argv)
{
	if (argc < 3) {
		fprintf(stderr, "usage: vcf_reader_check tmpdir file ...\n");
		return 2;
	}
	const std::string tmp = std::string(argv[1]) + "/vcf_reader_check.tmp";
	for (int a = 2; a < argc; ++a) {
		std::vector<uint8_t> text;
		int kind = -1;
		if (!slurp(argv[a], &text, &kind)) {
			fprintf(stderr, "%s: cannot be read\n", argv[a]);
			return 2;
		}
		uint64_t lines = 0, cut_lines = 0;
		uint8_t *whole = (uint8_t *)malloc(text.size() ? text.size() : 1);
		if (!text.empty()) memcpy(whole, text.data(), text.size());
		uint64_t h = walk(whole, text.size(), &lines);
		free(whole);
		const size_t cuts = text.size() < 4096 ? text.size() : 4096;
		for (size_t n = 0; n < cuts; ++n) {
			uint8_t *part = (uint8_t *)malloc(n ? n : 1);
			if (n) memcpy(part, text.data(), n);
			h = fnv(h, &n, sizeof n) ^ walk(part, n, &cut_lines);
			free(part);
		}
		if (kind == VC_VCF_GZIP || kind == VC_VCF_BGZF) {
			std::vector<uint8_t> raw;
			FILE *fp = fopen(argv[a], "rb");
			uint8_t buf[1 << 12];
			for (size_t n; fp && (n = fread(buf, 1, sizeof buf, fp)) > 0;) raw.insert(raw.end(), buf, buf + n);
			if (fp) fclose(fp);
			const size_t rcuts = raw.size() < 4096 ? raw.size() : 4096;
			for (size_t n = 0; n < rcuts; ++n) {
				fp = fopen(tmp.c_str(), "wb");
				if (!fp || fwrite(raw.data(), 1, n, fp) != n) {
					fprintf(stderr, "%s: cannot be written\n", tmp.c_str());
					return 2;
				}
				fclose(fp);
				std::vector<uint8_t> t2;
				int k2 = -1;
				if (slurp(tmp.c_str(), &t2, &k2)) {
					uint8_t *part = (uint8_t *)malloc(t2.size() ? t2.size() : 1);
					if (!t2.empty()) memcpy(part, t2.data(), t2.size());
					h ^= walk(part, t2.size(), &cut_lines);
					free(part);
				}
			}
			unlink(tmp.c_str());
		}
		printf("%s\tkind=%s\ttext=%zu\tlines=%llu\tcut_lines=%llu\t%016llx\n", argv[a], vc_vcf_kind_name(kind), text.size(),
		       (unsigned long long)lines, (unsigned long long)cut_lines, (unsigned long long)h);
	}
	return 0;
}
