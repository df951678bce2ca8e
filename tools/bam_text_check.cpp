// bam_text_check.cpp -- the device's BAM text scan (kmer-cnt_amd/csrc/vafc_bam_text.h:
// guess, link, emit and check) compiled for the host with a one-lane wave, in
// a stand-alone program for sanitizer runs (tools/bam_text_asan.sh): no GPU, no
// libvafc.so.  Every file given is one scan written by tests/bam_text_fixture.py:
// a text, its entry, cuts and final flag, and what the scan must report.  The
// text is copied into a heap block of exactly its size, so that a read outside
// it is seen; the stages run in the order of the kernels, each segment and
// each record on its own as a lane would.  One line per file:
//
//   <file> ok|BAD consumed records bases irregular irregular_off short_stop found rewalked
//
// and exit code 1 if any scan reports something else than the file states.
//
//   bam_text_check file ...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "vafc_bam_text.h"

namespace {

struct Head {
	char magic[4];
	int32_t n_ref;
	uint32_t final, rewalk_rule;   // rule 0: unstated, 1: none walked again, 2: at least one
	uint64_t entry, n_cuts, text_len;
	uint64_t consumed, records, bases, irr_off;
	uint32_t irr_n, short_stop, found, pad;
};

bool run(const char *path)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) {
		fprintf(stderr, "cannot open %s\n", path);
		exit(2);
	}
	std::vector<uint8_t> raw;
	uint8_t buf[65536];
	for (size_t got; (got = fread(buf, 1, sizeof buf, fp)) > 0;) raw.insert(raw.end(), buf, buf + got);
	fclose(fp);
	Head h;
	if (raw.size() < sizeof h) exit(2);
	memcpy(&h, raw.data(), sizeof h);
	if (memcmp(h.magic, "VBT1", 4) != 0 || raw.size() != sizeof h + 8 * h.n_cuts + 4 * (uint64_t)h.found + h.text_len) {
		fprintf(stderr, "%s is no case file\n", path);
		exit(2);
	}
	std::vector<uint64_t> cuts(h.n_cuts);
	if (h.n_cuts) memcpy(cuts.data(), raw.data() + sizeof h, 8 * h.n_cuts);
	std::vector<uint32_t> want_offs(h.found);
	if (h.found) memcpy(want_offs.data(), raw.data() + sizeof h + 8 * h.n_cuts, 4 * (size_t)h.found);
	uint8_t *text = (uint8_t *)malloc(h.text_len ? h.text_len : 1);
	if (h.text_len) memcpy(text, raw.data() + raw.size() - h.text_len, h.text_len);
	const uint64_t len = h.text_len;
	const uint32_t n_cuts = (uint32_t)h.n_cuts, n_seg = n_cuts + 1;

	// guess
	std::vector<VbtSeg> segs(n_seg);
	for (uint32_t s = 0; s < n_seg; ++s) {
		uint64_t a, b;
		vbt_seg_range(cuts.data(), n_cuts, len, s, &a, &b);
		VbtSeg sg = {vbt_guess(text, len, a, b, h.n_ref), 0, 0, 0};
		if (sg.entry != VBT_NONE) vbt_walk(text, len, sg.entry, b, &sg, nullptr, 0);
		segs[s] = sg;
	}
	// link
	VbtResult res;
	memset(&res, 0, sizeof res);
	uint64_t e = h.entry;
	uint32_t stop = VBT_STOP_NONE, rewalked = 0;
	for (uint32_t s = 0; s < n_seg; ++s) {
		uint64_t a, b;
		vbt_seg_range(cuts.data(), n_cuts, len, s, &a, &b);
		vbt_link_step(text, len, a, b, &segs[s], &e, &stop, &rewalked);
	}
	vbt_link_end(text, len, e, stop, h.final != 0, rewalked, &res);
	// emit: a list of exactly the size the link has counted
	uint64_t total = 0;
	for (const VbtSeg &sg : segs) total += sg.entry == VBT_NONE ? 0 : sg.count;
	std::vector<uint32_t> offs(total);
	for (uint32_t s = 0; s < n_seg; ++s) {
		const VbtSeg sg = segs[s];
		if (sg.entry == VBT_NONE || sg.count == 0) continue;
		uint64_t a, b;
		vbt_seg_range(cuts.data(), n_cuts, len, s, &a, &b);
		VbtSeg again;
		vbt_walk(text, len, sg.entry, b, &again, offs.data() + res.n_found, sg.count);
		res.n_found += sg.count;
	}
	// check
	for (uint32_t i = 0; i < res.n_found; ++i) {
		vc_bam_rec r;
		if (vbt_check(text, offs[i], &r)) {
			++res.records;
			res.bases += r.l_seq;
			// what the count kernels will read: the CIGAR and the bases lie inside the text
			if (r.off + 4 * (uint64_t)r.n_cigar + (((uint64_t)r.l_seq + 1) >> 1) > len) res.records += 1u << 30;
		} else {
			vbt_skip_rec(&r);
			++res.irr_n;
			res.irr_off = std::min<uint64_t>(res.irr_off, offs[i]);
		}
	}
	std::sort(offs.begin(), offs.end());
	const bool ok = res.consumed == h.consumed && res.records == h.records && res.bases == h.bases && res.irr_n == h.irr_n &&
	                res.irr_off == h.irr_off && res.short_stop == h.short_stop && res.n_found == h.found && offs == want_offs &&
	                (h.rewalk_rule != 1 || res.rewalked == 0) && (h.rewalk_rule != 2 || res.rewalked >= 1);
	const char *name = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;
	printf("%s %s %llu %llu %llu %u %lld %u %u %u\n", name, ok ? "ok" : "BAD", (unsigned long long)res.consumed,
	       (unsigned long long)res.records, (unsigned long long)res.bases, res.irr_n, (long long)res.irr_off, res.short_stop,
	       res.n_found, res.rewalked);
	free(text);
	return ok;
}

} // namespace

int main(int argc, char **argv)
{
	if (argc < 2) {
		fprintf(stderr, "usage: bam_text_check file ...\n");
		return 2;
	}
	int bad = 0;
	for (int a = 1; a < argc; ++a) bad += run(argv[a]) ? 0 : 1;
	if (bad) fprintf(stderr, "bam_text_check: %d of %d scans differ from their statement\n", bad, argc - 1);
	return bad ? 1 : 0;
}
