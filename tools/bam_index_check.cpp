// bam_index_check.cpp -- the BAI reader and seek planner
// (kmer-cnt_amd/csrc/vafc_bam_index.cpp) and the device's piece walk
// (kmer-cnt_amd/csrc/vafc_bam_text.h, vbt_piece_walk, compiled for the host with
// a one-lane wave) in a stand-alone program for sanitizer runs
// (tools/bam_index_asan.sh): no GPU, no libvafc.so.  Each file given is
//
//   *.vbp   a piece case of tests/bam_seek_fixture.py: a text, its pieces and
//           what the walk of each must report.  The text is copied into a heap
//           block of exactly its size, so that a read outside it is seen; every
//           piece is walked to count and again to emit, as a lane does.
//   other   a BAI index.  The parser and the planner run over the whole file
//           (which must plan), over every prefix of it and over FLIPS seeded
//           byte flips, each from a heap block of exactly its size; the regions
//           are a grid over every reference the file's own n_ref names.  A plan
//           that is made must ascend and keep its spans in separate members.
//
// One line per file, "<file> ok|BAD ...", and exit code 1 if any is BAD.
//
//   bam_index_check file ...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "vafc_bam_text.h"

#include "vafc_bam_index.cpp"

// vc_bam_index_plan looks for an index beside a BAM only without an index path; not here
extern "C" int vc_bam_index_usable(const char *, char *, size_t) { return 0; }

namespace {

const int FLIPS = 4000;

std::vector<uint8_t> slurp(const char *path)
{
	std::vector<uint8_t> raw;
	if (!read_all(path, raw)) {
		fprintf(stderr, "cannot read %s\n", path);
		exit(2);
	}
	return raw;
}

const char *base_name(const char *path) { return strrchr(path, '/') ? strrchr(path, '/') + 1 : path; }

bool run_pieces(const char *path)
{
	const std::vector<uint8_t> raw = slurp(path);
	uint32_t n_pieces = 0;
	uint64_t text_len = 0;
	if (raw.size() < 16 || memcmp(raw.data(), "VBP1", 4) != 0) exit(2);
	memcpy(&n_pieces, raw.data() + 4, 4);
	memcpy(&text_len, raw.data() + 8, 8);
	if (raw.size() != 16 + 40 * (uint64_t)n_pieces + text_len) {
		fprintf(stderr, "%s is no case file\n", path);
		exit(2);
	}
	uint8_t *text = (uint8_t *)malloc(text_len ? text_len : 1);
	if (text_len) memcpy(text, raw.data() + raw.size() - text_len, text_len);
	bool ok = true;
	uint64_t total = 0;
	for (uint32_t i = 0; i < n_pieces; ++i) {
		vc_bam_piece p;
		uint32_t want_status, want_found;
		uint64_t want_missing;
		const uint8_t *at = raw.data() + 16 + 40 * (size_t)i;
		memcpy(&p, at, 24);
		memcpy(&want_status, at + 24, 4);
		memcpy(&want_found, at + 28, 4);
		memcpy(&want_missing, at + 32, 8);
		uint32_t found = 0, again = 0;
		uint64_t missing = 0, none = 0;
		const uint32_t status = vbt_piece_walk(text, text_len, p, &found, &missing, nullptr, 0);
		// emit: a list of exactly the size the first walk has counted
		std::vector<uint32_t> offs(found);
		(void)vbt_piece_walk(text, text_len, p, &again, &none, offs.data(), found);
		for (uint32_t k = 0; k + 1 < found; ++k) ok = ok && offs[k] < offs[k + 1];
		const uint64_t limit = p.limit < text_len ? p.limit : text_len;
		for (uint32_t k = 0; k < found; ++k) ok = ok && offs[k] >= p.entry && offs[k] < p.stop && offs[k] + VBT_FIXED <= limit;
		ok = ok && status == want_status && found == want_found && missing == want_missing && again == found;
		total += found;
	}
	printf("%s %s %u pieces %llu records\n", base_name(path), ok ? "ok" : "BAD", n_pieces, (unsigned long long)total);
	free(text);
	return ok;
}

bool sound(const std::vector<vc_bam_span> &sp)
{
	for (size_t i = 0; i < sp.size(); ++i) {
		if (sp[i].end < sp[i].beg) return false;
		if (i && (sp[i].beg >> 16) <= (sp[i - 1].end >> 16)) return false;
	}
	return true;
}

bool run_index(const char *path)
{
	const std::vector<uint8_t> raw = slurp(path);
	if (raw.size() < 8) exit(2);
	int32_t n_ref = 0;
	memcpy(&n_ref, raw.data() + 4, 4);
	if (n_ref < 0 || n_ref > 1000) exit(2);
	std::vector<int32_t> tid, start, end;
	for (int32_t t = 0; t < n_ref; ++t) {
		for (int32_t s = 0; s < (1 << 29) - (1 << 22); s += (1 << 22) + 12345) {
			tid.push_back(t), start.push_back(s), end.push_back(s + 1 + s % 40000);
		}
		for (int32_t s = 0; s < 200000; s += 997) tid.push_back(t), start.push_back(s), end.push_back(s + 1);
		tid.push_back(t), start.push_back(0), end.push_back(1 << 29);
	}
	auto plan = [&](const std::vector<uint8_t> &bytes, std::vector<vc_bam_span> &sp) {
		sp.clear();
		const std::vector<uint8_t> exact(bytes.begin(), bytes.end());   // capacity == size
		return plan_bytes(exact, n_ref, tid.data(), start.data(), end.data(), tid.size(), sp);
	};
	std::vector<vc_bam_span> sp, whole;
	bool ok = plan(raw, whole) == VC_OK && sound(whole) && !whole.empty();
	size_t planned = 0;
	for (size_t n = 0; n < raw.size(); ++n) {
		const int rc = plan(std::vector<uint8_t>(raw.begin(), raw.begin() + n), sp);
		ok = ok && (rc == VC_BAM_NO_SEEK || (rc == VC_OK && sound(sp)));
		planned += rc == VC_OK;
	}
	ok = ok && planned <= 1;   // the prefix that lacks only n_no_coor
	uint64_t x = 0x9E3779B97F4A7C15ull;
	size_t flipped_ok = 0;
	for (int k = 0; k < FLIPS; ++k) {
		std::vector<uint8_t> b = raw;
		const int n = 1 + k % 3;
		for (int j = 0; j < n; ++j) {
			x ^= x << 13, x ^= x >> 7, x ^= x << 17;
			b[(x >> 8) % b.size()] ^= (uint8_t)(1u << (x & 7));
		}
		const int rc = plan(b, sp);
		ok = ok && (rc == VC_BAM_NO_SEEK || (rc == VC_OK && sound(sp)));
		flipped_ok += rc == VC_OK;
	}
	printf("%s %s %zu spans, %zu prefixes of which %zu plan, %d flips of which %zu plan\n", base_name(path), ok ? "ok" : "BAD",
	       whole.size(), raw.size(), planned, FLIPS, flipped_ok);
	return ok;
}

} // namespace

int main(int argc, char **argv)
{
	if (argc < 2) {
		fprintf(stderr, "usage: bam_index_check file ...\n");
		return 2;
	}
	int bad = 0;
	for (int a = 1; a < argc; ++a) {
		const size_t n = strlen(argv[a]);
		const bool pieces = n > 4 && strcmp(argv[a] + n - 4, ".vbp") == 0;
		bad += (pieces ? run_pieces(argv[a]) : run_index(argv[a])) ? 0 : 1;
	}
	if (bad) fprintf(stderr, "bam_index_check: %d of %d files differ from their statement\n", bad, argc - 1);
	return bad ? 1 : 0;
}
