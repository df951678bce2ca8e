// ed_main.cpp -- the `ed-vaf-counter` command on top of libvafc.so.
//
// Drop-in for the reference CLI (ed-vaf-counter.c:156-236): same options
// "p:o:e:" with ketopt's rules (vafc_opt.h), -e through atoi, same usage
// text, stderr lines, .vaf output and exit codes.  Every pattern k-mer is
// searched in every read with a bounded edit distance on the GPU (device:
// $VAFC_DEVICE, default 0); without a usable GPU the command exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vafc.h"
#include "vafc_opt.h"

int main(int argc, char *argv[])
{
	int c, max_edit_dist = 0;
	const char *pattern_fn = nullptr, *out_fn = nullptr;
	VcOpt o;
	while ((c = vc_opt_next(o, argc, argv, "p:o:e:")) >= 0) {
		if (c == 'p') pattern_fn = o.arg;
		else if (c == 'o') out_fn = o.arg;
		else if (c == 'e') max_edit_dist = atoi(o.arg);
	}
	if (!pattern_fn || !out_fn || o.files.empty()) {
		fprintf(stderr, "Usage: ed-vaf-counter [options] -p <patterns.txt> -o <output.vaf> <reads.fq> [reads2.fq ...]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -p FILE   input pattern file\n");
		fprintf(stderr, "  -o FILE   output VAF file\n");
		fprintf(stderr, "  -e INT    maximum edit distance for approximate matching [%d]\n", max_edit_dist);
		fprintf(stderr, "\nDescription:\n");
		fprintf(stderr, "  This program uses edlib to search for pattern k-mers in FASTQ reads.\n");
		fprintf(stderr, "  Unlike vaf-counter which extracts all k-mers from reads and looks them up,\n");
		fprintf(stderr, "  ed-vaf-counter searches for each pattern k-mer in the reads using approximate\n");
		fprintf(stderr, "  string matching. This can be more efficient for small pattern sets.\n");
		fprintf(stderr, "  Set -e 0 for exact matches only (default), or higher values to allow mismatches.\n");
		return 1;
	}

	fprintf(stderr, "[M::%s] Loading patterns...\n", "main");
	vc_patterns *db = nullptr;
	if (vc_patterns_load(pattern_fn, &db) != VC_OK) {
		fprintf(stderr, "Error: failed to load pattern file\n");
		return 1;
	}
	const int n = vc_patterns_count(db);
	fprintf(stderr, "[M::%s] Loaded %d patterns\n", "main", n);

	const char *dev_env = getenv("VAFC_DEVICE");
	vc_ed *ed = nullptr;
	int rc = vc_ed_create(&ed, db, max_edit_dist, dev_env ? atoi(dev_env) : 0);
	if (rc != VC_OK) {
		fprintf(stderr, "Error: failed to set up the GPU search (%s)\n", vc_strerror(rc));
		vc_patterns_free(db);
		return 1;
	}

	fprintf(stderr, "[M::%s] Searching for k-mers in FASTQ files (max edit distance: %d)...\n", "main", max_edit_dist);
	const char *thr_env = getenv("VAFC_THREADS");
	const int n_threads = thr_env ? atoi(thr_env) : 4;
	for (const char *fn : o.files) {
		fprintf(stderr, "[M::%s] Processing %s...\n", "main", fn);
		rc = vc_ed_count_file(ed, fn, n_threads, nullptr);
		if (rc == VC_EIO) {
			fprintf(stderr, "Warning: failed to open %s\n", fn);
			continue;
		}
		if (rc != VC_OK) {
			fprintf(stderr, "Error: searching failed on %s (%s)\n", fn, vc_strerror(rc));
			vc_ed_destroy(ed);
			vc_patterns_free(db);
			return 1;
		}
	}
	std::vector<uint32_t> counts(2 * (size_t)n + 2, 0);
	rc = vc_ed_finish(ed, counts.data());
	vc_ed_destroy(ed);
	if (rc != VC_OK) {
		fprintf(stderr, "Error: searching failed (%s)\n", vc_strerror(rc));
		vc_patterns_free(db);
		return 1;
	}
	uint64_t total_ref = 0, total_alt = 0;
	for (int i = 0; i < n; ++i) {
		total_ref += counts[2 * (size_t)i];
		total_alt += counts[2 * (size_t)i + 1];
	}
	const double avg_depth = (double)(total_ref + total_alt) / (n > 0 ? n : 1);

	fprintf(stderr, "[M::%s] Writing VAF file...\n", "main");
	if (vc_write_vaf(db, counts.data(), out_fn) != VC_OK) {
		fprintf(stderr, "Error: failed to open output file\n");
		vc_patterns_free(db);
		return 1;
	}
	fprintf(stderr, "[M::%s] Done. Average depth: %.2f\n", "main", avg_depth);
	vc_patterns_free(db);
	return 0;
}
