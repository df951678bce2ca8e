// bam_main.cpp -- the `bam-vaf-counter` command on top of libvafc.so.
//
// Drop-in for the reference CLI (bam-vaf-counter.c:472-578): same options
// "p:o:t:" with ketopt's rules (vafc_opt.h), -t through atoi, same usage text,
// the program's own stderr lines in the same order, .vaf output and exit
// codes.  The first file is opened for its header, a later file that cannot
// be opened is reported and skipped.  Records are counted on the GPU (device:
// $VAFC_DEVICE, default 0); without a usable GPU the command exits 1.  Input
// is BGZF-compressed BAM only: SAM text, CRAM and uncompressed BAM exit 1 with
// a message naming the format.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vafc.h"
#include "vafc_opt.h"

int main(int argc, char *argv[])
{
	int c, n_thread = 4;
	const char *pattern_fn = nullptr, *out_fn = nullptr;
	VcOpt o;
	while ((c = vc_opt_next(o, argc, argv, "p:o:t:")) >= 0) {
		if (c == 'p') pattern_fn = o.arg;
		else if (c == 'o') out_fn = o.arg;
		else if (c == 't') n_thread = atoi(o.arg);
	}
	if (!pattern_fn || !out_fn || o.files.empty()) {
		fprintf(stderr, "Usage: bam-vaf-counter [options] -p <patterns.txt> -o <output.vaf> <reads.bam> [reads2.bam ...]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -p FILE   input pattern file\n");
		fprintf(stderr, "  -o FILE   output VAF file\n");
		fprintf(stderr, "  -t INT    number of threads [%d]\n", n_thread);
		fprintf(stderr, "\nNote: This version directly counts ref/alt bases at SNP positions (no k-mer extraction).\n");
		fprintf(stderr, "      It is much faster than k-mer-based counting.\n");
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

	// the first file's header gives every row its tid
	fprintf(stderr, "[M::%s] Reading BAM header...\n", "main");
	int kind = VC_BAM_BGZF;
	if (vc_bam_probe(o.files[0], &kind) != VC_OK) {
		fprintf(stderr, "Error: failed to open BAM file: %s\n", o.files[0]);
		return 1;
	}
	if (kind != VC_BAM_BGZF) {
		fprintf(stderr, "Error: %s is %s; only BGZF-compressed BAM is read\n", o.files[0], vc_bam_kind_name(kind));
		return 1;
	}
	vc_bam_file *hdr = nullptr;
	int rc = vc_bam_read_header(o.files[0], &hdr);
	if (rc != VC_OK) {
		if (rc == VC_EIO) fprintf(stderr, "Error: failed to open BAM file: %s\n", o.files[0]);
		else fprintf(stderr, "Error: failed to read BAM header\n");
		vc_bam_file_free(hdr);
		return 1;
	}

	fprintf(stderr, "[M::%s] Creating SNP position map...\n", "main");
	std::vector<const char *> names;
	for (int i = 0; i < vc_bam_file_refs(hdr); ++i) names.push_back(vc_bam_file_ref_name(hdr, i));
	const char *dev_env = getenv("VAFC_DEVICE");
	vc_bam *bam = nullptr;
	rc = vc_bam_create(&bam, db, names.data(), (int)names.size(), dev_env ? atoi(dev_env) : 0);
	vc_bam_file_free(hdr);
	if (rc != VC_OK) {
		fprintf(stderr, "Error: failed to set up the GPU counter (%s)\n", vc_strerror(rc));
		vc_patterns_free(db);
		return 1;
	}

	fprintf(stderr, "[M::%s] Building target regions from patterns...\n", "main");
	std::vector<int32_t> first((size_t)(n > 0 ? n : 1)), ends((size_t)(n > 0 ? n : 1));
	const int n_regions = vc_bam_build_regions(db, first.data(), ends.data());
	if (n_regions <= 0) {
		fprintf(stderr, "Error: failed to build regions\n");
		vc_bam_destroy(bam);
		vc_patterns_free(db);
		return 1;
	}
	fprintf(stderr, "[M::%s] Built %d target regions (merged from %d patterns)\n", "main", n_regions, n);

	fprintf(stderr, "[M::%s] Counting variants in BAM files with %d threads...\n", "main", n_thread);
	for (const char *fn : o.files) {
		fprintf(stderr, "[M::%s] Processing %s...\n", "main", fn);
		if (vc_bam_probe(fn, &kind) == VC_OK && kind != VC_BAM_BGZF) {
			fprintf(stderr, "Error: %s is %s; only BGZF-compressed BAM is read\n", fn, vc_bam_kind_name(kind));
			vc_bam_destroy(bam);
			vc_patterns_free(db);
			return 1;
		}
		// a file that cannot be opened, or whose header cannot be read, is reported and skipped
		vc_file_stats fst;
		rc = vc_bam_count_file(bam, fn, n_thread, &fst);
		// VAFC_PHASES=1: where the file's BGZF members were inflated (all on the
		// host after a device pass that gave the file up) and what was read
		if (getenv("VAFC_PHASES") && rc == VC_OK) {
			uint64_t hm = 0, dm = 0;
			(void)vc_bam_inflate_info(bam, &hm, &dm);
			vc_bam_seek_res sk;
			memset(&sk, 0, sizeof sk);
			(void)vc_bam_seek_info(bam, &sk);
			fprintf(stderr, "[P::main] %s: inflate host %llu device %llu members, %llu records, %llu bases, %.4f s", fn,
			        (unsigned long long)hm, (unsigned long long)dm, (unsigned long long)fst.seqs,
			        (unsigned long long)fst.bases, fst.seconds);
			// $VAFC_BAM_INDEX=seek: the state (VC_BAM_SEEK_*), the plan's spans, the members read, the pieces read again
			if (sk.state != VC_BAM_SEEK_OFF)
				fprintf(stderr, ", seek state %u spans %llu members %llu rereads %llu", sk.state, (unsigned long long)sk.spans,
				        (unsigned long long)sk.members, (unsigned long long)sk.rereads);
			fprintf(stderr, "\n");
		}
		if (rc != VC_OK && rc != VC_EIO && rc != VC_EINVAL) {
			fprintf(stderr, "Error: counting failed on %s (%s)\n", fn, vc_strerror(rc));
			vc_bam_destroy(bam);
			vc_patterns_free(db);
			return 1;
		}
	}
	std::vector<uint32_t> counts(2 * (size_t)n + 2, 0);
	rc = vc_bam_finish(bam, counts.data());
	vc_bam_destroy(bam);
	if (rc != VC_OK) {
		fprintf(stderr, "Error: counting failed (%s)\n", vc_strerror(rc));
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
