// vcf_main.cpp -- the `vcf-vaf-counter` command on top of libvafc.so.
//
// Drop-in for the reference CLI (vcf-vaf-counter.c:206-278): same options
// "p:o:v:s:d:" with ketopt's rules (vafc_opt.h), -s and -d through atoi, same
// usage text, the program's own stderr lines in the same order, .vaf output
// and exit codes: an input that cannot be opened or has no VCF header is
// reported and the all-zero .vaf is still written with exit code 0.  Lines are
// matched against the panel on the GPU (device: $VAFC_DEVICE, default 0);
// without a usable GPU the command exits 1.  BCF exits 1 with a message naming
// the format.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vafc.h"
#include "vafc_opt.h"

int main(int argc, char *argv[])
{
	int c, sample_idx = 0, min_depth = 1;
	const char *pattern_fn = nullptr, *out_fn = nullptr, *vcf_fn = nullptr;
	VcOpt o;
	while ((c = vc_opt_next(o, argc, argv, "p:o:v:s:d:")) >= 0) {
		if (c == 'p') pattern_fn = o.arg;
		else if (c == 'o') out_fn = o.arg;
		else if (c == 'v') vcf_fn = o.arg;
		else if (c == 's') sample_idx = atoi(o.arg);
		else if (c == 'd') min_depth = atoi(o.arg);
	}
	if (!pattern_fn || !out_fn || !vcf_fn) {
		fprintf(stderr, "Usage: vcf-vaf-counter [options] -p <patterns.txt> -v <input.vcf> -o <output.vaf>\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -p FILE   input pattern file\n");
		fprintf(stderr, "  -v FILE   input VCF/BCF file\n");
		fprintf(stderr, "  -o FILE   output VAF file\n");
		fprintf(stderr, "  -s INT    sample index (0-based) [%d]\n", sample_idx);
		fprintf(stderr, "  -d INT    minimum depth [%d]\n", min_depth);
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

	fprintf(stderr, "[M::%s] Processing VCF file...\n", "main");
	std::vector<uint32_t> counts(2 * (size_t)n + 2, 0);
	int kind = VC_VCF_OTHER;
	if (vc_vcf_probe(vcf_fn, &kind) == VC_OK && kind == VC_VCF_BCF) {
		fprintf(stderr, "Error: %s is %s; only VCF text (plain, gzip or BGZF) is read\n", vcf_fn, vc_vcf_kind_name(kind));
		vc_patterns_free(db);
		return 1;
	}
	const char *dev_env = getenv("VAFC_DEVICE");
	vc_vcf *v = nullptr;
	int rc = vc_vcf_create(&v, db, dev_env ? atoi(dev_env) : 0);
	if (rc != VC_OK) {
		fprintf(stderr, "Error: failed to set up the GPU line matcher (%s)\n", vc_strerror(rc));
		vc_patterns_free(db);
		return 1;
	}
	// a file that cannot be opened, or has no header, is reported and counts nothing
	rc = vc_vcf_count_file(v, vcf_fn, sample_idx, min_depth, 4, counts.data(), nullptr);
	vc_vcf_destroy(v);
	if (rc == VC_VCF_ABORTED) {   // htslib's own exit(1) inside the reference's loop: no .vaf
		vc_patterns_free(db);
		return 1;
	}
	if (rc != VC_OK && rc != VC_EIO && rc != VC_EINVAL) {
		fprintf(stderr, "Error: processing failed on %s (%s)\n", vcf_fn, vc_strerror(rc));
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
