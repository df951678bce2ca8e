// vafc_vcf.h -- host side of vcf-vaf-counter (include/vafc.h, items 4-9 of its
// contract).  Plain C++ over zlib and the project's gzip inflater, no HIP: it
// links into libvafc.so and into stand-alone programs.
//
//   vc_vcf_header   sample count and declared FORMAT types of a VCF header
//   VcVcfText       the text of a plain, gzip or BGZF file, in order
//   vc_vcf_eval_line  one line under htslib's vcf_parse and process_vcf
#ifndef VAFC_VCF_H
#define VAFC_VCF_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <zlib.h>

#include <string>
#include <unordered_map>

#include "vafc.h"
#include "vafc_gzip.h"

struct vc_vcf_header {
	int n_samples = 0;
	std::unordered_map<std::string, int> fmt_type;   // FORMAT ID -> BCF_HT_*
};

// The decompressed bytes of a file, front to back.
class VcVcfText {
public:
	~VcVcfText() { close(); }
	// VC_OK or VC_EIO.  kind as vc_vcf_probe gives it.
	int open(const char *path, int kind, int n_threads);
	// Up to n next bytes into dst; 0 at the end (or at damaged compressed data).
	size_t read(uint8_t *dst, size_t n);
	void close();

private:
	FILE *fp_ = nullptr;
	gzFile gz_ = nullptr;
	VcGzParallel *gzp_ = nullptr;
};

#endif
