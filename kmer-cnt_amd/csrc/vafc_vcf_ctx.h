// vafc_vcf_ctx.h -- the vc_vcf of include/vafc.h: what the device unit
// (vafc_vcf.hip: kernels, table, scans) and the file passes
// (vafc_vcf_files.cpp) share.  Host code only.
#ifndef VAFC_VCF_CTX_H
#define VAFC_VCF_CTX_H

#include <string>
#include <unordered_map>
#include <vector>

#include "vafc_stage.h"

// The scan that has been launched and not yet collected.
struct VcVcfPending {
	const uint8_t *d_text = nullptr;
	uint64_t len = 0, file_off = 0;
	int final_block = 0;
	hipStream_t st = nullptr;
	bool active = false;
};

struct vc_vcf : VcDevice {
	uint32_t n_rows = 0;
	VcDevBuf<uint4> d_table;
	uint32_t mask = 0;
	VcDevBuf<uint8_t> d_names;
	VcDevBuf<uint16_t> d_row_ra;
	VcDevBuf<uint4> d_hits;       // max_hits entries once a scan has run
	size_t max_hits = (size_t)1 << 20;
	VcDevBuf<unsigned long long> d_n_hits;
	VcDevBuf<uint64_t> d_consumed;
	size_t block_bytes = (size_t)32 << 20;   // of one block of vc_vcf_count_file
	VcVcfPending pend;
	std::vector<vc_vcf_hit> acc;  // collected since the last vc_vcf_hits
	bool handed = false;          // acc was returned: the next scan starts a new list
	size_t last_consumed = 0;
	uint64_t lines_reported = 0;
	// the rows on the host, for the lines the device leaves to it
	std::unordered_map<std::string, uint32_t> first_row;   // vcf_host_key
	std::vector<uint16_t> row_ra;
	// BGZF input inflated on the device (created by the first such file)
	vc_bgzf *zf = nullptr;
	VcDevBuf<uint8_t> ztext[2];   // the text of two pieces in turn, each behind `zhead` bytes of room for a tail
	size_t zhead[2] = {0, 0};
	uint64_t z_device_blocks = 0, z_host_blocks = 0;   // vc_vcf_inflate_info
};

// chr + '\t' + start
inline std::string vcf_host_key(const char *chr, size_t len, int32_t start)
{
	std::string k(chr, len);
	k.push_back('\t');
	k += std::to_string(start);
	return k;
}

#endif
