// vafc_bam.h -- host reader of BGZF-compressed BAM for bam-vaf-counter
// (include/vafc.h, items 7 and 8 of its contract).  Plain C++ over zlib and
// threads, no HIP: it links into libvafc.so and into stand-alone programs.
//
//   VcBgzf        BGZF blocks found by their BC extra field, inflated by worker
//                 threads a group ahead of the consumer, delivered in order
//   VcBamReader   the BAM header, then records across block borders, each
//                 reduced to a descriptor, its CIGAR words and its packed bases
#ifndef VAFC_BAM_H
#define VAFC_BAM_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <future>
#include <string>
#include <vector>

#include "vafc.h"

// One group of consecutive blocks, inflated side by side into `text`.
struct VcBgzfGroup {
	std::vector<uint8_t> raw;      // compressed blocks, whole (and room for the next one read)
	std::vector<uint32_t> boff;    // block i at raw[boff[i]], boff[n] = end
	std::vector<uint32_t> toff;    // its text at text[toff[i]]
	std::vector<uint8_t> text;
	size_t text_len = 0;           // text of the blocks before the first bad one
	bool last = false;             // end of file, or a block that ends the stream (item 7)
};

class VcBgzf {
public:
	~VcBgzf() { close(); }
	bool open(const char *path, int n_threads);
	void close();
	// The next n bytes of text, contiguous (valid until the next call), or
	// NULL when fewer are left before the end of the stream.
	const uint8_t *take(size_t n);
	// Members inflated so far, the group read ahead included.
	uint64_t members() const { return members_.load(); }

private:
	std::atomic<uint64_t> members_{0};
	void load(VcBgzfGroup *g);     // read and inflate the next group
	bool advance();                // make `cur` the next group
	FILE *fp_ = nullptr;
	int threads_ = 1;
	VcBgzfGroup grp_[2];
	int cur_ = 0;
	size_t pos_ = 0;               // next byte of grp_[cur_].text
	bool have_cur_ = false;
	std::future<void> pending_;    // load of grp_[cur_ ^ 1]
	bool pending_valid_ = false;
	std::vector<uint8_t> carry_;   // a request that spans groups
};

class VcBamReader {
public:
	// VC_OK, VC_EIO (cannot open) or VC_EINVAL (not BGZF BAM: a message names
	// the format; or the header cannot be read: header_ok() is false).
	int open(const char *path, int n_threads);
	bool header_ok() const { return header_ok_; }
	const std::vector<std::string> &refs() const { return refs_; }
	// Append records until `data` holds max_bytes or `recs` max_recs of them (at
	// least one record is taken); false when the file's records have ended.
	// Offsets are relative to data[0] and multiples of 4.
	bool next_batch(std::vector<vc_bam_rec> &recs, std::vector<uint8_t> &data, size_t max_bytes, size_t max_recs);
	uint64_t bases = 0, records = 0;
	uint64_t members() const { return z_.members(); }   // BGZF members inflated for it

private:
	VcBgzf z_;
	bool header_ok_ = false, ended_ = false;
	uint32_t in_batch_ = 0;       // records read since the reference's batch of 1,000 began (item 7)
	uint32_t empty_batches_ = 0;  // batches a failed read closed empty: the second ends the file
	std::vector<std::string> refs_;
};

#endif
