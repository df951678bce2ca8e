// bam_reader_check.cpp -- the BAM host reader (kmer-cnt_amd/csrc/vafc_bam.cpp)
// in a stand-alone program for sanitizer runs (tools/bam_reader_asan.sh): no
// GPU, no libvafc.so.  For every file given it reads the header and every
// record with each thread count and prints one line with a checksum of the
// descriptors and the data, which must not depend on the thread count.
//
//   bam_reader_check [-t a,b,..] file.bam ...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vafc.h"
#include "vafc_bam.h"

// the reader looks at rows only through these two; no pattern file is read here
extern "C" int vc_patterns_count(const vc_patterns *) { return 0; }
extern "C" int vc_pattern_fields(const vc_patterns *, int, const char **, int *, const char **, char *, char *,
                                 const char **, const char **)
{
	return VC_EINVAL;
}

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
	const uint8_t *b = (const uint8_t *)p;
	for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
	return h;
}

int main(int argc, char **argv)
{
	std::vector<int> threads = {1, 4};
	int first = 1;
	if (argc > 2 && strcmp(argv[1], "-t") == 0) {
		threads.clear();
		for (char *tok = strtok(argv[2], ","); tok; tok = strtok(nullptr, ",")) threads.push_back(atoi(tok));
		first = 3;
	}
	int bad = 0;
	for (int a = first; a < argc; ++a) {
		uint64_t want = 0;
		for (size_t ti = 0; ti < threads.size(); ++ti) {
			VcBamReader rd;
			const int rc = rd.open(argv[a], threads[ti]);
			uint64_t h = 0xCBF29CE484222325ull;
			uint64_t n = 0, bytes = 0;
			if (rc == VC_OK) {
				for (const std::string &s : rd.refs()) h = fnv(h, s.c_str(), s.size() + 1);
				std::vector<vc_bam_rec> recs;
				std::vector<uint8_t> data;
				// small batches: the walk over the data checks every offset against its own batch
				while (recs.clear(), data.clear(), rd.next_batch(recs, data, 4096, 64)) {
					for (const vc_bam_rec &r : recs) {
						const size_t need = 4 * (size_t)r.n_cigar + ((size_t)r.l_seq + 1) / 2;
						if (r.off % 4 || r.off + need > data.size()) {
							fprintf(stderr, "%s: a descriptor leaves its batch\n", argv[a]);
							return 2;
						}
						h = fnv(h, &r, 20);
						h = fnv(h, data.data() + r.off, need);
					}
					n += recs.size();
					bytes += data.size();
				}
			}
			if (ti == 0) {
				want = h;
				printf("%s\trc=%d\trefs=%zu\trecords=%llu\tdata=%llu\t%016llx\n", argv[a], rc, rd.refs().size(),
				       (unsigned long long)n, (unsigned long long)bytes, (unsigned long long)h);
			} else if (h != want) {
				fprintf(stderr, "%s: %d threads give another checksum\n", argv[a], threads[ti]);
				bad = 1;
			}
		}
	}
	return bad;
}
