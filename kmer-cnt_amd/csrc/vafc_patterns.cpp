// vafc_patterns.cpp -- the pattern database of libvafc.so (vc_patterns_*,
// vc_write_vaf of include/vafc.h).  No HIP here.
//
//   patterns      load_patterns / create_combined_kmer_map   vaf-counter.c:149-252
//   write_vaf     .vaf writer                                  vaf-counter.c:653-681
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <unordered_map>
#include <vector>

#include "vafc.h"

namespace {

struct Pattern {
	char chr[256];
	int start, end;
	char rsid[256];
	char ref, alt;
	char ref_kmer[128];
	char alt_kmer[128];
};

unsigned char g_nt4[256];
bool g_nt4_init = false;

void init_nt4()
{
	if (g_nt4_init) return;
	for (int i = 0; i < 256; ++i) g_nt4[i] = 4;
	for (int i = 0; i < 4; ++i) g_nt4[i] = (unsigned char)i;
	const char *acgt[4] = {"Aa", "Cc", "Gg", "TtUu"};
	for (int c = 0; c < 4; ++c)
		for (const char *p = acgt[c]; *p; ++p) g_nt4[(unsigned char)*p] = (unsigned char)c;
	g_nt4_init = true;
}

// 2-bit key of the first k characters (vaf-counter.c:117-127); UINT64_MAX if
// any of them is not A/C/G/T/U (either case) or a raw byte 0..3.
uint64_t string_key(const char *s, int k)
{
	uint64_t x = 0;
	for (int i = 0; i < k; ++i) {
		unsigned c = g_nt4[(unsigned char)s[i]];
		if (c > 3) return UINT64_MAX;
		x = (x << 2) | c;
	}
	return x;
}

uint64_t canonical(uint64_t x, int k)
{
	uint64_t r = 0, y = x;
	for (int i = 0; i < k; ++i, y >>= 2) r = (r << 2) | (3u - (y & 3u));
	return r < x ? r : x;
}

} // namespace

struct vc_patterns {
	std::vector<Pattern> a;
};

extern "C" int vc_patterns_load(const char *path, vc_patterns **out)
{
	if (!path || !out) return VC_EINVAL;
	*out = nullptr;
	FILE *fp = fopen(path, "r");
	if (!fp) return VC_EIO;
	vc_patterns *db = new (std::nothrow) vc_patterns;
	if (!db) {
		fclose(fp);
		return VC_ENOMEM;
	}
	// One record buffer reused across records, like the reference's local
	// pattern_t: a k-mer string shorter than k is followed by its NUL and by
	// bytes of earlier longer strings (the reference's buffer starts as
	// uninitialised stack; this one starts zeroed).
	Pattern rec;
	memset(&rec, 0, sizeof(rec));
	while (fscanf(fp, "%255s%d%d%255s %c %c%127s%127s", rec.chr, &rec.start, &rec.end, rec.rsid,
	              &rec.ref, &rec.alt, rec.ref_kmer, rec.alt_kmer) == 8)
		db->a.push_back(rec);
	fclose(fp);
	*out = db;
	return VC_OK;
}

extern "C" void vc_patterns_free(vc_patterns *db) { delete db; }

extern "C" int vc_patterns_count(const vc_patterns *db) { return db ? (int)db->a.size() : 0; }

extern "C" int vc_pattern_fields(const vc_patterns *db, int i, const char **chr, int *start,
                                 const char **rsid, char *ref, char *alt, const char **ref_kmer,
                                 const char **alt_kmer)
{
	if (!db || i < 0 || (size_t)i >= db->a.size()) return VC_EINVAL;
	const Pattern &p = db->a[(size_t)i];
	if (chr) *chr = p.chr;
	if (start) *start = p.start;
	if (rsid) *rsid = p.rsid;
	if (ref) *ref = p.ref;
	if (alt) *alt = p.alt;
	if (ref_kmer) *ref_kmer = p.ref_kmer;
	if (alt_kmer) *alt_kmer = p.alt_kmer;
	return VC_OK;
}

extern "C" void vc_free(void *p) { free(p); }

extern "C" int vc_patterns_keys(const vc_patterns *db, int k, uint64_t **keys, uint32_t **vals,
                                size_t *n_keys, int *n_collisions)
{
	if (!db || !keys || !vals || !n_keys || k < 1 || k > 31) return VC_EINVAL;
	const size_t n = db->a.size();
	if (n > (size_t)(INT32_MAX >> 1)) return VC_ETOOMANY;   // vaf-counter.c:205-209
	init_nt4();
	uint64_t *K = (uint64_t *)malloc((2 * n + 1) * sizeof(uint64_t));
	uint32_t *V = (uint32_t *)malloc((2 * n + 1) * sizeof(uint32_t));
	if (!K || !V) {
		free(K);
		free(V);
		return VC_ENOMEM;
	}
	std::unordered_map<uint64_t, uint32_t> seen;
	seen.reserve(2 * n + 1);
	size_t m = 0;
	int coll = 0;
	for (size_t i = 0; i < n; ++i) {
		for (int allele = 0; allele < 2; ++allele) {
			const char *s = allele ? db->a[i].alt_kmer : db->a[i].ref_kmer;
			uint64_t x = string_key(s, k);
			if (x == UINT64_MAX) continue;
			uint64_t c = canonical(x, k);
			uint32_t v = ((uint32_t)i << 1) | (uint32_t)allele;
			if (seen.emplace(c, v).second) {
				K[m] = c;
				V[m] = v;
				++m;
			} else {
				++coll;                     // first insert wins (khashl.h:218)
			}
		}
	}
	*keys = K;
	*vals = V;
	*n_keys = m;
	if (n_collisions) *n_collisions = coll;
	return VC_OK;
}

extern "C" int vc_write_vaf(const vc_patterns *db, const uint32_t *counts, const char *path)
{
	if (!db || !path) return VC_EINVAL;
	const size_t n = db->a.size();
	uint64_t tot_ref = 0, tot_alt = 0;
	for (size_t i = 0; i < n; ++i) {
		tot_ref += counts ? counts[2 * i] : 0;
		tot_alt += counts ? counts[2 * i + 1] : 0;
	}
	const double avg = (double)(tot_ref + tot_alt) / (n > 0 ? (double)n : 1.0);
	FILE *fp = fopen(path, "w");
	if (!fp) return VC_EIO;
	setvbuf(fp, nullptr, _IOFBF, 1 << 20);
	fprintf(fp, "# Average depth: %.2f\n", avg);
	fprintf(fp, "CHR\tPOS\tRSID\tREF\tALT\tREF_COUNT\tALT_COUNT\tTOTAL_COUNT\tVAF\n");
	for (size_t i = 0; i < n; ++i) {
		const Pattern &p = db->a[i];
		const uint32_t rc = counts ? counts[2 * i] : 0, ac = counts ? counts[2 * i + 1] : 0;
		const uint32_t tot = rc + ac;                       // u32 wrap, as the reference
		const double vaf = tot > 0 ? (double)ac / tot : 0.0;
		fprintf(fp, "%s\t%d\t%s\t%c\t%c\t%u\t%u\t%u\t%.4f\n", p.chr, p.start, p.rsid, p.ref, p.alt, rc,
		        ac, tot, vaf);
	}
	return fclose(fp) == 0 ? VC_OK : VC_EIO;
}
