// vafc_vcf.cpp -- the host rules of vcf-vaf-counter: what kind of file, its
// header, and one data line under htslib's vcf_parse (vcf.c:3641-3805,
// vcf_parse_format :2818-3394) followed by process_vcf
// (vcf-vaf-counter.c:129-195).  No HIP here.
#include "vafc_vcf.h"

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

namespace {

const int HT_FLAG = 0, HT_INT = 1, HT_REAL = 2, HT_STR = 3;
const int32_t I32_MISSING = INT32_MIN, I32_VEND = INT32_MIN + 1;   // bcf_int32_missing, bcf_int32_vector_end
const int MAX_N_FMT = 255;

// The value of key in "k1=v1,k2="v,2",..." (the inside of <...>), quotes removed.
bool angle_value(const std::string &in, const char *key, std::string *val)
{
	size_t i = 0;
	const size_t klen = strlen(key);
	while (i < in.size()) {
		size_t eq = i;
		while (eq < in.size() && in[eq] != '=' && in[eq] != ',') ++eq;
		const std::string k = in.substr(i, eq - i);
		if (eq >= in.size() || in[eq] == ',') {   // a key without a value
			i = eq + 1;
			continue;
		}
		size_t p = eq + 1;
		std::string v;
		if (p < in.size() && in[p] == '"') {
			for (++p; p < in.size() && in[p] != '"'; ++p) {
				if (in[p] == '\\' && p + 1 < in.size()) ++p;
				v.push_back(in[p]);
			}
			while (p < in.size() && in[p] != ',') ++p;
		} else {
			while (p < in.size() && in[p] != ',') v.push_back(in[p++]);
		}
		if (k.size() == klen && memcmp(k.data(), key, klen) == 0) {
			*val = v;
			return true;
		}
		i = p + 1;
	}
	return false;
}

void header_format_line(vc_vcf_header *h, const std::string &line)
{
	static const char pre[] = "##FORMAT=<";
	if (line.compare(0, sizeof pre - 1, pre) != 0) return;
	const size_t close = line.rfind('>');
	if (close == std::string::npos || close < sizeof pre - 1) return;
	const std::string in = line.substr(sizeof pre - 1, close - (sizeof pre - 1));
	std::string id, type;
	if (!angle_value(in, "ID", &id) || !angle_value(in, "Type", &type) || id.empty()) return;
	int t;
	if (type == "Integer") t = HT_INT;
	else if (type == "Float") t = HT_REAL;
	else if (type == "String" || type == "Character") t = HT_STR;
	else if (type == "Flag") t = HT_FLAG;
	else return;
	h->fmt_type.emplace(id, t);   // the first declaration stays
}

// hts_str2uint (textutils_internal.h:297-329) for `bits` < 64: [+]digits; false
// if the value does not fit.  *end: the first byte not taken.
bool str2uint(const char *in, const char **end, int bits, uint64_t *val)
{
	const uint64_t limit = ((uint64_t)1 << bits) - 1;
	const unsigned char *v = (const unsigned char *)in;
	uint64_t n = 0;
	bool ok = true;
	if (*v == '+') ++v;
	for (; *v >= '0' && *v <= '9'; ++v) {
		const unsigned d = *v - '0';
		if (ok && (n < limit / 10 || (n == limit / 10 && d <= limit % 10))) n = n * 10 + d;
		else ok = false;
	}
	*end = (const char *)v;
	*val = ok ? n : limit;
	return ok;
}

// hts_str2int (:218-290) at 64 bits: [+-]digits; false on overflow.
bool str2int(const char *in, const char **end, int64_t *val)
{
	const unsigned char *v = (const unsigned char *)in;
	bool neg = false, ok = true;
	if (*v == '-') {
		neg = true;
		++v;
	} else if (*v == '+') {
		++v;
	}
	const uint64_t limit = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1;
	uint64_t n = 0;
	for (; *v >= '0' && *v <= '9'; ++v) {
		const unsigned d = *v - '0';
		if (ok && (n < limit / 10 || (n == limit / 10 && d <= limit % 10))) n = n * 10 + d;
		else ok = false;
	}
	*end = (const char *)v;
	*val = neg ? (int64_t)(0 - n) : (int64_t)n;
	return ok;
}

struct Fmt {
	int type = HT_STR;
	bool is_gt = false, dup = false;
	int max_m = 0, max_g = 0;
	std::vector<int32_t> val;   // [n_sample * width]
	int width = 0;
};

} // namespace

extern "C" const char *vc_vcf_kind_name(int kind)
{
	switch (kind) {
	case VC_VCF_PLAIN: return "VCF text";
	case VC_VCF_GZIP: return "gzip-compressed VCF";
	case VC_VCF_BGZF: return "BGZF-compressed VCF";
	case VC_VCF_BCF: return "BCF";
	default: return "not VCF";
	}
}

extern "C" int vc_vcf_probe(const char *path, int *kind)
{
	if (!path || !kind) return VC_EINVAL;
	FILE *fp = fopen(path, "rb");
	if (!fp) return VC_EIO;
	uint8_t b[18];
	const size_t n = fread(b, 1, sizeof b, fp);
	fclose(fp);
	if (n >= 2 && b[0] == 0x1f && b[1] == 0x8b) {
		// BGZF: FEXTRA with a BC subfield first (SAM spec 4.1)
		const bool bgzf = n >= 18 && (b[3] & 4) && b[12] == 'B' && b[13] == 'C' && b[14] == 2 && b[15] == 0;
		uint8_t t[4] = {0, 0, 0, 0};
		gzFile gz = gzopen(path, "rb");
		int got = 0;
		if (gz) {
			got = gzread(gz, t, sizeof t);
			gzclose(gz);
		}
		if (got >= 3 && memcmp(t, "BCF", 3) == 0) *kind = VC_VCF_BCF;
		else *kind = bgzf ? VC_VCF_BGZF : VC_VCF_GZIP;
		return VC_OK;
	}
	if (n >= 3 && memcmp(b, "BCF", 3) == 0) *kind = VC_VCF_BCF;
	else if (n >= 16 && memcmp(b, "##fileformat=VCF", 16) == 0) *kind = VC_VCF_PLAIN;
	else *kind = VC_VCF_OTHER;
	return VC_OK;
}

int VcVcfText::open(const char *path, int kind, int n_threads)
{
	close();
	if (kind == VC_VCF_GZIP || kind == VC_VCF_BGZF) {
		gzp_ = vc_gzp_open(path, n_threads > 0 ? n_threads : 1, 0);
		if (gzp_) return VC_OK;
		gz_ = gzopen(path, "rb");
		return gz_ ? VC_OK : VC_EIO;
	}
	fp_ = fopen(path, "rb");
	return fp_ ? VC_OK : VC_EIO;
}

size_t VcVcfText::read(uint8_t *dst, size_t n)
{
	size_t got = 0;
	while (got < n) {
		int64_t r;
		const size_t want = n - got < ((size_t)1 << 30) ? n - got : (size_t)1 << 30;
		if (gzp_) r = vc_gzp_read(gzp_, dst + got, want);
		else if (gz_) r = gzread(gz_, dst + got, (unsigned)want);
		else if (fp_) r = (int64_t)fread(dst + got, 1, want, fp_);
		else r = 0;
		if (r <= 0) break;
		got += (size_t)r;
	}
	return got;
}

void VcVcfText::close()
{
	if (gzp_) vc_gzp_close(gzp_);
	if (gz_) gzclose(gz_);
	if (fp_) fclose(fp_);
	gzp_ = nullptr;
	gz_ = nullptr;
	fp_ = nullptr;
}

extern "C" int vc_vcf_header_parse(const uint8_t *text, size_t len, int final, vc_vcf_header **out, size_t *body_off)
{
	if (!out || (len && !text)) return VC_EINVAL;
	*out = nullptr;
	if (body_off) *body_off = 0;
	// hts_open takes the file for VCF by these 16 bytes (hts.c hts_detect_format)
	if (len < 16) {
		if (!final && (len == 0 || memcmp(text, "##fileformat=VCF", len) == 0)) return VC_VCF_MORE;
		return VC_EINVAL;
	}
	if (memcmp(text, "##fileformat=VCF", 16) != 0) return VC_EINVAL;
	vc_vcf_header *h = new (std::nothrow) vc_vcf_header;
	if (!h) return VC_ENOMEM;
	size_t p = 0;
	for (;;) {
		if (p >= len) {   // vcf_hdr_read ran out of lines: no sample line
			delete h;
			return final ? VC_EINVAL : VC_VCF_MORE;
		}
		const uint8_t *nl = (const uint8_t *)memchr(text + p, '\n', len - p);
		if (!nl && !final) {
			delete h;
			return VC_VCF_MORE;
		}
		size_t end = nl ? (size_t)(nl - text) : len;
		const size_t next = nl ? end + 1 : len;
		if (end > p && text[end - 1] == '\r') --end;
		if (end == p) {   // empty lines of the header are passed over (vcf.c:2290)
			p = next;
			continue;
		}
		if (text[p] != '#') {   // "No sample line"
			delete h;
			return VC_EINVAL;
		}
		const std::string line((const char *)text + p, end - p);
		if (line.size() > 1 && line[1] == '#') {
			header_format_line(h, line);
			p = next;
			continue;
		}
		// the sample line (bcf_hdr_parse :1231): samples are the columns behind FORMAT
		if (line.compare(0, 7, "#CHROM\t") != 0 && line.compare(0, 7, "#CHROM ") != 0) {
			delete h;
			return VC_EINVAL;
		}
		int tabs = 0;
		for (char c : line) tabs += c == '\t';
		h->n_samples = tabs >= 9 ? tabs - 8 : 0;
		if (body_off) *body_off = next;
		*out = h;
		return VC_OK;
	}
}

extern "C" int vc_vcf_header_samples(const vc_vcf_header *h) { return h ? h->n_samples : 0; }

extern "C" int vc_vcf_header_type(const vc_vcf_header *h, const char *tag)
{
	if (!h || !tag) return -1;
	const auto it = h->fmt_type.find(tag);
	return it == h->fmt_type.end() ? -1 : it->second;
}

extern "C" void vc_vcf_header_free(vc_vcf_header *h) { delete h; }

extern "C" int vc_vcf_eval_line(const vc_vcf_header *h, const uint8_t *line, size_t len, int sample_idx, int min_depth,
                                vc_vcf_verdict *out)
{
	if (!h || !out || (len && !line)) return VC_EINVAL;
	memset(out, 0, sizeof *out);
	out->verdict = VC_VCF_END;
	if (len && line[len - 1] == '\n') --len;
	if (len && line[len - 1] == '\r') --len;
	if (const void *z = len ? memchr(line, 0, len) : nullptr) len = (size_t)((const uint8_t *)z - line);
	// the line as vcf_parse holds it: NUL-terminated with room behind (vcf.c:3664-3675)
	std::string text((const char *)line, len);
	text.append(4, '\0');
	char *b = &text[0];
	char *const end = b + len;

	// the columns (kstrtok on tabs: tabs + 1 tokens, empty ones included)
	std::vector<char *> col;
	col.push_back(b);
	for (char *p = b; p < end; ++p)
		if (*p == '\t' && col.size() < 10) {   // the sample columns stay one string
			*p = 0;
			col.push_back(p + 1);
		}
	// CHROM, POS (vcf.c:3681-3717)
	// (an empty CHROM is a contig like any other: fix_chromosome adds it, :3686-3696)
	out->chrom_len = (uint32_t)strlen(col[0]);
	if (col.size() < 6) return VC_OK;
	const char *e;
	uint64_t upos;
	if (!str2uint(col[1], &e, 62, &upos) || *e) return VC_OK;
	out->pos = (int64_t)upos - 1;
	out->head_ok = 1;
	// REF, ALT (:3727-3755)
	const char *ref = col[3], *alt = col[4];
	out->ref_len = (uint32_t)strlen(ref);
	out->ref = (uint8_t)ref[0];
	out->n_allele = 1;
	if (!(alt[0] == '.' && alt[1] == 0)) {
		const char *c = alt;
		out->n_allele = 2;
		for (; *c; ++c) out->n_allele += *c == ',';
		const char *first_end = strchr(alt, ',');
		out->alt_len = (uint32_t)(first_end ? first_end - alt : c - alt);
		out->alt = out->alt_len ? (uint8_t)alt[0] : 0;
	} else {
		out->alt_len = 0;
	}
	// QUAL, FILTER, INFO must be there (:3757-3788)
	if (col.size() < 8) return VC_OK;
	out->verdict = VC_VCF_SKIP;
	const int N = h->n_samples;
	if (col.size() == 8 || N == 0) return VC_OK;   // no FORMAT, or no samples: no GT
	// vcf_parse_format
	// a FORMAT column with no sample column is reported but passes (:3349-3350 turn the -1 into 0)
	char *fmt_s = col[8];
	if (col.size() == 9 || (fmt_s[0] == '.' && fmt_s[1] == 0)) return VC_OK;
	std::vector<Fmt> fmt;
	std::vector<std::string> tags;
	{
		char *t = fmt_s;
		for (;;) {
			char *c = t;
			while (*c && *c != ':') ++c;
			const bool last = *c == 0;
			const std::string tag(t, c - t);
			// (an empty tag is an undeclared one: the dummy header line is added, :2863-2880)
			if ((int)fmt.size() >= MAX_N_FMT || tag == ".") {
				out->verdict = VC_VCF_END;
				return VC_OK;
			}
			Fmt f;
			const auto it = h->fmt_type.find(tag);
			f.type = it == h->fmt_type.end() ? HT_STR : it->second;
			f.is_gt = tag == "GT";
			for (const std::string &u : tags) f.dup = f.dup || u == tag;
			tags.push_back(tag);
			fmt.push_back(f);
			if (last) break;
			t = c + 1;
		}
	}
	const int n_fmt = (int)fmt.size();
	// vcf_parse_format_max3: the widths, over the first N sample columns
	char *const q = col[9] - 1;   // the NUL behind FORMAT
	int n_sample = 0;
	{
		char *r = q + 1;
		while (r < end) {
			int j = 0, m = 1, g = 1;
			for (;;) {
				while (*r && *r != '\t' && *r != ',' && *r != '/' && *r != ':' && *r != '|') ++r;
				if (*r == ',') {
					++m;
				} else if (*r == '|' || *r == '/') {
					if (fmt[j].is_gt) ++g;
				} else {
					if (*r == '\t') *r = 0;
					if (fmt[j].max_m < m) fmt[j].max_m = m;
					if (fmt[j].is_gt && fmt[j].max_g < g) fmt[j].max_g = g;
					m = g = 1;
					if (*r == ':') {
						if (++j >= n_fmt) {   // "Incorrect number of FORMAT fields"
							out->verdict = VC_VCF_END;
							return VC_OK;
						}
					} else {
						break;
					}
				}
				if (r >= end) break;
				++r;
			}
			if (++n_sample == N) break;
			++r;
		}
	}
	// vcf_parse_format_alloc4
	for (Fmt &f : fmt) {
		if (!f.max_m) f.max_m = 1;
		if (f.type == HT_FLAG) {   // "The format type 0 ... is currently not supported"
			out->verdict = VC_VCF_END;
			return VC_OK;
		}
		if (f.type == HT_STR) f.width = f.is_gt ? f.max_g : 0;
		else f.width = f.max_m;
		if (!f.dup && (f.is_gt || f.type == HT_INT)) f.val.assign((size_t)n_sample * (size_t)f.width, 0);
	}
	// vcf_parse_format_fill5
	{
		const char *t = q + 1;
		int m = 0;
		while (t < end) {
			if (m == N) break;
			int j = 0;
			while (t < end) {
				Fmt &z = fmt[j++];
				int32_t *x = z.val.empty() ? nullptr : &z.val[(size_t)m * (size_t)z.width];
				if (z.dup) {
					while (*t != ':' && *t) ++t;
				} else if (z.type == HT_STR) {
					if (z.is_gt) {
						uint32_t is_phased = 0, max = 0;
						bool unreadable = false, overflow = false;
						int l = 0;
						for (;; ++t) {
							if (*t == '.') {
								++t;
								if (l < z.width) x[l] = (int32_t)is_phased;
								++l;
							} else {
								const char *tt = t;
								uint32_t val;
								if (*t >= '0' && *t <= '9' && !(t[1] >= '0' && t[1] <= '9')) {
									val = (uint32_t)(*t++ - '0');
								} else {
									// hts_str2uint at 506 bits: up to 152 digits wrap silently
									uint64_t n = 0;
									int digits = 0;
									if (*t == '+') ++t;
									for (; *t >= '0' && *t <= '9'; ++t, ++digits) n = n * 10 + (uint64_t)(*t - '0');
									if (digits > 152) overflow = true;
									val = (uint32_t)n;
									unreadable = unreadable || tt == t;
								}
								if (max < val) max = val;
								if (l < z.width) x[l] = (int32_t)(((val + 1) << 1) | is_phased);
								++l;
							}
							is_phased = *t == '|';
							if (*t != '|' && *t != '/') break;
						}
						if (overflow || max > (uint32_t)(INT32_MAX >> 1) - 1 || unreadable) {
							out->verdict = VC_VCF_END;
							return VC_OK;
						}
						for (; l < z.width; ++l) x[l] = I32_VEND;
					} else {
						while (*t != ':' && *t) ++t;
					}
				} else if (z.type == HT_INT) {
					int l = 0;
					for (;; ++t) {
						int32_t v;
						if (*t == '.') {
							v = I32_MISSING;
							++t;
						} else {
							const char *te;
							int64_t tmp;
							const bool ok = str2int(t, &te, &tmp);
							v = (te == t || !ok || tmp < -2147483640LL || tmp > 2147483647LL) ? I32_MISSING : (int32_t)tmp;
							t = te;
						}
						if (l < z.width) x[l] = v;
						++l;
						if (*t != ',') break;
					}
					for (; l < z.width; ++l) x[l] = I32_VEND;
				} else {   // Float: "." or what strtod takes, comma-separated
					for (;; ++t) {
						if (*t == '.' && !(t[1] >= '0' && t[1] <= '9')) {
							++t;
						} else {
							char *te;
							(void)strtod(t, &te);
							t = te;
						}
						if (*t != ',') break;
					}
				}
				if (*t == 0) break;
				if (*t == ':') {
					++t;
				} else {   // "Invalid character"
					out->verdict = VC_VCF_END;
					return VC_OK;
				}
			}
			for (; j < n_fmt; ++j) {   // trailing fields left out: missing, then padding
				Fmt &z = fmt[j];
				if (z.val.empty() || z.width == 0) continue;
				int32_t *x = &z.val[(size_t)m * (size_t)z.width];
				x[0] = I32_MISSING;
				for (int l = 1; l < z.width; ++l) x[l] = I32_VEND;
			}
			++m;
			++t;
		}
	}
	if (n_sample != N) {   // vcf_parse_format_check7
		out->verdict = VC_VCF_END;
		return VC_OK;
	}

	// process_vcf :137-195
	const Fmt *gt = nullptr, *ad = nullptr, *dp = nullptr;
	for (int j = 0; j < n_fmt; ++j) {
		if (fmt[j].dup) continue;
		if (tags[(size_t)j] == "GT") gt = &fmt[j];
		else if (tags[(size_t)j] == "AD") ad = &fmt[j];
		else if (tags[(size_t)j] == "DP") dp = &fmt[j];
	}
	if (!gt || gt->type != HT_STR) return VC_OK;
	const int64_t ngt = (int64_t)N * gt->width;
	if (gt->width == 0) {   // GT in FORMAT and in no sample column: bcf_get_format_values ends the program
		out->verdict = VC_VCF_ABORT;
		return VC_OK;
	}
	if (sample_idx < 0) return VC_OK;
	const int64_t s = sample_idx;
	if (ngt <= 0 || 2 * s + 1 >= ngt) return VC_OK;
	const int allele1 = (gt->val[(size_t)(2 * s)] >> 1) - 1, allele2 = (gt->val[(size_t)(2 * s + 1)] >> 1) - 1;
	if (allele1 < 0 || allele2 < 0) return VC_OK;
	int32_t depth = 0, ref_depth = 0, alt_depth = 0;
	if (ad && ad->type == HT_INT) {
		const int64_t nad = (int64_t)N * ad->width;
		if (2 * s + 1 < nad && ad->val[(size_t)(2 * s)] != I32_MISSING && ad->val[(size_t)(2 * s + 1)] != I32_MISSING) {
			ref_depth = ad->val[(size_t)(2 * s)];
			alt_depth = ad->val[(size_t)(2 * s + 1)];
			depth = (int32_t)((uint32_t)ref_depth + (uint32_t)alt_depth);
		}
	}
	if (depth == 0 && dp && dp->type == HT_INT) {
		const int64_t ndp = (int64_t)N * dp->width;
		if (s < ndp && dp->val[(size_t)s] != I32_MISSING) {
			depth = dp->val[(size_t)s];
			if (allele1 == 0 && allele2 == 0) {
				ref_depth = depth;
				alt_depth = 0;
			} else if (allele1 == 1 && allele2 == 1) {
				ref_depth = 0;
				alt_depth = depth;
			} else {
				ref_depth = depth / 2;
				alt_depth = depth - ref_depth;
			}
		}
	}
	if (depth < min_depth) return VC_OK;
	out->verdict = VC_VCF_SET;
	out->ref_count = (uint32_t)ref_depth;
	out->alt_count = (uint32_t)alt_depth;
	return VC_OK;
}
