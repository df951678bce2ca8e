// vafc_bam_index.cpp -- the BAI index of a BAM file and the plan a seeking pass
// reads by (vc_bam_index_plan of include/vafc.h, item 9 of the bam contract).
// Host only: no device, no zlib.
//
//   parse   SAM specification 5.2: "BAI\1", n_ref, per reference its bins with
//           their chunks (beg, end as virtual offsets) and its linear index, an
//           optional n_no_coor behind the last reference.  Every count is
//           bounded by the bytes left in the file before it sizes a loop or an
//           allocation; bin 37450 (the metadata pseudo-bin) gives no chunk.
//   plan    per region the bins of [s, e) (reg2bins, 6 levels, 14 bits), of
//           their chunks those that end behind the linear index's entry of
//           window s >> 14, the union sorted by beg and merged while the next
//           span begins in or before the member the current one ends in.
//
// Anything that is not exactly a BAI of the file's n_ref references is "not
// usable for seeking" (VC_BAM_NO_SEEK): the caller reads the whole file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "vafc.h"

namespace {

const uint32_t BAI_META_BIN = 37450;
const int64_t BAI_MAX_POS = (int64_t)1 << 29;   // what 6 levels over 14 bits reach
const size_t BAI_MAX_BYTES = (size_t)1 << 31;   // an index larger than this is not read

struct BaiBin {
	uint32_t bin;
	uint32_t n_chunk;
	size_t first;   // into chunks
};

struct BaiRef {
	std::vector<BaiBin> bins;   // ascending by bin
	std::vector<vc_bam_span> chunks;
	std::vector<uint64_t> linear;
};

struct Cursor {
	const uint8_t *p;
	size_t left;
	bool u32(uint32_t *v)
	{
		if (left < 4) return false;
		*v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
		p += 4, left -= 4;
		return true;
	}
	bool u64(uint64_t *v)
	{
		uint32_t lo, hi;
		if (left < 8 || !u32(&lo) || !u32(&hi)) return false;
		*v = (uint64_t)hi << 32 | lo;
		return true;
	}
};

bool read_all(const char *path, std::vector<uint8_t> &out)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) return false;
	uint8_t buf[65536];
	bool ok = true;
	for (size_t got; (got = fread(buf, 1, sizeof buf, fp)) > 0;) {
		if (out.size() + got > BAI_MAX_BYTES) {
			ok = false;
			break;
		}
		out.insert(out.end(), buf, buf + got);
	}
	ok = ok && !ferror(fp);
	fclose(fp);
	return ok;
}

// The index in `raw` as the references of a file with n_ref of them.
bool bai_parse(const std::vector<uint8_t> &raw, int32_t n_ref, std::vector<BaiRef> &refs)
{
	Cursor c{raw.data(), raw.size()};
	uint32_t n = 0;
	if (c.left < 8 || memcmp(c.p, "BAI\1", 4) != 0) return false;   // CSI comes as BGZF: no seeking by it
	c.p += 4, c.left -= 4;
	if (!c.u32(&n) || n != (uint32_t)n_ref || n > c.left / 8) return false;
	// the lists grow as their elements parse: a count alone sizes nothing
	refs.clear();
	for (uint32_t t = 0; t < n; ++t) {
		refs.emplace_back();
		BaiRef &r = refs.back();
		uint32_t n_bin = 0, n_intv = 0;
		if (!c.u32(&n_bin) || n_bin > c.left / 8) return false;
		for (uint32_t b = 0; b < n_bin; ++b) {
			BaiBin bin;
			if (!c.u32(&bin.bin) || !c.u32(&bin.n_chunk) || bin.n_chunk > c.left / 16) return false;
			bin.first = r.chunks.size();
			for (uint32_t k = 0; k < bin.n_chunk; ++k) {
				vc_bam_span s;
				if (!c.u64(&s.beg) || !c.u64(&s.end)) return false;
				if (bin.bin == BAI_META_BIN) continue;   // two pairs of numbers, no file offsets
				if (s.end < s.beg) return false;
				r.chunks.push_back(s);
			}
			if (bin.bin == BAI_META_BIN) continue;
			r.bins.push_back(bin);
		}
		std::sort(r.bins.begin(), r.bins.end(), [](const BaiBin &a, const BaiBin &b) { return a.bin < b.bin; });
		for (size_t i = 1; i < r.bins.size(); ++i)
			if (r.bins[i].bin == r.bins[i - 1].bin) return false;
		if (!c.u32(&n_intv) || n_intv > c.left / 8) return false;
		r.linear.resize(n_intv);   // n_intv * 8 bytes are there
		for (uint64_t &v : r.linear)
			if (!c.u64(&v)) return false;
	}
	return c.left == 0 || c.left == 8;   // n_no_coor or nothing
}

// The chunks of bin `b` that end behind min_off.
void take_bin(const BaiRef &r, uint32_t b, uint64_t min_off, std::vector<vc_bam_span> &out)
{
	const auto it = std::lower_bound(r.bins.begin(), r.bins.end(), b, [](const BaiBin &x, uint32_t v) { return x.bin < v; });
	if (it == r.bins.end() || it->bin != b) return;
	for (uint32_t k = 0; k < it->n_chunk; ++k) {
		const vc_bam_span &s = r.chunks[it->first + k];
		if (s.end > min_off) out.push_back(s);
	}
}

// The plan by the index bytes in raw; VC_OK and the spans in `all`, VC_BAM_NO_SEEK.
int plan_bytes(const std::vector<uint8_t> &raw, int32_t n_ref, const int32_t *tid, const int32_t *start, const int32_t *end,
               size_t n, std::vector<vc_bam_span> &all)
{
	std::vector<BaiRef> refs;
	if (!bai_parse(raw, n_ref, refs)) return VC_BAM_NO_SEEK;
	for (size_t i = 0; i < n; ++i) {
		if ((int64_t)end[i] > BAI_MAX_POS) return VC_BAM_NO_SEEK;   // past what a BAI's bins can say
		const BaiRef &r = refs[(size_t)tid[i]];
		const uint32_t s = (uint32_t)start[i], e = (uint32_t)end[i] - 1, win = s >> 14;
		const uint64_t min_off = win < r.linear.size() ? r.linear[win] : 0;
		take_bin(r, 0, min_off, all);
		const uint32_t base[5] = {1, 9, 73, 585, 4681};
		for (int l = 0; l < 5; ++l) {
			const int shift = 26 - 3 * l;
			for (uint32_t b = base[l] + (s >> shift); b <= base[l] + (e >> shift); ++b) take_bin(r, b, min_off, all);
		}
	}
	std::sort(all.begin(), all.end(), [](const vc_bam_span &a, const vc_bam_span &b) {
		return a.beg != b.beg ? a.beg < b.beg : a.end < b.end;
	});
	size_t m = 0;
	for (size_t i = 0; i < all.size(); ++i) {
		if (m && (all[i].beg >> 16) <= (all[m - 1].end >> 16)) {
			if (all[i].end > all[m - 1].end) all[m - 1].end = all[i].end;
		} else {
			all[m++] = all[i];
		}
	}
	all.resize(m);
	return VC_OK;
}

} // namespace

extern "C" int vc_bam_index_plan(const char *bam_path, const char *index_path, int32_t n_ref, const int32_t *tid,
                                 const int32_t *start, const int32_t *end, size_t n, vc_bam_span **spans, size_t *n_spans)
{
	if (!spans || !n_spans) return VC_EINVAL;
	*spans = nullptr;
	*n_spans = 0;
	if ((!bam_path && !index_path) || n_ref < 0 || (n && (!tid || !start || !end))) return VC_EINVAL;
	for (size_t i = 0; i < n; ++i)
		if (tid[i] < 0 || tid[i] >= n_ref || start[i] < 0 || start[i] >= end[i]) return VC_EINVAL;
	char found[4096];
	if (!index_path) {
		if (!vc_bam_index_usable(bam_path, found, sizeof found)) return VC_BAM_NO_SEEK;
		index_path = found;
	}
	std::vector<vc_bam_span> all;
	try {
		std::vector<uint8_t> raw;
		if (!read_all(index_path, raw)) return VC_BAM_NO_SEEK;
		const int rc = plan_bytes(raw, n_ref, tid, start, end, n, all);
		if (rc != VC_OK) return rc;
	} catch (const std::bad_alloc &) {
		return VC_ENOMEM;
	}
	if (all.empty()) return VC_OK;
	vc_bam_span *out = (vc_bam_span *)malloc(all.size() * sizeof(vc_bam_span));
	if (!out) return VC_ENOMEM;
	memcpy(out, all.data(), all.size() * sizeof(vc_bam_span));
	*spans = out;
	*n_spans = all.size();
	return VC_OK;
}

extern "C" void vc_bam_index_plan_free(vc_bam_span *spans) { free(spans); }
