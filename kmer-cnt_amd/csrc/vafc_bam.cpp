// vafc_bam.cpp -- host reader of BGZF-compressed BAM (vafc_bam.h) and the
// host-only entries of the vc_bam_* family (include/vafc.h): probe, reader,
// index rule, build_regions.  No HIP here.
//
// BGZF is a sequence of independent gzip members that carry their own size in
// a BC extra field, so the parallel cut is given: a group of blocks is read,
// its members' ISIZE words give every block's place in the group's text, and
// worker threads inflate them side by side (raw inflate, CRC-32 and ISIZE
// checked per block, vafc_bgzf_io.h).  The next group is loaded while this one is parsed.
#include "vafc_bam.h"
#include "vafc_bgzf_io.h"

#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <thread>

static const size_t BGZF_GROUP_BLOCKS = 256;   // blocks inflated side by side (up to 16 MB of text)

bool VcBgzf::open(const char *path, int n_threads)
{
	close();
	fp_ = fopen(path, "rb");
	if (!fp_) return false;
	threads_ = n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads);
	have_cur_ = false;
	cur_ = 0;
	pos_ = 0;
	carry_.clear();
	members_ = 0;
	return true;
}

void VcBgzf::close()
{
	if (pending_valid_) pending_.get();
	pending_valid_ = false;
	if (fp_) fclose(fp_);
	fp_ = nullptr;
}

void VcBgzf::load(VcBgzfGroup *g)
{
	g->boff.assign(1, 0);
	g->toff.assign(1, 0);
	g->text_len = 0;
	g->last = false;
	std::vector<VcBgzfMember> mem;
	while (mem.size() < BGZF_GROUP_BLOCKS) {
		// raw only grows: the blocks end at boff[n], not at its size
		const size_t at = g->boff.back();
		if (g->raw.size() < at + VC_BGZF_MAX_MEMBER) g->raw.resize(at + VC_BGZF_MAX_MEMBER);
		VcBgzfMember m;
		if (vc_bgzf_read_member(fp_, g->raw.data() + at, &m) <= 0) {   // (an ISIZE no BGZF block can hold among them)
			g->last = true;
			break;
		}
		mem.push_back(m);
		g->boff.push_back((uint32_t)(at + m.size));
		g->toff.push_back(g->toff.back() + m.isize);
	}
	const size_t n = mem.size();
	if (g->text.size() < g->toff[n] + 1) g->text.resize(g->toff[n] + 1);
	std::vector<uint8_t> ok(n, 0);
	std::atomic<size_t> next(0);
	auto work = [&]() {
		for (size_t i; (i = next.fetch_add(1)) < n;)
			ok[i] = vc_bgzf_inflate_member(g->raw.data() + g->boff[i], mem[i], g->text.data() + g->toff[i]);
	};
	const size_t nt = std::min<size_t>((size_t)threads_, n);
	std::vector<std::thread> pool;
	for (size_t t = 1; t < nt; ++t) pool.emplace_back(work);
	work();
	for (std::thread &t : pool) t.join();
	size_t good = 0;
	while (good < n && ok[good]) ++good;
	if (good < n) g->last = true;
	g->text_len = g->toff[good];
	members_ += good;
}

bool VcBgzf::advance()
{
	if (!fp_) return false;
	if (have_cur_) {
		if (grp_[cur_].last) return false;
		pending_.get();
		pending_valid_ = false;
		cur_ ^= 1;
	} else {
		load(&grp_[cur_]);
		have_cur_ = true;
	}
	pos_ = 0;
	if (!grp_[cur_].last) {
		VcBgzfGroup *nx = &grp_[cur_ ^ 1];
		pending_ = std::async(std::launch::async, [this, nx]() { load(nx); });
		pending_valid_ = true;
	}
	return true;
}

const uint8_t *VcBgzf::take(size_t n)
{
	carry_.clear();
	if (!have_cur_ && !advance()) return nullptr;
	{
		VcBgzfGroup &g = grp_[cur_];
		if (g.text_len - pos_ >= n) {
			const uint8_t *p = g.text.data() + pos_;
			pos_ += n;
			return p;
		}
		carry_.assign(g.text.data() + pos_, g.text.data() + g.text_len);
		pos_ = g.text_len;
	}
	while (carry_.size() < n) {
		if (!advance()) return nullptr;
		VcBgzfGroup &g = grp_[cur_];
		const size_t m = std::min(n - carry_.size(), g.text_len);
		carry_.insert(carry_.end(), g.text.data(), g.text.data() + m);
		pos_ = m;
	}
	return carry_.data();
}

// ---------------------------------------------------------------------------

extern "C" const char *vc_bam_kind_name(int kind)
{
	switch (kind) {
	case VC_BAM_BGZF: return "BGZF-compressed BAM";
	case VC_BAM_SAM: return "SAM text (or an unknown format)";
	case VC_BAM_CRAM: return "CRAM";
	case VC_BAM_RAW: return "uncompressed BAM";
	case VC_BAM_GZIP: return "gzip data that is not BGZF";
	case VC_BAM_BGZF_OTHER: return "BGZF data that is not BAM";
	}
	return "?";
}

namespace {

// The text of the first BGZF member of a file (empty: none that inflates);
// *read: whether it is one (vc_bgzf_read_member).
std::vector<uint8_t> first_member_text(FILE *fp, int *read = nullptr)
{
	std::vector<uint8_t> raw(VC_BGZF_MAX_MEMBER), text;
	VcBgzfMember m;
	const int r = vc_bgzf_read_member(fp, raw.data(), &m);
	if (read) *read = r;
	if (r != 1) return text;
	text.resize(m.isize + 1);
	if (!vc_bgzf_inflate_member(raw.data(), m, text.data())) return std::vector<uint8_t>();
	text.resize(m.isize);
	return text;
}

} // namespace

extern "C" int vc_bam_probe(const char *path, int *kind)
{
	if (!path || !kind) return VC_EINVAL;
	FILE *fp = fopen(path, "rb");
	if (!fp) return VC_EIO;
	uint8_t h[12] = {0};
	const size_t got = fread(h, 1, 12, fp);
	if (got >= 4 && memcmp(h, "CRAM", 4) == 0) *kind = VC_BAM_CRAM;
	else if (got >= 4 && memcmp(h, "BAM\1", 4) == 0) *kind = VC_BAM_RAW;
	else if (got >= 2 && h[0] == 31 && h[1] == 139) {
		rewind(fp);
		int read = 0;
		const std::vector<uint8_t> text = first_member_text(fp, &read);
		// a BGZF header that is cut short still names BGZF; anything else is plain gzip
		if (read < 0) *kind = got == 12 && h[2] == 8 && (h[3] & 4) && vc_le16(h + 10) >= 6 ? VC_BAM_BGZF : VC_BAM_GZIP;
		// a first block that does not inflate is a header that cannot be read
		else *kind = text.size() >= 4 && memcmp(text.data(), "BAM\1", 4) != 0 ? VC_BAM_BGZF_OTHER : VC_BAM_BGZF;
	} else {
		*kind = VC_BAM_SAM;
	}
	fclose(fp);
	return VC_OK;
}

int VcBamReader::open(const char *path, int n_threads)
{
	header_ok_ = ended_ = false;
	refs_.clear();
	bases = records = 0;
	int kind = 0;
	const int rc = vc_bam_probe(path, &kind);
	if (rc != VC_OK) return rc;
	if (kind != VC_BAM_BGZF) {
		fprintf(stderr, "[E::vafc] %s is %s: only BGZF-compressed BAM is read\n", path, vc_bam_kind_name(kind));
		return VC_EINVAL;
	}
	if (!z_.open(path, n_threads)) return VC_EIO;
	ended_ = true;
	const uint8_t *p = z_.take(8);
	if (!p || memcmp(p, "BAM\1", 4) != 0) return VC_EINVAL;
	const int32_t l_text = (int32_t)vc_le32(p + 4);
	if (l_text < 0 || !z_.take((size_t)l_text) || !(p = z_.take(4))) return VC_EINVAL;
	const int32_t n_ref = (int32_t)vc_le32(p);
	if (n_ref < 0) return VC_EINVAL;
	for (int32_t i = 0; i < n_ref; ++i) {
		if (!(p = z_.take(4))) return VC_EINVAL;
		const int32_t l_name = (int32_t)vc_le32(p);
		if (l_name < 1 || !(p = z_.take((size_t)l_name))) return VC_EINVAL;
		refs_.emplace_back((const char *)p, strnlen((const char *)p, (size_t)l_name));
		if (!z_.take(4)) return VC_EINVAL;
	}
	header_ok_ = true;
	ended_ = false;
	in_batch_ = empty_batches_ = 0;
	return VC_OK;
}

namespace {

// The CG:B,I array of a record's aux fields [a, e): its words and count.
// 0 = no such tag, 1 = found, -1 = malformed aux data before it.
int find_cg(const uint8_t *a, const uint8_t *e, const uint8_t **words, uint32_t *n_words)
{
	while (a < e) {
		if (e - a < 3) return -1;
		const bool cg = a[0] == 'C' && a[1] == 'G';
		const uint8_t type = a[2];
		a += 3;
		size_t size;
		switch (type) {
		case 'A': case 'c': case 'C': size = 1; break;
		case 's': case 'S': size = 2; break;
		case 'i': case 'I': case 'f': size = 4; break;
		case 'd': size = 8; break;
		case 'Z': case 'H': {
			const void *nul = memchr(a, 0, (size_t)(e - a));
			if (!nul) return -1;
			size = (size_t)((const uint8_t *)nul - a) + 1;
			break;
		}
		case 'B': {
			if (e - a < 5) return -1;
			size_t el;
			switch (a[0]) {
			case 'c': case 'C': el = 1; break;
			case 's': case 'S': el = 2; break;
			case 'i': case 'I': case 'f': el = 4; break;
			default: return -1;
			}
			const uint64_t cnt = vc_le32(a + 1);
			if (cnt * el > (uint64_t)(e - a - 5)) return -1;
			if (cg) {
				if (a[0] != 'I' && a[0] != 'i') return 0;
				*words = a + 5;
				*n_words = (uint32_t)cnt;
				return 1;
			}
			size = 5 + (size_t)(cnt * el);
			break;
		}
		default: return -1;
		}
		if (size > (size_t)(e - a)) return -1;
		if (cg) return 0;   // a CG tag of another type leaves the CIGAR alone
		a += size;
	}
	return 0;
}

} // namespace

bool VcBamReader::next_batch(std::vector<vc_bam_rec> &recs, std::vector<uint8_t> &data, size_t max_bytes, size_t max_recs)
{
	const size_t n0 = recs.size();
	// a record-level failure (item 7): the reference's batch closes there, and
	// the second batch of a file that closes empty ends it; otherwise reading
	// goes on after the bytes consumed so far
	auto soft_fail = [this]() {
		if (in_batch_ == 0 && ++empty_batches_ == 2) ended_ = true;
		in_batch_ = 0;
	};
	while (!ended_) {
		if (recs.size() > n0 && (data.size() >= max_bytes || recs.size() - n0 >= max_recs)) return true;
		const uint8_t *p = z_.take(4);
		if (!p) {
			ended_ = true;
			break;
		}
		const int32_t bl = (int32_t)vc_le32(p);
		if (bl < 32) {
			soft_fail();
			continue;
		}
		if (!(p = z_.take(32))) {
			ended_ = true;
			break;
		}
		vc_bam_rec r;
		r.tid = (int32_t)vc_le32(p);
		r.pos = (int32_t)vc_le32(p + 4);
		const uint32_t l_qname = p[8];
		r.n_cigar = vc_le16(p + 12);
		r.flag = vc_le16(p + 14);
		r.l_seq = vc_le32(p + 16);
		r.reserved = 0;
		const uint64_t seq_bytes = ((uint64_t)r.l_seq + 1) >> 1;
		if ((int32_t)r.l_seq < 0 || l_qname < 1 ||
		    ((uint64_t)r.n_cigar << 2) + l_qname + seq_bytes + r.l_seq > (uint64_t)bl - 32) {
			soft_fail();   // the 36 bytes read so far are gone
			continue;
		}
		const size_t body = (size_t)bl - 32;
		if (!(p = z_.take(body))) {
			ended_ = true;
			break;
		}
		const uint8_t *cigar = p + l_qname, *seq = cigar + 4 * (size_t)r.n_cigar;
		// the long-CIGAR convention (sam.c bam_tag2cigar): <l_seq>S<N>N plus CG:B,I
		if (r.n_cigar > 0 && vc_le32(cigar) == (r.l_seq << 4 | 4u) && r.tid >= 0 && r.pos >= 0) {
			const uint8_t *words = nullptr;
			uint32_t n_words = 0;
			const int f = find_cg(seq + seq_bytes + r.l_seq, p + body, &words, &n_words);
			if (f < 0) {
				soft_fail();
				continue;
			}
			if (f == 1 && n_words >= r.n_cigar && n_words < (1u << 29)) {
				cigar = words;
				r.n_cigar = n_words;
			}
		}
		if (r.n_cigar > 0) {
			uint64_t qlen = 0;
			for (uint32_t k = 0; k < r.n_cigar; ++k) {
				const uint32_t c = vc_le32(cigar + 4 * (size_t)k), op = c & 15;
				if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += c >> 4;
			}
			if (r.l_seq > 0 && !(r.flag & 4u) && qlen != r.l_seq) {
				soft_fail();
				continue;
			}
		}
		r.off = data.size();
		const size_t cb = 4 * (size_t)r.n_cigar, total = (cb + (size_t)seq_bytes + 3) & ~(size_t)3;
		data.resize(data.size() + total, 0);
		if (cb) memcpy(data.data() + r.off, cigar, cb);
		if (seq_bytes) memcpy(data.data() + r.off + cb, seq, (size_t)seq_bytes);
		recs.push_back(r);
		bases += r.l_seq;
		++records;
		if (++in_batch_ == 1000) in_batch_ = 0;   // the reference's batch_size (bam-vaf-counter.c:328)
	}
	return recs.size() > n0;
}

// ---------------------------------------------------------------------------

struct vc_bam_file {
	std::vector<std::string> refs;
	std::vector<vc_bam_rec> recs;
	std::vector<uint8_t> data;
};

extern "C" int vc_bam_read_file(const char *path, int n_threads, vc_bam_file **out)
{
	if (!path || !out) return VC_EINVAL;
	*out = nullptr;
	VcBamReader rd;
	const int rc = rd.open(path, n_threads);
	if (rc == VC_EIO) return rc;
	vc_bam_file *f = new (std::nothrow) vc_bam_file;
	if (!f) return VC_ENOMEM;
	*out = f;
	if (rc != VC_OK) return rc;
	f->refs = rd.refs();
	while (rd.next_batch(f->recs, f->data, ~(size_t)0, (size_t)1 << 20)) {
	}
	return VC_OK;
}

extern "C" int vc_bam_read_header(const char *path, vc_bam_file **out)
{
	if (!path || !out) return VC_EINVAL;
	*out = nullptr;
	VcBamReader rd;
	const int rc = rd.open(path, 1);
	if (rc == VC_EIO) return rc;
	vc_bam_file *f = new (std::nothrow) vc_bam_file;
	if (!f) return VC_ENOMEM;
	*out = f;
	if (rc == VC_OK) f->refs = rd.refs();
	return rc;
}

extern "C" int vc_bam_file_refs(const vc_bam_file *f) { return f ? (int)f->refs.size() : 0; }

extern "C" const char *vc_bam_file_ref_name(const vc_bam_file *f, int i)
{
	return f && i >= 0 && (size_t)i < f->refs.size() ? f->refs[(size_t)i].c_str() : nullptr;
}

extern "C" uint64_t vc_bam_file_records(const vc_bam_file *f, const vc_bam_rec **recs, const uint8_t **data,
                                        uint64_t *data_bytes)
{
	if (!f) return 0;
	if (recs) *recs = f->recs.data();
	if (data) *data = f->data.data();
	if (data_bytes) *data_bytes = f->data.size();
	return f->recs.size();
}

extern "C" void vc_bam_file_free(vc_bam_file *f) { delete f; }

extern "C" int vc_bam_index_usable(const char *path, char *buf, size_t buf_len)
{
	if (buf && buf_len) buf[0] = '\0';
	if (!path) return 0;
	// hts_idx_check_local: fn.csi, fn-minus-extension.csi, fn.bai, fn-minus-extension.bai;
	// the first that exists is the index, usable or not
	const std::string fn(path);
	std::string stem;
	for (size_t i = fn.size(); i-- > 1;)
		if (fn[i] == '.') {
			stem = fn.substr(0, i);
			break;
		}
	std::vector<std::string> cand;
	cand.push_back(fn + ".csi");
	if (!stem.empty()) cand.push_back(stem + ".csi");
	cand.push_back(fn + ".bai");
	if (!stem.empty()) cand.push_back(stem + ".bai");
	for (const std::string &c : cand) {
		struct stat sb;
		if (stat(c.c_str(), &sb) != 0) continue;
		if (buf && buf_len) snprintf(buf, buf_len, "%s", c.c_str());
		FILE *fp = fopen(c.c_str(), "rb");
		if (!fp) return 0;
		uint8_t h[4] = {0};
		const size_t got = fread(h, 1, 4, fp);
		int ok = got == 4 && memcmp(h, "BAI\1", 4) == 0;
		if (!ok && got == 4 && h[0] == 31 && h[1] == 139) {
			rewind(fp);
			const std::vector<uint8_t> text = first_member_text(fp);
			ok = text.size() >= 4 && memcmp(text.data(), "CSI\1", 4) == 0;
		}
		fclose(fp);
		return ok;
	}
	return 0;
}

extern "C" int vc_bam_build_regions(const vc_patterns *db, int32_t *first_row, int32_t *ends)
{
	if (!db || !first_row || !ends) return 0;
	const int n = vc_patterns_count(db);
	if (n <= 0) return 0;
	struct Row {
		const char *chr;
		int start, idx;
	};
	std::vector<Row> rows((size_t)n);
	for (int i = 0; i < n; ++i) {
		rows[(size_t)i].idx = i;
		if (vc_pattern_fields(db, i, &rows[(size_t)i].chr, &rows[(size_t)i].start, nullptr, nullptr, nullptr, nullptr,
		                      nullptr) != VC_OK)
			return 0;
	}
	std::stable_sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
		const int c = strcmp(a.chr, b.chr);
		return c != 0 ? c < 0 : a.start < b.start;
	});
	int w = 0;
	first_row[0] = rows[0].idx;
	ends[0] = (int32_t)((uint32_t)rows[0].start + 1u);
	for (int i = 1; i < n; ++i) {
		const Row &r = rows[(size_t)i];
		const int32_t end = (int32_t)((uint32_t)r.start + 1u);
		if (strcmp(rows[(size_t)w].chr, r.chr) == 0 && ends[w] >= r.start) {
			if (end > ends[w]) ends[w] = end;
		} else {
			++w;
			rows[(size_t)w] = r;
			first_row[w] = r.idx;
			ends[w] = end;
		}
	}
	return w + 1;
}
