// vafc_vcf_files.cpp -- the file passes of vcf-vaf-counter (process_vcf,
// vcf-vaf-counter.c): vc_vcf_count_file and vc_vcf_inflate_info.  A pass reads
// the header (read_header), then cuts the text into blocks, has each scanned
// and evaluates the lines the scan reports (walk_blocks).  Where the text comes
// from is the pass's source: HostText (plain and gzip input, and BGZF inflated
// on the host) or ZText (BGZF inflated on the device).  The kernels are
// reached through vc_vcf_scan_block and vc_vcf_scan_device (vafc_vcf.hip).
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "vafc_bgzf_io.h"
#include "vafc_vcf.h"
#include "vafc_vcf_ctx.h"

namespace {

// BGZF input without $VAFC_BGZF: inflated on the device (DESIGN 15 has the measurement that decided it)
const bool VCF_BGZF_DEFAULT_DEVICE = true;

// The lines a scan reported, in file order, under items 2-8: `text` holds the
// scanned block from its byte `base` on, up to `consumed`; set(row, ref, alt)
// receives item 7's assignments.  VC_OK (ended: a line ended the file), an
// error of vc_vcf_eval_line, or VC_VCF_ABORTED.
template <class Set>
int eval_hits(vc_vcf *c, const vc_vcf_header *hdr, const uint8_t *text, size_t base, size_t consumed, uint64_t file_off,
              const vc_vcf_hit *hits, size_t n_hits, int sample_idx, int min_depth, bool &ended, Set &&set)
{
	int rc = VC_OK;
	const uint8_t *block = text - base;   // only bytes [base, consumed) of it are read
	for (size_t i = 0; i < n_hits && !ended; ++i) {
		const size_t lo = (size_t)(hits[i].off - file_off);
		const uint8_t *nl = (const uint8_t *)memchr(block + lo, '\n', consumed - lo);
		const size_t len = nl ? (size_t)(nl - block) - lo : consumed - lo;
		vc_vcf_verdict v;
		if ((rc = vc_vcf_eval_line(hdr, block + lo, len, sample_idx, min_depth, &v)) != VC_OK) break;
		int64_t row = hits[i].row;
		if (row < 0) {
			if (!v.head_ok) {   // item 8: the file ends here
				ended = true;
				break;
			}
			// a line after all: matched here (items 2 and 3)
			const auto it = c->first_row.find(vcf_host_key((const char *)block + lo, v.chrom_len, (int32_t)(uint32_t)(uint64_t)v.pos));
			if (it == c->first_row.end()) continue;
			if (v.n_allele != 2 || v.ref_len != 1 || v.alt_len != 1 ||
			    c->row_ra[it->second] != (uint16_t)(v.ref | (uint16_t)v.alt << 8))
				continue;
			row = it->second;
		}
		if (v.verdict == VC_VCF_ABORT) {   // item 8: the reference's process ends here
			rc = VC_VCF_ABORTED;
			break;
		}
		if (v.verdict == VC_VCF_END) ended = true;
		else if (v.verdict == VC_VCF_SET) set((size_t)row, v.ref_count, v.alt_count);
	}
	return rc;
}

// The header: src.more appends text to buf (end: there is no more) until the
// #CHROM line is whole.  VC_OK, an error of src.more, or VC_EINVAL.
template <class Src> int read_header(Src &src, std::vector<uint8_t> &buf, vc_vcf_header **hdr, size_t *body)
{
	for (;;) {
		bool end = false;
		int rc = src.more(buf, end);
		if (rc != VC_OK) return rc;
		rc = vc_vcf_header_parse(buf.data(), buf.size(), end, hdr, body);
		if (rc == VC_OK) return VC_OK;
		if (rc != VC_VCF_MORE || end) return VC_EINVAL;
	}
}

// The data lines, from file offset file_off on, in blocks: up to cap bytes
// from a line start, a shorter one only at the end of the file (final); one
// without a '\n' is a line longer than the block, which grows.  The source
// gives a block (next; none: the text has ended), has it scanned (scan: the
// reported lines and the bytes up to the last '\n'), brings the bytes from
// the first reported line on to the host (lines), takes item 7's assignments
// (set) and is told how far the text is done with (consume).
template <class Src>
int walk_blocks(vc_vcf *c, const vc_vcf_header *hdr, Src &src, uint64_t file_off, int sample_idx, int min_depth, vc_file_stats &st)
{
	st.bases = file_off;
	int rc = VC_OK;
	bool ended = false;
	size_t cap = c->block_bytes;
	while (!ended) {
		const uint8_t *block = nullptr, *text = nullptr;
		size_t blen = 0, n_hits = 0, consumed = 0;
		bool final = false;
		if ((rc = src.next(cap, &block, &blen, &final)) != VC_OK || blen == 0) break;
		const vc_vcf_hit *hits = nullptr;
		if ((rc = src.scan(block, blen, file_off, final, &hits, &n_hits, &consumed)) != VC_OK) break;
		if (consumed == 0 && !final) {   // no '\n': a line longer than the block
			cap *= 2;
			continue;
		}
		++st.blocks;
		st.seqs += n_hits;
		if (n_hits) {
			const size_t lo = (size_t)(hits[0].off - file_off);
			if ((rc = src.lines(block, lo, consumed, &text)) != VC_OK) break;
			rc = eval_hits(c, hdr, text, lo, consumed, file_off, hits, n_hits, sample_idx, min_depth, ended,
			               [&](size_t row, uint32_t ref, uint32_t alt) { src.set(row, ref, alt); });
			if (rc != VC_OK) break;
		}
		st.bases += consumed;
		file_off += consumed;
		src.consume(consumed);
	}
	return rc;
}

// The text inflated (or read) on the host; the blocks go through the stager.
struct HostText {
	vc_vcf *c;
	uint32_t *counts;
	VcVcfText in;
	std::vector<uint8_t> text;   // what is read and not yet consumed: text[head ..)
	size_t head = 0;
	bool eof = false;

	// up to `want` more bytes of the text behind v
	void fill(std::vector<uint8_t> &v, size_t want)
	{
		const size_t at = v.size();
		v.resize(at + want);
		v.resize(at + in.read(v.data() + at, want));
		eof = v.size() - at < want;
	}
	int more(std::vector<uint8_t> &buf, bool &end) { return fill(buf, (size_t)1 << 16), end = eof, VC_OK; }
	int next(size_t cap, const uint8_t **block, size_t *blen, bool *final)
	{
		if (head && (head >= text.size() / 2 || eof)) {
			text.erase(text.begin(), text.begin() + (ptrdiff_t)head);
			head = 0;
		}
		while (!eof && text.size() - head < cap) fill(text, cap - (text.size() - head));
		*blen = std::min(text.size() - head, cap);
		*final = eof && *blen == text.size() - head;
		*block = text.data() + head;
		return VC_OK;
	}
	int scan(const uint8_t *block, size_t blen, uint64_t file_off, bool final, const vc_vcf_hit **hits, size_t *n_hits,
	         size_t *consumed)
	{
		const int rc = vc_vcf_scan_block(c, block, blen, file_off, final ? 1 : 0, consumed);
		return rc != VC_OK ? rc : vc_vcf_hits(c, hits, n_hits, nullptr);
	}
	int lines(const uint8_t *block, size_t lo, size_t, const uint8_t **at) { return *at = block + lo, VC_OK; }
	void set(size_t row, uint32_t ref, uint32_t alt) { counts[2 * row] = ref, counts[2 * row + 1] = alt; }
	void consume(size_t n) { head += n; }
};

int count_host(vc_vcf *c, const char *path, int kind, int sample_idx, int min_depth, int n_threads, uint32_t *counts,
               vc_file_stats &st)
{
	HostText src{c, counts};
	if (src.in.open(path, kind, n_threads) != VC_OK) {
		fprintf(stderr, "Error: failed to open VCF file: %s\n", path);
		return VC_EIO;
	}
	std::vector<uint8_t> buf;
	vc_vcf_header *hdr = nullptr;
	size_t body = 0;
	if (read_header(src, buf, &hdr, &body) != VC_OK) {
		fprintf(stderr, "Error: failed to read VCF header\n");
		return VC_EINVAL;
	}
	src.text.assign(buf.begin() + (ptrdiff_t)body, buf.end());
	buf = std::vector<uint8_t>();
	const int rc = walk_blocks(c, hdr, src, body, sample_idx, min_depth, st);
	vc_vcf_header_free(hdr);
	return rc;
}

// ---------------------------------------------------------------------------
// BGZF input inflated on the device.  The header's members are inflated here
// with zlib; from the member that holds the first data line on, pieces of
// whole members are read straight into the stager's pinned slots, copied to
// the device as they are and inflated there by the inflater's kernel
// (vafc_bgzf.hip) on the inflater's stream, into one of two text buffers, while
// the scan of the piece before runs on this handle's stream and its lines are
// evaluated here.  A piece's text lies behind `zhead` free bytes of its buffer;
// the unconsumed tail of the piece before is copied in front of it, so every
// scan starts at a line start and reads one contiguous range.  The lines the
// host evaluates reach it as one D2H copy of the scanned text from the first
// reported line on (none when the scan reports nothing).
//
// VCF_FALLBACK: the file cannot be finished this way (a member whose status
// is not 0, bytes that are no whole member before the end of the file, an
// ISIZE above 65,536).  Nothing has been written to counts or stderr then.
// ---------------------------------------------------------------------------
const int VCF_FALLBACK = 100;
const size_t VCF_ZHEAD = (size_t)1 << 20;         // room in front of a piece's text for the tail before it
const size_t VCF_PIECE_BLOCKS = 65536;            // members of one piece at most

struct ZPiece {
	size_t n_blocks = 0;
	uint64_t text_len = 0;
	bool last = false;        // the file ended behind it
	int buf = 0;              // its text buffer
};

struct ZSet { uint32_t row, ref, alt; };

struct ZText {
	vc_vcf *c;
	FILE *fp;
	hipEvent_t ev;   // on the handle's stream: the copy of a text buffer's tail out of it
	vc_bgzf *zf = c->zf;
	hipStream_t zst = (hipStream_t)vc_bgzf_stream(zf);
	uint64_t host_blocks = 0, device_blocks = 0;
	// the header
	std::vector<uint8_t> mem = std::vector<uint8_t>(VC_BGZF_MAX_MEMBER);
	std::vector<uint64_t> toff = std::vector<uint64_t>(1, 0);   // text offset of each header member
	std::vector<long> foff;                                      // ... and its file offset
	size_t first_skip = 0;   // bytes of the first piece's text in front of the first data line
	// the pieces: piece[k & 1] is scanned, the one after it is on its way once next_started
	ZPiece piece[2];
	int k = -1;
	bool file_ended = false, next_started = false;
	size_t cap = 0;   // of the block asked for last
	// the text to scan: ztext[sb][text_at, +text_len), done with up to pos; final: the file ends behind it
	int sb = 1;
	size_t text_at = 0, text_len = 0, pos = 0;
	bool final = false;
	std::vector<uint8_t> host_lines;
	std::vector<ZSet> sets;   // item 7's assignments, applied once the file is known to be whole

	// the header's members are inflated here
	int more(std::vector<uint8_t> &buf, bool &end)
	{
		const long at = ftell(fp);
		VcBgzfMember m;
		const int r = vc_bgzf_read_member(fp, mem.data(), &m);
		if (r < 0) return VCF_FALLBACK;
		if ((end = r == 0)) return VC_OK;
		const size_t len = buf.size();
		buf.resize(len + m.isize + 1);
		const bool ok = vc_bgzf_inflate_member(mem.data(), m, buf.data() + len);
		buf.resize(len + m.isize);
		if (!ok) return VCF_FALLBACK;
		foff.push_back(at);
		toff.push_back(buf.size());
		++host_blocks;
		return VC_OK;
	}

	// Read the next piece into the stager's slot and send it on its way: H2D and
	// inflate on the inflater's stream, into text buffer b behind its head room.
	int start_piece(ZPiece &p, int b)
	{
		p = ZPiece();
		p.buf = b;
		if (file_ended) {
			p.last = true;
			return VC_OK;
		}
		const size_t raw_room = cap + 65536, max_blocks = std::min(VCF_PIECE_BLOCKS, raw_room / 28 + 1);
		const size_t desc_at = (raw_room + 7) & ~(size_t)7;
		VcSlot *s;
		int rc = c->stage.acquire_for(desc_at + max_blocks * sizeof(vc_bgzf_block), 1, &s);
		if (rc != VC_OK) return rc;
		vc_bgzf_block *desc = reinterpret_cast<vc_bgzf_block *>(s->h_seq + desc_at);
		size_t raw_len = 0;
		while (p.text_len < cap && raw_len + 65536 <= raw_room && p.n_blocks < max_blocks) {
			VcBgzfMember m;
			const int r = vc_bgzf_read_member(fp, s->h_seq + raw_len, &m);
			if (r < 0) return VCF_FALLBACK;
			if (r == 0) {
				file_ended = p.last = true;
				break;
			}
			vc_bgzf_block &d = desc[p.n_blocks++];
			d.in_off = raw_len + m.payload;
			d.in_len = (uint32_t)m.payload_len;
			d.isize = m.isize;
			d.out_off = p.text_len;
			d.crc32 = m.crc32;
			d.reserved = 0;
			p.text_len += m.isize;
			raw_len += m.size;
		}
		if (p.n_blocks == 0) return VC_OK;
		// the text buffer: nobody reads it any more but the copy of its tail, which `ev` follows
		if (c->zhead[b] < VCF_ZHEAD) c->zhead[b] = VCF_ZHEAD;
		if (c->ztext[b].cap < c->zhead[b] + p.text_len) HIPCK(c->ztext[b].grow(c->zhead[b] + (size_t)p.text_len + 65536));
		HIPCK(hipStreamWaitEvent(zst, ev, 0));
		uint8_t *d_text = c->ztext[b] + c->zhead[b];
		const size_t nb = p.n_blocks;
		const uint64_t tl = p.text_len;
		// the descriptors travel with the compressed bytes: one copy of [0, desc_at + n * 32)
		return c->stage.submit(desc_at + nb * sizeof(vc_bgzf_block), 1, zst, [&](const VcSlot &sl) {
			return vc_bgzf_inflate_device(zf, sl.d_seq, raw_len, reinterpret_cast<const vc_bgzf_block *>(sl.d_seq + desc_at), nb,
			                              d_text, (size_t)tl, VC_STREAM_CTX);
		}, false);
	}
	// Whatever is in flight has ended before the buffers are left alone.
	void drain()
	{
		(void)vc_bgzf_finish(zf, nullptr, 0, nullptr, nullptr);
		(void)hipStreamSynchronize(c->st);
		c->stage.settle();
	}

	// The piece after the one in hand becomes the text to scan, behind what is
	// left of that one.
	int next_piece()
	{
		int rc;
		if (!next_started && (rc = start_piece(piece[(k + 1) & 1], sb ^ 1)) != VC_OK) return rc;
		next_started = false;
		// the unconsumed text of the piece before: ztext[tail_buf][tail_at, +tail_len)
		const int tail_buf = sb;
		const size_t tail_at = text_at + pos, tail_len = text_len - pos;
		ZPiece &p = piece[++k & 1];
		const int b = p.buf;
		if (p.n_blocks) {
			size_t n = 0, ok = 0;
			if ((rc = vc_bgzf_finish(zf, nullptr, 0, &n, &ok)) != VC_OK) return rc;
			if (ok != p.n_blocks) return VCF_FALLBACK;
			device_blocks += p.n_blocks;
		} else if (!p.last) {
			return VC_EINVAL;   // (a piece without members is the end of the file)
		}
		if (first_skip > p.text_len) return VCF_FALLBACK;   // cannot be: the header's member is the piece's first
		// the tail before, then this piece (the very first one from the first data line on)
		text_at = c->zhead[b] + first_skip;
		text_len = (size_t)p.text_len - first_skip;
		pos = first_skip = 0;
		if (p.n_blocks == 0) {
			// nothing new: what is left of the piece before (if anything) is the file's last line
			text_at = tail_at;
			text_len = tail_len;
			p.buf = tail_buf;
		} else if (tail_len) {
			if (tail_len > c->zhead[b]) {
				// a tail longer than the room in front of the text: a buffer with more room takes both
				size_t room = c->zhead[b];
				while (room < tail_len) room *= 2;
				VcDevBuf<uint8_t> nb;
				HIPCK(nb.alloc(room + (size_t)p.text_len + 65536));
				HIPCK(hipMemcpyAsync(nb + room, c->ztext[b] + c->zhead[b], (size_t)p.text_len, hipMemcpyDeviceToDevice, c->st));
				HIPCK(hipStreamSynchronize(c->st));
				c->ztext[b] = std::move(nb);
				c->zhead[b] = room;
				text_at = room;
			}
			HIPCK(hipMemcpyAsync(c->ztext[b] + text_at - tail_len, c->ztext[tail_buf] + tail_at, tail_len, hipMemcpyDeviceToDevice,
			                     c->st));
			text_at -= tail_len;
			text_len += tail_len;
		}
		HIPCK(hipEventRecord(ev, c->st));   // the other buffer's tail has left it
		sb = p.buf;
		final = p.last;
		return VC_OK;
	}
	int next(size_t cap_now, const uint8_t **block, size_t *blen, bool *fin)
	{
		cap = cap_now;
		for (int rc; k < 0 || (!final && text_len - pos < cap);)   // the rest waits for the next piece
			if ((rc = next_piece()) != VC_OK) return rc;
		*blen = std::min(text_len - pos, cap);
		*fin = final && pos + *blen == text_len;
		*block = c->ztext[sb] + text_at + pos;
		return VC_OK;
	}
	int scan(const uint8_t *d_text, size_t blen, uint64_t file_off, bool fin, const vc_vcf_hit **hits, size_t *n_hits,
	         size_t *consumed)
	{
		int rc = vc_vcf_scan_device(c, d_text, blen, file_off, fin ? 1 : 0, VC_STREAM_CTX);
		if (rc != VC_OK) return rc;
		// the next piece is read, copied and inflated while this one is scanned and evaluated
		if (!next_started && (rc = start_piece(piece[(k + 1) & 1], sb ^ 1)) != VC_OK) return rc;
		next_started = true;
		return vc_vcf_hits(c, hits, n_hits, consumed);
	}
	int lines(const uint8_t *d_text, size_t lo, size_t consumed, const uint8_t **at)
	{
		host_lines.resize(consumed - lo);
		HIPCK(hipMemcpy(host_lines.data(), d_text + lo, consumed - lo, hipMemcpyDeviceToHost));
		*at = host_lines.data();
		return VC_OK;
	}
	void set(size_t row, uint32_t ref, uint32_t alt) { sets.push_back(ZSet{(uint32_t)row, ref, alt}); }
	void consume(size_t n) { pos += n; }
};

int count_bgzf_device(vc_vcf *c, const char *path, int sample_idx, int min_depth, uint32_t *counts, vc_file_stats &st)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) return VCF_FALLBACK;   // the host pass reports it
	struct Closer {
		FILE *fp;
		vc_vcf_header *hdr = nullptr;
		hipEvent_t ev = nullptr;
		~Closer()
		{
			if (fp) fclose(fp);
			vc_vcf_header_free(hdr);
			if (ev) (void)hipEventDestroy(ev);
		}
	} own{fp};
	HIPCK(hipSetDevice(c->dev));
	int rc;
	if (!c->zf && (rc = vc_bgzf_create(&c->zf, c->dev)) != VC_OK) return rc;
	HIPCK(hipEventCreateWithFlags(&own.ev, hipEventDisableTiming));
	ZText src{c, fp, own.ev};
	std::vector<uint8_t> buf;
	size_t body = 0;
	// (the host pass says why: it sees the same text)
	if (read_header(src, buf, &own.hdr, &body) != VC_OK) return VCF_FALLBACK;
	// the member that holds the first data line; the device starts over with it
	size_t mb = 0;
	while (mb + 1 < src.toff.size() && src.toff[mb + 1] <= body) ++mb;
	src.first_skip = body - (size_t)src.toff[mb];
	if (mb < src.foff.size() && fseek(fp, src.foff[mb], SEEK_SET) != 0) return VCF_FALLBACK;
	buf = std::vector<uint8_t>();
	HIPCK(hipEventRecord(own.ev, c->st));
	rc = walk_blocks(c, own.hdr, src, body, sample_idx, min_depth, st);
	src.drain();
	if (rc == VCF_FALLBACK || (rc != VC_OK && rc != VC_VCF_ABORTED)) return rc;
	for (const ZSet &z : src.sets) {
		counts[2 * (size_t)z.row] = z.ref;
		counts[2 * (size_t)z.row + 1] = z.alt;
	}
	c->z_device_blocks = src.device_blocks;
	c->z_host_blocks = src.host_blocks;
	return rc;
}

// Whole BGZF members of a file, by their headers alone: a member whose body is
// cut counts, for the body is skipped with a seek.
uint64_t count_members(const char *path)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) return 0;
	uint64_t n = 0;
	uint8_t h[VC_BGZF_MAX_MEMBER];
	for (long size; (size = vc_bgzf_read_head(fp, h)) > 0; ++n)
		if (fseek(fp, size - (long)(VC_BGZF_HEAD + vc_bgzf_xlen(h)), SEEK_CUR) != 0) break;
	fclose(fp);
	return n;
}

} // namespace

extern "C" int vc_vcf_inflate_info(const vc_vcf *c, uint64_t *device_blocks, uint64_t *host_blocks)
{
	if (!c) return VC_EINVAL;
	if (device_blocks) *device_blocks = c->z_device_blocks;
	if (host_blocks) *host_blocks = c->z_host_blocks;
	return VC_OK;
}

extern "C" int vc_vcf_count_file(vc_vcf *c, const char *path, int sample_idx, int min_depth, int n_threads, uint32_t *counts,
                                 vc_file_stats *stats)
{
	if (!c || !path || (c->n_rows && !counts)) return VC_EINVAL;
	const double t0 = vc_now();
	vc_file_stats st;
	memset(&st, 0, sizeof st);
	if (stats) *stats = st;
	c->z_device_blocks = c->z_host_blocks = 0;
	int kind = VC_VCF_OTHER;
	if (vc_vcf_probe(path, &kind) != VC_OK) {
		fprintf(stderr, "Error: failed to open VCF file: %s\n", path);
		return VC_EIO;
	}
	if (kind == VC_VCF_BCF) {
		fprintf(stderr, "Error: %s is %s; only VCF text (plain, gzip or BGZF) is read\n", path, vc_vcf_kind_name(kind));
		return VC_EINVAL;
	}
	int rc = VCF_FALLBACK;
	if (kind == VC_VCF_BGZF) {
		// $VAFC_BGZF = host | device; unset: VCF_BGZF_DEFAULT_DEVICE
		const char *e = getenv("VAFC_BGZF");
		const bool device = e && *e ? strcmp(e, "device") == 0 : VCF_BGZF_DEFAULT_DEVICE;
		if (device) rc = count_bgzf_device(c, path, sample_idx, min_depth, counts, st);
		if (rc == VCF_FALLBACK) {
			memset(&st, 0, sizeof st);
			c->z_host_blocks = count_members(path);
		}
	}
	if (rc == VCF_FALLBACK) rc = count_host(c, path, kind, sample_idx, min_depth, n_threads, counts, st);
	st.seconds = vc_now() - t0;
	if (stats) *stats = st;
	return rc;
}
