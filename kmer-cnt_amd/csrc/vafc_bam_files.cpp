// vafc_bam_files.cpp -- bam-vaf-counter's file pass (count_bam_variants of
// bam-vaf-counter.c): vc_bam_count_file and vc_bam_inflate_info.  The stderr
// lines, the index rule and the regions are the same for both ways of reading
// the records:
//
//   host     VcBamReader (vafc_bam.cpp): zlib threads and one parsing thread,
//            batches of descriptors through vc_bam_count_block
//   device   (the default; $VAFC_BGZF=host|device forces one) the members behind the header go down
//            compressed in pieces of whole members (vafc_bgzf_io.h reads them
//            straight into the stager's pinned slots), are inflated by
//            vc_bgzf_inflate_device on the inflater's stream into one of two
//            text buffers, behind the unconsumed tail of the piece before, and
//            are read by the text scan of vafc_bam.hip with the members'
//            borders as cuts; piece k + 1 is read, copied and inflated while
//            piece k is scanned.  Anything the scan does not take (vafc.h lists
//            it) puts the counts back and leaves the file to the host pass.
//   seek     ($VAFC_BAM_INDEX=seek, beside an index and with regions) the plan
//            of vc_bam_index_plan: per span an fseek and its members, the spans
//            of a batch inflated back to back into one text buffer and walked
//            as pieces in one launch (vc_bam_scan_pieces_*), batch k + 1 read,
//            copied and inflated while batch k is walked; a cut piece is read
//            once more with further members.  Any doubt puts the counts back
//            and leaves the file to the two passes above.
//
// Compiled as HIP (it owns device buffers); no kernel is defined here.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "vafc.h"
#include "vafc_bam.h"
#include "vafc_bam_ctx.h"
#include "vafc_bgzf_io.h"
#include "vafc_stage.h"

namespace {

// records and data bytes of one batch of the host pass, text of one piece of
// the device pass ($VAFC_BATCH_BYTES: vc_batch_bytes)
const size_t BAM_BATCH_BYTES = (size_t)32 << 20;
const size_t BAM_BATCH_RECS = (size_t)1 << 19;
// BGZF input without $VAFC_BGZF: inflated and parsed on the device (DESIGN 16 has the measurement that decided it)
const bool BAM_BGZF_DEFAULT_DEVICE = true;

const int BAM_FALLBACK = 100;
const size_t BAM_ZHEAD = (size_t)4 << 20;   // room in front of a piece's text: the longest record the device pass takes
const size_t BAM_PIECE_BLOCKS = 65536;      // members of one piece at most

// Where the records begin in the text of a BAM whose first `len` bytes are
// there: 1 and *body, 0 when more text is needed, -1 for no BAM header.
int header_end(const uint8_t *t, size_t len, size_t *body)
{
	if (len < 12) return 0;
	if (memcmp(t, "BAM\1", 4) != 0) return -1;
	const int32_t l_text = (int32_t)vc_le32(t + 4);
	if (l_text < 0) return -1;
	size_t at = 8 + (size_t)l_text;
	if (len < at + 4) return 0;
	const int32_t n_ref = (int32_t)vc_le32(t + at);
	if (n_ref < 0) return -1;
	at += 4;
	for (int32_t i = 0; i < n_ref; ++i) {
		if (len < at + 4) return 0;
		const int32_t l_name = (int32_t)vc_le32(t + at);
		if (l_name < 1) return -1;
		at += 4 + (size_t)l_name + 4;
	}
	if (len < at) return 0;
	*body = at;
	return 1;
}

struct BamPiece {
	size_t n_blocks = 0;
	uint64_t text_len = 0;
	bool last = false;               // the file ended behind it
	int buf = 0;                     // its text buffer
	std::vector<uint64_t> starts;    // text offset of each member
};

struct BamZText {
	vc_bam *c;
	FILE *fp;
	hipEvent_t ev;   // on the handle's stream: the copy of a text buffer's tail out of it
	size_t cap;      // text of one piece
	vc_bgzf *zf = c->zf;
	hipStream_t zst = (hipStream_t)vc_bgzf_stream(zf);
	bool file_ended = false;
	uint64_t device_members = 0;

	// Read the next piece into the stager's slot and send it on its way: H2D and
	// inflate on the inflater's stream, into text buffer b behind its head room.
	int start_piece(BamPiece &p, int b)
	{
		p = BamPiece();
		p.buf = b;
		if (file_ended) {
			p.last = true;
			return VC_OK;
		}
		const size_t raw_room = cap + 65536, max_blocks = std::min(BAM_PIECE_BLOCKS, raw_room / 28 + 1);
		const size_t desc_at = (raw_room + 7) & ~(size_t)7;
		VcSlot *s;
		int rc = c->stage.acquire_for(desc_at + max_blocks * sizeof(vc_bgzf_block), 1, &s);
		if (rc != VC_OK) return rc;
		vc_bgzf_block *desc = reinterpret_cast<vc_bgzf_block *>(s->h_seq + desc_at);
		size_t raw_len = 0;
		while (p.text_len < cap && raw_len + 65536 <= raw_room && p.n_blocks < max_blocks) {
			VcBgzfMember m;
			const int r = vc_bgzf_read_member(fp, s->h_seq + raw_len, &m);
			if (r < 0) return BAM_FALLBACK;   // cut, not BGZF, or an ISIZE no member holds
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
			p.starts.push_back(p.text_len);
			p.text_len += m.isize;
			raw_len += m.size;
		}
		if (p.n_blocks == 0) return VC_OK;
		// the text buffer: nobody reads it any more but the copy of its tail, which `ev` follows
		c->zhead[b] = BAM_ZHEAD;
		if (c->ztext[b].cap < BAM_ZHEAD + p.text_len) HIPCK(c->ztext[b].grow(BAM_ZHEAD + (size_t)p.text_len + 65536));
		HIPCK(hipStreamWaitEvent(zst, ev, 0));
		uint8_t *d_text = c->ztext[b] + BAM_ZHEAD;
		const size_t nb = p.n_blocks;
		const uint64_t tl = p.text_len;
		// the descriptors travel with the compressed bytes: one copy of [0, desc_at + n * 32)
		return c->stage.submit(desc_at + nb * sizeof(vc_bgzf_block), 1, zst, [&](const VcSlot &sl) {
			return vc_bgzf_inflate_device(zf, sl.d_seq, raw_len, reinterpret_cast<const vc_bgzf_block *>(sl.d_seq + desc_at), nb,
			                              d_text, (size_t)tl, VC_STREAM_CTX);
		}, false);
	}
};

// The records of a BGZF BAM through the device inflater and the text scan.
// BAM_FALLBACK: the file is the host pass's; the counts may have been touched.
int count_device_pass(vc_bam *c, const char *path, vc_file_stats &st, uint64_t *host_members, uint64_t *device_members)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) return BAM_FALLBACK;
	struct Closer {
		FILE *fp;
		hipEvent_t ev = nullptr;
		~Closer()
		{
			if (fp) fclose(fp);
			if (ev) (void)hipEventDestroy(ev);
		}
	} own{fp};
	int rc;
	if (!c->zf && (rc = vc_bgzf_create(&c->zf, c->dev)) != VC_OK) return rc;
	HIPCK(hipEventCreateWithFlags(&own.ev, hipEventDisableTiming));

	// the header: members inflated here until it parses
	std::vector<uint8_t> mem(VC_BGZF_MAX_MEMBER), buf;
	std::vector<uint64_t> toff(1, 0);   // text offset of each header member
	std::vector<long> foff;             // ... and its file offset
	size_t body = 0;
	for (int got = 0; got == 0;) {
		const long at = ftell(fp);
		VcBgzfMember m;
		if (vc_bgzf_read_member(fp, mem.data(), &m) != 1) return BAM_FALLBACK;
		const size_t len = buf.size();
		buf.resize(len + m.isize + 1);
		const bool ok = vc_bgzf_inflate_member(mem.data(), m, buf.data() + len);
		buf.resize(len + m.isize);
		if (!ok) return BAM_FALLBACK;
		foff.push_back(at);
		toff.push_back(buf.size());
		if ((got = header_end(buf.data(), buf.size(), &body)) < 0) return BAM_FALLBACK;
	}
	*host_members = foff.size();
	// the member that holds the first record; the device starts over with it
	size_t mb = 0;
	while (mb + 1 < toff.size() && toff[mb + 1] <= body) ++mb;
	size_t first_skip = body - (size_t)toff[mb];
	if (mb < foff.size() && fseek(fp, foff[mb], SEEK_SET) != 0) return BAM_FALLBACK;
	buf = std::vector<uint8_t>();

	BamZText src{c, fp, own.ev, vc_batch_bytes(BAM_BATCH_BYTES)};
	HIPCK(hipEventRecord(own.ev, c->st));
	BamPiece piece[2];
	if ((rc = src.start_piece(piece[0], 0)) != VC_OK) return rc;
	int tail_buf = 0;
	size_t tail_at = 0, tail_len = 0;
	std::vector<uint64_t> cuts;
	for (int k = 0;; ++k) {
		BamPiece &p = piece[k & 1];
		const int b = p.buf;
		if (p.n_blocks) {
			size_t n = 0, ok = 0;
			if ((rc = vc_bgzf_finish(src.zf, nullptr, 0, &n, &ok)) != VC_OK) return rc;
			if (ok != p.n_blocks) return BAM_FALLBACK;   // a member that does not inflate
			src.device_members += p.n_blocks;
		}
		if (first_skip > p.text_len) return BAM_FALLBACK;   // cannot be: the header's member is the piece's first
		// the text to scan: the tail before, then this piece (the very first one from the first record on)
		const uint8_t *d_text;
		size_t text_len;
		cuts.clear();
		if (p.n_blocks == 0) {
			// nothing new: what is left of the piece before is the file's last, cut record
			d_text = c->ztext[tail_buf] + tail_at;
			text_len = tail_len;
		} else {
			if (tail_len > c->zhead[b]) return BAM_FALLBACK;   // a record longer than the room in front of a text buffer
			const size_t at = c->zhead[b] + first_skip - tail_len;
			if (tail_len)
				HIPCK(hipMemcpyAsync(c->ztext[b] + at, c->ztext[tail_buf] + tail_at, tail_len, hipMemcpyDeviceToDevice, c->st));
			d_text = c->ztext[b] + at;
			text_len = tail_len + (size_t)p.text_len - first_skip;
			for (const uint64_t s : p.starts)
				if (s > first_skip || (s == first_skip && tail_len)) cuts.push_back(tail_len + s - first_skip);
			tail_buf = b;
			tail_at = at;
		}
		first_skip = 0;
		HIPCK(hipEventRecord(own.ev, c->st));   // the other buffer's tail has left it
		const bool final = p.last;
		if ((rc = vc_bam_scan_text_cuts(c, d_text, text_len, 0, cuts.data(), cuts.size(), final ? 1 : 0)) != VC_OK) return rc;
		// the next piece is read, copied and inflated while this one is scanned and counted
		if (!final && (rc = src.start_piece(piece[(k + 1) & 1], b ^ 1)) != VC_OK) return rc;
		vc_bam_text_res res;
		if ((rc = vc_bam_text_result(c, &res)) != VC_OK) return rc;
		if (res.irregular || res.short_stop) return BAM_FALLBACK;
		st.seqs += res.records;
		st.bases += res.bases;
		++st.blocks;
		if (final) break;
		tail_at += (size_t)res.consumed;
		tail_len = text_len - (size_t)res.consumed;
	}
	*device_members = src.device_members;
	return VC_OK;
}

// ---------------------------------------------------------------------------
// The seeking pass ($VAFC_BAM_INDEX=seek; item 9 of the contract)
// ---------------------------------------------------------------------------

// The members of some spans, compressed, and the spans as pieces of the text
// the members inflate to.
struct SeekBatch {
	std::vector<uint8_t> raw;
	std::vector<vc_bgzf_block> desc;
	std::vector<vc_bam_piece> pieces;
	std::vector<size_t> span_of;   // each piece's span in the plan
	uint64_t text_len = 0;
	int buf = 0;
};

struct BamSeek {
	vc_bam *c;
	FILE *fp;
	uint64_t fsize;
	const vc_bam_span *spans;
	size_t n_spans;
	size_t cap;          // text of one batch
	vc_file_stats &st;
	size_t next = 0;     // span
	uint64_t members = 0, rereads = 0;
	uint32_t why = VC_BAM_SEEK_DONE;
	std::vector<uint8_t> mem = std::vector<uint8_t>(VC_BGZF_MAX_MEMBER);
	std::vector<std::pair<size_t, uint64_t>> again;   // spans whose piece was cut, and the bytes missing

	int give_up(uint32_t reason)
	{
		why = reason;
		return BAM_FALLBACK;
	}

	// The members of span i, from the one at beg >> 16 through the one at end >>
	// 16 and on until `extra` more bytes of text are there, behind what b holds.
	int read_span(SeekBatch &b, size_t i, uint64_t extra)
	{
		const uint64_t beg_c = spans[i].beg >> 16, end_c = spans[i].end >> 16;
		const uint32_t beg_u = (uint32_t)(spans[i].beg & 0xFFFF), end_u = (uint32_t)(spans[i].end & 0xFFFF);
		if (beg_c >= fsize || end_c > fsize || fseeko(fp, (off_t)beg_c, SEEK_SET) != 0) return give_up(VC_BAM_SEEK_OFFSET);
		vc_bam_piece p;
		p.entry = b.text_len + beg_u;
		p.stop = 0;
		bool first = true, have_stop = false;
		uint64_t pos = beg_c, extra_got = 0;
		while (!have_stop || extra_got < extra) {
			if (!have_stop && pos > end_c) return give_up(VC_BAM_SEEK_OFFSET);   // no member starts at end >> 16
			VcBgzfMember m;
			const int r = vc_bgzf_read_member(fp, mem.data(), &m);
			if (r < 0) return give_up(VC_BAM_SEEK_OFFSET);
			if (r == 0) {
				// the end of the file: where a span may end, with nothing behind it
				if (!have_stop && (pos != end_c || end_u != 0 || first)) return give_up(VC_BAM_SEEK_OFFSET);
				if (!have_stop) p.stop = b.text_len;
				have_stop = true;
				break;
			}
			if (first && beg_u >= m.isize) return give_up(VC_BAM_SEEK_OFFSET);
			first = false;
			if (have_stop) extra_got += m.isize;
			if (pos == end_c) {
				if (end_u > m.isize) return give_up(VC_BAM_SEEK_OFFSET);
				p.stop = b.text_len + end_u;
				have_stop = true;
			}
			vc_bgzf_block d;
			d.in_off = b.raw.size() + m.payload;
			d.in_len = (uint32_t)m.payload_len;
			d.isize = m.isize;
			d.out_off = b.text_len;
			d.crc32 = m.crc32;
			d.reserved = 0;
			b.desc.push_back(d);
			b.raw.insert(b.raw.end(), mem.data(), mem.data() + m.size);
			b.text_len += m.isize;
			pos += m.size;
			if (b.text_len >= 0xFFFFFFF0ull) return give_up(VC_BAM_SEEK_LONG);
		}
		p.limit = b.text_len;
		b.pieces.push_back(p);
		b.span_of.push_back(i);
		return VC_OK;
	}

	// The next spans of the plan, up to a batch's text.
	int fill(SeekBatch &b, int buf)
	{
		b = SeekBatch();
		b.buf = buf;
		while (next < n_spans && (b.pieces.empty() || b.text_len < cap)) {
			const int rc = read_span(b, next, 0);
			if (rc != VC_OK) return rc;
			++next;
		}
		return VC_OK;
	}

	// H2D and inflate on the inflater's stream, into the batch's text buffer.
	int submit(SeekBatch &b)
	{
		const size_t desc_at = (b.raw.size() + 7) & ~(size_t)7, nb = b.desc.size();
		const size_t total = desc_at + nb * sizeof(vc_bgzf_block);
		VcSlot *s;
		const int rc = c->stage.acquire_for(total + 8, 1, &s);
		if (rc != VC_OK) return rc;
		memcpy(s->h_seq, b.raw.data(), b.raw.size());
		memcpy(s->h_seq + desc_at, b.desc.data(), nb * sizeof(vc_bgzf_block));
		c->zhead[b.buf] = 0;
		if (c->ztext[b.buf].cap < b.text_len + 1) HIPCK(c->ztext[b.buf].grow((size_t)b.text_len + 65536));
		uint8_t *d_text = c->ztext[b.buf];
		const size_t raw_len = b.raw.size();
		const uint64_t tl = b.text_len;
		return c->stage.submit(total, 1, (hipStream_t)vc_bgzf_stream(c->zf), [&](const VcSlot &sl) {
			return vc_bgzf_inflate_device(c->zf, sl.d_seq, raw_len, reinterpret_cast<const vc_bgzf_block *>(sl.d_seq + desc_at), nb,
			                              d_text, (size_t)tl, VC_STREAM_CTX);
		}, false);
	}

	// Wait for the batch's text and walk, check and count its pieces.
	int scan(SeekBatch &b)
	{
		size_t n = 0, ok = 0;
		const int rc = vc_bgzf_finish(c->zf, nullptr, 0, &n, &ok);
		if (rc != VC_OK) return rc;
		if (ok != b.desc.size()) return give_up(VC_BAM_SEEK_INFLATE);
		members += b.desc.size();
		return vc_bam_scan_pieces_host(c, c->ztext[b.buf], (size_t)b.text_len, b.pieces.data(), b.pieces.size());
	}

	// What the batch's pieces came to; a cut piece of the plan's own batches is
	// noted to be read again, one of a second reading ends the pass.
	int result(SeekBatch &b, bool second)
	{
		vc_bam_pieces_res res;
		std::vector<vc_bam_piece_status> stat(b.pieces.size());
		const int rc = vc_bam_pieces_result(c, &res, stat.data(), stat.size(), nullptr, 0);
		if (rc != VC_OK) return rc;
		if (res.n_short) return give_up(VC_BAM_SEEK_SHORT);
		if (res.irregular) return give_up(VC_BAM_SEEK_IRREGULAR);
		if (res.n_noroom) return give_up(VC_BAM_SEEK_LONG);   // cannot be: the pieces are disjoint
		if (res.n_cut && second) return give_up(VC_BAM_SEEK_CUT);
		for (size_t i = 0; i < stat.size(); ++i)
			if (stat[i].status == VC_BAM_PIECE_CUT) again.emplace_back(b.span_of[i], stat[i].missing ? stat[i].missing : 1);
		st.seqs += res.records;
		st.bases += res.bases;
		++st.blocks;
		return VC_OK;
	}

	int run()
	{
		SeekBatch bt[2];
		int rc = fill(bt[0], 0);
		if (rc == VC_OK && !bt[0].pieces.empty()) rc = submit(bt[0]);
		for (int k = 0; rc == VC_OK && !bt[k & 1].pieces.empty(); ++k) {
			SeekBatch &b = bt[k & 1], &nx = bt[(k + 1) & 1];
			if ((rc = scan(b)) != VC_OK) break;
			// the next batch is read, copied and inflated while this one is walked and counted
			if ((rc = fill(nx, b.buf ^ 1)) != VC_OK) break;
			if (!nx.pieces.empty() && (rc = submit(nx)) != VC_OK) break;
			rc = result(b, false);
		}
		for (size_t i = 0; rc == VC_OK && i < again.size(); ++i) {
			SeekBatch b;
			if ((rc = read_span(b, again[i].first, again[i].second)) != VC_OK) break;
			if ((rc = submit(b)) != VC_OK || (rc = scan(b)) != VC_OK) break;
			rc = result(b, true);
			++rereads;
		}
		return rc;
	}
};

// The records the index's spans hold, through the device inflater and the
// piece walk.  BAM_FALLBACK: the file is the whole-file pass's (sk.state says
// why); the counts may have been touched.
int count_seek_pass(vc_bam *c, const char *path, const std::vector<int32_t> &tid, const std::vector<int32_t> &start,
                    const std::vector<int32_t> &end, vc_file_stats &st, vc_bam_seek_res &sk)
{
	vc_bam_span *spans = nullptr;
	size_t n_spans = 0;
	int rc = vc_bam_index_plan(path, nullptr, c->n_ref, tid.data(), start.data(), end.data(), tid.size(), &spans, &n_spans);
	struct Owner {
		vc_bam_span *spans;
		FILE *fp;
		~Owner()
		{
			vc_bam_index_plan_free(spans);
			if (fp) fclose(fp);
		}
	} own{spans, nullptr};
	if (rc != VC_OK) {
		sk.state = VC_BAM_SEEK_NO_INDEX;
		return rc == VC_BAM_NO_SEEK || rc == VC_EINVAL ? BAM_FALLBACK : rc;
	}
	sk.spans = n_spans;
	own.fp = fopen(path, "rb");
	if (!own.fp || fseeko(own.fp, 0, SEEK_END) != 0) {
		sk.state = VC_BAM_SEEK_OFFSET;
		return BAM_FALLBACK;
	}
	const uint64_t fsize = (uint64_t)ftello(own.fp);
	if (!c->zf && (rc = vc_bgzf_create(&c->zf, c->dev)) != VC_OK) return rc;
	BamSeek seek{c, own.fp, fsize, spans, n_spans, vc_batch_bytes(BAM_BATCH_BYTES), st};
	rc = seek.run();
	sk.members = seek.members;
	sk.rereads = seek.rereads;
	sk.state = seek.why;
	return rc;
}

// The device pass (or, with regions given, the seeking pass) with the handle's
// counts kept: VC_OK, BAM_FALLBACK with the counts as they were before the
// file, or an error.
int count_device(vc_bam *c, const char *path, int32_t n_ref, vc_file_stats &st, uint64_t header_members = 0,
                 const std::vector<int32_t> *tid = nullptr, const std::vector<int32_t> *start = nullptr,
                 const std::vector<int32_t> *end = nullptr)
{
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	c->stage.settle();
	std::vector<uint32_t> before(2 * (size_t)c->n_pat + 2);
	HIPCK(hipMemcpy(before.data(), c->d_counts, 2 * (size_t)c->n_pat * sizeof(uint32_t), hipMemcpyDeviceToHost));
	const int32_t n_ref_before = c->n_ref;
	c->n_ref = n_ref;
	uint64_t host_members = header_members, device_members = 0;
	int rc;
	if (tid) {
		rc = count_seek_pass(c, path, *tid, *start, *end, st, c->z_seek);
		device_members = c->z_seek.members;
	} else {
		rc = count_device_pass(c, path, st, &host_members, &device_members);
	}
	c->n_ref = n_ref_before;
	// whatever is in flight has ended before the buffers are left alone
	if (c->zf) (void)vc_bgzf_finish(c->zf, nullptr, 0, nullptr, nullptr);
	(void)hipStreamSynchronize(c->st);
	c->stage.settle();
	if (rc == VC_OK) {
		c->z_host_members = host_members;
		c->z_device_members = device_members;
		return VC_OK;
	}
	const int rc2 = vc_bam_set_counts(c, before.data());
	return rc2 != VC_OK ? rc2 : rc;
}

} // namespace

extern "C" int vc_bam_inflate_info(const vc_bam *c, uint64_t *host_members, uint64_t *device_members)
{
	if (!c) return VC_EINVAL;
	if (host_members) *host_members = c->z_host_members;
	if (device_members) *device_members = c->z_device_members;
	return VC_OK;
}

extern "C" int vc_bam_seek_info(const vc_bam *c, vc_bam_seek_res *res)
{
	if (!c || !res) return VC_EINVAL;
	*res = c->z_seek;
	return VC_OK;
}

extern "C" int vc_bam_count_file(vc_bam *c, const char *path, int n_threads, vc_file_stats *stats)
{
	if (!c || !path) return VC_EINVAL;
	const double t0 = vc_now();
	vc_file_stats st;
	memset(&st, 0, sizeof st);
	if (stats) *stats = st;
	VcBamReader rd;
	int rc = rd.open(path, n_threads);
	if (rc == VC_EIO) {
		fprintf(stderr, "Error: failed to open BAM file: %s\n", path);
		return rc;
	}
	if (rc != VC_OK) {
		int kind = VC_BAM_BGZF;
		if (vc_bam_probe(path, &kind) == VC_OK && kind == VC_BAM_BGZF) fprintf(stderr, "Error: failed to read BAM header\n");
		return rc;
	}
	// count_bam_variants :436-458: regions are used only beside an index
	const bool have_regions = !c->reg_chr.empty();
	const bool have_index = vc_bam_index_usable(path, nullptr, 0) != 0;
	std::vector<int32_t> tid, start, end;
	if (!have_index || !have_regions) {
		if (!have_index)
			fprintf(stderr, "[M::%s] Warning: failed to load BAM index for %s, processing all reads\n", "count_bam_variants", path);
		if (!have_regions)
			fprintf(stderr, "[M::%s] Warning: no target regions available, processing all reads\n", "count_bam_variants");
	} else {
		fprintf(stderr, "[M::%s] Using indexed access to fetch reads from %d target regions\n", "count_bam_variants",
		        (int)c->reg_chr.size());
		std::unordered_map<std::string, int32_t> tid_of;
		for (size_t i = 0; i < rd.refs().size(); ++i) tid_of.emplace(rd.refs()[i], (int32_t)i);
		for (size_t i = 0; i < c->reg_chr.size(); ++i) {
			const auto it = tid_of.find(c->reg_chr[i]);
			if (it == tid_of.end()) {
				fprintf(stderr, "Warning: chromosome %s not found in BAM\n", c->reg_chr[i].c_str());
				continue;
			}
			tid.push_back(it->second);
			start.push_back(c->reg_start[i]);
			end.push_back(c->reg_end[i]);
		}
	}
	const bool weighted = have_index && have_regions;
	const char *how = getenv("VAFC_BAM_INDEX");
	const bool seek = how && strcmp(how, "seek") == 0 && weighted && !tid.empty();
	memset(&c->z_seek, 0, sizeof c->z_seek);
	if (how && strcmp(how, "seek") == 0 && !seek)
		c->z_seek.state = !have_index ? VC_BAM_SEEK_NO_INDEX : VC_BAM_SEEK_NO_REGIONS;
	rc = vc_bam_set_regions(c, tid.data(), start.data(), end.data(), tid.size());
	if (rc != VC_OK) return rc;
	if (weighted && tid.empty()) {
		// every region is on a chromosome this file lacks: the reference fetches nothing
		st.seconds = vc_now() - t0;
		if (stats) *stats = st;
		return VC_OK;
	}
	// $VAFC_BAM_INDEX = seek: the index's spans alone, where the file can be read so
	if (seek) {
		rc = count_device(c, path, (int32_t)rd.refs().size(), st, rd.members(), &tid, &start, &end);
		if (rc != BAM_FALLBACK) {
			st.seconds = vc_now() - t0;
			if (stats) *stats = st;
			return rc;
		}
		memset(&st, 0, sizeof st);
	}
	// $VAFC_BGZF = host | device; unset: BAM_BGZF_DEFAULT_DEVICE
	const char *e = getenv("VAFC_BGZF");
	if (e && *e ? strcmp(e, "device") == 0 : BAM_BGZF_DEFAULT_DEVICE) {
		rc = count_device(c, path, (int32_t)rd.refs().size(), st);
		if (rc != BAM_FALLBACK) {
			st.seconds = vc_now() - t0;
			if (stats) *stats = st;
			return rc;
		}
		memset(&st, 0, sizeof st);
	}
	const size_t limit = vc_batch_bytes(BAM_BATCH_BYTES);
	std::vector<vc_bam_rec> recs;
	std::vector<uint8_t> data;
	for (;;) {
		recs.clear();
		data.clear();
		if (!rd.next_batch(recs, data, limit, BAM_BATCH_RECS)) break;
		if ((rc = vc_bam_count_block(c, recs.data(), recs.size(), data.data(), data.size())) != VC_OK) break;
		++st.blocks;
	}
	c->z_host_members = rd.members();
	c->z_device_members = 0;
	st.bases = rd.bases;
	st.seqs = rd.records;
	st.seconds = vc_now() - t0;
	if (stats) *stats = st;
	return rc;
}
