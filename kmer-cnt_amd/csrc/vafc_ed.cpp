// vafc_ed.cpp -- host side of the approximate pattern search (vc_ed_* of
// include/vafc.h): the reference's ed-vaf-counter.c with its edlibAlign calls
// replaced by the kernels of vafc_ed.hip.
//
//   queries       ref / alt k-mers of a pattern database, or raw byte strings
//   device data   byte -> class map, match masks [group][class][word][lane],
//                 per-lane query length and output index, one set per word width
//   count_block   host reads -> pinned staging -> H2D -> kernels (async)
//   count_file    count_fastq_kmers: kseq records into two alternating batches
//
// The staging (slots, the two-slot stager, the batch writer, the bridge to a
// caller's stream) is vafc_stage.h, shared with the k-mer counter; only the
// launch is this file's own.
//
// Nothing here searches on the CPU: any HIP failure is returned as VC_EHIP.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "vafc.h"
#include "vafc_ed.h"
#include "vafc_fastq.h"
#include "vafc_stage.h"

namespace {

// The queries of one word width, 64 to a group.
struct EdWidth {
	uint32_t n_groups = 0;
	int waves = 1;
	int lds_masks = 1;
	VcDevBuf<uint8_t> d_masks;
	VcDevBuf<uint32_t> d_qlen, d_qout;
};

// batches of vc_ed_count_file: bytes ($VAFC_BATCH_BYTES: vc_batch_bytes) and reads per pinned slot
const size_t ED_BATCH_BYTES = (size_t)8 << 20;
const size_t ED_BATCH_READS = (size_t)1 << 18;

} // namespace

struct vc_ed : VcDevice {
	int max_edit = 0;
	uint32_t n_out = 0;       // counts
	uint32_t n_class = 0;
	VcDevBuf<uint8_t> d_cls;
	VcDevBuf<uint32_t> d_counts;   // n_out + 2
	VcDevBuf<uint32_t> d_flags;
	EdWidth width[VC_ED_WIDTHS];
	uint32_t max_ranges = 0;   // vc_ed_set_max_ranges: 0 = sized from the device

	int submit(size_t bytes, uint64_t n_reads);   // the acquired slot of `stage`: H2D copies + kernels
};

namespace {

// One kernel per word width that has queries, all reads against each.
int launch(vc_ed *c, const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs, const uint32_t *d_lens,
           uint64_t n_reads, hipStream_t st)
{
	if (n_reads == 0) return VC_OK;
	HIPCK(c->timer.begin(st));
	for (int w = 0; w < VC_ED_WIDTHS; ++w) {
		const EdWidth &E = c->width[w];
		if (E.n_groups == 0) continue;
		VcEdArgs A;
		A.seq = d_seq;
		A.seq_bytes = seq_bytes;
		A.offs = d_offs;
		A.lens = d_lens;
		A.n_reads = n_reads;
		A.cls = c->d_cls;
		A.masks = E.d_masks;
		A.qlen = E.d_qlen;
		A.qout = E.d_qout;
		A.n_groups = E.n_groups;
		A.n_class = c->n_class;
		A.max_edit = c->max_edit;
		A.counts = c->d_counts;
		A.flags = c->d_flags;
		// query blocks x read ranges: about two rounds of blocks at 32 waves
		// per CU, so that a two-query panel fills the chip as well
		const uint64_t gx = (E.n_groups + (uint32_t)E.waves - 1) / (uint32_t)E.waves;
		const uint64_t target = (uint64_t)c->n_cu * (32u / (uint32_t)E.waves) * 2;
		uint64_t gy = (target + gx - 1) / gx;
		if (c->max_ranges && gy > c->max_ranges) gy = c->max_ranges;
		if (gy > n_reads) gy = n_reads;
		if (gy > 65535) gy = 65535;
		if (gy < 1) gy = 1;
		A.reads_per_range = (n_reads + gy - 1) / gy;
		gy = (n_reads + A.reads_per_range - 1) / A.reads_per_range;
		HIPCK(vc_ed_launch(&A, w, E.waves, E.lds_masks, (unsigned)gx, (unsigned)gy, st));
	}
	HIPCK(c->timer.end(st));
	return VC_OK;
}

template <typename W> void set_bit(std::vector<uint8_t> &tab, size_t word, unsigned bit)
{
	reinterpret_cast<W *>(tab.data())[word] |= (W)1 << bit;
}

// Build the device data of an open handle.  q: the query bytes, query i at
// offs[i] of length lens[i] (1..127), its count at out[i].
int ed_fill(vc_ed *c, const uint8_t *q, const uint32_t *offs, const uint32_t *lens, const uint32_t *out, size_t n)
{
	// symbol classes: one per byte value that occurs in a query, and class 0
	// for every other byte (no bit of any mask set); with all 256 values in
	// use there is no other byte and class = byte
	bool used[256] = {false};
	for (size_t i = 0; i < n; ++i)
		for (uint32_t j = 0; j < lens[i]; ++j) used[q[offs[i] + j]] = true;
	int n_used = 0;
	for (int b = 0; b < 256; ++b) n_used += used[b] ? 1 : 0;
	uint8_t cls[256];
	if (n_used == 256) {
		for (int b = 0; b < 256; ++b) cls[b] = (uint8_t)b;
		c->n_class = 256;
	} else {
		int next = 1;
		for (int b = 0; b < 256; ++b) cls[b] = used[b] ? (uint8_t)next++ : (uint8_t)0;
		c->n_class = (uint32_t)next;
	}
	HIPCK(c->d_cls.upload(cls, 256));
	HIPCK(c->d_counts.alloc((size_t)c->n_out + 2));
	HIPCK(c->d_counts.zero());
	HIPCK(c->d_flags.alloc(1));
	HIPCK(c->d_flags.zero());

	for (int w = 0; w < VC_ED_WIDTHS; ++w) {
		const uint32_t lo = w == VC_ED_W32 ? 1 : (w == VC_ED_W64 ? 33 : 65);
		const uint32_t hi = w == VC_ED_W32 ? 32 : (w == VC_ED_W64 ? 64 : 127);
		std::vector<size_t> ids;
		for (size_t i = 0; i < n; ++i)
			if (lens[i] >= lo && lens[i] <= hi) ids.push_back(i);
		if (ids.empty()) continue;
		EdWidth &E = c->width[w];
		const int nwords = vc_ed_width_words(w), wb = vc_ed_width_wordbytes(w);
		const unsigned bits = (unsigned)wb * 8;
		E.n_groups = (uint32_t)((ids.size() + 63) / 64);
		E.waves = E.n_groups < VC_ED_MAX_WAVES ? (int)E.n_groups : VC_ED_MAX_WAVES;
		E.lds_masks = (size_t)c->n_class * nwords * E.waves * 64 * wb <= VC_ED_LDS_MASKS ? 1 : 0;
		const size_t lanes = (size_t)E.n_groups * 64;
		const size_t words = lanes * c->n_class * nwords;
		std::vector<uint8_t> tab(words * wb, 0);
		std::vector<uint32_t> qlen(lanes, 0), qout(lanes, 0);
		for (size_t s = 0; s < ids.size(); ++s) {
			const size_t i = ids[s], g = s / 64, lane = s % 64;
			qlen[s] = lens[i];
			qout[s] = out[i];
			for (uint32_t j = 0; j < lens[i]; ++j) {
				const unsigned cl = cls[q[offs[i] + j]];
				const size_t word = ((g * c->n_class + cl) * nwords + j / bits) * 64 + lane;
				if (wb == 4) set_bit<uint32_t>(tab, word, j % bits);
				else set_bit<uint64_t>(tab, word, j % bits);
			}
		}
		HIPCK(E.d_masks.upload(tab.data(), tab.size()));
		HIPCK(E.d_qlen.upload(qlen.data(), lanes));
		HIPCK(E.d_qout.upload(qout.data(), lanes));
	}
	return VC_OK;
}

// A new handle for n checked queries; a failed step returns through vc_ed_destroy.
int ed_build(vc_ed **outp, const uint8_t *q, const uint32_t *offs, const uint32_t *lens, const uint32_t *out,
             size_t n, uint32_t n_out, int max_edit, int device)
{
	for (size_t i = 0; i < n; ++i)
		if (lens[i] < 1 || lens[i] > 127) return VC_EINVAL;
	vc_ed *c = new (std::nothrow) vc_ed;
	if (!c) return VC_ENOMEM;
	c->max_edit = max_edit;
	c->n_out = n_out;
	int rc = c->open(device);
	if (rc == VC_OK) rc = ed_fill(c, q, offs, lens, out, n);
	if (rc != VC_OK) {
		vc_ed_destroy(c);
		return rc;
	}
	*outp = c;
	return VC_OK;
}

} // namespace

int vc_ed::submit(size_t bytes, uint64_t n_reads)
{
	return stage.submit(bytes, n_reads, st, [&](const VcSlot &s) {
		return launch(this, s.d_seq, bytes, s.d_offs, s.d_lens, n_reads, st);
	});
}

extern "C" int vc_ed_create_raw(vc_ed **out, const uint8_t *queries, const uint32_t *q_offs, const uint32_t *q_lens,
                                size_t n_queries, int max_edit, int device)
{
	if (!out || (n_queries && (!queries || !q_offs || !q_lens)) || n_queries > 0x7FFFFFFFu) return VC_EINVAL;
	*out = nullptr;
	std::vector<uint32_t> idx(n_queries);
	for (size_t i = 0; i < n_queries; ++i) idx[i] = (uint32_t)i;
	return ed_build(out, queries, q_offs, q_lens, idx.data(), n_queries, (uint32_t)n_queries, max_edit, device);
}

extern "C" int vc_ed_create(vc_ed **out, const vc_patterns *db, int max_edit, int device)
{
	if (!out || !db) return VC_EINVAL;
	*out = nullptr;
	const int n = vc_patterns_count(db);
	if (n > (0x7FFFFFFF >> 1)) return VC_ETOOMANY;
	std::vector<uint8_t> q;
	std::vector<uint32_t> offs, lens, idx;
	for (int i = 0; i < n; ++i) {
		const char *rk = nullptr, *ak = nullptr;
		if (vc_pattern_fields(db, i, nullptr, nullptr, nullptr, nullptr, nullptr, &rk, &ak) != VC_OK) return VC_EINVAL;
		// kmer_len = strlen(ref_kmer) serves both searches (ed-vaf-counter.c:77,143-144)
		const size_t m = strlen(rk), ma = strnlen(ak, m);
		for (int allele = 0; allele < 2; ++allele) {
			offs.push_back((uint32_t)q.size());
			lens.push_back((uint32_t)m);
			idx.push_back(2u * (uint32_t)i + (uint32_t)allele);
			if (allele == 0) {
				q.insert(q.end(), rk, rk + m);
			} else {
				q.insert(q.end(), ak, ak + ma);
				q.insert(q.end(), m - ma, (uint8_t)0);   // a shorter alt_kmer is padded with NUL bytes
			}
		}
	}
	return ed_build(out, q.data(), offs.data(), lens.data(), idx.data(), lens.size(), 2u * (uint32_t)n, max_edit,
	                device);
}

extern "C" void vc_ed_destroy(vc_ed *c)
{
	if (!c) return;
	c->close();
	delete c;
}

extern "C" int vc_ed_count_block(vc_ed *c, const uint8_t *seq, size_t seq_bytes, const uint64_t *offs,
                                 const uint32_t *lens, uint64_t n_reads)
{
	if (!c || (n_reads && (!offs || !lens)) || (seq_bytes && !seq)) return VC_EINVAL;
	if (n_reads == 0) return VC_OK;
	for (uint64_t i = 0; i < n_reads; ++i)
		if (offs[i] > seq_bytes || lens[i] > seq_bytes - offs[i]) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	VcSlot *s;
	const int rc = c->stage.acquire_for(seq_bytes, n_reads, &s);
	if (rc != VC_OK) return rc;
	if (seq_bytes) memcpy(s->h_seq, seq, seq_bytes);
	memcpy(s->h_offs, offs, n_reads * sizeof(uint64_t));
	memcpy(s->h_lens, lens, n_reads * sizeof(uint32_t));
	return c->submit(seq_bytes, n_reads);
}

extern "C" int vc_ed_count_device(vc_ed *c, const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs,
                                  const uint32_t *d_lens, uint64_t n_reads, void *stream)
{
	if (!c || (n_reads && (!d_offs || !d_lens)) || (seq_bytes && !d_seq)) return VC_EINVAL;
	if (n_reads == 0) return VC_OK;
	HIPCK(hipSetDevice(c->dev));
	return c->on_stream(stream, [&](hipStream_t st) { return launch(c, d_seq, seq_bytes, d_offs, d_lens, n_reads, st); });
}

extern "C" int vc_ed_finish(vc_ed *c, uint32_t *counts)
{
	if (!c) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	c->stage.settle();
	uint32_t f = 0;
	HIPCK(hipMemcpy(&f, c->d_flags, sizeof f, hipMemcpyDeviceToHost));
	if (f & 1u) {
		fprintf(stderr, "[E::vafc] a device read reaches past seq_bytes: counts incomplete\n");
		return VC_EINVAL;
	}
	if (counts && c->n_out)
		HIPCK(hipMemcpy(counts, c->d_counts, (size_t)c->n_out * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return VC_OK;
}

extern "C" int vc_ed_reset(vc_ed *c)
{
	if (!c) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(c->d_counts.zero_async(c->st));
	HIPCK(c->d_flags.zero_async(c->st));
	return VC_OK;
}

extern "C" int vc_ed_set_counts(vc_ed *c, const uint32_t *counts)
{
	if (!c || (c->n_out && !counts)) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	if (c->n_out) {
		// pageable source: the copy has left the caller's buffer on return
		HIPCK(hipMemcpyAsync(c->d_counts, counts, (size_t)c->n_out * sizeof(uint32_t), hipMemcpyHostToDevice, c->st));
		HIPCK(hipStreamSynchronize(c->st));
	}
	return VC_OK;
}

extern "C" int vc_ed_set_max_ranges(vc_ed *c, uint32_t max_ranges)
{
	if (!c) return VC_EINVAL;
	c->max_ranges = max_ranges;
	return VC_OK;
}

extern "C" int vc_ed_shape(const vc_ed *c, int width, uint32_t *n_groups, int *waves, int *lds_masks)
{
	if (!c || width < 0 || width >= VC_ED_WIDTHS) return VC_EINVAL;
	const EdWidth &E = c->width[width];
	if (n_groups) *n_groups = E.n_groups;
	if (waves) *waves = E.waves;
	if (lds_masks) *lds_masks = E.lds_masks;
	return VC_OK;
}

extern "C" int vc_ed_kernel_ms(vc_ed *c, float *ms)
{
	return c ? c->timer.ms(ms) : VC_EINVAL;
}

extern "C" int vc_ed_count_file(vc_ed *c, const char *path, int n_threads, vc_file_stats *stats)
{
	if (!c || !path) return VC_EINVAL;
	const double t0 = vc_now();
	vc_file_stats st;
	memset(&st, 0, sizeof st);
	VcFastqReader rd;
	if (!(n_threads > 1 ? rd.open_parallel(path, n_threads) : rd.open(path))) return VC_EIO;
	HIPCK(hipSetDevice(c->dev));
	VcBatchWriter bw(vc_batch_bytes(ED_BATCH_BYTES), ED_BATCH_READS, [c]() { return c; });
	int rc = VC_OK;
	// a record that returns < 0 ends the file (ed-vaf-counter.c:137)
	while (rd.next() >= 0) {
		const size_t len = rd.seq_len();
		if ((rc = bw.add(rd.seq(), len)) != VC_OK) break;
		st.bases += len;
		++st.seqs;
	}
	if (rc == VC_OK) rc = bw.flush();
	st.blocks = bw.batches;
	st.seconds = vc_now() - t0;
	if (stats) *stats = st;
	return rc;
}
