// vafc_kc_host.cpp -- the histogram counter of kc-c4 and yak-count: the
// vc_kc_* calls and vc_yak_bloom_select of include/vafc.h over the kernels of
// vafc_kc.hip.  Batches reach it as they reach the pattern counter, through
// vc_ctx (vafc_ctx.h): vc_count_block, vc_count_device, the file passes.
#include "vafc_ctx.h"
#include "vafc_kc.h"

// The device hash table and its bookkeeping.
struct KcCounter final : vc_ctx {
	VcDevBuf<unsigned long long> d_table;    // 2 * slots
	uint64_t slots = 0;
	uint32_t tbits = 0;
	uint32_t n_parts = 1, part = 0;
	VcDevBuf<unsigned long long> d_stats;    // k-mers, distinct, table full, long-read list full
	VcDevBuf<unsigned long long> d_hist;     // up to 1024 bins + the slots counted
	VcDevBuf<uint32_t> d_nlong, d_long;      // d_long: the long-read list, d_long.cap entries
	VcDevBuf<uint64_t> d_segstart;           // d_long.cap + 1, grown with d_long
	VcDevBuf<uint64_t> d_first;              // first-occurrence stamps (vc_kc_track_first)
	bool track_first = false, lookup_only = false;
	uint64_t read_base = 0;                  // reads launched since the last reset

	int launch(const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs, const uint32_t *d_lens,
	           uint64_t n_reads, hipStream_t st, bool) override;
	int result(uint32_t *, uint64_t *kmers) override;
	int clear() override;
};

// NULL for no handle and for a pattern counter.
static KcCounter *as_kc(vc_ctx *c) { return dynamic_cast<KcCounter *>(c); }

// Enqueue the two counting kernels over device-resident reads on stream st.
int KcCounter::launch(const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs, const uint32_t *d_lens,
                      uint64_t n_reads, hipStream_t st, bool)
{
	if (n_reads == 0) return VC_OK;
	if (n_reads > 0xFFFFFFFFull) return VC_EINVAL;   // the long-read list holds u32 read indices
	const uint64_t need = seq_bytes / (KC_LONG + 1) + 1;
	if (need > d_long.cap) {
		HIPCK(hipStreamSynchronize(st));
		const uint64_t cap = need < 0xFFFFFFF0ull ? need : 0xFFFFFFF0ull;
		HIPCK(d_long.grow(cap, d_segstart, cap + 1));
	}
	KcArgs A;
	A.seq = d_seq;
	A.offs = d_offs;
	A.lens = d_lens;
	A.n_reads = n_reads;
	A.table = d_table;
	A.tmask = slots - 1;
	A.tbits = tbits;
	A.n_parts = n_parts;
	A.part = part;
	A.first = track_first && !lookup_only ? d_first : nullptr;
	A.read_base = read_base;
	A.lookup_only = lookup_only ? 1 : 0;
	read_base += n_reads;
	A.k = k;
	A.kmask = ((uint64_t)1 << (2 * k)) - 1;
	A.stats = d_stats;
	A.nlong = d_nlong;
	A.longlist = d_long;
	A.long_cap = (uint32_t)d_long.cap;
	A.segstart = d_segstart;
	const uint64_t blocks = (n_reads + KC_THREADS - 1) / KC_THREADS;
	const uint64_t maxg = (uint64_t)n_cu * 16;
	const int grid = (int)(blocks < maxg ? blocks : maxg);
	if (timing) HIPCK(timer.begin(st));
	HIPCK(vc_launch_kc(&A, grid, st));
	if (timing) HIPCK(timer.end(st));
	return VC_OK;
}

extern "C" int vc_kc_create(vc_ctx **out, int k, uint64_t table_slots, int device)
{
	if (!out) return VC_EINVAL;
	*out = nullptr;
	if (k < 1 || k > 31) return VC_EINVAL;
	KcCounter *c = new (std::nothrow) KcCounter;
	if (!c) return VC_ENOMEM;
	c->k = k;
	int rc = c->open(device);
	if (rc != VC_OK) {
		vc_destroy(c);
		return rc;
	}
	// at most 40 % of free HBM (rounded down to a power of two), so first-
	// occurrence stamps and yak's scratch table still fit beside it
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = (size_t)1 << 30;
	uint32_t cap_bits = 10;
	while (cap_bits < 40 && ((uint64_t)32 << cap_bits) <= (uint64_t)(fr * 0.4)) ++cap_bits;
	uint32_t tbits = cap_bits;
	if (table_slots) {
		tbits = 10;
		while (tbits < cap_bits && ((uint64_t)1 << tbits) < table_slots) ++tbits;
	}
	c->tbits = tbits;
	c->slots = (uint64_t)1 << tbits;
	if (c->d_table.alloc(2 * c->slots) != hipSuccess || c->d_stats.alloc(4) != hipSuccess ||
	    c->d_hist.alloc(1025) != hipSuccess || c->d_nlong.alloc(1) != hipSuccess) {
		vc_destroy(c);
		return VC_EHIP;
	}
	rc = vc_reset(c);
	if (rc == VC_OK && hipStreamSynchronize(c->st) != hipSuccess) rc = VC_EHIP;
	if (rc != VC_OK) {
		vc_destroy(c);
		return rc;
	}
	*out = c;
	return VC_OK;
}

// vc_finish: the k-mers seen (vc_kc_histogram gives the rest).
int KcCounter::result(uint32_t *, uint64_t *kmers)
{
	unsigned long long st[4];
	HIPCK(hipMemcpy(st, d_stats, sizeof st, hipMemcpyDeviceToHost));
	if (kmers) *kmers = st[0];
	if (st[3]) {
		fprintf(stderr, "[E::vafc] more reads longer than %d bases than the long-read list holds "
		        "(overlapping reads?): counts incomplete\n", KC_LONG);
		return VC_EINVAL;
	}
	return VC_OK;
}

int KcCounter::clear()
{
	HIPCK(hipMemsetAsync(d_table, 0, slots * 16, st));
	HIPCK(hipMemsetAsync(d_stats, 0, 4 * sizeof(unsigned long long), st));
	if (track_first) HIPCK(hipMemsetAsync(d_first, 0xFF, slots * 8, st));
	read_base = 0;
	lookup_only = false;
	return VC_OK;
}

extern "C" int vc_kc_set_partition(vc_ctx *ctx, uint32_t n_parts, uint32_t part)
{
	KcCounter *c = as_kc(ctx);
	if (!c || n_parts == 0 || n_parts > 1024 || part >= n_parts) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	c->n_parts = n_parts;
	c->part = part;
	return vc_reset(c);
}

extern "C" uint64_t vc_kc_slots(vc_ctx *c) { return as_kc(c) ? as_kc(c)->slots : 0; }

// hist[0..n_bins) on the host += the device histogram; *counted = slots in it
static int kc_hist(KcCounter *c, uint64_t *hist, uint32_t n_bins, uint64_t min_count, uint64_t *counted)
{
	HIPCK(hipMemsetAsync(c->d_hist, 0, 1025 * 8, c->st));
	const uint64_t blocks = (c->slots + 255) / 256;
	const uint64_t maxg = (uint64_t)c->n_cu * 8;
	HIPCK(vc_launch_kc_hist(c->d_table, c->slots, c->d_hist, n_bins, min_count, (int)(blocks < maxg ? blocks : maxg),
	                        c->st));
	std::vector<unsigned long long> h(n_bins + 1);
	HIPCK(hipMemcpyAsync(h.data(), c->d_hist, (n_bins + 1) * 8, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (hist)
		for (uint32_t i = 0; i < n_bins; ++i) hist[i] += h[i];
	if (counted) *counted = h[n_bins];
	return VC_OK;
}

extern "C" int vc_kc_histogram2(vc_ctx *ctx, uint64_t *hist, uint32_t n_bins, uint64_t min_count, uint64_t *distinct,
                                uint64_t *kmers)
{
	KcCounter *c = as_kc(ctx);
	if (!c || n_bins < 2 || n_bins > 1024) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	unsigned long long st[4];
	HIPCK(hipMemcpy(st, c->d_stats, sizeof st, hipMemcpyDeviceToHost));
	if (kmers) *kmers = st[0];
	if (distinct) *distinct = st[1];
	if (st[3]) return VC_EINVAL;   // long reads were left out (vc_finish said so): no histogram of the rest
	if (st[2] || st[1] > c->slots / 100 * 85) return VC_EFULL;
	uint64_t counted = 0;
	int rc = kc_hist(c, hist, n_bins, min_count, &counted);
	if (rc == VC_OK && distinct) *distinct = counted;
	return rc;
}

extern "C" int vc_kc_histogram(vc_ctx *c, uint64_t *hist, uint64_t *distinct, uint64_t *kmers)
{
	return vc_kc_histogram2(c, hist, 256, 1, distinct, kmers);
}

extern "C" int vc_kc_track_first(vc_ctx *ctx, int on)
{
	KcCounter *c = as_kc(ctx);
	if (!c) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	if (on && !c->d_first && c->d_first.alloc(c->slots) != hipSuccess) return VC_ENOMEM;
	c->track_first = on != 0;
	return vc_reset(c);
}

extern "C" int vc_yak_bloom_select(vc_ctx *ctx, int pre, int bf_shift, int n_hash)
{
	KcCounter *c = as_kc(ctx);
	if (!c || pre < 0 || pre > 40) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	unsigned long long st[4];
	HIPCK(hipMemcpy(st, c->d_stats, sizeof st, hipMemcpyDeviceToHost));
	if (st[3]) return VC_EINVAL;   // long reads were left out (vc_finish said so)
	if (st[2] || st[1] > c->slots / 100 * 85) return VC_EFULL;
	// yak_ch_init / yak_bf_init (yak-count.c:71-80, 115-121): filters exist only
	// for n_hash > 0 and 9 <= bf_shift - pre <= 55
	const int ns = bf_shift - pre;
	const bool bf_on = n_hash > 0 && bf_shift > pre && ns >= 9 && ns + 9 <= 64;
	if (bf_on && !c->track_first) return VC_EINVAL;
	YakBloom B;
	VcDevBuf<unsigned long long> wtab;   // the scratch table of this call
	B.table = c->d_table;
	B.counts_out = c->d_table;
	B.first = c->d_first;
	B.slots = c->slots;
	B.pre = (uint32_t)pre;
	B.ns = bf_on ? (uint32_t)ns : 9;
	B.n_hash = bf_on ? (uint32_t)n_hash : 0;
	B.wtab = nullptr;
	B.wslots = 1;
	B.wbits = 0;
	B.overflow = c->d_stats + 2;
	if (bf_on) {
		uint64_t singles = 0;
		std::vector<uint64_t> h(2, 0);
		int rc = kc_hist(c, h.data(), 2, 1, nullptr);   // h[1]: keys seen exactly once
		if (rc != VC_OK) return rc;
		singles = h[1];
		uint32_t wbits = 10;
		while (wbits < 48 && ((uint64_t)1 << wbits) < 2 * singles * (uint64_t)n_hash) ++wbits;
		B.wbits = wbits;
		B.wslots = (uint64_t)1 << wbits;
		// no room for the scratch table: report full, so the caller counts
		// again in more partitions (fewer singletons per pass)
		if (wtab.alloc(2 * B.wslots) != hipSuccess) return VC_EFULL;
		B.wtab = wtab;
		HIPCK(wtab.zero_async(c->st));
	}
	const uint64_t blocks = (c->slots + 255) / 256;
	const uint64_t maxg = (uint64_t)c->n_cu * 8;
	hipError_t e = vc_launch_yak_select(&B, (int)(blocks < maxg ? blocks : maxg), c->st);
	if (e == hipSuccess) e = hipStreamSynchronize(c->st);
	wtab.free();
	if (e != hipSuccess) return VC_EHIP;
	HIPCK(hipMemcpy(st, c->d_stats, sizeof st, hipMemcpyDeviceToHost));
	if (st[2]) return VC_EFULL;
	c->lookup_only = true;
	return VC_OK;
}
