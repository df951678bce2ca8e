// vafc_host.cpp -- the pattern counter of libvafc.so and the calls of
// include/vafc.h that every read counter answers.
//
//   PanelCounter  static key table + LDS prefilter in HBM, counts, its kernels
//   count_block   host block -> pinned staging -> H2D -> kernels (async)
//   count_device, finish, reset, destroy, timing: through vc_ctx (vafc_ctx.h),
//                 so they serve the histogram counter (vafc_kc_host.cpp) too
//
// The shards of a multi-GPU counter are vafc_shards.cpp and the file passes
// vafc_files.cpp.  The pattern database and the .vaf writer are
// vafc_patterns.cpp; the staging of host batches is vafc_stage.h.
//
// Nothing here computes counts on the CPU: every k-mer goes through the HIP
// kernels in vafc_kernels.hip, and any HIP failure is returned as VC_EHIP.
#include <math.h>

#include "vafc_ctx.h"
#include "vafc_internal.h"

struct PanelCounter final : vc_ctx {
	uint32_t n_patterns = 0;
	uint64_t n_keys = 0;
	VcDevBuf<vc_slot_t> d_table;
	int ablate = 0;                   // kernel ablation variant (libvafc_abl.so only)
	uint32_t variant = 0;             // kernel A/B experiment knobs ($VAFC_VARIANT, tools/ab.py)
	int nt4 = 0;                      // seq_nt4 decode everywhere (vc_set_nt4_decode)
	uint32_t tbits = 0;
	VcDevBuf<uint32_t> d_filter;
	uint32_t wbits = 0;
	VcDevBuf<uint32_t> d_l2f;              // second-level filter (large key sets only)
	uint32_t l2bits = 0;
	uint32_t fsh = 0;
	uint32_t flank = 0;                    // the filter is the flank bitmap (vafc_common.h)
	uint32_t big = 0;                      // the filter is the large-panel Bloom filter (vc_big_word)
	uint32_t fwords = 0;                   // LDS filter words
	uint32_t qcap = VC_QCAP;               // LDS queue entries per wave
	uint32_t *d_counts = nullptr;          // active outputs (own or bound)
	unsigned long long *d_tally = nullptr;
	VcDevBuf<uint32_t> own_counts;         // 2 * n_patterns + 2
	VcDevBuf<unsigned long long> own_tally;
	VcDevBuf<uint32_t> d_nlong;
	VcDevBuf<uint32_t> d_flags;            // kernel error flags (VcKernelArgs::flags)
	VcDevBuf<uint8_t> d_pad;               // 64 B staging for inputs under 16 B (kernels load 16 B)
	VcDevBuf<uint32_t> d_long;             // the long-read list (ensure_long_cap)

	int launch(const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs, const uint32_t *d_lens,
	           uint64_t n_reads, hipStream_t st, bool may_long) override;
	int check() override;
	int result(uint32_t *counts, uint64_t *kmers) override;
	int clear() override;
};

// NULL for no handle and for a histogram counter.
static PanelCounter *panel(vc_ctx *c) { return dynamic_cast<PanelCounter *>(c); }

static int ensure_long_cap(PanelCounter *c, uint64_t seq_bytes)
{
	uint64_t need = seq_bytes / (VC_LONG_READ + 1) + 1;
	if (need <= c->d_long.cap) return VC_OK;
	if (need > 0xFFFFFFFFull) need = 0xFFFFFFFFull;
	HIPCK(hipStreamSynchronize(c->st));
	HIPCK(c->d_long.grow(need));
	return VC_OK;
}

// The key table, the filters and the outputs of an open context.
static int ctx_fill(PanelCounter *c, const uint64_t *keys, const uint32_t *vals, size_t n_keys)
{
	const int k = c->k;
	const uint32_t n_patterns = c->n_patterns;
	HIPCK(vc_kernel_setup());

	// exact table: 16-byte {key, value} slots, linear probing, load <= 1/2
	uint32_t tbits = 4;
	while (((uint64_t)1 << tbits) < 2 * (uint64_t)n_keys + 2) ++tbits;
	const uint64_t tslots = (uint64_t)1 << tbits;
	std::vector<vc_slot_t> tab(tslots, vc_slot_t{VC_EMPTY_KEY, 0u, 0u});
	// LDS prefilter: >= 24 bits per key, 1 KiB .. 128 KiB, 2 bits per key
	uint32_t wbits = 8;
	while (wbits < VC_MAX_FILTER_WBITS && ((uint64_t)32 << wbits) < 24 * (uint64_t)n_keys) ++wbits;
	const uint32_t fsh = vc_filter_shift(k, wbits);
	std::vector<uint32_t> fw((size_t)1 << wbits, 0);
	// second level: >= 40 bits per key, up to 2 MiB, when the LDS filter saturates
	uint32_t l2bits = 0;
	if (n_keys > VC_L2F_MIN_KEYS) {
		uint64_t bpk = 40;                                   // filter bits per key
		if (const char *e = getenv("VAFC_L2F_BITS_PER_KEY")) bpk = strtoull(e, nullptr, 10);   // A/B knob
		l2bits = 12;
		while (l2bits < VC_L2F_MAX_BITS && ((uint64_t)32 << l2bits) < bpk * (uint64_t)n_keys) ++l2bits;
	}
	std::vector<uint32_t> l2w(l2bits ? (size_t)1 << l2bits : 0, 0);
	uint64_t inserted = 0;
	for (size_t i = 0; i < n_keys; ++i) {
		const uint64_t key = keys[i];
		if (key == VC_EMPTY_KEY) continue;
		const uint32_t h = vc_hash(key);
		uint32_t s = vc_table_slot(h, tbits);
		bool dup = false;
		while (tab[s].key != VC_EMPTY_KEY) {
			if (tab[s].key == key) { dup = true; break; }
			s = (s + 1) & (uint32_t)(tslots - 1);
		}
		if (dup) continue;             // first occurrence wins
		tab[s].key = key;
		tab[s].val = vals[i];
		const uint32_t flo = (uint32_t)key, rlo = (uint32_t)vc_revcomp(key, k);
		fw[vc_filter_word(flo, rlo, fsh, wbits)] |= vc_filter_mask(flo, rlo);
		if (l2bits) l2w[vc_hash(key) >> (32 - l2bits)] |= vc_l2f_mask(vc_hash2(key));
		++inserted;
	}
	// flank bitmap instead of the Bloom filter (vafc_common.h) for k >= 21 and
	// no second level, when a random window's pass rate (about the fourth
	// power of the bitmap's density) stays under 1 %; VAFC_FILTER=bloom|flank forces
	// one (A/B and tests; flank only where k allows it)
	{
		const char *fe = getenv("VAFC_FILTER");
		const bool force_bloom = fe && !strcmp(fe, "bloom"), force_flank = fe && !strcmp(fe, "flank");
		// large panels, k >= 21: the 144 KiB Bloom filter (vafc_common.h
		// vc_big_word; the queues shrink to VC_BIG_QCAP); VAFC_FILTER=bloom128
		// keeps the 128 KiB power-of-two filter (A/B and tests)
		const bool force_b128 = fe && !strcmp(fe, "bloom128");
		if (k >= VC_FLANK_MIN_K && l2bits && !force_b128) {
			std::vector<uint32_t> fbig(VC_BIG_FILTER_WORDS, 0);
			for (const vc_slot_t &e : tab)
				if (e.key != VC_EMPTY_KEY) {
					const uint32_t flo = (uint32_t)e.key, rlo = (uint32_t)vc_revcomp(e.key, k);
					fbig[vc_big_word(flo, rlo, VC_BIG_FILTER_WORDS)] |= vc_filter_mask(flo, rlo);
				}
			fw.swap(fbig);
			c->big = 1;
			c->qcap = VC_BIG_QCAP;
			// the big kernels queue both strands' low words: key the second
			// level by them (vc_l2s_*) instead of the canonical k-mer
			std::fill(l2w.begin(), l2w.end(), 0u);
			for (const vc_slot_t &e : tab)
				if (e.key != VC_EMPTY_KEY) {
					const uint32_t flo = (uint32_t)e.key, rlo = (uint32_t)vc_revcomp(e.key, k);
					l2w[vc_l2s_hash(flo, rlo) >> (32 - l2bits)] |= vc_l2f_mask(vc_l2s_hash2(flo, rlo));
				}
		}
		if (k >= VC_FLANK_MIN_K && !l2bits && !force_bloom) {
			std::vector<uint32_t> fb((size_t)1 << VC_FLANK_WBITS, 0);
			for (const vc_slot_t &e : tab)
				if (e.key != VC_EMPTY_KEY) {
					vc_flank_mark(fb.data(), e.key, k);
					vc_flank_mark(fb.data(), vc_revcomp(e.key, k), k);
				}
			uint64_t set = 0;
			for (uint32_t w : fb) set += (uint64_t)__builtin_popcount(w);
			const double dens = (double)set / (double)((uint64_t)1 << (2 * VC_FLANK_BASES));
			if (force_flank || dens * dens * dens * dens <= 0.01) {
				fw.swap(fb);
				wbits = VC_FLANK_WBITS;
				c->flank = 1;
			}
		}
	}
	c->n_keys = inserted;
	c->tbits = tbits;
	c->wbits = wbits;
	c->fwords = (uint32_t)fw.size();
	c->l2bits = l2bits;
	c->fsh = fsh;
	c->ablate = getenv("VAFC_ABLATE") ? atoi(getenv("VAFC_ABLATE")) : 0;
	c->variant = getenv("VAFC_VARIANT") ? (uint32_t)atoi(getenv("VAFC_VARIANT")) : 0u;

	HIPCK(c->d_table.upload(tab.data(), tslots));
	HIPCK(c->d_filter.upload(fw.data(), fw.size()));
	HIPCK(c->own_counts.alloc(2 * (size_t)n_patterns + 2));
	HIPCK(c->own_counts.zero());
	HIPCK(c->own_tally.alloc(1));
	HIPCK(c->own_tally.zero());
	c->d_counts = c->own_counts;
	c->d_tally = c->own_tally;
	HIPCK(c->d_nlong.alloc(1));
	HIPCK(c->d_flags.alloc(1));
	HIPCK(c->d_flags.zero());
	HIPCK(c->d_pad.alloc(64));
	HIPCK(c->d_pad.zero());
	if (l2bits) HIPCK(c->d_l2f.upload(l2w.data(), l2w.size()));
	return ensure_long_cap(c, (uint64_t)1 << 30);
}

extern "C" int vc_create(vc_ctx **out, int k, const uint64_t *keys, const uint32_t *vals,
                         size_t n_keys, uint32_t n_patterns, int device)
{
	if (!out || k < 1 || k > 31 || (n_keys && (!keys || !vals))) return VC_EINVAL;
	*out = nullptr;
	PanelCounter *c = new (std::nothrow) PanelCounter;
	if (!c) return VC_ENOMEM;
	c->k = k;
	c->n_patterns = n_patterns;
	int rc = c->open(device);
	if (rc == VC_OK) rc = ctx_fill(c, keys, vals, n_keys);
	if (rc != VC_OK) {
		vc_destroy(c);
		return rc;
	}
	*out = c;
	return VC_OK;
}

extern "C" void vc_destroy(vc_ctx *c)
{
	if (!c) return;
	destroy_shards(c);
	c->close();
	for (VcSlot &s : c->islot) vc_slot_destroy(s);
	if (c->cst) (void)hipStreamDestroy(c->cst);
	delete c;
}

int PanelCounter::launch(const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs, const uint32_t *d_lens,
                         uint64_t n_reads, hipStream_t st, bool may_long)
{
	if (n_reads == 0) return VC_OK;
	if (n_reads > 0xFFFFFFFFull) return VC_EINVAL;   // the long-read list holds u32 read indices
	int rc = ensure_long_cap(this, seq_bytes);
	if (rc != VC_OK) return rc;
	VcKernelArgs A;
	const uintptr_t p = (uintptr_t)d_seq;
	A.seq = (const uint8_t *)(p & ~(uintptr_t)3);
	A.off_adj = (uint64_t)(p & 3u);
	A.seq_words = (seq_bytes + A.off_adj + 3) / 4;
	const bool tiny = A.seq_words < 4;     // the scan loads whole 16-byte quads
	if (tiny) {
		HIPCK(hipMemcpyAsync(d_pad, d_seq, seq_bytes, hipMemcpyDeviceToDevice, st));
		A.seq = d_pad;
		A.off_adj = 0;
		A.seq_words = 16;
	}
	A.offs = d_offs;
	A.lens = d_lens;
	A.n_reads = n_reads;
	A.table = d_table;
	A.tbits = tbits;
	A.tmask = (uint32_t)(((uint64_t)1 << tbits) - 1);
	A.filter = d_filter;
	A.wbits = wbits;
	A.fsh = fsh;
	A.flank = flank;
	A.big = big;
	A.fwords = fwords;
	A.qcap = qcap;
	A.l2f = d_l2f;
	A.l2bits = l2bits;
	A.ablate = ablate;
	A.variant = variant;
	A.nt4 = (uint32_t)nt4;
	A.k = k;
	A.kmask = ((uint64_t)1 << (2 * k)) - 1;
	A.counts = d_counts;
	A.tally = d_tally;
	A.nlong = d_nlong;
	A.longlist = d_long;
	A.long_cap = (uint32_t)d_long.cap;
	A.flags = d_flags;
	uint64_t groups = (n_reads + VC_BLOCK - 1) / VC_BLOCK;
	int grid = (int)(groups < (uint64_t)n_cu ? groups : (uint64_t)n_cu);
	if (may_long) HIPCK(d_nlong.zero_async(st));
	if (timing) HIPCK(timer.begin(st));
	HIPCK(vc_launch_count(&A, grid, may_long ? n_cu : 0, st));
	if (tiny) HIPCK(hipStreamSynchronize(st));   // d_pad is reused by the next tiny call
	if (timing) HIPCK(timer.end(st));
	return VC_OK;
}

extern "C" int vc_set_nt4_decode(vc_ctx *ctx, int on)
{
	PanelCounter *c = panel(ctx);
	if (!c) return VC_EINVAL;
	c->nt4 = on ? 1 : 0;
	for (vc_ctx *r : c->rep) panel(r)->nt4 = c->nt4;
	return VC_OK;
}

extern "C" int vc_count_device(vc_ctx *c, const uint8_t *d_seq, size_t seq_bytes,
                               const uint64_t *d_offs, const uint32_t *d_lens, uint64_t n_reads,
                               void *stream)
{
	if (!c || (n_reads && (!d_seq || !d_offs || !d_lens))) return VC_EINVAL;
	if (!c->rep.empty() && n_reads) {
		// a multi-shard counter deals device batches round robin, like host
		// batches, over the shards that live on the device holding the reads
		int d = c->dev;
		hipPointerAttribute_t at;
		if (hipPointerGetAttributes(&at, d_seq) == hipSuccess && at.type == hipMemoryTypeDevice) d = at.device;
		(void)hipGetLastError();   // a host pointer is not an error here
		vc_ctx *sh = nullptr;
		for (int i = 0; i < n_shards(c) && !sh; ++i) {
			vc_ctx *x = next_shard(c);
			if (x->dev == d) sh = x;
		}
		if (!sh) return VC_EINVAL;
		c = sh;
		++c->batches;
	}
	HIPCK(hipSetDevice(c->dev));
	return c->on_stream(stream, [&](hipStream_t st) { return c->launch(d_seq, seq_bytes, d_offs, d_lens, n_reads, st); });
}

int vc_ctx::submit(size_t bytes, uint64_t n_reads)
{
	return stage.submit(bytes, n_reads, st, [&](const VcSlot &s) {
		const int rc = launch(s.d_seq, bytes, s.d_offs, s.d_lens, n_reads, st, any_long(s.h_lens, n_reads));
		batches += rc == VC_OK ? 1 : 0;
		return rc;
	});
}

extern "C" int vc_count_block(vc_ctx *c, const uint8_t *seq, size_t seq_bytes, const uint64_t *offs,
                              const uint32_t *lens, uint64_t n_reads)
{
	if (!c || (n_reads && (!seq || !offs || !lens))) return VC_EINVAL;
	if (n_reads == 0) return VC_OK;
	for (uint64_t i = 0; i < n_reads; ++i)
		if (offs[i] + lens[i] > seq_bytes) return VC_EINVAL;
	c = next_shard(c);
	HIPCK(hipSetDevice(c->dev));
	VcSlot *s;
	const int rc = c->stage.acquire_for(seq_bytes, n_reads, &s);
	if (rc != VC_OK) return rc;
	memcpy(s->h_seq, seq, seq_bytes);
	memcpy(s->h_offs, offs, n_reads * sizeof(uint64_t));
	memcpy(s->h_lens, lens, n_reads * sizeof(uint32_t));
	return c->submit(seq_bytes, n_reads);
}

int PanelCounter::check()   // kernel error flags (a sync point anyway)
{
	uint32_t f = 0;
	HIPCK(hipSetDevice(dev));
	// the shard's stream also waits for its launches on caller
	// streams (vc_count_device), so this covers every batch without
	// waiting on the caller's unrelated work on the device
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipMemcpy(&f, d_flags, sizeof f, hipMemcpyDeviceToHost));
	if (f & 1u) {
		fprintf(stderr, "[E::vafc] more reads longer than %d bases than the long-read list holds "
		        "(overlapping device reads?): counts incomplete\n", VC_LONG_READ);
		return VC_EINVAL;
	}
	return VC_OK;
}

int PanelCounter::result(uint32_t *counts, uint64_t *kmers)
{
	if (counts)
		HIPCK(hipMemcpy(counts, d_counts, 2 * (size_t)n_patterns * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (kmers) {
		unsigned long long t = 0;
		HIPCK(hipMemcpy(&t, d_tally, sizeof(t), hipMemcpyDeviceToHost));
		*kmers = t;
	}
	return VC_OK;
}

extern "C" int vc_finish(vc_ctx *c, uint32_t *counts, uint64_t *kmers)
{
	if (!c) return VC_EINVAL;
	for (int i = 0; i < n_shards(c); ++i) {
		const int rc = shard_at(c, i)->check();
		if (rc != VC_OK) return rc;
	}
	if (!c->rep.empty()) {   // only a pattern counter has shards (vc_create_multi)
		int rc = reduce_shards(c, 2 * (size_t)panel(c)->n_patterns);
		if (rc != VC_OK) return rc;
	}
	HIPCK(hipSetDevice(c->dev));
	HIPCK(hipStreamSynchronize(c->st));
	c->stage.settle();
	return c->result(counts, kmers);
}

int PanelCounter::clear()
{
	HIPCK(hipMemsetAsync(d_counts, 0, 2 * (size_t)n_patterns * sizeof(uint32_t), st));
	HIPCK(hipMemsetAsync(d_tally, 0, sizeof(unsigned long long), st));
	HIPCK(hipMemsetAsync(d_flags, 0, sizeof(uint32_t), st));
	return VC_OK;
}

extern "C" int vc_reset(vc_ctx *c)
{
	if (!c) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	int rc = c->clear();
	for (size_t i = 0; rc == VC_OK && i < c->rep.size(); ++i) rc = vc_reset(c->rep[i]);
	return rc;
}

extern "C" void *vc_device_counts(vc_ctx *c) { return panel(c) ? (void *)panel(c)->d_counts : nullptr; }
extern "C" int vc_bind_outputs(vc_ctx *ctx, void *d_counts, void *d_tally)
{
	PanelCounter *c = panel(ctx);
	if (!c) return VC_EINVAL;
	c->d_counts = d_counts ? (uint32_t *)d_counts : c->own_counts;
	c->d_tally = d_tally ? (unsigned long long *)d_tally : c->own_tally;
	return VC_OK;
}

extern "C" void *vc_device_tally(vc_ctx *c) { return panel(c) ? (void *)panel(c)->d_tally : nullptr; }
extern "C" void *vc_stream(vc_ctx *c) { return c ? (void *)c->st : nullptr; }

extern "C" int vc_set_timing(vc_ctx *c, int enable)
{
	if (!c) return VC_EINVAL;
	c->timing = enable != 0;
	c->timer.clear();
	return VC_OK;
}

extern "C" int vc_kernel_ms(vc_ctx *c, float *ms) { return c ? c->timer.ms(ms) : VC_EINVAL; }

extern "C" int vc_table_info(const vc_ctx *ctx, uint64_t *n_keys, uint64_t *slots, uint64_t *filter_bytes)
{
	const PanelCounter *c = dynamic_cast<const PanelCounter *>(ctx);
	if (!c) return VC_EINVAL;
	if (n_keys) *n_keys = c->n_keys;
	if (slots) *slots = (uint64_t)1 << c->tbits;
	if (filter_bytes) *filter_bytes = (uint64_t)4 * c->fwords;
	return VC_OK;
}

// ---------------------------------------------------------------------------
// synthetic reads, misc
// ---------------------------------------------------------------------------

extern "C" int vc_synth_reads(uint8_t *d_seq, uint64_t *d_offs, uint32_t *d_lens, uint64_t first,
                              uint64_t n_reads, uint32_t read_len, uint64_t seed, double f_snp,
                              const uint8_t *d_windows, const uint8_t *d_dosage, uint32_t n_snp,
                              void *stream)
{
	if (read_len < 1 || read_len > 301 || (n_snp && (!d_windows || !d_dosage))) return VC_EINVAL;
	double t = f_snp * 4294967296.0;
	uint64_t thr = t <= 0 ? 0 : (t >= 4294967296.0 ? (uint64_t)1 << 32 : (uint64_t)llround(t));
	HIPCK(vc_launch_synth(d_seq, d_offs, d_lens, first, n_reads, read_len, seed, thr, d_windows,
	                      d_dosage, n_snp, (hipStream_t)stream));
	return VC_OK;
}

// Test hook: device decode of whole reads to codes (0..3, 4 = invalid).
extern "C" int vc_debug_decode(const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs,
                               const uint32_t *d_lens, uint64_t n_reads, uint8_t *d_codes, void *stream)
{
	HIPCK(vc_launch_decode(d_seq, seq_bytes, d_offs, d_lens, n_reads, d_codes, (hipStream_t)stream));
	return VC_OK;
}

extern "C" const char *vc_strerror(int err)
{
	switch (err) {
	case VC_OK: return "ok";
	case VC_EINVAL: return "invalid argument";
	case VC_ENOMEM: return "out of host memory";
	case VC_EHIP: return "HIP runtime error";
	case VC_ENODEV: return "no HIP device";
	case VC_EIO: return "file could not be opened";
	case VC_ETOOMANY: return "too many patterns";
	case VC_EFULL: return "k-mer table full";
	default: return "unknown error";
	}
}

extern "C" int vc_version(void) { return VAFC_VERSION_MAJOR * 100 + VAFC_VERSION_MINOR; }
