// vafc_files.cpp -- the file passes of a read counter of either kind
// (count_fastq_kmers, vaf-counter.c:482-582): vc_count_file, its byte ranges
// and gzip shares, and the host-only scans.  Small inputs go through the
// sequential reader and the core's stager; plain and gzip files of size
// through the parallel reader (vafc_ingest.h), whose pinned slots DeviceSink
// ships to the shards.  The kernels are reached through vc_ctx::launch.
#include <ctype.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "vafc_ctx.h"
#include "vafc_fastq.h"
#include "vafc_gzip.h"
#include "vafc_ingest.h"

#ifndef VC_BATCH_BYTES
#define VC_BATCH_BYTES ((size_t)64 << 20)
#endif

// ---------------------------------------------------------------------------
// parallel ingest of plain files (vafc_ingest.h): pieces parsed by -t worker
// threads straight into pinned slots, shipped to the device in file order
// ---------------------------------------------------------------------------

#ifndef VC_PIECE_BYTES
#define VC_PIECE_BYTES ((uint64_t)16 << 20)
#endif
#ifndef VC_PIECE_BYTES_WARM
#define VC_PIECE_BYTES_WARM ((uint64_t)32 << 20)
#endif

static int ingest_slot_alloc(VcSlot &s, uint64_t piece);
static size_t ingest_slot_bytes(uint64_t piece);

namespace {

// Slot g of the reader lives on shard g % N (slot index g / N there), so the
// pieces of a file go round robin over the shards.
class DeviceSink : public VcIngestSink {
public:
	DeviceSink(vc_ctx *c, uint64_t piece) : c_(c), n_(n_shards(c)), piece_(piece) {}
	int acquire(int slot, VcSlotBuf *b) override
	{
		vc_ctx *sh;
		VcSlot &s = at(slot, &sh);
		HIPCK(hipSetDevice(sh->dev));
		int rc = vc_slot_wait(s);
		if (rc != VC_OK) return rc;
		// first use of the slot (reserve_ingest_slots, alloc = false), or
		// buffers sized for smaller pieces than this pass's
		if (!s.h_seq || s.cap_bytes < ingest_slot_bytes(piece_)) rc = ingest_slot_alloc(s, piece_);
		if (rc == VC_OK) fill(s, b);
		return rc;
	}
	int grow(int slot, VcSlotBuf *b, size_t bytes, size_t reads, size_t used_bytes, size_t used_reads) override
	{
		vc_ctx *sh;
		VcSlot &s = at(slot, &sh);
		HIPCK(hipSetDevice(sh->dev));
		const int rc = vc_slot_realloc(s, bytes, reads, used_bytes, used_reads);   // exact sizes: the reader's growth rule
		if (rc == VC_OK) fill(s, b);
		return rc;
	}
	// The copies go on the shard's copy stream and the kernels on its own
	// stream, ordered by one event per slot: the DMA engine streams the pieces
	// back to back instead of waiting for each piece's kernel.  A slot's next
	// copy comes after the worker has waited for its `done` (the kernel that
	// read its device buffers).
	int submit(int slot, const VcSlotBuf &, uint64_t n, uint64_t bytes) override
	{
		vc_ctx *sh;
		VcSlot &s = at(slot, &sh);
		HIPCK(hipSetDevice(sh->dev));
		if (!sh->cst) HIPCK(hipStreamCreateWithFlags(&sh->cst, hipStreamNonBlocking));
		if (!s.copied) HIPCK(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
		HIPCK(hipMemcpyAsync(s.d_seq, s.h_seq, bytes, hipMemcpyHostToDevice, sh->cst));
		HIPCK(hipMemcpyAsync(s.d_offs, s.h_offs, n * sizeof(uint64_t), hipMemcpyHostToDevice, sh->cst));
		HIPCK(hipMemcpyAsync(s.d_lens, s.h_lens, n * sizeof(uint32_t), hipMemcpyHostToDevice, sh->cst));
		HIPCK(hipEventRecord(s.copied, sh->cst));
		HIPCK(hipStreamWaitEvent(sh->st, s.copied, 0));
		int rc = sh->launch(s.d_seq, bytes, s.d_offs, s.d_lens, n, sh->st, any_long(s.h_lens, n));
		if (rc != VC_OK) return rc;
		HIPCK(hipEventRecord(s.done, sh->st));
		s.pending = true;
		++sh->batches;
		return VC_OK;
	}

private:
	vc_ctx *c_;
	int n_;
	uint64_t piece_;
	VcSlot &at(int slot, vc_ctx **sh)
	{
		*sh = shard_at(c_, slot % n_);
		return (*sh)->islot[(size_t)(slot / n_)];
	}
	static void fill(const VcSlot &s, VcSlotBuf *b)
	{
		b->seq = s.h_seq;
		b->offs = s.h_offs;
		b->lens = s.h_lens;
		b->cap_bytes = s.cap_bytes;
		b->cap_reads = s.cap_reads;
	}
};

} // namespace

// Plain files of at least this size take the parallel reader.
#ifndef VC_PARALLEL_MIN_BYTES
#define VC_PARALLEL_MIN_BYTES ((uint64_t)32 << 20)
#endif

static int clamp_threads(int n) { return n < 1 ? 1 : (n > 64 ? 64 : n); }

// Pinned + device buffers of the parallel reader's slots (2 x threads slots of
// one piece each: sequence bytes at about half a FASTQ piece, growing on
// demand for FASTA), rounded up to a multiple of the shards and spread over
// them.  Returns the reader's slot count (> 0) or an error (< 0).
static int reserve_ingest_slots(vc_ctx *c, size_t slots, bool alloc);

static int reserve_ingest(vc_ctx *c, int threads, bool alloc)
{
	const int N = n_shards(c);
	// two slots per worker: a piece that finishes late holds back only its
	// own slot while the others parse ahead (threads + 2 slots left the
	// workers waiting for slots 2-3x as long: profiles/r04l_slots_ab.json)
	const char *e = getenv("VAFC_INGEST_SLOTS");   // A/B knob: the reader's slot count (> threads)
	const int want = e && atoi(e) > threads ? atoi(e) : (threads < 2 ? threads + 2 : 2 * threads);
	const int slots = (want + N - 1) / N * N;
	for (int i = 0; i < N; ++i) {
		vc_ctx *sh = shard_at(c, i);
		HIPCK(hipSetDevice(sh->dev));
		int rc = reserve_ingest_slots(sh, (size_t)(slots / N), alloc);
		if (rc != VC_OK) return rc;
	}
	return slots;
}

// One slot's buffers.  FASTQ: at most half of a piece's records' text is
// sequence (the quality line is as long); FASTA and long records grow the slot.
static size_t ingest_slot_bytes(uint64_t piece) { return (size_t)piece / 2 + ((size_t)256 << 10); }

// A slot's pinned buffers as one anonymous mapping on transparent huge pages,
// touched and registered with hipHostRegister, and its device buffers as one
// allocation: pinning 32 slots of a 16 MB piece took 0.018 s this way against
// 0.041-0.057 s as three hipHostMalloc + three hipMalloc each, at the same
// 52 GB/s H2D (tools/pin_probe.hip, profiles/r06b_pin_probe.log).  The CLI pins
// its slots inside the counting timer, as the reference allocates its block
// buffers inside it.  VAFC_PIN=malloc keeps hipHostMalloc (A/B).
static int slot_alloc_mapped(VcSlot &s, size_t bytes, size_t reads)
{
	const size_t huge = (size_t)2 << 20;
	const size_t ob = (bytes + 63) / 64 * 64, lb = ob + reads * sizeof(uint64_t);
	const size_t need = lb + reads * sizeof(uint32_t);
	const size_t len = (need + huge - 1) / huge * huge;
	void *m = mmap(nullptr, len + huge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
	if (m == MAP_FAILED) return VC_ENOMEM;
	// the 2 MB-aligned part only (the slack before and after goes back)
	uint8_t *a = (uint8_t *)(((uintptr_t)m + huge - 1) / huge * huge);
	if (a > (uint8_t *)m) munmap(m, (size_t)(a - (uint8_t *)m));
	const size_t tail = (size_t)((uint8_t *)m + len + huge - (a + len));
	if (tail) munmap(a + len, tail);
	madvise(a, len, MADV_HUGEPAGE);
	for (size_t i = 0; i < len; i += 4096) a[i] = 0;   // fault the pages in (huge pages where granted)
	if (hipHostRegister(a, len, hipHostRegisterDefault) != hipSuccess) {
		(void)hipGetLastError();
		munmap(a, len);
		return VC_EHIP;
	}
	uint8_t *d = nullptr;
	if (hipMalloc(&d, need) != hipSuccess) {
		(void)hipGetLastError();
		(void)hipHostUnregister(a);
		munmap(a, len);
		return VC_EHIP;
	}
	s.map = a;
	s.map_len = len;
	s.h_seq = a;
	s.h_offs = (uint64_t *)(a + ob);
	s.h_lens = (uint32_t *)(a + lb);
	s.d_seq = d;
	s.d_offs = (uint64_t *)(d + ob);
	s.d_lens = (uint32_t *)(d + lb);
	s.d_one = true;
	s.cap_bytes = bytes;
	s.cap_reads = reads;
	return VC_OK;
}

static int ingest_slot_alloc(VcSlot &s, uint64_t piece)
{
	static const bool use_malloc = getenv("VAFC_PIN") && !strcmp(getenv("VAFC_PIN"), "malloc");
	const size_t bytes = ingest_slot_bytes(piece), reads = (size_t)piece / 256 + 4096;
	if (use_malloc) return vc_slot_reserve(s, bytes, reads);
	if (bytes <= s.cap_bytes && reads <= s.cap_reads) return VC_OK;
	const int rc = vc_slot_wait(s);
	if (rc != VC_OK) return rc;
	vc_slot_free(s);
	return slot_alloc_mapped(s, bytes + bytes / 4 + 4096, reads + reads / 4 + 1024);
}

// alloc = false: only the slot records and their events; each slot's buffers
// are then allocated by the worker that first fills it (DeviceSink::acquire),
// so pinning them overlaps the other workers' parsing instead of preceding it.
static int reserve_ingest_slots(vc_ctx *c, size_t slots, bool alloc)
{
	if (c->islot.size() < slots) {
		HIPCK(hipStreamSynchronize(c->st));
		const size_t old = c->islot.size();
		c->islot.resize(slots);
		for (size_t i = old; i < slots; ++i)
			HIPCK(hipEventCreateWithFlags(&c->islot[i].done, hipEventDisableTiming));
	}
	for (size_t i = 0; alloc && i < slots; ++i) {
		VcSlot &s = c->islot[i];
		if (s.h_seq) continue;
		int rc = ingest_slot_alloc(s, VC_PIECE_BYTES);
		if (rc != VC_OK) return rc;
	}
	return VC_OK;
}

extern "C" int vc_reserve_file_ingest(vc_ctx *c, int n_threads)
{
	if (!c) return VC_EINVAL;
	const int rc = reserve_ingest(c, clamp_threads(n_threads), true);
	return rc < 0 ? rc : VC_OK;
}

static int count_file_parallel(vc_ctx *c, int fd, uint64_t size, int block_bases, int n_threads,
                               vc_file_stats &st, VcTextRange *range = nullptr)
{
	const int threads = clamp_threads(n_threads);
	const int slots = reserve_ingest(c, threads, false);
	if (slots < 0) return slots;
	// pieces of 16 MB while the counter's slots are first pinned (the pinning
	// is paid inside the pass, by the workers); once a pass has pinned them,
	// later passes and files use 32 MB pieces (the slots grow once): half the
	// copies, kernels and events per byte (profiles/r05i_*: 39.7-40.5 against
	// 35.5-36.1 Gbases/s in one process; in a fresh CLI process the 32 MB
	// slots' pinning made the pass 40 % slower, profiles/r05i_cli_piece_ab.json)
	const uint64_t piece = vc_ingest_piece(c->ingest_warm ? VC_PIECE_BYTES_WARM : VC_PIECE_BYTES);
	DeviceSink sink(c, piece);
	const int rc = vc_ingest_plain(fd, size, c->k, block_bases, threads, slots, piece, sink, st, range);
	if (rc == VC_OK) c->ingest_warm = true;
	return rc;
}

// gzip input: the text the parallel inflater produces (n_threads workers) is
// parsed by the parallel reader's workers, fewer of them (vc_gz_parse_threads).
static int count_file_gzip(vc_ctx *c, VcGzParallel *g, int block_bases, int n_threads, vc_file_stats &st)
{
	const int parsers = vc_gz_parse_threads(clamp_threads(n_threads));
	const int slots = reserve_ingest(c, parsers, false);
	if (slots < 0) return slots;
	const uint64_t piece = vc_ingest_piece(VC_PIECE_BYTES);
	DeviceSink sink(c, piece);
	return vc_ingest_gzip(g, c->k, block_bases, parsers, slots, piece, (uint64_t)(slots + 2) * piece * 2, sink, st);
}

// Wait for every shard's queued batches.
static int sync_shards(vc_ctx *c)
{
	for (int i = 0; i < n_shards(c); ++i) {
		vc_ctx *sh = shard_at(c, i);
		HIPCK(hipSetDevice(sh->dev));
		HIPCK(hipStreamSynchronize(sh->st));
	}
	return hipSetDevice(c->dev) == hipSuccess ? VC_OK : VC_EHIP;
}

// CPUs of the NUMA node(s) the counter's GPUs hang off (sysfs, from each
// device's PCI bus id), within this process's affinity mask (vafc_affinity.h).
// Off when VAFC_NUMA=0, when sysfs says nothing, or when the node offers fewer
// CPUs of the mask than the reader has threads (or than the whole mask).
static VcCpuSet gpu_cpus(vc_ctx *c, int threads)
{
	if (c->cpus_threads == threads) return c->cpus;
	VcCpuSet out;
	const char *ne = getenv("VAFC_NUMA");
	cpu_set_t mask;
	CPU_ZERO(&out.set);
	if (!(ne && !strcmp(ne, "0")) && sched_getaffinity(0, sizeof mask, &mask) == 0) {
		bool any_node = false, bad = false;
		for (int i = 0; i < n_shards(c) && !bad; ++i) {
			char bus[64] = {0}, path[256], buf[4096];
			if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, shard_at(c, i)->dev) != hipSuccess) {
				(void)hipGetLastError();
				bad = true;
				break;
			}
			for (char *q = bus; *q; ++q) *q = (char)tolower((unsigned char)*q);
			snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
			FILE *f = fopen(path, "r");
			int node = -1;
			if (!f || fscanf(f, "%d", &node) != 1) node = -1;
			if (f) fclose(f);
			if (node < 0) {
				bad = true;
				break;
			}
			snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
			f = fopen(path, "r");
			size_t n = f ? fread(buf, 1, sizeof buf - 1, f) : 0;
			if (f) fclose(f);
			buf[n] = 0;
			for (char *q = buf; *q;) {   // "0-63,128-191"
				char *e;
				const long a = strtol(q, &e, 10);
				if (e == q) break;
				long b = a;
				if (*e == '-') b = strtol(e + 1, &e, 10);
				for (long x = a; x <= b && x < CPU_SETSIZE; ++x) CPU_SET((int)x, &out.set);
				any_node = true;
				q = *e == ',' ? e + 1 : e;
				if (*e != ',') break;
			}
		}
		if (!bad && any_node) {
			CPU_AND(&out.set, &out.set, &mask);
			const int have = CPU_COUNT(&out.set);
			out.on = have >= threads && have < CPU_COUNT(&mask);
		}
	}
	c->cpus = out;
	c->cpus_threads = threads;
	return out;
}

// The CPUs for the reader threads of a pass with `threads` (clamped) of them,
// on the GPU's NUMA node when it has a CPU for each: the parse workers, or
// for gzip the inflaters, the parsers of the inflated text, the pump and the
// block loop.
static VcCpuSet reader_cpus(vc_ctx *c, int threads, bool gz)
{
	return gpu_cpus(c, gz ? vc_gz_inflate_threads(threads) + vc_gz_parse_threads(threads) + 2 : threads);
}

namespace {

// What every file pass keeps: its stats, zeroed, and its start.
struct FilePass {
	vc_ctx *c;                 // NULL: nothing was queued on a device (vc_scan_file)
	vc_file_stats *out;
	vc_file_stats st = {0, 0, 0, 0.0};
	double t0 = vc_now();

	FilePass(vc_ctx *ctx, vc_file_stats *o) : c(ctx), out(o) {}
	// Every exit of a pass: wait for the shards' queued batches, stop the clock
	// and hand the stats out.
	int finish(int rc)
	{
		if (rc == VC_OK && c) rc = sync_shards(c);
		st.seconds = vc_now() - t0;
		if (out) *out = st;
		return rc;
	}
};

struct FileKind {
	int fd = -1;               // open iff the path is a regular file: the caller closes it
	bool regular = false, gzip = false;
	uint64_t size = 0;
};

// A path that is not a regular file (a FIFO, a device) is never opened here:
// it is opened exactly once, by the sequential reader; opening it only to look
// at it would let a pipe's writer see its reader go away (a pipe is read once,
// as the reference does).  False: the path cannot be read.
bool classify(const char *path, FileKind *f)
{
	struct stat sb;
	if (stat(path, &sb) != 0) return false;
	if (!S_ISREG(sb.st_mode)) return true;
	if ((f->fd = open(path, O_RDONLY)) < 0) return false;
	uint8_t magic[2] = {0, 0};
	f->regular = fstat(f->fd, &sb) == 0 && S_ISREG(sb.st_mode);
	f->gzip = f->regular && pread(f->fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
	f->size = f->regular ? (uint64_t)sb.st_size : 0;
	return true;
}

} // namespace

extern "C" int vc_count_file(vc_ctx *c, const char *path, int block_bases, int n_threads,
                             vc_file_stats *st)
{
	if (!c || !path) return VC_EINVAL;
	HIPCK(hipSetDevice(c->dev));
	FilePass fp(c, st);
	FileKind f;
	if (!classify(path, &f)) return fp.finish(VC_EIO);
	const int t = clamp_threads(n_threads);
	VcAffinityScope placement(reader_cpus(c, t, f.gzip));
	const char *me = getenv("VAFC_INGEST_MIN");        // test knob: smallest file for the parallel reader
	const uint64_t min_bytes = me ? (uint64_t)atoll(me) : VC_PARALLEL_MIN_BYTES;
	if (f.regular && !f.gzip && f.size >= min_bytes && f.size > 0) {
		const int rc = count_file_parallel(c, f.fd, f.size, block_bases, n_threads, fp.st);
		close(f.fd);
		return fp.finish(rc);
	}
	if (f.fd >= 0) close(f.fd);
	if (f.gzip) {   // parallel inflate + parallel parse (falls through if the inflater declines the file)
		VcGzParallel *g = vc_gzp_open(path, vc_gz_inflate_threads(t), vc_gz_chunk());
		if (g) {
			const int rc = count_file_gzip(c, g, block_bases, n_threads, fp.st);
			vc_gzp_close(g);
			return fp.finish(rc);
		}
	}
	VcFastqReader rd;   // small plain files, pipes, gzip the inflater declines
	if (!rd.open_parallel(path, t)) return fp.finish(VC_EIO);
	// with several shards each batch goes to the next shard (its own slots,
	// stream and device)
	const size_t limit = vc_batch_bytes(VC_BATCH_BYTES);
	VcBatchWriter bw(limit, limit / 64, [c]() -> vc_ctx * {
		vc_ctx *sh = next_shard(c);
		return hipSetDevice(sh->dev) == hipSuccess ? sh : nullptr;
	});
	int rc = vc_block_loop(rd, c->k, block_bases, [&bw](const char *s, size_t l) { return bw.add(s, l); }, fp.st);
	if (rc == VC_OK) rc = bw.flush();
	return fp.finish(rc);
}

extern "C" int vc_count_file_range(vc_ctx *c, const char *path, uint64_t begin, uint64_t end, int block_bases,
                                   int n_threads, vc_file_stats *st, vc_range_info *ri)
{
	if (!c || !path || !ri || end <= begin) return VC_EINVAL;
	*ri = vc_range_info{UINT64_MAX, UINT64_MAX, 0, 0, 1};
	HIPCK(hipSetDevice(c->dev));
	FilePass fp(c, st);
	FileKind f;
	if (!classify(path, &f)) return fp.finish(VC_EIO);
	if (!f.regular || f.gzip) {   // not split: the first range counts the whole file
		if (f.fd >= 0) close(f.fd);
		int rc = VC_OK;
		if (begin == 0) {
			rc = vc_count_file(c, path, block_bases, n_threads, &fp.st);
			if (rc == VC_OK) *ri = vc_range_info{0, UINT64_MAX, 0, 1, 1};
		}
		return fp.finish(rc);
	}
	VcTextRange R;
	R.begin = begin;
	R.end = end;
	int rc;
	{
		VcAffinityScope placement(reader_cpus(c, clamp_threads(n_threads), false));
		rc = count_file_parallel(c, f.fd, f.size, block_bases, n_threads, fp.st, &R);
	}
	close(f.fd);
	*ri = vc_range_info{R.first, R.next, R.errs, R.stopped ? 1u : 0u, 0u};
	return fp.finish(rc);
}

// One share of a gzip file (include/vafc.h, vafc_gzip.h): the inflater (from
// the share's first block with its known window, or a held share resumed),
// the parallel reader over the share's text as a range (plus the previous
// byte, for the first guess).  Takes g and closes it.
static int count_gz_share_g(vc_ctx *c, VcGzParallel *g, int fmt, int parsers, int first_share,
                            const uint8_t *window, uint64_t text_len, int block_bases, vc_file_stats &local,
                            vc_range_info *ri, vc_gz_share_crc *crc)
{
	int rc = reserve_ingest(c, parsers, false);
	VcTextRange R;
	const size_t np = first_share ? 0 : 1;
	if (rc >= 0) {
		const int slots = rc;
		const uint64_t piece = vc_ingest_piece(VC_PIECE_BYTES);
		DeviceSink sink(c, piece);
		R.begin = np;
		R.end = np + text_len;
		R.format = fmt;
		rc = vc_ingest_gzip_share(g, first_share ? nullptr : window + 32767, np, c->k, block_bases, parsers, slots,
		                          piece, (uint64_t)(slots + 2) * piece * 2, sink, local, &R);
	}
	VcGzShareCrc sc;
	vc_gzp_share_crc(g, &sc);
	vc_gzp_close(g);
	*ri = vc_range_info{R.first == UINT64_MAX ? UINT64_MAX : R.first - np,
	                    R.next == UINT64_MAX ? UINT64_MAX : R.next - np - text_len, R.errs, R.stopped ? 1u : 0u, 0u};
	*crc = vc_gz_share_crc{sc.events, sc.head_crc, sc.head_len, sc.head_expect_crc, sc.head_expect_isize,
	                       sc.tail_crc, sc.tail_len, sc.crc_error, sc.complete};
	return rc;
}

extern "C" int vc_count_gz_share(vc_ctx *c, const char *path, int first_share, uint64_t start_bit,
                                 const uint8_t *window, uint64_t text_len, int block_bases, int n_threads,
                                 vc_file_stats *st, vc_range_info *ri, vc_gz_share_crc *crc)
{
	if (!c || !path || !ri || !crc || text_len == 0 || (!first_share && !window)) return VC_EINVAL;
	*ri = vc_range_info{UINT64_MAX, UINT64_MAX, 0, 0, 0};
	memset(crc, 0, sizeof *crc);
	HIPCK(hipSetDevice(c->dev));
	FilePass fp(c, st);
	const int fmt = vc_gz_text_format(path);
	if (fmt < 0) return fp.finish(VC_EINVAL);
	const int t = clamp_threads(n_threads);
	VcAffinityScope placement(reader_cpus(c, t, true));
	VcGzParallel *g = vc_gzp_open_share(path, vc_gz_inflate_threads(t), vc_gz_chunk(), first_share != 0, start_bit,
	                                    window, text_len);
	if (!g) return fp.finish(VC_EIO);
	return fp.finish(count_gz_share_g(c, g, fmt, vc_gz_parse_threads(t), first_share, window, text_len, block_bases,
	                                  fp.st, ri, crc));
}

extern "C" int vc_gz_share_open(vc_ctx *c, const char *path, uint64_t begin, uint64_t end, int n_threads,
                                uint64_t chunk_bytes, uint64_t hold_bytes, vc_gz_share_info *out,
                                uint16_t *window_sym, vc_gz_share **held)
{
	if (!path || !out || !held || end <= begin) return VC_EINVAL;
	*held = nullptr;
	const int t = n_threads < 1 ? 1 : n_threads;
	// the scan's threads where the count's will run (the GPU's NUMA node):
	// the chunks they keep are first touched there, so the count reads them
	// from local memory
	VcCpuSet none;
	CPU_ZERO(&none.set);
	if (c) HIPCK(hipSetDevice(c->dev));
	VcAffinityScope placement(c ? reader_cpus(c, clamp_threads(t), true) : none);
	VcGzShare sh;
	VcGzParallel *g = nullptr;
	if (!vc_gzp_scan_share_hold(path, t, chunk_bytes, begin, end, hold_bytes, &sh, window_sym, &g)) return VC_EIO;
	out->start_bit = sh.start_bit;
	out->end_bit = sh.end_bit;
	out->text_len = sh.text_len;
	out->ok = sh.ok ? 1u : 0u;
	out->ended = sh.start_bit != UINT64_MAX && sh.end_bit == UINT64_MAX ? 1u : 0u;
	if (g) {
		vc_gz_share *h = new vc_gz_share;
		h->g = g;
		h->format = vc_gz_text_format(path);
		h->threads = t;
		*held = h;
	}
	return VC_OK;
}

extern "C" int vc_count_gz_share_held(vc_ctx *c, vc_gz_share *h, int first_share, const uint8_t *window,
                                      uint64_t text_len, int block_bases, int n_threads, vc_file_stats *st,
                                      vc_range_info *ri, vc_gz_share_crc *crc)
{
	if (!c || !h || !h->g || !ri || !crc || text_len == 0 || (!first_share && !window)) return VC_EINVAL;
	*ri = vc_range_info{UINT64_MAX, UINT64_MAX, 0, 0, 0};
	memset(crc, 0, sizeof *crc);
	HIPCK(hipSetDevice(c->dev));
	FilePass fp(c, st);
	if (h->format < 0) return fp.finish(VC_EINVAL);
	const int t = clamp_threads(n_threads);
	VcAffinityScope placement(reader_cpus(c, t, true));
	VcGzParallel *g = h->g;
	h->g = nullptr;   // counted once; count_gz_share_g closes it
	if (!vc_gzp_resume_share(g, first_share ? nullptr : window, text_len)) {
		vc_gzp_close(g);
		return fp.finish(VC_EINVAL);
	}
	return fp.finish(count_gz_share_g(c, g, h->format, vc_gz_held_parse_threads(t), first_share, window, text_len,
	                                  block_bases, fp.st, ri, crc));
}

extern "C" int vc_scan_file(const char *path, int k, int block_bases, vc_file_stats *st,
                            uint8_t *seq_out, size_t seq_cap, uint32_t *lens_out, size_t lens_cap)
{
	if (!path || !st) return VC_EINVAL;
	FilePass fp(nullptr, st);
	VcFastqReader rd;
	if (!rd.open(path)) return fp.finish(VC_EIO);
	size_t nb = 0, nr = 0;
	return fp.finish(vc_block_loop(rd, k, block_bases, [&](const char *s, size_t l) {
		if (seq_out && nb + l <= seq_cap) memcpy(seq_out + nb, s, l);
		if (lens_out && nr < lens_cap) lens_out[nr] = (uint32_t)l;
		nb += l;
		++nr;
		return VC_OK;
	}, fp.st));
}

extern "C" int64_t vc_scan_records(const char *path, int32_t *rets, int64_t cap)
{
	if (!path) return VC_EINVAL;
	VcFastqReader rd;
	if (!rd.open(path)) return VC_EIO;
	int64_t n = 0;
	int ret;
	do {
		ret = rd.next();
		if (n < cap && rets) rets[n] = ret;
		++n;
	} while (ret != -1);
	return n;
}
