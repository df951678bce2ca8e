/*
 * vafc.h -- C ABI of the MI355X-native vaf-counter hot path (libvafc.so).
 *
 * The reference (gerbenvoshol/kmer-cnt, vaf-counter.c) is a monolithic C
 * program with no plugin/FFI API; its in-process seam is
 *
 *     void count_fastq_kmers(const char *fn, int k, int n_thread, int block_size,
 *                            kmer_cnt_t *kmer_map, pattern_db_t *db);   // vaf-counter.c:550
 *
 * fed by load_patterns() (vaf-counter.c:149) and create_combined_kmer_map()
 * (vaf-counter.c:198), with steps 1+2 of its pipeline (extract k-mers
 * vaf-counter.c:519-535, look up + increment vaf-counter.c:537-544) as the hot
 * path.  This header is that seam re-cut at a device boundary: plain pointers
 * and sizes, no torch or HIP types, C linkage.  Every entry point names the
 * reference interface it replaces.
 *
 * Counts layout: uint32 counts[2*n_patterns], REF of pattern i at [2i], ALT at
 * [2i+1] -- i.e. indexed by the reference's map value (i<<1)|is_alt
 * (vaf-counter.c:227,239).  Counts wrap modulo 2^32 exactly like the
 * reference's uint32 fields (vaf-counter.c:101-102,473-477).
 *
 * Errors: 0 = ok, <0 = VC_E* below; vc_strerror() gives text.  HIP failures
 * are reported, never silently degraded to a CPU path.
 */
#ifndef VAFC_H
#define VAFC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAFC_VERSION_MAJOR 0
#define VAFC_VERSION_MINOR 1

enum {
	VC_OK = 0,
	VC_EINVAL = -1,      /* bad argument (k outside 1..31, NULL pointer, ...) */
	VC_ENOMEM = -2,      /* host allocation failed */
	VC_EHIP = -3,        /* HIP runtime / kernel launch error */
	VC_ENODEV = -4,      /* no usable GPU */
	VC_EIO = -5,         /* file could not be opened / read */
	VC_ETOOMANY = -6,    /* more than INT32_MAX>>1 patterns (vaf-counter.c:205-209) */
	VC_EFULL = -7        /* k-mer histogram: more distinct k-mers than the table holds */
};

typedef struct vc_ctx vc_ctx;
typedef struct vc_patterns vc_patterns;

/* ------------------------------------------------------------------ */
/* Pattern database -- replaces load_patterns (vaf-counter.c:149-184)  */
/* and create_combined_kmer_map (vaf-counter.c:198-252).               */
/* ------------------------------------------------------------------ */

/* Load patterns.txt (records "chr start end rsid ref alt ref_kmer alt_kmer",
 * read with the reference's fscanf conversion; reading stops at the first
 * record that does not convert completely).  Returns VC_EIO if the file
 * cannot be opened (the reference then exits 1, vaf-counter.c:624-627). */
int vc_patterns_load(const char *path, vc_patterns **out);
void vc_patterns_free(vc_patterns *db);
int vc_patterns_count(const vc_patterns *db);

/* Canonical 2-bit keys and values (i<<1)|is_alt in insertion order (ref of
 * pattern i, then alt of pattern i), first insert wins, keys of strings with a
 * non-ACGTU character among their first k skipped.  *keys / *vals are malloc'd
 * (caller frees with vc_free).  *n_collisions = duplicate inserts ignored. */
int vc_patterns_keys(const vc_patterns *db, int k, uint64_t **keys, uint32_t **vals,
                     size_t *n_keys, int *n_collisions);

/* Write the .vaf file (vaf-counter.c:653-681): header "# Average depth",
 * column line, one row per pattern in file order. counts as above. */
int vc_write_vaf(const vc_patterns *db, const uint32_t *counts, const char *path);

/* Field access for host-side mirrors (Python): returns 0 and fills the
 * pointers (valid until vc_patterns_free). */
int vc_pattern_fields(const vc_patterns *db, int i, const char **chr, int *start,
                      const char **rsid, char *ref, char *alt,
                      const char **ref_kmer, const char **alt_kmer);

void vc_free(void *p);

/* ------------------------------------------------------------------ */
/* Device counter -- replaces the kmer_cnt_t map + pattern_t counters  */
/* (vaf-counter.c:67,92-108) and steps 1+2 of worker_pipeline          */
/* (vaf-counter.c:519-544, worker_lookup :449-479).                    */
/* ------------------------------------------------------------------ */

/* Create a counter on HIP device `device` for k in 1..31 from (key, value)
 * pairs as produced by vc_patterns_keys (first occurrence of a key wins).
 * The static key table and its LDS prefilter are built on the host and copied
 * once to HBM.  Counts start at zero. */
int vc_create(vc_ctx **out, int k, const uint64_t *keys, const uint32_t *vals,
              size_t n_keys, uint32_t n_patterns, int device);
void vc_destroy(vc_ctx *ctx);

/* Count one block of host-resident reads (asynchronous; accumulates).
 * seq: raw read bytes exactly as the FASTA/Q parser returned them (the
 * position-dependent 2-bit decode of vaf-counter.c:261-291 is applied on the
 * device); read i is seq[offs[i] .. offs[i]+lens[i]).  The caller may reuse
 * its buffers as soon as the call returns (they are staged into pinned
 * memory).  Reads shorter than k contribute nothing. */
int vc_count_block(vc_ctx *ctx, const uint8_t *seq, size_t seq_bytes,
                   const uint64_t *offs, const uint32_t *lens, uint64_t n_reads);

/* The counter's own (non-blocking) stream as vc_count_device's `stream`. */
#define VC_STREAM_CTX ((void *)(intptr_t)-1)

/* Same for device-resident reads (HBM pointers, e.g. from torch or
 * hipMalloc); enqueued on `stream`, a hipStream_t: NULL is HIP's null stream,
 * ordered with the legacy default stream (torch's default stream) as for any
 * HIP API; VC_STREAM_CTX is the counter's own stream (vc_stream).  Whatever
 * the stream, the launch is ordered after the counter's earlier work on its
 * own stream (vc_reset, earlier batches) and before its later work (vc_finish,
 * the shard sum), so vc_finish needs no device-wide synchronisation.  No host
 * synchronisation.  seq_bytes bounds every device read. */
int vc_count_device(vc_ctx *ctx, const uint8_t *d_seq, size_t seq_bytes,
                    const uint64_t *d_offs, const uint32_t *d_lens, uint64_t n_reads,
                    void *stream);

/* Wait for all queued work; copy counts[2*n_patterns] and the number of valid
 * k-mers extracted (perf_stats_t.total_kmers_extracted, vaf-counter.c:388)
 * to the host.  Either output may be NULL. */
int vc_finish(vc_ctx *ctx, uint32_t *counts, uint64_t *kmers_extracted);

/* Zero counts and the k-mer tally (asynchronous on the ctx stream). */
int vc_reset(vc_ctx *ctx);

/* Device pointer of the uint32 counts[2*n_patterns] array (for a device-side
 * all-reduce across ranks, e.g. RCCL through torch.distributed).  NULL for a
 * histogram counter (vc_kc_create), which has no pattern counts. */
void *vc_device_counts(vc_ctx *ctx);
/* Count into caller-owned device buffers instead (uint32[2*n_patterns] and
 * one uint64), e.g. torch tensors that an RCCL all-reduce then sums across
 * ranks; NULL restores the ctx's own buffers.  Not zeroed by this call.
 * VC_EINVAL for a histogram counter (vc_kc_create). */
int vc_bind_outputs(vc_ctx *ctx, void *d_counts, void *d_tally);
/* Device pointer of the uint64 k-mer tally; NULL for a histogram counter. */
void *vc_device_tally(vc_ctx *ctx);
void *vc_stream(vc_ctx *ctx);

/* Kernel timing: when enabled, every count call records HIP events around
 * the k-mer kernel on the stream it runs on; vc_kernel_ms synchronises on the
 * last pair and returns its elapsed milliseconds (sum of both kernels). */
int vc_set_timing(vc_ctx *ctx, int enable);
int vc_kernel_ms(vc_ctx *ctx, float *ms);

/* Table/prefilter geometry, for reports: n_keys, table slots, filter bytes.
 * VC_EINVAL for a histogram counter (vc_kc_create; its table is vc_kc_slots). */
int vc_table_info(const vc_ctx *ctx, uint64_t *n_keys, uint64_t *slots, uint64_t *filter_bytes);

/* ------------------------------------------------------------------ */
/* Multi-GPU counter -- the reference counts all     */
/* files into one set of counters in one process (vaf-counter.c:473-477,*/
/* 647-650) and writes them once (:653-681).                           */
/* ------------------------------------------------------------------ */

#define VC_MAX_SHARDS 64

/* A counter with one shard per entry of devices[0..n_devices): each shard
 * holds a replica of the static table and its own counts on its device (a
 * device may repeat: several shards on one GPU).  Host reads given to
 * vc_count_block / vc_count_file are dealt to the shards batch by batch,
 * round robin (the -b block loop and its stop rule still run once, in file
 * order); vc_count_device deals device batches the same way over the
 * shards that live on the device holding d_seq (VC_EINVAL if none does).
 * vc_finish reduces the shards -- same-device shards summed on their device,
 * then, when the shards span more than one device, one RCCL reduce (ncclSum
 * of the u32 counts and the u64 k-mer tally) to shard 0 over xGMI -- and
 * returns the totals, bit-identical
 * to a single device counting everything (u32 sums wrap like the
 * reference's counters).  vc_reset / vc_set_nt4_decode apply to every shard;
 * vc_bind_outputs, vc_device_counts, timing and vc_table_info to shard 0.
 * n_devices == 1 is vc_create.  With more than one distinct device,
 * librccl.so.1 ($VAFC_RCCL_LIB names another) is loaded before any device is
 * touched; if it cannot be loaded the call fails with VC_EHIP. */
int vc_create_multi(vc_ctx **out, int k, const uint64_t *keys, const uint32_t *vals, size_t n_keys,
                    uint32_t n_patterns, const int *devices, int n_devices);
/* Shards of a counter (1 for vc_create), and shard i's device and the host
 * batches it has counted so far. */
int vc_shard_count(const vc_ctx *ctx);
int vc_shard_info(const vc_ctx *ctx, int i, int *device, uint64_t *batches);

/* ------------------------------------------------------------------ */
/* Whole-file pass -- replaces count_fastq_kmers (vaf-counter.c:550).  */
/* ------------------------------------------------------------------ */

typedef struct {
	uint64_t bases;        /* bases of reads with len >= k (pipeline_t.total_bases) */
	uint64_t seqs;         /* reads with len >= k (pipeline_t.total_seqs) */
	uint64_t blocks;       /* non-empty -b blocks */
	double seconds;        /* wall time of this file */
} vc_file_stats;

/* Parse FASTA/FASTQ (plain or gzip) with kseq_read semantics (kseq.h:192-232)
 * under the reference's block loop: blocks of >= block_bases bases, reads
 * shorter than k skipped, a read error (-2) or EOF ends a block, the file ends
 * at the third empty block (vaf-counter.c:486-517, kthread.c:97-128).  Reads
 * are streamed to the device in large pinned batches.  Plain (uncompressed)
 * files of 32 MB or more are parsed by n_threads worker threads (the CLI's
 * -t; vafc_ingest.h) with identical results; gzip files are inflated by
 * n_threads workers (vafc_gzip.h, gzread's output) while (n_threads + 3) / 5
 * workers parse the inflated text in parallel (VAFC_GZ_PARSERS overrides);
 * small plain files use one reader thread.  Returns VC_EIO if the file cannot be opened (the reference
 * skips such files silently, vaf-counter.c:557). */
int vc_count_file(vc_ctx *ctx, const char *path, int block_bases, int n_threads,
                  vc_file_stats *st);

/* One rank's share of a file (one process per GPU, kmer-cnt_amd/vafc_dist.py):
 * the records of a plain FASTA/FASTQ file whose header lies in the byte range
 * [first, end), where first is the first record header at or after `begin`
 * (begin = 0: the file's start; later: the record shape found there, as the
 * parallel reader's pieces do, vafc_ingest.h).  Counted like vc_count_file,
 * the block loop starting afresh at `first`.  The reference counts a file in
 * one kseq stream (vaf-counter.c:486-517,550-582); consecutive ranges
 * [b_0 = 0, b_1), [b_1, b_2), ... count exactly its reads iff every range's
 * ri.first equals the previous range's ri.next and no range has ri.errs > 0
 * (a -2 from the reader ends a block, and the reference's third-empty-block
 * stop depends on the blocks before it).  The caller checks that and
 * otherwise counts the file whole in one range (begin = 0, end = UINT64_MAX,
 * which is vc_count_file's result).  gzip files (and anything but a regular
 * file) are not split: begin = 0 counts the whole file (ri.whole = 1),
 * begin > 0 counts nothing (ri.first = ri.next = UINT64_MAX, ri.whole = 1).
 * VC_EIO if the file cannot be opened. */
typedef struct {
	uint64_t first;     /* header offset counting began at; UINT64_MAX: none found, nothing counted */
	uint64_t next;      /* header offset of the first record at or past end; UINT64_MAX: the file ended */
	uint64_t errs;      /* reader -2 returns (truncated records) met in the range */
	uint32_t stopped;   /* the block loop ended the file inside the range */
	uint32_t whole;     /* 1: the file is not split by ranges (gzip, pipe) */
} vc_range_info;
int vc_count_file_range(vc_ctx *ctx, const char *path, uint64_t begin, uint64_t end, int block_bases,
                        int n_threads, vc_file_stats *st, vc_range_info *ri);
/* Host-only: the same range through the parallel reader without a device;
 * accepted read bytes / lengths copied out while they fit (as
 * vc_scan_file_parallel). */
int vc_scan_file_range(const char *path, int k, int block_bases, int n_threads, uint64_t piece_bytes,
                       uint64_t begin, uint64_t end, vc_file_stats *st, vc_range_info *ri, uint8_t *seq_out,
                       size_t seq_cap, uint32_t *lens_out, size_t lens_cap);

/* Where the calling thread's last pass through the parallel reader
 * (vc_count_file / vc_count_file_range on a plain or gzip file,
 * vc_scan_file_parallel, vc_scan_file_range) spent its time: prof[0..7) =
 * the reader's wall seconds; main-thread seconds waiting for the next piece,
 * submitting pieces (H2D copies and kernel launches), re-parsing mis-guessed
 * pieces; worker thread-seconds parsing, waiting for a slot the main thread
 * had not released, waiting for a slot's previous copy to leave it.  Returns
 * the pieces of that pass (0: none yet).  prof may be NULL. */
uint64_t vc_ingest_profile(double *prof);

/* The same pass's profile with the workers' parse split (round 6): the first
 * min(n, VC_INGEST_PROFILE_FIELDS) of prof[] = the seven fields above, then
 * the workers' seconds reading the source (pread: the copy out of the page
 * cache) and the bytes read, seconds copying accepted sequences into the slots
 * and the bytes copied (0 with VAFC_SLOT_COPY=0, which copies per read
 * untimed), seconds guessing record starts, the workers' CPU seconds and
 * wall seconds (CPU < wall: descheduled, e.g. a CPU quota's throttling), the
 * main thread's CPU seconds, the worker count and the slot-copy mode.
 * Returns the pieces of that pass. */
#define VC_INGEST_PROFILE_FIELDS 17
uint64_t vc_ingest_profile_ex(double *prof, int n);

/* Optional: allocate vc_count_file's parallel-reader buffers for n_threads
 * reader threads now (pinned host + device memory, about 20 MB per thread),
 * so that a later vc_count_file does not pay for the allocation.  Without
 * it, vc_count_file's workers allocate each buffer on its first use, while
 * the other workers parse.  The CLI does not call it (VAFC_RESERVE=1 makes
 * it, inside the counting timer). */
int vc_reserve_file_ingest(vc_ctx *ctx, int n_threads);

/* Host-only: the same reader + block loop without a device (no counting).
 * Accepted read bytes / lengths are copied out while they fit (either output
 * may be NULL).  Lets the reader semantics be checked on machines without a
 * GPU and measures host ingest speed. */
int vc_scan_file(const char *path, int k, int block_bases, vc_file_stats *st,
                 uint8_t *seq_out, size_t seq_cap, uint32_t *lens_out, size_t lens_cap);

/* Host-only: vc_count_file's parallel reader for plain (uncompressed) files,
 * without a device: n_threads workers parse pieces of piece_bytes of the file
 * concurrently (vafc_ingest.h); accepted reads come out in file order, exactly
 * as vc_scan_file's.  Lets the parallel reader be checked without a GPU and
 * measures its speed.  gzip input: n_threads inflate workers with chunks of
 * piece_bytes compressed bytes (the reader of vc_count_file for .gz), the
 * block loop in the calling thread. */
int vc_scan_file_parallel(const char *path, int k, int block_bases, int n_threads, uint64_t piece_bytes,
                          vc_file_stats *st, uint8_t *seq_out, size_t seq_cap, uint32_t *lens_out,
                          size_t lens_cap);

/* Host-only gzip inflate (test and speed hooks): the whole decompressed
 * stream of `path` -- through the parallel inflater (n_threads workers,
 * chunk_bytes compressed bytes per chunk; stats6 = chunks, accepted, skipped,
 * zlib fallbacks, members checked, CRC error) or through zlib's gzread --
 * written to out while it fits.  Returns the stream's length, or -1 if the
 * file cannot be opened (parallel: is not gzip). */
int64_t vc_gz_inflate_parallel(const char *path, int n_threads, uint64_t chunk_bytes, uint8_t *out,
                               uint64_t cap, uint64_t *stats6);
int64_t vc_gz_inflate_zlib(const char *path, uint8_t *out, uint64_t cap);
/* Host-only: zlib-compatible CRC-32 of p[0..n) continuing from crc (the
 * inflater's member check; PCLMULQDQ folding where the CPU has it). */
uint32_t vc_gz_crc32(uint32_t crc, const uint8_t *p, uint64_t n);
/* zlib's crc32_combine: the CRC-32 of A then B from crc(A), crc(B), len(B). */
uint32_t vc_gz_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);

/* One gzip file over several ranks (round 6, kmer-cnt_amd/vafc_dist.py; the
 * reference reads it with one gzread, vaf-counter.c:557, kseq.h:74-85).
 * Rank r's share is the text of the deflate blocks from the first dynamic
 * block starting at or after byte A_r of the file up to the first dynamic
 * block starting at or after A_{r+1} (A_0 = 0: the stream's start).
 *
 * 1. vc_gz_share_scan: each rank decodes its share speculatively without
 *    the history before it and reports where the share starts and ends (bit
 *    offsets), its text length, and its last 32 KiB of text as symbols
 *    (window_sym, 32768 entries: a byte value < 256, or 0x8000 | i for byte i
 *    of the unknown 32 KiB before the share).  ok = 0: the share could not be
 *    decoded without that history (the caller counts the file whole).
 * 2. The shares chain iff each share's start_bit equals the previous
 *    (non-empty) share's end_bit; the 32 KiB before share r+1 is share r's
 *    window_sym with every 0x8000 | i replaced by byte i of the 32 KiB before
 *    share r (share 0's history is empty).
 * 3. vc_count_gz_share: the share's reads, counted from start_bit with that
 *    window: the records whose header lies in the share's text, the block
 *    loop starting afresh at the first, as vc_count_file_range does for a
 *    byte range of a plain file.  ri.first / ri.next are offsets in the
 *    share's own text / the next share's text, so consecutive shares are
 *    exact under the same chain rule (first == previous next, no -2).  crc
 *    reports the CRC-32 accounting of the share: members wholly inside are
 *    checked (crc_error), the member open at the share's start closes at its
 *    first member end (head_*, to be checked by the caller with the previous
 *    shares' tails) and the one open at its end is the tail. */
typedef struct {
	uint64_t start_bit;   /* UINT64_MAX: no dynamic block starts in the share's bytes (an empty share) */
	uint64_t end_bit;     /* UINT64_MAX: the stream ended inside the share */
	uint64_t text_len;    /* bytes of text from start_bit to end_bit */
	uint32_t ok;
	uint32_t ended;
} vc_gz_share_info;
int vc_gz_share_scan(const char *path, uint64_t begin, uint64_t end, int n_threads, uint64_t chunk_bytes,
                     vc_gz_share_info *out, uint16_t *window_sym);

typedef struct {
	uint32_t events;            /* member ends inside the share */
	uint32_t head_crc;          /* CRC-32 of the share's text up to its first member end */
	uint64_t head_len;
	uint32_t head_expect_crc;   /* that member's trailer (CRC-32, ISIZE) */
	uint32_t head_expect_isize;
	uint32_t tail_crc;          /* from the last member end (or the share's start) to the share's end */
	uint64_t tail_len;
	uint32_t crc_error;         /* a member wholly inside the share failed its check */
	uint32_t complete;          /* the accounting reached the share's end */
} vc_gz_share_crc;
/* first_share: the stream's start (start_bit and window unused).  Counts like
 * vc_count_file_range (NULL ri/crc not allowed); VC_EIO if the file cannot be
 * opened as gzip. */
int vc_count_gz_share(vc_ctx *ctx, const char *path, int first_share, uint64_t start_bit, const uint8_t *window,
                      uint64_t text_len, int block_bases, int n_threads, vc_file_stats *st, vc_range_info *ri,
                      vc_gz_share_crc *crc);
/* Host-only: the same reader without a device (accepted reads copied out
 * while they fit, as vc_scan_file_range). */
int vc_scan_gz_share(const char *path, int k, int first_share, uint64_t start_bit, const uint8_t *window,
                     uint64_t text_len, int block_bases, int n_threads, vc_file_stats *st, vc_range_info *ri,
                     vc_gz_share_crc *crc, uint8_t *seq_out, size_t seq_cap, uint32_t *lens_out, size_t lens_cap);

/* One pass per share instead of two: vc_gz_share_open scans as
 * vc_gz_share_scan and keeps the share's decoded chunks (one to two bytes of
 * memory per byte of text: two for every symbol decoded while the chunk can
 * still refer to the unknown window, which in FASTQ is most of it; at most
 * hold_bytes),
 * so that the count resolves them with the window instead of inflating the
 * share again.  *held is NULL when the share did not fit in hold_bytes (or
 * could not be scanned): the caller then counts with vc_count_gz_share.  A
 * held share is counted once (vc_count_gz_share_held / vc_scan_gz_share_held,
 * same outputs as the unheld forms) and closed with vc_gz_share_close.  ctx:
 * the counter that will count the share (the scan's threads run on its GPU's
 * NUMA node, where the kept text is then read), or NULL. */
typedef struct vc_gz_share vc_gz_share;
int vc_gz_share_open(vc_ctx *ctx, const char *path, uint64_t begin, uint64_t end, int n_threads,
                     uint64_t chunk_bytes, uint64_t hold_bytes, vc_gz_share_info *out, uint16_t *window_sym,
                     vc_gz_share **held);
int vc_count_gz_share_held(vc_ctx *ctx, vc_gz_share *held, int first_share, const uint8_t *window, uint64_t text_len,
                           int block_bases, int n_threads, vc_file_stats *st, vc_range_info *ri, vc_gz_share_crc *crc);
int vc_scan_gz_share_held(vc_gz_share *held, int k, int first_share, const uint8_t *window, uint64_t text_len,
                          int block_bases, int n_threads, vc_file_stats *st, vc_range_info *ri, vc_gz_share_crc *crc,
                          uint8_t *seq_out, size_t seq_cap, uint32_t *lens_out, size_t lens_cap);
void vc_gz_share_close(vc_gz_share *held);

/* Host-only: the kseq_read return value of every record until -1 (inclusive),
 * written while they fit; returns the number of calls made, or VC_EIO. */
int64_t vc_scan_records(const char *path, int32_t *rets, int64_t cap);

/* ------------------------------------------------------------------ */
/* snp-pattern-gen                            */
/* ------------------------------------------------------------------ */

/* A reference genome in host memory: records, names and sequences exactly
 * as load_fasta keeps them (snp-pattern-gen.c:67-103: kseq_read until the
 * first negative return; name = the header up to the first whitespace).
 * Sequences are stored back to back (vc_fasta_data gives the concatenated
 * view that vc_count_candidates takes).  Plain or gzip input. */
typedef struct vc_fasta vc_fasta;
int vc_fasta_load(const char *path, vc_fasta **out);   /* VC_EIO if unopenable; gzip inflated
                                                          by up to 16 threads (VAFC_THREADS) */
int vc_fasta_count(const vc_fasta *fa);
const char *vc_fasta_name(const vc_fasta *fa, int i);
const uint8_t *vc_fasta_seq(const vc_fasta *fa, int i, uint32_t *len);
int vc_fasta_data(const vc_fasta *fa, const uint8_t **seq, size_t *bytes, const uint64_t **offs,
                  const uint32_t **lens);
void vc_fasta_free(vc_fasta *fa);

/* ------------------------------------------------------------------ */
/* kc-c4: histogram of canonical k-mer occurrence counts               */
/* (kc-c4.c)                                   */
/* ------------------------------------------------------------------ */

/* A counter in histogram mode: every canonical k-mer (seq_nt4_table decode,
 * kc-c4.c:85-101) of the reads given to vc_count_block / vc_count_device /
 * vc_count_file is counted in a device hash table of `table_slots` slots
 * (16 B each, rounded up to a power of two, at most 40 % of free HBM; 0 =
 * that maximum).
 * Replaces kc-c4's kc_c4x_t sub-tables and count_file (kc-c4.c:56-66,
 * 170-182).  vc_reset clears the table; vc_finish returns the k-mers seen.
 * Reads may overlap, but when a call holds more reads longer than 4096 bases
 * than seq_bytes / 4097 + 1 the surplus is not counted: vc_finish,
 * vc_kc_histogram2 and vc_yak_bloom_select then return VC_EINVAL until
 * vc_reset. */
int vc_kc_create(vc_ctx **out, int k, uint64_t table_slots, int device);
/* Count only the k-mers of partition `part` of `n_parts` (1..1024), by the
 * low 10 bits of hash64 (kc-c4.c:40-50): ((h & 1023) * n_parts) >> 10 ==
 * part, so a partition holds whole kc-c4 / yak sub-tables (kc-c4.c:74-83,
 * p >= 10): a set larger than the table is counted in n_parts passes, or on
 * n_parts GPUs, whose histograms add up.  n_parts = 1 counts everything.
 * Clears the table. */
int vc_kc_set_partition(vc_ctx *ctx, uint32_t n_parts, uint32_t part);
/* Slots of the table (after rounding). */
uint64_t vc_kc_slots(vc_ctx *ctx);
/* Synchronizes; hist[c] (c = 1..255, 256 entries) += the number of distinct
 * k-mers counted min(c, 255) times (print_hist, kc-c4.c:196-223); distinct
 * and kmers receive the table's distinct k-mers and the k-mers seen.
 * VC_EFULL (hist untouched) when the table ran out of room: count again
 * with more partitions or a larger table. */
int vc_kc_histogram(vc_ctx *ctx, uint64_t *hist, uint64_t *distinct, uint64_t *kmers);
/* General form: hist[min(c, n_bins - 1)] += 1 (n_bins 2..1024) for every key
 * counted c >= min_count times and not dropped by vc_yak_bloom_select;
 * *distinct = the keys added.  yak-count's histogram (yak-count.c:209-240,
 * 500-503) is n_bins 1024, min_count 1 (no filter) or 2 (after its shrink to
 * [2, 1023], :268-288). */
int vc_kc_histogram2(vc_ctx *ctx, uint64_t *hist, uint32_t n_bins, uint64_t min_count, uint64_t *distinct,
                     uint64_t *kmers);

/* yak-count -b (yak-count.c:440-452), pass 1 to pass 2.  Count file 1 with
 * first-occurrence tracking on (vc_kc_track_first, which also clears), then
 * vc_yak_bloom_select replays yak's per-sub-table blocked Bloom filters
 * (2^(bf_shift - pre) bits each, n_hash bits per k-mer, yak-count.c:71-108,
 * 150-176) over the stream order to find the keys yak would have inserted,
 * restarts their counts at 0 and drops the rest; later count calls (file 2)
 * then only count those keys (yak's create_new = 0).  Without a valid filter
 * (n_hash <= 0, or bf_shift - pre outside 9..55) every key stays.  A later
 * vc_reset returns to insert mode. */
int vc_kc_track_first(vc_ctx *ctx, int on);
int vc_yak_bloom_select(vc_ctx *ctx, int pre, int bf_shift, int n_hash);

/* Decode mode of a counter: on = seq_nt4_table at every position, the decode
 * of snp-pattern-gen (snp-pattern-gen.c:165), instead of vaf-counter's
 * position-dependent one (the default).  Applies to later count calls.
 * VC_EINVAL for a histogram counter (vc_kc_create). */
int vc_set_nt4_decode(vc_ctx *ctx, int on);

/* count_candidate_kmers (snp-pattern-gen.c:159-190) on the GPU: counts[i]
 * (u32, wrapping like the reference's khash values) = the number of
 * canonical k-mers of all n_seqs sequences that equal keys[i].  Sequences
 * are decoded with seq_nt4_table at every position (no vaf-counter quirk);
 * any other byte ends the current window.  keys must be distinct canonical
 * k-mers; seq/offs/lens are host buffers (sequence i at seq + offs[i]). */
int vc_count_candidates(int k, const uint8_t *seq, size_t seq_bytes, const uint64_t *offs,
                        const uint32_t *lens, uint64_t n_seqs, const uint64_t *keys, size_t n_keys,
                        uint32_t *counts, int device);

/* ------------------------------------------------------------------ */
/* correlation-matrix: depth-aware Pearson between .vaf samples + tree  */
/* (correlation-matrix.c)                      */
/* ------------------------------------------------------------------ */

typedef struct vc_vafset vc_vafset;
int vc_vafset_create(vc_vafset **out);
void vc_vafset_free(vc_vafset *s);
/* load_vaf_file (correlation-matrix.c:25-90): fgets lines of at most 4095
 * bytes, '#' and "CHR" lines skipped, rows read with the reference's 9-field
 * sscanf conversion (vaf = field 9, depth = field 8), at most 100,000 rows
 * (then the reference's warning on stderr); name = basename cut at the first
 * ".vaf".  VC_EIO if the file cannot be opened (the reference exits 1). */
int vc_vafset_add(vc_vafset *s, const char *path);
/* The same for n files read by n_threads threads: files are appended in
 * order up to the first one that cannot be opened (*n_added = its index,
 * VC_EIO; VC_OK if all were); truncated[i] = 1 where the 100,000-row cap was
 * hit, for the caller to print the reference's warning in file order
 * (load_vaf_file prints it while loading, correlation-matrix.c:70-73). */
int vc_vafset_add_many(vc_vafset *s, const char *const *paths, int n, int n_threads, int *n_added,
                       uint8_t *truncated);
/* A sample from arrays (n <= 100,000 rows). */
int vc_vafset_add_arrays(vc_vafset *s, const char *name, const double *vaf, const int32_t *depth, int n);
int vc_vafset_count(const vc_vafset *s);
const char *vc_vafset_name(const vc_vafset *s, int i);
int vc_vafset_snps(const vc_vafset *s, int i);
/* calculate_correlation_matrix + pearson_correlation_depth_aware
 * (correlation-matrix.c:94-162) on the GPU: corr[i*n + j] (n = samples, row
 * major, symmetric, 1.0 on the diagonal) is bit-identical to the reference's
 * double: for i < j the rows [0, rows of sample i) that have depth >=
 * min_depth in both samples (rows past sample j's end count as vaf 0, depth
 * 0), 0.0 below min_snps of them.  kernel_ms (may be NULL) receives the
 * kernel time. */
int vc_corr_matrix(const vc_vafset *s, int min_snps, int min_depth, double *corr, int device, float *kernel_ms);
/* The same on arrays: sample i has n_snps[i] rows at vaf/depth + i*stride. */
int vc_corr_matrix_raw(const double *vaf, const int32_t *depth, const int32_t *n_snps, int n_samples,
                       size_t stride, int min_snps, int min_depth, double *corr, int device, float *kernel_ms);
/* The .corr file (correlation-matrix.c:350-366): header row of names, then
 * one row per sample, "%.6f" cells.  VC_EIO if it cannot be created. */
int vc_corr_write(const vc_vafset *s, const double *corr, const char *path);
/* build_tree (correlation-matrix.c:190-257): average linkage on 1 - r, the
 * same merge order, ties and "%.4f" text.  VC_EIO if it cannot be created. */
int vc_corr_tree(const vc_vafset *s, const double *corr, const char *path);

/* ------------------------------------------------------------------ */
/* ed-vaf-counter: approximate pattern search in reads                 */
/* (ed-vaf-counter.c; its edlibAlign calls in HW mode, EDLIB_TASK_LOC) */
/* ------------------------------------------------------------------ */

/* A query is a byte string of length m, 1 <= m <= 127; bytes compare exactly
 * (no case folding, N = N, bytes >= 0x80 are ordinary symbols).  For a read T
 * of n bytes and a query P let D be the edit-distance table with D[0][j] = 0,
 * D[i][-1] = i and unit costs, s_j = D[m][j], e' = m if max_edit < 0 else
 * max_edit, k' = min(e', m).  The hit count of (T, P) is 1 when n = 0;
 * otherwise the candidates are s_0..s_{n-1}, plus one of value m when k' = m
 * and n < 64 * ceil(m / 64) - m, and the count is the number of candidates
 * equal to their minimum b if b <= k', else 0.  This is what the reference
 * adds per search_kmer_in_seq call (ed-vaf-counter.c:95-119: numLocations of
 * edlibAlign).  Counts are uint32 sums over all reads and wrap modulo 2^32
 * (ed-vaf-counter.c:37-38,147-148).  Forward strand only. */
typedef struct vc_ed vc_ed;

/* The queries of a pattern database (load_patterns, ed-vaf-counter.c:47-83,
 * and the two searches per pattern, :143-144): pattern i's ref query is the
 * m = strlen(ref_kmer) bytes of ref_kmer, its alt query the first m bytes of
 * alt_kmer, padded with NUL bytes when alt_kmer is shorter.  Counts layout
 * [2 * n_patterns]: ref of pattern i at [2i], alt at [2i + 1].  max_edit is
 * the CLI's -e.  VC_EINVAL for a length outside 1..127. */
int vc_ed_create(vc_ed **out, const vc_patterns *db, int max_edit, int device);
/* The same from arbitrary byte strings: query i is queries[q_offs[i] ..
 * q_offs[i] + q_lens[i]), counts layout [n_queries]. */
int vc_ed_create_raw(vc_ed **out, const uint8_t *queries, const uint32_t *q_offs, const uint32_t *q_lens,
                     size_t n_queries, int max_edit, int device);
void vc_ed_destroy(vc_ed *ed);
/* Search one block of host-resident reads (the loop body of count_fastq_kmers,
 * ed-vaf-counter.c:137-150): staged through pinned memory, asynchronous,
 * accumulating, buffers reusable on return -- as vc_count_block.  Every read
 * counts, empty ones included. */
int vc_ed_count_block(vc_ed *ed, const uint8_t *seq, size_t seq_bytes, const uint64_t *offs, const uint32_t *lens,
                      uint64_t n_reads);
/* The same for device-resident reads on `stream` (NULL: HIP's null stream,
 * VC_STREAM_CTX: the handle's own), with vc_count_device's ordering
 * contract: after the handle's earlier work, before its later work, no host
 * synchronisation.  seq_bytes bounds every device read; a read reaching past
 * it makes vc_ed_finish return VC_EINVAL. */
int vc_ed_count_device(vc_ed *ed, const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs,
                       const uint32_t *d_lens, uint64_t n_reads, void *stream);
/* Wait for all queued work and copy the counts to the host (the counters the
 * reference sums and writes, ed-vaf-counter.c:204-228). */
int vc_ed_finish(vc_ed *ed, uint32_t *counts);
/* Zero the counts (asynchronous on the handle's stream). */
int vc_ed_reset(vc_ed *ed);
/* Start the counts from host values instead of zero (asynchronous), e.g. to
 * continue an earlier run or to check the wrap at 2^32. */
int vc_ed_set_counts(vc_ed *ed, const uint32_t *counts);
/* Test and experiment hook: later count calls split a batch into at most
 * max_ranges read ranges per query block (0, the default: sized from the
 * device's CU count so that a batch fills it).  Fewer ranges mean more reads
 * per block; the counts do not depend on it. */
int vc_ed_set_max_ranges(vc_ed *ed, uint32_t max_ranges);
/* Test hook, read-only: the kernel shape chosen at creation for the queries
 * of one word width (0: 1..32 bytes, 32-bit words; 1: 33..64 bytes, one
 * 64-bit word; 2: 65..127 bytes, two 64-bit words).  *n_groups: groups of 64
 * queries, 0 when the handle has no query of that width (then *waves = 1 and
 * *lds_masks = 1, and no kernel runs for it); *waves: groups per block, 1..4;
 * *lds_masks: 1 when a block keeps its match masks in LDS, 0 when it reads
 * them from HBM.  Each output may be NULL.  VC_EINVAL for a NULL handle or a
 * width outside 0..2. */
int vc_ed_shape(const vc_ed *ed, int width, uint32_t *n_groups, int *waves, int *lds_masks);
/* Elapsed milliseconds of the kernels of the last count call (HIP events
 * recorded around them on the stream they ran on; synchronises on it). */
int vc_ed_kernel_ms(vc_ed *ed, float *ms);
/* count_fastq_kmers (ed-vaf-counter.c:122-154): every record of a FASTA/FASTQ
 * file, plain or gzip, read with kseq_read semantics until the first negative
 * return, searched in pinned batches that alternate with the kernel.
 * n_threads: inflate threads for gzip input.  st (may be NULL): bases and
 * seqs of all records, blocks = batches.  VC_EIO if the file cannot be
 * opened (the reference warns and skips it, :129-132). */
int vc_ed_count_file(vc_ed *ed, const char *path, int n_threads, vc_file_stats *st);

/* ------------------------------------------------------------------ */
/* bam-vaf-counter: ref/alt base counts at SNP positions from BAM      */
/* (bam-vaf-counter.c; record rules of htslib's sam.c bam_read1)       */
/* ------------------------------------------------------------------ */

/* The contract, read from bam-vaf-counter.c and htslib and pinned by the
 * goldens of tests/golden/bam:
 *
 * 1. Patterns and tids.  Row i of vc_patterns_load has chr, pos = start, ref
 *    and alt (one byte each, compared exactly: lower case never matches).  A
 *    row's tid is the index of chr in the FIRST input file's reference list
 *    and is used for every later file.  A row whose chr is absent gets a
 *    warning line and never counts.  Duplicate positions warn, and every such
 *    row counts on its own.
 * 2. A record with flag 0x4, 0x200 or 0x400 is skipped (secondary and
 *    supplementary records count).  A record with tid < 0 overlaps nothing.
 * 3. The CIGAR walk.  For a record at (tid, pos), end = pos + rlen, rlen the
 *    reference length of its CIGAR (ops M, D, N, =, X), or 1 if that is 0.
 *    Every row with that tid and pos <= row.pos < end is looked at; the walk
 *    starts at cur = pos, rp = 0.  M, = and X of length L: if cur <= row.pos <
 *    cur + L the base is "=ACMGRSVTWYHKDBN"[nibble rp + row.pos - cur]; base
 *    == ref adds w to ref_count, else base == alt adds w to alt_count; either
 *    way the walk stops.  Otherwise cur and rp advance by L.  I and S advance
 *    rp.  D and N: inside, the walk stops with no count; otherwise cur
 *    advances.  H, P and op codes 9..15 do nothing.  ref == alt counts as ref.
 * 4. Counts are uint32 sums over all records of all files and wrap.
 * 5. Without a usable index w = 1.
 * 6. With an index (the first existing of <fn>.csi, <fn minus its last
 *    extension>.csi, <fn>.bai, <fn minus its last extension>.bai, if it
 *    carries the BAI\1 magic or is BGZF whose text starts CSI\1) the
 *    reference fetches every merged region in turn and counts all overlapping
 *    rows of every record fetched, so w = the number of merged regions [s, e)
 *    with region tid == tid, pos < e and end > s.  Regions (build_regions,
 *    :124-175): one [pos, pos + 1) per row, sorted by strcmp(chr) then start,
 *    merged while prev.end >= next.start; a region's tid is looked up in THIS
 *    file's header, regions on an absent chromosome warn and are skipped.  The
 *    whole file is read and w applied; nothing seeks, but under item 9.
 * 7. What ends a file's records, keeping those before, silently and with exit
 *    code 0.  A BGZF block that is truncated, does not inflate or fails its
 *    CRC-32 / ISIZE, and a record cut off by the end of the data, end them
 *    (htslib's BGZF error is sticky).  A failure of one record (sam.c
 *    bam_read1) does so only where the reference's reading loop (:380-397)
 *    and kt_pipeline's two workers make it: records are read in batches of
 *    1,000, a failed read closes the batch, and the file ends at the second
 *    batch that closes empty (each worker leaves at its first).  So a
 *    block_size < 32, fields that do not fit the block_size (or l_read_name
 *    = 0, l_seq < 0), malformed aux data in front of a CG tag that is looked
 *    for, and a record with n_cigar > 0, l_seq > 0, flag 0x4 clear and a
 *    CIGAR query length != l_seq drop that record, and reading goes on behind
 *    the bytes htslib has consumed: the 4 of the block_size word, the 36 up
 *    to the fixed fields, or the whole record.  The file ends where such a
 *    failure is, for the second time, the first read of its batch (right
 *    after 1,000 good records or after another failure): three failures in a
 *    row always end it.  A missing EOF block ends nothing.
 * 8. Deviations: BGZF-compressed BAM only; a base index at or past l_seq
 *    counts nothing (so l_seq == 0 with a CIGAR counts nothing); a record in
 *    the CG:B,I long-CIGAR convention is counted with its real CIGAR, as
 *    htslib moves it in; htslib's own [E::/[W:: lines are not reproduced.
 * 9. The seek plan (vc_bam_index_plan), for a BAI index and item 6's merged
 *    regions (tid, s, e).  Per region: the bins of [s, e) in the 6-level,
 *    14-bit scheme (reg2bins); of their chunks (beg, end as virtual offsets,
 *    compressed offset << 16 | offset in the member's text) those with end >
 *    min_off, min_off the linear index's entry of window s >> 14, or 0 where
 *    the linear index is shorter.  The union over all regions is sorted by
 *    beg and merged while the next span's beg >> 16 is <= the current span's
 *    end >> 16, so the spans ascend, no BGZF member belongs to two of them and
 *    no record is read twice.  A span is read from the record at beg through
 *    the last record that starts before end.  This is a superset of what
 *    htslib's iterator returns for the regions; item 6's weights and the
 *    kernels' own overlap test make the counts those of the whole file.  The
 *    index is not usable for seeking when it is no BAI (a CSI among them), is
 *    truncated, carries a count its length cannot hold or bytes behind
 *    n_no_coor, has an n_ref other than the header's, a bin twice in one
 *    reference or a chunk with end < beg, or when a region ends past 2^29.  An
 *    index that passes all this and belongs to another file is not detected:
 *    as with the reference, the counts are then those of whatever records
 *    the stale offsets lead to. */

/* One record as the kernels read it: its n_cigar CIGAR words (BAM encoding,
 * len << 4 | op) at data + off, off a multiple of 4, followed by its (l_seq +
 * 1) / 2 bytes of packed 4-bit bases. */
typedef struct {
	int32_t tid, pos;
	uint32_t flag, n_cigar, l_seq;
	uint32_t reserved;     /* 0 */
	uint64_t off;
} vc_bam_rec;

typedef struct vc_bam vc_bam;
typedef struct vc_bam_file vc_bam_file;

/* Kinds of input, vc_bam_probe: only VC_BAM_BGZF is read. */
enum { VC_BAM_BGZF = 0, VC_BAM_SAM = 1, VC_BAM_CRAM = 2, VC_BAM_RAW = 3, VC_BAM_GZIP = 4, VC_BAM_BGZF_OTHER = 5 };
/* What a file is by its first bytes; VC_EIO if it cannot be opened. */
int vc_bam_probe(const char *path, int *kind);
const char *vc_bam_kind_name(int kind);

/* Host reader (zlib and threads, no GPU): the header and every record of a
 * BGZF BAM under items 7 and 8, as descriptors into one data buffer.  VC_EIO:
 * cannot be opened; VC_EINVAL: not BGZF BAM, or the header cannot be read
 * (the file object is still returned with no references when it opened).
 * vc_bam_read_header stops behind the header (sam_hdr_read of main, :512-527). */
int vc_bam_read_file(const char *path, int n_threads, vc_bam_file **out);
int vc_bam_read_header(const char *path, vc_bam_file **out);
int vc_bam_file_refs(const vc_bam_file *f);
const char *vc_bam_file_ref_name(const vc_bam_file *f, int i);
uint64_t vc_bam_file_records(const vc_bam_file *f, const vc_bam_rec **recs, const uint8_t **data, uint64_t *data_bytes);
void vc_bam_file_free(vc_bam_file *f);
/* The index file item 6 finds for `path` (a copy into buf), 1 if it carries a
 * usable magic, 0 if there is none or it does not. */
int vc_bam_index_usable(const char *path, char *buf, size_t buf_len);
/* build_regions (bam-vaf-counter.c:124-175): row indices whose (chr, start)
 * open a merged region, its end in ends[]; both arrays hold
 * vc_patterns_count entries, the return value is the number of regions. */
int vc_bam_build_regions(const vc_patterns *db, int32_t *first_row, int32_t *ends);
/* Item 9's plan, no GPU: the spans to read for n merged regions (tid in [0,
 * n_ref), 0 <= start < end) by the BAI at index_path, or, with index_path
 * NULL, by the index item 6 finds for bam_path.  n_ref: the references of the
 * BAM's header.  VC_OK: *spans holds *n_spans spans, ascending and disjoint
 * (NULL and 0 where no chunk is wanted), to be freed by
 * vc_bam_index_plan_free.  VC_BAM_NO_SEEK: there is no index, or it is not
 * usable for seeking.  VC_EINVAL: a bad argument or region. */
typedef struct {
	uint64_t beg, end;     /* virtual offsets */
} vc_bam_span;
#define VC_BAM_NO_SEEK 1
int vc_bam_index_plan(const char *bam_path, const char *index_path, int32_t n_ref, const int32_t *tid, const int32_t *start,
                      const int32_t *end, size_t n, vc_bam_span **spans, size_t *n_spans);
void vc_bam_index_plan_free(vc_bam_span *spans);

/* A counter for the rows of db, their tids from ref_names[0..n_refs) (the
 * first file's header, create_snp_map :187-215, whose two warnings are
 * written to stderr).  Counts layout [2 * n_patterns] as vc_ed_create. */
int vc_bam_create(vc_bam **out, const vc_patterns *db, const char *const *ref_names, int n_refs, int device);
void vc_bam_destroy(vc_bam *b);
/* The merged regions of the file being counted, for item 6's weights: tids in
 * that file's header, n = 0 for item 5 (all weights 1, the state after
 * create).  Asynchronous on the handle's stream; holds for later count calls. */
int vc_bam_set_regions(vc_bam *b, const int32_t *tid, const int32_t *start, const int32_t *end, size_t n);
/* Count one block of host-resident records (staged through pinned memory,
 * asynchronous, accumulating, buffers reusable on return). */
int vc_bam_count_block(vc_bam *b, const vc_bam_rec *recs, uint64_t n_recs, const uint8_t *data, size_t data_bytes);
/* The same for HBM-resident records on `stream`, with vc_count_device's
 * ordering contract.  data_bytes bounds every device read: a descriptor that
 * points outside it (or off a 4-byte boundary) is not followed and makes
 * vc_bam_finish return VC_EINVAL. */
int vc_bam_count_device(vc_bam *b, const vc_bam_rec *d_recs, uint64_t n_recs, const uint8_t *d_data,
                        size_t data_bytes, void *stream);
int vc_bam_finish(vc_bam *b, uint32_t *counts);
int vc_bam_reset(vc_bam *b);
int vc_bam_set_counts(vc_bam *b, const uint32_t *counts);
/* Records of more than `ops` CIGAR operations get a wave each instead of a
 * lane (default 64; 0: every record with a CIGAR, UINT32_MAX: none).  The
 * counts do not depend on it. */
int vc_bam_set_long_threshold(vc_bam *b, uint32_t ops);
int vc_bam_kernel_ms(vc_bam *b, float *ms);

/* Records found, checked and counted in inflated BAM text on the device: the
 * text never reaches the host.  A text is a piece of a file's record stream
 * (behind the header): a chain in which the record at offset o, with its
 * block_size word bl, is followed by the one at o + 4 + bl.
 *
 *  - entry: the offset of the piece's first record (<= text_bytes).  cuts: n
 *    offsets, ascending, each <= text_bytes, that divide the text into n + 1
 *    segments (the file pass uses the BGZF members' borders); they decide how
 *    the work is shared out and never what is found.  Each segment guesses
 *    its first record start (a run of plausible headers: block_size >= 32,
 *    -1 <= tid, next_tid < the handle's n_refs, pos >= -1, l_read_name >= 1,
 *    l_seq >= 0, fields that fit, a NUL at the name's end) and walks from it;
 *    one wave then links the segments in order from `entry`, walking again
 *    every segment whose guess is not the true entry, so the records are
 *    those of the serial walk whatever the guesses were.
 *  - The walk takes a record when its block_size is >= 32 and it lies whole
 *    inside the text.  It stops at a block_size < 32 (short_stop) and at a
 *    record the text cuts off; `consumed` is the offset where it stopped, or
 *    text_bytes.  A caller with more text scans the next piece from there;
 *    with final != 0 the records end there (item 7: a cut record ends the
 *    file).
 *  - Each record found gets the tests of the host reader.  It is irregular,
 *    and not counted, when its fields do not fit its block_size, l_read_name
 *    = 0, l_seq < 0, its CIGAR's query length is not l_seq (n_cigar > 0,
 *    l_seq > 0, flag 0x4 clear), or its first CIGAR word is l_seq << 4 | 4
 *    with tid >= 0, pos >= 0 and aux bytes behind the qualities (the CG
 *    long-CIGAR convention: the tag may be among them).  With final
 *    != 0 a cut last record whose 36 leading bytes are there and whose fields
 *    do not fit is irregular too.  The host reader drops such records and
 *    reads on elsewhere (item 7), so a caller that sees irregular > 0 or
 *    short_stop and wants the contract's counts reads the file on the host.
 *  - Every other record is counted where it lies, under items 2 to 6, the
 *    regions of vc_bam_set_regions and the long threshold included, by the
 *    kernels of vc_bam_count_block; counts accumulate as there.
 *
 * text_bytes < 2^32 - 16.  Every device read is bounded by text_bytes.
 * vc_bam_scan_text_device: text and cuts in HBM (cuts 8-byte aligned) on
 * `stream`, with vc_count_device's ordering contract; both stay valid until
 * the stream has passed the call.  vc_bam_scan_text_block: host bytes staged
 * through pinned memory, asynchronous, buffers reusable on return.
 * vc_bam_text_result waits for the handle's stream and reports the last scan.
 * vc_bam_text_kernel_ms: the last scan's guess, link and emit launches
 * (find_ms) and its check kernel (check_ms), either may be NULL; the count
 * kernels behind them are vc_bam_kernel_ms. */
typedef struct {
	uint64_t consumed;
	uint64_t records;        /* regular records: counted */
	uint64_t bases;          /* the sum of their l_seq */
	uint64_t irregular_off;  /* lowest offset of an irregular record, UINT64_MAX without one */
	uint32_t irregular;
	uint32_t rewalked;       /* segments whose guess was not their true entry */
	uint32_t short_stop;
	uint32_t found;          /* records found, the irregular ones among them */
} vc_bam_text_res;
int vc_bam_scan_text_device(vc_bam *b, const uint8_t *d_text, size_t text_bytes, uint64_t entry, const uint64_t *d_cuts,
                            size_t n_cuts, int final, void *stream);
int vc_bam_scan_text_block(vc_bam *b, const uint8_t *text, size_t text_bytes, uint64_t entry, const uint64_t *cuts,
                           size_t n_cuts, int final);
int vc_bam_text_result(vc_bam *b, vc_bam_text_res *res);
int vc_bam_text_kernel_ms(vc_bam *b, float *find_ms, float *check_ms);

/* Many short record chains of one text walked in one launch: what a seeking
 * pass has after it inflated the members of its spans back to back.  A piece
 * is a chain whose first record the index gives: the walk starts at `entry`
 * and takes every record that starts before `stop` and lies whole below
 * `limit`, the end of the piece's own text, under the text scan's walk rule (a
 * record is a block_size >= 32).  limit is clamped to text_bytes, entry and
 * stop to limit; entry >= stop is an empty piece.  One lane walks one piece.
 *
 * A piece ends VC_BAM_PIECE_OK; _CUT, when a record that starts before stop
 * runs past limit (missing: the bytes of it that lie past limit, 0 where not
 * even its block_size word is whole); _SHORT at a block_size < 32; or _NOROOM,
 * when the pieces overlap so far that their records outnumber text_bytes / 36
 * + 1.  Only the records of OK pieces are emitted: each is checked and counted
 * as a record of a text scan is (irregular ones are not counted), in no
 * particular order.  `found` of a piece that did not end OK is the number of
 * records before the one that stopped it.  A caller that sees a cut piece
 * walks it again with more text; one that wants the contract's counts and sees
 * short, irregular or noroom reads the file another way.
 *
 * text_bytes < 2^32 - 16.  Every device read of the text is below the piece's
 * clamped limit.  vc_bam_scan_pieces_device: text and pieces (8-byte aligned)
 * in HBM on `stream`, with vc_count_device's ordering contract.
 * vc_bam_scan_pieces_block: host bytes staged through pinned memory.
 * vc_bam_pieces_result waits for the handle's stream and reports the last
 * piece scan: the totals, the first n_status per-piece outcomes in the
 * pieces' order, and the first n_offs emitted record offsets (a piece's own
 * are offs[first .. first + found), ascending); either array may be NULL.
 * vc_bam_text_kernel_ms reports the walk as find_ms. */
typedef struct {
	uint64_t entry, stop, limit;
} vc_bam_piece;
enum { VC_BAM_PIECE_OK = 0, VC_BAM_PIECE_CUT = 1, VC_BAM_PIECE_SHORT = 2, VC_BAM_PIECE_NOROOM = 3 };
typedef struct {
	uint32_t status;
	uint32_t found;
	uint64_t missing;
	uint32_t first;          /* OK and found > 0: its slot in the emitted list */
	uint32_t reserved;       /* 0 */
} vc_bam_piece_status;
typedef struct {
	uint64_t records;        /* regular records of OK pieces: counted */
	uint64_t bases;
	uint64_t irregular_off;  /* UINT64_MAX without one */
	uint32_t found;          /* records emitted, the irregular ones among them */
	uint32_t irregular;
	uint32_t n_short, n_cut, n_noroom;   /* pieces */
	uint32_t n_pieces;
} vc_bam_pieces_res;
int vc_bam_scan_pieces_device(vc_bam *b, const uint8_t *d_text, size_t text_bytes, const vc_bam_piece *d_pieces,
                              size_t n_pieces, void *stream);
int vc_bam_scan_pieces_block(vc_bam *b, const uint8_t *text, size_t text_bytes, const vc_bam_piece *pieces, size_t n_pieces);
int vc_bam_pieces_result(vc_bam *b, vc_bam_pieces_res *res, vc_bam_piece_status *status, size_t n_status, uint32_t *offs,
                         size_t n_offs);

/* count_bam_variants (bam-vaf-counter.c:417-470) for one file: its own stderr
 * lines, the regions and weights of items 5 and 6 from this file's header and
 * index, every record through the kernels.  n_threads inflate BGZF blocks.
 * VC_EIO: cannot be opened; VC_EINVAL: not BGZF BAM or no readable header
 * (nothing counted in both cases).  st: seqs = records, bases = sum of l_seq,
 * blocks = batches.
 *
 * By default, and with $VAFC_BGZF = device, the members behind the header are copied down
 * compressed, inflated by vc_bgzf_inflate_device and read by
 * vc_bam_scan_text_device, in pieces of whole members; only the counts come
 * back.  The pass gives up, puts the handle's counts back to what they were
 * before the file and leaves the file to the host reader at a member that
 * does not inflate, bytes that are no whole member, an ISIZE above 65,536, an
 * irregular record, a short block_size, or a record longer than a text
 * buffer: the result on such files is the host reader's, and n_threads sizes
 * it.  $VAFC_BGZF = host: the host reader alone (DESIGN 16 has the
 * measurement that decided the default).  vc_bam_inflate_info: the members of the last file that were
 * inflated on the host (header members of a device pass among them) and on
 * the device (0 after a fallback).
 *
 * $VAFC_BAM_INDEX = seek (unset or `ignore`: nothing of this paragraph
 * happens).  A file with an index by item 6 and with regions is read by item
 * 9's plan when its BAI is usable for seeking: per span the members from beg
 * >> 16 through the one at end >> 16 are read with a seek, the spans of a batch
 * ($VAFC_BATCH_BYTES of text, always at least one span) inflated by
 * vc_bgzf_inflate_device back to back, batch k + 1 while batch k is walked,
 * and each span walked as one piece by vc_bam_scan_pieces_device from beg's to
 * end's place in the text.  A piece that ends cut is read once more on its own
 * with as many further members as the missing bytes ask for.  The stderr
 * lines and the counts are those of the whole-file pass; st counts the records
 * read (seqs, bases; blocks = batches, the re-read ones among them) and
 * vc_bam_inflate_info the members inflated (device: every member read, one
 * read a second time counted twice; host: what the host reader, which opens
 * the file for its header and reads ahead on its threads, had inflated when
 * the pass began, so at least the header's and a number that may differ from
 * run to run).  On any
 * doubt the counts are put back and the file is read as without the variable:
 * a compressed offset of the plan that is outside the file or where no whole
 * BGZF member starts, an offset in the text at or past (end: past) its
 * member's ISIZE, a member that does not inflate, a piece that ends short or
 * cut for the second time (the end of the file cuts it every time), an
 * irregular record, or a batch of 2^32 - 16 bytes of text or more.
 * vc_bam_seek_info: the last file's state, one of VC_BAM_SEEK_*, the spans
 * planned, the members read (those of a second reading counted again) and the
 * pieces read again. */
enum {
	VC_BAM_SEEK_OFF = 0,         /* not asked for */
	VC_BAM_SEEK_DONE = 1,        /* the file was read by its index */
	VC_BAM_SEEK_NO_INDEX = 2,    /* no index, one with a wrong magic, or one not usable for seeking (item 9) */
	VC_BAM_SEEK_NO_REGIONS = 3,
	VC_BAM_SEEK_OFFSET = 4,      /* fallbacks from here on */
	VC_BAM_SEEK_INFLATE = 5,
	VC_BAM_SEEK_SHORT = 6,
	VC_BAM_SEEK_IRREGULAR = 7,
	VC_BAM_SEEK_CUT = 8,
	VC_BAM_SEEK_LONG = 9
};
typedef struct {
	uint64_t spans, members, rereads;
	uint32_t state;
	uint32_t reserved;       /* 0 */
} vc_bam_seek_res;
int vc_bam_count_file(vc_bam *b, const char *path, int n_threads, vc_file_stats *st);
int vc_bam_inflate_info(const vc_bam *b, uint64_t *host_members, uint64_t *device_members);
int vc_bam_seek_info(const vc_bam *b, vc_bam_seek_res *res);

/* ------------------------------------------------------------------ */
/* vcf-vaf-counter: genotypes of a VCF as .vaf counts                  */
/* (vcf-vaf-counter.c; line rules of htslib's vcf.c vcf_parse)         */
/* ------------------------------------------------------------------ */

/* The contract, read from vcf-vaf-counter.c and htslib's vcf.c and pinned by
 * the goldens of tests/golden/vcf:
 *
 * 1. Patterns load as vc_patterns_load (the fscanf of vcf-vaf-counter.c:52
 *    is vaf-counter.c:164's); the .vaf writer is vc_write_vaf (:246-273).
 * 2. Row matching (find_pattern :83-92, called at :126).  A record's row is
 *    the FIRST row in file order with strcmp(chr, CHROM) == 0 and start ==
 *    (int)(POS - 1): the cast truncates a 64-bit position (POS = 2^32 + 100 is
 *    start 99), POS 0 and an empty POS are start -1.  A later row with the
 *    same chr and start never receives anything.  POS may have leading zeros
 *    or a '+' (hts_str2uint).  A CHROM the header does not declare is matched
 *    like any other (vcf.c:3686-3696 only warns).
 * 3. Allele filter (:130-135): exactly two alleles (ALT "." is one, "T,G" is
 *    three), REF one byte and ALT one byte, both equal to that first row's
 *    ref and alt exactly (lower case does not match).  A mismatch does not
 *    fall through to a duplicate row.
 * 4. GT (:138-148).  ngt = samples * the largest ploidy on the line; the
 *    reference reads flat entries 2s and 2s+1 for sample index s whatever the
 *    ploidy, and skips the record if 2s+1 >= ngt.  A missing allele ('.'), a
 *    missing trailing GT field and a padding entry all give an allele below
 *    0: skipped.  '/' and '|' are the same.  GT must be Type=String in the
 *    header or absent from it; with another type bcf_get_genotypes refuses.
 * 5. AD (:155-165) is used only if the header declares it Type=Integer (an
 *    undeclared tag is taken as String, vcf.c:2856-2880).  nad = samples *
 *    the longest AD vector on the line; flat entries 2s and 2s+1 are read if
 *    2s+1 < nad, and if both differ from the missing code ('.'), ref =
 *    first, alt = second, depth = their sum.  A padding entry is not missing:
 *    it enters as the vector-end value 0x80000001.
 * 6. DP (:168-188) is tried if depth is still 0 (AD 0,0 included), must be
 *    Type=Integer; flat entry s must exist and not be missing.  Genotype 0/0
 *    gives (DP, 0), 1/1 gives (0, DP), anything else (DP/2, DP - DP/2).
 * 7. depth < min_depth: skipped.  Otherwise the row's two counts are SET,
 *    not added: the last qualifying record in file order wins, and with
 *    min_depth <= 0 a record of depth 0 sets 0 0 (:191-195).
 * 8. What ends the file, keeping everything before it, exit code 0: a line
 *    vcf_parse rejects (:118).  Fewer than 8 columns; a POS that is not
 *    [+]digits below 2^62; a FORMAT tag "."; more than 255 tags; a tag
 *    declared Type=Flag; a sample column with more fields than FORMAT; fewer
 *    sample columns than the header has samples (more are ignored); a GT value
 *    that is neither a number nor '.'; a character other than ':' behind a
 *    value (vcf.c:3216-3229).  An empty line and a '#' line behind the header
 *    are such lines.  These are not: an empty CHROM (a contig like any other,
 *    :3686-3696); an empty FORMAT tag (an undeclared tag like any other,
 *    :2863-2880); a FORMAT column with no sample column behind it
 *    (:3349-3350 turn the error into success: the line is skipped).  One line
 *    ends the PROGRAM: GT named in FORMAT and present in no sample column, on a
 *    line that passes items 2 and 3, makes bcf_get_format_values call exit(1);
 *    no .vaf is written.  An input that cannot be opened, or whose header
 *    cannot be read (it does not begin with ##fileformat=VCF, a data line comes
 *    before the #CHROM line, there is no #CHROM line) gets the reference's
 *    Error: line and counts nothing; the all-zero .vaf is still written, exit 0.
 * 9. Input: plain text, gzip and BGZF (inflated on the device, or on the host
 *    as the multi-member gzip it is: vc_vcf_inflate_info; the result is the
 *    same); a '\r' in front of the '\n' is dropped; a last line needs no '\n'.
 * 10. Deviations.  BCF is refused with a message naming the format.  htslib's
 *    own [W::/[E:: lines are not reproduced.  A negative sample index counts
 *    nothing.  Item 8 is reproduced where the first five columns of ANY line
 *    are malformed, and for every defect named there of a line that passes
 *    items 2 and 3; a line that does not pass them is never looked at behind
 *    its ALT column, where the reference might stop.  FILTER and INFO are not
 *    validated.  Header lines are read for their FORMAT IDs and types only
 *    (first declaration wins).  Compressed input that is damaged or cut off
 *    ends as if the text ended there (htslib stops with a read error in front
 *    of the cut line).  AD/DP values outside int32 and sums that overflow int
 *    are outside the contract. */

typedef struct vc_vcf vc_vcf;
typedef struct vc_vcf_header vc_vcf_header;

/* Bytes of text one workgroup scans per step (256 lanes x 16 bytes): a line
 * belongs to the tile its first byte is in. */
#define VC_VCF_TILE_BYTES 4096

/* One reported line: the file offset of its first byte and the first row
 * with its (CHROM, POS - 1) whose ref / alt equal its REF / ALT, or row = -1
 * for a line the device leaves to the host (fewer than five tabs or a control
 * character in the first five columns, an empty CHROM or one longer than 255
 * bytes (neither is malformed: the host then matches the line itself), a POS
 * that is not 1..18 digits). */
typedef struct {
	uint64_t off;
	int32_t row;
	uint32_t reserved;   /* 0 */
} vc_vcf_hit;

/* Kinds of input, vc_vcf_probe: VC_VCF_BCF* are refused, VC_VCF_OTHER is not
 * VCF (the header read fails as in the reference). */
enum { VC_VCF_PLAIN = 0, VC_VCF_GZIP = 1, VC_VCF_BGZF = 2, VC_VCF_BCF = 3, VC_VCF_OTHER = 4 };
/* What a file is by its first bytes (a compressed one by its first inflated
 * bytes); VC_EIO if it cannot be opened. */
int vc_vcf_probe(const char *path, int *kind);
const char *vc_vcf_kind_name(int kind);

/* Host only.  The header of VCF text: *out holds the sample count and the
 * declared FORMAT types, *body_off the offset of the first data line.
 * Returns VC_OK, VC_EINVAL (item 8: no header), or VC_VCF_MORE when text ends
 * before the #CHROM line does and final == 0. */
#define VC_VCF_MORE 1
/* vc_vcf_count_file: a line ended the program (item 8); the counts are void. */
#define VC_VCF_ABORTED 2
int vc_vcf_header_parse(const uint8_t *text, size_t len, int final, vc_vcf_header **out, size_t *body_off);
int vc_vcf_header_samples(const vc_vcf_header *h);
/* Declared type of a FORMAT tag: htslib's BCF_HT_* (0 Flag, 1 Integer, 2
 * Float, 3 String or Character), -1 undeclared. */
int vc_vcf_header_type(const vc_vcf_header *h, const char *tag);
void vc_vcf_header_free(vc_vcf_header *h);

enum { VC_VCF_SKIP = 0, VC_VCF_SET = 1, VC_VCF_END = 2, VC_VCF_ABORT = 3 };
typedef struct {
	int32_t verdict;       /* VC_VCF_*: what the line does to a row it hits (items 4-8; ABORT: the program ends) */
	int32_t head_ok;       /* its first five columns are well-formed (0: verdict is VC_VCF_END) */
	int64_t pos;           /* POS - 1, untruncated */
	uint32_t chrom_len;    /* CHROM is line[0 .. chrom_len) */
	int32_t n_allele;
	uint32_t ref_len, alt_len;   /* bytes of REF and of the first ALT allele */
	uint8_t ref, alt;      /* their first bytes */
	uint8_t reserved[2];
	uint32_t ref_count, alt_count;   /* verdict VC_VCF_SET */
} vc_vcf_verdict;
/* Host only.  One line (with or without its "\n" / "\r\n") under items 4-8 for
 * sample index sample_idx. */
int vc_vcf_eval_line(const vc_vcf_header *h, const uint8_t *line, size_t len, int sample_idx, int min_depth,
                     vc_vcf_verdict *out);

/* The panel of db as a hash table on HIP device `device`: keyed by (hash of
 * chr, start), one entry per distinct (chr, start) holding the first such
 * row, the chr bytes beside it. */
int vc_vcf_create(vc_vcf **out, const vc_patterns *db, int device);
/* The same from arrays, with table_slots entries (a power of two >= the
 * number of distinct (chr, start), 0: chosen as vc_vcf_create does), so that a
 * test can force every probe to chain.  Names are at most 255 bytes. */
int vc_vcf_create_raw(vc_vcf **out, const char *const *chr, const int32_t *start, const char *ref, const char *alt,
                      size_t n, size_t table_slots, int device);
void vc_vcf_destroy(vc_vcf *v);
/* Scan a block of host text that begins at a line start (staged through
 * pinned memory, asynchronous, text reusable on return).  file_off is the
 * offset of text[0], added to every reported offset.  final == 0: the bytes
 * behind the block's last '\n' are left to the next block; *consumed is the
 * number of bytes scanned (0 when the block holds no '\n').  Lines found are
 * added to those vc_vcf_hits returns. */
int vc_vcf_scan_block(vc_vcf *v, const uint8_t *text, size_t len, uint64_t file_off, int final, size_t *consumed);
/* The same for HBM-resident text (any alignment) on `stream`, with
 * vc_count_device's ordering contract; the bytes consumed come with
 * vc_vcf_hits.  d_text must stay valid until then; a scan still pending from
 * an earlier call is collected (synchronised) first. */
int vc_vcf_scan_device(vc_vcf *v, const uint8_t *d_text, size_t len, uint64_t file_off, int final, void *stream);
/* Wait for the scans since the last call; their lines sorted by offset
 * (valid until the next call on v) and the bytes the last scan consumed.  A
 * scan that found more lines than the list holds is run again with a larger
 * list: the result does not depend on the capacity. */
int vc_vcf_hits(vc_vcf *v, const vc_vcf_hit **hits, size_t *n_hits, size_t *consumed);
/* Test hooks: capacity of the device's hit list (default 1 << 20), and the
 * bytes of one block of vc_vcf_count_file (default 32 MiB; a longer line
 * grows the block). */
int vc_vcf_set_max_hits(vc_vcf *v, size_t max_hits);
int vc_vcf_set_block_bytes(vc_vcf *v, size_t bytes);
/* Elapsed milliseconds of the kernels of the last scan. */
int vc_vcf_kernel_ms(vc_vcf *v, float *ms);
/* process_vcf (vcf-vaf-counter.c:95-204) with its stderr lines: the header on
 * the host, the body through the kernel block by block, the lines it reports
 * through vc_vcf_eval_line in file order; counts[2 * n_patterns] receives
 * item 7's assignments (it is not zeroed).  n_threads inflate gzip input.
 * VC_EIO: cannot be opened; VC_EINVAL: no VCF header, or BCF (nothing is
 * counted in either case); VC_VCF_ABORTED: item 8's line that ends the program.  st: seqs = lines reported by the device, bases =
 * bytes of text, blocks = blocks scanned. */
int vc_vcf_count_file(vc_vcf *v, const char *path, int sample_idx, int min_depth, int n_threads, uint32_t *counts,
                      vc_file_stats *st);
/* How the last vc_vcf_count_file got its text: BGZF members inflated on the
 * device and members inflated on the host (the header's; all of them when the
 * host path ran, 0 and 0 for plain text and for gzip that is not BGZF).  For
 * BGZF input $VAFC_BGZF = host | device picks the path; unset, it is the
 * device's.  A file the device path cannot finish (a member whose status is
 * not 0, bytes that are no whole member before the end of the file, an ISIZE
 * above 65,536) is counted again from its start by the host path before
 * anything is written to counts or stderr: the result is the host path's. */
int vc_vcf_inflate_info(const vc_vcf *v, uint64_t *device_blocks, uint64_t *host_blocks);

/* ------------------------------------------------------------------ */
/* BGZF members inflated on the device                                 */
/* ------------------------------------------------------------------ */

/* The contract:
 *
 * 1. A block is the raw deflate payload of one BGZF member (RFC 1951: stored,
 *    fixed and dynamic blocks), named by a descriptor: in_len payload bytes at
 *    in_off of the compressed buffer, isize bytes of text to out_off of the
 *    output buffer, the trailer's crc32.  Blocks are independent: one wave
 *    inflates one block, and no distance reaches in front of a block's text.
 * 2. A block's status is 0 iff the stream reaches the end of its final
 *    deflate block, the text has exactly isize bytes and its CRC-32 is crc32
 *    (what zlib's raw inflate, its total_out and crc32() say of the same
 *    bytes).  Payload bytes behind the final deflate block are ignored.
 * 3. Otherwise the status is the VC_BGZF_E* code of the first defect in
 *    stream order.  Malformed data never ends in anything else: for every
 *    block the device reads only inside [in_off, in_off + in_len) and reads
 *    and writes only inside [out_off, out_off + isize), and every loop of the
 *    decoder consumes input or produces output.  Text of a block with a
 *    non-zero status is unspecified inside that range.
 * 4. A descriptor with isize or in_len above 65,536, or with a range that is
 *    not inside the buffers of the call, gets VC_BGZF_EISIZE and is not
 *    touched.  Output ranges of different blocks must not overlap. */
typedef struct {
	uint64_t in_off;
	uint32_t in_len;
	uint32_t isize;
	uint64_t out_off;
	uint32_t crc32;
	uint32_t reserved;   /* 0 */
} vc_bgzf_block;

enum {
	VC_BGZF_EBTYPE = 1,    /* block type 3 */
	VC_BGZF_ESTORED = 2,   /* stored block: LEN is not the complement of NLEN */
	VC_BGZF_ETOOMANY = 3,  /* more than 286 literal/length or 30 distance codes */
	VC_BGZF_ELENS = 4,     /* a code-length set that is over-subscribed or (where that is not allowed) incomplete */
	VC_BGZF_EREPEAT = 5,   /* a repeat with no length before it, or one that runs past the last length */
	VC_BGZF_ENOEOB = 6,    /* no end-of-block code */
	VC_BGZF_ESYMBOL = 7,   /* bits that are no code, literal/length symbol 286/287, distance symbol 30/31 */
	VC_BGZF_EDIST = 8,     /* a distance that reaches in front of the block's first byte */
	VC_BGZF_EPAST = 9,     /* more text than isize */
	VC_BGZF_ESHORT = 10,   /* the final deflate block ended with less text than isize */
	VC_BGZF_EINPUT = 11,   /* the payload ended before the final deflate block did */
	VC_BGZF_ECRC = 12,     /* the text's CRC-32 is not crc32 */
	VC_BGZF_EISIZE = 13    /* item 4 */
};

/* Host only.  The whole BGZF members at the front of raw[0..len), as
 * descriptors: in_off from raw[0], out_off running from 0.  *n receives their
 * number (at most cap), *consumed the bytes they take.  Returns why the walk
 * stopped: VC_OK, all len bytes are whole members; VC_BGZF_MORE, the bytes at
 * *consumed can be the front of a member that the end of raw cuts off and
 * final == 0 (call again with more); VC_BGZF_NOT_MEMBER, they are not a BGZF
 * member (another gzip member, other bytes, or a cut member with final != 0);
 * VC_BGZF_TOO_LONG, a member with ISIZE above 65,536; VC_BGZF_FULL, cap
 * descriptors are written and more members follow. */
#define VC_BGZF_MORE 1
#define VC_BGZF_NOT_MEMBER 2
#define VC_BGZF_TOO_LONG 3
#define VC_BGZF_FULL 4
int vc_bgzf_index(const uint8_t *raw, size_t len, int final, vc_bgzf_block *blocks, size_t cap, size_t *n,
                  size_t *consumed);

typedef struct vc_bgzf vc_bgzf;
int vc_bgzf_create(vc_bgzf **out, int device);
void vc_bgzf_destroy(vc_bgzf *z);
/* Inflate n blocks of host bytes raw[0..raw_len) into text[0..text_cap):
 * staged through pinned memory, inflated on the handle's stream, the text
 * copied back; text is complete on return, raw reusable.  The blocks' status
 * comes with vc_bgzf_finish. */
int vc_bgzf_inflate_block(vc_bgzf *z, const uint8_t *raw, size_t raw_len, const vc_bgzf_block *blocks, size_t n,
                          uint8_t *text, size_t text_cap);
/* The same for HBM-resident compressed bytes, descriptors and output (any
 * alignment) on `stream`, with vc_count_device's ordering contract; the
 * buffers must stay valid until vc_bgzf_finish or until `stream` has passed
 * the call.  A later call replaces the status of an earlier one. */
int vc_bgzf_inflate_device(vc_bgzf *z, const uint8_t *d_raw, size_t raw_len, const vc_bgzf_block *d_blocks, size_t n,
                           uint8_t *d_text, size_t text_cap, void *stream);
/* Wait for the last inflate call: status[i] (up to cap of them; may be NULL)
 * of its blocks, *n_blocks their number, *ok_blocks the number of leading
 * blocks whose status is 0 (the text of blocks [0, ok_blocks) is whole). */
int vc_bgzf_finish(vc_bgzf *z, uint32_t *status, size_t cap, size_t *n_blocks, size_t *ok_blocks);
/* Elapsed milliseconds of the kernel of the last inflate call. */
int vc_bgzf_kernel_ms(vc_bgzf *z, float *ms);
/* The handle's own stream (a hipStream_t), what VC_STREAM_CTX stands for. */
void *vc_bgzf_stream(vc_bgzf *z);
const char *vc_bgzf_status_name(uint32_t status);

/* ------------------------------------------------------------------ */
/* Synthetic workload (bench / tests): the generator of vafc_synth.py,  */
/* evaluated on the device.                                            */
/* ------------------------------------------------------------------ */

/* Generate reads first..first+n_reads-1 (fixed length read_len) into device
 * buffers d_seq[n_reads*read_len], d_offs[n_reads], d_lens[n_reads].
 * d_windows: device [n_snp][2][301] ASCII SNP windows, d_dosage: [n_snp] u8. */
int vc_synth_reads(uint8_t *d_seq, uint64_t *d_offs, uint32_t *d_lens, uint64_t first,
                   uint64_t n_reads, uint32_t read_len, uint64_t seed, double f_snp,
                   const uint8_t *d_windows, const uint8_t *d_dosage, uint32_t n_snp,
                   void *stream);

/* Test hook: position-dependent 2-bit decode (vaf-counter.c:261-291) of
 * device-resident reads into d_codes (same offsets as d_seq; 0..3, 4 =
 * invalid) by the kernels' own decode path. */
int vc_debug_decode(const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs,
                    const uint32_t *d_lens, uint64_t n_reads, uint8_t *d_codes, void *stream);

const char *vc_strerror(int err);
int vc_version(void);
/* Hash of the sources this library was built from (16 hex digits: sha256 of
 * every file of kmer-cnt_amd/csrc in name order, then include/vafc.h).  The same string
 * is embedded as "VAFC_BUILD_ID=<hex>" in the library and every CLI, so a
 * checker can compare it with the tree without loading the binary. */
const char *vc_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
