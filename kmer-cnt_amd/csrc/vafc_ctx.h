// vafc_ctx.h -- the core of a read counter (the vc_ctx of include/vafc.h):
// what the pattern counter (PanelCounter, vafc_host.cpp) and the histogram
// counter (KcCounter, vafc_kc_host.cpp) share, and the four virtual members
// through which the shard code (vafc_shards.cpp) and the file passes
// (vafc_files.cpp) reach a kind's kernels and tables.  Host code only.
#ifndef VAFC_CTX_H
#define VAFC_CTX_H

#include <hip/hip_runtime.h>

#include <vector>

#include "vafc_affinity.h"
#include "vafc_common.h"
#include "vafc_stage.h"

typedef struct ncclComm *ncclComm_t;   // as rccl.h has it; only vafc_shards.cpp includes that

// The core's `stage` takes the host batches (vc_count_block, the sequential file pass).
struct vc_ctx : VcDevice {
	int k = 21;
	std::vector<VcSlot> islot;             // parallel ingest (vc_count_file on plain files)
	hipStream_t cst = nullptr;             // the parallel reader's H2D copies (created on first use)
	bool ingest_warm = false;              // a parallel-reader pass has completed: its slots are pinned
	bool timing = false;              // vc_set_timing: the timer records only while this is on
	VcCpuSet cpus;                    // the GPUs' NUMA-node CPUs for the reader threads (gpu_cpus)
	int cpus_threads = -1;            // the thread count cpus was computed for
	// multi-GPU (vc_create_multi): this ctx is shard 0; rep[i - 1] is shard i
	std::vector<vc_ctx *> rep;
	std::vector<int> lead;                 // per shard: the first shard on the same device
	std::vector<ncclComm_t> comms;         // one rank per distinct device, rank 0 = shard 0
	std::vector<int> comm_shard;           // the shard each rank reduces
	uint64_t rr = 0;                       // host batches dealt so far (round robin)
	uint64_t batches = 0;                  // batches counted by this shard (vc_shard_info)

	virtual ~vc_ctx() {}
	// Enqueue the kind's kernels over device-resident reads on stream st.
	// may_long = false: the caller knows no read is longer than VC_LONG_READ (a
	// host batch), so the long-read kernel and its list reset are not launched.
	virtual int launch(const uint8_t *d_seq, size_t seq_bytes, const uint64_t *d_offs, const uint32_t *d_lens,
	                   uint64_t n_reads, hipStream_t st, bool may_long = true) = 0;
	// vc_finish: wait for this shard and check its kernel error flags (before
	// the shards are reduced); then, the stream idle, copy the results out.
	virtual int check() { return VC_OK; }
	virtual int result(uint32_t *counts, uint64_t *kmers) = 0;
	virtual int clear() = 0;               // vc_reset: zero the outputs, asynchronously on st

	int submit(size_t bytes, uint64_t n_reads);   // the acquired slot of `stage`: H2D copies + kernels
};

static inline int n_shards(const vc_ctx *c) { return 1 + (int)c->rep.size(); }
static inline vc_ctx *shard_at(vc_ctx *c, int i) { return i == 0 ? c : c->rep[(size_t)i - 1]; }
// The shard that takes the next host batch.
static inline vc_ctx *next_shard(vc_ctx *c) { return shard_at(c, (int)(c->rr++ % (uint64_t)n_shards(c))); }

// Whether any of n host-side read lengths takes the long-read kernel.
static inline bool any_long(const uint32_t *lens, uint64_t n)
{
	uint32_t m = 0;
	for (uint64_t i = 0; i < n; ++i) m = lens[i] > m ? lens[i] : m;
	return m > VC_LONG_READ;
}

// vafc_shards.cpp, for vc_finish and vc_destroy of a pattern counter: the sum
// of the shards' n counts and k-mer tallies into shard 0; the communicators
// and the replicas freed.
int reduce_shards(vc_ctx *c, size_t n);
void destroy_shards(vc_ctx *c);

#endif
