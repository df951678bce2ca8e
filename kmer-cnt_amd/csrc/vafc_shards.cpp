// vafc_shards.cpp -- the multi-GPU shards of a pattern counter (SURVEY.md
// §8(e)), and the only unit that knows RCCL.  The reference counts every block of
// every file into one set of u32 counters (vaf-counter.c:473-477, files in
// order :647-650) and writes them once (:653-681).  Here each shard (one per
// entry of the device list) holds a replica of the static table and its own
// counts; host batches are dealt round robin over the shards, the block loop
// and its stop rule still run once, in file order, on the host.  vc_finish
// reduces: shards sharing a device are summed on it (vc_shard_add_kernel),
// then one RCCL reduce (sum) of the per-device vectors to shard 0 over xGMI.
// u32 addition modulo 2^32 commutes, so the result is bit-identical to one
// device counting everything.
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <mutex>

#include "vafc_ctx.h"
#include "vafc_internal.h"

namespace {

// RCCL, loaded on first use so that single-GPU users do not need it.
struct RcclApi {
	bool tried = false, ok = false;
	decltype(&ncclCommInitAll) comm_init_all = nullptr;
	decltype(&ncclCommDestroy) comm_destroy = nullptr;
	decltype(&ncclReduce) reduce = nullptr;
	decltype(&ncclGroupStart) group_start = nullptr;
	decltype(&ncclGroupEnd) group_end = nullptr;
	decltype(&ncclGetErrorString) error_string = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mu;

const RcclApi *rccl()
{
	std::lock_guard<std::mutex> lk(g_rccl_mu);
	if (g_rccl.tried) return g_rccl.ok ? &g_rccl : nullptr;
	g_rccl.tried = true;
	// VAFC_RCCL_LIB names another library (tests point it at a missing file
	// to exercise the RCCL-missing path)
	const char *env = getenv("VAFC_RCCL_LIB");
	void *h = dlopen(env && *env ? env : "librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
	if (!h && !(env && *env)) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
	if (!h) {
		fprintf(stderr, "[E::vafc] cannot load RCCL: %s\n", dlerror());
		return nullptr;
	}
	RcclApi &R = g_rccl;
	R.comm_init_all = (decltype(R.comm_init_all))dlsym(h, "ncclCommInitAll");
	R.comm_destroy = (decltype(R.comm_destroy))dlsym(h, "ncclCommDestroy");
	R.reduce = (decltype(R.reduce))dlsym(h, "ncclReduce");
	R.group_start = (decltype(R.group_start))dlsym(h, "ncclGroupStart");
	R.group_end = (decltype(R.group_end))dlsym(h, "ncclGroupEnd");
	R.error_string = (decltype(R.error_string))dlsym(h, "ncclGetErrorString");
	R.ok = R.comm_init_all && R.comm_destroy && R.reduce && R.group_start && R.group_end && R.error_string;
	if (!R.ok) fprintf(stderr, "[E::vafc] RCCL lacks the symbols vafc needs\n");
	return R.ok ? &R : nullptr;
}

} // namespace

#define NCCK(R, call)                                                                               \
	do {                                                                                            \
		ncclResult_t e_ = (call);                                                                   \
		if (e_ != ncclSuccess) {                                                                    \
			fprintf(stderr, "[E::vafc] %s failed: %s (%s:%d)\n", #call, (R)->error_string(e_),      \
			        __FILE__, __LINE__);                                                            \
			return VC_EHIP;                                                                         \
		}                                                                                           \
	} while (0)

static void rccl_comms_destroy(vc_ctx *c)
{
	if (c->comms.empty()) return;
	const RcclApi *R = rccl();
	if (R)
		for (ncclComm_t m : c->comms) (void)R->comm_destroy(m);
	c->comms.clear();
	c->comm_shard.clear();
}

void destroy_shards(vc_ctx *c)
{
	rccl_comms_destroy(c);
	for (vc_ctx *r : c->rep) vc_destroy(r);
	c->rep.clear();
}

extern "C" int vc_create_multi(vc_ctx **out, int k, const uint64_t *keys, const uint32_t *vals, size_t n_keys,
                               uint32_t n_patterns, const int *devices, int n_devices)
{
	if (!out || !devices || n_devices < 1 || n_devices > VC_MAX_SHARDS) return VC_EINVAL;
	*out = nullptr;
	// RCCL is needed only to reduce across distinct devices (shards that share
	// a device are summed on it); load it before any device is touched, so a
	// missing library fails fast and leaves nothing to free
	int n_distinct = 0;
	for (int i = 0; i < n_devices; ++i) {
		bool seen = false;
		for (int j = 0; j < i; ++j) seen = seen || devices[j] == devices[i];
		n_distinct += seen ? 0 : 1;
	}
	if (n_distinct > 1 && !rccl()) return VC_EHIP;
	vc_ctx *c = nullptr;
	int rc = vc_create(&c, k, keys, vals, n_keys, n_patterns, devices[0]);
	if (rc != VC_OK) return rc;
	c->lead.assign(1, 0);
	for (int i = 1; i < n_devices; ++i) {
		vc_ctx *r = nullptr;
		if ((rc = vc_create(&r, k, keys, vals, n_keys, n_patterns, devices[i])) != VC_OK) {
			vc_destroy(c);
			return rc;
		}
		c->rep.push_back(r);
		int l = i;
		for (int j = 0; j < i; ++j)
			if (devices[j] == devices[i]) {
				l = j;
				break;
			}
		c->lead.push_back(l);
	}
	if (n_distinct > 1) {
		// one RCCL rank per distinct device; rank 0 is shard 0 (the reduce root)
		const RcclApi *R = rccl();
		std::vector<int> devs;
		for (int i = 0; i < n_devices; ++i)
			if (c->lead[(size_t)i] == i) {
				devs.push_back(devices[i]);
				c->comm_shard.push_back(i);
			}
		c->comms.assign(devs.size(), nullptr);
		const ncclResult_t e = R->comm_init_all(c->comms.data(), (int)devs.size(), devs.data());
		if (e != ncclSuccess) {
			fprintf(stderr, "[E::vafc] ncclCommInitAll over %d devices failed: %s\n", (int)devs.size(),
			        R->error_string(e));
			c->comms.clear();
			vc_destroy(c);
			return VC_EHIP;
		}
	}
	*out = c;
	return VC_OK;
}

// A shard's active outputs (own or bound), as the public getters give them.
static uint32_t *counts_of(vc_ctx *sh) { return (uint32_t *)vc_device_counts(sh); }
static unsigned long long *tally_of(vc_ctx *sh) { return (unsigned long long *)vc_device_tally(sh); }

// All shards' counts (and k-mer tallies) into shard 0; the other shards
// restart from zero, so the sum over shards is unchanged and vc_finish may be
// called again.
int reduce_shards(vc_ctx *c, size_t n)
{
	const int N = n_shards(c);
	for (int i = 0; i < N; ++i) {   // every batch counted
		vc_ctx *sh = shard_at(c, i);
		HIPCK(hipSetDevice(sh->dev));
		HIPCK(hipStreamSynchronize(sh->st));
	}
	for (int i = 0; i < N; ++i) {   // same-device shards into the device's first shard
		const int l = c->lead[(size_t)i];
		if (l == i) continue;
		vc_ctx *L = shard_at(c, l), *S = shard_at(c, i);
		HIPCK(hipSetDevice(L->dev));
		HIPCK(vc_launch_shard_add(counts_of(L), counts_of(S), n, tally_of(L), tally_of(S), L->st));
	}
	if (c->comms.size() <= 1) {   // one distinct device: the on-device sum is the whole sum
		HIPCK(hipSetDevice(c->dev));
		HIPCK(hipStreamSynchronize(c->st));
		return VC_OK;
	}
	const RcclApi *R = rccl();
	if (!R) return VC_EHIP;
	NCCK(R, R->group_start());
	// every enqueue goes in, and the group is always closed, before an error
	// is returned: an open group would leave RCCL's thread-local state pending
	// for the next collective or for ncclCommDestroy in vc_destroy
	ncclResult_t first = ncclSuccess;
	for (size_t j = 0; j < c->comms.size() && first == ncclSuccess; ++j) {
		vc_ctx *L = shard_at(c, c->comm_shard[j]);
		(void)hipSetDevice(L->dev);   // the rank's device (its comm and stream live there)
		// in place on every rank: sendbuff == recvbuff; non-root ranks' buffers
		// are left as they were (zeroed below)
		if (n) first = R->reduce(counts_of(L), counts_of(L), n, ncclUint32, ncclSum, 0, c->comms[j], L->st);
		if (first == ncclSuccess)
			first = R->reduce(tally_of(L), tally_of(L), 1, ncclUint64, ncclSum, 0, c->comms[j], L->st);
	}
	const ncclResult_t ge = R->group_end();
	if (first == ncclSuccess) first = ge;
	if (first != ncclSuccess) {
		fprintf(stderr, "[E::vafc] RCCL reduce of the shard counts failed: %s\n", R->error_string(first));
		return VC_EHIP;
	}
	for (size_t j = 1; j < c->comms.size(); ++j) {   // non-root ranks restart from zero
		vc_ctx *L = shard_at(c, c->comm_shard[j]);
		HIPCK(hipSetDevice(L->dev));
		HIPCK(hipMemsetAsync(counts_of(L), 0, n * sizeof(uint32_t), L->st));
		HIPCK(hipMemsetAsync(tally_of(L), 0, sizeof(unsigned long long), L->st));
	}
	for (size_t j = 0; j < c->comms.size(); ++j) {
		vc_ctx *L = shard_at(c, c->comm_shard[j]);
		HIPCK(hipSetDevice(L->dev));
		HIPCK(hipStreamSynchronize(L->st));
	}
	return VC_OK;
}

extern "C" int vc_shard_count(const vc_ctx *c) { return c ? n_shards(c) : 0; }

extern "C" int vc_shard_info(const vc_ctx *c, int i, int *device, uint64_t *batches)
{
	if (!c || i < 0 || i >= n_shards(c)) return VC_EINVAL;
	const vc_ctx *sh = shard_at(const_cast<vc_ctx *>(c), i);
	if (device) *device = sh->dev;
	if (batches) *batches = sh->batches;
	return VC_OK;
}
