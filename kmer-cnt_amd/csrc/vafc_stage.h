// vafc_stage.h -- how host batches reach the device and what a long-lived
// device handle is made of, shared by the four handles (vc_ctx, in its two
// kinds: the pattern counter and the histogram counter of vafc_ctx.h; vc_ed,
// vc_bam, vc_vcf).  Host code only.
//
//   VcSlot          pinned + device buffers of one batch, released by an event
//   VcStager        two slots filled and shipped in turn on the handle's stream;
//                   acquire_for() gives the next slot with room for a block
//   VcBatchWriter   reads appended into the open slot, a full slot submitted
//   VcStreamBridge  a launch on a caller's stream, ordered with the handle's
//   VcDevice        the core of a handle: device, stream, stager, bridge, timer;
//                   open(), close(), stream_of(), on_stream()
//
// HIPCK, vc_now, the owning device buffer VcDevBuf and VcTimer are
// vafc_device.h, which the one-shot device functions use on their own.
#ifndef VAFC_STAGE_H
#define VAFC_STAGE_H

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <utility>

#include "vafc.h"
#include "vafc_device.h"

struct VcSlot {
	uint8_t *h_seq = nullptr;     // pinned
	uint64_t *h_offs = nullptr;
	uint32_t *h_lens = nullptr;
	uint8_t *d_seq = nullptr;
	uint64_t *d_offs = nullptr;
	uint32_t *d_lens = nullptr;
	size_t cap_bytes = 0, cap_reads = 0;
	hipEvent_t done = nullptr;    // the kernels that read the device buffers have run
	hipEvent_t copied = nullptr;  // parallel reader: the slot's H2D copies (copy stream) are done
	bool pending = false;         // a batch is in flight: wait for `done` before writing
	void *map = nullptr;          // one registered mapping holds h_seq, h_offs, h_lens (slot_alloc_mapped)
	size_t map_len = 0;
	bool d_one = false;           // d_offs, d_lens point into d_seq's allocation
};

// Free a slot's buffers; its events stay.
inline void vc_slot_free(VcSlot &s)
{
	if (s.map) {
		(void)hipHostUnregister(s.map);
		munmap(s.map, s.map_len);
	} else {
		if (s.h_seq) (void)hipHostFree(s.h_seq);
		if (s.h_offs) (void)hipHostFree(s.h_offs);
		if (s.h_lens) (void)hipHostFree(s.h_lens);
	}
	if (s.d_seq) (void)hipFree(s.d_seq);
	if (!s.d_one) {
		if (s.d_offs) (void)hipFree(s.d_offs);
		if (s.d_lens) (void)hipFree(s.d_lens);
	}
	const hipEvent_t done = s.done, copied = s.copied;
	s = VcSlot();
	s.done = done;
	s.copied = copied;
}

inline void vc_slot_destroy(VcSlot &s)
{
	vc_slot_free(s);
	if (s.done) (void)hipEventDestroy(s.done);
	if (s.copied) (void)hipEventDestroy(s.copied);
	s.done = s.copied = nullptr;
}

// Wait until a slot's previous batch has left its buffers.
inline int vc_slot_wait(VcSlot &s)
{
	if (s.pending) HIPCK(hipEventSynchronize(s.done));
	s.pending = false;
	return VC_OK;
}

// New buffers of exactly (bytes, reads) for an idle slot; the first keep_bytes
// and keep_reads entries of the old ones are carried over.  If an allocation
// fails the slot is left as it was.
inline int vc_slot_realloc(VcSlot &s, size_t bytes, size_t reads, size_t keep_bytes, size_t keep_reads)
{
	VcSlot n;
	if (hipHostMalloc((void **)&n.h_seq, bytes, hipHostMallocDefault) != hipSuccess ||
	    hipHostMalloc((void **)&n.h_offs, reads * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess ||
	    hipHostMalloc((void **)&n.h_lens, reads * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
	    hipMalloc((void **)&n.d_seq, bytes) != hipSuccess ||
	    hipMalloc((void **)&n.d_offs, reads * sizeof(uint64_t)) != hipSuccess ||
	    hipMalloc((void **)&n.d_lens, reads * sizeof(uint32_t)) != hipSuccess) {
		fprintf(stderr, "[E::vafc] batch buffers of %zu bytes, %zu reads: %s\n", bytes, reads,
		        hipGetErrorString(hipGetLastError()));
		vc_slot_free(n);
		return VC_EHIP;
	}
	if (keep_bytes) memcpy(n.h_seq, s.h_seq, keep_bytes);
	if (keep_reads) {
		memcpy(n.h_offs, s.h_offs, keep_reads * sizeof(uint64_t));
		memcpy(n.h_lens, s.h_lens, keep_reads * sizeof(uint32_t));
	}
	n.cap_bytes = bytes;
	n.cap_reads = reads;
	n.done = s.done;
	n.copied = s.copied;
	vc_slot_free(s);
	s = n;
	return VC_OK;
}

// Room for `bytes` and `reads` in a slot whose contents are not needed; a
// dimension that grows gets a quarter of headroom.
inline int vc_slot_reserve(VcSlot &s, size_t bytes, size_t reads)
{
	if (bytes <= s.cap_bytes && reads <= s.cap_reads) return VC_OK;
	const int rc = vc_slot_wait(s);
	if (rc != VC_OK) return rc;
	return vc_slot_realloc(s, s.cap_bytes >= bytes ? s.cap_bytes : bytes + bytes / 4 + 4096,
	                       s.cap_reads >= reads ? s.cap_reads : reads + reads / 4 + 1024, 0, 0);
}

// Two slots used in turn: the host fills one while the device reads the other.
struct VcStager {
	VcSlot slot[2];
	int cur = 0;

	int init()
	{
		for (VcSlot &s : slot) HIPCK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
		return VC_OK;
	}
	void destroy()
	{
		for (VcSlot &s : slot) vc_slot_destroy(s);
	}
	// The slot to fill next, once its previous batch has left it.
	int acquire(VcSlot **out)
	{
		*out = &slot[cur];
		return vc_slot_wait(slot[cur]);
	}
	// The same, with room for a block of (bytes, reads).
	int acquire_for(size_t bytes, size_t reads, VcSlot **out)
	{
		const int rc = acquire(out);
		return rc == VC_OK ? vc_slot_reserve(**out, bytes, reads) : rc;
	}
	// H2D copies of the acquired slot's first n_reads reads (bytes of sequence)
	// and launch(slot) on stream st; the slot is released by its event.  A batch
	// that keeps its per-record data inside the byte buffer (the BAM counter's
	// descriptors) passes per_read = false: offs and lens are not shipped.
	template <class Launch>
	int submit(size_t bytes, uint64_t n_reads, hipStream_t st, Launch &&launch, bool per_read = true)
	{
		VcSlot &s = slot[cur];
		if (n_reads) {
			if (bytes) HIPCK(hipMemcpyAsync(s.d_seq, s.h_seq, bytes, hipMemcpyHostToDevice, st));
			if (per_read) {
				HIPCK(hipMemcpyAsync(s.d_offs, s.h_offs, n_reads * sizeof(uint64_t), hipMemcpyHostToDevice, st));
				HIPCK(hipMemcpyAsync(s.d_lens, s.h_lens, n_reads * sizeof(uint32_t), hipMemcpyHostToDevice, st));
			}
			const int rc = launch(s);
			if (rc != VC_OK) return rc;
			HIPCK(hipEventRecord(s.done, st));
			s.pending = true;
		}
		cur ^= 1;
		return VC_OK;
	}
	// After the stream has been synchronised: no batch is in flight.
	void settle()
	{
		for (VcSlot &s : slot) s.pending = false;
	}
};

// $VAFC_BATCH_BYTES (test knob: smaller batches) or dflt: the sequence bytes
// of one batch of a file pass, which size its slots as well.
inline size_t vc_batch_bytes(size_t dflt)
{
	const char *e = getenv("VAFC_BATCH_BYTES");
	return e && atoll(e) >= 1 ? (size_t)atoll(e) : dflt;
}

// Reads of a file are written straight into a pinned slot; a full slot is
// shipped to the device and the next one is filled meanwhile.  next() gives
// the handle that takes the next batch (NULL: it cannot be used); a handle has
// a VcStager `stage` and submit(bytes, n_reads) for its acquired slot.  A batch
// is closed by the read that would take it past `limit` bytes or `max_reads`
// reads; a single longer read grows its (empty) slot.
template <class Next> struct VcBatchWriter {
	size_t limit, max_reads;
	Next next;
	decltype(std::declval<Next &>()()) h = nullptr;   // handle of the open slot
	VcSlot *s = nullptr;
	size_t bytes = 0;
	uint64_t n = 0;
	uint64_t batches = 0;           // submitted so far
	int err = VC_OK;

	VcBatchWriter(size_t limit_bytes, size_t limit_reads, Next nx)
	    : limit(limit_bytes), max_reads(limit_reads ? limit_reads : 1), next(nx)
	{
	}

	int open_slot()
	{
		if (!(h = next())) return VC_EHIP;
		const int rc = h->stage.acquire_for(limit, max_reads, &s);
		if (rc != VC_OK) s = nullptr;
		bytes = 0;
		n = 0;
		return rc;
	}
	int flush()
	{
		if (!s) return VC_OK;
		const int rc = h->submit(bytes, n);
		batches += n ? 1 : 0;
		s = nullptr;
		bytes = 0;
		n = 0;
		return rc;
	}
	int add(const char *seq, size_t len)
	{
		if (!s && (err = open_slot()) != VC_OK) return err;
		if (n > 0 && (bytes + len > limit || n >= max_reads)) {
			if ((err = flush()) != VC_OK) return err;
			if ((err = open_slot()) != VC_OK) return err;
		}
		// only the first read of a batch can be longer than the room left
		if (len > s->cap_bytes - bytes && (err = vc_slot_reserve(*s, len, 1)) != VC_OK) return err;
		if (len) memcpy(s->h_seq + bytes, seq, len);
		s->h_offs[n] = bytes;
		s->h_lens[n] = (uint32_t)len;
		bytes += len;
		++n;
		return VC_OK;
	}
};

// A launch on a stream other than the handle's own: own's work so far -> that
// stream (in), and the launch -> own (out), so that a reset before the call,
// the finish after it and the shard sum, all on own, stay ordered with it
// without a host sync.  The events are created on first use; on the handle's
// own stream enter and leave do nothing.
struct VcStreamBridge {
	hipEvent_t in = nullptr, out = nullptr;

	int enter(hipStream_t own, hipStream_t st)
	{
		if (st == own) return VC_OK;
		if (!in) HIPCK(hipEventCreateWithFlags(&in, hipEventDisableTiming));
		if (!out) HIPCK(hipEventCreateWithFlags(&out, hipEventDisableTiming));
		HIPCK(hipEventRecord(in, own));           // e.g. a reset before this call
		HIPCK(hipStreamWaitEvent(st, in, 0));
		return VC_OK;
	}
	int leave(hipStream_t own, hipStream_t st)
	{
		if (st == own) return VC_OK;
		HIPCK(hipEventRecord(out, st));
		HIPCK(hipStreamWaitEvent(own, out, 0));   // finish waits on own only
		return VC_OK;
	}
	void destroy()
	{
		if (in) (void)hipEventDestroy(in);
		if (out) (void)hipEventDestroy(out);
		in = out = nullptr;
	}
};

// What every long-lived handle has around its own tables: a handle derives
// from this, declares its tables as VcDevBuf members, and its destroy
// function is close() and delete.
struct VcDevice {
	int dev = 0;
	int n_cu = 256;
	hipStream_t st = nullptr;   // the handle's own, non-blocking
	VcStager stage;
	VcStreamBridge bridge;      // a launch on a caller's stream
	VcTimer timer;

	// VC_ENODEV without a device, VC_EINVAL for one that is not there; then
	// the device is made current and the stream and every event are created.
	// After a failure the owner still calls close().
	int open(int device)
	{
		int ndev = 0;
		if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VC_ENODEV;
		if (device < 0 || device >= ndev) return VC_EINVAL;
		HIPCK(hipSetDevice(device));
		dev = device;
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
			n_cu = prop.multiProcessorCount;
		HIPCK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
		HIPCK(timer.init());
		return stage.init();
	}
	// Before the handle is deleted: waits for the stream and destroys the
	// events.  The delete then frees the handle's VcDevBuf members while the
	// stream still exists, and this base's destructor destroys the stream last.
	void close()
	{
		(void)hipSetDevice(dev);
		if (st) (void)hipStreamSynchronize(st);
		stage.destroy();
		timer.destroy();
		bridge.destroy();
	}
	~VcDevice()
	{
		if (st) (void)hipStreamDestroy(st);
	}
	// NULL is HIP's null stream (ordered with the legacy default stream, which
	// is torch's default stream), as for every HIP API; VC_STREAM_CTX is the
	// handle's own stream.
	hipStream_t stream_of(void *stream) const { return stream == VC_STREAM_CTX ? st : (hipStream_t)stream; }
	// launch(stream) on a caller's stream, ordered with the handle's own.
	template <class Launch> int on_stream(void *stream, Launch &&launch)
	{
		const hipStream_t s = stream_of(stream);
		int rc = bridge.enter(st, s);
		if (rc == VC_OK) rc = launch(s);
		if (rc == VC_OK) rc = bridge.leave(st, s);
		return rc;
	}
};

#endif
