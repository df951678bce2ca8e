// vafc_device.h -- what every piece of host code that owns device memory
// shares.  Host code only.
//
//   HIPCK      a failed HIP call is reported and returned as VC_EHIP
//   vc_now     monotonic seconds
//   VcDevBuf   a move-only owner of one device allocation
//   VcTimer    the two events around a handle's last launch
//
// The handle core that is built from these (VcDevice) is in vafc_stage.h,
// beside the stager it holds.
#ifndef VAFC_DEVICE_H
#define VAFC_DEVICE_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <time.h>

#include "vafc.h"

#define HIPCK(call)                                                                         \
	do {                                                                                    \
		hipError_t e_ = (call);                                                             \
		if (e_ != hipSuccess) {                                                             \
			fprintf(stderr, "[E::vafc] %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), \
			        __FILE__, __LINE__);                                                    \
			return VC_EHIP;                                                                 \
		}                                                                                   \
	} while (0)

// Monotonic seconds.
inline double vc_now()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec + ts.tv_nsec * 1e-9;
}

// One device allocation of `cap` elements, freed by its owner's destructor.
// It converts to T *, so it is passed to HIP calls and into kernel arguments
// like the pointer it replaces.  Every call returns HIP's error for HIPCK.
template <class T> struct VcDevBuf {
	T *p = nullptr;
	size_t cap = 0;   // elements; 0 whenever p is null

	VcDevBuf() = default;
	VcDevBuf(const VcDevBuf &) = delete;
	VcDevBuf &operator=(const VcDevBuf &) = delete;
	VcDevBuf(VcDevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
	VcDevBuf &operator=(VcDevBuf &&o) noexcept
	{
		if (this != &o) {
			free();
			p = o.p, cap = o.cap;
			o.p = nullptr, o.cap = 0;
		}
		return *this;
	}
	~VcDevBuf() { free(); }

	operator T *() const { return p; }
	size_t bytes() const { return cap * sizeof(T); }

	hipError_t alloc(size_t n)
	{
		free();
		const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
		if (e != hipSuccess) p = nullptr;
		cap = p ? n : 0;
		return e;
	}
	// alloc(n) and a synchronous copy of n elements from the host
	hipError_t upload(const T *src, size_t n)
	{
		const hipError_t e = alloc(n);
		return e != hipSuccess || n == 0 ? e : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
	}
	hipError_t zero() { return hipMemset(p, 0, bytes()); }
	hipError_t zero_async(hipStream_t st) { return hipMemsetAsync(p, 0, bytes(), st); }
	void free()
	{
		T *old = p;
		p = nullptr;
		cap = 0;
		if (old) (void)hipFree(old);
	}
	// A fresh buffer of n elements in place of the old one, whose contents are
	// dropped: the lists that are sized on demand.  The capacity is 0 before
	// the old buffer is freed, so a failed allocation leaves an empty buffer.
	// Nothing here waits for the device: either the caller has synchronised
	// the stream that still reads the old list, or it relies on hipFree, which
	// waits for the device.
	hipError_t grow(size_t n)
	{
		T *old = p;
		p = nullptr;
		cap = 0;
		const hipError_t e = old ? hipFree(old) : hipSuccess;
		return e == hipSuccess ? alloc(n) : e;
	}
	// Two lists that share one capacity: both are replaced or both end up empty.
	template <class U> hipError_t grow(size_t n, VcDevBuf<U> &other, size_t n_other)
	{
		other.free();
		hipError_t e = grow(n);
		if (e == hipSuccess) e = other.alloc(n_other);
		if (e != hipSuccess) free();
		return e;
	}
};

// The events around a handle's last launch.
struct VcTimer {
	hipEvent_t t0 = nullptr, t1 = nullptr;
	bool timed = false;   // a launch has been recorded since init / clear

	VcTimer() = default;
	VcTimer(const VcTimer &) = delete;
	VcTimer &operator=(const VcTimer &) = delete;
	~VcTimer() { destroy(); }

	hipError_t init()
	{
		const hipError_t e = hipEventCreate(&t0);
		return e == hipSuccess ? hipEventCreate(&t1) : e;
	}
	void destroy()
	{
		if (t0) (void)hipEventDestroy(t0);
		if (t1) (void)hipEventDestroy(t1);
		t0 = t1 = nullptr;
		timed = false;
	}
	hipError_t begin(hipStream_t st) { return hipEventRecord(t0, st); }
	hipError_t end(hipStream_t st)
	{
		const hipError_t e = hipEventRecord(t1, st);
		timed = timed || e == hipSuccess;
		return e;
	}
	void clear() { timed = false; }
	// Milliseconds of the last launch; VC_EINVAL before any.
	int ms(float *out)
	{
		if (!out || !timed) return VC_EINVAL;
		HIPCK(hipEventSynchronize(t1));
		HIPCK(hipEventElapsedTime(out, t0, t1));
		return VC_OK;
	}
};

#endif
