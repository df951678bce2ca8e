// vafc_bgzf.hip -- BGZF members inflated on the device (vc_bgzf_* of
// include/vafc.h): the kernel around the decoder of vafc_inflate.h, the
// handle, and the host-only index of a buffer's members (vafc_bgzf.h's walk).
//
//   kernel   one wave per workgroup, one BGZF block per wave at a time,
//            grid-striding over the batch.  The decode tables and the CRC table
//            are the workgroup's LDS (sizeof(VciTables), 5,152 bytes).  The bit
//            reader and the symbol loop are wave-uniform; a literal is stored
//            by lane 0, a match or a stored run by all lanes, 64 bytes a step;
//            the CRC-32 is taken slice by slice and joined across the lanes.
//   bounds   a descriptor is checked against the buffers of the call before
//            anything of its block is touched; inside the block the decoder
//            keeps to [in_off, in_off + in_len) and [out_off, out_off + isize)
//            by construction (vafc_inflate.h), whatever the payload holds.
#include <hip/hip_runtime.h>

#include <string.h>

#include <new>
#include <vector>

#include "vafc.h"
#include "vafc_bgzf.h"
#include "vafc_inflate.h"
#include "vafc_stage.h"

static_assert(sizeof(vc_bgzf_block) == 32, "a descriptor is 32 bytes");
static_assert(sizeof(VciTables) <= 10240, "at least 16 one-wave workgroups per CU");
static_assert(VC_BGZF_EISIZE == VCI_EISIZE && VC_BGZF_EBTYPE == VCI_EBTYPE && VC_BGZF_ECRC == VCI_ECRC,
              "the public codes are the decoder's");

namespace {

const int BGZF_WAVE = 64;
const int BGZF_WGS_PER_CU = 32;   // the grid: more than are resident, so a long block does not hold its CU's queue up

struct VcBgzfArgs {
	const uint8_t *raw;
	uint64_t raw_len;
	const vc_bgzf_block *blocks;   // 8-byte aligned
	uint64_t n;
	uint8_t *text;
	uint64_t text_cap;
	uint32_t *status;              // [n]
};

__global__ void __launch_bounds__(BGZF_WAVE) bgzf_inflate_kernel(VcBgzfArgs A)
{
	__shared__ VciTables T;
	const uint32_t lane = threadIdx.x;
	vci_crc_table<BGZF_WAVE>(T, lane);
	for (uint64_t i = blockIdx.x; i < A.n; i += gridDim.x) {
		const vc_bgzf_block d = A.blocks[i];
		int rc;
		if (d.isize > VCI_MAX_TEXT || d.in_len > VCI_MAX_TEXT || d.in_off > A.raw_len || d.in_len > A.raw_len - d.in_off ||
		    d.out_off > A.text_cap || d.isize > A.text_cap - d.out_off)
			rc = VCI_EISIZE;
		else
			rc = vci_inflate<BGZF_WAVE>(T, A.raw + d.in_off, d.in_len, A.text + d.out_off, d.isize, d.crc32, lane);
		if (lane == 0) A.status[i] = (uint32_t)rc;
		__syncthreads();   // the tables are free for the next block
	}
}

} // namespace

struct vc_bgzf : VcDevice {
	VcDevBuf<uint32_t> d_status;
	VcDevBuf<uint8_t> d_text;        // vc_bgzf_inflate_block's output
	size_t n_last = 0;               // blocks of the last call
	hipStream_t last_st = nullptr;   // the stream it ran on
	bool active = false;             // ... and has not been waited for
	std::vector<uint32_t> status;
};

namespace {

int wait_last(vc_bgzf *z)
{
	if (z->active) HIPCK(hipStreamSynchronize(z->last_st));
	z->active = false;
	return VC_OK;
}

// The kernel over n blocks on st; d_status has room for them.
int launch(vc_bgzf *z, const uint8_t *d_raw, size_t raw_len, const vc_bgzf_block *d_blocks, size_t n, uint8_t *d_text,
           size_t text_cap, hipStream_t st)
{
	VcBgzfArgs A;
	A.raw = d_raw;
	A.raw_len = raw_len;
	A.blocks = d_blocks;
	A.n = n;
	A.text = d_text;
	A.text_cap = text_cap;
	A.status = z->d_status;
	uint64_t grid = (uint64_t)z->n_cu * BGZF_WGS_PER_CU;
	if (grid > n) grid = n;
	HIPCK(z->timer.begin(st));
	hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)grid), dim3(BGZF_WAVE), 0, st, A);
	HIPCK(hipGetLastError());
	HIPCK(z->timer.end(st));
	z->n_last = n;
	z->last_st = st;
	z->active = true;
	return VC_OK;
}

// Before a launch: the call before it has left the status list, which then has room for n.
int begin_call(vc_bgzf *z, size_t n)
{
	HIPCK(hipSetDevice(z->dev));
	if (z->d_status.cap < n) {
		const int rc = wait_last(z);
		if (rc != VC_OK) return rc;
		HIPCK(z->d_status.grow(n + n / 4 + 64));
	}
	z->n_last = 0;
	return VC_OK;
}

} // namespace

extern "C" int vc_bgzf_create(vc_bgzf **out, int device)
{
	if (!out) return VC_EINVAL;
	*out = nullptr;
	vc_bgzf *z = new (std::nothrow) vc_bgzf;
	if (!z) return VC_ENOMEM;
	const int rc = z->open(device);
	if (rc != VC_OK) {
		vc_bgzf_destroy(z);
		return rc;
	}
	*out = z;
	return VC_OK;
}

extern "C" void vc_bgzf_destroy(vc_bgzf *z)
{
	if (!z) return;
	(void)hipSetDevice(z->dev);
	if (z->active && z->last_st) (void)hipStreamSynchronize(z->last_st);
	z->close();
	delete z;
}

extern "C" int vc_bgzf_inflate_block(vc_bgzf *z, const uint8_t *raw, size_t raw_len, const vc_bgzf_block *blocks, size_t n,
                                     uint8_t *text, size_t text_cap)
{
	if (!z || (raw_len && !raw) || (n && !blocks) || (text_cap && !text)) return VC_EINVAL;
	int rc = begin_call(z, n);
	if (rc != VC_OK || n == 0) return rc;
	if ((rc = wait_last(z)) != VC_OK) return rc;
	if (z->d_text.cap < text_cap) HIPCK(z->d_text.grow(text_cap + text_cap / 4 + 4096));
	// one pinned buffer: the compressed bytes, then the descriptors at the next multiple of 8
	const size_t desc_at = (raw_len + 7) & ~(size_t)7, bytes = desc_at + n * sizeof(vc_bgzf_block);
	VcSlot *s;
	if ((rc = z->stage.acquire_for(bytes, 1, &s)) != VC_OK) return rc;
	if (raw_len) memcpy(s->h_seq, raw, raw_len);
	memcpy(s->h_seq + desc_at, blocks, n * sizeof(vc_bgzf_block));
	// what lies between the blocks' ranges in `text` is the caller's: it goes to the device and comes back
	if (text_cap) HIPCK(hipMemcpyAsync(z->d_text, text, text_cap, hipMemcpyHostToDevice, z->st));
	rc = z->stage.submit(bytes, 1, z->st, [&](const VcSlot &sl) {
		return launch(z, sl.d_seq, raw_len, reinterpret_cast<const vc_bgzf_block *>(sl.d_seq + desc_at), n, z->d_text,
		              text_cap, z->st);
	}, false);
	if (rc != VC_OK) return rc;
	if (text_cap) HIPCK(hipMemcpyAsync(text, z->d_text, text_cap, hipMemcpyDeviceToHost, z->st));
	HIPCK(hipStreamSynchronize(z->st));
	z->stage.settle();
	return VC_OK;
}

extern "C" int vc_bgzf_inflate_device(vc_bgzf *z, const uint8_t *d_raw, size_t raw_len, const vc_bgzf_block *d_blocks,
                                      size_t n, uint8_t *d_text, size_t text_cap, void *stream)
{
	if (!z || (raw_len && !d_raw) || (n && !d_blocks) || (text_cap && !d_text) || ((uintptr_t)d_blocks & 7)) return VC_EINVAL;
	const int rc = begin_call(z, n);
	if (rc != VC_OK || n == 0) return rc;
	return z->on_stream(stream, [&](hipStream_t st) { return launch(z, d_raw, raw_len, d_blocks, n, d_text, text_cap, st); });
}

extern "C" int vc_bgzf_finish(vc_bgzf *z, uint32_t *status, size_t cap, size_t *n_blocks, size_t *ok_blocks)
{
	if (!z || (cap && !status)) return VC_EINVAL;
	HIPCK(hipSetDevice(z->dev));
	const int rc = wait_last(z);
	if (rc != VC_OK) return rc;
	z->status.resize(z->n_last);
	if (z->n_last) HIPCK(hipMemcpy(z->status.data(), z->d_status, z->n_last * sizeof(uint32_t), hipMemcpyDeviceToHost));
	size_t ok = 0;
	while (ok < z->n_last && z->status[ok] == 0) ++ok;
	if (status) memcpy(status, z->status.data(), (cap < z->n_last ? cap : z->n_last) * sizeof(uint32_t));
	if (n_blocks) *n_blocks = z->n_last;
	if (ok_blocks) *ok_blocks = ok;
	return VC_OK;
}

extern "C" int vc_bgzf_kernel_ms(vc_bgzf *z, float *ms)
{
	return z ? z->timer.ms(ms) : VC_EINVAL;
}

extern "C" void *vc_bgzf_stream(vc_bgzf *z)
{
	return z ? (void *)z->st : nullptr;
}

extern "C" const char *vc_bgzf_status_name(uint32_t status)
{
	switch (status) {
	case 0: return "ok";
	case VC_BGZF_EBTYPE: return "block type 3";
	case VC_BGZF_ESTORED: return "stored block: LEN and NLEN disagree";
	case VC_BGZF_ETOOMANY: return "too many length or distance symbols";
	case VC_BGZF_ELENS: return "invalid code-length set";
	case VC_BGZF_EREPEAT: return "invalid code-length repeat";
	case VC_BGZF_ENOEOB: return "missing end-of-block code";
	case VC_BGZF_ESYMBOL: return "invalid literal/length or distance symbol";
	case VC_BGZF_EDIST: return "distance before the block's start";
	case VC_BGZF_EPAST: return "output past ISIZE";
	case VC_BGZF_ESHORT: return "output short of ISIZE at the final block";
	case VC_BGZF_EINPUT: return "input exhausted";
	case VC_BGZF_ECRC: return "CRC-32 mismatch";
	case VC_BGZF_EISIZE: return "ISIZE above 65,536 or a range outside the buffers";
	}
	return "?";
}

extern "C" int vc_bgzf_index(const uint8_t *raw, size_t len, int final, vc_bgzf_block *blocks, size_t cap, size_t *n,
                             size_t *consumed)
{
	if ((len && !raw) || (cap && !blocks) || !n || !consumed) return VC_EINVAL;
	size_t at = 0, k = 0;
	uint64_t out_off = 0;
	int why = VC_OK;
	while (at < len) {
		VcBgzfMember m;
		const int rc = vc_bgzf_member_at(raw + at, len - at, &m);
		if (rc == 0) {
			why = final ? VC_BGZF_NOT_MEMBER : VC_BGZF_MORE;
			break;
		}
		if (rc < 0) {
			why = VC_BGZF_NOT_MEMBER;
			break;
		}
		if (m.isize > VC_BGZF_MAX_TEXT) {
			why = VC_BGZF_TOO_LONG;
			break;
		}
		if (k == cap) {
			why = VC_BGZF_FULL;
			break;
		}
		vc_bgzf_block &b = blocks[k++];
		b.in_off = at + m.payload;
		b.in_len = (uint32_t)m.payload_len;
		b.isize = m.isize;
		b.out_off = out_off;
		b.crc32 = m.crc32;
		b.reserved = 0;
		out_off += m.isize;
		at += m.size;
	}
	*n = k;
	*consumed = at;
	return why;
}
