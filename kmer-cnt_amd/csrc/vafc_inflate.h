// vafc_inflate.h -- raw deflate (RFC 1951) of one BGZF block by one wave,
// shared by the kernel (vafc_bgzf.hip) and, with a one-lane "wave", by host
// programs (tools/bgzf_inflate_check.cpp runs this text under the sanitizers).
// Not part of the public C ABI (include/vafc.h), but for the status codes,
// which are VC_BGZF_E* there.  Written from the RFC: stored, fixed and dynamic
// blocks; nothing here comes from zlib.
//
// Shape.  The bit reader and the symbol loop are the same in every lane of the
// wave (LANES of them): every lane reads the same input bytes and takes the
// same branches.  Lanes differ only where the work is shared out: building the
// decode tables, storing a literal (lane 0), copying a match or a stored run
// (lane i takes bytes i, i + LANES, ...), and the CRC-32 (lane i takes the
// i-th slice of the text).
//
// Tables (VciTables, 5,152 bytes; in LDS on the device).  A code is kept in
// canonical form: cnt[len] codes of each length and the symbols sorted by
// (length, symbol), from which a code is decoded a bit at a time with the
// RFC's next_code recurrence.  In front of that stands a direct table on the
// next VCI_LBITS / VCI_DBITS input bits, filled by running that same decode
// on every index; a longer code, and an index no code owns, misses it (entry
// 0) and is decoded, or refused, bit by bit.
//
// Bounds, by construction (the machine that runs this is shared, and the
// input is whatever a file holds):
//   * input is read only through VciBits, at byte positions < len;
//   * output is written, and a match's source read, only at positions < isize:
//     a literal checks op < isize, a match and a stored run op + n <= isize,
//     a match dist <= op;
//   * every trip of every loop consumes at least one input bit, produces at
//     least one output byte, or advances a counter with a fixed bound (288
//     code lengths, 15 code bits, 64 lanes), so the symbol loops end after at
//     most 8 * len + isize trips whatever the data says; `budget` counts them
//     and ends the decode should that reasoning ever fail;
//   * table indices: a symbol taken from sym[] is below the n the table was
//     built for; positions in sym[] are below the number of coded symbols by
//     the over-subscription check (vci_build refuses a set it fails).
// Malformed data ends in one of the codes below and in nothing else.
#ifndef VAFC_INFLATE_H
#define VAFC_INFLATE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VCI_HD __host__ __device__ __forceinline__
#else
#define VCI_HD inline
#endif

// Per-block status (VC_BGZF_E* of include/vafc.h): 0 = the text is there, has
// ISIZE bytes and the trailer's CRC-32.
enum {
	VCI_OK = 0,
	VCI_EBTYPE = 1,     // block type 3
	VCI_ESTORED = 2,    // stored block: LEN != ~NLEN
	VCI_ETOOMANY = 3,   // dynamic header: more than 286 literal/length or 30 distance codes
	VCI_ELENS = 4,      // a code-length set that is over-subscribed, or incomplete where that is not allowed
	VCI_EREPEAT = 5,    // repeat code 16 with nothing before it, or a repeat that runs past the last length
	VCI_ENOEOB = 6,     // the literal/length code has no end-of-block symbol
	VCI_ESYMBOL = 7,    // bits that are no code of the table, or literal/length symbol 286/287, distance symbol 30/31
	VCI_EDIST = 8,      // a distance that reaches in front of the block's first byte
	VCI_EPAST = 9,      // more text than ISIZE
	VCI_ESHORT = 10,    // the final block ended with less text than ISIZE
	VCI_EINPUT = 11,    // the payload ended before the final block did
	VCI_ECRC = 12,      // the text's CRC-32 is not the trailer's
	VCI_EISIZE = 13,    // the descriptor: ISIZE above 65,536, or a range outside the buffers it names
	VCI_NCODES = 14
};

#define VCI_MAX_TEXT 65536u   // of one BGZF block
#define VCI_LBITS 10          // direct-table bits of the literal/length code
#define VCI_DBITS 8           // ... of the distance code (and, with 7 of them, of the code-length code)
#define VCI_CRC_POLY 0xEDB88320u

struct VciCode {
	uint16_t cnt[16];    // codes of each length; cnt[0] = 0
	uint16_t sym[288];   // symbols by (length, symbol)
};

struct VciTables {
	uint16_t lfast[1 << VCI_LBITS];   // symbol | length << 9; 0 = decode bit by bit
	uint16_t dfast[1 << VCI_DBITS];
	VciCode lit, dist;                // dist (and the code-length code, before it) uses 32 of sym[]
	uint8_t lens[320];                // code lengths as the header gives them: literal/length, then distance
	uint8_t cl[32];                   // lengths of the code-length code
	uint32_t crc[256];                // raw CRC-32 of one byte
};

// What a lane needs to know of its wave.
template <int LANES> struct VciWave {
	static VCI_HD void sync()
	{
#if defined(__HIP_DEVICE_COMPILE__)
		if (LANES > 1) __syncthreads();   // one wave per workgroup: orders its LDS and global accesses
#endif
	}
	// Before a lane reads text that another lane of the wave stored: a wave's
	// memory operations are performed in the order it issues them, so this
	// only keeps the compiler from moving accesses across it.
	static VCI_HD void text_fence()
	{
#if defined(__HIP_DEVICE_COMPILE__)
		if (LANES > 1) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#endif
	}
	static VCI_HD uint32_t shfl_down(uint32_t v, int d)
	{
#if defined(__HIP_DEVICE_COMPILE__)
		if (LANES > 1) return (uint32_t)__shfl_down((int)v, (unsigned)d, 64);
#endif
		(void)d;
		return v;
	}
	static VCI_HD uint32_t from_lane0(uint32_t v)
	{
#if defined(__HIP_DEVICE_COMPILE__)
		if (LANES > 1) return (uint32_t)__shfl((int)v, 0, 64);
#endif
		return v;
	}
};

// ---------------------------------------------------------------------------
// Bit reader: LSB first; buf holds cnt valid bits (bits above them are either
// zero or a copy of the input bits that come next, never anything else).
// ---------------------------------------------------------------------------
struct VciBits {
	const uint8_t *in;
	uint32_t len, pos;   // next byte to load; pos <= len
	uint64_t buf;
	uint32_t cnt;
	int err;             // VCI_EINPUT once more bits were asked for than the payload has
};

VCI_HD void vci_bits_open(VciBits &b, const uint8_t *in, uint32_t len)
{
	b.in = in;
	b.len = len;
	b.pos = 0;
	b.buf = 0;
	b.cnt = 0;
	b.err = VCI_OK;
}

// At least 56 valid bits, or all that are left.
VCI_HD void vci_refill(VciBits &b)
{
	if (b.len - b.pos >= 8) {
		uint64_t w;
		__builtin_memcpy(&w, b.in + b.pos, 8);
		b.buf |= w << b.cnt;
		const uint32_t take = (63 - b.cnt) >> 3;
		b.pos += take;
		b.cnt += take * 8;
	} else {
		while (b.cnt < 56 && b.pos < b.len) {
			b.buf |= (uint64_t)b.in[b.pos++] << b.cnt;
			b.cnt += 8;
		}
	}
}

VCI_HD uint32_t vci_peek(const VciBits &b, uint32_t n) { return (uint32_t)b.buf & ((1u << n) - 1u); }

VCI_HD void vci_drop(VciBits &b, uint32_t n)
{
	if (n > b.cnt) {
		b.err = VCI_EINPUT;
		n = b.cnt;
	}
	b.buf >>= n;
	b.cnt -= n;
}

// n <= 16 bits
VCI_HD uint32_t vci_take(VciBits &b, uint32_t n)
{
	const uint32_t v = vci_peek(b, n);
	vci_drop(b, n);
	return v;
}

// ---------------------------------------------------------------------------
// Canonical codes
// ---------------------------------------------------------------------------

// The symbol whose code the low bits of v begin with, among codes of at most
// max_len bits: its symbol | length << 9, or 0 when those bits begin no code.
// RFC 1951 3.2.2: codes of one length are consecutive, the first of length n
// is (first of n - 1 + count of n - 1) << 1.
VCI_HD uint32_t vci_canon(const VciCode &c, uint32_t v, uint32_t max_len)
{
	uint32_t code = 0, first = 0, index = 0;
	for (uint32_t len = 1; len <= max_len; ++len) {
		code = code << 1 | (v & 1u);
		v >>= 1;
		const uint32_t n = c.cnt[len];
		if (code - first < n) return c.sym[index + (code - first)] | len << 9;
		index += n;
		first = (first + n) << 1;
	}
	return 0;
}

// The code of n symbols with lengths lens[0..n), and its direct table on
// fast_bits bits.  cl: the code-length code, which may not be incomplete.
// Returns VCI_OK or VCI_ELENS, the same in every lane.
template <int LANES>
VCI_HD int vci_build(VciCode &c, uint16_t *fast, uint32_t fast_bits, const uint8_t *lens, uint32_t n, bool cl,
                     uint32_t lane)
{
	VciWave<LANES>::sync();   // lens is written
	for (uint32_t l = lane; l < 16; l += LANES) {
		uint32_t k = 0;
		for (uint32_t s = 0; s < n; ++s) k += lens[s] == l ? 1u : 0u;
		c.cnt[l] = (uint16_t)(l ? k : 0);
	}
	VciWave<LANES>::sync();
	int32_t left = 1;
	uint32_t max = 0;
	bool over = false;
	for (uint32_t l = 1; l < 16; ++l) {
		const uint32_t k = c.cnt[l];
		left = left * 2 - (int32_t)k;   // k <= 288 and left <= 2^15: no overflow
		if (left < 0) over = true;
		if (over) left = 0;
		if (k) max = l;
	}
	// a set with no code at all decodes nothing, which is an error only when a
	// symbol is asked of it; one code of one bit is the other incomplete set
	// that deflate allows (a single distance code)
	if (over || (max != 0 && left > 0 && (cl || max != 1))) return VCI_ELENS;
	for (uint32_t l = 1 + lane; l < 16; l += LANES) {
		uint32_t at = 0;
		for (uint32_t m = 1; m < l; ++m) at += c.cnt[m];
		for (uint32_t s = 0; s < n; ++s)
			if (lens[s] == l) c.sym[at++] = (uint16_t)s;   // at < the number of coded symbols <= n
	}
	VciWave<LANES>::sync();
	for (uint32_t j = lane; j < (1u << fast_bits); j += LANES) fast[j] = (uint16_t)vci_canon(c, j, fast_bits);
	VciWave<LANES>::sync();
	return VCI_OK;
}

// The next symbol of a code: from the direct table, else bit by bit.  -1 with
// b.err or *err set when there is none.
VCI_HD int32_t vci_symbol(VciBits &b, const VciCode &c, const uint16_t *fast, uint32_t fast_bits, int *err)
{
	uint32_t e = fast[vci_peek(b, fast_bits)];
	if (e == 0) e = vci_canon(c, (uint32_t)b.buf & 0x7FFFu, 15);
	if (e == 0) {
		// no code begins like this; with fewer than 15 bits left it may be the end of the payload instead
		*err = b.cnt < 15 ? VCI_EINPUT : VCI_ESYMBOL;
		return -1;
	}
	vci_drop(b, e >> 9);
	if (b.err) return -1;
	return (int32_t)(e & 511u);
}

// ---------------------------------------------------------------------------
// CRC-32 (the gzip one: reflected, polynomial VCI_CRC_POLY).  In this form bit
// 31 of a word is the coefficient of x^0.
// ---------------------------------------------------------------------------

// a * b mod P
VCI_HD uint32_t vci_gf_mul(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) {
		if (a & (0x80000000u >> i)) p ^= b;
		b = (b >> 1) ^ ((b & 1u) ? VCI_CRC_POLY : 0u);   // b * x
	}
	return p;
}

// x^(8 n) mod P
VCI_HD uint32_t vci_gf_x8n(uint32_t n)
{
	uint32_t r = 0x80000000u, base = 0x00800000u;   // 1, x^8
	for (; n; n >>= 1) {
		if (n & 1u) r = vci_gf_mul(r, base);
		base = vci_gf_mul(base, base);
	}
	return r;
}

template <int LANES> VCI_HD void vci_crc_table(VciTables &T, uint32_t lane)
{
	for (uint32_t i = lane; i < 256; i += LANES) {
		uint32_t r = i;
		for (int k = 0; k < 8; ++k) r = (r >> 1) ^ ((r & 1u) ? VCI_CRC_POLY : 0u);
		T.crc[i] = r;
	}
	VciWave<LANES>::sync();
}

// The CRC-32 of text[0..n), n <= VCI_MAX_TEXT; valid in lane 0 (the same in
// every lane when LANES is 1).  The register of a CRC is linear in (its
// initial value, the message): with initial value 0 ("raw") zero bytes in
// front of a message change nothing, and raw(A B) = raw(A) x^(8 |B|) + raw(B).
// So the text is cut into LANES slices of L bytes that end at its end (the
// first slices may be short or empty), each lane takes the raw CRC of one, and
// six pairwise steps with x^(8 L), x^(16 L), ... join them.  The initial
// 0xFFFFFFFF of the real CRC then enters as 0xFFFFFFFF x^(8 n).
template <int LANES> VCI_HD uint32_t vci_crc32(const VciTables &T, const uint8_t *text, uint32_t n, uint32_t lane)
{
	const uint32_t L = (n + LANES - 1) / LANES;
	// slice `lane` is [n - (LANES - lane) L, n - (LANES - 1 - lane) L) cut to [0, n)
	const uint32_t back_lo = (uint32_t)(LANES - lane) * L, back_hi = (uint32_t)(LANES - 1 - lane) * L;
	const uint32_t lo = back_lo > n ? 0 : n - back_lo, hi = back_hi > n ? 0 : n - back_hi;
	uint32_t c = 0;
	for (uint32_t i = lo; i < hi; ++i) c = (c >> 8) ^ T.crc[(c ^ text[i]) & 255u];
	uint32_t pw = vci_gf_x8n(L);
	for (int d = 1; d < LANES; d <<= 1) {
		const uint32_t right = VciWave<LANES>::shfl_down(c, d);
		if ((lane & (uint32_t)(2 * d - 1)) == 0) c = vci_gf_mul(c, pw) ^ right;
		pw = vci_gf_mul(pw, pw);
	}
	return c ^ vci_gf_mul(0xFFFFFFFFu, vci_gf_x8n(n)) ^ 0xFFFFFFFFu;
}

// ---------------------------------------------------------------------------
// The decoder
// ---------------------------------------------------------------------------

// RFC 1951 3.2.7: the i-th length of the code-length code belongs to symbol
// 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 (five bits each, packed).
VCI_HD uint32_t vci_cl_order(uint32_t i)
{
	const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
	                    10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
	const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
	return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// The symbols of one fixed or dynamic block up to its end-of-block code.
template <int LANES>
VCI_HD int vci_symbols(VciBits &b, const VciTables &T, uint8_t *out, uint32_t isize, uint32_t &op, uint32_t &budget,
                       uint32_t lane)
{
	for (;;) {
		if (budget-- == 0) return VCI_EINPUT;
		if (b.cnt < 48) vci_refill(b);   // a length and its distance take at most 15 + 5 + 15 + 13 bits
		int err = VCI_OK;
		int32_t s = vci_symbol(b, T.lit, T.lfast, VCI_LBITS, &err);
		if (s < 0) return b.err ? b.err : err;
		if (s < 256) {
			if (op >= isize) return VCI_EPAST;
			if (lane == 0) out[op] = (uint8_t)s;
			++op;
			continue;
		}
		if (s == 256) return VCI_OK;
		s -= 257;
		if (s >= 29) return VCI_ESYMBOL;
		// RFC 1951 3.2.5: lengths 3..10 one code each, then four codes per extra bit, 258 alone
		uint32_t len;
		if (s < 8) len = 3 + (uint32_t)s;
		else if (s == 28) len = 258;
		else {
			const uint32_t eb = ((uint32_t)s - 4) >> 2;
			len = 3 + ((4 + ((uint32_t)s & 3u)) << eb) + vci_take(b, eb);
		}
		const int32_t d = vci_symbol(b, T.dist, T.dfast, VCI_DBITS, &err);
		if (d < 0) return b.err ? b.err : err;
		if (d >= 30) return VCI_ESYMBOL;
		// distances 1..4 one code each, then two codes per extra bit
		uint32_t dist;
		if (d < 4) dist = 1 + (uint32_t)d;
		else {
			const uint32_t eb = ((uint32_t)d - 2) >> 1;
			dist = 1 + ((2 + ((uint32_t)d & 1u)) << eb) + vci_take(b, eb);
		}
		if (b.err) return b.err;
		if (dist > op) return VCI_EDIST;
		if (len > isize - op) return VCI_EPAST;
		// every source byte is in [op - dist, op): text the wave has stored.  A
		// match longer than its distance repeats those dist bytes, so byte i
		// comes from i mod dist and no lane waits for another's store.
		VciWave<LANES>::text_fence();
		const uint8_t *src = out + (op - dist);
		if (dist >= len) {
			for (uint32_t i = lane; i < len; i += LANES) out[op + i] = src[i];
		} else {
			for (uint32_t i = lane; i < len; i += LANES) out[op + i] = src[i % dist];
		}
		VciWave<LANES>::text_fence();
		op += len;
	}
}

// Inflate the raw deflate stream in[0..in_len) into out[0..isize) and check
// its length and CRC-32.  Bytes behind the final block are ignored.  Returns
// a VCI_* code, the same in every lane.
template <int LANES>
VCI_HD int vci_inflate(VciTables &T, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t isize, uint32_t want_crc,
                       uint32_t lane)
{
	if (isize > VCI_MAX_TEXT || in_len > VCI_MAX_TEXT) return VCI_EISIZE;   // no BGZF member is longer
	VciBits b;
	vci_bits_open(b, in, in_len);
	uint32_t op = 0;
	// trips of the block and symbol loops: each takes a bit or gives a byte
	uint32_t budget = 8u * in_len + isize + 8u;
	for (;;) {
		if (budget-- == 0) return VCI_EINPUT;
		vci_refill(b);
		const uint32_t bfinal = vci_take(b, 1), btype = vci_take(b, 2);
		if (b.err) return b.err;
		if (btype == 3) return VCI_EBTYPE;
		if (btype == 0) {
			vci_drop(b, b.cnt & 7u);
			vci_refill(b);
			const uint32_t len = vci_take(b, 16), nlen = vci_take(b, 16);
			if (b.err) return b.err;
			if (len != (nlen ^ 0xFFFFu)) return VCI_ESTORED;
			// cnt is a multiple of 8 here: the bytes still in the buffer go back
			const uint32_t at = b.pos - (b.cnt >> 3);
			if (len > in_len - at) return VCI_EINPUT;
			if (len > isize - op) return VCI_EPAST;
			for (uint32_t i = lane; i < len; i += LANES) out[op + i] = in[at + i];
			op += len;
			b.pos = at + len;
			b.buf = 0;
			b.cnt = 0;
		} else {
			// the fixed code: 288 and 32 symbols, of which 286, 287, 30 and 31 only fill the code space
			uint32_t hlit = 288, hdist = 32;
			if (btype == 1) {
				VciWave<LANES>::sync();   // nobody still decodes with the old tables
				for (uint32_t i = lane; i < 320; i += LANES)
					T.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
			} else {
				hlit = 257 + vci_take(b, 5);
				hdist = 1 + vci_take(b, 5);
				const uint32_t hclen = 4 + vci_take(b, 4);
				if (b.err) return b.err;
				if (hlit > 286 || hdist > 30) return VCI_ETOOMANY;
				VciWave<LANES>::sync();
				for (uint32_t i = lane; i < 32; i += LANES) T.cl[i] = 0;
				VciWave<LANES>::sync();
				for (uint32_t i = 0; i < hclen; ++i) {
					if (b.cnt < 3) vci_refill(b);
					const uint32_t v = vci_take(b, 3);
					if (lane == 0) T.cl[vci_cl_order(i)] = (uint8_t)v;
				}
				if (b.err) return b.err;
				// the code-length code borrows the distance code's tables
				int rc = vci_build<LANES>(T.dist, T.dfast, 7, T.cl, 19, true, lane);
				if (rc != VCI_OK) return rc;
				uint32_t n = 0, prev = 0;
				const uint32_t total = hlit + hdist;
				while (n < total) {   // every trip adds at least one length
					if (b.cnt < 32) vci_refill(b);
					int err = VCI_OK;
					const int32_t s = vci_symbol(b, T.dist, T.dfast, 7, &err);
					if (s < 0) return b.err ? b.err : err;
					uint32_t rep = 1, val = (uint32_t)s;
					if (s == 16) {
						if (n == 0) return VCI_EREPEAT;
						rep = 3 + vci_take(b, 2);
						val = prev;
					} else if (s == 17) {
						rep = 3 + vci_take(b, 3);
						val = 0;
					} else if (s == 18) {
						rep = 11 + vci_take(b, 7);
						val = 0;
					}
					if (b.err) return b.err;
					if (rep > total - n) return VCI_EREPEAT;
					for (uint32_t i = lane; i < rep; i += LANES) T.lens[n + i] = (uint8_t)val;
					n += rep;
					prev = val;
				}
				VciWave<LANES>::sync();
				if (T.lens[256] == 0) return VCI_ENOEOB;
			}
			int rc = vci_build<LANES>(T.lit, T.lfast, VCI_LBITS, T.lens, hlit, false, lane);
			if (rc == VCI_OK) rc = vci_build<LANES>(T.dist, T.dfast, VCI_DBITS, T.lens + hlit, hdist, false, lane);
			if (rc == VCI_OK) rc = vci_symbols<LANES>(b, T, out, isize, op, budget, lane);
			if (rc != VCI_OK) return rc;
		}
		if (bfinal) break;
	}
	if (op != isize) return VCI_ESHORT;
	VciWave<LANES>::sync();   // the text is stored
	// lane 0 holds it, and every lane returns the same code
	const uint32_t crc = VciWave<LANES>::from_lane0(vci_crc32<LANES>(T, out, isize, lane));
	return crc == want_crc ? VCI_OK : VCI_ECRC;
}

#endif
