/* stub_xzk_dec.c -- TEST INFRASTRUCTURE ONLY: the decoder half of the kernels_api.h layer on the CPU (next to stub_xzk.c), so
 * that the plain-C host code of the device decoder (xzamd_framing.c, xzamd_decode.c, xzamd_file.c) runs without a GPU and
 * under sanitizers (tests/test_host_decode.py, driven by driver_decode.c).  "Device" memory is host memory.  The Block Header
 * kernel is xzb_block per record (xzamd_block_parse.h, the text the device compiles too), the scan gives one unit per Block,
 * the decode is the oracle's LZMA2 decoder, the comparisons are byte-wise; of the inverse filters only delta is real (BCJ
 * stages copy).  Every call appends itself to a trace: its name and its scalar arguments, no pointers (a pointer shows as
 * 0 / 1: absent / present), no wave counts -- what the host code decided, which a refactor of it must leave alone:
 *   headers(xz_size,nblocks)  scan(nblocks,units_cap,split,rec,rec_stride,nrec)  d2d(bytes)
 *   units(nblocks,units_cap,total_units,expected,per_unit,rec,rec_stride)  unfilter(nblocks,stage,total_tiles,kinds)
 *   compare(n)  compare_blocks(nblocks,total_tiles)  and, from stub_xzk.c, crc(n,block_size,nblocks,strip,crc32)
 *   sha256(n,block_size,nblocks)  x86_bcj(n,block_size,nblocks)  prefilter(n,block_size,nblocks,kind,dist) */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../xz_amd/csrc/kernels_api.h"
#include "../../xz_amd/csrc/xzamd_block_parse.h"
#include "../../oracle/oracle.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the hooks of stub_xzk.c (off by default) */
extern void (*stub_xzk_trace)(const char *fmt, ...);
extern int (*stub_xzk_sha256)(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint8_t *d_out32);

static char *g_trace;
static size_t g_len, g_cap;
static int64_t g_scan_fail = -1;

static void trace(const char *fmt, ...)
{
	char line[256];
	va_list ap;
	va_start(ap, fmt);
	const int n = vsnprintf(line, sizeof(line), fmt, ap);
	va_end(ap);
	if (n <= 0) return;
	if (g_len + (size_t)n + 2 > g_cap) {
		g_cap = 2 * g_cap + 4096;
		g_trace = (char *)realloc(g_trace, g_cap);
		if (!g_trace) abort();
	}
	memcpy(g_trace + g_len, line, (size_t)n);
	g_len += (size_t)n;
	g_trace[g_len++] = ' ';
	g_trace[g_len] = 0;
}

/* the trace so far ("" when empty); stub_dec_trace_reset empties it */
const char *stub_dec_trace(void) { return g_trace && g_len ? g_trace : ""; }
void stub_dec_trace_reset(void) { g_len = 0; if (g_trace) g_trace[0] = 0; }
void stub_dec_trace_free(void) { free(g_trace); g_trace = NULL; g_len = g_cap = 0; }
/* the next scan reports error 11 (unit table full) for Block k */
void stub_dec_scan_fail(uint64_t k) { g_scan_fail = (int64_t)k; }

/* check/sha256.c restated (FIPS 180-4) */
static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
void stub_sha256(const uint8_t *p, uint64_t n, uint8_t out[32])
{
	static const uint32_t K[64] = {
		0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
		0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
		0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
		0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
		0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
		0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
		0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2 };
	uint32_t h[8] = { 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19 };
	const uint64_t total = (n + 9 + 63) & ~63ull;
	for (uint64_t off = 0; off < total; off += 64) {
		uint8_t blk[64];
		uint32_t w[64], s[8];
		for (uint32_t i = 0; i < 64; ++i) {
			const uint64_t q = off + i;
			blk[i] = q < n ? p[q] : q == n ? 0x80 : q >= total - 8 ? (uint8_t)((n * 8) >> (8 * (total - 1 - q))) : 0;
		}
		for (int i = 0; i < 16; ++i)
			w[i] = (uint32_t)blk[4 * i] << 24 | (uint32_t)blk[4 * i + 1] << 16 | (uint32_t)blk[4 * i + 2] << 8 | blk[4 * i + 3];
		for (int i = 16; i < 64; ++i)
			w[i] = w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7]
					+ (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10));
		memcpy(s, h, sizeof(s));
		for (int i = 0; i < 64; ++i) {
			const uint32_t t1 = s[7] + (ror(s[4], 6) ^ ror(s[4], 11) ^ ror(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + K[i] + w[i];
			const uint32_t t2 = (ror(s[0], 2) ^ ror(s[0], 13) ^ ror(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
			s[7] = s[6]; s[6] = s[5]; s[5] = s[4]; s[4] = s[3] + t1; s[3] = s[2]; s[2] = s[1]; s[1] = s[0]; s[0] = t1 + t2;
		}
		for (int i = 0; i < 8; ++i) h[i] += s[i];
	}
	for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(h[i / 4] >> (8 * (3 - i % 4)));
}

static int sha256_blocks(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint8_t *d_out32)
{
	for (uint32_t b = 0; b < nblocks; ++b) {
		const uint64_t bs = (uint64_t)b * block_size;
		const uint64_t len = bs >= n ? 0 : n - bs < block_size ? n - bs : block_size;
		stub_sha256(d_in + (len ? bs : 0), len, d_out32 + 32 * (uint64_t)b);
	}
	return 0;
}

/* switch the trace of this unit's and of stub_xzk.c's functions on, and the real SHA-256 in */
void stub_dec_enable(void) { stub_xzk_trace = trace; stub_xzk_sha256 = sha256_blocks; }

int xzk_dec_headers(const uint8_t *d_xz, uint64_t xz_size, const xzamd_hdr_rec *d_recs, uint32_t nblocks, void *d_table, void *stream)
{
	(void)stream;
	trace("headers(%llu,%u)", (unsigned long long)xz_size, nblocks);
	if (nblocks == 0) return 0;
	xzamd_dec_block *blocks = (xzamd_dec_block *)d_table;
	xzamd_dec_chain *chains = (xzamd_dec_chain *)(blocks + nblocks);
	uint8_t *stored = (uint8_t *)(chains + nblocks);
	xzamd_hdr_err *errs = (xzamd_hdr_err *)(stored + (uint64_t)nblocks * XZAMD_HDR_CHECK_BYTES);
	for (uint32_t b = 0; b < nblocks; ++b) {
		xzamd_hdr_rec r = d_recs[b];
		uint32_t step = XZB_S_NONE;
		if (r.end > xz_size) r.hpos = r.end = 0;
		errs[b].code = xzb_block(d_xz, &r, &blocks[b], &chains[b], stored + (uint64_t)b * XZAMD_HDR_CHECK_BYTES, &step);
		errs[b].step = step;
	}
	return 0;
}

int xzk_dec_scan(const uint8_t *d_xz, xzamd_dec_block *d_blocks, uint32_t nblocks, xzamd_dec_unit *d_units,
		uint32_t units_cap, int split, const uint8_t *d_rec, uint32_t rec_stride, uint32_t nrec, void *stream)
{
	(void)d_xz; (void)stream;
	trace("scan(%u,%u,%d,%d,%u,%u)", nblocks, units_cap, split, d_rec != NULL, rec_stride, nrec);
	for (uint32_t b = 0; b < nblocks; ++b) {
		xzamd_dec_unit *u = &d_units[(uint64_t)b * units_cap];
		memset(u, 0, sizeof(*u));
		u->cpos = d_blocks[b].cpos; u->block = b; u->rec = XZAMD_RESUME_NONE;
		d_blocks[b].nunits = 1; d_blocks[b].error = 0; d_blocks[b].nrecs = 0;
		if (g_scan_fail == (int64_t)b) { d_blocks[b].nunits = 0; d_blocks[b].error = 11; }
	}
	g_scan_fail = -1;
	return 0;
}

int xzk_dec_units(const uint8_t *d_xz, const xzamd_dec_block *d_blocks, uint32_t nblocks, const xzamd_dec_unit *d_units,
		uint32_t units_cap, const uint32_t *d_unit_first, uint32_t total_units, uint8_t *d_out, const uint8_t *d_expected,
		uint16_t *d_lit_pool, uint32_t waves, uint32_t *d_counter, uint32_t *d_block_err, int per_unit,
		const uint8_t *d_rec, uint32_t rec_stride, void *stream)
{
	(void)d_units; (void)d_lit_pool; (void)waves; (void)d_counter; (void)stream;
	trace("units(%u,%u,%u,%d,%d,%d,%u)", nblocks, units_cap, total_units,
			d_expected != NULL, per_unit, d_rec != NULL, rec_stride);
	for (uint32_t b = 0; b < nblocks; ++b) {
		const xzamd_dec_block *B = &d_blocks[b];
		uint64_t got = 0;
		if (d_unit_first[b + 1] == d_unit_first[b]) continue;      /* taken out of the decode by the host */
		if (orc_lzma2_decode(d_xz + B->cpos, B->csize, B->dict_size, d_out + B->upos, B->usize, &got, NULL) || got != B->usize)
			d_block_err[b] = 1;
	}
	return 0;
}

int xzk_dec_compare(const uint8_t *a, const uint8_t *b, uint64_t n, unsigned long long *d_mismatches, void *stream)
{
	(void)stream;
	trace("compare(%llu)", (unsigned long long)n);
	for (uint64_t i = 0; i < n; ++i) *d_mismatches += a[i] != b[i];
	return 0;
}

int xzk_dec_compare_blocks(const uint8_t *d_out, const uint8_t *d_expected, const xzamd_dec_block *d_blocks,
		const uint32_t *d_tile_first, uint32_t nblocks, uint32_t total_tiles, unsigned long long *d_counts, void *stream)
{
	(void)stream;
	trace("compare_blocks(%u,%u)", nblocks, total_tiles);
	for (uint32_t b = 0; b < nblocks; ++b) {
		if (d_tile_first[b + 1] == d_tile_first[b]) continue;
		for (uint64_t i = d_blocks[b].upos; i < d_blocks[b].upos + d_blocks[b].usize; ++i) d_counts[b] += d_out[i] != d_expected[i];
	}
	return 0;
}

int xzk_dec_unfilter(const xzamd_unf_args *a, uint32_t total_tiles, uint32_t kinds, void *stream)
{
	(void)stream;
	trace("unfilter(%u,%u,%u,%u)", a->nblocks, a->stage, total_tiles, kinds);
	for (uint32_t b = 0; b < a->nblocks; ++b) {
		const xzamd_dec_chain *ch = &a->chains[b];
		const uint64_t up = a->blocks[b].upos, n = a->blocks[b].usize;
		if (a->tile_first[b + 1] == a->tile_first[b]) continue;
		const uint8_t *src = ((a->stage & 1) ? a->t1 : a->t0) + up;
		uint8_t *dst = (ch->n == 0 || a->stage + 1 == ch->n ? a->out : (a->stage & 1) ? a->t0 : a->t1) + up;
		const uint32_t f = ch->n ? ch->f[ch->n - 1 - a->stage] : 0;
		const uint64_t dist = (f & 0xFFu) == 3u ? (f >> 8) + 1 : 0;
		for (uint64_t i = 0; i < n; ++i) dst[i] = (uint8_t)(src[i] + (dist && i >= dist ? dst[i - dist] : 0));
	}
	return 0;
}

int xzk_d2d(void *dst, const void *src, uint64_t bytes, void *stream)
{
	(void)stream;
	trace("d2d(%llu)", (unsigned long long)bytes);
	memcpy(dst, src, bytes);
	return 0;
}
