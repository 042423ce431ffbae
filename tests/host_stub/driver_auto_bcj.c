/* driver_auto_bcj.c -- TEST INFRASTRUCTURE ONLY: the host side of the automatic per-Block BCJ filter (XZAMD_F_AUTO_BCJ:
 * xz_amd/csrc/xzamd_host.c, xzamd_frame.c, xzamd_options.c) over the CPU stand-ins of the kernel layer (stub_xzk.c,
 * stub_xzk_delta.c, stub_xzk_autobcj.c), as a stand-alone program under ASan / UBSan (tests/test_host_auto_bcj.py).
 *
 * Five Blocks of 128 KiB -- text, an int32 walk, synthetic x86 code, synthetic ARM64 code whose other words are a walk (so the
 * delta rule fires on it too), and a short tail of the x86 code -- so that one job holds Blocks with no filter, a delta filter
 * and both BCJ filters, planned from three header sizes.  Checked: the chain and size of every Block Header, that every Block's
 * LZMA2 payload decodes (through the oracle) to the input as its filter leaves it and carries the right Check, the framing of
 * the Stream, XZAMD_F_BLOCKS_ONLY, the precedence of the BCJ rule over the delta rule, a stored Block (no filter in its header),
 * both encode modes of the host layer, several batches in one call, the analysis on its own, the debug fetches and the
 * combinations the flag declines.  With a path as argument the Stream of a job without ARM64 (text, walk, x86 code, random,
 * x86 tail; both flags) is written there, for a decoder that knows only the older filters. */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../include/xz_amd.h"
#include "../../oracle/oracle.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

#define BS (128u << 10)
#define NB 5u
#define TAIL 40001u
#define N (4u * BS + TAIL)
#define HIST_WORDS (2u * 2u * 4096u)

extern int stub_delta_force_stored;
extern int stub_delta_calls[3];
extern int stub_bcj_calls[3];
void stub_arm64_encode(uint8_t *buf, uint32_t size);

static uint32_t rnd_state = 2463534242u;
static uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* with_arm64 = 0: Block 3 is random bytes */
static void make_input(uint8_t *in, int with_arm64)
{
	xzamd_corpus_lorem(in, BS);
	uint32_t v = 1u << 28;
	for (uint32_t i = 0; i < BS / 4; ++i) { v += rnd() % 2001u - 1000u; put32(in + BS + 4 * i, v); }
	/* x86: bytes below 200 (no E8 / E9), every 24 bytes a CALL to one of 64 function starts, the low ones more often */
	uint8_t *x = in + 2 * BS;
	for (uint32_t i = 0; i < BS; ++i) x[i] = (uint8_t)(rnd() % 200u);
	for (uint32_t p = 7; p + 5 <= BS; p += 24) {
		const uint32_t a = rnd() % 64u, b = rnd() % 64u, target = (a < b ? a : b) * 2048u;
		x[p] = 0xE8;
		put32(x + p + 1, target - (p + 5));
	}
	if (with_arm64) {
		/* ARM64: ORR-like words whose low bytes walk, every 8th word a BL to one of 64 function starts */
		uint32_t w = 0;
		for (uint32_t k = 0; k < BS / 4; ++k) {
			w = (w + 5u + rnd() % 3u) & 0xFFFFu;
			uint32_t instr = 0xAA000000u | w;
			if ((k & 7u) == 3u) {
				const uint32_t a = rnd() % 64u, b = rnd() % 64u, target = (a < b ? a : b) * 512u;
				instr = 0x94000000u | ((target - k) & 0x03FFFFFFu);
			}
			put32(in + 3 * BS + 4 * k, instr);
		}
	} else {
		for (uint32_t i = 0; i < BS; ++i) in[3 * BS + i] = (uint8_t)(rnd() >> 5);
	}
	for (uint32_t i = 0; i < TAIL; ++i) in[4 * BS + i] = in[2 * BS + i];
}

static uint32_t vli_get(const uint8_t *b, uint32_t *p, uint64_t *v)
{
	*v = 0;
	for (uint32_t s = 0; s < 63; s += 7) {
		const uint8_t c = b[(*p)++];
		*v |= (uint64_t)(c & 0x7F) << s;
		if (!(c & 0x80)) return 1;
	}
	return 0;
}

/* what the encoder-side filter `chain` (0: none, 4: x86, 0x0A: ARM64, 0x300 + d: delta d) makes of a Block */
static void forward(uint8_t *buf, uint32_t size, uint32_t chain)
{
	if (chain == XZAMD_BCJ_X86) orc_x86_encode(buf, size);
	else if (chain == XZAMD_BCJ_ARM64) stub_arm64_encode(buf, size);
	else if (chain >= 0x300u) {
		const uint32_t d = chain - 0x300u;
		for (uint32_t i = size; i-- > d; ) buf[i] = (uint8_t)(buf[i] - buf[i - d]);
	}
}

/* Block `bi` inside `buf`: header size, chain in the form of forward(); its payload decodes to forward(want); sizes; Check */
static int block_ok(const uint8_t *buf, const xzamd_block_info *bi, uint32_t dict_size, int check, const uint8_t *want, uint32_t usize_want,
		uint32_t *hs_out, uint32_t *chain_out, int *stored_out)
{
	const uint8_t *h = buf + bi->out_offset;
	const uint32_t hs = (h[0] + 1u) * 4u;
	uint32_t p = 2, chain = 0;
	uint64_t csize = 0, usize = 0, id = 0, ps = 0;
	if ((h[1] & 0xC0) != 0xC0 || !vli_get(h, &p, &csize) || !vli_get(h, &p, &usize)) return 0;
	const uint32_t nf = (h[1] & 3u) + 1u;
	if (nf > 2) return 0;                                  /* never a two-filter chain in front of LZMA2 */
	for (uint32_t i = 0; i < nf; ++i) {
		if (!vli_get(h, &p, &id) || !vli_get(h, &p, &ps)) return 0;
		if (i + 1 < nf) {
			if (id == 3 && ps == 1) chain = 0x300u + h[p] + 1u;
			else if ((id == XZAMD_BCJ_X86 || id == XZAMD_BCJ_ARM64) && ps == 0) chain = (uint32_t)id;
			else return 0;
		} else if (id != 0x21 || ps != 1) return 0;
		p += (uint32_t)ps;
	}
	if (p > hs - 4 || orc_crc32(h, hs - 4, 0) != (h[hs - 4] | (uint32_t)h[hs - 3] << 8 | (uint32_t)h[hs - 2] << 16 | (uint32_t)h[hs - 1] << 24)) return 0;
	for (uint32_t q = p; q < hs - 4; ++q) if (h[q]) return 0;      /* Header Padding */
	const uint32_t cb = orc_check_size(check);
	if (usize != usize_want || bi->uncompressed_size != usize || bi->unpadded_size != hs + csize + cb
			|| bi->total_size != ((bi->unpadded_size + 3) & ~3ull)) return 0;
	uint8_t *out = (uint8_t *)malloc(usize + 1), *exp = (uint8_t *)malloc(usize + 1);
	uint64_t got = 0;
	memcpy(exp, want, usize);
	forward(exp, (uint32_t)usize, chain);
	int ok = orc_lzma2_decode(h + hs, csize, dict_size, out, usize, &got, NULL) == 0 && got == usize;
	ok = ok && memcmp(out, exp, usize) == 0;
	const uint8_t *ck = h + ((hs + csize + 3) & ~3ull);
	if (ok && check == XZAMD_CHECK_CRC64) {
		uint64_t v = 0;
		for (int i = 7; i >= 0; --i) v = v << 8 | ck[i];
		ok = v == orc_crc64(want, usize, 0);
	} else if (ok && check == XZAMD_CHECK_CRC32) {
		ok = (ck[0] | (uint32_t)ck[1] << 8 | (uint32_t)ck[2] << 16 | (uint32_t)ck[3] << 24) == orc_crc32(want, usize, 0);
	}
	free(out); free(exp);
	*hs_out = hs; *chain_out = chain;
	*stored_out = csize == usize + ((usize + 65535) / 65536) * 3 + 1 && h[hs] == 0x01;
	return ok;
}

/* every Block of a Stream / of bare Blocks against the chains in `want` */
static void blocks_ok(const char *what, const uint8_t *buf, const xzamd_block_info *bi, const xzamd_lzma_options *opt, int check,
		const uint8_t *in, const uint32_t *want, int forced, uint32_t hs_of[3])
{
	for (uint32_t b = 0; b < NB; ++b) {
		uint32_t hs = 0, chain = 99;
		int stored = 0;
		const int ok = block_ok(buf, &bi[b], opt->dict_size, check, in + (uint64_t)b * BS, b + 1 < NB ? BS : TAIL, &hs, &chain, &stored);
		CHECK(ok, "%s: Block %u does not parse or decode", what, b);
		if (!ok) continue;
		CHECK(stored || (int)b != forced, "%s: Block %u does not have the stored form", what, b);
		CHECK(chain == ((int)b == forced ? 0u : want[b]), "%s: Block %u: chain %#x in its header, %#x expected", what, b, chain, want[b]);
		if (hs_of && b < 4 && (int)b != forced) {
			uint32_t *slot = &hs_of[chain == 0 ? 0 : chain >= 0x300u ? 1 : 2];
			CHECK(*slot == 0 || *slot == hs, "%s: Block %u: header of %u bytes, %u for the same kind of chain before", what, b, hs, *slot);
			*slot = hs;
		}
	}
}

int main(int argc, char **argv)
{
	xzamd_ctx *ctx = NULL;
	CHECK(xzamd_ctx_create(&ctx, 0) == XZAMD_OK, "ctx");
	if (!ctx) return 1;
	uint8_t *in = (uint8_t *)malloc(N);
	const uint64_t cap = xzamd_stream_buffer_bound(N, BS);
	uint8_t *out = (uint8_t *)malloc(cap), *bare = (uint8_t *)malloc(cap);
	make_input(in, 1);
	static const uint32_t want_bcj[NB] = { 0, 0, XZAMD_BCJ_X86, XZAMD_BCJ_ARM64, XZAMD_BCJ_X86 };          /* XZAMD_F_AUTO_BCJ */
	static const uint32_t want_delta[NB] = { 0, 0x304, 0, 0x320, 0 };                                       /* XZAMD_F_AUTO_DELTA: the ARM64 Block repeats every 8 words */
	static const uint32_t want_both[NB] = { 0, 0x304, XZAMD_BCJ_X86, XZAMD_BCJ_ARM64, XZAMD_BCJ_X86 };      /* both: BCJ first */

	/* the analysis on its own, and what it leaves to fetch */
	{
		uint32_t kind[NB], fetched[NB];
		uint64_t nb = 0;
		int rc = xzamd_auto_bcj_device(ctx, in, N, BS, kind, NB, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == NB, "analysis: rc %d, %llu Blocks", rc, (unsigned long long)nb);
		CHECK(memcmp(kind, want_bcj, sizeof(kind)) == 0, "analysis: %u %u %u %u %u", kind[0], kind[1], kind[2], kind[3], kind[4]);
		CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_BCJ_KIND, fetched, sizeof(fetched)) == XZAMD_OK && memcmp(fetched, kind, sizeof(kind)) == 0,
				"fetch of the choices");
		const uint64_t words = (uint64_t)NB * (HIST_WORDS + 2);
		uint32_t *hist = (uint32_t *)malloc(words * 4);
		CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_BCJ_HIST, hist, words * 4) == XZAMD_OK, "fetch of the histograms");
		const uint32_t *ns = hist + (uint64_t)NB * HIST_WORDS;
		for (uint32_t b = 0; b < NB; ++b)
			for (uint32_t k = 0; k < 4; ++k) {
				uint64_t s = 0;
				for (uint32_t v = 0; v < 4096; ++v) s += hist[((uint64_t)b * 4 + k) * 4096 + v];
				CHECK(s == ns[2 * b + k / 2], "Block %u, histogram %u: %llu entries, %u sites", b, k, (unsigned long long)s, ns[2 * b + k / 2]);
			}
		CHECK(ns[0] == 0 && ns[1] == 0 && ns[2 * 2] >= BS / 24 - 1 && ns[2 * 3 + 1] == BS / 32, "sites: text %u %u, x86 %u, ARM64 %u", ns[0], ns[1],
				ns[4], ns[7]);
		free(hist);
		rc = xzamd_auto_bcj_device(ctx, in, N, BS, kind, NB - 1, &nb, NULL);
		CHECK(rc == XZAMD_BUF_ERROR && nb == NB, "analysis into a short table: rc %d", rc);
		CHECK(xzamd_auto_bcj_device(ctx, in, N, 0, kind, NB, &nb, NULL) == XZAMD_OPTIONS_ERROR, "analysis with block_size 0");
		nb = 77;
		CHECK(xzamd_auto_bcj_device(ctx, in, 0, BS, kind, NB, &nb, NULL) == XZAMD_OK && nb == 0, "analysis of nothing");
	}

	static const int presets[2] = { 1, 6 }, checks[3] = { XZAMD_CHECK_CRC64, XZAMD_CHECK_CRC32, XZAMD_CHECK_NONE };
	for (int pi = 0; pi < 2; ++pi)
		for (int ci = 0; ci < 3; ++ci)
			for (int forced = -1; forced <= (pi == 0 ? 2 : -1); forced += 3) {       /* forced = 2: the x86 Block goes out stored (single-phase stub) */
				xzamd_lzma_options opt;
				xzamd_block_info bi[NB], bb[NB];
				uint64_t size = 0, bsize = 0, nb = 0;
				xzamd_stats st;
				xzamd_lzma_preset(&opt, (uint32_t)presets[pi]);
				const int check = checks[ci];
				char what[64];
				snprintf(what, sizeof(what), "both flags (preset %d, check %d, forced %d)", presets[pi], check, forced);
				stub_delta_force_stored = forced;
				memset(stub_delta_calls, 0, sizeof(stub_delta_calls));
				memset(stub_bcj_calls, 0, sizeof(stub_bcj_calls));
				int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, check, XZAMD_F_AUTO_BCJ | XZAMD_F_AUTO_DELTA, out, cap, &size, bi, NB, &nb, NULL);
				CHECK(rc == XZAMD_OK && nb == NB, "%s: rc %d %s", what, rc, xzamd_last_error(ctx));
				if (rc != XZAMD_OK || nb != NB) continue;
				CHECK(stub_bcj_calls[0] == 1 && stub_bcj_calls[1] == 1 && stub_bcj_calls[2] == 1 && stub_delta_calls[2] == 1, "one launch of each per batch");
				xzamd_get_stats(ctx, &st);
				CHECK(st.blocks_stored == (forced >= 0 ? 1u : 0u), "stored Blocks: %llu", (unsigned long long)st.blocks_stored);
				uint32_t hs_of[3] = { 0, 0, 0 };          /* header size of a Block with no filter, a delta filter, a BCJ filter */
				blocks_ok(what, out, bi, &opt, check, in, want_both, forced, hs_of);
				/* {LZMA2}: 3 bytes of Filter Flags; delta adds 3, a BCJ filter 2: both round up to the next multiple of four */
				CHECK(hs_of[0] != 0 && hs_of[1] == hs_of[0] + 4 && (forced == 2 || hs_of[2] == hs_of[0] + 4), "header sizes in one job: %u, %u, %u", hs_of[0], hs_of[1], hs_of[2]);
				/* the framing: Stream Header, every Block Header and its padding, Index, Footer */
				{
					xzamd_xz_block xb[NB];
					xzamd_xz_stream xs[1];
					uint64_t ns = 0, nbl = 0, usz = 0;
					rc = xzamd_file_index_host(out, size, xs, 1, &ns, xb, NB, &nbl, &usz);
					CHECK(rc == XZAMD_OK && ns == 1 && nbl == NB && usz == N, "index of the Stream: rc %d", rc);
					for (uint32_t b = 0; rc == XZAMD_OK && b < NB; ++b) {
						const uint32_t ch = (int)b == forced ? 0 : want_both[b];
						CHECK(xb[b].filter_count == (ch ? 2u : 1u) && xb[b].filter_ids[0] == (ch == 0 ? 0x21u : ch >= 0x300u ? 3u : ch)
								&& xb[b].header_offset == bi[b].out_offset, "index row of Block %u", b);
					}
				}
				/* the same Blocks, bare */
				rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, check, XZAMD_F_AUTO_BCJ | XZAMD_F_AUTO_DELTA | XZAMD_F_BLOCKS_ONLY, bare, cap, &bsize, bb, NB, &nb, NULL);
				CHECK(rc == XZAMD_OK && nb == NB && bsize <= size - 12 && memcmp(bare, out + 12, bsize) == 0, "blocks only: rc %d", rc);
				for (uint32_t b = 0; rc == XZAMD_OK && b < NB; ++b)
					CHECK(bb[b].out_offset + 12 == bi[b].out_offset && bb[b].unpadded_size == bi[b].unpadded_size, "blocks only: row %u", b);
				stub_delta_force_stored = -1;
				if (forced >= 0 || ci != 0) continue;
				/* each flag alone: the ARM64 Block is the delta rule's when the BCJ rule is not asked */
				memset(stub_delta_calls, 0, sizeof(stub_delta_calls));
				rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, check, XZAMD_F_AUTO_BCJ, out, cap, &size, bi, NB, &nb, NULL);
				CHECK(rc == XZAMD_OK && nb == NB && stub_delta_calls[0] + stub_delta_calls[1] + stub_delta_calls[2] == 0, "auto bcj alone: rc %d", rc);
				if (rc == XZAMD_OK) blocks_ok("auto bcj alone", out, bi, &opt, check, in, want_bcj, -1, NULL);
				memset(stub_bcj_calls, 0, sizeof(stub_bcj_calls));
				rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, check, XZAMD_F_AUTO_DELTA, out, cap, &size, bi, NB, &nb, NULL);
				CHECK(rc == XZAMD_OK && nb == NB && stub_bcj_calls[0] + stub_bcj_calls[1] + stub_bcj_calls[2] == 0, "auto delta alone: rc %d", rc);
				if (rc == XZAMD_OK) blocks_ok("auto delta alone", out, bi, &opt, check, in, want_delta, -1, NULL);
				/* without the flags: every Block {LZMA2}, the kernels not called */
				memset(stub_delta_calls, 0, sizeof(stub_delta_calls));
				rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, check, 0, out, cap, &size, bi, NB, &nb, NULL);
				CHECK(rc == XZAMD_OK && stub_bcj_calls[0] + stub_bcj_calls[1] + stub_bcj_calls[2] + stub_delta_calls[0] == 0, "plain encode: rc %d", rc);
				static const uint32_t none[NB] = { 0, 0, 0, 0, 0 };
				if (rc == XZAMD_OK) blocks_ok("plain encode", out, bi, &opt, check, in, none, -1, NULL);
			}
	stub_delta_force_stored = -1;

	/* several batches in one call: the choices of every batch reach its own layout */
	{
		xzamd_lzma_options opt;
		xzamd_block_info bi[NB];
		uint64_t size = 0, nb = 0;
		xzamd_lzma_preset(&opt, 6);
		CHECK(xzamd_ctx_set_batch_bytes(ctx, 2 * BS) == XZAMD_OK, "batch bytes");
		memset(stub_bcj_calls, 0, sizeof(stub_bcj_calls));
		int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_BCJ | XZAMD_F_AUTO_DELTA, out, cap, &size, bi, NB, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == NB && stub_bcj_calls[0] == 3 && stub_bcj_calls[2] == 3, "three batches: rc %d, %d launches", rc, stub_bcj_calls[0]);
		if (rc == XZAMD_OK) blocks_ok("three batches", out, bi, &opt, XZAMD_CHECK_CRC64, in, want_both, -1, NULL);
		CHECK(xzamd_ctx_set_batch_bytes(ctx, 1ull << 30) == XZAMD_OK, "batch bytes");
	}

	/* what the flag declines: XZAMD_OPTIONS_ERROR and a text */
	{
		xzamd_lzma_options opt;
		xzamd_block_info bi[NB];
		uint64_t size = 0, nb = 0;
		xzamd_lzma_preset(&opt, 6);
		static const uint32_t bad[3] = { XZAMD_F_SEGMENTS, XZAMD_F_SINGLE, XZAMD_F_REPAIR };
		for (int i = 0; i < 3; ++i) {
			const int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_BCJ | bad[i], out, cap, &size, bi, NB, &nb, NULL);
			CHECK(rc == XZAMD_OPTIONS_ERROR && strstr(xzamd_last_error(ctx), "auto bcj") != NULL, "flag %u: rc %d '%s'", bad[i], rc, xzamd_last_error(ctx));
		}
		opt.bcj = XZAMD_FILTER_DELTA(4);
		int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_BCJ, out, cap, &size, bi, NB, &nb, NULL);
		CHECK(rc == XZAMD_OPTIONS_ERROR && strstr(xzamd_last_error(ctx), "auto bcj") != NULL, "a chain with a filter: rc %d '%s'", rc, xzamd_last_error(ctx));
		opt.bcj = XZAMD_BCJ_X86;
		rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_BCJ, out, cap, &size, bi, NB, &nb, NULL);
		CHECK(rc == XZAMD_OPTIONS_ERROR && strstr(xzamd_last_error(ctx), "auto bcj") != NULL, "a chain with x86 BCJ: rc %d", rc);
	}

	/* a job without ARM64, written out for a decoder of the caller's */
	if (argc > 1) {
		xzamd_lzma_options opt;
		xzamd_block_info bi[NB];
		uint64_t size = 0, nb = 0;
		static const uint32_t want_file[NB] = { 0, 0x304, XZAMD_BCJ_X86, 0, XZAMD_BCJ_X86 };
		char path[4096];
		xzamd_lzma_preset(&opt, 6);
		make_input(in, 0);
		int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_BCJ | XZAMD_F_AUTO_DELTA, out, cap, &size, bi, NB, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == NB, "job for the file: rc %d", rc);
		if (rc == XZAMD_OK) blocks_ok("job for the file", out, bi, &opt, XZAMD_CHECK_CRC64, in, want_file, -1, NULL);
		snprintf(path, sizeof(path), "%s.xz", argv[1]);
		FILE *f = fopen(path, "wb");
		CHECK(f && fwrite(out, 1, size, f) == size && fclose(f) == 0, "writing %s", path);
		f = fopen(argv[1], "wb");
		CHECK(f && fwrite(in, 1, N, f) == N && fclose(f) == 0, "writing %s", argv[1]);
	}

	xzamd_ctx_destroy(ctx);
	free(in); free(out); free(bare);
	if (failures) { printf("driver_auto_bcj: %d failure(s)\n", failures); return 1; }
	printf("driver_auto_bcj: ok\n");
	return 0;
}
