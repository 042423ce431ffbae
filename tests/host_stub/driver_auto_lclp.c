/* driver_auto_lclp.c -- TEST INFRASTRUCTURE ONLY: the host side of the automatic per-Block literal context (XZAMD_F_AUTO_LCLP:
 * xz_amd/csrc/xzamd_host.c, xzamd_options.c) over the CPU stand-ins of the kernel layer (stub_xzk.c, stub_xzk_lclp.c), as a
 * stand-alone program under ASan / UBSan (tests/test_host_auto_lclp.py).
 *
 * Five Blocks of 128 KiB -- text, a float32 walk, RGBA pixels, random bytes, and a short tail of the float32 walk.  Checked: the
 * analysis on its own and its errors, the two debug fetches, that every launch of the parse and of the coder (both encode modes
 * of the host layer: single-phase, preset 1; two-phase, preset 6) carries the props table of ITS batch -- with one batch and
 * with three, where the two pipeline parities alternate -- that the table is NULL without the flag and the kernels are not
 * called, that the Stream decodes, and the combinations the flag declines. */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../include/xz_amd.h"
#include "../../oracle/oracle.h"
#include "../../xz_amd/csrc/lclp_rule.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

#define BS (128u << 10)
#define NB 5u
#define TAIL 40001u
#define N (4u * BS + TAIL)

#ifndef DRIVER_NO_LCLP_KERNELS
extern int stub_lclp_calls[3], stub_lclp_seen, stub_lclp_bad;
void stub_lclp_reset(int expect);
#endif

static uint32_t rnd_state = 4321;
static uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static void make_input(uint8_t *in)
{
	xzamd_corpus_lorem(in, BS);
	float v = 100.0f;
	for (uint32_t i = 0; i < BS / 4; ++i) {
		v += (float)(rnd() % 2001u) / 1000.0f - 1.0f;
		memcpy(in + BS + 4 * i, &v, 4);
	}
	for (uint32_t i = 0; i < BS / 4; ++i) {
		uint8_t *p = in + 2 * BS + 4 * i;
		p[0] = (uint8_t)((i % 1024u) / 8u * 8u + rnd() % 3u); p[1] = (uint8_t)((i / 1024u) * 8u + rnd() % 3u);
		p[2] = (uint8_t)((((i % 1024u) / 32u) ^ (i / 32768u)) * 16u + rnd() % 3u); p[3] = 255;
	}
	for (uint32_t i = 0; i < BS; ++i) in[3 * BS + i] = (uint8_t)(rnd() >> 5);
	for (uint32_t i = 0; i < TAIL; ++i) in[4 * BS + i] = in[BS + i];
}

#ifndef DRIVER_NO_LCLP_KERNELS
/* what the rule says for a Block, by the plainest route: its histogram, then xzamd_ll_choose */
static uint32_t want_props(const uint8_t *x, uint32_t blen, uint32_t lc, uint32_t lp, uint32_t *h)
{
	static const uint8_t T[256] = XZAMD_AD_LOG_TABLE;
	memset(h, 0, XZAMD_LL_HIST_WORDS * 4);
	for (uint32_t i = 0; i < blen; ++i)
		if (i % XZAMD_AD_PERIOD < XZAMD_AD_WINDOW) ++h[(((i & 7u) * 8u + ((i ? x[i - 1] : 0u) >> 5)) << 8) + x[i]];
	return xzamd_ll_choose(h, lc, lp, T);
}
#endif

#ifdef DRIVER_NO_LCLP_KERNELS
/* Built without stub_xzk_lclp.c: a kernel layer that lacks the entry points.  The flag and the analysis are declined. */
int main(void)
{
	xzamd_ctx *ctx = NULL;
	CHECK(xzamd_ctx_create(&ctx, 0) == XZAMD_OK, "ctx");
	if (!ctx) return 1;
	uint8_t *in = (uint8_t *)malloc(N);
	const uint64_t cap = xzamd_stream_buffer_bound(N, BS);
	uint8_t *out = (uint8_t *)malloc(cap);
	xzamd_lzma_options opt;
	xzamd_block_info bi[NB];
	uint64_t size = 0, nb = 0;
	uint32_t props[NB];
	make_input(in);
	xzamd_lzma_preset(&opt, 6);
	int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_LCLP, out, cap, &size, bi, NB, &nb, NULL);
	CHECK(rc == XZAMD_OPTIONS_ERROR && strstr(xzamd_last_error(ctx), "no kernels") != NULL, "encode: rc %d '%s'", rc, xzamd_last_error(ctx));
	rc = xzamd_auto_lclp_device(ctx, in, N, BS, 3, 0, props, NB, &nb, NULL);
	CHECK(rc == XZAMD_OPTIONS_ERROR && strstr(xzamd_last_error(ctx), "no kernels") != NULL, "analysis: rc %d '%s'", rc, xzamd_last_error(ctx));
	CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_LCLP_PROPS, props, 4) == XZAMD_PROG_ERROR, "fetch");
	rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, 0, out, cap, &size, bi, NB, &nb, NULL);
	CHECK(rc == XZAMD_OK && nb == NB, "plain encode: rc %d", rc);
	xzamd_ctx_destroy(ctx);
	free(in); free(out);
	if (failures) { printf("driver_auto_lclp: %d failure(s)\n", failures); return 1; }
	printf("driver_auto_lclp: ok (no kernels)\n");
	return 0;
}
#else
int main(void)
{
	xzamd_ctx *ctx = NULL;
	CHECK(xzamd_ctx_create(&ctx, 0) == XZAMD_OK, "ctx");
	if (!ctx) return 1;
	uint8_t *in = (uint8_t *)malloc(N), *back = (uint8_t *)malloc(N);
	const uint64_t cap = xzamd_stream_buffer_bound(N, BS);
	uint8_t *out = (uint8_t *)malloc(cap), *plain = (uint8_t *)malloc(cap);
	uint32_t *h = (uint32_t *)malloc(XZAMD_LL_HIST_WORDS * 4), *hist = (uint32_t *)malloc((size_t)NB * XZAMD_LL_HIST_WORDS * 4);
	uint32_t want[NB];
	make_input(in);
	for (uint32_t b = 0; b < NB; ++b) want[b] = want_props(in + (size_t)b * BS, b + 1 < NB ? BS : TAIL, 3, 0, h);
	/* (8,192 random samples cannot fill 2,048 cells: the cell charge sends them to fewer contexts, whatever that is worth) */
	CHECK(want[0] == XZAMD_LL_PROPS(3, 0) && (want[3] & 255u) + (want[3] >> 8) <= 3, "text keeps the job's pair: %x %x", want[0], want[3]);
	CHECK((want[1] >> 8) >= 2 && (want[2] >> 8) >= 2 && want[4] == want[1], "aligned data gets lp >= 2: %x %x %x", want[1], want[2], want[4]);

	/* the analysis on its own, and what it leaves to fetch */
	{
		uint32_t props[NB], fetched[NB];
		uint64_t nb = 0;
		stub_lclp_reset(1);
		int rc = xzamd_auto_lclp_device(ctx, in, N, BS, 3, 0, props, NB, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == NB, "analysis: rc %d, %llu Blocks", rc, (unsigned long long)nb);
		CHECK(memcmp(props, want, sizeof(props)) == 0, "analysis: %x %x %x %x %x", props[0], props[1], props[2], props[3], props[4]);
		CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_LCLP_PROPS, fetched, sizeof(fetched)) == XZAMD_OK && memcmp(fetched, props, sizeof(props)) == 0,
				"fetch of the choices");
		CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_LCLP_HIST, hist, (uint64_t)NB * XZAMD_LL_HIST_WORDS * 4) == XZAMD_OK, "fetch of the histograms");
		CHECK(stub_lclp_calls[2] == 2, "the fetches go through the read-back entry: %d", stub_lclp_calls[2]);
		for (uint32_t b = 0; b < NB; ++b) {
			uint64_t s = 0;
			for (uint32_t i = 0; i < XZAMD_LL_HIST_WORDS; ++i) s += hist[(size_t)b * XZAMD_LL_HIST_WORDS + i];
			CHECK(s == (b < 4 ? 2 * 4096u : 4096u), "samples of Block %u: %llu", b, (unsigned long long)s);
			(void)want_props(in + (size_t)b * BS, b + 1 < NB ? BS : TAIL, 3, 0, h);
			CHECK(memcmp(h, hist + (size_t)b * XZAMD_LL_HIST_WORDS, XZAMD_LL_HIST_WORDS * 4) == 0, "histogram of Block %u", b);
		}
		CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_LCLP_HIST, hist, 1000) == XZAMD_PROG_ERROR, "fetch of a part of a histogram");
		/* a job with another pair: its own candidates; a pair the statistic cannot price stays */
		rc = xzamd_auto_lclp_device(ctx, in, N, BS, 2, 2, props, NB, &nb, NULL);
		CHECK(rc == XZAMD_OK, "analysis (2, 2): rc %d", rc);
		for (uint32_t b = 0; b < NB; ++b)
			CHECK(props[b] == want_props(in + (size_t)b * BS, b + 1 < NB ? BS : TAIL, 2, 2, h), "analysis (2, 2): Block %u: %x", b, props[b]);
		rc = xzamd_auto_lclp_device(ctx, in, N, BS, 4, 0, props, NB, &nb, NULL);
		CHECK(rc == XZAMD_OK && props[1] == XZAMD_LL_PROPS(4, 0) && props[2] == XZAMD_LL_PROPS(4, 0), "analysis (4, 0): rc %d", rc);
		rc = xzamd_auto_lclp_device(ctx, in, N, BS, 3, 0, props, NB - 1, &nb, NULL);
		CHECK(rc == XZAMD_BUF_ERROR && nb == NB, "analysis into a short table: rc %d", rc);
		CHECK(xzamd_auto_lclp_device(ctx, in, N, 0, 3, 0, props, NB, &nb, NULL) == XZAMD_OPTIONS_ERROR, "analysis with block_size 0");
		CHECK(xzamd_auto_lclp_device(ctx, in, N, BS, 3, 2, props, NB, &nb, NULL) == XZAMD_OPTIONS_ERROR, "analysis with lc + lp = 5");
		nb = 77;
		CHECK(xzamd_auto_lclp_device(ctx, in, 0, BS, 3, 0, props, NB, &nb, NULL) == XZAMD_OK && nb == 0, "analysis of nothing");
	}

	static const int presets[2] = { 1, 6 };
	static const uint64_t batches[2] = { 1ull << 30, 2 * BS };       /* one batch; three: parities 0, 1, 0 */
	for (int pi = 0; pi < 2; ++pi)
		for (int bi_ = 0; bi_ < 2; ++bi_) {
			xzamd_lzma_options opt;
			xzamd_block_info bi[NB];
			uint64_t size = 0, psize = 0, nb = 0, got = 0, nbl = 0;
			uint32_t fetched[NB];
			xzamd_lzma_preset(&opt, (uint32_t)presets[pi]);
			CHECK(xzamd_ctx_set_batch_bytes(ctx, batches[bi_]) == XZAMD_OK, "batch bytes");
			const int nbatch = bi_ ? 3 : 1;
			stub_lclp_reset(1);
			int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_LCLP, out, cap, &size, bi, NB, &nb, NULL);
			CHECK(rc == XZAMD_OK && nb == NB, "encode (preset %d, %d batches): rc %d %s", presets[pi], nbatch, rc, xzamd_last_error(ctx));
			if (rc != XZAMD_OK) continue;
			CHECK(stub_lclp_calls[0] == nbatch && stub_lclp_calls[1] == nbatch, "one statistic and one choice per batch: %d %d",
					stub_lclp_calls[0], stub_lclp_calls[1]);
			CHECK(stub_lclp_seen >= nbatch && stub_lclp_bad == 0, "preset %d, %d batches: %d launches seen, %d without the props table of their batch",
					presets[pi], nbatch, stub_lclp_seen, stub_lclp_bad);
			/* the last batch's choices stay fetchable */
			const uint32_t last_nb = bi_ ? 1u : NB, last_b0 = bi_ ? 4u : 0u;
			CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_LCLP_PROPS, fetched, 4ull * last_nb) == XZAMD_OK
					&& memcmp(fetched, want + last_b0, 4ull * last_nb) == 0, "choices of the last batch");
			CHECK(orc_xz_decode(out, size, back, N, &got, &nbl) == 0 && got == N && nbl == NB && memcmp(back, in, N) == 0, "the Stream decodes");
			/* without the flag: no table, no kernel -- and (stub coder: stored chunks) the same bytes */
			stub_lclp_reset(0);
			rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, 0, plain, cap, &psize, bi, NB, &nb, NULL);
			CHECK(rc == XZAMD_OK && stub_lclp_calls[0] + stub_lclp_calls[1] == 0 && stub_lclp_seen >= nbatch && stub_lclp_bad == 0,
					"plain encode: rc %d, %d calls, %d launches with a table", rc, stub_lclp_calls[0] + stub_lclp_calls[1], stub_lclp_bad);
			CHECK(psize == size && memcmp(plain, out, size) == 0, "plain encode: the stub coder's bytes do not depend on the flag");
			/* the flag with XZAMD_F_BLOCKS_ONLY and with XZAMD_F_KEEP_RESUME */
			stub_lclp_reset(1);
			rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC32, XZAMD_F_AUTO_LCLP | XZAMD_F_BLOCKS_ONLY, plain, cap, &psize, bi, NB, &nb, NULL);
			CHECK(rc == XZAMD_OK && nb == NB && stub_lclp_bad == 0 && stub_lclp_calls[0] == nbatch, "blocks only: rc %d", rc);
		}
	CHECK(xzamd_ctx_set_batch_bytes(ctx, 1ull << 30) == XZAMD_OK, "batch bytes");

	/* what the flag declines: XZAMD_OPTIONS_ERROR and a text */
	{
		xzamd_lzma_options opt;
		xzamd_block_info bi[NB];
		uint64_t size = 0, nb = 0;
		xzamd_lzma_preset(&opt, 6);
		static const uint32_t bad[3] = { XZAMD_F_SEGMENTS, XZAMD_F_SINGLE, XZAMD_F_REPAIR };
		for (int i = 0; i < 3; ++i) {
			const int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_LCLP | bad[i], out, cap, &size, bi, NB, &nb, NULL);
			CHECK(rc == XZAMD_OPTIONS_ERROR && strstr(xzamd_last_error(ctx), "auto lclp") != NULL, "flag %u: rc %d '%s'", bad[i], rc, xzamd_last_error(ctx));
		}
	}

	xzamd_ctx_destroy(ctx);
	free(in); free(back); free(out); free(plain); free(h); free(hist);
	if (failures) { printf("driver_auto_lclp: %d failure(s)\n", failures); return 1; }
	printf("driver_auto_lclp: ok\n");
	return 0;
}
#endif
