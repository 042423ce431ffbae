/* driver_build_ahead.c -- TEST INFRASTRUCTURE ONLY: the batch loop of xz_amd/csrc/xzamd_host.c with the structure build of
 * batch i + 1 issued ahead (XZAMD_BUILD_AHEAD), over the CPU stand-ins of the kernel layer, as a stand-alone
 * program under ASan / UBSan (tests/test_host_build_ahead.py).  stub_xzk_log.c prints every kernel-layer call with its stream;
 * this program prints, around them,
 *     case <name> <knob>
 *     end <rc> <bytes> <batches> <equal to the same job with the knob at 0: 1 | 0> <decodes: 1 | 0 | -1 not tried> <batches issued ahead>
 * and the test turns the lines in between into a happens-before graph.  The jobs: Blocks of 128 KiB, two to a batch, four
 * batches with a ragged last one; XZAMD_F_AUTO_DELTA so that every batch also has a filtered copy and choices per parity. */
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
#define N (7u * BS + 40001u)

extern int stub_log_on;

static uint8_t *in, *out, *base, *dec;
static uint64_t cap;

static void make_input(void)
{
	/* text and an int32 walk, Block by Block: Blocks with and without a delta filter */
	uint32_t s = 12345, v = 1u << 28;
	xzamd_corpus_lorem(in, N);
	for (uint32_t b = 1; b * BS < N; b += 2)
		for (uint32_t i = b * BS; i + 4 <= N && i < (b + 1) * BS; i += 4) {
			s = s * 1664525u + 1013904223u;
			v += (s >> 8) % 2001u - 1000u;
			in[i] = (uint8_t)v; in[i + 1] = (uint8_t)(v >> 8); in[i + 2] = (uint8_t)(v >> 16); in[i + 3] = (uint8_t)(v >> 24);
		}
}

/* One logged encode.  `base_size` != 0: the bytes must equal `base`. */
static uint64_t run(xzamd_ctx *ctx, const char *name, const char *knob, int preset, uint32_t flags, uint64_t n, int logged, uint64_t base_size,
		int decode)
{
	xzamd_lzma_options opt;
	xzamd_stats st;
	uint64_t size = 0, nb = 0;
	CHECK(xzamd_lzma_preset(&opt, (uint32_t)preset) == 0, "preset");
	if (knob) setenv("XZAMD_BUILD_AHEAD", knob, 1); else unsetenv("XZAMD_BUILD_AHEAD");
	if (logged) printf("case %s %s\n", name, knob ? knob : "default");
	stub_log_on = logged;
	const int rc = xzamd_stream_encode_device(ctx, in, n, BS, &opt, XZAMD_CHECK_CRC64, flags, out, cap, &size, NULL, 0, &nb, NULL);
	stub_log_on = 0;
	xzamd_get_stats(ctx, &st);
	int dec_ok = -1;
	if (decode && rc == XZAMD_OK) {
		uint64_t got = 0, blocks = 0;
		dec_ok = orc_xz_decode(out, size, dec, n, &got, &blocks) == 0 && got == n && memcmp(dec, in, n) == 0;
	}
	if (logged)
		printf("end %d %llu %llu %d %d %u\n", rc, (unsigned long long)size, (unsigned long long)st.batches,
				base_size ? (size == base_size && memcmp(out, base, size) == 0) : 1, dec_ok, st.batches_ahead);
	CHECK(rc == XZAMD_OK, "%s %s: rc %d (%s)", name, knob ? knob : "default", rc, xzamd_last_error(ctx));
	return rc == XZAMD_OK ? size : 0;
}

int main(void)
{
	static const char *const knobs[] = { "plan", "part", "iter1", NULL };
	in = (uint8_t *)malloc(N);
	cap = xzamd_stream_buffer_bound(N, BS) + 64;
	out = (uint8_t *)malloc(cap); base = (uint8_t *)malloc(cap); dec = (uint8_t *)malloc(N + 1);
	make_input();
	unsetenv("XZAMD_TEST_ALLOC_LIMIT_MIB");
	unsetenv("XZAMD_NO_OVERLAP");
	unsetenv("XZAMD_BACK_BESIDE_BUILD");
	unsetenv("XZAMD_BUILD_AHEAD_STREAM");

	xzamd_ctx *ctx = NULL;
	CHECK(xzamd_ctx_create(&ctx, 0) == XZAMD_OK && xzamd_ctx_set_batch_bytes(ctx, 2 * BS) == XZAMD_OK, "ctx");
	if (!ctx) return 1;
	/* a context that has never run: the second batch grows the tables of its parity and so runs serially, the later ones ahead */
	(void)run(ctx, "cold", "part", 6, XZAMD_F_AUTO_DELTA, N, 1, 0, 0);
	/* every buffer is there now: the reference bytes, then every start point; 4 x a 1-byte batch less is a job of another size */
	uint64_t bsz = run(ctx, "warm", "0", 6, XZAMD_F_AUTO_DELTA, N, 1, 0, 0);
	memcpy(base, out, bsz);
	for (int k = 0; knobs[k]; ++k)
		(void)run(ctx, "warm", knobs[k], 6, XZAMD_F_AUTO_DELTA, N, 1, bsz, 0);
	(void)run(ctx, "warm", NULL, 6, XZAMD_F_AUTO_DELTA, N, 1, bsz, 0);
	/* the chain {LZMA2}: decodes through the oracle; a second, shorter job on the same context (no state of the first survives) */
	bsz = run(ctx, "plain", "0", 6, 0, N, 1, 0, 1);
	memcpy(base, out, bsz);
	for (int k = 0; knobs[k]; ++k)
		(void)run(ctx, "plain", knobs[k], 6, 0, N, 1, bsz, 1);
	bsz = run(ctx, "short", "0", 6, 0, 4 * BS + 1, 1, 0, 1);
	memcpy(base, out, bsz);
	(void)run(ctx, "short", "part", 6, 0, 4 * BS + 1, 1, bsz, 1);
	/* a single-phase preset: the span kernel reads the structure while it codes, nothing is issued ahead */
	bsz = run(ctx, "single_phase", "0", 1, 0, N, 1, 0, 1);
	memcpy(base, out, bsz);
	(void)run(ctx, "single_phase", "part", 1, 0, N, 1, bsz, 1);
	xzamd_ctx_destroy(ctx);

	/* the forced allocation limit: a context whose first batch (four Blocks) does not fit, so the job goes on in halves of two
	 * Blocks; the two batches that had to allocate run serially, the two behind them ahead, and the Stream is the one of the
	 * serial schedule */
	{
		const char *lim = getenv("DRIVER_ALLOC_LIMIT_MIB");
		uint64_t size0 = 0;
		for (int pass = 0; pass < 2; ++pass) {
			setenv("XZAMD_TEST_ALLOC_LIMIT_MIB", lim ? lim : "10", 1);
			ctx = NULL;
			CHECK(xzamd_ctx_create(&ctx, 0) == XZAMD_OK && xzamd_ctx_set_batch_bytes(ctx, 4 * BS) == XZAMD_OK, "ctx with a limit");
			unsetenv("XZAMD_TEST_ALLOC_LIMIT_MIB");
			if (!ctx) return 1;
			size0 = run(ctx, "alloc_limit", pass ? "part" : "0", 6, XZAMD_F_AUTO_DELTA, N, 1, pass ? size0 : 0, 0);
			if (!pass) memcpy(base, out, size0);
			xzamd_ctx_destroy(ctx);
		}
	}
	free(in); free(out); free(base); free(dec);
	if (failures) { printf("driver_build_ahead: %d failure(s)\n", failures); return 1; }
	printf("driver_build_ahead: ok\n");
	return 0;
}
