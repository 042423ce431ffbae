/* driver_single.c -- TEST INFRASTRUCTURE ONLY: drives the single-Block encoder (lzma_easy_encoder / lzma_stream_encoder of
 * xzamd_stream.c, over xzamd_host.c, xzamd_frame.c, xzamd_options.c and the CPU stand-in stub_xzk.c) the way a liblzma
 * client does.  A program of its own, so that it can be built with sanitizers and simply run.
 * usage: driver_single OUTDIR
 *   OUTDIR/input.bin                     the 300,000 input bytes
 *   OUTDIR/{plain,sync,full}_{1,4097,all}.xz   no flush / LZMA_SYNC_FLUSH behind byte 100,000 / LZMA_FULL_FLUSH behind
 *                                        byte 200,000, fed 1 byte, 4097 bytes at a time, and all at once
 *   OUTDIR/sync_{...}.cut                decimal: bytes handed out when the sync flush returned LZMA_STREAM_END
 * Exit code 0 and "driver_single: ok" when every call behaved. */
#include "../../include/xz_amd.h"
#include "../../include/xz_amd_lzma.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver_single: %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
#define N 300000u

static void save(const char *dir, const char *name, const void *p, size_t n)
{
	char path[512];
	snprintf(path, sizeof(path), "%s/%s", dir, name);
	FILE *f = fopen(path, "wb");
	CHECK(f != NULL);
	CHECK(fwrite(p, 1, n, f) == n);
	fclose(f);
}

/* feed `in` in pieces of in_step into small output pieces; flush_at != 0: `flush_action` once that many bytes are in */
static size_t encode(const uint8_t *in, size_t n, size_t in_step, size_t flush_at, lzma_action flush_action,
		uint8_t *out, size_t out_cap, size_t *out_at_flush)
{
	lzma_stream s = LZMA_STREAM_INIT;
	CHECK(lzma_easy_encoder(&s, 6, LZMA_CHECK_CRC64) == LZMA_OK);
	size_t ipos = 0, opos = 0;
	int flushed = flush_at == 0;
	for (;;) {
		lzma_action act = LZMA_RUN;
		const size_t limit = flushed ? n : flush_at;
		if (s.avail_in == 0 && ipos < limit) {
			const size_t k = limit - ipos < in_step ? limit - ipos : in_step;
			s.next_in = in + ipos;
			s.avail_in = k;
			ipos += k;
		}
		if (ipos == limit && !flushed) act = flush_action;
		else if (ipos == n) act = LZMA_FINISH;
		if (s.avail_out == 0) {
			CHECK(opos < out_cap);
			const size_t k = out_cap - opos < 3000 ? out_cap - opos : 3000;
			s.next_out = out + opos;
			s.avail_out = k;
			opos += k;
		}
		const lzma_ret r = lzma_code(&s, act);
		uint64_t pin = 0, pout = 0;
		lzma_get_progress(&s, &pin, &pout);
		CHECK(pin <= n && pout == s.total_out);
		if (r == LZMA_STREAM_END) {
			if (act == LZMA_FINISH) break;
			CHECK(act == flush_action && s.avail_in == 0 && s.total_in == flush_at);
			if (out_at_flush) *out_at_flush = (size_t)s.total_out;
			flushed = 1;
			continue;
		}
		CHECK(r == LZMA_OK);
	}
	opos -= s.avail_out;
	CHECK(s.total_in == n && s.total_out == opos);
	CHECK(lzma_code(&s, LZMA_FINISH) == LZMA_STREAM_END);
	lzma_end(&s);
	return opos;
}

int main(int argc, char **argv)
{
	CHECK(argc == 2);
	const char *dir = argv[1];
	uint8_t *in = (uint8_t *)malloc(N);
	const size_t cap = N + N / 4 + 65536;
	uint8_t *out = (uint8_t *)malloc(cap);
	CHECK(in && out);
	xzamd_corpus_lorem(in, N);
	save(dir, "input.bin", in, N);
	setenv("XZAMD_SEGMENT_KIB", "64", 1);

	static const struct { const char *name; size_t step; } feeds[3] = { { "1", 1 }, { "4097", 4097 }, { "all", N } };
	for (int f = 0; f < 3; ++f) {
		char name[64], num[32];
		size_t cut = 0;
		size_t w = encode(in, N, feeds[f].step, 0, LZMA_RUN, out, cap, NULL);
		snprintf(name, sizeof(name), "plain_%s.xz", feeds[f].name);
		save(dir, name, out, w);
		w = encode(in, N, feeds[f].step, 100000, LZMA_SYNC_FLUSH, out, cap, &cut);
		snprintf(name, sizeof(name), "sync_%s.xz", feeds[f].name);
		save(dir, name, out, w);
		CHECK(cut > 0 && cut < w);
		snprintf(name, sizeof(name), "sync_%s.cut", feeds[f].name);
		snprintf(num, sizeof(num), "%zu", cut);
		save(dir, name, num, strlen(num));
		w = encode(in, N, feeds[f].step, 200000, LZMA_FULL_FLUSH, out, cap, NULL);
		snprintf(name, sizeof(name), "full_%s.xz", feeds[f].name);
		save(dir, name, out, w);
	}

	/* two workers on the one stub device: same bytes */
	{
		uint8_t *out2 = (uint8_t *)malloc(cap);
		CHECK(out2 != NULL);
		setenv("XZAMD_TEST_WORKERS", "2", 1);
		setenv("XZAMD_BATCH_MIB", "1", 1);
		const size_t w1 = encode(in, N, 4097, 0, LZMA_RUN, out, cap, NULL);
		unsetenv("XZAMD_TEST_WORKERS");
		unsetenv("XZAMD_BATCH_MIB");
		const size_t w2 = encode(in, N, N, 0, LZMA_RUN, out2, cap, NULL);
		CHECK(w1 == w2 && memcmp(out, out2, w1) == 0);
		free(out2);
	}

	/* empty input: a Stream without Blocks; LZMA_FULL_BARRIER ends a Block like a flush */
	{
		const size_t w = encode(in, 0, 1, 0, LZMA_RUN, out, cap, NULL);
		CHECK(w == 32);
		save(dir, "empty.xz", out, w);
		const size_t wb = encode(in, N, N, 200000, LZMA_FULL_BARRIER, out, cap, NULL);
		save(dir, "barrier.xz", out, wb);
	}

	/* option checks at init (stream_encoder.c:286-337, easy_encoder.c) */
	{
		lzma_stream s = LZMA_STREAM_INIT;
		lzma_options_lzma l;
		memset(&l, 0, sizeof(l));
		l.dict_size = 1u << 20; l.lc = 3; l.lp = 0; l.pb = 2; l.mode = LZMA_MODE_NORMAL; l.nice_len = 64; l.mf = LZMA_MF_BT4;
		lzma_filter plain[2] = { { LZMA_FILTER_LZMA2, &l }, { LZMA_VLI_UNKNOWN, NULL } };
		lzma_filter x86[3] = { { LZMA_FILTER_X86, NULL }, { LZMA_FILTER_LZMA2, &l }, { LZMA_VLI_UNKNOWN, NULL } };
		CHECK(lzma_stream_encoder(&s, NULL, LZMA_CHECK_CRC64) == LZMA_PROG_ERROR);
		CHECK(lzma_stream_encoder(&s, x86, LZMA_CHECK_CRC64) == LZMA_OPTIONS_ERROR);
		CHECK(s.internal == NULL);
		CHECK(lzma_stream_encoder(&s, plain, LZMA_CHECK_SHA256) == LZMA_OPTIONS_ERROR);
		CHECK(lzma_easy_encoder(&s, 6, LZMA_CHECK_SHA256) == LZMA_OPTIONS_ERROR);
		CHECK(lzma_easy_encoder(&s, 77, LZMA_CHECK_CRC64) == LZMA_OPTIONS_ERROR);
		CHECK(lzma_easy_encoder(&s, 6, (lzma_check)99) == LZMA_PROG_ERROR);
		CHECK(lzma_easy_encoder(&s, 6, (lzma_check)2) == LZMA_UNSUPPORTED_CHECK);
		CHECK(lzma_stream_encoder(&s, plain, LZMA_CHECK_CRC32) == LZMA_OK);
		/* a new chain between Blocks; none inside one */
		CHECK(lzma_filters_update(&s, x86) == LZMA_OPTIONS_ERROR);
		CHECK(lzma_filters_update(&s, plain) == LZMA_OK);
		s.next_in = in; s.avail_in = 1000; s.next_out = out; s.avail_out = cap;
		CHECK(lzma_code(&s, LZMA_SYNC_FLUSH) == LZMA_STREAM_END);
		CHECK(lzma_filters_update(&s, plain) == LZMA_PROG_ERROR);
		CHECK(lzma_code(&s, LZMA_FULL_FLUSH) == LZMA_STREAM_END);
		CHECK(lzma_filters_update(&s, plain) == LZMA_OK);
		/* re-init of a live stream replaces the coder; a failing init ends it */
		CHECK(lzma_easy_encoder(&s, 1, LZMA_CHECK_NONE) == LZMA_OK);
		CHECK(lzma_easy_encoder(&s, 6, LZMA_CHECK_SHA256) == LZMA_OPTIONS_ERROR);
		CHECK(s.internal == NULL);
		lzma_end(&s);
	}
	xzamd_release_parked();
	free(in);
	free(out);
	printf("driver_single: ok\n");
	return 0;
}
