/* stub_xzk_lclp.c -- TEST INFRASTRUCTURE ONLY: CPU stand-ins for the three kernel entry points of the automatic per-Block
 * literal context (xz_amd/csrc/lzma_filters.hip: xzk_lclp_stats, xzk_lclp_choose, xzk_lclp_read), next to stub_xzk.c, for the
 * host-layer program tests/host_stub/driver_auto_lclp.c (tests/test_host_auto_lclp.py) and, through the small entry points at
 * the end, for the rule test (tests/test_auto_lclp_rule.py loads this file alone as a shared object).  They restate
 * xz_amd/csrc/lclp_rule.h in the plainest form: one loop over the sample set, then xzamd_ll_choose.
 *   __wrap_xzk_parse_pieces, _model_snapshots, _encode_syms, _span_encode
 *       the program is linked with --wrap for the four: each call is checked against the batch it belongs to -- the batch
 *       whose statistic was taken of the same input pointer -- before the stand-in of stub_xzk.c runs: the props table in the
 *       span arguments must be the one xzk_lclp_choose filled for THAT batch (the right pipeline parity) and still hold what
 *       it wrote; without the flag it must be NULL.  stub_lclp_seen counts the checked calls, stub_lclp_bad the failures. */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../xz_amd/csrc/kernels_api.h"
#include "../../xz_amd/csrc/lclp_rule.h"
#include <string.h>

static const uint8_t T[256] = XZAMD_AD_LOG_TABLE;

#ifndef STUB_LCLP_RULE_ONLY
#define LOG_MAX 64
#define LOG_BLOCKS 16
static struct {
	const uint8_t *in;              /* the input the statistic was taken of: names the batch */
	const uint32_t *hist;
	const uint32_t *props;          /* where xzk_lclp_choose wrote */
	uint32_t nb, wrote[LOG_BLOCKS];
} batch_log[LOG_MAX];
static uint32_t nlog;
int stub_lclp_calls[3];         /* calls of the three entry points */
int stub_lclp_seen, stub_lclp_bad;
int stub_lclp_expect;           /* 1: the encode runs with the flag */

void stub_lclp_reset(int expect)
{
	nlog = 0;
	memset(stub_lclp_calls, 0, sizeof(stub_lclp_calls));
	stub_lclp_seen = stub_lclp_bad = 0;
	stub_lclp_expect = expect;
}
#endif

static void stats_block(const uint8_t *x, uint32_t blen, uint32_t *h)
{
	for (uint32_t i = 0; i < blen; ++i) {
		if (i % XZAMD_AD_PERIOD >= XZAMD_AD_WINDOW) continue;
		const uint32_t prev = i ? x[i - 1] : 0u;
		++h[(((i & 7u) * 8u + (prev >> 5)) << 8) + x[i]];
	}
}

int xzk_lclp_stats(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t *d_hist, void *stream)
{
	(void)stream;
	memset(d_hist, 0, (size_t)nblocks * XZAMD_LL_HIST_WORDS * 4);
	for (uint32_t b = 0; b < nblocks; ++b) {
		const uint64_t bs = (uint64_t)b * block_size;
		if (bs >= n) break;
		stats_block(d_in + bs, n - bs < block_size ? (uint32_t)(n - bs) : block_size, d_hist + (size_t)b * XZAMD_LL_HIST_WORDS);
	}
#ifndef STUB_LCLP_RULE_ONLY
	++stub_lclp_calls[0];
	if (nlog < LOG_MAX) { batch_log[nlog].in = d_in; batch_log[nlog].hist = d_hist; batch_log[nlog].props = NULL; batch_log[nlog].nb = nblocks; ++nlog; }
#endif
	return 0;
}

int xzk_lclp_choose(const uint32_t *d_hist, uint32_t nblocks, uint32_t lc, uint32_t lp, uint32_t *d_props, void *stream)
{
	(void)stream;
	for (uint32_t b = 0; b < nblocks; ++b)
		d_props[b] = xzamd_ll_choose(d_hist + (size_t)b * XZAMD_LL_HIST_WORDS, lc, lp, T);
#ifndef STUB_LCLP_RULE_ONLY
	++stub_lclp_calls[1];
	if (nlog && batch_log[nlog - 1].hist == d_hist && batch_log[nlog - 1].nb == nblocks) {
		batch_log[nlog - 1].props = d_props;
		for (uint32_t b = 0; b < nblocks && b < LOG_BLOCKS; ++b) batch_log[nlog - 1].wrote[b] = d_props[b];
	} else
		++stub_lclp_bad;
#endif
	return 0;
}

int xzk_lclp_read(const uint32_t *d_hist, const uint32_t *d_props, uint32_t nblocks, uint32_t *h_hist, uint32_t *h_props, void *stream)
{
	(void)stream;
#ifndef STUB_LCLP_RULE_ONLY
	++stub_lclp_calls[2];
#endif
	if (h_hist) memcpy(h_hist, d_hist, (size_t)nblocks * XZAMD_LL_HIST_WORDS * 4);
	if (h_props) memcpy(h_props, d_props, (size_t)nblocks * 4);
	return 0;
}

#ifndef STUB_LCLP_RULE_ONLY
static void seen(const xzamd_span_args *a)
{
	++stub_lclp_seen;
	if (!stub_lclp_expect) {
		if (a->props_tab) ++stub_lclp_bad;
		return;
	}
	for (uint32_t i = nlog; i-- > 0; )
		if (batch_log[i].in == a->in) {
			if (a->props_tab == NULL || a->props_tab != batch_log[i].props) { ++stub_lclp_bad; return; }
			for (uint32_t b = 0; b < batch_log[i].nb && b < LOG_BLOCKS; ++b)
				if (a->props_tab[b] != batch_log[i].wrote[b]) { ++stub_lclp_bad; return; }
			return;
		}
	++stub_lclp_bad;            /* a launch on an input no statistic was taken of */
}

int __real_xzk_parse_pieces(const xzamd_span_args *a, uint32_t nblocks, int phase, uint32_t waves, uint32_t *counter, void *stream);
int __wrap_xzk_parse_pieces(const xzamd_span_args *a, uint32_t nblocks, int phase, uint32_t waves, uint32_t *counter, void *stream)
{
	seen(a);
	return __real_xzk_parse_pieces(a, nblocks, phase, waves, counter, stream);
}
int __real_xzk_model_snapshots(const xzamd_span_args *a, uint32_t nblocks, void *stream);
int __wrap_xzk_model_snapshots(const xzamd_span_args *a, uint32_t nblocks, void *stream)
{
	seen(a);
	return __real_xzk_model_snapshots(a, nblocks, stream);
}
int __real_xzk_encode_syms(const xzamd_span_args *a, uint32_t nblocks, void *stream);
int __wrap_xzk_encode_syms(const xzamd_span_args *a, uint32_t nblocks, void *stream)
{
	seen(a);
	return __real_xzk_encode_syms(a, nblocks, stream);
}
int __real_xzk_span_encode(const xzamd_span_args *a, uint32_t nslots, uint32_t waves, uint32_t *counter, void *stream);
int __wrap_xzk_span_encode(const xzamd_span_args *a, uint32_t nslots, uint32_t waves, uint32_t *counter, void *stream)
{
	seen(a);
	return __real_xzk_span_encode(a, nslots, waves, counter, stream);
}
#endif

/* for the rule test: histogram, candidates and costs of one Block in one call; returns the chosen lc | lp << 8 */
uint32_t stub_lclp_block(const uint8_t *x, uint32_t blen, uint32_t lc, uint32_t lp, uint32_t *hist, uint32_t *cand, uint64_t *S,
		uint32_t *ncand_out)
{
	uint32_t n[XZAMD_LL_CELLS];
	memset(hist, 0, XZAMD_LL_HIST_WORDS * 4);
	stats_block(x, blen, hist);
	const uint32_t ncand = xzamd_ll_cands(lc, lp, cand);
	for (uint32_t i = 0; i < XZAMD_LL_CELLS; ++i) {
		n[i] = 0;
		for (uint32_t v = 0; v < 256; ++v) n[i] += hist[i * 256 + v];
	}
	S[0] = 0;                   /* (a pair that stands alone is not priced) */
	for (uint32_t k = 0; ncand > 1 && k < ncand; ++k) {
		uint64_t cl = 0;
		uint32_t used = 0;
		for (uint32_t v = 0; v < 256; ++v) xzamd_ll_byte(hist + v, 256, cand[k] & 255u, cand[k] >> 8, T, &cl, &used);
		S[k] = xzamd_ll_cost(xzamd_ll_ctx(n, cand[k] & 255u, cand[k] >> 8, T), cl, used);
	}
	*ncand_out = ncand;
	return xzamd_ll_choose(hist, lc, lp, T);
}
