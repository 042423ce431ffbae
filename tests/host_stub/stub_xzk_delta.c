/* stub_xzk_delta.c -- TEST INFRASTRUCTURE ONLY: CPU stand-ins for the three kernel entry points of the automatic per-Block
 * delta filter (xz_amd/csrc/lzma_filters.hip: xzk_delta_stats, xzk_delta_choose, xzk_delta_blocks), next to stub_xzk.c, for
 * the host-layer program tests/host_stub/driver_auto_delta.c (tests/test_host_auto_delta.py).  They restate
 * xz_amd/csrc/delta_rule.h in the plainest form: one loop over the sample set per candidate.
 *   __wrap_xzk_span_encode   the program is linked with --wrap=xzk_span_encode: the stand-in of stub_xzk.c runs, and the
 *                            spans of Block `stub_delta_force_stored` (-1: none) then report 4096 bytes more than they
 *                            wrote, which makes the layout send that Block out stored */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../xz_amd/csrc/kernels_api.h"
#include "../../xz_amd/csrc/delta_rule.h"
#include <string.h>

int stub_delta_force_stored = -1;
int stub_delta_calls[3];        /* calls of the three entry points */

int xzk_delta_stats(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t *d_hist, void *stream)
{
	(void)stream;
	++stub_delta_calls[0];
	memset(d_hist, 0, (size_t)nblocks * XZAMD_AD_HIST_WORDS * 4);
	for (uint32_t b = 0; b < nblocks; ++b) {
		const uint64_t bs = (uint64_t)b * block_size;
		if (bs >= n) break;
		const uint32_t blen = n - bs < block_size ? (uint32_t)(n - bs) : block_size;
		const uint8_t *x = d_in + bs;
		uint32_t *h = d_hist + (size_t)b * XZAMD_AD_HIST_WORDS;
		for (uint32_t i = 0; i < blen; ++i) {
			if (i % XZAMD_AD_PERIOD >= XZAMD_AD_WINDOW) continue;
			for (uint32_t k = 0; k < XZAMD_AD_NCAND; ++k) {
				const uint32_t d = xzamd_ad_dist(k);
				const uint32_t prev = d != 0 && i >= d ? x[i - d] : 0u;
				++h[k * 256 + ((x[i] - prev) & 255u)];
			}
		}
	}
	return 0;
}

int xzk_delta_choose(const uint32_t *d_hist, uint32_t nblocks, uint32_t *d_dist, void *stream)
{
	static const uint8_t T[256] = XZAMD_AD_LOG_TABLE;
	(void)stream;
	++stub_delta_calls[1];
	for (uint32_t b = 0; b < nblocks; ++b) {
		const uint32_t *h = d_hist + (size_t)b * XZAMD_AD_HIST_WORDS;
		uint64_t S[XZAMD_AD_NCAND], ns = 0;
		for (uint32_t v = 0; v < 256; ++v) ns += h[v];
		for (uint32_t k = 0; k < XZAMD_AD_NCAND; ++k) {
			uint64_t sum = 0;
			for (uint32_t v = 0; v < 256; ++v) sum += (uint64_t)h[k * 256 + v] * xzamd_ad_log(h[k * 256 + v], T);
			S[k] = ns * xzamd_ad_log((uint32_t)ns, T) - sum;
		}
		d_dist[b] = xzamd_ad_dist(xzamd_ad_rule(S, ns));
	}
	return 0;
}

int xzk_delta_blocks(const uint8_t *d_in, uint8_t *d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, const uint32_t *d_dist,
		void *stream)
{
	(void)stream; (void)nblocks;
	++stub_delta_calls[2];
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t b = i / block_size, off = i - b * block_size, d = d_dist[b];
		d_out[i] = (uint8_t)(d_in[i] - (d != 0 && off >= d ? d_in[i - d] : 0));
	}
	return 0;
}

int __real_xzk_span_encode(const xzamd_span_args *a, uint32_t nslots, uint32_t waves, uint32_t *counter, void *stream);
int __wrap_xzk_span_encode(const xzamd_span_args *a, uint32_t nslots, uint32_t waves, uint32_t *counter, void *stream)
{
	const int e = __real_xzk_span_encode(a, nslots, waves, counter, stream);
	if (e || stub_delta_force_stored < 0) return e;
	for (uint32_t s = 0; s < nslots; ++s) {
		const uint32_t b = s / a->max_spb, k = s - b * a->max_spb;
		if ((int)b == stub_delta_force_stored && (uint64_t)b * a->block_size < a->n && k < a->span_cnt[b])
			a->span_bytes[s] += 4096;
	}
	return 0;
}
