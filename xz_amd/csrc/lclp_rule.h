/* lclp_rule.h -- the automatic per-Block literal context (DESIGN.md 3.5 "Automatic literal context"): statistic, candidates,
 * costs and the rule, in plain C so that the device kernels (lzma_filters.hip), the CPU stand-in of the host tests and the
 * numpy model of the tests (tests/_auto_lclp.py restates it) compute the same integers.  Sample set, integer log and its
 * table are those of the automatic delta (delta_rule.h). */
#ifndef XZAMD_LCLP_RULE_H
#define XZAMD_LCLP_RULE_H
#include "delta_rule.h"

/* The statistic of a Block: H[pos & 7][prev >> 5][byte] over its sample set -- pos = offset in the Block, prev = the byte in
 * front (0 at offset 0), of the bytes LZMA2 codes.  The context histogram of every candidate is a marginal of it. */
#define XZAMD_LL_CELLS 64u                  /* (pos & 7) * 8 + (prev >> 5) */
#define XZAMD_LL_HIST_WORDS (XZAMD_LL_CELLS * 256u)   /* uint32_t per Block */
#define XZAMD_LL_MAXCAND 15u                /* pairs with lc <= 3, lp <= 3, lc + lp <= 4: 13, and room for the job's own */
#define XZAMD_LL_CELL 3072u                 /* 1/256 bit charged per used (context, byte) cell: what the adaptive coder pays to learn it */
#define XZAMD_LL_MARGIN 32u                 /* 1/256 bit per sampled byte the best candidate must win by: an eighth of a bit */
#define XZAMD_LL_PROPS(lc, lp) ((uint32_t)(lc) | (uint32_t)(lp) << 8)      /* an entry of the props table */

/* The candidates of a job with (lc, lp): its own pair first, then every other pair with no more literal coders, lc <= 3 and
 * lp <= 3, by lp then lc.  A job's pair the statistic cannot price (lc or lp above 3) stands alone.  Returns their number;
 * cand[k] = XZAMD_LL_PROPS of candidate k. */
XZAMD_DR_FN uint32_t xzamd_ll_cands(uint32_t lc, uint32_t lp, uint32_t cand[XZAMD_LL_MAXCAND])
{
	uint32_t n = 0;
	cand[n++] = XZAMD_LL_PROPS(lc, lp);
	if (lc > 3 || lp > 3) return n;
	for (uint32_t p = 0; p < 4; ++p)
		for (uint32_t c = 0; c < 4; ++c)
			if (c + p <= lc + lp && !(c == lc && p == lp)) cand[n++] = XZAMD_LL_PROPS(c, p);
	return n;
}

/* One byte value's part of a candidate's cost: h[cell * stride] = its 64 counts.  Adds sum over the contexts of c * L(c) to
 * *cl and the number of contexts with c != 0 to *used, c = the count of the byte under the context (the low lp bits of pos,
 * the high lc bits of prev). */
XZAMD_DR_FN void xzamd_ll_byte(const uint32_t *h, uint32_t stride, uint32_t lc, uint32_t lp, const uint8_t *T, uint64_t *cl,
		uint32_t *used)
{
	for (uint32_t a = 0; a < (1u << lp); ++a)
		for (uint32_t b = 0; b < (1u << lc); ++b) {
			uint32_t c = 0;
			for (uint32_t p = a; p < 8; p += 1u << lp)
				for (uint32_t q = b << (3 - lc); q < (b + 1) << (3 - lc); ++q)
					c += h[(p * 8 + q) * stride];
			*cl += (uint64_t)c * xzamd_ad_log(c, T);
			*used += c != 0;
		}
}

/* sum over the contexts of N * L(N), N = the sampled bytes under the context; n[cell] = the sampled bytes of every cell */
XZAMD_DR_FN uint64_t xzamd_ll_ctx(const uint32_t n[XZAMD_LL_CELLS], uint32_t lc, uint32_t lp, const uint8_t *T)
{
	uint64_t s = 0;
	for (uint32_t a = 0; a < (1u << lp); ++a)
		for (uint32_t b = 0; b < (1u << lc); ++b) {
			uint32_t c = 0;
			for (uint32_t p = a; p < 8; p += 1u << lp)
				for (uint32_t q = b << (3 - lc); q < (b + 1) << (3 - lc); ++q)
					c += n[p * 8 + q];
			s += (uint64_t)c * xzamd_ad_log(c, T);
		}
	return s;
}

/* cost of a candidate in 1/256 bit: the order-0 cost of the bytes under its contexts and the charge for the cells it uses */
XZAMD_DR_FN uint64_t xzamd_ll_cost(uint64_t ctx, uint64_t cl, uint32_t used)
{
	return ctx - cl + (uint64_t)XZAMD_LL_CELL * used;
}

/* The rule on the costs S[k] of the ncand candidates (Ns = samples): the index of the candidate to use.  The cheapest one
 * -- ties: fewer literal coders, then the smaller lp -- when it beats the job's own (index 0) by the margin. */
XZAMD_DR_FN uint32_t xzamd_ll_rule(const uint64_t *S, const uint32_t *cand, uint32_t ncand, uint64_t Ns)
{
	uint32_t best = 0;
	for (uint32_t k = 1; k < ncand; ++k) {
		const uint32_t sk = (cand[k] & 255u) + (cand[k] >> 8), sb = (cand[best] & 255u) + (cand[best] >> 8);
		if (S[k] < S[best] || (S[k] == S[best] && (sk < sb || (sk == sb && (cand[k] >> 8) < (cand[best] >> 8))))) best = k;
	}
	return Ns != 0 && S[best] + (uint64_t)XZAMD_LL_MARGIN * Ns <= S[0] ? best : 0u;
}

/* Statistic -> choice, serially (the CPU stand-in; the device splits the same calls over a workgroup): XZAMD_LL_PROPS of
 * the pair for a Block with the histogram H of a job with (lc, lp). */
XZAMD_DR_FN uint32_t xzamd_ll_choose(const uint32_t *H, uint32_t lc, uint32_t lp, const uint8_t *T)
{
	uint32_t cand[XZAMD_LL_MAXCAND], n[XZAMD_LL_CELLS];
	uint64_t S[XZAMD_LL_MAXCAND], Ns = 0;
	const uint32_t ncand = xzamd_ll_cands(lc, lp, cand);
	if (ncand == 1) return cand[0];
	for (uint32_t i = 0; i < XZAMD_LL_CELLS; ++i) {
		n[i] = 0;
		for (uint32_t v = 0; v < 256; ++v) n[i] += H[i * 256 + v];
		Ns += n[i];
	}
	for (uint32_t k = 0; k < ncand; ++k) {
		uint64_t cl = 0;
		uint32_t used = 0;
		for (uint32_t v = 0; v < 256; ++v) xzamd_ll_byte(H + v, 256, cand[k] & 255u, cand[k] >> 8, T, &cl, &used);
		S[k] = xzamd_ll_cost(xzamd_ll_ctx(n, cand[k] & 255u, cand[k] >> 8, T), cl, used);
	}
	return cand[xzamd_ll_rule(S, cand, ncand, Ns)];
}
#endif
