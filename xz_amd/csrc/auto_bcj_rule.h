/* auto_bcj_rule.h -- the automatic per-Block BCJ filter (DESIGN.md 3.5 "Automatic BCJ"): candidates, call-site tests, the
 * operand hash and the rule, in plain C so that the device kernels (lzma_filters.hip), the CPU stand-in of the host tests
 * and the numpy model of the tests (tests/_auto_bcj.py restates it) compute the same integers.  The filters themselves are
 * in bcj_rules.h; the integer log L and its table are those of delta_rule.h. */
#ifndef XZAMD_AUTO_BCJ_RULE_H
#define XZAMD_AUTO_BCJ_RULE_H
#include <stdint.h>
#include "delta_rule.h"

/* Candidates, in the order of the rule's preference on a tie.  A further kind is one entry here, its filter id in
 * xzamd_ab_kind, its call-site test in xzamd_ab_site and its encoder in the per-Block filter stage. */
#define XZAMD_AB_NCAND 2u
#define XZAMD_AB_X86 0u
#define XZAMD_AB_ARM64 1u

#define XZAMD_AB_BUCKETS 4096u             /* per histogram; two histograms (operand as it is / made absolute) per candidate */
#define XZAMD_AB_HIST_WORDS (XZAMD_AB_NCAND * 2u * XZAMD_AB_BUCKETS)      /* uint32_t per Block: [candidate][rel, abs][bucket] */
#define XZAMD_AB_NMIN 256u                 /* call sites a Block must hold */
#define XZAMD_AB_DENS 2048u                /* ... and at least one per so many bytes: N * DENS >= len */
#define XZAMD_AB_MARGIN 128u               /* 1/256 bit per site the absolute operands must win by: half a bit */

XZAMD_DR_FN uint32_t xzamd_ab_kind(uint32_t cand)
{
	return cand == XZAMD_AB_X86 ? 4u : 0x0Au;
}

/* the bucket of an operand: Knuth's multiplicative hash, top 12 bits */
XZAMD_DR_FN uint32_t xzamd_ab_hash(uint32_t v)
{
	return (uint32_t)(v * 2654435761u) >> 20;
}

/* Is offset i of the Block x[0..len) a call site of candidate `cand`?  Then *rel = its operand as stored, *ab = the operand
 * the filter would store.  x86: E8 / E9 whose operand's top byte is 00 / FF (the encoder's prev_mask refinement is not
 * modelled); ARM64: BL at a 4-byte offset of the Block (ADRP is not counted).  A site whose operand would cross the Block end
 * is none. */
XZAMD_DR_FN int xzamd_ab_site(const uint8_t *x, uint32_t len, uint32_t i, uint32_t cand, uint32_t *rel, uint32_t *ab)
{
	if (cand == XZAMD_AB_X86) {
		if (len < 5 || i >= len - 4 || (x[i] & 0xFEu) != 0xE8u || (x[i + 4] != 0x00u && x[i + 4] != 0xFFu)) return 0;
		*rel = (uint32_t)x[i + 1] | (uint32_t)x[i + 2] << 8 | (uint32_t)x[i + 3] << 16 | (uint32_t)x[i + 4] << 24;
		*ab = *rel + i + 5u;
		return 1;
	}
	if ((i & 3u) != 0 || len < 4 || i >= len - 3) return 0;
	const uint32_t w = (uint32_t)x[i] | (uint32_t)x[i + 1] << 8 | (uint32_t)x[i + 2] << 16 | (uint32_t)x[i + 3] << 24;
	if ((w >> 26) != 0x25u) return 0;
	*rel = w & 0x03FFFFFFu;
	*ab = (*rel + (i >> 2)) & 0x03FFFFFFu;
	return 1;
}

/* S = N * L(N) - sum: the order-0 cost of a histogram of N operands whose sum of c * L(c) is `sum`, in 1/256 bit */
XZAMD_DR_FN uint64_t xzamd_ab_cost(uint64_t N, uint64_t sum, const uint8_t *T)
{
	return N * xzamd_ad_log((uint32_t)N, T) - sum;
}

/* The rule on the costs of a Block of len bytes: the filter id to use, 0 = no filter.  A candidate fires with enough sites,
 * dense enough, whose absolute operands are cheaper by the margin; among those that fire the larger saving wins, the earlier
 * candidate on a tie. */
XZAMD_DR_FN uint32_t xzamd_ab_rule(const uint64_t S_rel[XZAMD_AB_NCAND], const uint64_t S_abs[XZAMD_AB_NCAND],
		const uint64_t N[XZAMD_AB_NCAND], uint32_t len)
{
	uint32_t kind = 0;
	uint64_t best = 0;
	for (uint32_t k = 0; k < XZAMD_AB_NCAND; ++k) {
		if (N[k] < XZAMD_AB_NMIN || N[k] * XZAMD_AB_DENS < len) continue;
		if (S_abs[k] + (uint64_t)XZAMD_AB_MARGIN * N[k] > S_rel[k]) continue;
		const uint64_t save = S_rel[k] - S_abs[k];
		if (kind == 0 || save > best) { kind = xzamd_ab_kind(k); best = save; }
	}
	return kind;
}
#endif
