/* stub_xzk_autobcj.c -- TEST INFRASTRUCTURE ONLY: CPU stand-ins for the three kernel entry points of the automatic per-Block
 * BCJ filter (xz_amd/csrc/lzma_filters.hip: xzk_bcj_stats, xzk_bcj_choose, xzk_bcj_blocks), next to stub_xzk.c and
 * stub_xzk_delta.c, for the host-layer program tests/host_stub/driver_auto_bcj.c (tests/test_host_auto_bcj.py).  They restate
 * xz_amd/csrc/auto_bcj_rule.h in the plainest form: one loop over every offset of the Block per candidate.  The x86 encoder is
 * the oracle's; the ARM64 encoder (BL and ADRP, pc = offset inside the Block) is written out here. */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../xz_amd/csrc/kernels_api.h"
#include "../../xz_amd/csrc/auto_bcj_rule.h"
#include "../../oracle/oracle.h"
#include <string.h>

int stub_bcj_calls[3];          /* calls of the three entry points */

int xzk_bcj_stats(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t *d_hist, uint32_t *d_nsites,
		void *stream)
{
	(void)stream;
	++stub_bcj_calls[0];
	memset(d_hist, 0, (size_t)nblocks * XZAMD_AB_HIST_WORDS * 4);
	memset(d_nsites, 0, (size_t)nblocks * XZAMD_AB_NCAND * 4);
	for (uint32_t b = 0; b < nblocks; ++b) {
		const uint64_t bs = (uint64_t)b * block_size;
		if (bs >= n) break;
		const uint32_t blen = n - bs < block_size ? (uint32_t)(n - bs) : block_size;
		for (uint32_t k = 0; k < XZAMD_AB_NCAND; ++k) {
			uint32_t *h = d_hist + ((size_t)b * XZAMD_AB_NCAND + k) * 2 * XZAMD_AB_BUCKETS;
			for (uint32_t i = 0; i < blen; ++i) {
				uint32_t rel, ab;
				if (!xzamd_ab_site(d_in + bs, blen, i, k, &rel, &ab)) continue;
				++h[xzamd_ab_hash(rel)];
				++h[XZAMD_AB_BUCKETS + xzamd_ab_hash(ab)];
				++d_nsites[b * XZAMD_AB_NCAND + k];
			}
		}
	}
	return 0;
}

int xzk_bcj_choose(const uint32_t *d_hist, const uint32_t *d_nsites, uint32_t n, uint32_t block_size, uint32_t nblocks,
		uint32_t *d_kind, uint32_t *d_dist, void *stream)
{
	static const uint8_t T[256] = XZAMD_AD_LOG_TABLE;
	(void)stream;
	++stub_bcj_calls[1];
	for (uint32_t b = 0; b < nblocks; ++b) {
		const uint64_t bs = (uint64_t)b * block_size;
		const uint32_t blen = bs >= n ? 0 : n - bs < block_size ? (uint32_t)(n - bs) : block_size;
		uint64_t S[2][XZAMD_AB_NCAND], N[XZAMD_AB_NCAND];
		for (uint32_t k = 0; k < XZAMD_AB_NCAND; ++k) {
			N[k] = d_nsites[b * XZAMD_AB_NCAND + k];
			for (uint32_t w = 0; w < 2; ++w) {
				const uint32_t *h = d_hist + (((size_t)b * XZAMD_AB_NCAND + k) * 2 + w) * XZAMD_AB_BUCKETS;
				uint64_t sum = 0;
				for (uint32_t v = 0; v < XZAMD_AB_BUCKETS; ++v) sum += (uint64_t)h[v] * xzamd_ad_log(h[v], T);
				S[w][k] = xzamd_ab_cost(N[k], sum, T);
			}
		}
		d_kind[b] = xzamd_ab_rule(S[0], S[1], N, blen);
		if (d_dist && d_kind[b]) d_dist[b] = 0;
	}
	return 0;
}

/* ARM64 BCJ encoder of one Block, start offset 0 */
void stub_arm64_encode(uint8_t *buf, uint32_t size)
{
	for (uint32_t pc = 0; pc + 4 <= size; pc += 4) {
		uint32_t instr = buf[pc] | (uint32_t)buf[pc + 1] << 8 | (uint32_t)buf[pc + 2] << 16 | (uint32_t)buf[pc + 3] << 24;
		if ((instr >> 26) == 0x25) {
			instr = 0x94000000u | ((instr + (pc >> 2)) & 0x03FFFFFFu);
		} else if ((instr & 0x9F000000u) == 0x90000000u) {
			const uint32_t src = ((instr >> 29) & 3) | ((instr >> 3) & 0x001FFFFCu);
			if ((src + 0x00020000u) & 0x001C0000u) continue;
			instr &= 0x9000001Fu;
			const uint32_t dest = src + (pc >> 12);
			instr |= (dest & 3) << 29;
			instr |= (dest & 0x0003FFFCu) << 3;
			instr |= (0u - (dest & 0x00020000u)) & 0x00E00000u;
		} else continue;
		buf[pc] = (uint8_t)instr; buf[pc + 1] = (uint8_t)(instr >> 8); buf[pc + 2] = (uint8_t)(instr >> 16); buf[pc + 3] = (uint8_t)(instr >> 24);
	}
}

int xzk_bcj_blocks(const uint8_t *d_in, uint8_t *d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, const uint32_t *d_kind,
		int copy, void *stream)
{
	(void)stream;
	++stub_bcj_calls[2];
	if (copy) memcpy(d_out, d_in, n);
	for (uint32_t b = 0; b < nblocks; ++b) {
		const uint64_t bs = (uint64_t)b * block_size;
		if (bs >= n) break;
		const uint32_t blen = n - bs < block_size ? (uint32_t)(n - bs) : block_size;
		if (d_kind[b] == 0) continue;
		memcpy(d_out + bs, d_in + bs, blen);      /* (the encoders read original bytes, as the kernels do) */
		if (d_kind[b] == 4u) orc_x86_encode(d_out + bs, blen);
		else if (d_kind[b] == 0x0Au) stub_arm64_encode(d_out + bs, blen);
		else return 1;
	}
	return 0;
}
