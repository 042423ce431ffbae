/* rule_auto_bcj.c -- TEST INFRASTRUCTURE ONLY: xz_amd/csrc/auto_bcj_rule.h as a program (tests/test_auto_bcj_rule.py).
 *   rule_auto_bcj INPUT BLOCK_SIZE HIST_OUT
 * cuts INPUT into Blocks and prints per Block one line "kind N_x86 N_arm64 S_rel_x86 S_abs_x86 S_rel_arm64 S_abs_arm64"; the
 * histograms ([Block][candidate][stored, absolute][bucket], uint32_t, as the device lays them out) go to HIST_OUT. */
#include "../../xz_amd/csrc/auto_bcj_rule.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv)
{
	static const uint8_t T[256] = XZAMD_AD_LOG_TABLE;
	if (argc != 4) return 2;
	const uint32_t bs = (uint32_t)strtoul(argv[2], NULL, 10);
	FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[3], "wb");
	if (!f || !g || bs == 0) return 2;
	uint8_t *x = (uint8_t *)malloc((size_t)bs + 1);
	uint32_t *h = (uint32_t *)malloc(XZAMD_AB_HIST_WORDS * 4);
	if (!x || !h) return 2;
	for (;;) {
		const uint32_t len = (uint32_t)fread(x, 1, bs, f);
		if (len == 0) break;
		uint64_t N[XZAMD_AB_NCAND], S[2][XZAMD_AB_NCAND];
		memset(h, 0, XZAMD_AB_HIST_WORDS * 4);
		for (uint32_t k = 0; k < XZAMD_AB_NCAND; ++k) {
			N[k] = 0;
			for (uint32_t i = 0; i < len; ++i) {
				uint32_t rel, ab;
				if (!xzamd_ab_site(x, len, i, k, &rel, &ab)) continue;
				++h[(k * 2 + 0) * XZAMD_AB_BUCKETS + xzamd_ab_hash(rel)];
				++h[(k * 2 + 1) * XZAMD_AB_BUCKETS + xzamd_ab_hash(ab)];
				++N[k];
			}
			for (uint32_t w = 0; w < 2; ++w) {
				uint64_t sum = 0;
				for (uint32_t v = 0; v < XZAMD_AB_BUCKETS; ++v) {
					const uint32_t c = h[(k * 2 + w) * XZAMD_AB_BUCKETS + v];
					sum += (uint64_t)c * xzamd_ad_log(c, T);
				}
				S[w][k] = xzamd_ab_cost(N[k], sum, T);
			}
		}
		printf("%u %llu %llu %llu %llu %llu %llu\n", xzamd_ab_rule(S[0], S[1], N, len), (unsigned long long)N[0], (unsigned long long)N[1],
				(unsigned long long)S[0][0], (unsigned long long)S[1][0], (unsigned long long)S[0][1], (unsigned long long)S[1][1]);
		if (fwrite(h, 4, XZAMD_AB_HIST_WORDS, g) != XZAMD_AB_HIST_WORDS) return 2;
	}
	free(x); free(h);
	return fclose(g) != 0 || fclose(f) != 0;
}
