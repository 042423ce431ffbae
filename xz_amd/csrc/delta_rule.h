/* delta_rule.h -- the automatic per-Block delta filter (DESIGN.md 3.5 "Automatic delta"): candidates, sample set, integer
 * log and the rule, in plain C so that the device kernels (lzma_filters.hip), the CPU stand-in of the host tests and the
 * numpy model of the tests (tests/_auto_delta.py restates it) compute the same integers. */
#ifndef XZAMD_DELTA_RULE_H
#define XZAMD_DELTA_RULE_H
#include <stdint.h>

#ifdef __HIPCC__
#define XZAMD_DR_FN __host__ __device__ static inline
#else
#define XZAMD_DR_FN static inline
#endif

#define XZAMD_AD_NCAND 11u                 /* candidates: index 0 = no filter */
#define XZAMD_AD_MAXDIST 32u
#define XZAMD_AD_PERIOD 65536u             /* the sample set of a Block: offsets i with (i mod PERIOD) < WINDOW */
#define XZAMD_AD_WINDOW 4096u
#define XZAMD_AD_MARGIN 128u               /* 1/256 bit per sampled byte the best filter must win by: half a bit */
#define XZAMD_AD_HIST_WORDS (XZAMD_AD_NCAND * 256u)   /* uint32_t per Block */

/* the distance of candidate k (0: none) */
XZAMD_DR_FN uint32_t xzamd_ad_dist(uint32_t k)
{
	return k <= 4 ? k : k == 5 ? 6u : k == 6 ? 8u : k == 7 ? 12u : k == 8 ? 16u : k == 9 ? 24u : 32u;
}

/* T[m] = floor(256 * log2(1 + m / 256) + 0.5) */
#define XZAMD_AD_LOG_TABLE { \
	  0,   1,   3,   4,   6,   7,   9,  10,  11,  13,  14,  16,  17,  18,  20,  21, \
	 22,  24,  25,  26,  28,  29,  30,  32,  33,  34,  36,  37,  38,  40,  41,  42, \
	 44,  45,  46,  47,  49,  50,  51,  52,  54,  55,  56,  57,  59,  60,  61,  62, \
	 63,  65,  66,  67,  68,  69,  71,  72,  73,  74,  75,  77,  78,  79,  80,  81, \
	 82,  84,  85,  86,  87,  88,  89,  90,  92,  93,  94,  95,  96,  97,  98,  99, \
	100, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 116, 117, \
	118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 130, 131, 132, 133, \
	134, 135, 136, 137, 138, 139, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149, \
	150, 151, 152, 153, 154, 155, 155, 156, 157, 158, 159, 160, 161, 162, 163, 164, \
	165, 166, 167, 168, 169, 169, 170, 171, 172, 173, 174, 175, 176, 177, 178, 178, \
	179, 180, 181, 182, 183, 184, 185, 185, 186, 187, 188, 189, 190, 191, 192, 192, \
	193, 194, 195, 196, 197, 198, 198, 199, 200, 201, 202, 203, 203, 204, 205, 206, \
	207, 208, 208, 209, 210, 211, 212, 212, 213, 214, 215, 216, 216, 217, 218, 219, \
	220, 220, 221, 222, 223, 224, 224, 225, 226, 227, 228, 228, 229, 230, 231, 231, \
	232, 233, 234, 234, 235, 236, 237, 238, 238, 239, 240, 241, 241, 242, 243, 244, \
	244, 245, 246, 247, 247, 248, 249, 249, 250, 251, 252, 252, 253, 254, 255, 255 }

/* L(c) = 256 * log2(c) in 1/256 bit: 256 * e + T[the 8 bits below the leading one of c], L(0) = 0 */
XZAMD_DR_FN uint32_t xzamd_ad_log(uint32_t c, const uint8_t *T)
{
	if (c == 0) return 0;
	uint32_t e = 31;
	while (!(c >> e)) --e;
	const uint32_t m = (e >= 8 ? c >> (e - 8) : c << (8 - e)) & 255u;
	return 256u * e + T[m];
}

/* The rule on the costs S[k] of the candidates (Ns = samples): the candidate index to use, 0 = no filter.  The cheapest
 * filter (ties: the smaller distance) when it beats no filter by the margin. */
XZAMD_DR_FN uint32_t xzamd_ad_rule(const uint64_t S[XZAMD_AD_NCAND], uint64_t Ns)
{
	uint32_t best = 1;
	for (uint32_t k = 2; k < XZAMD_AD_NCAND; ++k)
		if (S[k] < S[best]) best = k;
	return Ns != 0 && S[best] + (uint64_t)XZAMD_AD_MARGIN * Ns <= S[0] ? best : 0u;
}
#endif
