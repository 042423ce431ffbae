/*
 * xzamd_options.c -- what an LZMA2 option set means on the device path: the presets and their device mapping, the
 * option sets the device path runs, the encode mode an option set selects and the work memory it needs.  Plain host
 * code: no device call and no context.
 */
#include "xzamd_internal.h"
#include "delta_rule.h"
#include "auto_bcj_rule.h"
#include "lclp_rule.h"

#include <string.h>

/* ------------------------------------------------------------------ */
/* presets                                                              */
/* ------------------------------------------------------------------ */
/* What a BT2/BT3/BT4 request runs on the device: the suffix-neighbourhood finder over a suffix order deep enough
 * for the request's nice_len, the windowed optimal parser, cost-balanced spans. */
void xzamd_sn_defaults(xzamd_lzma_options *o)
{
	o->gpu_sa_window = XZAMD_SA_WINDOW_MAX;
	o->gpu_parser = 1;
	o->gpu_sa_depth = o->gpu_nice_len <= 32 ? 32 : o->gpu_nice_len <= 64 ? 64 : 256;
	/* nice_len > 128 (the extreme presets) asks for ratio first: twice the output per span on compressible Blocks */
	o->span_cost = XZAMD_SPAN_COST_DEFAULT;
	o->span_bits = (o->gpu_nice_len > 128 ? 2 : 1) * XZAMD_SPAN_BITS_DEFAULT;
	o->enc_span_bits = XZAMD_ENC_SPAN_BITS_DEFAULT;
}

int xzamd_lzma_preset(xzamd_lzma_options *o, uint32_t preset)
{
	/* lzma/lzma_encoder_presets.c:17-63 */
	const uint32_t level = preset & 0x1F;
	const uint32_t flags = preset & ~0x1Fu;
	if (level > 9 || (flags & ~XZAMD_PRESET_EXTREME))
		return 1;
	static const uint8_t dict_log2[10] = { 18, 20, 21, 22, 22, 23, 23, 24, 25, 26 };
	memset(o, 0, sizeof(*o));
	o->dict_size = 1u << dict_log2[level];
	o->lc = 3; o->lp = 0; o->pb = 2;
	if (level <= 3) {
		static const uint8_t depths[4] = { 4, 8, 24, 48 };
		o->mode = XZAMD_MODE_FAST;
		o->mf = level == 0 ? XZAMD_MF_HC3 : XZAMD_MF_HC4;
		o->nice_len = level <= 1 ? 128 : 273;
		o->depth = depths[level];
	} else {
		o->mode = XZAMD_MODE_NORMAL;
		o->mf = XZAMD_MF_BT4;
		o->nice_len = level == 4 ? 16 : (level == 5 ? 32 : 64);
		o->depth = 0;
	}
	if (flags & XZAMD_PRESET_EXTREME) {
		o->mode = XZAMD_MODE_NORMAL;
		o->mf = XZAMD_MF_BT4;
		if (level == 3 || level == 5) { o->nice_len = 192; o->depth = 0; }
		else { o->nice_len = 273; o->depth = 512; }
	}
	/* Device mapping.  Fast-mode HC3/HC4 chains run exactly as requested.
	 * BT4/normal chains (presets 4-9, -e): BT4 relinks its tree at every
	 * insert, i.e. is sequential per Block; the device runs its parallel
	 * successor, the suffix-neighbourhood finder (the recency records of the
	 * 32-byte-prefix suffix order are the nodes BT4's descent visits), and a
	 * windowed form of the optimal parser. */
	if (o->mf == XZAMD_MF_HC3 || o->mf == XZAMD_MF_HC4) {
		o->gpu_mf = o->mf;
		o->gpu_nice_len = o->nice_len;
		o->gpu_depth = o->depth;
	} else {
		/* BT4 + normal mode -> suffix-neighbourhood finder + windowed optimal parser */
		o->gpu_mf = XZAMD_MF_HC4;
		o->gpu_nice_len = o->nice_len;
		o->gpu_depth = 1;
		xzamd_sn_defaults(o);
	}
	o->span_size = XZAMD_SPAN_DEFAULT;
	return 0;
}

uint64_t xzamd_mt_block_size(const xzamd_lzma_options *o)
{
	const uint64_t b = (uint64_t)o->dict_size * 3;
	return b > (1u << 20) ? b : (1u << 20);
}

/* The one place that says which LZMA2 option sets the device path runs (used by the batch entry point and
 * by lzma_stream_encoder_mt, so an unsupported set is refused at init, not mid-stream).  NULL = fine. */
const char *xzamd_options_check(const xzamd_lzma_options *opt)
{
	if (opt->lc > 4 || opt->lp > 4 || opt->lc + opt->lp > 4 || opt->pb > 4)
		return "lc + lp <= 4 and pb <= 4 required (lzma_encoder.c:440-470)";
	if ((opt->gpu_mf != XZAMD_MF_HC3 && opt->gpu_mf != XZAMD_MF_HC4)
			|| opt->gpu_depth < 1 || opt->gpu_depth > 56 || opt->gpu_sa_window > XZAMD_SA_WINDOW_MAX
			|| (opt->gpu_sa_window && (opt->gpu_mf != XZAMD_MF_HC4 || !opt->gpu_parser)) || opt->gpu_parser > 1
			|| opt->gpu_nice_len < (opt->gpu_mf & 0x0F) || opt->gpu_nice_len > 273)
		return "unsupported match finder options for the device path";
	if (opt->dict_size < 4096 || opt->dict_size > (1u << 30))
		return "dict_size must be 4 KiB .. 1 GiB on the device path";
	if ((opt->bcj != 0 && !xzamd_prefilter_valid_(opt->bcj)) || (opt->bcj2 != 0 && (opt->bcj == 0 || !xzamd_prefilter_valid_(opt->bcj2)))
			|| (opt->bcj3 != 0 && (opt->bcj2 == 0 || !xzamd_prefilter_valid_(opt->bcj3))))
		return "filters in front of LZMA2: up to three of x86 / PowerPC / IA-64 / ARM / ARM-Thumb / SPARC / ARM64 / RISC-V BCJ or delta";
	/* pb = 3, 4 (lzma/lzma_common.h:32-37) with the optimal parser: in two-phase mode the parse pieces price with a
	 * pb = 2 view of the positions (their model is the parser's alone) and the coder's continuous model runs the real pb
	 * (k_parse_pieces / k_model_syms).  The single-phase span kernel has ONE model for both: pb <= 2. */
	if (opt->gpu_parser && opt->pb > 2 && !xzamd_mode_of_(opt).two)
		return "pb > 2 with the optimal parser needs the two-phase mode (default spans); the single-phase parser's price tables cover pb <= 2";
	if (opt->gpu_sa_depth != 0 && opt->gpu_sa_depth != 32 && opt->gpu_sa_depth != 64 && opt->gpu_sa_depth != 128
			&& opt->gpu_sa_depth != 256)
		return "gpu_sa_depth: 32, 64, 128 or 256";
	if (opt->part_iters > XZAMD_PART_ITERS_MAX)
		return "part_iters: 0 (default) .. 8";
	return NULL;
}

/* The encode mode of an option set -- which span plan, which parse / code split, which list format -- derived here and
 * nowhere else: the batch encoder (xzamd_host.c) and the memory figure below read the same answers. */
#define DEFAULT_SPAN (64u * 1024u)          /* fast parser, dictionaries < 1 MiB (preset 0: 1 MiB Blocks) */
#define DEFAULT_SPAN_FAST_BIG (256u * 1024u) /* fast parser, dictionaries >= 1 MiB (presets 1-3: Blocks of 3 MiB and more): a state
                                             * reset costs ~1.3 KB on text / HTML at these presets -- 64 KiB spans: +1.3 ... +2.3 %
                                             * vs liblzma, 256 KiB: +0.5 ... +0.7 % (round 5, 16 MiB Blocks through the oracle) */
#define DEFAULT_SPAN_OPT (128u * 1024u)     /* optimal parser: fewer state resets, still >> resident waves */
xzamd_mode xzamd_mode_of_(const xzamd_lzma_options *opt)
{
	xzamd_mode m;
	/* Match lists of the optimal parser: 8 x u32 per position (7 entries length << 23 | distance-1 and a
	 * trailer) when distances fit 23 bits, else 8 x u32 distances + 8 x u16 lengths. */
	m.list_packed = opt->gpu_parser && opt->dict_size <= (1u << 23);
	/* Span plan.  Optimal parser over the suffix-neighbourhood finder with no explicit span size: cost-balanced
	 * spans cut on the device from the match lists (xzk_span_plan).  Else spans of a fixed size, table written on the host. */
	m.adaptive = opt->gpu_parser && opt->gpu_sa_window && opt->span_cost != 0
			&& (opt->span_size == XZAMD_SPAN_DEFAULT || opt->span_size == XZAMD_SPAN_AUTO);
	/* Two-phase: the spans of the plan are parse pieces, the symbols they record are coded per encode span */
	m.two = m.adaptive && opt->enc_span_bits != 0;
	m.model_slots = (1846u + (0x300u << (opt->lc + opt->lp)) + 63u) & ~63u;   /* probabilities of the model, padded */
	m.span_default = opt->gpu_parser ? DEFAULT_SPAN_OPT : opt->dict_size >= (1u << 20) ? DEFAULT_SPAN_FAST_BIG : DEFAULT_SPAN;
	return m;
}

/* Device work buffers per input byte of a batch: what the batch planner budgets with and what
 * lzma_stream_encoder_mt_memusage reports -- one expression for both. */
double xzamd_work_bytes_per_byte_(const xzamd_lzma_options *opt)
{
	const xzamd_mode m = xzamd_mode_of_(opt);
	double per_byte = 16.0 + 8.0 + 1.2 + 0.5;                        /* sort buffers, two link arrays, scratch, tables */
	if (opt->gpu_sa_window) per_byte += 4.0 + 16.0 + 8.0 + 16.0 + 8.0;   /* prev4, rp8/16, prev24/32, key64, sa + rank */
	else per_byte += 8.0;                                            /* rank, sorted_pos */
	if (opt->gpu_parser) per_byte += 32.0 + 2.0 + (m.list_packed ? 0.0 : 16.0);
	if (m.two) per_byte += 12.0 + 2.0 * XZAMD_TOK_PER_BYTE + 0.3;     /* recorded parse x 2, tokens, piece models in L2 */
	if (m.two) {
		/* the carried model walk: bounds, logged bits and start model per encode-span slot (>= 256 KiB of input), two sets */
		per_byte += 2.0 * (4.0 * XZAMD_LOG_WORDS + 6.0) * (double)m.model_slots / (double)XZAMD_ENC_MIN_LEN;
	}
	if (opt->bcj) per_byte += opt->bcj2 ? 3.0 : 2.0;
	return per_byte;
}

/* What XZAMD_F_AUTO_DELTA adds to that figure: the filtered copy (one per pipeline parity, like a filter named by the
 * caller) and the 11 histograms of every Block. */
double xzamd_auto_delta_bytes_per_byte_(uint64_t block_size)
{
	return 2.0 + 4.0 * XZAMD_AD_HIST_WORDS / (double)(block_size ? block_size : 1);
}

/* What XZAMD_F_AUTO_BCJ adds: the filtered copy (unless the automatic delta has it already) and the four histograms and two
 * site counts of every Block. */
double xzamd_auto_bcj_bytes_per_byte_(uint64_t block_size, int with_auto_delta)
{
	return (with_auto_delta ? 0.0 : 2.0) + 4.0 * (XZAMD_AB_HIST_WORDS + XZAMD_AB_NCAND) / (double)(block_size ? block_size : 1);
}

/* What XZAMD_F_AUTO_LCLP adds: the joint histogram of every Block and its entry of the props table (one per pipeline parity).
 * No copy of the input, and no literal-coder or model buffer grows: a Block never gets more literal coders than the job's. */
double xzamd_auto_lclp_bytes_per_byte_(uint64_t block_size)
{
	return (4.0 * XZAMD_LL_HIST_WORDS + 8.0) / (double)(block_size ? block_size : 1);
}
