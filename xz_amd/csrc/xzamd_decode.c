/*
 * xzamd_decode.c -- host side of the device .xz Stream decoder: container parsing and
 * launch of the Block-parallel LZMA2 decode kernels (lzma_decode.hip).
 *
 * Restates, for a whole single-Stream .xz file resident in HBM, the checks of the reference's decoder chain:
 *   common/stream_flags_decoder.c:30-82     Stream Header / Footer (magic, flags, CRC32, Backward Size)
 *   common/index_decoder.c / index_hash.c   Index (indicator, record count, records, padding, CRC32;
 *                                           sizes must match the Blocks)
 *   common/block_header_decoder.c:17-125    Block Header (size, flags, VLIs, filter flags, padding, CRC32)
 *   common/block_decoder.c:47-230           Compressed / Uncompressed Size vs the header, Block Padding, Check
 *   common/filter_flags_decoder.c:15-45,    Filter Flags: ids, sizes of properties, the rules of a chain (1 to 4 filters,
 *   filter_common.c:250-294,                LZMA2 last and only last), BCJ properties (none, or a 4-byte start offset),
 *   simple/simple_decoder.c:15-39,          delta properties (one byte, distance - 1)
 *   delta/delta_decoder.c:67-85
 *   lzma/lzma2_decoder.c, lzma_decoder.c    -> k_dec_scan / k_dec_units
 *   simple/ (the decoder direction),       -> xzk_dec_unfilter: the inverse filters, last filter of the chain first
 *   delta/delta_decoder.c:17-25
 *   check/crc32_fast.c, crc64_fast.c        -> the encoder's k_crc_strips / k_crc_fold over the decoded bytes
 * Scheduling model of common/stream_decoder_mt.c: independent Blocks in parallel; with the original data at
 * hand (verification) every state-resetting chunk chain is its own unit.
 * The device part (unit scan, decode, inverse filters, Checks, comparison) is xzamd_dec_run_, which the whole-file entries of
 * xzamd_file.c run over the Blocks of several Streams; the per-Block header checks are xzb_header (xzamd_block_parse.h).
 * Supported here: one Stream; the filter chains {LZMA2} and {up to three of: delta | x86 | PowerPC | IA-64 | ARM | ARM-Thumb |
 * SPARC | ARM64 | RISC-V, LZMA2}, which may differ from Block to Block; checks none / CRC32 / CRC64 / SHA-256, all
 * verified.  Declined with XZAMD_OPTIONS_ERROR: a BCJ filter with a non-zero start offset (nothing in this project
 * writes one), every other filter id, every chain the reference's lzma_validate_chain refuses.
 *
 * Buffers of a Stream with filtered Blocks: the LZMA2 stage decodes into a temporary, each inverse stage reads one
 * buffer and writes another (a second temporary for chains of two or three filters), the last stage of a Block writes
 * d_out.  A Stream whose Blocks are all {LZMA2} allocates no temporary and launches no inverse stage.
 * Verification decode of a filtered Stream: the history of the span-parallel units is the FILTERED original, made with
 * the encoder's own forward kernels when the Blocks form the geometry our encoder writes (equally long but the last,
 * one chain); otherwise unit = Block.  The decoded, unfiltered bytes are compared with the original either way.
 */
#include "xzamd_internal.h"
#include "kernels_api.h"
#include "xzamd_block_parse.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define FORMAT_ERROR 7      /* LZMA_FORMAT_ERROR */

/* test instrumentation (not public API): [0] temporary buffers allocated for inverse filters, [1] xzk_dec_unfilter calls,
 * [2] forward-filter launches of verification decodes; process-wide, since the library was loaded */
static uint64_t dec_counters[3];
void xzamd_debug_decode_counters_(uint64_t out[3])
{
	for (int i = 0; i < 3; ++i) out[i] = __atomic_load_n(&dec_counters[i], __ATOMIC_RELAXED);
}
static void count_(int i) { __atomic_fetch_add(&dec_counters[i], 1, __ATOMIC_RELAXED); }
/* ... and of the last decode launch of the process: [0] units, [1] Blocks, [2] the split mode of its scan */
static uint64_t dec_last_units[3];
void xzamd_debug_decode_units_(uint64_t out[3])
{
	for (int i = 0; i < 3; ++i) out[i] = __atomic_load_n(&dec_last_units[i], __ATOMIC_RELAXED);
}

static void reads_(const xzamd_dec_job *j, uint64_t n) { if (j->counts) j->counts[0] += n; }
static void launches_(const xzamd_dec_job *j, uint64_t n) { if (j->counts) j->counts[1] += n; }

const char *xzamd_block_step_msg_(uint32_t step)
{
	static const char *const msg[XZB_S_COUNT] = {
		"", "Block beyond the Index", "Index indicator where a Block Header was expected", "Block Header beyond the Index",
		"Block Header CRC32", "reserved Block Flags", "Block Header Compressed Size", "Block Header Uncompressed Size", "Filter Flags",
		"LZMA2 properties (dictionary size byte)", "delta filter: size of properties", "BCJ filter: size of properties",
		"BCJ filter with a non-zero start offset is not decoded on the device", "filter id the device decoder does not know",
		"Block Header padding", "filter chain: LZMA2 must be the last filter and only the last",
		"Unpadded Size smaller than its header", "Block Header sizes differ from the Index", "Block beyond the Index",
		"Block Padding", "Block too large for the device decoder" };
	return step < XZB_S_COUNT ? msg[step] : "";
}
static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

#define FAILD(code, msg) do { rc = xzamd_ctx_fail_(c, (code), (msg)); goto done; } while (0)
#define HIPD(call, msg) do { if (call) FAILD(XZAMD_DEVICE_ERROR, msg); } while (0)

/* A defect of Block b found by step `vstep` (XZAMD_VSTEP_*): XZAMD_DATA_ERROR, the message names the Block, and the job's report
 * (when it has one) keeps the first such defect */
static int fail_block_(xzamd_ctx *c, const xzamd_dec_job *j, uint64_t b, uint32_t vstep, const char *msg)
{
	char buf[160];
	if (j->report && j->report->first_bad_step == XZAMD_VSTEP_NONE) {
		j->report->first_bad_step = vstep;
		j->report->first_bad_block = b;
	}
	if (b == UINT64_MAX) return xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, msg);
	snprintf(buf, sizeof(buf), "Block %llu: %s", (unsigned long long)b, msg);
	return xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, buf);
}
#define FAILB(b, vstep, msg) do { rc = fail_block_(c, j, (b), (vstep), (msg)); goto done; } while (0)
/* ... in collect mode (j->steps): the Block is marked and the run goes on; the message and the report keep the first defect */
static void mark_block_(xzamd_ctx *c, const xzamd_dec_job *j, uint64_t b, uint32_t vstep, const char *msg, int *any)
{
	if (j->steps[b] == XZAMD_VSTEP_NONE) j->steps[b] = (uint8_t)vstep;
	if (!*any) (void)fail_block_(c, j, b, vstep, msg);
	*any = 1;
}
#define BADB(b, vstep, msg) do { if (!j->steps) FAILB((b), (vstep), (msg)); mark_block_(c, j, (b), (vstep), (msg), &any_bad); } while (0)
#define IS_BAD(b) (j->steps && j->steps[b] != XZAMD_VSTEP_NONE)

/* The device part of a decode: the Blocks of j->hb (parsed and validated: xzb_block) through unit scan, LZMA2 decode,
 * inverse filters, Checks (per group of Blocks = per Stream) and the comparison with the original. */
int xzamd_dec_run_(xzamd_ctx *c, void *st, const xzamd_dec_job *j)
{
	const uint8_t *d_xz = j->d_xz;
	uint8_t *d_out = j->d_out;
	const uint8_t *d_expected = j->d_expected;
	const uint64_t nb = j->nb;
	xzamd_dec_block *hb = j->hb;
	const xzamd_dec_chain *hc = j->hc;
	uint64_t *mismatches = j->mismatches;
	int rc = XZAMD_OK;
	uint64_t *h_crc = NULL;
	uint8_t *h_sha = NULL;
	void *d_sha = NULL;
	uint32_t *unit_first = NULL, *h_err = NULL;
	void *d_blocks = NULL, *d_units = NULL, *d_first = NULL, *d_lit = NULL, *d_misc = NULL, *d_strip = NULL, *d_crc = NULL;
	uint32_t *tile_first = NULL;
	void *d_chains = NULL, *d_tiles = NULL, *d_t0 = NULL, *d_t1 = NULL, *d_filt = NULL, *d_tsum = NULL, *d_tcarry = NULL;
	uint32_t max_nf = 0;
	int any_filtered = 0, any_plain = 0;
	int any_bad = 0;                   /* collect mode: some Block is marked */
	void *d_cmp = NULL;
	uint64_t utotal = 0, max_usize = 0;
	if (j->report) j->report->blocks = nb;
	if (nb == 0) return XZAMD_OK;
	if (nb >= (1ull << 31)) return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR, "too many Blocks for the device decoder");
	for (uint64_t b = 0; b < nb; ++b) {
		if (IS_BAD(b)) any_bad = 1;        /* (marked by the caller, who has reported it) */
		if (hc[b].n) { any_filtered = 1; if (hc[b].n > max_nf) max_nf = hc[b].n; } else any_plain = 1;
		utotal += hb[b].usize;
		if (hb[b].usize > max_usize) max_usize = hb[b].usize;
	}
	h_crc = (uint64_t *)calloc(nb, 8);
	h_err = (uint32_t *)calloc(nb, 4);
	unit_first = (uint32_t *)calloc(nb + 1, 4);
	tile_first = (uint32_t *)calloc(nb + 1, 4);
	if (!h_crc || !h_err || !unit_first || !tile_first) FAILD(XZAMD_MEM_ERROR, "malloc");

	/* unit scan + decode */
	{
		const uint32_t nbk = (uint32_t)nb;
		/* units: with the original (verification) at every state reset that carries the properties; without it at every
		 * dictionary reset -- nothing in front of one can be referenced, so the units of a Block decode side by side with
		 * the output itself as history.  The unit count of a Block is data: the table holds usize / 4096 + 8 per Block,
		 * and in the plain mode a Block with more resets keeps the rest inside its last unit. */
		const int verif = d_expected != NULL && !j->plain_history;      /* the units read their history from the original */
		const int with_table = verif && j->allow_split && j->d_rec != NULL && j->nrec != 0;
		int split = verif ? (j->allow_split ? (with_table ? 3 : 1) : 0) : 2;
		uint32_t units_cap = split ? (uint32_t)(max_usize / 4096 + 8) : 1;
		if ((uint64_t)units_cap * nb > (1ull << 27)) { split = 0; units_cap = 1; }
		uint32_t waves = xzamd_ctx_wave_slots_(c);
		uint8_t *dec_out = d_out;          /* where the LZMA2 stage writes */
		const uint8_t *hist_src = d_expected;
		if (any_filtered) {
			/* the LZMA2 stage of every Block decodes into t0 (one kernel, one output base); a second temporary only for
			 * chains of two or three filters */
			HIPD(xzk_malloc(&d_t0, utotal + 16), "hipMalloc");
			count_(0);
			if (max_nf >= 2) { HIPD(xzk_malloc(&d_t1, utotal + 16), "hipMalloc"); count_(0); }
			HIPD(xzk_malloc(&d_chains, nb * sizeof(xzamd_dec_chain)), "hipMalloc");
			HIPD(xzk_malloc(&d_tiles, 4 * (nb + 1)), "hipMalloc");
			HIPD(xzk_h2d(d_chains, hc, nb * sizeof(xzamd_dec_chain), st), "h2d chains");
			dec_out = (uint8_t *)d_t0;
			if (split == 1 || split == 3) {
				/* The history of a span-parallel unit is what the LZMA2 encoder saw: the filtered original.  Make it with the
				 * encoder's forward kernels when the Stream has the geometry they filter (Blocks equally long but the last,
				 * one chain, < 2 GiB); any other Stream: unit = Block. */
				const uint64_t bs0 = hb[0].usize;
				int same = !any_plain && bs0 != 0 && utotal < (1ull << 31) && hb[nb - 1].usize <= bs0;
				for (uint64_t b = 0; same && b < nb; ++b)
					same = memcmp(&hc[b], &hc[0], sizeof(hc[0])) == 0 && (b + 1 == nb || hb[b].usize == bs0);
				if (!same) { split = 0; units_cap = 1; }
				else {
					HIPD(xzk_malloc(&d_filt, utotal + 16), "hipMalloc");
					count_(0);
					const uint32_t nf = hc[0].n;
					const uint8_t *src = d_expected;
					for (uint32_t i = 0; i < nf; ++i) {
						/* in -> F, in -> t0 -> F, in -> F -> t0 -> F: no step in place; t0 is free until the decode */
						uint8_t *dst = ((nf - 1 - i) & 1) ? (uint8_t *)d_t0 : (uint8_t *)d_filt;
						const uint32_t f = hc[0].f[i];
						HIPD(f == 4u ? xzk_x86_bcj(src, dst, (uint32_t)utotal, (uint32_t)bs0, nbk, st)
								: xzk_prefilter(src, dst, (uint32_t)utotal, (uint32_t)bs0, nbk, f & 0xFFu, (f >> 8) + 1, st),
								"forward filter of the verification decode");
						launches_(j, 1);
						count_(2);
						src = dst;
					}
					hist_src = (const uint8_t *)d_filt;
				}
			}
		}
		HIPD(xzk_malloc(&d_blocks, nb * sizeof(xzamd_dec_block)), "hipMalloc");
		HIPD(xzk_malloc(&d_misc, 4096 + 4 * nb), "hipMalloc");
		HIPD(xzk_malloc(&d_first, 4 * (nb + 1)), "hipMalloc");
	rescan:
		HIPD(xzk_malloc(&d_units, (uint64_t)units_cap * nb * sizeof(xzamd_dec_unit)), "hipMalloc");
		HIPD(xzk_h2d(d_blocks, hb, nb * sizeof(xzamd_dec_block), st), "h2d blocks");
		HIPD(xzk_dec_scan(d_xz, (xzamd_dec_block *)d_blocks, nbk, (xzamd_dec_unit *)d_units, units_cap, split,
				split == 3 ? j->d_rec : NULL, j->rec_stride, j->nrec, st), "scan launch");
		launches_(j, 1);
		HIPD(xzk_d2h(hb, d_blocks, nb * sizeof(xzamd_dec_block), st) || xzk_sync(st), "d2h blocks");
		reads_(j, 1);
		uint32_t total_units = 0;
		uint64_t recs_used = 0;
		int overflow = 0;
		for (uint64_t b = 0; b < nb; ++b) {
			if (!IS_BAD(b)) {                         /* (bad already: its header -- the Block has no chunk chain to speak of) */
				if (hb[b].error == 11) overflow = 1;
				else if (hb[b].error == 13) BADB(b, XZAMD_VSTEP_GRAMMAR, "a resume record names a span start that is no LZMA2 chunk start");
				else if (hb[b].error) BADB(b, XZAMD_VSTEP_GRAMMAR, "LZMA2 chunk grammar");
			}
			if (IS_BAD(b)) hb[b].nunits = 0;          /* out of the decode: its units are not listed */
			unit_first[b] = total_units;
			total_units += hb[b].nunits;
			recs_used += hb[b].nrecs;
		}
		unit_first[nb] = total_units;
		if (overflow) {
			/* more state resets than anticipated: one unit per Block, compared afterwards all the same */
			xzk_free(d_units); d_units = NULL;
			for (uint64_t b = 0; b < nb; ++b) { hb[b].error = 0; hb[b].nunits = 0; }
			/* (collect mode: the Blocks the first scan marked stay marked -- their defect does not depend on the split) */
			split = 0; units_cap = 1;
			goto rescan;
		}
		const uint8_t *hist = split == 1 || split == 3 ? hist_src : NULL;
		const uint32_t work = split ? total_units : nbk;
		if (j->report) {
			j->report->units = work;
			j->report->blocks = nb;
			j->report->table_used = split == 3;
			j->report->records_used = split == 3 ? recs_used : 0;
		}
		__atomic_store_n(&dec_last_units[0], work, __ATOMIC_RELAXED);
		__atomic_store_n(&dec_last_units[1], nb, __ATOMIC_RELAXED);
		__atomic_store_n(&dec_last_units[2], (uint64_t)split, __ATOMIC_RELAXED);
		if (waves > work) waves = work ? work : 1;
		HIPD(xzk_malloc(&d_lit, (uint64_t)waves * (0x300ull << 4) * 2), "hipMalloc");
		HIPD(xzk_memset(d_misc, 0, 4096 + 4 * nb, st), "memset");
		HIPD(xzk_h2d(d_first, unit_first, 4 * (nb + 1), st), "h2d");
		uint32_t *d_counter = (uint32_t *)d_misc;
		unsigned long long *d_mism = (unsigned long long *)((uint8_t *)d_misc + 64);
		uint32_t *d_berr = (uint32_t *)((uint8_t *)d_misc + 4096);
		HIPD(xzk_dec_units(d_xz, (const xzamd_dec_block *)d_blocks, nbk, (const xzamd_dec_unit *)d_units, units_cap,
				(const uint32_t *)d_first, total_units, dec_out, hist, (uint16_t *)d_lit, waves, d_counter, d_berr, split == 2,
				split == 3 ? j->d_rec : NULL, j->rec_stride, st), "decode launch");
		launches_(j, 1);
		HIPD(xzk_d2h(h_err, d_berr, 4 * nb, st) || xzk_sync(st), "decode");
		reads_(j, 1);
		for (uint64_t b = 0; b < nb; ++b)
			if (h_err[b] && !IS_BAD(b)) BADB(b, XZAMD_VSTEP_DECODE, "LZMA2 data (range coder / distances / chunk sizes)");
		if (any_filtered) {
			/* inverse stages, the filter next to LZMA2 first; an unfiltered Block of a mixed Stream is copied in stage 0 */
			xzamd_unf_args ua;
			memset(&ua, 0, sizeof(ua));
			ua.blocks = (const xzamd_dec_block *)d_blocks;
			ua.chains = (const xzamd_dec_chain *)d_chains;
			ua.tile_first = (const uint32_t *)d_tiles;
			ua.nblocks = nbk;
			ua.t0 = (uint8_t *)d_t0; ua.t1 = (uint8_t *)d_t1; ua.out = d_out;
			for (uint32_t k = 0; k < max_nf; ++k) {
				uint64_t tiles = 0;
				uint32_t kinds = 0;
				for (uint64_t b = 0; b < nb; ++b) {
					tile_first[b] = (uint32_t)tiles;
					if (IS_BAD(b)) continue;
					if (hc[b].n > k || (hc[b].n == 0 && k == 0)) {
						const uint32_t kind = hc[b].n ? hc[b].f[hc[b].n - 1 - k] & 0xFFu : 0u;
						tiles += (hb[b].usize + XZAMD_UNF_TILE - 1) / XZAMD_UNF_TILE;
						if (hb[b].usize)
							kinds |= kind == 3u ? XZAMD_UNF_DELTA : kind ? XZAMD_UNF_COPY | XZAMD_UNF_BCJ : XZAMD_UNF_COPY;
					}
				}
				tile_first[nb] = (uint32_t)tiles;
				if (tiles >= (1ull << 31)) FAILD(XZAMD_OPTIONS_ERROR, "Stream too large for the inverse filters");
				if (tiles == 0) continue;
				if ((kinds & XZAMD_UNF_DELTA) && !d_tsum) {
					/* every later stage covers a subset of this stage's Blocks: its tiles fit */
					HIPD(xzk_malloc(&d_tsum, tiles * XZAMD_UNF_ROW) || xzk_malloc(&d_tcarry, tiles * XZAMD_UNF_ROW), "hipMalloc");
				}
				ua.tile_sum = (uint8_t *)d_tsum; ua.tile_carry = (uint8_t *)d_tcarry;
				ua.stage = k;
				/* tile_first is rewritten for the next stage: the copy must have left the host buffer first */
				HIPD(xzk_h2d(d_tiles, tile_first, 4 * (nb + 1), st) || xzk_sync(st), "h2d tiles");
				HIPD(xzk_dec_unfilter(&ua, (uint32_t)tiles, kinds, st), "inverse filter launch");
				launches_(j, 1);
				count_(1);
			}
		}
		/* Block checks over the decoded bytes, one group of Blocks (= the Blocks of one Stream, one kind of Check) after
		 * another; the results of all groups come back in one read per kind */
		int any_crc = 0, any_sha = 0;
		for (uint32_t g = 0; g < j->ngroups; ++g) {
			if (j->groups[g].count == 0) continue;
			if (j->groups[g].check == XZAMD_CHECK_CRC32 || j->groups[g].check == XZAMD_CHECK_CRC64) any_crc = 1;
			if (j->groups[g].check == XZAMD_CHECK_SHA256) any_sha = 1;
		}
		if (any_crc) {
			const uint64_t spb = (max_usize + 4096 - 1) / 4096 + 1;
			HIPD(xzk_malloc(&d_strip, 8 * spb * nb + 64), "hipMalloc");
			HIPD(xzk_malloc(&d_crc, 8 * nb + 64), "hipMalloc");
		}
		if (any_sha) {
			HIPD(xzk_malloc(&d_sha, 32 * nb + 64), "hipMalloc");
			h_sha = (uint8_t *)malloc(32 * nb);
			if (!h_sha) FAILD(XZAMD_MEM_ERROR, "malloc");
		}
		for (uint32_t g = 0; g < j->ngroups; ++g) {
			const int check = j->groups[g].check;
			const uint64_t gn = j->groups[g].count;
			const xzamd_dec_block *gb = hb + j->groups[g].first;
			if (gn == 0 || check == XZAMD_CHECK_NONE) continue;
			/* equally long Blocks but the last: one launch for the group, else one launch per Block */
			int uniform = 1;
			uint64_t gtotal = 0;
			for (uint64_t b = 0; b < gn; ++b) gtotal += gb[b].usize;
			for (uint64_t b = 0; b + 1 < gn; ++b)
				if (gb[b].usize != gb[0].usize) uniform = 0;
			if (gn > 1 && gb[gn - 1].usize > gb[0].usize) uniform = 0;
			uint8_t *gout = d_out + gb[0].upos;
			if (check == XZAMD_CHECK_CRC32 || check == XZAMD_CHECK_CRC64) {
				const uint32_t strip = 4096;
				const uint64_t bs0 = gb[0].usize ? gb[0].usize : 1;
				uint64_t *g_crc = (uint64_t *)d_crc + j->groups[g].first;
				if (uniform && gtotal < (1ull << 31)) {
					HIPD(xzk_crc_blocks(gout, (uint32_t)gtotal, (uint32_t)bs0, (uint32_t)gn, strip, check == XZAMD_CHECK_CRC32,
							(uint64_t *)d_strip, g_crc, st), "crc launch");
					launches_(j, 1);
				} else {
					for (uint64_t b = 0; b < gn; ++b) {
						if (gb[b].usize == 0) { HIPD(xzk_memset(g_crc + b, 0, 8, st), "memset"); continue; }
						HIPD(xzk_crc_blocks(d_out + gb[b].upos, (uint32_t)gb[b].usize, (uint32_t)gb[b].usize, 1, strip,
								check == XZAMD_CHECK_CRC32, (uint64_t *)d_strip, g_crc + b, st), "crc launch");
						launches_(j, 1);
					}
				}
			} else {
				/* check/sha256.c over the decoded bytes: one hash per Block (serial by nature) */
				uint8_t *g_sha = (uint8_t *)d_sha + 32 * j->groups[g].first;
				if (uniform && gtotal < (1ull << 31) && gb[0].usize) {
					HIPD(xzk_sha256_blocks(gout, (uint32_t)gtotal, (uint32_t)gb[0].usize, (uint32_t)gn, g_sha, st), "sha256 launch");
					launches_(j, 1);
				} else {
					for (uint64_t b = 0; b < gn; ++b) {
						HIPD(xzk_sha256_blocks(d_out + gb[b].upos, (uint32_t)gb[b].usize, gb[b].usize ? (uint32_t)gb[b].usize : 1u, 1,
								g_sha + 32 * b, st), "sha256 launch");
						launches_(j, 1);
					}
				}
			}
		}
		if (any_crc) { HIPD(xzk_d2h(h_crc, d_crc, 8 * nb, st), "d2h crc"); reads_(j, 1); }
		if (any_sha) { HIPD(xzk_d2h(h_sha, d_sha, 32 * nb, st), "d2h sha256"); reads_(j, 1); }
		if (any_crc || any_sha) HIPD(xzk_sync(st), "d2h checks");
		for (uint32_t g = 0; g < j->ngroups; ++g) {
			const int check = j->groups[g].check;
			for (uint64_t b = j->groups[g].first; b < j->groups[g].first + j->groups[g].count; ++b) {
				const uint8_t *sb = j->stored + XZAMD_HDR_CHECK_BYTES * b;
				if (IS_BAD(b)) continue;
				if (check == XZAMD_CHECK_CRC32 || check == XZAMD_CHECK_CRC64) {
					uint64_t sv = 0;
					for (uint32_t i = 0; i < (check == XZAMD_CHECK_CRC32 ? 4u : 8u); ++i) sv |= (uint64_t)sb[i] << (8 * i);
					if (h_crc[b] != sv) BADB(b, XZAMD_VSTEP_CHECK, "Block Check mismatch");
				} else if (check == XZAMD_CHECK_SHA256) {
					if (memcmp(h_sha + 32 * b, sb, 32) != 0) BADB(b, XZAMD_VSTEP_CHECK, "Block Check mismatch (SHA-256)");
				}
			}
		}
		if (d_expected && j->steps) {
			/* collect mode: one count of differing bytes per Block that got this far (k_dec_compare_blocks); the global word
			 * count of the plain path only when that path would have reached its comparison */
			uint64_t tiles = 0;
			unsigned long long mm = 0;
			for (uint64_t b = 0; b < nb; ++b) {
				tile_first[b] = (uint32_t)tiles;
				if (!IS_BAD(b)) tiles += (hb[b].usize + XZAMD_UNF_TILE - 1) / XZAMD_UNF_TILE;
			}
			tile_first[nb] = (uint32_t)tiles;
			if (tiles >= (1ull << 31)) FAILD(XZAMD_OPTIONS_ERROR, "Stream too large for the per-Block comparison");
			unsigned long long *h_cnt = (unsigned long long *)h_crc;      /* (the Checks have been looked at) */
			HIPD(xzk_malloc(&d_cmp, 12 * nb + 16), "hipMalloc");
			uint32_t *d_tf = (uint32_t *)((uint8_t *)d_cmp + 8 * nb);
			HIPD(xzk_memset(d_cmp, 0, 8 * nb, st) || xzk_h2d(d_tf, tile_first, 4 * (nb + 1), st), "h2d tiles");
			HIPD(xzk_dec_compare_blocks(d_out, d_expected, (const xzamd_dec_block *)d_blocks, d_tf, nbk, (uint32_t)tiles,
					(unsigned long long *)d_cmp, st), "compare launch");
			launches_(j, 1);
			if (!any_bad) { HIPD(xzk_dec_compare(d_out, d_expected, utotal, d_mism, st), "compare launch"); launches_(j, 1); }
			HIPD(xzk_d2h(h_cnt, d_cmp, 8 * nb, st) || xzk_d2h(&mm, d_mism, 8, st) || xzk_sync(st), "d2h compare");
			reads_(j, 1);
			if (mismatches) *mismatches = mm;
			if (j->report) j->report->mismatching_words = mm;
			for (uint64_t b = 0; b < nb; ++b)
				if (!IS_BAD(b) && h_cnt[b]) BADB(b, XZAMD_VSTEP_COMPARE, "decoded bytes differ from the original");
		} else if (d_expected) {
			unsigned long long mm = 0;
			HIPD(xzk_dec_compare(d_out, d_expected, utotal, d_mism, st), "compare launch");
			launches_(j, 1);
			HIPD(xzk_d2h(&mm, d_mism, 8, st) || xzk_sync(st), "d2h compare");
			reads_(j, 1);
			if (mismatches) *mismatches = mm;
			if (j->report) j->report->mismatching_words = mm;
			if (mm) FAILB(UINT64_MAX, XZAMD_VSTEP_COMPARE, "decoded bytes differ from the original");
		}
	}
	if (any_bad) rc = XZAMD_DATA_ERROR;       /* (message and report: the first defect, set when it was marked) */
done:
	xzk_sync(st);
	if (d_cmp) xzk_free(d_cmp);
	if (d_blocks) xzk_free(d_blocks);
	if (d_units) xzk_free(d_units);
	if (d_first) xzk_free(d_first);
	if (d_lit) xzk_free(d_lit);
	if (d_misc) xzk_free(d_misc);
	if (d_strip) xzk_free(d_strip);
	if (d_crc) xzk_free(d_crc);
	if (d_sha) xzk_free(d_sha);
	if (d_chains) xzk_free(d_chains);
	if (d_tiles) xzk_free(d_tiles);
	if (d_t0) xzk_free(d_t0);
	if (d_t1) xzk_free(d_t1);
	if (d_filt) xzk_free(d_filt);
	if (d_tsum) xzk_free(d_tsum);
	if (d_tcarry) xzk_free(d_tcarry);
	free(tile_first); free(h_sha);
	free(h_crc); free(h_err); free(unit_first);
	return rc;
}

/* xzamd_stream_decode_device; `tab` / `report` (both optional): the verification of xzamd_stream_verify_device */
static int stream_decode_(xzamd_ctx *c, const void *d_xz_, uint64_t xz_size, void *d_out_, uint64_t out_cap,
		uint64_t *out_size, const void *d_expected_, uint64_t expected_size, uint64_t *mismatches, uint64_t *nblocks_out,
		void *stream, const xzamd_resume_view *tab, xzamd_verify_report *report)
{
	if (!c || !d_xz_ || !out_size || (!d_out_ && out_cap))
		return XZAMD_PROG_ERROR;
	const uint8_t *d_xz = (const uint8_t *)d_xz_;
	uint8_t *d_out = (uint8_t *)d_out_;
	const uint8_t *d_expected = (const uint8_t *)d_expected_;
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	int rc = XZAMD_OK;
	uint8_t *index = NULL;
	xzamd_dec_block *hb = NULL;
	uint8_t *stored32 = NULL;          /* the stored Check bytes of every Block */
	xzamd_dec_chain *hc = NULL;        /* per Block: the filters in front of LZMA2 */
	*out_size = 0;
	if (mismatches) *mismatches = 0;
	if (nblocks_out) *nblocks_out = 0;
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");

	/* Stream Header + Footer */
	static const uint8_t magic[6] = { 0xFD, '7', 'z', 'X', 'Z', 0x00 };
	uint8_t hf[24];
	if (xz_size < 32 || (xz_size & 3))
		FAILD(FORMAT_ERROR, "not an .xz Stream (size)");
	HIPD(xzk_d2h(hf, d_xz, 12, st) || xzk_d2h(hf + 12, d_xz + xz_size - 12, 12, st) || xzk_sync(st), "d2h stream flags");
	if (memcmp(hf, magic, 6) != 0 || hf[22] != 'Y' || hf[23] != 'Z')
		FAILD(FORMAT_ERROR, "bad magic bytes");
	if (rd32(hf + 8) != xzamd_crc32_host_(hf + 6, 2) || rd32(hf + 12) != xzamd_crc32_host_(hf + 16, 6))
		FAILD(XZAMD_DATA_ERROR, "Stream Header / Footer CRC32");
	if (hf[6] != 0 || (hf[7] & 0xF0) || hf[6] != hf[20] || hf[7] != hf[21])
		FAILD(XZAMD_OPTIONS_ERROR, "unsupported or inconsistent Stream Flags");
	const int check = hf[7] & 0x0F;
	/* a Check that cannot be verified is reported, not skipped (the reference: LZMA_UNSUPPORTED_CHECK) */
	if (check != XZAMD_CHECK_NONE && check != XZAMD_CHECK_CRC32 && check != XZAMD_CHECK_CRC64 && check != XZAMD_CHECK_SHA256)
		FAILD(XZAMD_UNSUPPORTED_CHECK, "Check id the device decoder cannot verify");
	static const uint8_t check_sizes[16] = { 0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64 };
	const uint32_t csz = check_sizes[check];
	const uint64_t index_size = ((uint64_t)rd32(hf + 16) + 1) * 4;
	if (index_size + 24 > xz_size)
		FAILD(XZAMD_DATA_ERROR, "Backward Size");

	/* Index */
	index = (uint8_t *)malloc(index_size);
	if (!index) FAILD(XZAMD_MEM_ERROR, "malloc");
	HIPD(xzk_d2h(index, d_xz + xz_size - 12 - index_size, index_size, st) || xzk_sync(st), "d2h index");
	if (index[0] != 0x00 || rd32(index + index_size - 4) != xzamd_crc32_host_(index, index_size - 4))
		FAILD(XZAMD_DATA_ERROR, "Index indicator / CRC32");
	uint64_t ip = 1;
	uint64_t nb = 0;
	if (xzb_vli(index, index_size - 4, &ip, &nb) || nb > (index_size / 2))
		FAILD(XZAMD_DATA_ERROR, "Index record count");
	hb = (xzamd_dec_block *)calloc(nb ? nb : 1, sizeof(*hb));
	stored32 = (uint8_t *)calloc(nb ? nb : 1, XZAMD_HDR_CHECK_BYTES);
	hc = (xzamd_dec_chain *)calloc(nb ? nb : 1, sizeof(*hc));
	if (!hb || !stored32 || !hc) FAILD(XZAMD_MEM_ERROR, "malloc");
	uint64_t pos = 12, utotal = 0;
	for (uint64_t b = 0; b < nb; ++b) {
		uint64_t unpadded = 0, usize = 0;
		if (xzb_vli(index, index_size - 4, &ip, &unpadded) || xzb_vli(index, index_size - 4, &ip, &usize)
				|| unpadded < 5 + csz || unpadded > (1ull << 62))
			FAILD(XZAMD_DATA_ERROR, "Index record");
		/* Block Header */
		uint8_t bh[1024];
		if (pos + 8 > xz_size - 12 - index_size)
			FAILD(XZAMD_DATA_ERROR, "Block beyond the Index");
		const uint64_t avail_h = xz_size - 12 - index_size - pos;
		HIPD(xzk_d2h(bh, d_xz + pos, avail_h < 64 ? avail_h : 64, st) || xzk_sync(st), "d2h block header");
		if (bh[0] == 0)
			FAILD(XZAMD_DATA_ERROR, "Index indicator where a Block Header was expected");
		const uint32_t hs = ((uint32_t)bh[0] + 1) * 4;
		if (hs > avail_h)
			FAILD(XZAMD_DATA_ERROR, "Block Header beyond the Index");
		if (hs > 64)
			HIPD(xzk_d2h(bh, d_xz + pos, hs, st) || xzk_sync(st), "d2h block header");
		uint64_t h_csize, h_usize;
		uint32_t dict = 0, step = 0;
		const uint32_t hcode = xzb_header(bh, hs, &h_csize, &h_usize, &hc[b], &dict, &step);
		if (hcode) FAILD((int)hcode, xzamd_block_step_msg_(step));
		if (unpadded < hs + csz)
			FAILD(XZAMD_DATA_ERROR, "Unpadded Size smaller than its header");
		const uint64_t csize = unpadded - hs - csz;
		if ((h_csize != UINT64_MAX && h_csize != csize) || (h_usize != UINT64_MAX && h_usize != usize) || csize == 0)
			FAILD(XZAMD_DATA_ERROR, "Block Header sizes differ from the Index");
		const uint64_t padded = (unpadded + 3) & ~3ull;
		if (pos + padded > xz_size - 12 - index_size)
			FAILD(XZAMD_DATA_ERROR, "Block beyond the Index");
		hb[b].cpos = pos + hs;
		hb[b].csize = csize;
		hb[b].upos = utotal;
		hb[b].usize = usize;
		hb[b].dict_size = dict;
		/* Block Padding must be zero; the stored Check */
		uint8_t tail[3 + 64];
		const uint32_t padn = (uint32_t)(padded - unpadded);
		HIPD(xzk_d2h(tail, d_xz + pos + hs + csize, padn + csz, st) || xzk_sync(st), "d2h check");
		for (uint32_t i = 0; i < padn; ++i)
			if (tail[i] != 0) FAILD(XZAMD_DATA_ERROR, "Block Padding");
		memcpy(stored32 + XZAMD_HDR_CHECK_BYTES * b, tail + padn, csz);
		pos += padded;
		utotal += usize;
		if (usize >= (1ull << 31) || csize >= (1ull << 32))
			FAILD(XZAMD_OPTIONS_ERROR, "Block too large for the device decoder");
	}
	for (; ip < index_size - 4; ++ip)
		if (index[ip] != 0) FAILD(XZAMD_DATA_ERROR, "Index Padding");
	if (pos != xz_size - 12 - index_size)
		FAILD(XZAMD_DATA_ERROR, "Blocks do not end where the Index starts");
	if (nblocks_out) *nblocks_out = nb;
	*out_size = utotal;
	if (utotal > out_cap)
		FAILD(XZAMD_BUF_ERROR, "output buffer too small");
	if (d_expected && expected_size != utotal)
		FAILD(XZAMD_DATA_ERROR, "the Stream's uncompressed size differs from the size of the original given for verification");
	/* Blocks of zero bytes still carry a chunk chain: they are decoded like any other */
	if (nb != 0) {
		const xzamd_dec_group group = { 0, nb, check };
		xzamd_dec_job job;
		memset(&job, 0, sizeof(job));
		job.d_xz = d_xz; job.d_out = d_out; job.d_expected = d_expected;
		job.nb = nb; job.hb = hb; job.hc = hc; job.stored = stored32;
		job.groups = &group; job.ngroups = 1;
		job.allow_split = 1;
		job.mismatches = mismatches;
		job.report = report;
		if (tab && tab->d_rec && tab->nrec && d_expected) {
			/* the kept table fits when the Stream has the Blocks of the encode it was kept from: as many, of the same sizes
			 * (the properties are the records' own; a chunk that carries others overrides them as in any decode) */
			int fits = nb == tab->nblocks && utotal == tab->in_size;
			for (uint64_t b = 0; fits && b < nb; ++b) {
				const uint64_t left = tab->in_size - b * tab->block_size;
				fits = hb[b].usize == (left < tab->block_size ? left : tab->block_size);
			}
			if (fits) { job.d_rec = tab->d_rec; job.rec_stride = tab->stride; job.nrec = tab->nrec; }
		}
		rc = xzamd_dec_run_(c, st, &job);
	}
done:
	xzk_sync(st);
	/* a defect of the container (nothing was decoded); a device or memory failure is no finding about the Stream */
	if ((rc == XZAMD_DATA_ERROR || rc == FORMAT_ERROR) && report && report->first_bad_step == XZAMD_VSTEP_NONE)
		report->first_bad_step = XZAMD_VSTEP_GRAMMAR;
	free(hc); free(stored32); free(index); free(hb);
	return rc;
}

int xzamd_stream_decode_device(xzamd_ctx *c, const void *d_xz_, uint64_t xz_size, void *d_out_, uint64_t out_cap,
		uint64_t *out_size, const void *d_expected_, uint64_t expected_size, uint64_t *mismatches, uint64_t *nblocks_out,
		void *stream)
{
	return stream_decode_(c, d_xz_, xz_size, d_out_, out_cap, out_size, d_expected_, expected_size, mismatches, nblocks_out,
			stream, NULL, NULL);
}

int xzamd_stream_verify_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size,
		xzamd_verify_report *report, void *stream)
{
	if (!c || !d_xz || (!d_original && original_size))
		return XZAMD_PROG_ERROR;
	xzamd_verify_report *rp = xzamd_ctx_report_(c);
	xzamd_resume_view tab;
	struct timespec t0, t1;
	void *d_tmp = NULL;
	uint64_t osz = 0, mm = 0, nbk = 0;
	int rc;
	clock_gettime(CLOCK_MONOTONIC, &t0);
	memset(rp, 0, sizeof(*rp));
	rp->first_bad_block = UINT64_MAX;
	xzamd_ctx_resume_(c, &tab);
	if (report) *report = *rp;
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	if (xzk_malloc(&d_tmp, original_size + 16))
		return xzamd_ctx_fail_(c, XZAMD_MEM_ERROR, "hipMalloc (verification output)");
	/* (an original of no bytes still needs a pointer for "this is a verification") */
	rc = stream_decode_(c, d_xz, xz_size, d_tmp, original_size, &osz, d_original ? d_original : d_tmp, original_size, &mm, &nbk,
			stream, &tab, rp);
	if (rc == XZAMD_BUF_ERROR) {
		rp->first_bad_step = XZAMD_VSTEP_COMPARE;
		rc = xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, "the Stream's uncompressed size differs from the size of the original");
	}
	xzk_free(d_tmp);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	rp->ms_verify = (float)((double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-6);
	if (report) *report = *rp;
	return rc;
}

int xzamd_verify_kept_(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size, void *stream)
{
	return xzamd_stream_verify_device(c, d_xz, xz_size, d_original, original_size, NULL, stream);
}

/* ---- per-Block verification (DESIGN.md 3.6 "Repair") ---- */

/* The framing of stream_decode_ without its Blocks: Stream Header, Footer, Index -> the Index records as the table the
 * Block Header kernel reads.  Same checks, same codes; what the Blocks themselves hold is the collecting run's business. */
int xzamd_stream_table_(xzamd_ctx *c, const uint8_t *d_xz, uint64_t xz_size, xzamd_hdr_rec **recs_out, uint64_t *nb_out, int *check_out,
		void *st)
{
	static const uint8_t magic[6] = { 0xFD, '7', 'z', 'X', 'Z', 0x00 };
	static const uint8_t check_sizes[16] = { 0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64 };
	int rc = XZAMD_OK;
	uint8_t hf[24];
	uint8_t *index = NULL;
	xzamd_hdr_rec *recs = NULL;
	*recs_out = NULL; *nb_out = 0; *check_out = 0;
	if (xz_size < 32 || (xz_size & 3))
		FAILD(FORMAT_ERROR, "not an .xz Stream (size)");
	HIPD(xzk_d2h(hf, d_xz, 12, st) || xzk_d2h(hf + 12, d_xz + xz_size - 12, 12, st) || xzk_sync(st), "d2h stream flags");
	if (memcmp(hf, magic, 6) != 0 || hf[22] != 'Y' || hf[23] != 'Z')
		FAILD(FORMAT_ERROR, "bad magic bytes");
	if (rd32(hf + 8) != xzamd_crc32_host_(hf + 6, 2) || rd32(hf + 12) != xzamd_crc32_host_(hf + 16, 6))
		FAILD(XZAMD_DATA_ERROR, "Stream Header / Footer CRC32");
	if (hf[6] != 0 || (hf[7] & 0xF0) || hf[6] != hf[20] || hf[7] != hf[21])
		FAILD(XZAMD_OPTIONS_ERROR, "unsupported or inconsistent Stream Flags");
	const int check = hf[7] & 0x0F;
	if (check != XZAMD_CHECK_NONE && check != XZAMD_CHECK_CRC32 && check != XZAMD_CHECK_CRC64 && check != XZAMD_CHECK_SHA256)
		FAILD(XZAMD_UNSUPPORTED_CHECK, "Check id the device decoder cannot verify");
	const uint32_t csz = check_sizes[check];
	const uint64_t index_size = ((uint64_t)rd32(hf + 16) + 1) * 4;
	if (index_size + 24 > xz_size)
		FAILD(XZAMD_DATA_ERROR, "Backward Size");
	const uint64_t index_at = xz_size - 12 - index_size;
	index = (uint8_t *)malloc(index_size);
	if (!index) FAILD(XZAMD_MEM_ERROR, "malloc");
	HIPD(xzk_d2h(index, d_xz + index_at, index_size, st) || xzk_sync(st), "d2h index");
	if (index[0] != 0x00 || rd32(index + index_size - 4) != xzamd_crc32_host_(index, index_size - 4))
		FAILD(XZAMD_DATA_ERROR, "Index indicator / CRC32");
	uint64_t ip = 1, nb = 0;
	if (xzb_vli(index, index_size - 4, &ip, &nb) || nb > (index_size / 2))
		FAILD(XZAMD_DATA_ERROR, "Index record count");
	if (nb >= (1ull << 31)) FAILD(XZAMD_OPTIONS_ERROR, "too many Blocks for the device decoder");
	recs = (xzamd_hdr_rec *)calloc(nb ? nb : 1, sizeof(*recs));
	if (!recs) FAILD(XZAMD_MEM_ERROR, "malloc");
	uint64_t pos = 12, utotal = 0;
	for (uint64_t b = 0; b < nb; ++b) {
		uint64_t unpadded = 0, usize = 0;
		if (xzb_vli(index, index_size - 4, &ip, &unpadded) || xzb_vli(index, index_size - 4, &ip, &usize)
				|| unpadded < 5 + csz || unpadded > (1ull << 62) || usize > (1ull << 62))
			FAILD(XZAMD_DATA_ERROR, "Index record");
		const uint64_t padded = (unpadded + 3) & ~3ull;
		if (padded > index_at - pos)
			FAILD(XZAMD_DATA_ERROR, "Block beyond the Index");
		recs[b].hpos = pos; recs[b].unpadded = unpadded; recs[b].usize = usize;
		recs[b].end = index_at; recs[b].upos = utotal; recs[b].csz = csz;
		pos += padded;
		utotal += usize;
	}
	for (; ip < index_size - 4; ++ip)
		if (index[ip] != 0) FAILD(XZAMD_DATA_ERROR, "Index Padding");
	if (pos != index_at)
		FAILD(XZAMD_DATA_ERROR, "Blocks do not end where the Index starts");
	*recs_out = recs; recs = NULL;
	*nb_out = nb; *check_out = check;
done:
	free(index); free(recs);
	return rc;
}

int xzamd_verify_table_(xzamd_ctx *c, const uint8_t *d_xz, uint64_t xz_size, const xzamd_hdr_rec *recs, uint64_t nb, int check,
		const uint8_t *d_original, uint64_t original_size, int mode, uint8_t *steps, xzamd_verify_report *rp, void *st)
{
	int rc = XZAMD_OK;
	void *d_recs = NULL, *d_table = NULL, *d_tmp = NULL;
	uint8_t *h_table = NULL;
	xzamd_dec_block *hb = NULL;
	xzamd_dec_chain *hc = NULL;
	uint8_t *stored = NULL;
	xzamd_dec_block *hb2 = NULL;     /* the second run: Blocks that failed with the original as history */
	xzamd_dec_chain *hc2 = NULL;
	uint8_t *stored2 = NULL, *steps2 = NULL;
	uint64_t utotal = 0;
	memset(steps, 0, nb);
	if (rp) rp->blocks = nb;
	if (nb == 0) return XZAMD_OK;
	for (uint64_t b = 0; b < nb; ++b) utotal += recs[b].usize;
	if (d_original && original_size != utotal) {
		if (rp && rp->first_bad_step == XZAMD_VSTEP_NONE) rp->first_bad_step = XZAMD_VSTEP_COMPARE;
		return xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, "the Stream's uncompressed size differs from the size of the original");
	}
	const uint64_t tbytes = XZAMD_HDR_TABLE_BYTES(nb);
	hb = (xzamd_dec_block *)calloc(nb, sizeof(*hb));
	hc = (xzamd_dec_chain *)calloc(nb, sizeof(*hc));
	stored = (uint8_t *)calloc(nb, XZAMD_HDR_CHECK_BYTES);
	h_table = (uint8_t *)malloc(tbytes);
	if (!hb || !hc || !stored || !h_table) FAILD(XZAMD_MEM_ERROR, "malloc");
	/* every Block Header, the sizes against the table, Block Padding, the stored Check: one thread per Block */
	HIPD(xzk_malloc(&d_recs, nb * sizeof(*recs)) || xzk_malloc(&d_table, tbytes), "hipMalloc");
	HIPD(xzk_h2d(d_recs, recs, nb * sizeof(*recs), st)
			|| xzk_dec_headers(d_xz, xz_size, (const xzamd_hdr_rec *)d_recs, (uint32_t)nb, d_table, st)
			|| xzk_d2h(h_table, d_table, tbytes, st) || xzk_sync(st), "Block Header kernel");
	{
		const uint8_t *p = h_table;
		memcpy(hb, p, nb * sizeof(*hb)); p += nb * sizeof(*hb);
		memcpy(hc, p, nb * sizeof(*hc)); p += nb * sizeof(*hc);
		memcpy(stored, p, nb * XZAMD_HDR_CHECK_BYTES); p += nb * XZAMD_HDR_CHECK_BYTES;
		const xzamd_hdr_err *he = (const xzamd_hdr_err *)p;
		for (uint64_t b = 0; b < nb; ++b) {
			if (!he[b].code) continue;
			/* a Block whose header cannot be read: the table still gives its extent and its uncompressed size.  It takes no
			 * part in the run (no chunk chain, no filters) */
			char buf[160];
			steps[b] = XZAMD_VSTEP_GRAMMAR;
			if (rp && rp->first_bad_step == XZAMD_VSTEP_NONE) {
				rp->first_bad_step = XZAMD_VSTEP_GRAMMAR;
				rp->first_bad_block = b;
				snprintf(buf, sizeof(buf), "Block %llu: %s", (unsigned long long)b, xzamd_block_step_msg_(he[b].step));
				(void)xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, buf);
			}
			hb[b].cpos = recs[b].hpos; hb[b].csize = 0; hb[b].upos = recs[b].upos; hb[b].usize = recs[b].usize;
			hb[b].dict_size = 0; hb[b].nunits = 0; hb[b].error = 0; hb[b].nrecs = 0;
			memset(&hc[b], 0, sizeof(hc[b]));
			if (recs[b].usize >= (1ull << 31)) FAILD(XZAMD_OPTIONS_ERROR, "Block too large for the device decoder");
		}
	}
	HIPD(xzk_malloc(&d_tmp, utotal + 16), "hipMalloc (verification output)");
	{
		const xzamd_dec_group group = { 0, nb, check };
		xzamd_dec_job job;
		xzamd_resume_view tab;
		memset(&job, 0, sizeof(job));
		job.d_xz = d_xz; job.d_out = (uint8_t *)d_tmp; job.d_expected = d_original;
		job.nb = nb; job.hb = hb; job.hc = hc; job.stored = stored;
		job.groups = &group; job.ngroups = 1;
		/* (the forward filters of the span-parallel history read the original in aligned words) */
		job.allow_split = ((uintptr_t)d_original & 15) == 0;
		job.report = rp;
		job.steps = steps;
		xzamd_ctx_resume_(c, &tab);
		if ((mode & XZAMD_VT_KEPT) && tab.d_rec && tab.nrec && d_original) {
			/* the kept table fits under the rule of xzamd_stream_verify_device */
			int fits = nb == tab.nblocks && utotal == tab.in_size;
			for (uint64_t b = 0; fits && b < nb; ++b) {
				const uint64_t left = tab.in_size - b * tab.block_size;
				fits = hb[b].usize == (left < tab.block_size ? left : tab.block_size);
			}
			if (fits) { job.d_rec = tab.d_rec; job.rec_stride = tab.stride; job.nrec = tab.nrec; }
		}
		rc = xzamd_dec_run_(c, st, &job);
		if (rc == XZAMD_DATA_ERROR && d_original && (mode & XZAMD_VT_PRECISE)) {
			/* The verdicts speak about the STREAM.  A verification unit reads its history from the original, so a wrong
			 * original makes a unit fail, or decode other bytes, as surely as wrong LZMA2 data does.  The Blocks that failed
			 * at "decode" or "check" go through once more on their own -- history = their own output, units at dictionary
			 * resets -- and that run decides: a sound Block of a Stream whose original differs ends at "compare". */
			uint64_t n2 = 0;
			for (uint64_t b = 0; b < nb; ++b) n2 += steps[b] == XZAMD_VSTEP_DECODE || steps[b] == XZAMD_VSTEP_CHECK;
			if (n2) {
				hb2 = (xzamd_dec_block *)calloc(n2, sizeof(*hb2));
				hc2 = (xzamd_dec_chain *)calloc(n2, sizeof(*hc2));
				stored2 = (uint8_t *)calloc(n2, XZAMD_HDR_CHECK_BYTES);
				steps2 = (uint8_t *)calloc(n2, 1);
				if (!hb2 || !hc2 || !stored2 || !steps2) FAILD(XZAMD_MEM_ERROR, "malloc");
			}
			/* one run of ADJACENT such Blocks per call: the Checks of a group of Blocks are taken over one stretch of the output */
			for (uint64_t b0 = 0; b0 < nb && n2; ) {
				if (steps[b0] != XZAMD_VSTEP_DECODE && steps[b0] != XZAMD_VSTEP_CHECK) { ++b0; continue; }
				uint64_t n = 0;
				while (b0 + n < nb && (steps[b0 + n] == XZAMD_VSTEP_DECODE || steps[b0 + n] == XZAMD_VSTEP_CHECK)) {
					hb2[n] = hb[b0 + n]; hb2[n].nunits = 0; hb2[n].error = 0; hb2[n].nrecs = 0;
					hc2[n] = hc[b0 + n];
					memcpy(stored2 + XZAMD_HDR_CHECK_BYTES * n, stored + XZAMD_HDR_CHECK_BYTES * (b0 + n), XZAMD_HDR_CHECK_BYTES);
					steps2[n] = XZAMD_VSTEP_NONE;
					++n;
				}
				const xzamd_dec_group group2 = { 0, n, check };
				xzamd_dec_job job2 = job;
				job2.nb = n; job2.hb = hb2; job2.hc = hc2; job2.stored = stored2; job2.groups = &group2;
				job2.d_rec = NULL; job2.nrec = 0; job2.plain_history = 1;
				job2.report = NULL; job2.steps = steps2;
				rc = xzamd_dec_run_(c, st, &job2);
				if (rc != XZAMD_OK && rc != XZAMD_DATA_ERROR) goto done;
				for (uint64_t i = 0; i < n; ++i) steps[b0 + i] = steps2[i];
				b0 += n;
			}
			rc = XZAMD_OK;
			for (uint64_t b = 0; b < nb; ++b) if (steps[b] != XZAMD_VSTEP_NONE) rc = XZAMD_DATA_ERROR;
			/* what a run that stops at the first defect reports: the steps in their order, the lowest Block of a step */
			static const char *const what[5] = { "", "container framing / LZMA2 chunk grammar", "LZMA2 data (range coder / distances / chunk sizes)",
				"Block Check mismatch", "decoded bytes differ from the original" };
			if (rp) { rp->first_bad_step = XZAMD_VSTEP_NONE; rp->first_bad_block = UINT64_MAX; }
			for (uint32_t v = XZAMD_VSTEP_GRAMMAR; v <= XZAMD_VSTEP_COMPARE && rc == XZAMD_DATA_ERROR; ++v) {
				uint64_t b = 0;
				while (b < nb && steps[b] != v) ++b;
				if (b == nb) continue;
				char buf[160];
				snprintf(buf, sizeof(buf), "Block %llu: %s", (unsigned long long)b, what[v]);
				(void)xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, buf);
				if (rp) { rp->first_bad_step = v; rp->first_bad_block = b; }
				break;
			}
		}
	}
done:
	xzk_sync(st);
	if (d_recs) xzk_free(d_recs);
	if (d_table) xzk_free(d_table);
	if (d_tmp) xzk_free(d_tmp);
	free(h_table); free(hb); free(hc); free(stored);
	free(hb2); free(hc2); free(stored2); free(steps2);
	return rc;
}

int xzamd_stream_verify_blocks_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size,
		uint8_t *block_steps, uint64_t steps_cap, uint64_t *nblocks, xzamd_verify_report *report, void *stream)
{
	if (!c || !d_xz || (!d_original && original_size) || (!block_steps && steps_cap))
		return XZAMD_PROG_ERROR;
	xzamd_verify_report *rp = xzamd_ctx_report_(c);
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	struct timespec t0, t1;
	xzamd_hdr_rec *recs = NULL;
	uint64_t nb = 0;
	int check = 0, rc;
	clock_gettime(CLOCK_MONOTONIC, &t0);
	memset(rp, 0, sizeof(*rp));
	rp->first_bad_block = UINT64_MAX;
	if (nblocks) *nblocks = 0;
	if (report) *report = *rp;
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	rc = xzamd_stream_table_(c, (const uint8_t *)d_xz, xz_size, &recs, &nb, &check, st);
	if (rc == XZAMD_OK) {
		if (nblocks) *nblocks = nb;
		if (nb > steps_cap) rc = xzamd_ctx_fail_(c, XZAMD_BUF_ERROR, "block_steps too small");
	}
	if (rc == XZAMD_OK)
		rc = xzamd_verify_table_(c, (const uint8_t *)d_xz, xz_size, recs, nb, check, (const uint8_t *)d_original, original_size,
				XZAMD_VT_KEPT | XZAMD_VT_PRECISE, block_steps, rp, st);
	/* a defect of the container: no Block to name */
	if ((rc == XZAMD_DATA_ERROR || rc == FORMAT_ERROR) && rp->first_bad_step == XZAMD_VSTEP_NONE)
		rp->first_bad_step = XZAMD_VSTEP_GRAMMAR;
	free(recs);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	rp->ms_verify = (float)((double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-6);
	if (report) *report = *rp;
	return rc;
}

void xzamd_get_verify_report(const xzamd_ctx *c, xzamd_verify_report *out)
{
	if (!c || !out) return;
	*out = *xzamd_ctx_report_((xzamd_ctx *)c);
}

int xzamd_debug_resume_peek_(xzamd_ctx *c, uint32_t record, uint32_t hdr_out[8], uint32_t *nrec_out)
{
	xzamd_resume_view tab;
	if (!c) return XZAMD_PROG_ERROR;
	xzamd_ctx_resume_(c, &tab);
	if (nrec_out) *nrec_out = tab.d_rec ? tab.nrec : 0;
	if (!hdr_out) return XZAMD_OK;
	if (!tab.d_rec || record >= tab.nrec) return XZAMD_PROG_ERROR;
	void *st = xzamd_ctx_stream_(c);
	if (xzk_set_device(xzamd_ctx_device(c))) return XZAMD_DEVICE_ERROR;
	if (xzk_d2h(hdr_out, tab.d_rec + (uint64_t)record * tab.stride, XZAMD_RESUME_HDR, st) || xzk_sync(st)) return XZAMD_DEVICE_ERROR;
	return XZAMD_OK;
}

int xzamd_debug_resume_poke_(xzamd_ctx *c, uint32_t record, int field, uint32_t value)
{
	xzamd_resume_view tab;
	if (!c) return XZAMD_PROG_ERROR;
	xzamd_ctx_resume_(c, &tab);
	if (!tab.d_rec || record >= tab.nrec || field < 0 || field > 3)
		return XZAMD_PROG_ERROR;
	void *st = xzamd_ctx_stream_(c);
	uint8_t *rec = tab.d_rec + (uint64_t)record * tab.stride;
	int e;
	if (xzk_set_device(xzamd_ctx_device(c))) return XZAMD_DEVICE_ERROR;
	if (field == 0) e = xzk_h2d(rec + 4, &value, 4, st);
	else if (field == 1) { const uint8_t k = (uint8_t)value; e = xzk_h2d(rec + XZAMD_RESUME_KIND_OFF, &k, 1, st); }
	else if (field == 2) e = xzk_h2d(rec + 12, &value, 4, st);
	else {
		const uint32_t n = (tab.stride - XZAMD_RESUME_HDR) / 2;
		uint16_t *flat = (uint16_t *)malloc(2ull * n);
		if (!flat) return XZAMD_MEM_ERROR;
		for (uint32_t i = 0; i < n; ++i) flat[i] = 1024;
		e = xzk_h2d(rec + XZAMD_RESUME_HDR, flat, 2ull * n, st);
		if (!e) e = xzk_sync(st);
		free(flat);
	}
	if (!e) e = xzk_sync(st);
	return e ? XZAMD_DEVICE_ERROR : XZAMD_OK;
}

