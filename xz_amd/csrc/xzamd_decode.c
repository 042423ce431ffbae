/*
 * xzamd_decode.c -- host side of the device .xz Stream decoder: the run over a Block table, and the
 * single-Stream entries (decode, verification, per-Block verdicts) that make one from a Stream.
 *
 * The container is read by xzamd_framing.c (Stream Header / Footer / Index -> one record per Block -> the Block table of
 * xzb_block, xzamd_block_parse.h).  xzamd_dec_run_ takes a table -- of one Stream here, of all Streams of a file in
 * xzamd_file.c -- through its stages:
 *   survey, history, scan   lzma/lzma2_decoder.c chunk grammar -> decode units (k_dec_scan)
 *   decode                  lzma/lzma_decoder.c (k_dec_units)
 *   inverse filters         simple/ and delta/delta_decoder.c, the last filter of the chain first (xzk_dec_unfilter)
 *   Checks                  check/crc32_fast.c, crc64_fast.c, sha256.c: the encoder's kernels over the decoded bytes
 *   comparison              with the original, when one is given (verification)
 * Scheduling model of common/stream_decoder_mt.c: independent Blocks in parallel; with the original data at hand every
 * state-resetting chunk chain is its own unit, and with the resume table an encode kept, every encode span.
 * Supported: the chains {LZMA2} and {up to three of: delta | x86 | PowerPC | IA-64 | ARM | ARM-Thumb | SPARC | ARM64 | RISC-V,
 * LZMA2}, which may differ from Block to Block; Checks none / CRC32 / CRC64 / SHA-256, all verified.  Declined with
 * XZAMD_OPTIONS_ERROR: a BCJ filter with a non-zero start offset, every other filter id, every chain the reference's
 * lzma_validate_chain refuses.
 *
 * Buffers of a run with filtered Blocks: the LZMA2 stage decodes into a temporary, each inverse stage reads one buffer and
 * writes another (a second temporary for chains of two or three filters), the last stage of a Block writes d_out.  A run
 * whose Blocks are all {LZMA2} allocates no temporary and launches no inverse stage.  Verification of filtered Blocks: the
 * history of the span-parallel units is the FILTERED original, made with the encoder's own forward kernels when the Blocks
 * form the geometry our encoder writes (equally long but the last, one chain); otherwise unit = Block.
 */
#include "xzamd_internal.h"
#include "kernels_api.h"

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

#define FAILD(code, msg) do { rc = xzamd_ctx_fail_(c, (code), (msg)); goto done; } while (0)
#define HIPD(call, msg) do { if (call) FAILD(XZAMD_DEVICE_ERROR, msg); } while (0)

/* A defect of Block b found by step `vstep` (XZAMD_VSTEP_*): XZAMD_DATA_ERROR, the message names the Block, and the report
 * (when there is one) keeps the first such defect */
static int fail_block_(xzamd_ctx *c, xzamd_verify_report *report, uint64_t b, uint32_t vstep, const char *msg)
{
	char buf[160];
	if (report && report->first_bad_step == XZAMD_VSTEP_NONE) {
		report->first_bad_step = vstep;
		report->first_bad_block = b;
	}
	if (b == UINT64_MAX) return xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, msg);
	snprintf(buf, sizeof(buf), "Block %llu: %s", (unsigned long long)b, msg);
	return xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, buf);
}

/* ---- the device part of a decode, in stages ---- */

/* The state of one run: the job, what the survey derives from it, the unit geometry, the host arrays and every device buffer */
typedef struct {
	xzamd_ctx *c;
	void *st;
	const xzamd_dec_job *j;
	uint32_t nbk;                   /* j->nb */
	uint64_t utotal, max_usize;
	uint32_t max_nf;                /* longest chain of filters in front of LZMA2 */
	int any_filtered, any_plain;
	int any_bad;                    /* collect mode: some Block is marked */
	int split;                      /* of xzk_dec_scan */
	uint32_t units_cap, total_units;
	uint32_t work;                  /* wavefronts' work items of the decode: units, or Blocks */
	uint8_t *dec_out;               /* where the LZMA2 stage writes: d_out, or t0 of a run with filtered Blocks */
	const uint8_t *hist_src;        /* history of the span-parallel units: the original, or its forward-filtered copy */
	uint64_t *h_crc;
	uint8_t *h_sha;
	uint32_t *unit_first, *h_err, *tile_first;
	void *d_blocks, *d_units, *d_first, *d_lit, *d_misc, *d_strip, *d_crc, *d_sha, *d_cmp;
	void *d_chains, *d_tiles, *d_t0, *d_t1, *d_filt, *d_tsum, *d_tcarry;
} dec_run;

static void run_free_(dec_run *r)
{
	void *const dev[] = { r->d_cmp, r->d_blocks, r->d_units, r->d_first, r->d_lit, r->d_misc, r->d_strip, r->d_crc, r->d_sha, r->d_chains,
		r->d_tiles, r->d_t0, r->d_t1, r->d_filt, r->d_tsum, r->d_tcarry };
	for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); ++i)
		if (dev[i]) xzk_free(dev[i]);
	free(r->tile_first); free(r->h_sha);
	free(r->h_crc); free(r->h_err); free(r->unit_first);
}

/* a failure of the call (device, memory, limits): the stage returns the code */
#define RUN_FAIL(r, code, msg) return xzamd_ctx_fail_((r)->c, (code), (msg))
#define RUN_DEV(r, call, msg) do { if (call) RUN_FAIL(r, XZAMD_DEVICE_ERROR, msg); } while (0)

static int is_bad_(const dec_run *r, uint64_t b) { return r->j->steps && r->j->steps[b] != XZAMD_VSTEP_NONE; }

/* A defect of Block b found by step `vstep`.  Returns non-zero when the run stops: the code.  In collect mode (j->steps) the
 * Block is marked, the message and the report keep the first defect, and the run goes on: 0. */
static int block_bad_(dec_run *r, uint64_t b, uint32_t vstep, const char *msg)
{
	const xzamd_dec_job *j = r->j;
	if (!j->steps) return fail_block_(r->c, j->report, b, vstep, msg);
	if (j->steps[b] == XZAMD_VSTEP_NONE) j->steps[b] = (uint8_t)vstep;
	if (!r->any_bad) (void)fail_block_(r->c, j->report, b, vstep, msg);
	r->any_bad = 1;
	return 0;
}

/* tile_first = exclusive prefix sum of the XZAMD_UNF_TILE tiles of the Blocks that take part: every Block that is not marked
 * (stage < 0), or those of them with an inverse stage `stage`, whose kinds of work go to *kinds.  Returns the total. */
static uint64_t tile_prefix_(dec_run *r, int stage, uint32_t *kinds)
{
	const xzamd_dec_job *j = r->j;
	uint64_t tiles = 0;
	for (uint64_t b = 0; b < j->nb; ++b) {
		const xzamd_dec_chain *ch = &j->hc[b];
		r->tile_first[b] = (uint32_t)tiles;
		if (is_bad_(r, b)) continue;
		if (stage >= 0) {
			if (!(ch->n > (uint32_t)stage || (ch->n == 0 && stage == 0))) continue;
			const uint32_t kind = ch->n ? ch->f[ch->n - 1 - stage] & 0xFFu : 0u;
			if (j->hb[b].usize)
				*kinds |= kind == 3u ? XZAMD_UNF_DELTA : kind ? XZAMD_UNF_COPY | XZAMD_UNF_BCJ : XZAMD_UNF_COPY;
		}
		tiles += (j->hb[b].usize + XZAMD_UNF_TILE - 1) / XZAMD_UNF_TILE;
	}
	r->tile_first[j->nb] = (uint32_t)tiles;
	return tiles;
}

/* survey: sizes, kinds of Blocks, Blocks marked on entry; the host arrays; the unit geometry the job asks for.
 * Units: with the original (verification) at every state reset that carries the properties; without it at every dictionary
 * reset -- nothing in front of one can be referenced, so the units of a Block decode side by side with the output itself as
 * history.  The unit count of a Block is data: the table holds usize / 4096 + 8 per Block, and in the plain mode a Block with
 * more resets keeps the rest inside its last unit. */
static int run_survey_(dec_run *r)
{
	const xzamd_dec_job *j = r->j;
	const uint64_t nb = j->nb;
	for (uint64_t b = 0; b < nb; ++b) {
		if (is_bad_(r, b)) r->any_bad = 1;        /* (marked by the caller, who has reported it) */
		if (j->hc[b].n) { r->any_filtered = 1; if (j->hc[b].n > r->max_nf) r->max_nf = j->hc[b].n; } else r->any_plain = 1;
		r->utotal += j->hb[b].usize;
		if (j->hb[b].usize > r->max_usize) r->max_usize = j->hb[b].usize;
	}
	r->h_crc = (uint64_t *)calloc(nb, 8);
	r->h_err = (uint32_t *)calloc(nb, 4);
	r->unit_first = (uint32_t *)calloc(nb + 1, 4);
	r->tile_first = (uint32_t *)calloc(nb + 1, 4);
	if (!r->h_crc || !r->h_err || !r->unit_first || !r->tile_first) RUN_FAIL(r, XZAMD_MEM_ERROR, "malloc");
	const int verif = j->d_expected != NULL && !j->plain_history;      /* the units read their history from the original */
	const int with_table = verif && j->allow_split && j->d_rec != NULL && j->nrec != 0;
	r->split = verif ? (j->allow_split ? (with_table ? 3 : 1) : 0) : 2;
	r->units_cap = r->split ? (uint32_t)(r->max_usize / 4096 + 8) : 1;
	if ((uint64_t)r->units_cap * nb > (1ull << 27)) { r->split = 0; r->units_cap = 1; }
	r->dec_out = j->d_out;
	r->hist_src = j->d_expected;
	return 0;
}

/* history: the temporaries of a run with filtered Blocks -- the LZMA2 stage of every Block decodes into t0 (one kernel, one
 * output base); a second temporary only for chains of two or three filters -- and, for span-parallel units, their history. */
static int run_history_(dec_run *r)
{
	const xzamd_dec_job *j = r->j;
	const uint64_t nb = j->nb;
	if (!r->any_filtered) return 0;
	RUN_DEV(r, xzk_malloc(&r->d_t0, r->utotal + 16), "hipMalloc");
	count_(0);
	if (r->max_nf >= 2) { RUN_DEV(r, xzk_malloc(&r->d_t1, r->utotal + 16), "hipMalloc"); count_(0); }
	RUN_DEV(r, xzk_malloc(&r->d_chains, nb * sizeof(xzamd_dec_chain)) || xzk_malloc(&r->d_tiles, 4 * (nb + 1)), "hipMalloc");
	RUN_DEV(r, xzk_h2d(r->d_chains, j->hc, nb * sizeof(xzamd_dec_chain), r->st), "h2d chains");
	r->dec_out = (uint8_t *)r->d_t0;
	if (r->split != 1 && r->split != 3) return 0;
	/* The history of a span-parallel unit is what the LZMA2 encoder saw: the filtered original.  Make it with the
	 * encoder's forward kernels when the Stream has the geometry they filter (Blocks equally long but the last,
	 * one chain, < 2 GiB); any other Stream: unit = Block. */
	const uint64_t bs0 = j->hb[0].usize;
	int same = !r->any_plain && bs0 != 0 && r->utotal < (1ull << 31) && j->hb[nb - 1].usize <= bs0;
	for (uint64_t b = 0; same && b < nb; ++b)
		same = memcmp(&j->hc[b], &j->hc[0], sizeof(j->hc[0])) == 0 && (b + 1 == nb || j->hb[b].usize == bs0);
	if (!same) { r->split = 0; r->units_cap = 1; return 0; }
	RUN_DEV(r, xzk_malloc(&r->d_filt, r->utotal + 16), "hipMalloc");
	count_(0);
	const uint32_t nf = j->hc[0].n;
	const uint8_t *src = j->d_expected;
	for (uint32_t i = 0; i < nf; ++i) {
		/* in -> F, in -> t0 -> F, in -> F -> t0 -> F: no step in place; t0 is free until the decode */
		uint8_t *dst = ((nf - 1 - i) & 1) ? (uint8_t *)r->d_t0 : (uint8_t *)r->d_filt;
		const uint32_t f = j->hc[0].f[i];
		RUN_DEV(r, f == 4u ? xzk_x86_bcj(src, dst, (uint32_t)r->utotal, (uint32_t)bs0, r->nbk, r->st)
				: xzk_prefilter(src, dst, (uint32_t)r->utotal, (uint32_t)bs0, r->nbk, f & 0xFFu, (f >> 8) + 1, r->st),
				"forward filter of the verification decode");
		launches_(j, 1);
		count_(2);
		src = dst;
	}
	r->hist_src = (const uint8_t *)r->d_filt;
	return 0;
}

/* scan: the units of every Block (k_dec_scan) -> unit_first, total_units, the report, dec_last_units.  A Block with more state
 * resets than the table anticipates sends every Block through a second pass, one unit per Block (compared afterwards all the
 * same; in collect mode the Blocks the first pass marked stay marked -- their defect does not depend on the split). */
/* (the scan of bare chains is referred to weakly: a build of this unit over a kernel layer without it has no chain jobs) */
extern int xzk_dec_scan_chains(const uint8_t *d_chains, xzamd_dec_block *d_blocks, uint32_t nchains, xzamd_dec_unit *d_units,
		uint32_t units_cap, int split, const uint8_t *d_rec, uint32_t rec_stride, uint32_t nrec, void *stream) __attribute__((weak));

static int run_scan_(dec_run *r)
{
	const xzamd_dec_job *j = r->j;
	const uint64_t nb = j->nb;
	xzamd_dec_block *hb = j->hb;
	uint64_t recs_used = 0;
	int rc;
	if (j->chains && !xzk_dec_scan_chains) RUN_FAIL(r, XZAMD_OPTIONS_ERROR, "this build has no scan of bare chunk chains");
	RUN_DEV(r, xzk_malloc(&r->d_blocks, nb * sizeof(xzamd_dec_block)) || xzk_malloc(&r->d_misc, 4096 + 4 * nb)
			|| xzk_malloc(&r->d_first, 4 * (nb + 1)), "hipMalloc");
	for (int pass = 0; ; ++pass) {
		int overflow = 0;
		RUN_DEV(r, xzk_malloc(&r->d_units, (uint64_t)r->units_cap * nb * sizeof(xzamd_dec_unit)), "hipMalloc");
		RUN_DEV(r, xzk_h2d(r->d_blocks, hb, nb * sizeof(xzamd_dec_block), r->st), "h2d blocks");
		RUN_DEV(r, (j->chains ? xzk_dec_scan_chains : xzk_dec_scan)(j->d_xz, (xzamd_dec_block *)r->d_blocks, r->nbk,
				(xzamd_dec_unit *)r->d_units, r->units_cap, r->split, r->split == 3 ? j->d_rec : NULL, j->rec_stride, j->nrec, r->st),
				"scan launch");
		launches_(j, 1);
		RUN_DEV(r, xzk_d2h(hb, r->d_blocks, nb * sizeof(xzamd_dec_block), r->st) || xzk_sync(r->st), "d2h blocks");
		reads_(j, 1);
		r->total_units = 0;
		recs_used = 0;
		for (uint64_t b = 0; b < nb; ++b) {
			rc = 0;
			if (!is_bad_(r, b)) {                     /* (bad already: its header -- the Block has no chunk chain to speak of) */
				if (hb[b].error == 11) overflow = 1;
				else if (hb[b].error == 13)
					rc = block_bad_(r, b, XZAMD_VSTEP_GRAMMAR, "a resume record names a span start that is no LZMA2 chunk start");
				else if (hb[b].error) rc = block_bad_(r, b, XZAMD_VSTEP_GRAMMAR, "LZMA2 chunk grammar");
			}
			if (rc) return rc;
			if (is_bad_(r, b)) hb[b].nunits = 0;      /* out of the decode: its units are not listed */
			r->unit_first[b] = r->total_units;
			r->total_units += hb[b].nunits;
			recs_used += hb[b].nrecs;
		}
		r->unit_first[nb] = r->total_units;
		if (!overflow) break;
		if (pass) RUN_FAIL(r, XZAMD_PROG_ERROR, "unit table overflow with one unit per Block");
		xzk_free(r->d_units); r->d_units = NULL;
		for (uint64_t b = 0; b < nb; ++b) { hb[b].error = 0; hb[b].nunits = 0; }
		r->split = 0; r->units_cap = 1;
	}
	r->work = r->split ? r->total_units : r->nbk;
	if (j->report) {
		j->report->units = r->work;
		j->report->blocks = nb;
		j->report->table_used = r->split == 3;
		j->report->records_used = r->split == 3 ? recs_used : 0;
	}
	__atomic_store_n(&dec_last_units[0], r->work, __ATOMIC_RELAXED);
	__atomic_store_n(&dec_last_units[1], nb, __ATOMIC_RELAXED);
	__atomic_store_n(&dec_last_units[2], (uint64_t)r->split, __ATOMIC_RELAXED);
	return 0;
}

/* d_misc: [0] the work counter of the persistent decode, [64] the global count of mismatching words, [4096 ...] one error word
 * per Block */
static unsigned long long *misc_mismatches_(const dec_run *r) { return (unsigned long long *)((uint8_t *)r->d_misc + 64); }

/* decode: the LZMA2 stage of every unit */
static int run_decode_(dec_run *r)
{
	const xzamd_dec_job *j = r->j;
	const uint64_t nb = j->nb;
	const int by_rec = r->split == 3;
	const uint8_t *hist = r->split == 1 || by_rec ? r->hist_src : NULL;
	uint32_t *d_berr = (uint32_t *)((uint8_t *)r->d_misc + 4096);
	uint32_t waves = xzamd_ctx_wave_slots_(r->c);
	int rc;
	if (waves > r->work) waves = r->work ? r->work : 1;
	RUN_DEV(r, xzk_malloc(&r->d_lit, (uint64_t)waves * (0x300ull << 4) * 2), "hipMalloc");
	RUN_DEV(r, xzk_memset(r->d_misc, 0, 4096 + 4 * nb, r->st), "memset");
	RUN_DEV(r, xzk_h2d(r->d_first, r->unit_first, 4 * (nb + 1), r->st), "h2d");
	RUN_DEV(r, xzk_dec_units(j->d_xz, (const xzamd_dec_block *)r->d_blocks, r->nbk, (const xzamd_dec_unit *)r->d_units, r->units_cap,
			(const uint32_t *)r->d_first, r->total_units, r->dec_out, hist, (uint16_t *)r->d_lit, waves, (uint32_t *)r->d_misc, d_berr,
			r->split == 2, by_rec ? j->d_rec : NULL, j->rec_stride, r->st), "decode launch");
	launches_(j, 1);
	RUN_DEV(r, xzk_d2h(r->h_err, d_berr, 4 * nb, r->st) || xzk_sync(r->st), "decode");
	reads_(j, 1);
	for (uint64_t b = 0; b < nb; ++b)
		if (r->h_err[b] && !is_bad_(r, b)
				&& (rc = block_bad_(r, b, XZAMD_VSTEP_DECODE, "LZMA2 data (range coder / distances / chunk sizes)")) != 0)
			return rc;
	return 0;
}

/* inverse filters: one stage after another, the filter next to LZMA2 first; an unfiltered Block of a mixed Stream is copied
 * in stage 0 */
static int run_unfilter_(dec_run *r)
{
	const xzamd_dec_job *j = r->j;
	const uint64_t nb = j->nb;
	xzamd_unf_args ua;
	if (!r->any_filtered) return 0;
	memset(&ua, 0, sizeof(ua));
	ua.blocks = (const xzamd_dec_block *)r->d_blocks;
	ua.chains = (const xzamd_dec_chain *)r->d_chains;
	ua.tile_first = (const uint32_t *)r->d_tiles;
	ua.nblocks = r->nbk;
	ua.t0 = (uint8_t *)r->d_t0; ua.t1 = (uint8_t *)r->d_t1; ua.out = j->d_out;
	for (uint32_t k = 0; k < r->max_nf; ++k) {
		uint32_t kinds = 0;
		const uint64_t tiles = tile_prefix_(r, (int)k, &kinds);
		if (tiles >= (1ull << 31)) RUN_FAIL(r, XZAMD_OPTIONS_ERROR, "Stream too large for the inverse filters");
		if (tiles == 0) continue;
		if ((kinds & XZAMD_UNF_DELTA) && !r->d_tsum) {
			/* every later stage covers a subset of this stage's Blocks: its tiles fit */
			RUN_DEV(r, xzk_malloc(&r->d_tsum, tiles * XZAMD_UNF_ROW) || xzk_malloc(&r->d_tcarry, tiles * XZAMD_UNF_ROW), "hipMalloc");
		}
		ua.tile_sum = (uint8_t *)r->d_tsum; ua.tile_carry = (uint8_t *)r->d_tcarry;
		ua.stage = k;
		/* tile_first is rewritten for the next stage: the copy must have left the host buffer first */
		RUN_DEV(r, xzk_h2d(r->d_tiles, r->tile_first, 4 * (nb + 1), r->st) || xzk_sync(r->st), "h2d tiles");
		RUN_DEV(r, xzk_dec_unfilter(&ua, (uint32_t)tiles, kinds, r->st), "inverse filter launch");
		launches_(j, 1);
		count_(1);
	}
	return 0;
}

static int is_crc_(int check) { return check == XZAMD_CHECK_CRC32 || check == XZAMD_CHECK_CRC64; }

/* the Check of nblocks Blocks of block_size bytes (but the last) at `in`, n bytes in all; `first`: the job's index of the first */
static int check_launch_(dec_run *r, int check, uint64_t first, const uint8_t *in, uint64_t n, uint64_t block_size, uint64_t nblocks)
{
	RUN_DEV(r, is_crc_(check) ? xzk_crc_blocks(in, (uint32_t)n, (uint32_t)block_size, (uint32_t)nblocks, 4096, check == XZAMD_CHECK_CRC32,
					(uint64_t *)r->d_strip, (uint64_t *)r->d_crc + first, r->st)
			/* check/sha256.c over the decoded bytes: one hash per Block (serial by nature) */
			: xzk_sha256_blocks(in, (uint32_t)n, (uint32_t)block_size, (uint32_t)nblocks, (uint8_t *)r->d_sha + 32 * first, r->st),
			"Check launch");
	launches_(r->j, 1);
	return 0;
}

/* The Checks of a group.  Equally long Blocks but the last: one launch for the group, else one launch per Block. */
static int group_launch_(dec_run *r, const xzamd_dec_group *g)
{
	const xzamd_dec_block *gb = r->j->hb + g->first;
	const uint64_t gn = g->count;
	const int crc = is_crc_(g->check);
	int uniform = 1, rc;
	uint64_t gtotal = 0;
	for (uint64_t b = 0; b < gn; ++b) gtotal += gb[b].usize;
	for (uint64_t b = 0; b + 1 < gn; ++b)
		if (gb[b].usize != gb[0].usize) uniform = 0;
	if (gn > 1 && gb[gn - 1].usize > gb[0].usize) uniform = 0;
	if (uniform && gtotal < (1ull << 31) && (crc || gb[0].usize))
		return check_launch_(r, g->check, g->first, r->j->d_out + gb[0].upos, gtotal, gb[0].usize ? gb[0].usize : 1, gn);
	for (uint64_t b = 0; b < gn; ++b) {
		if (crc && gb[b].usize == 0) { RUN_DEV(r, xzk_memset((uint64_t *)r->d_crc + g->first + b, 0, 8, r->st), "memset"); continue; }
		if ((rc = check_launch_(r, g->check, g->first + b, r->j->d_out + gb[b].upos, gb[b].usize, gb[b].usize ? gb[b].usize : 1, 1)) != 0)
			return rc;
	}
	return 0;
}

/* Checks over the decoded bytes, one group of Blocks (= the Blocks of one Stream, one kind of Check) after another; the
 * results of all groups come back in one read per kind and are compared with the stored bytes */
static int run_checks_(dec_run *r)
{
	const xzamd_dec_job *j = r->j;
	const uint64_t nb = j->nb;
	int any_crc = 0, any_sha = 0, rc;
	for (uint32_t g = 0; g < j->ngroups; ++g) {
		if (j->groups[g].count == 0) continue;
		if (is_crc_(j->groups[g].check)) any_crc = 1;
		if (j->groups[g].check == XZAMD_CHECK_SHA256) any_sha = 1;
	}
	if (any_crc) {
		const uint64_t spb = (r->max_usize + 4096 - 1) / 4096 + 1;
		RUN_DEV(r, xzk_malloc(&r->d_strip, 8 * spb * nb + 64) || xzk_malloc(&r->d_crc, 8 * nb + 64), "hipMalloc");
	}
	if (any_sha) {
		RUN_DEV(r, xzk_malloc(&r->d_sha, 32 * nb + 64), "hipMalloc");
		r->h_sha = (uint8_t *)malloc(32 * nb);
		if (!r->h_sha) RUN_FAIL(r, XZAMD_MEM_ERROR, "malloc");
	}
	for (uint32_t g = 0; g < j->ngroups; ++g)
		if (j->groups[g].count != 0 && j->groups[g].check != XZAMD_CHECK_NONE && (rc = group_launch_(r, &j->groups[g])) != 0)
			return rc;
	if (any_crc) { RUN_DEV(r, xzk_d2h(r->h_crc, r->d_crc, 8 * nb, r->st), "d2h crc"); reads_(j, 1); }
	if (any_sha) { RUN_DEV(r, xzk_d2h(r->h_sha, r->d_sha, 32 * nb, r->st), "d2h sha256"); reads_(j, 1); }
	if (any_crc || any_sha) RUN_DEV(r, xzk_sync(r->st), "d2h checks");
	for (uint32_t g = 0; g < j->ngroups; ++g) {
		const int check = j->groups[g].check;
		for (uint64_t b = j->groups[g].first; b < j->groups[g].first + j->groups[g].count; ++b) {
			const uint8_t *sb = j->stored + XZAMD_HDR_CHECK_BYTES * b;
			int differs = 0;
			if (is_bad_(r, b)) continue;
			if (is_crc_(check)) {
				uint64_t sv = 0;
				for (uint32_t i = 0; i < (check == XZAMD_CHECK_CRC32 ? 4u : 8u); ++i) sv |= (uint64_t)sb[i] << (8 * i);
				differs = r->h_crc[b] != sv;
			} else if (check == XZAMD_CHECK_SHA256) {
				differs = memcmp(r->h_sha + 32 * b, sb, 32) != 0;
			}
			if (differs && (rc = block_bad_(r, b, XZAMD_VSTEP_CHECK, is_crc_(check) ? "Block Check mismatch" : "Block Check mismatch (SHA-256)")) != 0)
				return rc;
		}
	}
	return 0;
}

/* comparison with the original.  Collect mode: one count of differing bytes per Block that got this far
 * (k_dec_compare_blocks), and the global word count of the plain path only when that path would have reached its comparison. */
static int run_compare_(dec_run *r)
{
	const xzamd_dec_job *j = r->j;
	const uint64_t nb = j->nb;
	unsigned long long mm = 0;
	unsigned long long *h_cnt = (unsigned long long *)r->h_crc;      /* (the Checks have been looked at) */
	int rc;
	if (!j->d_expected) return 0;
	if (j->steps) {
		const uint64_t tiles = tile_prefix_(r, -1, NULL);
		if (tiles >= (1ull << 31)) RUN_FAIL(r, XZAMD_OPTIONS_ERROR, "Stream too large for the per-Block comparison");
		RUN_DEV(r, xzk_malloc(&r->d_cmp, 12 * nb + 16), "hipMalloc");
		uint32_t *d_tf = (uint32_t *)((uint8_t *)r->d_cmp + 8 * nb);
		RUN_DEV(r, xzk_memset(r->d_cmp, 0, 8 * nb, r->st) || xzk_h2d(d_tf, r->tile_first, 4 * (nb + 1), r->st), "h2d tiles");
		RUN_DEV(r, xzk_dec_compare_blocks(j->d_out, j->d_expected, (const xzamd_dec_block *)r->d_blocks, d_tf, r->nbk, (uint32_t)tiles,
				(unsigned long long *)r->d_cmp, r->st), "compare launch");
		launches_(j, 1);
	}
	if (!j->steps || !r->any_bad) {
		RUN_DEV(r, xzk_dec_compare(j->d_out, j->d_expected, r->utotal, misc_mismatches_(r), r->st), "compare launch");
		launches_(j, 1);
	}
	RUN_DEV(r, (j->steps && xzk_d2h(h_cnt, r->d_cmp, 8 * nb, r->st)) || xzk_d2h(&mm, misc_mismatches_(r), 8, r->st) || xzk_sync(r->st),
			"d2h compare");
	reads_(j, 1);
	if (j->mismatches) *j->mismatches = mm;
	if (j->report) j->report->mismatching_words = mm;
	if (!j->steps)
		return mm ? fail_block_(r->c, j->report, UINT64_MAX, XZAMD_VSTEP_COMPARE, "decoded bytes differ from the original") : 0;
	for (uint64_t b = 0; b < nb; ++b)
		if (!is_bad_(r, b) && h_cnt[b] && (rc = block_bad_(r, b, XZAMD_VSTEP_COMPARE, "decoded bytes differ from the original")) != 0)
			return rc;
	return 0;
}

/* The device part of a decode: the Blocks of j->hb (parsed and validated: xzb_block) through unit scan, LZMA2 decode,
 * inverse filters, Checks (per group of Blocks = per Stream) and the comparison with the original. */
int xzamd_dec_run_(xzamd_ctx *c, void *st, const xzamd_dec_job *j)
{
	static int (*const stages[])(dec_run *) = { run_survey_, run_history_, run_scan_, run_decode_, run_unfilter_, run_checks_, run_compare_ };
	dec_run r;
	int rc = XZAMD_OK;
	if (j->report) j->report->blocks = j->nb;
	if (j->nb == 0) return XZAMD_OK;
	if (j->nb >= (1ull << 31)) return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR, "too many Blocks for the device decoder");
	memset(&r, 0, sizeof(r));
	r.c = c; r.st = st; r.j = j; r.nbk = (uint32_t)j->nb;
	for (size_t i = 0; i < sizeof(stages) / sizeof(stages[0]) && rc == XZAMD_OK; ++i) rc = stages[i](&r);
	if (rc == XZAMD_OK && r.any_bad) rc = XZAMD_DATA_ERROR;     /* (message and report: the first defect, set when it was marked) */
	xzk_sync(st);
	run_free_(&r);
	return rc;
}

/* The kept resume table fits when the Stream has the Blocks of the encode it was kept from: as many, of the same sizes (the
 * properties are the records' own; a chunk that carries others overrides them as in any decode).  Then the job gets it. */
static void job_take_table_(xzamd_dec_job *job, const xzamd_resume_view *tab, uint64_t utotal)
{
	if (!tab->d_rec || !tab->nrec || !job->d_expected) return;
	int fits = job->nb == tab->nblocks && utotal == tab->in_size;
	for (uint64_t b = 0; fits && b < job->nb; ++b) {
		const uint64_t left = tab->in_size - b * tab->block_size;
		fits = job->hb[b].usize == (left < tab->block_size ? left : tab->block_size);
	}
	if (fits) { job->d_rec = tab->d_rec; job->rec_stride = tab->stride; job->nrec = tab->nrec; }
}

/* xzamd_stream_decode_device; `tab` / `report` (both optional): the verification of xzamd_stream_verify_device.
 * Stream framing -> Index records -> Block table (the first bad Block decides the code) -> one job of one group. */
static int stream_decode_(xzamd_ctx *c, const void *d_xz_, uint64_t xz_size, void *d_out_, uint64_t out_cap,
		uint64_t *out_size, const void *d_expected_, uint64_t expected_size, uint64_t *mismatches, uint64_t *nblocks_out,
		void *stream, const xzamd_resume_view *tab, xzamd_verify_report *report)
{
	if (!c || !d_xz_ || !out_size || (!d_out_ && out_cap))
		return XZAMD_PROG_ERROR;
	const uint8_t *d_expected = (const uint8_t *)d_expected_;
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	xzamd_src s = { NULL, (const uint8_t *)d_xz_, st, xz_size, 0 };
	xzamd_hdr_rec *recs = NULL;
	xzamd_blocks B = { NULL, NULL, NULL, NULL };
	const char *msg = "";
	uint64_t nb = 0, utotal = 0;
	int check = 0, rc;
	*out_size = 0;
	if (mismatches) *mismatches = 0;
	if (nblocks_out) *nblocks_out = 0;
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	/* (this entry leaves an Uncompressed Size of the Index to the Block's own checks, whatever it is) */
	rc = xzamd_stream_walk_(&s, UINT64_MAX, &recs, &nb, &check, &msg);
	if (!rc) rc = xzamd_block_table_(&s, recs, nb, &B, NULL, &msg);
	if (!rc) rc = xzamd_blocks_first_bad_(&B, nb, &msg);
	if (rc) FAILD(rc, msg);
	for (uint64_t b = 0; b < nb; ++b) utotal += recs[b].usize;
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
		job.d_xz = s.dev; job.d_out = (uint8_t *)d_out_; job.d_expected = d_expected;
		job.nb = nb; job.hb = B.hb; job.hc = B.hc; job.stored = B.stored;
		job.groups = &group; job.ngroups = 1;
		job.allow_split = 1;
		job.mismatches = mismatches;
		job.report = report;
		if (tab) job_take_table_(&job, tab, utotal);
		rc = xzamd_dec_run_(c, st, &job);
	}
done:
	xzk_sync(st);
	/* a defect of the container (nothing was decoded); a device or memory failure is no finding about the Stream */
	if ((rc == XZAMD_DATA_ERROR || rc == FORMAT_ERROR) && report && report->first_bad_step == XZAMD_VSTEP_NONE)
		report->first_bad_step = XZAMD_VSTEP_GRAMMAR;
	xzamd_blocks_free_(&B);
	free(recs);
	return rc;
}

int xzamd_stream_decode_device(xzamd_ctx *c, const void *d_xz_, uint64_t xz_size, void *d_out_, uint64_t out_cap,
		uint64_t *out_size, const void *d_expected_, uint64_t expected_size, uint64_t *mismatches, uint64_t *nblocks_out,
		void *stream)
{
	return stream_decode_(c, d_xz_, xz_size, d_out_, out_cap, out_size, d_expected_, expected_size, mismatches, nblocks_out,
			stream, NULL, NULL);
}

/* What the verifying entries share: the context's report, cleared (and copied out, for a call that fails early), and the clock */
static xzamd_verify_report *verify_begin_(xzamd_ctx *c, xzamd_verify_report *report, struct timespec *t0)
{
	xzamd_verify_report *rp = xzamd_ctx_report_(c);
	clock_gettime(CLOCK_MONOTONIC, t0);
	memset(rp, 0, sizeof(*rp));
	rp->first_bad_block = UINT64_MAX;
	if (report) *report = *rp;
	return rp;
}
static int verify_end_(xzamd_verify_report *rp, xzamd_verify_report *report, const struct timespec *t0, int rc)
{
	struct timespec t1;
	clock_gettime(CLOCK_MONOTONIC, &t1);
	rp->ms_verify = (float)((double)(t1.tv_sec - t0->tv_sec) * 1e3 + (double)(t1.tv_nsec - t0->tv_nsec) * 1e-6);
	if (report) *report = *rp;
	return rc;
}

int xzamd_stream_verify_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size,
		xzamd_verify_report *report, void *stream)
{
	if (!c || !d_xz || (!d_original && original_size))
		return XZAMD_PROG_ERROR;
	struct timespec t0;
	xzamd_verify_report *rp = verify_begin_(c, report, &t0);
	xzamd_resume_view tab;
	void *d_tmp = NULL;
	uint64_t osz = 0, mm = 0, nbk = 0;
	int rc;
	xzamd_ctx_resume_(c, &tab);
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
	return verify_end_(rp, report, &t0, rc);
}

int xzamd_verify_kept_(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size, void *stream)
{
	return xzamd_stream_verify_device(c, d_xz, xz_size, d_original, original_size, NULL, stream);
}

/* ---- per-Block verification (DESIGN.md 3.6 "Repair") ---- */

static int step_is_retried_(uint8_t step) { return step == XZAMD_VSTEP_DECODE || step == XZAMD_VSTEP_CHECK; }

/* XZAMD_VT_PRECISE.  The verdicts speak about the STREAM.  A verification unit reads its history from the original, so a
 * wrong original makes a unit fail, or decode other bytes, as surely as wrong LZMA2 data does.  The Blocks of `job` that
 * failed at "decode" or "check" go through once more on their own -- history = their own output, units at dictionary resets
 * -- and that run decides: a sound Block of a Stream whose original differs ends at "compare".  Rewrites steps, the message
 * and the report's first defect; returns the code of the verification. */
static int verify_again_(xzamd_ctx *c, void *st, const xzamd_dec_job *job, uint8_t *steps, xzamd_verify_report *rp)
{
	const uint64_t nb = job->nb;
	const int check = job->groups[0].check;
	int rc = XZAMD_OK;
	uint64_t n2 = 0;
	for (uint64_t b = 0; b < nb; ++b) n2 += step_is_retried_(steps[b]);
	xzamd_dec_block *hb2 = (xzamd_dec_block *)calloc(n2 ? n2 : 1, sizeof(*hb2));
	xzamd_dec_chain *hc2 = (xzamd_dec_chain *)calloc(n2 ? n2 : 1, sizeof(*hc2));
	uint8_t *stored2 = (uint8_t *)calloc(n2 ? n2 : 1, XZAMD_HDR_CHECK_BYTES);
	uint8_t *steps2 = (uint8_t *)calloc(n2 ? n2 : 1, 1);
	if (!hb2 || !hc2 || !stored2 || !steps2) FAILD(XZAMD_MEM_ERROR, "malloc");
	/* one run of ADJACENT such Blocks per call: the Checks of a group of Blocks are taken over one stretch of the output */
	for (uint64_t b0 = 0; b0 < nb && n2; ) {
		if (!step_is_retried_(steps[b0])) { ++b0; continue; }
		uint64_t n = 0;
		for (; b0 + n < nb && step_is_retried_(steps[b0 + n]); ++n) {
			hb2[n] = job->hb[b0 + n]; hb2[n].nunits = 0; hb2[n].error = 0; hb2[n].nrecs = 0;
			hc2[n] = job->hc[b0 + n];
			memcpy(stored2 + XZAMD_HDR_CHECK_BYTES * n, job->stored + XZAMD_HDR_CHECK_BYTES * (b0 + n), XZAMD_HDR_CHECK_BYTES);
			steps2[n] = XZAMD_VSTEP_NONE;
		}
		const xzamd_dec_group group2 = { 0, n, check };
		xzamd_dec_job job2 = *job;
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
		(void)fail_block_(c, rp, b, v, what[v]);
		break;
	}
done:
	free(hb2); free(hc2); free(stored2); free(steps2);
	return rc;
}

int xzamd_verify_job_(xzamd_ctx *c, void *st, xzamd_dec_job *job, uint64_t utotal, int mode, xzamd_verify_report *rp)
{
	int rc;
	if (mode & XZAMD_VT_KEPT) {
		xzamd_resume_view tab;
		xzamd_ctx_resume_(c, &tab);
		job_take_table_(job, &tab, utotal);
	}
	rc = xzamd_dec_run_(c, st, job);
	if (rc == XZAMD_DATA_ERROR && job->d_expected && (mode & XZAMD_VT_PRECISE))
		rc = verify_again_(c, st, job, job->steps, rp);
	return rc;
}

int xzamd_verify_table_(xzamd_ctx *c, const uint8_t *d_xz, uint64_t xz_size, const xzamd_hdr_rec *recs, uint64_t nb, int check,
		const uint8_t *d_original, uint64_t original_size, int mode, uint8_t *steps, xzamd_verify_report *rp, void *st)
{
	int rc = XZAMD_OK;
	void *d_tmp = NULL;
	xzamd_src s = { NULL, d_xz, st, xz_size, 0 };
	xzamd_blocks B = { NULL, NULL, NULL, NULL };
	const char *msg = "";
	uint64_t utotal = 0;
	memset(steps, 0, nb);
	if (rp) rp->blocks = nb;
	if (nb == 0) return XZAMD_OK;
	for (uint64_t b = 0; b < nb; ++b) utotal += recs[b].usize;
	if (d_original && original_size != utotal) {
		if (rp && rp->first_bad_step == XZAMD_VSTEP_NONE) rp->first_bad_step = XZAMD_VSTEP_COMPARE;
		return xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, "the Stream's uncompressed size differs from the size of the original");
	}
	/* every Block Header, the sizes against the table, Block Padding, the stored Check */
	rc = xzamd_block_table_(&s, recs, nb, &B, NULL, &msg);
	if (rc) FAILD(rc, msg);
	for (uint64_t b = 0; b < nb; ++b) {
		if (!B.err[b].code) continue;
		/* a Block whose header cannot be read: the table still gives its extent and its uncompressed size.  It takes no
		 * part in the run (no chunk chain, no filters) */
		steps[b] = XZAMD_VSTEP_GRAMMAR;
		if (rp && rp->first_bad_step == XZAMD_VSTEP_NONE)
			(void)fail_block_(c, rp, b, XZAMD_VSTEP_GRAMMAR, xzamd_block_step_msg_(B.err[b].step));
		memset(&B.hb[b], 0, sizeof(B.hb[b]));
		B.hb[b].cpos = recs[b].hpos; B.hb[b].upos = recs[b].upos; B.hb[b].usize = recs[b].usize;
		memset(&B.hc[b], 0, sizeof(B.hc[b]));
		if (recs[b].usize >= (1ull << 31)) FAILD(XZAMD_OPTIONS_ERROR, "Block too large for the device decoder");
	}
	HIPD(xzk_malloc(&d_tmp, utotal + 16), "hipMalloc (verification output)");
	const xzamd_dec_group group = { 0, nb, check };
	xzamd_dec_job job;
	memset(&job, 0, sizeof(job));
	job.d_xz = d_xz; job.d_out = (uint8_t *)d_tmp; job.d_expected = d_original;
	job.nb = nb; job.hb = B.hb; job.hc = B.hc; job.stored = B.stored;
	job.groups = &group; job.ngroups = 1;
	/* (the forward filters of the span-parallel history read the original in aligned words) */
	job.allow_split = ((uintptr_t)d_original & 15) == 0;
	job.report = rp;
	job.steps = steps;
	rc = xzamd_verify_job_(c, st, &job, utotal, mode, rp);
done:
	xzk_sync(st);
	if (d_tmp) xzk_free(d_tmp);
	xzamd_blocks_free_(&B);
	return rc;
}

int xzamd_stream_verify_blocks_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size,
		uint8_t *block_steps, uint64_t steps_cap, uint64_t *nblocks, xzamd_verify_report *report, void *stream)
{
	if (!c || !d_xz || (!d_original && original_size) || (!block_steps && steps_cap))
		return XZAMD_PROG_ERROR;
	struct timespec t0;
	xzamd_verify_report *rp = verify_begin_(c, report, &t0);
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	xzamd_hdr_rec *recs = NULL;
	uint64_t nb = 0;
	int check = 0, rc;
	if (nblocks) *nblocks = 0;
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
	return verify_end_(rp, report, &t0, rc);
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

