/*
 * xzamd_repair.c -- repair of a Stream the device decoder rejects (DESIGN.md 3.6 "Repair"): per-Block verdicts, re-encode
 * of the rejected Blocks from their slices of the original, splice.
 *
 * A span-parallel encoder can emit chunk sequences a sequential one cannot, and a defect of that kind makes a Stream no
 * decoder accepts.  Whatever the defect, the library can hand back a valid Stream at the price of the rejected Blocks:
 *   rung 1  the caller's options SINGLE-PHASE (an explicit span size: every span starts with a state reset and the
 *           properties, k_span_encode) -- or, where xzamd_options_check refuses that (the optimal parser with pb > 2 needs the
 *           two-phase mode), the fast parser with the same dict_size / lc / lp / pb / filters; verified again
 *   rung 2  the stored form (uncompressed LZMA2 chunks, filters dropped): cannot fail
 * The re-encode is the batch encoder itself with XZAMD_F_BLOCKS_ONLY, on the context of the call: the context's kept resume
 * table and stats are set aside meanwhile (xzamd_ctx_save_).  The splice is laid out by xzamd_repair_plan_ and gathered by the
 * encoder's own xzk_assemble into a temporary that is copied over the Stream in one piece; all sizes are known before the first
 * byte moves, and the old tail is kept until the spliced Stream has passed its verification: all or nothing.
 * The batch encoder refers to xzamd_repair_encoded_ weakly: a build of the host layer without this unit has no XZAMD_F_REPAIR.
 */
#include "xzamd_internal.h"
#include "kernels_api.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define RUNG1_SPAN (256u << 10)     /* DESIGN.md 3.6 "Repair": 256 KiB spans cost +0.38 % against two-phase on text, 64 KiB +1.46 % */
#define RUNG1_MIN_BLOCK 65536u      /* the batch encoder takes no Block size below a span (4096); a shorter Block is coded alone */

static double ms_between(const struct timespec *a, const struct timespec *b)
{
	return (double)(b->tv_sec - a->tv_sec) * 1e3 + (double)(b->tv_nsec - a->tv_nsec) * 1e-6;
}

#define FAILR(code, msg) do { rc = xzamd_ctx_fail_(c, (code), (msg)); goto done; } while (0)
#define HIPR(call, msg) do { if (call) FAILR(XZAMD_DEVICE_ERROR, msg); } while (0)

/* XZAMD_TEST_REPAIR_REJECT="0,2" (tests): the first pass treats these Blocks as rejected at step "decode" */
void xzamd_repair_knob_reject_(uint8_t *steps, uint64_t nb)
{
	const char *e = getenv("XZAMD_TEST_REPAIR_REJECT");
	while (e && *e) {
		char *end = NULL;
		const unsigned long long b = strtoull(e, &end, 10);
		if (end == e) break;
		if (b < nb && steps[b] == XZAMD_VSTEP_NONE) steps[b] = XZAMD_VSTEP_DECODE;
		e = *end == ',' ? end + 1 : end;
		if (*end != ',') break;
	}
}

/* XZAMD_TEST_REPAIR_RUNG=2 (tests): what rung 1 made counts as rejected, so the stored rung runs */
int xzamd_repair_knob_rung2_(void)
{
	const char *e = getenv("XZAMD_TEST_REPAIR_RUNG");
	return e && *e == '2';
}

/* scratch of a re-encoded Block: what the batch encoder may write for it */
static uint64_t slot_bytes(uint64_t usize)
{
	return (xzamd_block_buffer_bound(usize < RUNG1_MIN_BLOCK ? RUNG1_MIN_BLOCK : usize) + 15) & ~15ull;
}

void xzamd_repair_rung1_options_(const xzamd_lzma_options *opt, xzamd_lzma_options *o)
{
	*o = *opt;
	if (o->span_size == XZAMD_SPAN_DEFAULT || o->span_size == XZAMD_SPAN_AUTO)
		o->span_size = RUNG1_SPAN;
	if (xzamd_options_check(o) != NULL) {
		/* the fast parser over the exact HC4 finder (what preset 2 runs), same dictionary, lc / lp / pb and filters */
		o->gpu_parser = 0; o->gpu_sa_window = 0; o->gpu_sa_depth = 0;
		o->gpu_mf = XZAMD_MF_HC4; o->gpu_depth = 24;
		if (o->gpu_nice_len < 4) o->gpu_nice_len = 4;
		o->span_cost = 0; o->span_bits = 0; o->enc_span_bits = 0; o->part_iters = 0;
	}
}

/* the Check of no bytes (a bad Block of uncompressed size 0 is stored without an encode) */
static void check_of_nothing(int check, uint8_t out[32])
{
	static const uint8_t sha_empty[32] = { 0xe3, 0xb0, 0xc4, 0x42, 0x98, 0xfc, 0x1c, 0x14, 0x9a, 0xfb, 0xf4, 0xc8, 0x99, 0x6f, 0xb9, 0x24,
		0x27, 0xae, 0x41, 0xe4, 0x64, 0x9b, 0x93, 0x4c, 0xa4, 0x95, 0x99, 0x1b, 0x78, 0x52, 0xb8, 0x55 };
	memset(out, 0, 32);
	if (check == XZAMD_CHECK_SHA256) memcpy(out, sha_empty, 32);
}

/* Blocks `recs` of d_xz (framed: a whole Stream of `size` bytes, else bare Blocks that end at `size`): verdicts, re-encode,
 * splice.  recs[b].upos = the Block's first byte in the original. */
static int repair_run_(xzamd_ctx *c, uint8_t *d_xz, uint64_t size, uint64_t cap, const xzamd_hdr_rec *recs, uint64_t nb, int check,
		int framed, const uint8_t *d_orig, uint64_t orig_size, const xzamd_lzma_options *opt, xzamd_block_info *binfo,
		uint64_t binfo_cap, uint64_t *new_size, void *st)
{
	int rc = XZAMD_OK;
	xzamd_repair_report *R = xzamd_ctx_repair_report_(c);
	xzamd_verify_report *rp = xzamd_ctx_report_(c);
	const uint32_t cbytes = xzamd_check_bytes_(check);
	struct timespec t_begin, t0, t1;
	uint8_t *steps = NULL, *steps_run = NULL;
	xzamd_rp_block *blocks = NULL;
	xzamd_block_info *bi_run = NULL;
	xzamd_hdr_rec *recs_run = NULL, *recs_new = NULL;
	xzamd_copy_seg *segs2 = NULL;
	uint64_t *scr_off = NULL;       /* per Block: where its re-encode run starts in the scratch buffer */
	void *d_scr = NULL, *d_tmp = NULL, *d_old = NULL, *d_segs = NULL, *d_lits = NULL, *d_bad = NULL;
	xzamd_rp_plan plan;
	xzamd_ctx_saved saved;
	int have_saved = 0, moved = 0;
	uint64_t nbad = 0, scr_total = 0, zero_check_off = 0;
	memset(&plan, 0, sizeof(plan));
	memset(R, 0, sizeof(*R));
	R->blocks = nb; R->size_before = size; R->size_after = size;
	*new_size = size;
	clock_gettime(CLOCK_MONOTONIC, &t_begin);
	if (cbytes == 0xFFFFFFFFu) return xzamd_ctx_fail_(c, XZAMD_UNSUPPORTED_CHECK, "checks: none, CRC32, CRC64, SHA-256");
	steps = (uint8_t *)calloc(nb ? nb : 1, 1);
	if (!steps) FAILR(XZAMD_MEM_ERROR, "malloc");

	/* 1. verdicts */
	memset(rp, 0, sizeof(*rp));
	rp->first_bad_block = UINT64_MAX;
	rc = xzamd_verify_table_(c, d_xz, size, recs, nb, check, d_orig, orig_size, XZAMD_VT_KEPT, steps, rp, st);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	rp->ms_verify = (float)ms_between(&t_begin, &t1);
	R->passes = 1;
	R->ms_verify_passes = rp->ms_verify;
	if (rc != XZAMD_OK && rc != XZAMD_DATA_ERROR) goto done;
	xzamd_repair_knob_reject_(steps, nb);
	for (uint64_t b = 0; b < nb; ++b) nbad += steps[b] != XZAMD_VSTEP_NONE;
	R->blocks_bad = nbad;
	if (nbad == 0) goto done;       /* all good (XZAMD_OK), or a defect no Block carries (the sizes of Stream and original differ) */
	rc = XZAMD_OK;

	/* 2. re-encode the bad Blocks, rung 1; runs of adjacent Blocks of one size in one call */
	clock_gettime(CLOCK_MONOTONIC, &t0);
	blocks = (xzamd_rp_block *)calloc(nb, sizeof(*blocks));
	scr_off = (uint64_t *)calloc(nb, sizeof(*scr_off));
	steps_run = (uint8_t *)calloc(nb, 1);
	bi_run = (xzamd_block_info *)calloc(nb, sizeof(*bi_run));
	recs_run = (xzamd_hdr_rec *)calloc(nb, sizeof(*recs_run));
	if (!blocks || !scr_off || !steps_run || !bi_run || !recs_run) FAILR(XZAMD_MEM_ERROR, "malloc");
	for (uint64_t b = 0; b < nb; ++b) {
		blocks[b].pos = recs[b].hpos; blocks[b].unpadded = recs[b].unpadded; blocks[b].usize = recs[b].usize;
		blocks[b].uoff = recs[b].upos;
		blocks[b].repl = XZAMD_RP_KEEP;
		if (steps[b] != XZAMD_VSTEP_NONE) {
			scr_off[b] = scr_total;
			scr_total += slot_bytes(recs[b].usize);
		}
	}
	zero_check_off = scr_total;
	scr_total += 32;
	HIPR(xzk_malloc(&d_scr, scr_total + 16), "hipMalloc (repair scratch)");
	{
		uint8_t zc[32];
		check_of_nothing(check, zc);
		HIPR(xzk_h2d((uint8_t *)d_scr + zero_check_off, zc, 32, st) || xzk_sync(st), "h2d");
	}
	xzamd_ctx_save_(c, &saved);
	have_saved = 1;
	{
		xzamd_lzma_options o1;
		const int force2 = xzamd_repair_knob_rung2_();
		double ms_v = 0;
		xzamd_repair_rung1_options_(opt, &o1);
		for (uint64_t b = 0; b < nb; ) {
			if (steps[b] == XZAMD_VSTEP_NONE) { ++b; continue; }
			if (recs[b].usize == 0) {
				blocks[b].repl = XZAMD_RP_STORED;
				blocks[b].src = zero_check_off;
				++R->blocks_stored;
				++b;
				continue;
			}
			const uint64_t bs = recs[b].usize < RUNG1_MIN_BLOCK ? RUNG1_MIN_BLOCK : recs[b].usize;
			uint64_t n = 1, bytes = recs[b].usize, run_cap = slot_bytes(recs[b].usize);
			while (b + n < nb && steps[b + n] != XZAMD_VSTEP_NONE && recs[b + n - 1].usize == bs && recs[b + n].usize != 0
					&& recs[b + n].usize <= bs && bytes + recs[b + n].usize < (1ull << 40)) {
				bytes += recs[b + n].usize;
				run_cap += slot_bytes(recs[b + n].usize);
				++n;
			}
			/* (the scratch slots of a run are adjacent: the run is written from the first one on) */
			const uint64_t run_off = scr_off[b];
			uint64_t osz = 0, nbk = 0;
			rc = xzamd_encode_device_(c, d_orig + recs[b].upos, bytes, bs, &o1, check, XZAMD_F_BLOCKS_ONLY, (uint8_t *)d_scr + run_off,
					run_cap, &osz, bi_run, n, &nbk, st, NULL);
			if (rc != XZAMD_OK) goto done;
			if (nbk != n) FAILR(XZAMD_PROG_ERROR, "repair: the re-encode made another number of Blocks");
			/* ... and through the verification again, against their slice of the original */
			uint64_t up = 0;
			for (uint64_t i = 0; i < n; ++i) {
				recs_run[i].hpos = run_off + bi_run[i].out_offset;
				recs_run[i].unpadded = bi_run[i].unpadded_size;
				recs_run[i].usize = bi_run[i].uncompressed_size;
				recs_run[i].end = run_off + osz;
				recs_run[i].upos = up;
				recs_run[i].csz = cbytes;
				up += bi_run[i].uncompressed_size;
			}
			xzamd_verify_report vr;
			struct timespec v0, v1;
			memset(&vr, 0, sizeof(vr));
			vr.first_bad_block = UINT64_MAX;
			clock_gettime(CLOCK_MONOTONIC, &v0);
			rc = xzamd_verify_table_(c, (const uint8_t *)d_scr, scr_total, recs_run, n, check, d_orig + recs[b].upos, bytes, 0, steps_run,
					&vr, st);
			clock_gettime(CLOCK_MONOTONIC, &v1);
			ms_v += ms_between(&v0, &v1);
			if (rc != XZAMD_OK && rc != XZAMD_DATA_ERROR) goto done;
			rc = XZAMD_OK;
			for (uint64_t i = 0; i < n; ++i) {
				const uint64_t total = (bi_run[i].unpadded_size + 3) & ~3ull;
				if (steps_run[i] == XZAMD_VSTEP_NONE && !force2) {
					blocks[b + i].repl = XZAMD_RP_CODED;
					blocks[b + i].src = recs_run[i].hpos;
					blocks[b + i].new_unpadded = bi_run[i].unpadded_size;
					++R->blocks_reencoded;
				} else {
					/* rung 2; the Check at the end of the re-encoded Block is that of the slice whatever its chunks are */
					blocks[b + i].repl = XZAMD_RP_STORED;
					blocks[b + i].src = recs_run[i].hpos + total - cbytes;
					++R->blocks_stored;
				}
			}
			b += n;
		}
		++R->passes;
		R->ms_verify_passes += (float)ms_v;
		clock_gettime(CLOCK_MONOTONIC, &t1);
		R->ms_reencode = (float)(ms_between(&t0, &t1) - ms_v);
	}
	xzamd_ctx_restore_(c, &saved);
	have_saved = 0;

	/* 3. splice: layout first -- every size is known before a byte moves */
	clock_gettime(CLOCK_MONOTONIC, &t0);
	rc = xzamd_repair_plan_(blocks, nb, check, framed, &plan);
	if (rc != XZAMD_OK) FAILR(rc, "repair: splice layout");
	*new_size = plan.new_size;
	if (plan.new_size > cap) FAILR(XZAMD_BUF_ERROR, "repair: the repaired Stream does not fit the buffer");
	{
		/* two gathers into the temporary: scratch / literals / the old Stream, then the raw chunks of stored Blocks from the
		 * original (the gather has one third source per launch) */
		uint64_t na = 0, nbs = 0;
		segs2 = (xzamd_copy_seg *)malloc((plan.nsegs ? plan.nsegs : 1) * sizeof(*segs2));
		if (!segs2) FAILR(XZAMD_MEM_ERROR, "malloc");
		for (uint64_t i = 0; i < plan.nsegs; ++i)
			if (plan.segs[i].kind != 3) segs2[na++] = plan.segs[i];
		for (uint64_t i = 0; i < plan.nsegs; ++i)
			if (plan.segs[i].kind == 3) { segs2[na + nbs] = plan.segs[i]; segs2[na + nbs].kind = 2; ++nbs; }
		if (plan.nsegs >= (1ull << 31)) FAILR(XZAMD_OPTIONS_ERROR, "repair: too many segments");
		const uint64_t old_tail = size - plan.tail_pos;
		HIPR(xzk_malloc(&d_tmp, plan.tail_len + 16) || xzk_malloc(&d_old, old_tail + 16)
				|| xzk_malloc(&d_segs, (plan.nsegs ? plan.nsegs : 1) * sizeof(*segs2)) || xzk_malloc(&d_lits, plan.lits_len + 16),
				"hipMalloc (splice)");
		HIPR(xzk_h2d(d_segs, segs2, plan.nsegs * sizeof(*segs2), st) || xzk_h2d(d_lits, plan.lits, plan.lits_len, st), "h2d splice plan");
		HIPR(xzk_assemble((const xzamd_copy_seg *)d_segs, (uint32_t)na, (const uint8_t *)d_scr, (const uint8_t *)d_lits, d_xz,
				(uint8_t *)d_tmp, st), "gather");
		HIPR(xzk_assemble((const xzamd_copy_seg *)d_segs + na, (uint32_t)nbs, (const uint8_t *)d_scr, (const uint8_t *)d_lits, d_orig,
				(uint8_t *)d_tmp, st), "gather");
		HIPR(xzk_d2d(d_old, d_xz + plan.tail_pos, old_tail, st) || xzk_sync(st), "gather");
		/* nothing of the Stream has changed so far */
		moved = 1;
		HIPR(xzk_d2d(d_xz + plan.tail_pos, d_tmp, plan.tail_len, st) || xzk_sync(st), "copy of the spliced tail");
	}
	clock_gettime(CLOCK_MONOTONIC, &t1);
	R->ms_splice = (float)ms_between(&t0, &t1);

	/* the records of the repaired Blocks match nothing any more */
	{
		xzamd_resume_view tab;
		xzamd_ctx_resume_(c, &tab);
		if (tab.d_rec && tab.nrec && tab.nblocks == nb) {
			HIPR(xzk_malloc(&d_bad, nb + 16), "hipMalloc");
			HIPR(xzk_h2d(d_bad, steps, nb, st) || xzk_resume_void_blocks(tab.d_rec, tab.stride, tab.nrec, (const uint8_t *)d_bad,
					(uint32_t)nb, st) || xzk_sync(st), "void resume records");
		}
	}

	/* 4. the spliced Stream through the per-Block verification once more */
	clock_gettime(CLOCK_MONOTONIC, &t0);
	if (framed) {
		uint64_t nb2 = 0;
		rc = xzamd_stream_verify_blocks_device(c, d_xz, plan.new_size, d_orig, orig_size, steps_run, nb, &nb2, NULL, st);
	} else {
		recs_new = (xzamd_hdr_rec *)malloc(nb * sizeof(*recs_new));
		if (!recs_new) FAILR(XZAMD_MEM_ERROR, "malloc");
		for (uint64_t b = 0; b < nb; ++b) {
			recs_new[b] = recs[b];
			recs_new[b].hpos = blocks[b].new_pos; recs_new[b].unpadded = blocks[b].new_unpadded; recs_new[b].end = plan.new_size;
		}
		memset(rp, 0, sizeof(*rp));
		rp->first_bad_block = UINT64_MAX;
		rc = xzamd_verify_table_(c, d_xz, plan.new_size, recs_new, nb, check, d_orig, orig_size, XZAMD_VT_KEPT, steps_run, rp, st);
		clock_gettime(CLOCK_MONOTONIC, &t1);
		rp->ms_verify = (float)ms_between(&t0, &t1);
	}
	clock_gettime(CLOCK_MONOTONIC, &t1);
	++R->passes;
	R->ms_verify_passes += (float)ms_between(&t0, &t1);
	if (rc != XZAMD_OK) goto done;
	moved = 0;
	R->size_after = plan.new_size;
	for (uint64_t b = plan.first; binfo && b < nb && b < binfo_cap; ++b) {
		binfo[b].unpadded_size = blocks[b].new_unpadded;
		binfo[b].uncompressed_size = blocks[b].usize;
		binfo[b].out_offset = blocks[b].new_pos;
		binfo[b].total_size = (blocks[b].new_unpadded + 3) & ~3ull;
	}
	(void)xzamd_ctx_fail_(c, XZAMD_OK, "");      /* (the message of the first defect: repaired) */
done:
	if (have_saved) xzamd_ctx_restore_(c, &saved);
	if (moved) {
		/* the spliced Stream did not pass (or a device call failed behind the copy): the old tail comes back */
		if (xzk_d2d(d_xz + plan.tail_pos, d_old, size - plan.tail_pos, st) || xzk_sync(st))
			rc = xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "repair: restoring the Stream");
		*new_size = size;
	}
	xzk_sync(st);
	if (d_scr) xzk_free(d_scr);
	if (d_tmp) xzk_free(d_tmp);
	if (d_old) xzk_free(d_old);
	if (d_segs) xzk_free(d_segs);
	if (d_lits) xzk_free(d_lits);
	if (d_bad) xzk_free(d_bad);
	xzamd_repair_plan_free_(&plan);
	free(steps); free(steps_run); free(blocks); free(scr_off); free(bi_run); free(recs_run); free(recs_new); free(segs2);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	R->ms_repair = (float)ms_between(&t_begin, &t1);
	return rc;
}

int xzamd_stream_repair_device(xzamd_ctx *c, void *d_xz, uint64_t xz_size, uint64_t xz_cap, const void *d_original,
		uint64_t original_size, const xzamd_lzma_options *opt, uint64_t *new_size, xzamd_repair_report *report, void *stream)
{
	if (!c || !d_xz || !opt || !new_size || (!d_original && original_size) || xz_cap < xz_size)
		return XZAMD_PROG_ERROR;
	const int rc = xzamd_repair_encoded_(c, d_xz, xz_size, xz_cap, d_original, original_size, 0, opt, -1, 1, NULL, 0, 0, new_size, stream);
	if (report) xzamd_get_repair_report(c, report);
	return rc;
}

/* framed: the Block table and the Check come from the Stream itself (check, block_size and nblocks are not looked at); else
 * from binfo: bare Blocks of block_size uncompressed bytes but the last, written back to back from d_out on */
int xzamd_repair_encoded_(xzamd_ctx *c, void *d_out, uint64_t size, uint64_t cap, const void *d_in, uint64_t in_size,
		uint64_t block_size, const xzamd_lzma_options *opt, int check, int framed, xzamd_block_info *binfo, uint64_t binfo_cap,
		uint64_t nblocks, uint64_t *new_size, void *stream)
{
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	xzamd_hdr_rec *recs = NULL;
	uint64_t nb = 0;
	int rc;
	*new_size = size;
	memset(xzamd_ctx_repair_report_(c), 0, sizeof(xzamd_repair_report));
	{
		const char *why = xzamd_options_check(opt);
		if (why) return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR, why);
	}
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	if (framed) {
		xzamd_verify_report *rp = xzamd_ctx_report_(c);
		memset(rp, 0, sizeof(*rp));
		rp->first_bad_block = UINT64_MAX;
		rc = xzamd_stream_table_(c, (const uint8_t *)d_out, size, &recs, &nb, &check, st);
		if (rc != XZAMD_OK) {
			if (rc == XZAMD_DATA_ERROR || rc == 7) rp->first_bad_step = XZAMD_VSTEP_GRAMMAR;
			return rc;
		}
	} else {
		const uint32_t cbytes = xzamd_check_bytes_(check);
		if (cbytes == 0xFFFFFFFFu || nblocks > binfo_cap || (nblocks && !binfo))
			return xzamd_ctx_fail_(c, XZAMD_PROG_ERROR, "repair of bare Blocks: their table is binfo");
		nb = nblocks;
		recs = (xzamd_hdr_rec *)calloc(nb ? nb : 1, sizeof(*recs));
		if (!recs) return xzamd_ctx_fail_(c, XZAMD_MEM_ERROR, "malloc");
		uint64_t up = 0;
		for (uint64_t b = 0; b < nb; ++b) {
			if (binfo[b].out_offset > size || up != b * block_size) {
				free(recs);
				return xzamd_ctx_fail_(c, XZAMD_PROG_ERROR, "repair of bare Blocks: binfo does not describe them");
			}
			recs[b].hpos = binfo[b].out_offset; recs[b].unpadded = binfo[b].unpadded_size; recs[b].usize = binfo[b].uncompressed_size;
			recs[b].end = size; recs[b].upos = up; recs[b].csz = cbytes;
			up += binfo[b].uncompressed_size;
		}
	}
	rc = repair_run_(c, (uint8_t *)d_out, size, cap, recs, nb, check, framed, (const uint8_t *)d_in, in_size, opt, binfo, binfo_cap,
			new_size, st);
	free(recs);
	return rc;
}

void xzamd_get_repair_report(const xzamd_ctx *c, xzamd_repair_report *out)
{
	if (!c || !out) return;
	*out = *xzamd_ctx_repair_report_((xzamd_ctx *)c);
}
