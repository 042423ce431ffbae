/*
 * xzamd_chains.c -- verification and repair of BARE CHUNK CHAINS, and the single-Block Stream made of them on the device
 * (DESIGN.md 3.6 "Chains", 3.7).
 *
 * The single-Block Stream of lzma_stream_encoder / lzma_easy_encoder is coded in segments (XZAMD_F_SEGMENTS): per segment only
 * its LZMA2 chunk chain -- no Block Header, no end marker, no Check -- and a row of xzamd_block_info: where the chain lies,
 * how long it is, how many bytes it decodes to, and the segment's CRC.  That table is all the device decoder needs: a row
 * becomes an xzamd_dec_block (cpos = out_offset, csize = total_size, upos = running sum), the "stored Check" is the row's CRC,
 * the scan is the bare-chain one (xzk_dec_scan_chains) and every later stage of xzamd_dec_run_ is what it is for Blocks.  A
 * chain starts with a dictionary reset, so nothing in front of it can be referenced: it is a decode unit on the grounds a
 * dictionary reset inside a Block is one.
 *
 * The repair follows xzamd_repair.c -- verdicts, rung 1 (the options single-phase, through the batch encoder with
 * XZAMD_F_SEGMENTS), rung 2 (the stored chain), splice (xzamd_chains_plan_: every chain behind the first replaced one moves;
 * there is no padding, Index or Footer), one more pass of the verdicts, all or nothing.
 *
 * The batch encoder and the streaming front end refer to this unit weakly: a build of the host layer without it has no
 * XZAMD_F_SINGLE and no repair of segments.
 */
#include "xzamd_internal.h"
#include "kernels_api.h"

#include <stdlib.h>
#include <string.h>
#include <time.h>

#define RUNG1_MIN_SEGMENT 65536u    /* as RUNG1_MIN_BLOCK of xzamd_repair.c: a shorter segment is coded alone */

static double ms_between(const struct timespec *a, const struct timespec *b)
{
	return (double)(b->tv_sec - a->tv_sec) * 1e3 + (double)(b->tv_nsec - a->tv_nsec) * 1e-6;
}

#define FAILC(code, msg) do { rc = xzamd_ctx_fail_(c, (code), (msg)); goto done; } while (0)
#define HIPC(call, msg) do { if (call) FAILC(XZAMD_DEVICE_ERROR, msg); } while (0)

static int check_is_combinable(int check)
{
	return check == XZAMD_CHECK_NONE || check == XZAMD_CHECK_CRC32 || check == XZAMD_CHECK_CRC64;
}

static void report_clear(xzamd_verify_report *rp)
{
	memset(rp, 0, sizeof(*rp));
	rp->first_bad_block = UINT64_MAX;
}

/* ---- verdicts ---- */

int xzamd_chains_verify_(xzamd_ctx *c, const uint8_t *d_chains, uint64_t size, const xzamd_block_info *binfo, uint64_t nseg,
		uint32_t dict_size, int check, const uint8_t *d_original, uint64_t original_size, int mode, uint8_t *steps,
		xzamd_verify_report *rp, void *st)
{
	int rc = XZAMD_OK;
	void *d_tmp = NULL;
	xzamd_dec_block *hb = NULL;
	xzamd_dec_chain *hc = NULL;
	uint8_t *stored = NULL;
	uint64_t utotal = 0;
	memset(steps, 0, nseg);
	if (rp) rp->blocks = nseg;
	if (nseg == 0) return XZAMD_OK;
	if (!check_is_combinable(check))
		return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR, "chains: Checks none, CRC32, CRC64");
	hb = (xzamd_dec_block *)calloc(nseg, sizeof(*hb));
	hc = (xzamd_dec_chain *)calloc(nseg, sizeof(*hc));
	stored = (uint8_t *)calloc(nseg, XZAMD_HDR_CHECK_BYTES);
	if (!hb || !hc || !stored) FAILC(XZAMD_MEM_ERROR, "malloc");
	for (uint64_t i = 0; i < nseg; ++i) {
		/* no row may name a byte outside the buffer: the scan reads what the table says */
		if (binfo[i].out_offset > size || binfo[i].total_size > size - binfo[i].out_offset)
			FAILC(XZAMD_PROG_ERROR, "chains: binfo names bytes outside the buffer");
		if (binfo[i].uncompressed_size >= (1ull << 31)) FAILC(XZAMD_OPTIONS_ERROR, "segment too large for the device decoder");
		hb[i].cpos = binfo[i].out_offset; hb[i].csize = binfo[i].total_size;
		hb[i].upos = utotal; hb[i].usize = binfo[i].uncompressed_size;
		hb[i].dict_size = dict_size;
		for (uint32_t k = 0; k < 8; ++k) stored[XZAMD_HDR_CHECK_BYTES * i + k] = (uint8_t)(binfo[i].unpadded_size >> (8 * k));
		utotal += binfo[i].uncompressed_size;
	}
	if (d_original && original_size != utotal) {
		if (rp && rp->first_bad_step == XZAMD_VSTEP_NONE) rp->first_bad_step = XZAMD_VSTEP_COMPARE;
		FAILC(XZAMD_DATA_ERROR, "the segments' uncompressed size differs from the size of the original");
	}
	HIPC(xzk_malloc(&d_tmp, utotal + 16), "hipMalloc (verification output)");
	{
		const xzamd_dec_group group = { 0, nseg, check };
		xzamd_dec_job job;
		memset(&job, 0, sizeof(job));
		job.d_xz = d_chains; job.d_out = (uint8_t *)d_tmp; job.d_expected = d_original;
		job.nb = nseg; job.hb = hb; job.hc = hc; job.stored = stored;
		job.groups = &group; job.ngroups = 1;
		job.allow_split = 1;            /* (no filters: nothing reads the original in aligned words) */
		job.report = rp;
		job.steps = steps;
		job.chains = 1;
		rc = xzamd_verify_job_(c, st, &job, utotal, mode, rp);
	}
done:
	xzk_sync(st);
	if (d_tmp) xzk_free(d_tmp);
	free(hb); free(hc); free(stored);
	return rc;
}

int xzamd_chains_verify_device(xzamd_ctx *c, const void *d_chains, uint64_t size, const xzamd_block_info *binfo, uint64_t nsegments,
		const xzamd_lzma_options *opt, int check, const void *d_original, uint64_t original_size, uint8_t *seg_steps,
		uint64_t steps_cap, xzamd_verify_report *report, void *stream)
{
	if (!c || !opt || (!d_chains && size) || (!binfo && nsegments) || (!d_original && original_size) || (!seg_steps && steps_cap))
		return XZAMD_PROG_ERROR;
	struct timespec t0, t1;
	xzamd_verify_report *rp = xzamd_ctx_report_(c);
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	int rc;
	clock_gettime(CLOCK_MONOTONIC, &t0);
	report_clear(rp);
	if (report) *report = *rp;
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	if (nsegments > steps_cap) {
		rp->blocks = nsegments;
		rc = xzamd_ctx_fail_(c, XZAMD_BUF_ERROR, "seg_steps too small");
	} else
		rc = xzamd_chains_verify_(c, (const uint8_t *)d_chains, size, binfo, nsegments, opt->dict_size, check,
				(const uint8_t *)d_original, original_size, XZAMD_VT_KEPT | XZAMD_VT_PRECISE, seg_steps, rp, st);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	rp->ms_verify = (float)ms_between(&t0, &t1);
	if (report) *report = *rp;
	return rc;
}

/* ---- repair ---- */

/* scratch of a re-encoded segment: what the batch encoder may write for it */
static uint64_t slot_bytes(uint64_t usize)
{
	return (xzamd_block_buffer_bound(usize < RUNG1_MIN_SEGMENT ? RUNG1_MIN_SEGMENT : usize) + 15) & ~15ull;
}

static int chains_repair_(xzamd_ctx *c, uint8_t *d_chains, uint64_t size, uint64_t cap, xzamd_block_info *binfo, uint64_t nseg,
		const xzamd_lzma_options *opt, int check, const uint8_t *d_orig, uint64_t orig_size, uint64_t *new_size, void *st)
{
	int rc = XZAMD_OK;
	xzamd_repair_report *R = xzamd_ctx_repair_report_(c);
	xzamd_verify_report *rp = xzamd_ctx_report_(c);
	struct timespec t_begin, t0, t1;
	uint8_t *steps = NULL, *steps_run = NULL;
	xzamd_cp_chain *chains = NULL;
	xzamd_block_info *bi_run = NULL, *bi_new = NULL;
	xzamd_copy_seg *segs2 = NULL;
	uint64_t *scr_off = NULL;
	void *d_scr = NULL, *d_tmp = NULL, *d_old = NULL, *d_segs = NULL, *d_lits = NULL, *d_bad = NULL;
	xzamd_rp_plan plan;
	xzamd_ctx_saved saved;
	int have_saved = 0, moved = 0;
	uint64_t nbad = 0, scr_total = 0, uoff = 0;
	memset(&plan, 0, sizeof(plan));
	memset(R, 0, sizeof(*R));
	R->blocks = nseg; R->size_before = size; R->size_after = size;
	*new_size = size;
	clock_gettime(CLOCK_MONOTONIC, &t_begin);
	steps = (uint8_t *)calloc(nseg ? nseg : 1, 1);
	if (!steps) FAILC(XZAMD_MEM_ERROR, "malloc");

	/* 1. verdicts */
	report_clear(rp);
	rc = xzamd_chains_verify_(c, d_chains, size, binfo, nseg, opt->dict_size, check, d_orig, orig_size, XZAMD_VT_KEPT, steps, rp, st);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	rp->ms_verify = (float)ms_between(&t_begin, &t1);
	R->passes = 1;
	R->ms_verify_passes = rp->ms_verify;
	if (rc != XZAMD_OK && rc != XZAMD_DATA_ERROR) goto done;
	xzamd_repair_knob_reject_(steps, nseg);
	for (uint64_t i = 0; i < nseg; ++i) nbad += steps[i] != XZAMD_VSTEP_NONE;
	R->blocks_bad = nbad;
	if (nbad == 0) goto done;       /* all good (XZAMD_OK), or a defect no segment carries (the sizes differ) */
	rc = XZAMD_OK;

	/* 2. re-encode the bad segments, rung 1; runs of adjacent segments of one size in one call */
	clock_gettime(CLOCK_MONOTONIC, &t0);
	chains = (xzamd_cp_chain *)calloc(nseg, sizeof(*chains));
	scr_off = (uint64_t *)calloc(nseg, sizeof(*scr_off));
	steps_run = (uint8_t *)calloc(nseg, 1);
	bi_run = (xzamd_block_info *)calloc(nseg, sizeof(*bi_run));
	bi_new = (xzamd_block_info *)calloc(nseg, sizeof(*bi_new));
	if (!chains || !scr_off || !steps_run || !bi_run || !bi_new) FAILC(XZAMD_MEM_ERROR, "malloc");
	for (uint64_t i = 0; i < nseg; ++i) {
		chains[i].pos = binfo[i].out_offset; chains[i].len = binfo[i].total_size; chains[i].usize = binfo[i].uncompressed_size;
		chains[i].uoff = uoff;
		chains[i].repl = XZAMD_RP_KEEP;
		uoff += binfo[i].uncompressed_size;
		if (steps[i] != XZAMD_VSTEP_NONE) {
			scr_off[i] = scr_total;
			scr_total += slot_bytes(binfo[i].uncompressed_size);
		}
	}
	HIPC(xzk_malloc(&d_scr, scr_total + 16), "hipMalloc (repair scratch)");
	xzamd_ctx_save_(c, &saved);
	have_saved = 1;
	{
		xzamd_lzma_options o1;
		const int force2 = xzamd_repair_knob_rung2_();
		double ms_v = 0;
		xzamd_repair_rung1_options_(opt, &o1);
		for (uint64_t b = 0; b < nseg; ) {
			if (steps[b] == XZAMD_VSTEP_NONE) { ++b; continue; }
			if (chains[b].usize == 0) {
				/* (no encode writes a segment of no bytes; its chain is none either) */
				chains[b].repl = XZAMD_RP_STORED;
				++R->blocks_stored;
				++b;
				continue;
			}
			const uint64_t bs = chains[b].usize < RUNG1_MIN_SEGMENT ? RUNG1_MIN_SEGMENT : chains[b].usize;
			uint64_t n = 1, bytes = chains[b].usize, run_cap = slot_bytes(chains[b].usize);
			while (b + n < nseg && steps[b + n] != XZAMD_VSTEP_NONE && chains[b + n - 1].usize == bs && chains[b + n].usize != 0
					&& chains[b + n].usize <= bs && bytes + chains[b + n].usize < (1ull << 40)) {
				bytes += chains[b + n].usize;
				run_cap += slot_bytes(chains[b + n].usize);
				++n;
			}
			/* (the scratch slots of a run are adjacent: the run is written from the first one on) */
			const uint64_t run_off = scr_off[b];
			uint64_t osz = 0, nbk = 0;
			rc = xzamd_encode_device_(c, d_orig + chains[b].uoff, bytes, bs, &o1, check, XZAMD_F_SEGMENTS, (uint8_t *)d_scr + run_off,
					run_cap, &osz, bi_run, n, &nbk, st, NULL);
			if (rc != XZAMD_OK) goto done;
			if (nbk != n) FAILC(XZAMD_PROG_ERROR, "repair: the re-encode made another number of segments");
			/* ... and through the verification again, against their slice of the original */
			for (uint64_t i = 0; i < n; ++i) bi_run[i].out_offset += run_off;
			xzamd_verify_report vr;
			struct timespec v0, v1;
			report_clear(&vr);
			clock_gettime(CLOCK_MONOTONIC, &v0);
			rc = xzamd_chains_verify_(c, (const uint8_t *)d_scr, scr_total, bi_run, n, opt->dict_size, check, d_orig + chains[b].uoff, bytes,
					0, steps_run, &vr, st);
			clock_gettime(CLOCK_MONOTONIC, &v1);
			ms_v += ms_between(&v0, &v1);
			if (rc != XZAMD_OK && rc != XZAMD_DATA_ERROR) goto done;
			rc = XZAMD_OK;
			for (uint64_t i = 0; i < n; ++i) {
				if (steps_run[i] == XZAMD_VSTEP_NONE && !force2) {
					chains[b + i].repl = XZAMD_RP_CODED;
					chains[b + i].src = bi_run[i].out_offset;
					chains[b + i].new_len = bi_run[i].total_size;
					++R->blocks_reencoded;
				} else {
					chains[b + i].repl = XZAMD_RP_STORED;     /* rung 2 */
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
	rc = xzamd_chains_plan_(chains, nseg, &plan);
	if (rc != XZAMD_OK) FAILC(rc, "repair: splice layout of the chains");
	*new_size = plan.new_size;
	if (plan.new_size > cap) FAILC(XZAMD_BUF_ERROR, "repair: the repaired chains do not fit the buffer");
	{
		/* two gathers into the temporary: scratch / literals / the old chains, then the raw chunks of stored chains from the
		 * original (the gather has one third source per launch) */
		uint64_t na = 0, nbs = 0;
		segs2 = (xzamd_copy_seg *)malloc((plan.nsegs ? plan.nsegs : 1) * sizeof(*segs2));
		if (!segs2) FAILC(XZAMD_MEM_ERROR, "malloc");
		for (uint64_t i = 0; i < plan.nsegs; ++i)
			if (plan.segs[i].kind != 3) segs2[na++] = plan.segs[i];
		for (uint64_t i = 0; i < plan.nsegs; ++i)
			if (plan.segs[i].kind == 3) { segs2[na + nbs] = plan.segs[i]; segs2[na + nbs].kind = 2; ++nbs; }
		if (plan.nsegs >= (1ull << 31)) FAILC(XZAMD_OPTIONS_ERROR, "repair: too many segments of the gather");
		const uint64_t old_tail = size - plan.tail_pos;
		HIPC(xzk_malloc(&d_tmp, plan.tail_len + 16) || xzk_malloc(&d_old, old_tail + 16)
				|| xzk_malloc(&d_segs, (plan.nsegs ? plan.nsegs : 1) * sizeof(*segs2)) || xzk_malloc(&d_lits, plan.lits_len + 16),
				"hipMalloc (splice)");
		/* (a splice of coded replacements alone has no literal bytes) */
		HIPC(xzk_h2d(d_segs, segs2, plan.nsegs * sizeof(*segs2), st) || (plan.lits_len && xzk_h2d(d_lits, plan.lits, plan.lits_len, st)),
				"h2d splice plan");
		HIPC(xzk_assemble((const xzamd_copy_seg *)d_segs, (uint32_t)na, (const uint8_t *)d_scr, (const uint8_t *)d_lits, d_chains,
				(uint8_t *)d_tmp, st), "gather");
		HIPC(xzk_assemble((const xzamd_copy_seg *)d_segs + na, (uint32_t)nbs, (const uint8_t *)d_scr, (const uint8_t *)d_lits, d_orig,
				(uint8_t *)d_tmp, st), "gather");
		HIPC(xzk_d2d(d_old, d_chains + plan.tail_pos, old_tail, st) || xzk_sync(st), "gather");
		/* nothing of the chains has changed so far */
		moved = 1;
		HIPC(xzk_d2d(d_chains + plan.tail_pos, d_tmp, plan.tail_len, st) || xzk_sync(st), "copy of the spliced tail");
	}
	clock_gettime(CLOCK_MONOTONIC, &t1);
	R->ms_splice = (float)ms_between(&t0, &t1);

	/* the records of the replaced segments match nothing any more */
	{
		xzamd_resume_view tab;
		xzamd_ctx_resume_(c, &tab);
		if (tab.d_rec && tab.nrec && tab.nblocks == nseg) {
			HIPC(xzk_malloc(&d_bad, nseg + 16), "hipMalloc");
			HIPC(xzk_h2d(d_bad, steps, nseg, st) || xzk_resume_void_blocks(tab.d_rec, tab.stride, tab.nrec, (const uint8_t *)d_bad,
					(uint32_t)nseg, st) || xzk_sync(st), "void resume records");
		}
	}

	/* 4. the spliced chains through the verdicts once more; the old tail is kept until they pass */
	clock_gettime(CLOCK_MONOTONIC, &t0);
	for (uint64_t i = 0; i < nseg; ++i) {
		bi_new[i] = binfo[i];
		bi_new[i].out_offset = chains[i].new_pos; bi_new[i].total_size = chains[i].new_len;
	}
	report_clear(rp);
	rc = xzamd_chains_verify_(c, d_chains, plan.new_size, bi_new, nseg, opt->dict_size, check, d_orig, orig_size, XZAMD_VT_KEPT,
			steps_run, rp, st);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	rp->ms_verify = (float)ms_between(&t0, &t1);
	++R->passes;
	R->ms_verify_passes += rp->ms_verify;
	if (rc != XZAMD_OK) goto done;
	moved = 0;
	R->size_after = plan.new_size;
	for (uint64_t i = plan.first; i < nseg; ++i) binfo[i] = bi_new[i];      /* (the CRC and the uncompressed size stay) */
	(void)xzamd_ctx_fail_(c, XZAMD_OK, "");      /* (the message of the first defect: repaired) */
done:
	if (have_saved) xzamd_ctx_restore_(c, &saved);
	if (moved) {
		/* the spliced chains did not pass (or a device call failed behind the copy): the old tail comes back */
		if (xzk_d2d(d_chains + plan.tail_pos, d_old, size - plan.tail_pos, st) || xzk_sync(st))
			rc = xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "repair: restoring the chains");
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
	free(steps); free(steps_run); free(chains); free(scr_off); free(bi_run); free(bi_new); free(segs2);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	R->ms_repair = (float)ms_between(&t_begin, &t1);
	return rc;
}

/* the chains must lie back to back, in order: what XZAMD_F_SEGMENTS writes, and what the splice can shift */
static int chains_adjacent(const xzamd_block_info *binfo, uint64_t nseg, uint64_t size)
{
	for (uint64_t i = 0; i < nseg; ++i) {
		if (binfo[i].out_offset > size || binfo[i].total_size > size - binfo[i].out_offset) return 0;
		if (i + 1 < nseg && binfo[i + 1].out_offset != binfo[i].out_offset + binfo[i].total_size) return 0;
	}
	return nseg == 0 || binfo[nseg - 1].out_offset + binfo[nseg - 1].total_size == size;
}

int xzamd_chains_repair_device(xzamd_ctx *c, void *d_chains, uint64_t size, uint64_t cap, xzamd_block_info *binfo, uint64_t nsegments,
		const xzamd_lzma_options *opt, int check, const void *d_original, uint64_t original_size, uint64_t *new_size,
		xzamd_repair_report *report, void *stream)
{
	if (!c || !opt || !new_size || (!d_chains && size) || (!binfo && nsegments) || (!d_original && original_size) || cap < size)
		return XZAMD_PROG_ERROR;
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	int rc;
	*new_size = size;
	memset(xzamd_ctx_repair_report_(c), 0, sizeof(xzamd_repair_report));
	{
		const char *why = xzamd_options_check(opt);
		if (why) return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR, why);
	}
	if (!check_is_combinable(check) || opt->bcj != 0)
		return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR, "chains: the chain {LZMA2} and Checks none, CRC32, CRC64");
	if (!chains_adjacent(binfo, nsegments, size))
		return xzamd_ctx_fail_(c, XZAMD_PROG_ERROR, "repair of chains: binfo does not describe chains that lie back to back and end at `size`");
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	rc = chains_repair_(c, (uint8_t *)d_chains, size, cap, binfo, nsegments, opt, check, (const uint8_t *)d_original, original_size,
			new_size, st);
	if (report) xzamd_get_repair_report(c, report);
	return rc;
}

int xzamd_chains_encoded_(xzamd_ctx *c, void *d_out, uint64_t size, uint64_t cap, const void *d_in, uint64_t in_size,
		const xzamd_lzma_options *opt, int check, int repair, xzamd_block_info *binfo, uint64_t nseg, uint64_t *new_size, void *stream)
{
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	*new_size = size;
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	if (repair) {
		memset(xzamd_ctx_repair_report_(c), 0, sizeof(xzamd_repair_report));
		return chains_repair_(c, (uint8_t *)d_out, size, cap, binfo, nseg, opt, check, (const uint8_t *)d_in, in_size, new_size, st);
	}
	/* verified encode: any defect is XZAMD_DATA_ERROR, nothing is rewritten */
	struct timespec t0, t1;
	xzamd_verify_report *rp = xzamd_ctx_report_(c);
	uint8_t *steps = (uint8_t *)calloc(nseg ? nseg : 1, 1);
	if (!steps) return xzamd_ctx_fail_(c, XZAMD_MEM_ERROR, "malloc");
	clock_gettime(CLOCK_MONOTONIC, &t0);
	report_clear(rp);
	const int rc = xzamd_chains_verify_(c, (const uint8_t *)d_out, size, binfo, nseg, opt->dict_size, check, (const uint8_t *)d_in, in_size,
			XZAMD_VT_KEPT, steps, rp, st);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	rp->ms_verify = (float)ms_between(&t0, &t1);
	free(steps);
	return rc;
}

/* ---- XZAMD_F_SINGLE: the Stream lzma_stream_encoder writes, on the device ---- */

#define SINGLE_HEAD 24u     /* Stream Header + the Block Header without sizes */

int xzamd_single_encode_(xzamd_ctx *c, const void *d_in, uint64_t in_size, uint64_t block_size, const xzamd_lzma_options *opt,
		int check, uint32_t flags, void *d_out_, uint64_t out_cap, uint64_t *out_size, xzamd_block_info *binfo, uint64_t binfo_cap,
		uint64_t *nsegments, void *stream)
{
	if (!c || !opt || !out_size || (!d_in && in_size) || !d_out_)
		return XZAMD_PROG_ERROR;
	uint8_t *d_out = (uint8_t *)d_out_;
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	xzamd_block_info *bi = NULL;
	uint8_t buf[96];
	uint64_t w, nseg = 0, csz = 0;
	int rc = XZAMD_OK, enc_rc;
	*out_size = 0;
	if (nsegments) *nsegments = 0;
	if (flags & (XZAMD_F_BLOCKS_ONLY | XZAMD_F_SEGMENTS))
		return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR, "single: a whole Stream, not with XZAMD_F_BLOCKS_ONLY or XZAMD_F_SEGMENTS");
	if (!check_is_combinable(check) || opt->bcj != 0)
		return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR,
				"single: the chain {LZMA2} and a Check that can be combined from parts (none, CRC32, CRC64)");
	{
		const char *why = xzamd_options_check(opt);
		if (why) return xzamd_ctx_fail_(c, XZAMD_OPTIONS_ERROR, why);
	}
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	if (block_size == 0) block_size = xzamd_mt_block_size(opt);
	const uint32_t cbytes = xzamd_check_bytes_(check);
	if (in_size == 0) {
		/* stream_encoder.c: no input, no Block -- Stream Header, an Index without records, Stream Footer */
		w = xzamd_frame_header(buf, check);
		w += xzamd_frame_index_footer(buf + w, sizeof(buf) - w, check, NULL, NULL, 0);
		if (w > out_cap) return xzamd_ctx_fail_(c, XZAMD_BUF_ERROR, "output buffer too small");
		if (xzk_h2d(d_out, buf, w, st) || xzk_sync(st)) return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "h2d framing");
		*out_size = w;
		return XZAMD_OK;
	}
	/* what follows the chains: end marker, padding, Check, Index of one record, Footer */
	const uint64_t tail_max = 1 + 3 + cbytes + 32 + 12;
	if (out_cap < SINGLE_HEAD + tail_max) return xzamd_ctx_fail_(c, XZAMD_BUF_ERROR, "output buffer too small");
	nseg = (in_size + block_size - 1) / block_size;
	/* the segment table is needed whole, whatever the caller's binfo holds */
	bi = (xzamd_block_info *)calloc(nseg, sizeof(*bi));
	if (!bi) return xzamd_ctx_fail_(c, XZAMD_MEM_ERROR, "malloc");
	enc_rc = xzamd_encode_device_(c, d_in, in_size, block_size, opt, check,
			XZAMD_F_SEGMENTS | XZAMD_F_CHAINS_ | (flags & (XZAMD_F_KEEP_RESUME | XZAMD_F_VERIFY | XZAMD_F_REPAIR)),
			d_out + SINGLE_HEAD, out_cap - SINGLE_HEAD - tail_max, &csz, bi, nseg, &nseg, st, NULL);
	/* a verified encode that found a defect still delivers the framed Stream, with XZAMD_DATA_ERROR */
	if (enc_rc != XZAMD_OK && !(enc_rc == XZAMD_DATA_ERROR && (flags & XZAMD_F_VERIFY) && !(flags & XZAMD_F_REPAIR) && csz != 0)) {
		rc = enc_rc;
		goto done;
	}
	{
		uint64_t usize = 0, crc = 0;
		for (uint64_t i = 0; i < nseg; ++i) {
			if (check == XZAMD_CHECK_CRC32) crc = xzamd_crc32_combine((uint32_t)crc, (uint32_t)bi[i].unpadded_size, bi[i].uncompressed_size);
			else if (check == XZAMD_CHECK_CRC64) crc = xzamd_crc64_combine(crc, bi[i].unpadded_size, bi[i].uncompressed_size);
			usize += bi[i].uncompressed_size;
			bi[i].out_offset += SINGLE_HEAD;
		}
		w = xzamd_frame_header(buf, check);
		w += xzamd_block_header_nosizes_(buf + w, xzamd_dict_size_byte_(opt->dict_size));
		if (w != SINGLE_HEAD) FAILC(XZAMD_PROG_ERROR, "single: framing");
		HIPC(xzk_h2d(d_out, buf, SINGLE_HEAD, st), "h2d framing");
		const uint64_t payload = csz + 1;       /* Compressed Size: the chains and the end marker */
		const uint64_t unpadded = 12 + payload + cbytes;
		w = 0;
		buf[w++] = 0x00;
		while ((payload + (w - 1)) & 3) buf[w++] = 0;
		for (uint32_t k = 0; k < cbytes; ++k) buf[w++] = (uint8_t)(crc >> (8 * k));
		w += xzamd_frame_index_footer(buf + w, sizeof(buf) - w, check, &unpadded, &usize, 1);
		if (SINGLE_HEAD + csz + w > out_cap) FAILC(XZAMD_BUF_ERROR, "output buffer too small");
		HIPC(xzk_h2d(d_out + SINGLE_HEAD + csz, buf, w, st) || xzk_sync(st), "h2d framing");
		*out_size = SINGLE_HEAD + csz + w;
	}
	if (nsegments) *nsegments = nseg;
	for (uint64_t i = 0; binfo && i < nseg && i < binfo_cap; ++i) binfo[i] = bi[i];
	rc = enc_rc;
done:
	free(bi);
	return rc;
}
