/*
 * xzamd_file.c -- whole .xz files for the device decoder: concatenated Streams, Stream Padding, the file index and
 * range decode (include/xz_amd.h, "whole .xz files").
 *
 * The entries here only compose: xzamd_file_walk_ (xzamd_framing.c) validates the framing of every Stream and lists the
 * Index records, xzamd_block_table_ turns the records that are wanted -- all of them, or those a range touches -- into the
 * Block table, the first bad Block in file order decides the code, and xzamd_dec_run_ (xzamd_decode.c) decodes one table
 * for all Streams, with one group of Blocks per Stream for the Checks.  What is left is the bookkeeping of each entry: the
 * lists of xzamd_file_index_*, the Blocks and the cut of a range, the read / launch counters of the tests.
 */
#include "xzamd_internal.h"
#include "kernels_api.h"

#include <stdlib.h>
#include <string.h>

/* test instrumentation (not public API), of the last file call on a file in device memory: [0] device-to-host reads,
 * [1] kernel-launch calls (a device-to-device copy counts as one), [2] Blocks decoded */
static uint64_t file_counters[3];
void xzamd_debug_file_counters_(uint64_t out[3])
{
	for (int i = 0; i < 3; ++i) out[i] = __atomic_load_n(&file_counters[i], __ATOMIC_RELAXED);
}
static void counters_set(uint64_t reads, uint64_t launches, uint64_t blocks)
{
	__atomic_store_n(&file_counters[0], reads, __ATOMIC_RELAXED);
	__atomic_store_n(&file_counters[1], launches, __ATOMIC_RELAXED);
	__atomic_store_n(&file_counters[2], blocks, __ATOMIC_RELAXED);
}

/* The Block table of n records of the file; the first Block in file order with a defect decides the code. */
static int file_headers(xzamd_src *s, const xzamd_hdr_rec *recs, uint64_t n, xzamd_blocks *B, uint64_t *launches, const char **msg)
{
	int rc = xzamd_block_table_(s, recs, n, B, launches, msg);
	if (!rc && (rc = xzamd_blocks_first_bad_(B, n, msg)) != 0) xzamd_blocks_free_(B);
	return rc;
}

static int fail(xzamd_ctx *c, int code, const char *msg) { return c ? xzamd_ctx_fail_(c, code, msg) : code; }

static int file_index(xzamd_ctx *c, xzamd_src *s, xzamd_xz_stream *streams, uint64_t streams_cap, uint64_t *nstreams,
		xzamd_xz_block *blocks, uint64_t blocks_cap, uint64_t *nblocks, uint64_t *uncompressed_size)
{
	xzamd_walk w;
	xzamd_blocks B = { NULL, NULL, NULL, NULL };
	const char *msg = "";
	uint64_t launches = 0;
	int rc = xzamd_file_walk_(s, &w, &msg);
	if (rc) return fail(c, rc, msg);
	if (nstreams) *nstreams = w.nstreams;
	if (nblocks) *nblocks = w.nrecs;
	if (uncompressed_size) *uncompressed_size = w.usize;
	rc = file_headers(s, w.recs, w.nrecs, &B, &launches, &msg);
	if (rc) { rc = fail(c, rc, msg); goto out; }
	if (w.nstreams > streams_cap || w.nrecs > blocks_cap || (w.nstreams && !streams) || (w.nrecs && !blocks)) {
		rc = fail(c, XZAMD_BUF_ERROR, "more Streams or Blocks than the lists hold");
		goto out;
	}
	memcpy(streams, w.streams, w.nstreams * sizeof(*streams));
	for (uint64_t b = 0; b < w.nrecs; ++b) {
		xzamd_xz_block *o = &blocks[b];
		memset(o, 0, sizeof(*o));
		o->header_offset = w.recs[b].hpos;
		o->unpadded_size = w.recs[b].unpadded;
		o->total_size = (w.recs[b].unpadded + 3) & ~3ull;
		o->uncompressed_size = w.recs[b].usize;
		o->uncompressed_offset = w.recs[b].upos;
		o->stream = w.rec_stream[b];
		for (uint32_t i = 0; i < B.hc[b].n; ++i) o->filter_ids[i] = B.hc[b].f[i] & 0xFFu;
		o->filter_ids[B.hc[b].n] = 0x21;
		o->filter_count = B.hc[b].n + 1;
	}
out:
	if (!s->host) counters_set(s->reads, launches, 0);
	xzamd_blocks_free_(&B);
	xzamd_walk_free_(&w);
	return rc;
}

int xzamd_file_index_host(const void *xz, uint64_t xz_size, xzamd_xz_stream *streams, uint64_t streams_cap, uint64_t *nstreams,
		xzamd_xz_block *blocks, uint64_t blocks_cap, uint64_t *nblocks, uint64_t *uncompressed_size)
{
	if (!xz && xz_size) return XZAMD_PROG_ERROR;
	static const uint8_t none[1] = { 0 };
	xzamd_src s = { xz ? (const uint8_t *)xz : none, NULL, NULL, xz_size, 0 };
	if (nstreams) *nstreams = 0;
	if (nblocks) *nblocks = 0;
	if (uncompressed_size) *uncompressed_size = 0;
	return file_index(NULL, &s, streams, streams_cap, nstreams, blocks, blocks_cap, nblocks, uncompressed_size);
}

int xzamd_file_index_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, xzamd_xz_stream *streams, uint64_t streams_cap,
		uint64_t *nstreams, xzamd_xz_block *blocks, uint64_t blocks_cap, uint64_t *nblocks, uint64_t *uncompressed_size)
{
	if (!c || !d_xz) return XZAMD_PROG_ERROR;
	if (nstreams) *nstreams = 0;
	if (nblocks) *nblocks = 0;
	if (uncompressed_size) *uncompressed_size = 0;
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	xzamd_src s = { NULL, (const uint8_t *)d_xz, xzamd_ctx_stream_(c), xz_size, 0 };
	return file_index(c, &s, streams, streams_cap, nstreams, blocks, blocks_cap, nblocks, uncompressed_size);
}

/* the Blocks [r0, r1) of the walk as groups of one Check each: the runs of Blocks of one Stream */
static xzamd_dec_group *make_groups(const xzamd_walk *w, uint64_t r0, uint64_t r1, uint32_t *ngroups)
{
	xzamd_dec_group *g = (xzamd_dec_group *)calloc(w->nstreams ? w->nstreams : 1, sizeof(*g));
	uint32_t n = 0;
	if (!g) return NULL;
	for (uint64_t r = r0; r < r1; ++r) {
		if (n == 0 || w->rec_stream[r] != w->rec_stream[r - 1]) {
			g[n].first = r - r0;
			g[n].count = 0;
			g[n].check = (int)w->streams[w->rec_stream[r]].check;
			++n;
		}
		++g[n - 1].count;
	}
	*ngroups = n;
	return g;
}

int xzamd_file_decode_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, void *d_out, uint64_t out_cap,
		uint64_t *out_size, const void *d_expected, uint64_t expected_size, uint64_t *mismatches, uint64_t *nblocks_out,
		void *stream)
{
	if (!c || !d_xz || !out_size || (!d_out && out_cap))
		return XZAMD_PROG_ERROR;
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	xzamd_walk w;
	xzamd_blocks B = { NULL, NULL, NULL, NULL };
	xzamd_dec_group *groups = NULL;
	uint32_t ngroups = 0;
	const char *msg = "";
	uint64_t counts[2] = { 0, 0 };
	int rc;
	*out_size = 0;
	if (mismatches) *mismatches = 0;
	if (nblocks_out) *nblocks_out = 0;
	counters_set(0, 0, 0);
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	xzamd_src s = { NULL, (const uint8_t *)d_xz, st, xz_size, 0 };
	rc = xzamd_file_walk_(&s, &w, &msg);
	if (rc) return xzamd_ctx_fail_(c, rc, msg);
	rc = file_headers(&s, w.recs, w.nrecs, &B, &counts[1], &msg);
	if (rc) { rc = xzamd_ctx_fail_(c, rc, msg); goto out; }
	if (nblocks_out) *nblocks_out = w.nrecs;
	*out_size = w.usize;
	if (w.usize > out_cap) { rc = xzamd_ctx_fail_(c, XZAMD_BUF_ERROR, "output buffer too small"); goto out; }
	if (d_expected && expected_size != w.usize) {
		rc = xzamd_ctx_fail_(c, XZAMD_DATA_ERROR, "the file's uncompressed size differs from the size of the original given for verification");
		goto out;
	}
	if (w.nrecs) {
		groups = make_groups(&w, 0, w.nrecs, &ngroups);
		if (!groups) { rc = xzamd_ctx_fail_(c, XZAMD_MEM_ERROR, "malloc"); goto out; }
		xzamd_dec_job job;
		memset(&job, 0, sizeof(job));
		job.d_xz = (const uint8_t *)d_xz; job.d_out = (uint8_t *)d_out; job.d_expected = (const uint8_t *)d_expected;
		job.nb = w.nrecs; job.hb = B.hb; job.hc = B.hc; job.stored = B.stored;
		job.groups = groups; job.ngroups = ngroups;
		job.allow_split = w.nstreams == 1;
		job.mismatches = mismatches;
		job.counts = counts;
		rc = xzamd_dec_run_(c, st, &job);
	}
out:
	xzk_sync(st);
	counters_set(s.reads + counts[0], counts[1], rc ? 0 : w.nrecs);
	free(groups);
	xzamd_blocks_free_(&B);
	xzamd_walk_free_(&w);
	return rc;
}

int xzamd_file_decode_range_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, uint64_t uoffset, uint64_t ulen,
		void *d_out, uint64_t out_cap, uint64_t *out_size, uint64_t *blocks_decoded, void *stream)
{
	if (!c || !d_xz || !out_size || (!d_out && out_cap))
		return XZAMD_PROG_ERROR;
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	xzamd_walk w;
	xzamd_blocks B = { NULL, NULL, NULL, NULL };
	xzamd_dec_group *groups = NULL;
	xzamd_hdr_rec *recs = NULL;
	void *d_tmp = NULL;
	uint32_t ngroups = 0;
	const char *msg = "";
	uint64_t counts[2] = { 0, 0 }, ndec = 0;
	int rc;
	*out_size = 0;
	if (blocks_decoded) *blocks_decoded = 0;
	counters_set(0, 0, 0);
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	xzamd_src s = { NULL, (const uint8_t *)d_xz, st, xz_size, 0 };
	rc = xzamd_file_walk_(&s, &w, &msg);
	if (rc) return xzamd_ctx_fail_(c, rc, msg);
	if (uoffset >= w.usize || ulen == 0) goto out;          /* like pread: nothing there, nothing read */
	{
		const uint64_t uend = ulen > w.usize - uoffset ? w.usize : uoffset + ulen;
		const uint64_t len = uend - uoffset;
		*out_size = len;
		if (len > out_cap) { rc = xzamd_ctx_fail_(c, XZAMD_BUF_ERROR, "output buffer too small"); goto out; }
		/* r0 = the first Block that ends behind uoffset, r1 = the first that starts at or behind uend (upos ascends) */
		uint64_t lo = 0, hi = w.nrecs;
		while (lo < hi) {
			const uint64_t mid = (lo + hi) / 2;
			if (w.recs[mid].upos + w.recs[mid].usize > uoffset) hi = mid; else lo = mid + 1;
		}
		const uint64_t r0 = lo;
		hi = w.nrecs;
		while (lo < hi) {
			const uint64_t mid = (lo + hi) / 2;
			if (w.recs[mid].upos >= uend) hi = mid; else lo = mid + 1;
		}
		const uint64_t r1 = lo;
		ndec = r1 - r0;
		const uint64_t base = w.recs[r0].upos;
		const uint64_t span = w.recs[r1 - 1].upos + w.recs[r1 - 1].usize - base;
		recs = (xzamd_hdr_rec *)malloc(ndec * sizeof(*recs));
		if (!recs) { rc = xzamd_ctx_fail_(c, XZAMD_MEM_ERROR, "malloc"); goto out; }
		memcpy(recs, w.recs + r0, ndec * sizeof(*recs));
		for (uint64_t i = 0; i < ndec; ++i) recs[i].upos -= base;     /* offsets in the decoded run of Blocks */
		rc = file_headers(&s, recs, ndec, &B, &counts[1], &msg);
		if (rc) { rc = xzamd_ctx_fail_(c, rc, msg); goto out; }
		/* a range of whole Blocks goes straight to d_out; else the touched Blocks go into a temporary and the range is cut out */
		const int whole = base == uoffset && base + span == uend;
		if (!whole && xzk_malloc(&d_tmp, span + 16)) { rc = xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipMalloc"); goto out; }
		groups = make_groups(&w, r0, r1, &ngroups);
		if (!groups) { rc = xzamd_ctx_fail_(c, XZAMD_MEM_ERROR, "malloc"); goto out; }
		xzamd_dec_job job;
		memset(&job, 0, sizeof(job));
		job.d_xz = (const uint8_t *)d_xz; job.d_out = whole ? (uint8_t *)d_out : (uint8_t *)d_tmp;
		job.nb = ndec; job.hb = B.hb; job.hc = B.hc; job.stored = B.stored;
		job.groups = groups; job.ngroups = ngroups;
		job.counts = counts;
		rc = xzamd_dec_run_(c, st, &job);
		if (rc) { *out_size = 0; goto out; }
		if (!whole) {
			if (xzk_d2d(d_out, (const uint8_t *)d_tmp + (uoffset - base), len, st) || xzk_sync(st)) {
				*out_size = 0;
				rc = xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "copy of the range");
				goto out;
			}
			++counts[1];
		}
		if (blocks_decoded) *blocks_decoded = ndec;
	}
out:
	xzk_sync(st);
	counters_set(s.reads + counts[0], counts[1], rc ? 0 : ndec);
	if (d_tmp) xzk_free(d_tmp);
	free(groups); free(recs);
	xzamd_blocks_free_(&B);
	xzamd_walk_free_(&w);
	return rc;
}
