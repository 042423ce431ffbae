/*
 * xzamd_file.c -- whole .xz files for the device decoder: concatenated Streams, Stream Padding, the file index and
 * range decode (include/xz_amd.h, "whole .xz files").
 *
 * file_walk restates the backward walk of the reference's common/file_info.c for a file that is resident in memory
 * (host or device): Stream Padding, Stream Footer, Backward Size, Index; the padded Block sizes of the Index give the
 * Stream Header; in front of it lies the previous Stream.  Per Stream it reads the tail of the file in front of the
 * position (padding + footer), the Index and the header: nothing per Block.  The codes are those of
 * common/stream_decoder.c with LZMA_CONCATENATED: LZMA_FORMAT_ERROR belongs to the first twelve bytes of the file alone.
 * The per-Block framing is xzb_block (xzamd_block_parse.h): on the host for a file in host memory, as k_dec_headers
 * (one thread per Block; one upload, one launch, one read-back) for a file in device memory.
 * The decode itself is xzamd_dec_run_ (xzamd_decode.c) over one Block table for all Streams.
 */
#include "xzamd_internal.h"
#include "kernels_api.h"
#include "xzamd_block_parse.h"

#include <stdlib.h>
#include <string.h>

#define FORMAT_ERROR 7      /* LZMA_FORMAT_ERROR */
#define TAIL_WINDOW 1024u   /* bytes in front of a position read at once to find the end of Stream Padding */

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

typedef struct {
	const uint8_t *host;    /* the file in host memory, or */
	const uint8_t *dev;     /* in device memory, read through st */
	void *st;
	uint64_t size;
	uint64_t reads;         /* device-to-host reads so far */
} xsrc;

static int src_read(xsrc *s, uint64_t off, void *buf, uint64_t n)
{
	if (s->host) { memcpy(buf, s->host + off, n); return 0; }
	++s->reads;
	return xzk_d2h(buf, s->dev + off, n, s->st) || xzk_sync(s->st);
}

typedef struct {
	xzamd_xz_stream *streams;   /* file order */
	uint64_t nstreams;
	xzamd_hdr_rec *recs;        /* one per Block of the file, file order; upos = offset in the decoded file */
	uint32_t *rec_stream;
	uint64_t nrecs;
	uint64_t usize;
} xwalk;

static void walk_free(xwalk *w)
{
	free(w->streams); free(w->recs); free(w->rec_stream);
	memset(w, 0, sizeof(*w));
}

static const uint8_t check_sizes[16] = { 0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64 };
static const uint8_t magic[6] = { 0xFD, '7', 'z', 'X', 'Z', 0x00 };

/* Validate the framing of every Stream of the file and list Streams and Index records.  Returns 0 or the code; *msg. */
static int file_walk(xsrc *s, xwalk *w, const char **msg)
{
#define WFAIL(code, m) do { rc = (code); *msg = (m); goto out; } while (0)
#define WREAD(off, buf, n) do { if (src_read(s, (off), (buf), (n))) WFAIL(XZAMD_DEVICE_ERROR, "d2h file framing"); } while (0)
	typedef struct { xzamd_xz_stream s; uint8_t *index; uint64_t index_size; } tmp_stream;
	int rc = 0;
	tmp_stream *tmp = NULL;         /* the Streams as the walk meets them: last one first */
	uint64_t ntmp = 0, cap = 0, nrecs = 0, utotal = 0;
	uint8_t head[12], win[TAIL_WINDOW];
	memset(w, 0, sizeof(*w));
	if (s->size < 32) WFAIL(FORMAT_ERROR, "not an .xz file (shorter than an empty Stream)");
	WREAD(0, head, 12);
	if (memcmp(head, magic, 6) != 0) WFAIL(FORMAT_ERROR, "not an .xz file (Header Magic)");
	uint64_t pos = s->size;
	while (pos > 0) {
		/* Stream Padding: the zero bytes in front of pos; the twelve bytes in front of them are the Stream Footer */
		uint64_t e = pos;
		uint8_t foot[12], hdr[12];
		int have_foot = 0;
		while (e > 0) {
			const uint64_t n = e < TAIL_WINDOW ? e : TAIL_WINDOW;
			WREAD(e - n, win, n);
			uint64_t k = n;
			while (k > 0 && win[k - 1] == 0) --k;
			if (k > 0) {
				if (k >= 12) { memcpy(foot, win + k - 12, 12); have_foot = 1; }
				e = e - n + k;
				break;
			}
			e -= n;
		}
		const uint64_t padding = pos - e;
		if (padding & 3) WFAIL(XZAMD_DATA_ERROR, "Stream Padding is not a multiple of four bytes");
		if (e < 32) WFAIL(XZAMD_DATA_ERROR, "bytes in front of a Stream that are no Stream");
		if (!have_foot) WREAD(e - 12, foot, 12);
		if (foot[10] != 'Y' || foot[11] != 'Z') WFAIL(XZAMD_DATA_ERROR, "Stream Footer magic");
		if (xzb_rd32(foot) != xzamd_crc32_host_(foot + 4, 6)) WFAIL(XZAMD_DATA_ERROR, "Stream Footer CRC32");
		if (foot[8] != 0 || (foot[9] & 0xF0)) WFAIL(XZAMD_OPTIONS_ERROR, "unsupported Stream Flags");
		const int check = foot[9] & 0x0F;
		/* a Check that cannot be verified is reported, not skipped (the reference: LZMA_UNSUPPORTED_CHECK) */
		if (check != XZAMD_CHECK_NONE && check != XZAMD_CHECK_CRC32 && check != XZAMD_CHECK_CRC64 && check != XZAMD_CHECK_SHA256)
			WFAIL(XZAMD_UNSUPPORTED_CHECK, "Check id the device decoder cannot verify");
		const uint32_t csz = check_sizes[check];
		const uint64_t index_size = ((uint64_t)xzb_rd32(foot + 4) + 1) * 4;
		if (index_size + 24 > e) WFAIL(XZAMD_DATA_ERROR, "Backward Size");

		if (ntmp == cap) {
			cap = cap ? 2 * cap : 4;
			tmp_stream *t = (tmp_stream *)realloc(tmp, cap * sizeof(*tmp));
			if (!t) WFAIL(XZAMD_MEM_ERROR, "malloc");
			tmp = t;
		}
		tmp_stream *T = &tmp[ntmp];
		memset(T, 0, sizeof(*T));
		T->index = (uint8_t *)malloc(index_size);
		if (!T->index) WFAIL(XZAMD_MEM_ERROR, "malloc");
		++ntmp;
		T->index_size = index_size;
		const uint8_t *index = T->index;
		WREAD(e - 12 - index_size, T->index, index_size);
		if (index[0] != 0x00 || xzb_rd32(index + index_size - 4) != xzamd_crc32_host_(index, index_size - 4))
			WFAIL(XZAMD_DATA_ERROR, "Index indicator / CRC32");
		uint64_t ip = 1, nb = 0, blocks_total = 0, usum = 0;
		if (xzb_vli(index, index_size - 4, &ip, &nb) || nb > (index_size / 2))
			WFAIL(XZAMD_DATA_ERROR, "Index record count");
		for (uint64_t b = 0; b < nb; ++b) {
			uint64_t unpadded = 0, usize = 0;
			if (xzb_vli(index, index_size - 4, &ip, &unpadded) || xzb_vli(index, index_size - 4, &ip, &usize)
					|| unpadded < 5 + csz || unpadded > (1ull << 62))
				WFAIL(XZAMD_DATA_ERROR, "Index record");
			blocks_total += (unpadded + 3) & ~3ull;
			usum += usize;
			if (blocks_total > e || usum > (1ull << 62))
				WFAIL(XZAMD_DATA_ERROR, "the Block sizes of the Index do not land on a Stream Header");
		}
		if (index_size - 4 - ip > 3) WFAIL(XZAMD_DATA_ERROR, "Index Padding");
		for (; ip < index_size - 4; ++ip)
			if (index[ip] != 0) WFAIL(XZAMD_DATA_ERROR, "Index Padding");
		if (blocks_total + index_size + 24 > e)
			WFAIL(XZAMD_DATA_ERROR, "the Block sizes of the Index do not land on a Stream Header");
		const uint64_t sstart = e - 24 - index_size - blocks_total;
		if (sstart == 0) memcpy(hdr, head, 12);
		else WREAD(sstart, hdr, 12);
		/* the magic of the file's first twelve bytes has been looked at: this is a later Stream, or a Stream Header
		 * that is not where the Index says */
		if (memcmp(hdr, magic, 6) != 0) WFAIL(XZAMD_DATA_ERROR, "Stream Header magic");
		if (xzb_rd32(hdr + 8) != xzamd_crc32_host_(hdr + 6, 2)) WFAIL(XZAMD_DATA_ERROR, "Stream Header CRC32");
		if (hdr[6] != 0 || (hdr[7] & 0xF0)) WFAIL(XZAMD_OPTIONS_ERROR, "unsupported Stream Flags");
		if (hdr[7] != foot[9]) WFAIL(XZAMD_DATA_ERROR, "Stream Header and Stream Footer disagree");
		T->s.offset = sstart;
		T->s.size = e - sstart;
		T->s.padding = padding;
		T->s.block_count = nb;
		T->s.uncompressed_size = usum;
		T->s.check = (uint32_t)check;
		nrecs += nb;
		utotal += usum;
		if (nrecs >= (1ull << 31) || utotal > (1ull << 62)) WFAIL(XZAMD_OPTIONS_ERROR, "too many Blocks for the device decoder");
		pos = sstart;
	}

	/* file order; the Indexes (valid by now) once more for the records */
	w->streams = (xzamd_xz_stream *)calloc(ntmp ? ntmp : 1, sizeof(*w->streams));
	w->recs = (xzamd_hdr_rec *)calloc(nrecs ? nrecs : 1, sizeof(*w->recs));
	w->rec_stream = (uint32_t *)calloc(nrecs ? nrecs : 1, 4);
	if (!w->streams || !w->recs || !w->rec_stream) WFAIL(XZAMD_MEM_ERROR, "malloc");
	uint64_t r = 0, upos = 0;
	for (uint64_t i = 0; i < ntmp; ++i) {
		const tmp_stream *T = &tmp[ntmp - 1 - i];
		xzamd_xz_stream *S = &w->streams[i];
		*S = T->s;
		S->first_block = r;
		S->uncompressed_offset = upos;
		const uint64_t index_at = S->offset + S->size - 12 - T->index_size;
		uint64_t ip = 1, nb = 0, hpos = S->offset + 12;
		xzb_vli(T->index, T->index_size - 4, &ip, &nb);
		for (uint64_t b = 0; b < nb; ++b, ++r) {
			uint64_t unpadded = 0, usize = 0;
			xzb_vli(T->index, T->index_size - 4, &ip, &unpadded);
			xzb_vli(T->index, T->index_size - 4, &ip, &usize);
			w->recs[r].hpos = hpos;
			w->recs[r].unpadded = unpadded;
			w->recs[r].usize = usize;
			w->recs[r].end = index_at;
			w->recs[r].upos = upos;
			w->recs[r].csz = check_sizes[S->check];
			w->rec_stream[r] = (uint32_t)i;
			hpos += (unpadded + 3) & ~3ull;
			upos += usize;
		}
	}
	w->nstreams = ntmp;
	w->nrecs = nrecs;
	w->usize = utotal;
out:
	for (uint64_t i = 0; i < ntmp; ++i) free(tmp[i].index);
	free(tmp);
	if (rc) walk_free(w);
	return rc;
#undef WFAIL
#undef WREAD
}

/* The parsed Blocks of a file (or of a run of its Blocks) */
typedef struct {
	xzamd_dec_block *hb;
	xzamd_dec_chain *hc;
	uint8_t *stored;        /* XZAMD_HDR_CHECK_BYTES per Block */
} xblocks;

static void blocks_free(xblocks *B) { free(B->hb); free(B->hc); free(B->stored); memset(B, 0, sizeof(*B)); }

/* xzb_block over n records: on the host for a file in host memory, as k_dec_headers else.  The first Block in file order
 * with a defect decides the code. */
static int file_headers(xsrc *s, const xzamd_hdr_rec *recs, uint64_t n, xblocks *B, uint64_t *launches, const char **msg)
{
	int rc = 0;
	void *d_recs = NULL, *d_table = NULL;
	uint8_t *h_table = NULL;
	memset(B, 0, sizeof(*B));
	B->hb = (xzamd_dec_block *)calloc(n ? n : 1, sizeof(*B->hb));
	B->hc = (xzamd_dec_chain *)calloc(n ? n : 1, sizeof(*B->hc));
	B->stored = (uint8_t *)calloc(n ? n : 1, XZAMD_HDR_CHECK_BYTES);
	if (!B->hb || !B->hc || !B->stored) { *msg = "malloc"; rc = XZAMD_MEM_ERROR; goto out; }
	if (n == 0) goto out;
	if (s->host) {
		for (uint64_t b = 0; b < n && !rc; ++b) {
			uint32_t step = 0;
			rc = (int)xzb_block(s->host, &recs[b], &B->hb[b], &B->hc[b], B->stored + XZAMD_HDR_CHECK_BYTES * b, &step);
			if (rc) *msg = xzamd_block_step_msg_(step);
		}
		goto out;
	}
	const uint64_t tbytes = XZAMD_HDR_TABLE_BYTES(n);
	h_table = (uint8_t *)malloc(tbytes);
	if (!h_table) { *msg = "malloc"; rc = XZAMD_MEM_ERROR; goto out; }
	if (xzk_malloc(&d_recs, n * sizeof(*recs)) || xzk_malloc(&d_table, tbytes)
			|| xzk_h2d(d_recs, recs, n * sizeof(*recs), s->st)
			|| xzk_dec_headers(s->dev, s->size, (const xzamd_hdr_rec *)d_recs, (uint32_t)n, d_table, s->st)) {
		*msg = "Block Header kernel"; rc = XZAMD_DEVICE_ERROR; goto out;
	}
	++s->reads;
	if (xzk_d2h(h_table, d_table, tbytes, s->st) || xzk_sync(s->st)) { *msg = "d2h Block table"; rc = XZAMD_DEVICE_ERROR; goto out; }
	if (launches) ++*launches;
	{
		const uint8_t *p = h_table;
		memcpy(B->hb, p, n * sizeof(*B->hb)); p += n * sizeof(*B->hb);
		memcpy(B->hc, p, n * sizeof(*B->hc)); p += n * sizeof(*B->hc);
		memcpy(B->stored, p, n * XZAMD_HDR_CHECK_BYTES); p += n * XZAMD_HDR_CHECK_BYTES;
		const xzamd_hdr_err *he = (const xzamd_hdr_err *)p;
		for (uint64_t b = 0; b < n; ++b)
			if (he[b].code) { rc = (int)he[b].code; *msg = xzamd_block_step_msg_(he[b].step); break; }
	}
out:
	if (d_recs) xzk_free(d_recs);
	if (d_table) xzk_free(d_table);
	free(h_table);
	if (rc) blocks_free(B);
	return rc;
}

static int fail(xzamd_ctx *c, int code, const char *msg) { return c ? xzamd_ctx_fail_(c, code, msg) : code; }

static int file_index(xzamd_ctx *c, xsrc *s, xzamd_xz_stream *streams, uint64_t streams_cap, uint64_t *nstreams,
		xzamd_xz_block *blocks, uint64_t blocks_cap, uint64_t *nblocks, uint64_t *uncompressed_size)
{
	xwalk w;
	xblocks B = { NULL, NULL, NULL };
	const char *msg = "";
	uint64_t launches = 0;
	int rc = file_walk(s, &w, &msg);
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
	blocks_free(&B);
	walk_free(&w);
	return rc;
}

int xzamd_file_index_host(const void *xz, uint64_t xz_size, xzamd_xz_stream *streams, uint64_t streams_cap, uint64_t *nstreams,
		xzamd_xz_block *blocks, uint64_t blocks_cap, uint64_t *nblocks, uint64_t *uncompressed_size)
{
	if (!xz && xz_size) return XZAMD_PROG_ERROR;
	static const uint8_t none[1] = { 0 };
	xsrc s = { xz ? (const uint8_t *)xz : none, NULL, NULL, xz_size, 0 };
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
	xsrc s = { NULL, (const uint8_t *)d_xz, xzamd_ctx_stream_(c), xz_size, 0 };
	return file_index(c, &s, streams, streams_cap, nstreams, blocks, blocks_cap, nblocks, uncompressed_size);
}

/* the Blocks [r0, r1) of the walk as groups of one Check each: the runs of Blocks of one Stream */
static xzamd_dec_group *make_groups(const xwalk *w, uint64_t r0, uint64_t r1, uint32_t *ngroups)
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
	xwalk w;
	xblocks B = { NULL, NULL, NULL };
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
	xsrc s = { NULL, (const uint8_t *)d_xz, st, xz_size, 0 };
	rc = file_walk(&s, &w, &msg);
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
	blocks_free(&B);
	walk_free(&w);
	return rc;
}

int xzamd_file_decode_range_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, uint64_t uoffset, uint64_t ulen,
		void *d_out, uint64_t out_cap, uint64_t *out_size, uint64_t *blocks_decoded, void *stream)
{
	if (!c || !d_xz || !out_size || (!d_out && out_cap))
		return XZAMD_PROG_ERROR;
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	xwalk w;
	xblocks B = { NULL, NULL, NULL };
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
	xsrc s = { NULL, (const uint8_t *)d_xz, st, xz_size, 0 };
	rc = file_walk(&s, &w, &msg);
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
	blocks_free(&B);
	walk_free(&w);
	return rc;
}
