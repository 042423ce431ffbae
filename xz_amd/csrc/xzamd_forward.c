/*
 * xzamd_forward.c -- the forward framing reader of the device decoder: an .xz file read from its front, the way
 * common/stream_decoder.c reads it, instead of from its Footer (xzamd_framing.c, common/file_info.c).
 *
 *   Stream Header       twelve bytes, read to the host: magic, CRC32, Stream Flags (the primitives of xzamd_framing.c)
 *   Blocks              xzk_dec_walk (one wavefront) lists the whole Blocks that follow: the table an Index would have given.
 *                       xzamd_block_table_ (k_dec_headers) validates header against row, Block Padding, stored Check, exactly as
 *                       for a table from an Index; xzamd_dec_run_ in its collecting mode decodes them and verifies the Checks,
 *                       and the Blocks in front of the first one that fails any of this are delivered
 *   Index, Footer       what these Blocks call for is built (xzamd_frame_index_footer: the encoding is canonical -- minimal
 *                       VLIs, zero padding, CRC32) and compared with the bytes of the file (index_hash.c compares as much);
 *                       a difference inside the Index is a data error whatever it is, one inside the Footer is named in the
 *                       reference's order: magic and CRC32, footer flags, Backward Size, header against footer
 *   Stream Padding      with XZAMD_FWD_CONCATENATED: zeros, a multiple of four, then the next Stream Header
 *
 * The reader is one resumable step (xzamd_forward_step_, xzamd_internal.h): its state keeps the phase, the Check, the
 * sizes of the Stream's Blocks and the totals, so a step may end inside any piece and go on in the next buffer from that
 * piece's first byte.  The small reads go through a window of WIN bytes, so that the pieces that lie together (Index,
 * Footer, padding, the next header) cost one read: a constant number of reads and one walk launch per Stream, whatever its
 * Block count (a full walk table adds launches).
 */
#include "xzamd_internal.h"
#include "kernels_api.h"
#include "xzamd_block_parse.h"

#include <stdlib.h>
#include <string.h>

#define FORMAT_ERROR 7      /* LZMA_FORMAT_ERROR */
#define WIN 1024u
#define ROWS_FIRST 64u      /* rows that come back with the walk's result in one read */

enum { XZF_HEADER = 0, XZF_BLOCKS, XZF_INDEX, XZF_PADDING, XZF_DONE };

static uint64_t fwd_counters[4];
void xzamd_debug_forward_counters_(uint64_t out[4])
{
	for (int i = 0; i < 4; ++i) out[i] = __atomic_load_n(&fwd_counters[i], __ATOMIC_RELAXED);
}

void xzamd_forward_init_(xzamd_forward_state *s, uint32_t flags)
{
	memset(s, 0, sizeof(*s));
	s->flags = flags;
	s->first_stream = 1;
	s->phase = XZF_HEADER;
}

void xzamd_forward_free_(xzamd_forward_state *s)
{
	free(s->unp); free(s->usz);
	s->unp = s->usz = NULL;
	s->npairs = s->pairs_cap = 0;
}

/* one step's view of its buffer: the source, the read window, the scratch of the walk */
typedef struct {
	xzamd_ctx *c;
	xzamd_forward_state *s;
	xzamd_src src;
	uint8_t *d_out;
	uint64_t out_cap;
	int final;
	uint8_t win[WIN];
	uint64_t win_pos, win_len;
	uint8_t *big;                   /* a piece longer than the window */
	void *d_tab;                    /* xzamd_walk_result (64 bytes), then walk_cap rows */
	uint8_t *h_tab;
	uint32_t walk_cap;
	uint64_t counts[2];             /* of the decode runs */
} fwd;

/* n bytes at pos (pos + n <= size) in host memory */
static int fetch(fwd *f, uint64_t pos, uint64_t n, const uint8_t **p)
{
	if (pos >= f->win_pos && pos + n <= f->win_pos + f->win_len) { *p = f->win + (pos - f->win_pos); return 0; }
	if (n > WIN) {
		free(f->big);
		f->big = (uint8_t *)malloc(n);
		if (!f->big) return xzamd_ctx_fail_(f->c, XZAMD_MEM_ERROR, "malloc");
		if (xzamd_src_read_(&f->src, pos, f->big, n)) return xzamd_ctx_fail_(f->c, XZAMD_DEVICE_ERROR, "d2h container framing");
		*p = f->big;
		return 0;
	}
	const uint64_t m = f->src.size - pos < WIN ? f->src.size - pos : WIN;
	f->win_len = 0;
	if (xzamd_src_read_(&f->src, pos, f->win, m)) return xzamd_ctx_fail_(f->c, XZAMD_DEVICE_ERROR, "d2h container framing");
	f->win_pos = pos; f->win_len = m;
	*p = f->win;
	return 0;
}

static int stop_(fwd *f, uint32_t stop, uint64_t pos)
{
	f->s->stop = stop;
	f->s->consumed = pos;
	return XZAMD_OK;
}

static int defect_(fwd *f, uint64_t pos, int code, uint32_t step, const char *msg)
{
	f->s->stop = XZAMD_FWD_DEFECT;
	f->s->code = (uint32_t)code;
	f->s->step = step;
	f->s->consumed = pos;
	return xzamd_ctx_fail_(f->c, code, msg);
}

/* the bytes end inside the piece at pos */
static int short_(fwd *f, uint64_t pos) { return stop_(f, f->final ? XZAMD_FWD_TRUNCATED : XZAMD_FWD_MORE, pos); }

static int pairs_push(fwd *f, const xzamd_hdr_rec *rows, uint64_t n)
{
	xzamd_forward_state *s = f->s;
	if (s->npairs + n > s->pairs_cap) {
		uint64_t cap = s->pairs_cap ? s->pairs_cap : 256;
		while (cap < s->npairs + n) cap *= 2;
		uint64_t *a = (uint64_t *)realloc(s->unp, cap * 8);
		if (a) s->unp = a;
		uint64_t *b = (uint64_t *)realloc(s->usz, cap * 8);
		if (b) s->usz = b;
		if (!a || !b) return xzamd_ctx_fail_(f->c, XZAMD_MEM_ERROR, "malloc");
		s->pairs_cap = cap;
	}
	for (uint64_t i = 0; i < n; ++i) { s->unp[s->npairs] = rows[i].unpadded; s->usz[s->npairs++] = rows[i].usize; }
	return 0;
}

/* Stream Header at *pos */
static int phase_header(fwd *f, uint64_t *pos, int *go)
{
	xzamd_forward_state *s = f->s;
	const uint8_t *h;
	const char *msg = "";
	int rc;
	*go = 0;
	if (f->src.size - *pos < 12) return short_(f, *pos);
	if ((rc = fetch(f, *pos, 12, &h)) != 0) return rc;
	switch (xzamd_fr_header_(h)) {
	case XZAMD_FR_MAGIC:
		/* stream_decoder.c: LZMA_FORMAT_ERROR for the first Stream only; behind Stream Padding these are bytes that are no Stream */
		return defect_(f, *pos, s->first_stream ? FORMAT_ERROR : XZAMD_DATA_ERROR, 0, s->first_stream ? "not an .xz file (Header Magic)" : "Stream Header magic");
	case XZAMD_FR_CRC:
		return defect_(f, *pos, XZAMD_DATA_ERROR, 0, "Stream Header CRC32");
	}
	if ((rc = xzamd_fr_flags_(h + 6, &s->check, &msg)) != 0) return defect_(f, *pos, rc, 0, msg);
	s->first_stream = 0;
	s->npairs = 0;
	s->phase = XZF_BLOCKS;
	*pos += 12;
	*go = 1;
	return 0;
}

/* The whole Blocks from *pos on: walk, Block table, decode.  *go: the phase (or this one, after a full table) goes on. */
static int phase_blocks(fwd *f, uint64_t *pos, int *go)
{
	xzamd_forward_state *s = f->s;
	void *st = f->src.st;
	xzamd_blocks B = { NULL, NULL, NULL, NULL };
	uint8_t *steps = NULL;
	const char *msg = "";
	int rc = 0;
	*go = 0;
	if (!f->d_tab) {
		f->walk_cap = s->walk_cap ? s->walk_cap : XZAMD_FWD_WALK_CAP;
		const uint64_t bytes = 64 + (uint64_t)f->walk_cap * sizeof(xzamd_hdr_rec);
		f->h_tab = (uint8_t *)malloc(bytes);
		if (!f->h_tab) return xzamd_ctx_fail_(f->c, XZAMD_MEM_ERROR, "malloc");
		if (xzk_malloc(&f->d_tab, bytes)) return xzamd_ctx_fail_(f->c, XZAMD_DEVICE_ERROR, "hipMalloc (walk table)");
	}
	xzamd_walk_result *res = (xzamd_walk_result *)f->h_tab;
	xzamd_hdr_rec *rows = (xzamd_hdr_rec *)(f->h_tab + 64);
	xzamd_hdr_rec *d_rows = (xzamd_hdr_rec *)((uint8_t *)f->d_tab + 64);
	if (xzk_dec_walk(f->src.dev, f->src.size, *pos, xzamd_fr_check_size_(s->check), s->produced, d_rows, f->walk_cap,
			(xzamd_walk_result *)f->d_tab, st))
		return xzamd_ctx_fail_(f->c, XZAMD_DEVICE_ERROR, "walk launch");
	++s->launches; ++s->walks;
	/* the result and the first rows in one read; a longer table in a second */
	const uint32_t first = f->walk_cap < ROWS_FIRST ? f->walk_cap : ROWS_FIRST;
	++f->src.reads;
	if (xzk_d2h(f->h_tab, f->d_tab, 64 + (uint64_t)first * sizeof(*rows), st) || xzk_sync(st))
		return xzamd_ctx_fail_(f->c, XZAMD_DEVICE_ERROR, "d2h walk result");
	if (res->nrows > f->walk_cap || res->pos > f->src.size || res->pos < *pos)
		return xzamd_ctx_fail_(f->c, XZAMD_PROG_ERROR, "walk result out of range");
	if (res->nrows > first) {
		++f->src.reads;
		if (xzk_d2h(rows + first, d_rows + first, (uint64_t)(res->nrows - first) * sizeof(*rows), st) || xzk_sync(st))
			return xzamd_ctx_fail_(f->c, XZAMD_DEVICE_ERROR, "d2h walk rows");
	}
	const uint64_t nrows = res->nrows;
	s->blocks += nrows;

	/* the rows whose output fits.  A run addresses its output, and the temporaries of its inverse filters, by upos from 0 on:
	 * the rows of this launch count from `base`, where the first of them goes */
	const uint64_t base = s->produced;
	uint64_t n = 0;
	while (n < nrows && rows[n].upos >= base && rows[n].usize <= f->out_cap - rows[n].upos) ++n;
	for (uint64_t b = 0; b < nrows; ++b) rows[b].upos -= base;
	for (uint64_t b = 0; b < n; ++b) rows[b].end = res->pos;

	/* Block Headers against the rows, Block Padding, the stored Checks; then the decode of those in front of the first bad one */
	uint64_t good = n;
	uint32_t bad_code = 0, bad_step = 0;
	const char *bad_msg = "";
	if (n) {
		uint64_t launches = 0;
		rc = xzamd_block_table_(&f->src, rows, n, &B, &launches, &msg);
		s->launches += launches;
		if (rc) { rc = xzamd_ctx_fail_(f->c, rc, msg); goto out; }
		for (uint64_t b = 0; b < n; ++b)
			if (B.err[b].code) {
				good = b; bad_code = B.err[b].code; bad_step = B.err[b].step; bad_msg = xzamd_block_step_msg_(bad_step);
				break;
			}
	}
	if (good) {
		const xzamd_dec_group group = { 0, good, s->check };
		xzamd_dec_job job;
		steps = (uint8_t *)calloc(good, 1);
		if (!steps) { rc = xzamd_ctx_fail_(f->c, XZAMD_MEM_ERROR, "malloc"); goto out; }
		memset(&job, 0, sizeof(job));
		job.d_xz = f->src.dev; job.d_out = f->d_out ? f->d_out + base : NULL;
		job.nb = good; job.hb = B.hb; job.hc = B.hc; job.stored = B.stored;
		job.groups = &group; job.ngroups = 1;
		job.steps = steps;
		job.counts = f->counts;
		rc = xzamd_dec_run_(f->c, st, &job);
		if (rc != XZAMD_OK && rc != XZAMD_DATA_ERROR) goto out;
		rc = 0;
		for (uint64_t b = 0; b < good; ++b)
			if (steps[b] != XZAMD_VSTEP_NONE) {
				static const char *const what[5] = { "", "LZMA2 chunk grammar", "LZMA2 data (range coder / distances / chunk sizes)",
					"Block Check mismatch", "" };
				good = b; bad_code = XZAMD_DATA_ERROR; bad_step = 0; bad_msg = what[steps[b] < 5 ? steps[b] : 0];
				break;
			}
	}
	if ((rc = pairs_push(f, rows, good)) != 0) goto out;
	s->blocks_delivered += good;
	if (good) s->produced = base + rows[good - 1].upos + rows[good - 1].usize;
	if (bad_code) { rc = defect_(f, rows[good].hpos, (int)bad_code, bad_step, bad_msg); goto out; }
	if (n < nrows) {
		s->need = rows[n].usize;
		rc = stop_(f, XZAMD_FWD_OUT_FULL, rows[n].hpos);
		goto out;
	}
	*pos = res->pos;
	switch (res->stop) {
	case XZAMD_WALK_INDEX: s->phase = XZF_INDEX; *go = 1; break;
	case XZAMD_WALK_TABLE_FULL: *go = 1; break;
	case XZAMD_WALK_INCOMPLETE: rc = short_(f, *pos); break;
	case XZAMD_WALK_DEFECT:
		rc = defect_(f, *pos, (int)res->code, res->step, xzamd_block_step_msg_(res->step));
		break;
	default: rc = xzamd_ctx_fail_(f->c, XZAMD_PROG_ERROR, "walk result"); break;
	}
out:
	free(steps);
	xzamd_blocks_free_(&B);
	return rc;
}

/* Index and Stream Footer at *pos against the Blocks of the Stream */
static int phase_index(fwd *f, uint64_t *pos, int *go)
{
	xzamd_forward_state *s = f->s;
	const uint64_t cap = 18 * s->npairs + 64;
	const uint8_t *have;
	int rc = 0;
	*go = 0;
	uint8_t *want = (uint8_t *)malloc(cap);
	if (!want) return xzamd_ctx_fail_(f->c, XZAMD_MEM_ERROR, "malloc");
	const uint64_t w = xzamd_frame_index_footer(want, cap, s->check, s->unp, s->usz, s->npairs);
	if (w < 20) { free(want); return xzamd_ctx_fail_(f->c, XZAMD_PROG_ERROR, "Index of the Blocks read"); }
	const uint64_t avail = f->src.size - *pos, n = avail < w ? avail : w;
	if (n && (rc = fetch(f, *pos, n, &have)) != 0) { free(want); return rc; }
	uint64_t d = 0;
	while (d < n && have[d] == want[d]) ++d;
	if (d < n && d < w - 12) {
		/* index_hash.c / index_decoder.c: whatever differs inside an Index -- record count, a record, padding, CRC32 */
		rc = defect_(f, *pos, XZAMD_DATA_ERROR, 0, "the Index differs from the Blocks of its Stream");
	} else if (n < w) {
		rc = short_(f, *pos);
	} else if (d < w) {
		/* stream_flags_decoder.c:52-82 and stream_decoder.c: magic, CRC32, the footer's flags, Backward Size, header against footer */
		const uint8_t *ft = have + w - 12;
		const char *msg = "";
		uint64_t index_size = 0;
		int check = 0;
		const int fr = xzamd_fr_footer_(ft, &index_size);
		if (fr == XZAMD_FR_MAGIC) rc = defect_(f, *pos + w - 12, XZAMD_DATA_ERROR, 0, "Stream Footer magic");
		else if (fr == XZAMD_FR_CRC) rc = defect_(f, *pos + w - 12, XZAMD_DATA_ERROR, 0, "Stream Footer CRC32");
		else if (xzamd_fr_flags_(ft + 8, &check, &msg) == XZAMD_OPTIONS_ERROR) rc = defect_(f, *pos + w - 12, XZAMD_OPTIONS_ERROR, 0, msg);
		else if (index_size != w - 12) rc = defect_(f, *pos + w - 12, XZAMD_DATA_ERROR, 0, "Backward Size");
		else rc = defect_(f, *pos + w - 12, XZAMD_DATA_ERROR, 0, "Stream Header and Stream Footer disagree");
	} else {
		*pos += w;
		++s->streams;
		s->padding = 0;
		s->phase = (s->flags & XZAMD_FWD_CONCATENATED) ? XZF_PADDING : XZF_DONE;
		*go = 1;
	}
	free(want);
	return rc;
}

/* Stream Padding from *pos on: zeros, a multiple of four (stream_decoder.c:364-400) */
static int phase_padding(fwd *f, uint64_t *pos, int *go)
{
	xzamd_forward_state *s = f->s;
	int rc;
	*go = 0;
	for (;;) {
		const uint64_t avail = f->src.size - *pos;
		if (avail == 0) {
			if (!f->final) return stop_(f, XZAMD_FWD_MORE, *pos);
			if (s->padding & 3) return defect_(f, *pos, XZAMD_DATA_ERROR, 0, "Stream Padding is not a multiple of four bytes");
			return stop_(f, XZAMD_FWD_END, *pos);
		}
		const uint8_t *p;
		uint64_t m = avail < WIN ? avail : WIN;
		if (*pos >= f->win_pos && *pos < f->win_pos + f->win_len) m = f->win_pos + f->win_len - *pos;     /* what the window still holds */
		if ((rc = fetch(f, *pos, m, &p)) != 0) return rc;
		uint64_t k = 0;
		while (k < m && p[k] == 0) ++k;
		*pos += k;
		s->padding += k;
		if (k < m) break;
	}
	if (s->padding & 3) return defect_(f, *pos, XZAMD_DATA_ERROR, 0, "Stream Padding is not a multiple of four bytes");
	s->phase = XZF_HEADER;
	/* a caller that looks at every Stream Header itself gets the step back in front of it */
	if (s->pause_at_header) return stop_(f, XZAMD_FWD_PAUSE, *pos);
	*go = 1;
	return 0;
}

int xzamd_forward_step_(xzamd_ctx *c, xzamd_forward_state *s, const uint8_t *d_buf, uint64_t size, int final, uint8_t *d_out,
		uint64_t out_cap, void *stream)
{
	fwd *f = (fwd *)calloc(1, sizeof(*f));
	uint64_t pos = 0;
	int rc = 0, go = 1;
	if (!f) return xzamd_ctx_fail_(c, XZAMD_MEM_ERROR, "malloc");
	f->c = c; f->s = s; f->d_out = d_out; f->out_cap = out_cap; f->final = final;
	f->src.dev = d_buf; f->src.st = stream; f->src.size = size;
	s->consumed = s->produced = s->need = 0;
	s->stop = XZAMD_FWD_MORE; s->code = 0; s->step = 0;
	while (go && rc == 0) {
		switch (s->phase) {
		case XZF_HEADER: rc = phase_header(f, &pos, &go); break;
		case XZF_BLOCKS: rc = phase_blocks(f, &pos, &go); break;
		case XZF_INDEX: rc = phase_index(f, &pos, &go); break;
		case XZF_PADDING: rc = phase_padding(f, &pos, &go); break;
		default: rc = stop_(f, XZAMD_FWD_END, pos); go = 0; break;
		}
	}
	s->offset += s->consumed;
	s->reads += f->src.reads + f->counts[0];
	s->launches += f->counts[1];
	if (f->d_tab) xzk_free(f->d_tab);
	free(f->h_tab); free(f->big);
	free(f);
	return rc;
}

int xzamd_file_decode_forward_device(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, uint32_t flags, void *d_out, uint64_t out_cap,
		uint64_t *out_size, xzamd_forward_report *report, void *stream)
{
	if (!c || (!d_xz && xz_size) || !out_size || (!d_out && out_cap) || (flags & ~XZAMD_FWD_CONCATENATED))
		return XZAMD_PROG_ERROR;
	static const uint8_t none[16] = { 0 };
	void *st = stream ? stream : xzamd_ctx_stream_(c);
	xzamd_forward_state s;
	int rc;
	*out_size = 0;
	if (report) memset(report, 0, sizeof(*report));
	for (int i = 0; i < 4; ++i) __atomic_store_n(&fwd_counters[i], 0, __ATOMIC_RELAXED);
	if (xzk_set_device(xzamd_ctx_device(c)))
		return xzamd_ctx_fail_(c, XZAMD_DEVICE_ERROR, "hipSetDevice");
	xzamd_forward_init_(&s, flags);
	/* (no byte of an input of no bytes is read) */
	rc = xzamd_forward_step_(c, &s, d_xz ? (const uint8_t *)d_xz : none, xz_size, 1, (uint8_t *)d_out, out_cap, st);
	xzk_sync(st);
	*out_size = s.produced;
	if (report) {
		report->streams = s.streams; report->blocks = s.blocks; report->blocks_delivered = s.blocks_delivered;
		report->consumed = s.consumed; report->stop_offset = s.consumed;
		report->stop = s.stop; report->code = s.code; report->step = s.step;
	}
	__atomic_store_n(&fwd_counters[0], s.reads, __ATOMIC_RELAXED);
	__atomic_store_n(&fwd_counters[1], s.launches, __ATOMIC_RELAXED);
	__atomic_store_n(&fwd_counters[2], s.blocks_delivered, __ATOMIC_RELAXED);
	__atomic_store_n(&fwd_counters[3], s.walks, __ATOMIC_RELAXED);
	const uint32_t stop = s.stop;
	xzamd_forward_free_(&s);
	if (rc) return rc;
	if (stop == XZAMD_FWD_TRUNCATED) return xzamd_ctx_fail_(c, XZAMD_BUF_ERROR, "the input ends inside a Stream");
	if (stop == XZAMD_FWD_OUT_FULL) return xzamd_ctx_fail_(c, XZAMD_BUF_ERROR, "output buffer too small");
	return XZAMD_OK;
}
