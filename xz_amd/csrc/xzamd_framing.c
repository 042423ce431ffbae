/*
 * xzamd_framing.c -- the one reader of .xz container framing of the device decoder: container bytes, in host or in device
 * memory, become the tables a run consumes (xzamd_dec_run_, xzamd_decode.c): one xzamd_hdr_rec per Block from the Indexes,
 * and from those the Block table (xzamd_dec_block, xzamd_dec_chain, the stored Check, the verdict of xzb_block per Block).
 *
 * Restated from the reference's decoder chain, each check once:
 *   common/stream_flags_decoder.c:30-82     Stream Header / Footer (magic, CRC32, flags, Backward Size)
 *   common/index_decoder.c / index_hash.c   Index (indicator, CRC32, record count, records, padding)
 *   common/file_info.c                      the backward walk over concatenated Streams and Stream Padding
 * The per-Block checks are xzb_block (xzamd_block_parse.h): on the host for a file in host memory, as k_dec_headers (one
 * thread per Block; one upload, one launch, one read-back) for device memory.
 * The primitives report WHAT is wrong; the two walks decide the code, because the entries differ (DESIGN.md 3.6 lists where):
 * xzamd_stream_walk_ (one Stream: xzamd_stream_decode_device and the verifying entries) answers LZMA_FORMAT_ERROR for bad
 * magic bytes at either end, xzamd_file_walk_ (the file entries; common/stream_decoder.c with LZMA_CONCATENATED) only for the
 * first twelve bytes of the file.
 */
#include "xzamd_internal.h"
#include "kernels_api.h"
#include "xzamd_block_parse.h"

#include <stdlib.h>
#include <string.h>

#define FORMAT_ERROR 7      /* LZMA_FORMAT_ERROR */
#define TAIL_WINDOW 1024u   /* bytes in front of a position read at once to find the end of Stream Padding */

static const uint8_t check_sizes[16] = { 0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64 };
static const uint8_t magic[6] = { 0xFD, '7', 'z', 'X', 'Z', 0x00 };

int xzamd_src_read_(xzamd_src *s, uint64_t off, void *buf, uint64_t n)
{
	if (s->host) { memcpy(buf, s->host + off, n); return 0; }
	++s->reads;
	return xzk_d2h(buf, s->dev + off, n, s->st) || xzk_sync(s->st);
}

const char *xzamd_block_step_msg_(uint32_t step)
{
	static const char *const msg[XZB_S_COUNT] = {
		"", "Block beyond the Index", "Index indicator where a Block Header was expected", "Block Header beyond the Index",
		"Block Header CRC32", "reserved Block Flags", "Block Header Compressed Size", "Block Header Uncompressed Size", "Filter Flags",
		"LZMA2 properties (dictionary size byte)", "delta filter: size of properties", "BCJ filter: size of properties",
		"BCJ filter with a non-zero start offset is not decoded on the device", "filter id the device decoder does not know",
		"Block Header padding", "filter chain: LZMA2 must be the last filter and only the last",
		"Unpadded Size smaller than its header", "Block Header sizes differ from the Index", "Block beyond the Index",
		"Block Padding", "Block too large for the device decoder", "LZMA2 chunk control byte",
		"Block Header sizes differ from the LZMA2 chunk chain" };
	return step < XZB_S_COUNT ? msg[step] : "";
}

/* ---- the primitives ---- */
enum { FR_OK = 0, FR_MAGIC, FR_CRC };

/* the twelve bytes of a Stream Header: magic, CRC32 of the Stream Flags */
static int header_read(const uint8_t h[12])
{
	if (memcmp(h, magic, 6) != 0) return FR_MAGIC;
	return xzb_rd32(h + 8) == xzamd_crc32_host_(h + 6, 2) ? FR_OK : FR_CRC;
}

/* ... of a Stream Footer: magic, CRC32; *index_size from the Backward Size */
static int footer_read(const uint8_t f[12], uint64_t *index_size)
{
	*index_size = ((uint64_t)xzb_rd32(f + 4) + 1) * 4;
	if (f[10] != 'Y' || f[11] != 'Z') return FR_MAGIC;
	return xzb_rd32(f) == xzamd_crc32_host_(f + 4, 6) ? FR_OK : FR_CRC;
}

/* Stream Flags: reserved bits are XZAMD_OPTIONS_ERROR; a Check that cannot be verified is reported, not skipped (the
 * reference: LZMA_UNSUPPORTED_CHECK) */
static int flags_read(const uint8_t f[2], int *check, const char **msg)
{
	*check = f[1] & 0x0F;
	if (f[0] != 0 || (f[1] & 0xF0)) { *msg = "unsupported Stream Flags"; return XZAMD_OPTIONS_ERROR; }
	if (*check != XZAMD_CHECK_NONE && *check != XZAMD_CHECK_CRC32 && *check != XZAMD_CHECK_CRC64 && *check != XZAMD_CHECK_SHA256) {
		*msg = "Check id the device decoder cannot verify";
		return XZAMD_UNSUPPORTED_CHECK;
	}
	return 0;
}

/* the same primitives for the forward reader (xzamd_forward.c), which meets the pieces of a Stream in file order */
int xzamd_fr_header_(const uint8_t h[12]) { return header_read(h); }
int xzamd_fr_footer_(const uint8_t f[12], uint64_t *index_size) { return footer_read(f, index_size); }
int xzamd_fr_flags_(const uint8_t f[2], int *check, const char **msg) { return flags_read(f, check, msg); }
uint32_t xzamd_fr_check_size_(int check) { return check_sizes[check & 0x0F]; }

#define WFAIL(code, m) do { rc = (code); *msg = (m); goto out; } while (0)
#define WREAD(off, buf, n) do { if (xzamd_src_read_(s, (off), (buf), (n))) WFAIL(XZAMD_DEVICE_ERROR, "d2h container framing"); } while (0)

/* Where the entries differ about an Index: the bytes its Blocks may take, the largest Uncompressed Size of a record and of
 * the Stream, the longest Index Padding */
typedef struct { uint64_t room, usize_max, usum_max, pad_max; } index_limits;

/* An Index in host memory (index_size bytes, the CRC32 last; csz = size of the Stream's Check): Index Indicator, CRC32,
 * record count, the records, Index Padding.  One record per Block (malloc'ed), hpos and upos counted from the Stream's
 * first byte and first decoded byte, `end` left to the caller; blocks[0] = the padded sizes of the Blocks together,
 * blocks[1] = their uncompressed sizes together. */
static int index_read(const uint8_t *index, uint64_t index_size, uint32_t csz, const index_limits *lim, xzamd_hdr_rec **recs_out,
		uint64_t *nb_out, uint64_t blocks[2], const char **msg)
{
	const uint64_t end = index_size - 4;
	int rc = 0;
	uint64_t ip = 1, nb = 0, pos = 12, usum = 0;
	xzamd_hdr_rec *recs = NULL;
	if (index[0] != 0x00 || xzb_rd32(index + end) != xzamd_crc32_host_(index, end)) WFAIL(XZAMD_DATA_ERROR, "Index indicator / CRC32");
	if (xzb_vli(index, end, &ip, &nb) || nb > (index_size / 2)) WFAIL(XZAMD_DATA_ERROR, "Index record count");
	if (nb >= (1ull << 31)) WFAIL(XZAMD_OPTIONS_ERROR, "too many Blocks for the device decoder");
	recs = (xzamd_hdr_rec *)calloc(nb ? nb : 1, sizeof(*recs));
	if (!recs) WFAIL(XZAMD_MEM_ERROR, "malloc");
	for (uint64_t b = 0; b < nb; ++b) {
		xzamd_hdr_rec *r = &recs[b];
		if (xzb_vli(index, end, &ip, &r->unpadded) || xzb_vli(index, end, &ip, &r->usize)
				|| r->unpadded < 5 + csz || r->unpadded > (1ull << 62) || r->usize > lim->usize_max)
			WFAIL(XZAMD_DATA_ERROR, "Index record");
		r->hpos = pos; r->upos = usum; r->csz = csz;
		pos += (r->unpadded + 3) & ~3ull;
		usum += r->usize;
		if (pos - 12 > lim->room || usum > lim->usum_max) WFAIL(XZAMD_DATA_ERROR, "the Block sizes of the Index exceed the Stream");
	}
	if (end - ip > lim->pad_max) WFAIL(XZAMD_DATA_ERROR, "Index Padding");
	for (; ip < end; ++ip)
		if (index[ip] != 0) WFAIL(XZAMD_DATA_ERROR, "Index Padding");
	*recs_out = recs; recs = NULL;
	*nb_out = nb; blocks[0] = pos - 12; blocks[1] = usum;
out:
	free(recs);
	return rc;
}

/* ---- one Stream ---- */
int xzamd_stream_walk_(xzamd_src *s, uint64_t usize_max, xzamd_hdr_rec **recs_out, uint64_t *nb_out, int *check_out, const char **msg)
{
	int rc = XZAMD_OK, check = 0;
	uint8_t hf[24];
	uint8_t *index = NULL;
	xzamd_hdr_rec *recs = NULL;
	uint64_t index_size = 0, nb = 0, blocks[2];
	*recs_out = NULL; *nb_out = 0; *check_out = 0;
	if (s->size < 32 || (s->size & 3)) WFAIL(FORMAT_ERROR, "not an .xz Stream (size)");
	WREAD(0, hf, 12);
	WREAD(s->size - 12, hf + 12, 12);
	const int h = header_read(hf), f = footer_read(hf + 12, &index_size);
	if (h == FR_MAGIC || f == FR_MAGIC) WFAIL(FORMAT_ERROR, "bad magic bytes");
	if (h || f) WFAIL(XZAMD_DATA_ERROR, "Stream Header / Footer CRC32");
	rc = flags_read(hf + 6, &check, msg);
	if (rc == XZAMD_OPTIONS_ERROR || memcmp(hf + 6, hf + 20, 2) != 0)
		WFAIL(XZAMD_OPTIONS_ERROR, "unsupported or inconsistent Stream Flags");
	if (rc) goto out;
	if (index_size + 24 > s->size) WFAIL(XZAMD_DATA_ERROR, "Backward Size");
	const uint64_t index_at = s->size - 12 - index_size;
	const index_limits lim = { index_at - 12, usize_max, UINT64_MAX, UINT64_MAX };
	index = (uint8_t *)malloc(index_size);
	if (!index) WFAIL(XZAMD_MEM_ERROR, "malloc");
	WREAD(index_at, index, index_size);
	if ((rc = index_read(index, index_size, check_sizes[check], &lim, &recs, &nb, blocks, msg)) != 0) goto out;
	if (blocks[0] != index_at - 12) WFAIL(XZAMD_DATA_ERROR, "Blocks do not end where the Index starts");
	for (uint64_t b = 0; b < nb; ++b) recs[b].end = index_at;
	*recs_out = recs; recs = NULL;
	*nb_out = nb; *check_out = check;
out:
	free(index); free(recs);
	return rc;
}

int xzamd_stream_table_(xzamd_ctx *c, const uint8_t *d_xz, uint64_t xz_size, xzamd_hdr_rec **recs, uint64_t *nb, int *check, void *st)
{
	xzamd_src s = { NULL, d_xz, st, xz_size, 0 };
	const char *msg = "";
	const int rc = xzamd_stream_walk_(&s, 1ull << 62, recs, nb, check, &msg);
	return rc ? xzamd_ctx_fail_(c, rc, msg) : XZAMD_OK;
}

/* ---- a whole file ---- */
void xzamd_walk_free_(xzamd_walk *w)
{
	free(w->streams); free(w->recs); free(w->rec_stream);
	memset(w, 0, sizeof(*w));
}

/* The Stream that ends at `pos` (Stream Padding included), found from its end: padding, Footer, Index, the Header where
 * the Block sizes of the Index say it is.  *S (but first_block and uncompressed_offset) and its records (malloc'ed; upos
 * counted from the Stream's first decoded byte). */
static int stream_back(xzamd_src *s, uint64_t pos, const uint8_t head[12], xzamd_xz_stream *S, xzamd_hdr_rec **recs_out, const char **msg)
{
	int rc = 0, check = 0, hcheck = 0;
	uint8_t foot[12], hdr[12], win[TAIL_WINDOW];
	uint8_t *index = NULL;
	xzamd_hdr_rec *recs = NULL;
	uint64_t e = pos, index_size = 0, nb = 0, blocks[2];
	int have_foot = 0;
	/* Stream Padding: the zero bytes in front of pos; the twelve bytes in front of them are the Stream Footer */
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
	if ((pos - e) & 3) WFAIL(XZAMD_DATA_ERROR, "Stream Padding is not a multiple of four bytes");
	if (e < 32) WFAIL(XZAMD_DATA_ERROR, "bytes in front of a Stream that are no Stream");
	if (!have_foot) WREAD(e - 12, foot, 12);
	switch (footer_read(foot, &index_size)) {
	case FR_MAGIC: WFAIL(XZAMD_DATA_ERROR, "Stream Footer magic");
	case FR_CRC: WFAIL(XZAMD_DATA_ERROR, "Stream Footer CRC32");
	}
	if ((rc = flags_read(foot + 8, &check, msg)) != 0) goto out;
	if (index_size + 24 > e) WFAIL(XZAMD_DATA_ERROR, "Backward Size");
	const index_limits lim = { e, UINT64_MAX, 1ull << 62, 3 };
	index = (uint8_t *)malloc(index_size);
	if (!index) WFAIL(XZAMD_MEM_ERROR, "malloc");
	WREAD(e - 12 - index_size, index, index_size);
	if ((rc = index_read(index, index_size, check_sizes[check], &lim, &recs, &nb, blocks, msg)) != 0) goto out;
	if (blocks[0] + index_size + 24 > e)
		WFAIL(XZAMD_DATA_ERROR, "the Block sizes of the Index do not land on a Stream Header");
	const uint64_t sstart = e - 24 - index_size - blocks[0];
	if (sstart == 0) memcpy(hdr, head, 12);
	else WREAD(sstart, hdr, 12);
	/* the magic of the file's first twelve bytes has been looked at: this is a later Stream, or a Stream Header
	 * that is not where the Index says */
	switch (header_read(hdr)) {
	case FR_MAGIC: WFAIL(XZAMD_DATA_ERROR, "Stream Header magic");
	case FR_CRC: WFAIL(XZAMD_DATA_ERROR, "Stream Header CRC32");
	}
	if (flags_read(hdr + 6, &hcheck, msg) == XZAMD_OPTIONS_ERROR) { rc = XZAMD_OPTIONS_ERROR; goto out; }
	if (hdr[7] != foot[9]) WFAIL(XZAMD_DATA_ERROR, "Stream Header and Stream Footer disagree");
	for (uint64_t b = 0; b < nb; ++b) { recs[b].hpos += sstart; recs[b].end = e - 12 - index_size; }
	memset(S, 0, sizeof(*S));
	S->offset = sstart;
	S->size = e - sstart;
	S->padding = pos - e;
	S->block_count = nb;
	S->uncompressed_size = blocks[1];
	S->check = (uint32_t)check;
	*recs_out = recs; recs = NULL;
out:
	free(index); free(recs);
	return rc;
}

int xzamd_file_walk_(xzamd_src *s, xzamd_walk *w, const char **msg)
{
	typedef struct { xzamd_xz_stream s; xzamd_hdr_rec *recs; } tmp_stream;
	int rc = 0;
	tmp_stream *tmp = NULL;         /* the Streams as the walk meets them: last one first */
	uint64_t ntmp = 0, cap = 0, nrecs = 0, utotal = 0;
	uint8_t head[12];
	memset(w, 0, sizeof(*w));
	if (s->size < 32) WFAIL(FORMAT_ERROR, "not an .xz file (shorter than an empty Stream)");
	WREAD(0, head, 12);
	if (memcmp(head, magic, 6) != 0) WFAIL(FORMAT_ERROR, "not an .xz file (Header Magic)");
	for (uint64_t pos = s->size; pos > 0; pos = tmp[ntmp - 1].s.offset) {
		if (ntmp == cap) {
			cap = cap ? 2 * cap : 4;
			tmp_stream *t = (tmp_stream *)realloc(tmp, cap * sizeof(*tmp));
			if (!t) WFAIL(XZAMD_MEM_ERROR, "malloc");
			tmp = t;
		}
		tmp_stream *T = &tmp[ntmp];
		if ((rc = stream_back(s, pos, head, &T->s, &T->recs, msg)) != 0) goto out;
		++ntmp;
		nrecs += T->s.block_count;
		utotal += T->s.uncompressed_size;
		if (nrecs >= (1ull << 31) || utotal > (1ull << 62)) WFAIL(XZAMD_OPTIONS_ERROR, "too many Blocks for the device decoder");
	}

	/* file order */
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
		for (uint64_t b = 0; b < S->block_count; ++b, ++r) {
			w->recs[r] = T->recs[b];
			w->recs[r].upos += upos;
			w->rec_stream[r] = (uint32_t)i;
		}
		upos += S->uncompressed_size;
	}
	w->nstreams = ntmp;
	w->nrecs = nrecs;
	w->usize = utotal;
out:
	for (uint64_t i = 0; i < ntmp; ++i) free(tmp[i].recs);
	free(tmp);
	if (rc) xzamd_walk_free_(w);
	return rc;
}

/* ---- the Block table ---- */
void xzamd_blocks_free_(xzamd_blocks *B)
{
	free(B->hb); free(B->hc); free(B->stored); free(B->err);
	memset(B, 0, sizeof(*B));
}

int xzamd_block_table_(xzamd_src *s, const xzamd_hdr_rec *recs, uint64_t n, xzamd_blocks *B, uint64_t *launches, const char **msg)
{
	int rc = 0;
	void *d_recs = NULL, *d_table = NULL;
	uint8_t *h_table = NULL;
	memset(B, 0, sizeof(*B));
	B->hb = (xzamd_dec_block *)calloc(n ? n : 1, sizeof(*B->hb));
	B->hc = (xzamd_dec_chain *)calloc(n ? n : 1, sizeof(*B->hc));
	B->stored = (uint8_t *)calloc(n ? n : 1, XZAMD_HDR_CHECK_BYTES);
	B->err = (xzamd_hdr_err *)calloc(n ? n : 1, sizeof(*B->err));
	if (!B->hb || !B->hc || !B->stored || !B->err) WFAIL(XZAMD_MEM_ERROR, "malloc");
	if (n == 0) goto out;
	if (s->host) {
		for (uint64_t b = 0; b < n; ++b)
			B->err[b].code = xzb_block(s->host, &recs[b], &B->hb[b], &B->hc[b], B->stored + XZAMD_HDR_CHECK_BYTES * b, &B->err[b].step);
		goto out;
	}
	const uint64_t tbytes = XZAMD_HDR_TABLE_BYTES(n);
	h_table = (uint8_t *)malloc(tbytes);
	if (!h_table) WFAIL(XZAMD_MEM_ERROR, "malloc");
	if (xzk_malloc(&d_recs, n * sizeof(*recs)) || xzk_malloc(&d_table, tbytes)
			|| xzk_h2d(d_recs, recs, n * sizeof(*recs), s->st)
			|| xzk_dec_headers(s->dev, s->size, (const xzamd_hdr_rec *)d_recs, (uint32_t)n, d_table, s->st))
		WFAIL(XZAMD_DEVICE_ERROR, "Block Header kernel");
	++s->reads;
	if (xzk_d2h(h_table, d_table, tbytes, s->st) || xzk_sync(s->st)) WFAIL(XZAMD_DEVICE_ERROR, "d2h Block table");
	if (launches) ++*launches;
	const uint8_t *p = h_table;
	memcpy(B->hb, p, n * sizeof(*B->hb)); p += n * sizeof(*B->hb);
	memcpy(B->hc, p, n * sizeof(*B->hc)); p += n * sizeof(*B->hc);
	memcpy(B->stored, p, n * XZAMD_HDR_CHECK_BYTES); p += n * XZAMD_HDR_CHECK_BYTES;
	memcpy(B->err, p, n * sizeof(*B->err));
out:
	if (d_recs) xzk_free(d_recs);
	if (d_table) xzk_free(d_table);
	free(h_table);
	if (rc) xzamd_blocks_free_(B);
	return rc;
}

int xzamd_blocks_first_bad_(const xzamd_blocks *B, uint64_t n, const char **msg)
{
	for (uint64_t b = 0; b < n; ++b)
		if (B->err[b].code) { *msg = xzamd_block_step_msg_(B->err[b].step); return (int)B->err[b].code; }
	return 0;
}
