/* driver_decode.c -- TEST INFRASTRUCTURE ONLY: drives the host code of the device decoder (xzamd_framing.c, xzamd_decode.c,
 * xzamd_file.c) over the CPU stand-ins stub_xzk.c + stub_xzk_dec.c and prints, per case and entry point, what the host code
 * decided: the return code, the Block count, the per-Block steps and the report where the entry has them, and the trace of
 * the kernel-layer calls with their scalar arguments.  No message texts.  A program of its own, so that it can be built
 * with sanitizers and simply run; tests/test_host_decode.py compares its output with tests/golden/decode_host_trace.txt.
 * usage: driver_decode FILE.xz ...      (the reference fixtures; the other cases are made here) */
#include "../../xz_amd/csrc/xzamd_internal.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver_decode: %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
#define OUT_CAP (4u << 20)
#define MAXB 160

void stub_dec_enable(void);
const char *stub_dec_trace(void);
void stub_dec_trace_reset(void);
void stub_dec_trace_free(void);
void stub_dec_scan_fail(uint64_t k);
void stub_sha256(const uint8_t *p, uint64_t n, uint8_t out[32]);

static xzamd_ctx *ctx;
static uint8_t *outbuf;

/* ---- Streams of stored Blocks: xzamd_stored_blocks_host_ per Block, Index and Footer of xzamd_frame.c ---- */
typedef struct {
	uint8_t *p;
	uint64_t len, cap, nb, index_at;
	int check;
	uint64_t unp[MAXB], usz[MAXB], hpos[MAXB];
} sbuild;

static void sb_begin(sbuild *s, uint8_t *buf, uint64_t cap, int check)
{
	memset(s, 0, sizeof(*s));
	s->p = buf; s->cap = cap; s->check = check;
	s->len = xzamd_frame_header(buf, check);
}

static void sb_block(sbuild *s, const uint8_t *data, uint64_t usize)
{
	const int sha = s->check == XZAMD_CHECK_SHA256;
	xzamd_block_info bi;
	uint64_t w = 0, nb = 0;
	CHECK(s->nb < MAXB);
	s->hpos[s->nb] = s->len;
	if (usize) {
		CHECK(xzamd_stored_blocks_host_(data, usize, usize, sha ? XZAMD_CHECK_NONE : s->check, s->p + s->len, s->cap - s->len, &w,
				&bi, 1, &nb) == XZAMD_OK && nb == 1);
		s->len += w;
		s->unp[s->nb] = bi.unpadded_size;
	} else {
		/* the writer makes no Block of no bytes: Block Header, the end marker, Block Padding, the Check of nothing */
		const uint32_t hs = xzamd_block_header_size_(1, 0, NULL);
		const uint32_t cb = sha ? 0 : xzamd_check_bytes_(s->check);
		CHECK(s->len + hs + 4 + cb <= s->cap);
		xzamd_block_header_put_(s->p + s->len, hs, 1, 0, 0x00, NULL);
		memset(s->p + s->len + hs, 0, 4 + cb);
		s->len += hs + 4 + cb;
		s->unp[s->nb] = hs + 1 + cb;
	}
	if (sha) {
		CHECK(s->len + 32 <= s->cap);
		stub_sha256(data, usize, s->p + s->len);
		s->len += 32;
		s->unp[s->nb] += 32;
	}
	s->usz[s->nb++] = usize;
}

static uint64_t sb_end(sbuild *s)
{
	s->index_at = s->len;
	const uint64_t w = xzamd_frame_index_footer(s->p + s->len, s->cap - s->len, s->check, s->unp, s->usz, s->nb);
	CHECK(w != 0);
	s->len += w;
	return s->len;
}

/* n bytes in Blocks of block_size */
static uint64_t sb_stream(sbuild *s, uint8_t *buf, uint64_t cap, int check, const uint8_t *data, uint64_t n, uint64_t block_size)
{
	sb_begin(s, buf, cap, check);
	for (uint64_t at = 0; at < n; at += block_size) sb_block(s, data + at, n - at < block_size ? n - at : block_size);
	return sb_end(s);
}

/* ---- the entries; every buffer handed in is an allocation of exactly its size ---- */
static uint8_t *dup_(const uint8_t *p, uint64_t n)
{
	uint8_t *q = (uint8_t *)malloc(n ? n : 1);
	CHECK(q != NULL);
	if (n) memcpy(q, p, n);
	return q;
}

/* Output: one line per case, "NAME | ENTRY rc/blocks [steps] [report] ID | ...", ID naming the trace of the entry's kernel-layer
 * calls; equal traces are printed once, at the end ("t ID: calls", the calls as stub_xzk_dec.c writes them).  The steps: one
 * digit per Block, or digit*count when all are equal.  The report: sSTEP@BLOCK (first bad step and Block, -1 = none), uUNITS,
 * and T when the resume table was used.  The single-byte flips hold the results of their three entries together, so that
 * neighbouring bytes with the same outcome share a line.  Entries: decode / verify / vblocks = xzamd_stream_decode_device /
 * _verify_device / _verify_blocks_device, index / file / range = xzamd_file_index_device / _decode_device / _decode_range_device;
 * +x = with the original. */
static char R[1024];
static size_t Rn;
static struct { uint32_t id; char *text; } *traces;
static size_t ntraces;

static void put(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	const int n = vsnprintf(R + Rn, sizeof(R) - Rn, fmt, ap);
	va_end(ap);
	CHECK(n >= 0 && (size_t)n < sizeof(R) - Rn);
	Rn += (size_t)n;
}
static void head(const char *entry) { put(" | %s", entry); stub_dec_trace_reset(); }
static void tail(const char *name)
{
	const char *t = stub_dec_trace();
	uint32_t id = 2166136261u;                  /* FNV-1a of the trace text */
	for (const char *q = t; *q; ++q) id = (id ^ (uint8_t)*q) * 16777619u;
	size_t i = 0;
	while (i < ntraces && traces[i].id != (id & 0xFFFFFFu)) ++i;
	if (i == ntraces) {
		traces = realloc(traces, (ntraces + 1) * sizeof(*traces));
		CHECK(traces != NULL);
		traces[ntraces].id = id & 0xFFFFFFu;
		traces[ntraces].text = strdup(t);
		CHECK(traces[ntraces++].text != NULL);
	}
	CHECK(strcmp(traces[i].text, t) == 0);
	(void)name;
	put(" %06x", id & 0xFFFFFFu);
}
static void trace_table(void)
{
	for (size_t i = 0; i < ntraces; ++i) {
		printf("t %06x: %s\n", traces[i].id, traces[i].text);
		free(traces[i].text);
	}
	free(traces);
}
/* the case is complete: its line */
static void done(const char *name) { printf("%s%s\n", name, R); Rn = 0; R[0] = 0; }
static void report(void)
{
	xzamd_verify_report r;
	xzamd_get_verify_report(ctx, &r);
	put(" s%u@%lld u%llu%s", r.first_bad_step, (long long)r.first_bad_block, (unsigned long long)r.units, r.table_used ? " T" : "");
}

static int e_decode(const char *name, const uint8_t *xz, uint64_t n, const uint8_t *orig, uint64_t on)
{
	uint8_t *d = dup_(xz, n), *o = orig ? dup_(orig, on) : NULL;
	uint64_t osz = 0, mm = 0, nb = 0;
	head(orig ? "decode+x" : "decode");
	const int rc = xzamd_stream_decode_device(ctx, d, n, outbuf, OUT_CAP, &osz, o, on, &mm, &nb, NULL);
	put(" %d/%llu", rc, (unsigned long long)nb);
	tail(name);
	free(d); free(o);
	return rc;
}

static void e_verify(const char *name, const uint8_t *xz, uint64_t n, const uint8_t *orig, uint64_t on)
{
	uint8_t *d = dup_(xz, n), *o = dup_(orig, on);
	xzamd_verify_report r;
	head("verify");
	const int rc = xzamd_stream_verify_device(ctx, d, n, o, on, &r, NULL);
	put(" %d/%llu", rc, (unsigned long long)r.blocks);
	report();
	tail(name);
	free(d); free(o);
}

static void steps_put(const uint8_t *steps, uint64_t nb)
{
	uint64_t same = 1;
	for (uint64_t b = 1; b < nb; ++b) same &= steps[b] == steps[0];
	if (nb > 4 && same) { put("%u*%llu", steps[0], (unsigned long long)nb); return; }
	for (uint64_t b = 0; b < nb && b < MAXB; ++b) put("%u", steps[b]);
	if (!nb) put("-");
}

static void e_verify_blocks(const char *name, const uint8_t *xz, uint64_t n, const uint8_t *orig, uint64_t on)
{
	uint8_t *d = dup_(xz, n), *o = orig ? dup_(orig, on) : NULL;
	uint8_t steps[MAXB];
	uint64_t nb = 0;
	head(orig ? "vblocks+x" : "vblocks");
	const int rc = xzamd_stream_verify_blocks_device(ctx, d, n, o, orig ? on : 0, steps, MAXB, &nb, NULL, NULL);
	put(" %d/%llu ", rc, (unsigned long long)nb);
	if (rc == XZAMD_OK || rc == XZAMD_DATA_ERROR)
		steps_put(steps, nb);
	report();
	tail(name);
	free(d); free(o);
}

static void e_file_index(const char *name, const uint8_t *xz, uint64_t n)
{
	uint8_t *d = dup_(xz, n);
	static xzamd_xz_stream ss[8];
	static xzamd_xz_block bb[2 * MAXB];
	uint64_t ns = 0, nb = 0, us = 0;
	head("index");
	const int rc = xzamd_file_index_device(ctx, d, n, ss, 8, &ns, bb, 2 * MAXB, &nb, &us);
	put(" %d/%llu/%llu", rc, (unsigned long long)nb, (unsigned long long)ns);
	tail(name);
	free(d);
}

static void e_file_decode(const char *name, const uint8_t *xz, uint64_t n, const uint8_t *orig, uint64_t on)
{
	uint8_t *d = dup_(xz, n), *o = orig ? dup_(orig, on) : NULL;
	uint64_t osz = 0, mm = 0, nb = 0;
	head(orig ? "file+x" : "file");
	const int rc = xzamd_file_decode_device(ctx, d, n, outbuf, OUT_CAP, &osz, o, on, &mm, &nb, NULL);
	put(" %d/%llu", rc, (unsigned long long)nb);
	tail(name);
	free(d); free(o);
}

static void e_range(const char *name, const uint8_t *xz, uint64_t n, uint64_t uoff, uint64_t ulen, const uint8_t *orig, uint64_t on)
{
	uint8_t *d = dup_(xz, n);
	uint64_t osz = 0, nb = 0;
	char entry[96];
	snprintf(entry, sizeof(entry), "range(%llu,%llu)", (unsigned long long)uoff, (unsigned long long)ulen);
	head(entry);
	const int rc = xzamd_file_decode_range_device(ctx, d, n, uoff, ulen, outbuf, OUT_CAP, &osz, &nb, NULL);
	put(" %d/%llu", rc, (unsigned long long)nb);
	if (rc == XZAMD_OK) {
		const uint64_t want = uoff >= on ? 0 : ulen > on - uoff ? on - uoff : ulen;
		CHECK(osz == want && (want == 0 || memcmp(outbuf, orig + uoff, want) == 0));
	}
	tail(name);
	done(name);
	free(d);
}

/* the entries that take nothing but the file */
static void all_plain(const char *name, const uint8_t *xz, uint64_t n)
{
	(void)e_decode(name, xz, n, NULL, 0);
	e_verify_blocks(name, xz, n, NULL, 0);
	e_file_index(name, xz, n);
	e_file_decode(name, xz, n, NULL, 0);
}
/* ... and those that take the original */
static void all_expected(const char *name, const uint8_t *xz, uint64_t n, const uint8_t *orig, uint64_t on)
{
	(void)e_decode(name, xz, n, orig, on);
	e_verify(name, xz, n, orig, on);
	e_verify_blocks(name, xz, n, orig, on);
	e_file_decode(name, xz, n, orig, on);
}

static void le32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i)); }

/* every single-byte flip of [at, at + len) of the Stream: as it is, and with the CRC32 field at crc_at recomputed over
 * [cov, cov + cov_len); runs of bytes with the same results from the three entries are one line */
static void flips(const char *region, const uint8_t *xz, uint64_t n, uint64_t at, uint64_t len, uint64_t crc_at, uint64_t cov, uint64_t cov_len)
{
	static const uint8_t masks[2] = { 0x01, 0x80 };
	uint8_t *m = dup_(xz, n);
	for (int k = 0; k < 2; ++k)
		for (int fix = 0; fix < 2; ++fix) {
			char prev[sizeof(R)] = "";
			uint64_t first = 0;
			for (uint64_t i = 0; i <= len; ++i) {
				if (i < len) {
					memcpy(m, xz, n);
					m[at + i] ^= masks[k];
					if (fix) le32(m + crc_at, xzamd_crc32_host_(m + cov, cov_len));
					(void)e_decode(region, m, n, NULL, 0);
					e_verify_blocks(region, m, n, NULL, 0);
					e_file_decode(region, m, n, NULL, 0);
				}
				if (i && (i == len || strcmp(prev, R) != 0)) {
					printf("flip %s ^%02x%s %llu-%llu%s\n", region, masks[k], fix ? " crcfixed" : "", (unsigned long long)first,
							(unsigned long long)(i - 1), prev);
					first = i;
				}
				memcpy(prev, R, sizeof(R));
				Rn = 0; R[0] = 0;
			}
		}
	free(m);
}

static void reference_file(const char *path)
{
	FILE *f = fopen(path, "rb");
	CHECK(f != NULL);
	uint8_t *xz = (uint8_t *)malloc(1u << 20);
	CHECK(xz != NULL);
	const uint64_t n = fread(xz, 1, 1u << 20, f);
	fclose(f);
	/* the name: the last two components of the path */
	const char *name = path, *slash = NULL;
	for (const char *q = path; *q; ++q)
		if (*q == '/') { if (slash) name = slash + 1; slash = q; }
	all_plain(name, xz, n);
	uint64_t osz = 0, nb = 0;
	uint8_t *d = dup_(xz, n);
	if (xzamd_file_decode_device(ctx, d, n, outbuf, OUT_CAP, &osz, NULL, 0, NULL, &nb, NULL) == XZAMD_OK) {
		uint8_t *orig = dup_(outbuf, osz);
		all_expected(name, xz, n, orig, osz);
		free(orig);
	}
	done(name);
	free(d);
	free(xz);
}

int main(int argc, char **argv)
{
	const uint64_t cap = 3u << 20;
	uint8_t *data = (uint8_t *)malloc(1u << 20), *xz = (uint8_t *)malloc(cap), *cat = (uint8_t *)malloc(cap);
	outbuf = (uint8_t *)malloc(OUT_CAP);
	CHECK(data && xz && cat && outbuf);
	xzamd_corpus_lorem(data, 1u << 20);
	stub_dec_enable();
	CHECK(xzamd_ctx_create(&ctx, 0) == XZAMD_OK);
	sbuild s;
	char name[96];

	for (int i = 1; i < argc; ++i) reference_file(argv[i]);

	/* Streams of 0, 1, 3, 130 stored Blocks (the Index's record count grows a byte at 128) of 1, 4096, 4097 bytes (the last
	 * one shorter where there is room), every Check */
	static const uint64_t counts[4] = { 0, 1, 3, 130 }, sizes[3] = { 1, 4096, 4097 };
	static const int checks[4] = { XZAMD_CHECK_NONE, XZAMD_CHECK_CRC32, XZAMD_CHECK_CRC64, XZAMD_CHECK_SHA256 };
	for (int a = 0; a < 4; ++a)
		for (int b = 0; b < 3; ++b)
			for (int k = 0; k < 4; ++k) {
				const uint64_t n = counts[a] * sizes[b] - (counts[a] > 1 ? sizes[b] / 2 : 0);
				const uint64_t len = sb_stream(&s, xz, cap, checks[k], data, n, sizes[b]);
				CHECK(s.nb == counts[a]);
				snprintf(name, sizeof(name), "stored-%llux%llu-check%d", (unsigned long long)counts[a], (unsigned long long)sizes[b], checks[k]);
				all_plain(name, xz, len);
				all_expected(name, xz, len, data, n);
				done(name);
			}

	/* two and three Streams, Stream Padding 0, 4, 8 between and behind them */
	for (int ns = 2; ns <= 3; ++ns)
		for (uint64_t pad = 0; pad <= 8; pad += 4) {
			uint64_t len = 0, n = 0;
			for (int i = 0; i < ns; ++i) {
				const uint64_t part = i == 1 ? 1 : 2 * 4096 + 100;
				len += sb_stream(&s, cat + len, cap - len, i == 1 ? XZAMD_CHECK_CRC32 : i ? XZAMD_CHECK_SHA256 : XZAMD_CHECK_CRC64, data + n,
						part, 4096);
				n += part;
				memset(cat + len, 0, pad);
				len += pad;
			}
			snprintf(name, sizeof(name), "concat-%d-pad%llu", ns, (unsigned long long)pad);
			all_plain(name, cat, len);
			all_expected(name, cat, len, data, n);
			done(name);
		}

	/* the Stream of the single-defect and verification cases: three Blocks of 4096, 4096, 100 bytes, CRC64 */
	const uint64_t N = 2 * 4096 + 100;
	const uint64_t L = sb_stream(&s, xz, cap, XZAMD_CHECK_CRC64, data, N, 4096);
	{
		const uint64_t hs1 = ((uint64_t)xz[s.hpos[1]] + 1) * 4;
		flips("header", xz, L, 0, 12, 8, 6, 2);
		flips("footer", xz, L, L - 12, 12, L - 12, L - 8, 6);
		flips("index", xz, L, s.index_at, L - 12 - s.index_at, L - 16, s.index_at, L - 16 - s.index_at);
		flips("blockheader1", xz, L, s.hpos[1], hs1, s.hpos[1] + hs1 - 4, s.hpos[1], hs1 - 4);

		/* verification */
		uint8_t *orig = dup_(data, N), *m = dup_(xz, L);
		all_expected("verify-right-original", xz, L, orig, N);
		done("verify-right-original");
		orig[4096 + 17] ^= 0x40;
		all_expected("verify-original-flipped-in-block1", xz, L, orig, N);
		done("verify-original-flipped-in-block1");
		orig[4096 + 17] ^= 0x40;
		all_expected("verify-original-5-short", xz, L, orig, N - 5);
		done("verify-original-5-short");
		m[s.hpos[1] + hs1 + 3 + 1000] ^= 0x04;             /* a byte of Block 1's stored chunk */
		all_expected("verify-payload-flipped", m, L, orig, N);
		all_plain("verify-payload-flipped", m, L);
		done("verify-payload-flipped");
		memcpy(m, xz, L);
		m[s.hpos[1] + hs1] = 0x03;                         /* ... its control byte: LZMA2 data error */
		all_expected("verify-chunk-control-flipped", m, L, orig, N);
		done("verify-chunk-control-flipped");
		memcpy(m, xz, L);
		m[s.hpos[2] - 1] ^= 0x10;                          /* the last byte of Block 1's stored Check */
		all_expected("verify-check-flipped", m, L, orig, N);
		all_plain("verify-check-flipped", m, L);
		done("verify-check-flipped");

		/* the unit table of the first scan overflows for Block 1: a second scan, one unit per Block */
		stub_dec_scan_fail(1);
		(void)e_decode("scan-overflow", xz, L, orig, N);
		stub_dec_scan_fail(1);
		e_verify_blocks("scan-overflow", xz, L, orig, N);
		stub_dec_scan_fail(1);
		e_file_decode("scan-overflow", xz, L, orig, N);
		done("scan-overflow");

		/* ranges: whole Blocks, inside one Block, across two, the whole file, clipped, nothing */
		e_range("range-whole-block1", xz, L, 4096, 4096, data, N);
		e_range("range-whole-blocks01", xz, L, 0, 8192, data, N);
		e_range("range-inside-block0", xz, L, 100, 50, data, N);
		e_range("range-across-blocks01", xz, L, 4000, 200, data, N);
		e_range("range-all", xz, L, 0, N, data, N);
		e_range("range-clipped", xz, L, 8000, 1000, data, N);
		e_range("range-behind-end", xz, L, N, 10, data, N);
		e_range("range-nothing", xz, L, 10, 0, data, N);
		e_range("range-payload-flipped-elsewhere", m, L, 0, 4096, data, N);
		free(orig); free(m);
	}

	/* a Block of no bytes between two others, and alone */
	for (int k = 0; k < 4; ++k) {
		sb_begin(&s, xz, cap, checks[k]);
		sb_block(&s, data, 4096); sb_block(&s, data + 4096, 0); sb_block(&s, data + 4096, 100);
		snprintf(name, sizeof(name), "empty-block-middle-check%d", checks[k]);
		all_plain(name, xz, sb_end(&s));
		all_expected(name, xz, s.len, data, 4196);
		done(name);
		sb_begin(&s, xz, cap, checks[k]);
		sb_block(&s, data, 0);
		snprintf(name, sizeof(name), "empty-block-alone-check%d", checks[k]);
		all_plain(name, xz, sb_end(&s));
		all_expected(name, xz, s.len, data, 0);
		done(name);
	}

	trace_table();
	xzamd_ctx_destroy(ctx);
	xzamd_release_parked();
	stub_dec_trace_free();
	free(data); free(xz); free(cat); free(outbuf);
	printf("driver_decode: ok\n");
	return 0;
}
