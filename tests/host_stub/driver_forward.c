/* driver_forward.c -- TEST INFRASTRUCTURE ONLY: drives the forward reader of the device decoder (xzamd_forward.c) over the CPU
 * stand-ins stub_xzk.c + stub_xzk_dec.c + stub_xzk_walk.c and checks what it delivers against the backward reader
 * (xzamd_file_decode_device over the same stubs) and against the layout of the files it builds.  A program of its own, so that
 * it can be built with sanitizers and simply run (tests/test_host_forward.py); every buffer handed in is an allocation of
 * exactly its size.  Prints one line per group of cases and "driver_forward: ok"; a failed check names its line and exits 1.
 * usage: driver_forward FILE.xz ...      (the reference fixtures; the other cases are made here) */
#include "../../xz_amd/csrc/xzamd_internal.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver_forward: %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_case); exit(1); } } while (0)
#define OUT_CAP (4u << 20)
#define MAXB 160
#define FORMAT_ERROR 7

void stub_dec_enable(void);
void stub_dec_trace_reset(void);
void stub_dec_trace_free(void);
void stub_sha256(const uint8_t *p, uint64_t n, uint8_t out[32]);
uint64_t stub_walk_calls(void);

static xzamd_ctx *ctx;
static uint8_t *outbuf, *outbuf2;
static char g_case[128] = "";

/* ---- Streams of stored Blocks, with or without the sizes in the Block Header ---- */
typedef struct {
	uint8_t *p;
	uint64_t len, cap, nb, index_at;
	int check, nosizes;
	uint64_t unp[MAXB], usz[MAXB], hpos[MAXB], bend[MAXB];
} sbuild;

static void sb_begin(sbuild *s, uint8_t *buf, uint64_t cap, int check, int nosizes)
{
	memset(s, 0, sizeof(*s));
	s->p = buf; s->cap = cap; s->check = check; s->nosizes = nosizes;
	s->len = xzamd_frame_header(buf, check);
}

static void sb_block(sbuild *s, const uint8_t *data, uint64_t usize)
{
	const int sha = s->check == XZAMD_CHECK_SHA256;
	const uint32_t cb = sha ? 32 : xzamd_check_bytes_(s->check);
	xzamd_block_info bi;
	uint64_t w = 0, nb = 0;
	uint8_t *tmp = (uint8_t *)malloc(usize + usize / 1024 + 256);
	CHECK(tmp != NULL && s->nb < MAXB && usize > 0);
	CHECK(xzamd_stored_blocks_host_(data, usize, usize, sha ? XZAMD_CHECK_NONE : s->check, tmp, usize + usize / 1024 + 256, &w, &bi, 1,
			&nb) == XZAMD_OK && nb == 1);
	const uint32_t hs1 = ((uint32_t)tmp[0] + 1) * 4;
	const uint64_t csize = bi.unpadded_size - hs1 - (sha ? 0 : cb);
	uint8_t check_bytes[32];
	if (sha) stub_sha256(data, usize, check_bytes);
	else memcpy(check_bytes, tmp + ((bi.unpadded_size + 3) & ~3ull) - cb, cb);
	/* the Block again: its header (as it is, or the one without sizes), the chunk chain, Block Padding, the Check */
	s->hpos[s->nb] = s->len;
	uint32_t hs = hs1;
	if (s->nosizes) {
		uint8_t h12[12];
		hs = xzamd_block_header_nosizes_(h12, 0x00);
		CHECK(hs == 12 && s->len + hs <= s->cap);
		memcpy(s->p + s->len, h12, hs);
	} else {
		CHECK(s->len + hs <= s->cap);
		memcpy(s->p + s->len, tmp, hs);
	}
	s->len += hs;
	CHECK(s->len + csize + 3 + cb <= s->cap);
	memcpy(s->p + s->len, tmp + hs1, csize);
	s->len += csize;
	while ((s->len - s->hpos[s->nb]) & 3) s->p[s->len++] = 0;
	memcpy(s->p + s->len, check_bytes, cb);
	s->len += cb;
	s->unp[s->nb] = hs + csize + cb;
	s->bend[s->nb] = s->len;
	s->usz[s->nb++] = usize;
	free(tmp);
}

static uint64_t sb_end(sbuild *s)
{
	s->index_at = s->len;
	const uint64_t w = xzamd_frame_index_footer(s->p + s->len, s->cap - s->len, s->check, s->unp, s->usz, s->nb);
	CHECK(w != 0);
	s->len += w;
	return s->len;
}

static uint64_t sb_stream(sbuild *s, uint8_t *buf, uint64_t cap, int check, int nosizes, const uint8_t *data, uint64_t n, uint64_t block_size)
{
	sb_begin(s, buf, cap, check, nosizes);
	for (uint64_t at = 0; at < n; at += block_size) sb_block(s, data + at, n - at < block_size ? n - at : block_size);
	return sb_end(s);
}

static uint8_t *dup_(const uint8_t *p, uint64_t n)
{
	uint8_t *q = (uint8_t *)malloc(n ? n : 1);
	CHECK(q != NULL);
	if (n) memcpy(q, p, n);
	return q;
}

/* the public entry over an exact copy of the file; the output lands in outbuf */
static int forward(const uint8_t *xz, uint64_t n, uint32_t flags, uint64_t *osz, xzamd_forward_report *rp)
{
	uint8_t *d = dup_(xz, n);
	stub_dec_trace_reset();
	const int rc = xzamd_file_decode_forward_device(ctx, d, n, flags, outbuf, OUT_CAP, osz, rp, NULL);
	free(d);
	return rc;
}

static int backward(const uint8_t *xz, uint64_t n, uint64_t *osz, uint64_t *nb)
{
	uint8_t *d = dup_(xz, n);
	stub_dec_trace_reset();
	const int rc = xzamd_file_decode_device(ctx, d, n, outbuf2, OUT_CAP, osz, NULL, 0, NULL, nb, NULL);
	free(d);
	return rc;
}

/* an intact file: the forward reader gives what the backward reader gives -- bytes and Block count */
static void same_as_backward(const uint8_t *xz, uint64_t n, const uint8_t *data, uint64_t dn, uint64_t nstreams)
{
	uint64_t o1 = 0, o2 = 0, nb = 0;
	xzamd_forward_report rp;
	CHECK(backward(xz, n, &o2, &nb) == XZAMD_OK);
	CHECK(forward(xz, n, XZAMD_FWD_CONCATENATED, &o1, &rp) == XZAMD_OK);
	CHECK(o1 == o2 && memcmp(outbuf, outbuf2, o1) == 0);
	CHECK(rp.blocks == nb && rp.blocks_delivered == nb && rp.stop == XZAMD_FWD_END && rp.consumed == n && rp.streams == nstreams);
	if (data) CHECK(o1 == dn && memcmp(outbuf, data, dn) == 0);
}

static void reference_file(const char *path)
{
	FILE *f = fopen(path, "rb");
	CHECK(f != NULL);
	uint8_t *xz = (uint8_t *)malloc(1u << 20);
	CHECK(xz != NULL);
	const uint64_t n = fread(xz, 1, 1u << 20, f);
	fclose(f);
	const char *name = path, *slash = NULL;
	for (const char *q = path; *q; ++q)
		if (*q == '/') { if (slash) name = slash + 1; slash = q; }
	snprintf(g_case, sizeof(g_case), "%s", name);
	uint64_t o1 = 0, o2 = 0, nb = 0;
	xzamd_forward_report rp;
	const int rb = backward(xz, n, &o2, &nb);
	const int rf = forward(xz, n, XZAMD_FWD_CONCATENATED, &o1, &rp);
	printf("%s: backward %d forward %d stop %u blocks %llu/%llu\n", name, rb, rf, rp.stop, (unsigned long long)rp.blocks_delivered,
			(unsigned long long)rp.blocks);
	if (rb == XZAMD_OK) {
		CHECK(rf == XZAMD_OK && o1 == o2 && memcmp(outbuf, outbuf2, o1) == 0 && rp.blocks_delivered == nb && rp.stop == XZAMD_FWD_END);
	} else {
		/* a file the backward reader refuses: the same code, or "the bytes end early" where the defect is a missing end */
		CHECK(rf != XZAMD_OK);
		CHECK(rf == rb || (rf == XZAMD_BUF_ERROR && rp.stop == XZAMD_FWD_TRUNCATED && rb == XZAMD_DATA_ERROR));
		CHECK(rf == XZAMD_BUF_ERROR || (rp.stop == XZAMD_FWD_DEFECT && rp.code == (uint32_t)rf));
	}
	free(xz);
}

/* the step fed in pieces of `piece` bytes: what is not consumed stays in front of the next piece */
static void fed_in_pieces(const uint8_t *xz, uint64_t n, uint64_t piece, uint32_t walk_cap, const uint8_t *data, uint64_t dn, uint64_t nblocks,
		uint64_t *walks_out)
{
	xzamd_forward_state s;
	uint8_t *acc = (uint8_t *)malloc(n ? n : 1);
	uint64_t have = 0, fed = 0, out = 0;
	CHECK(acc != NULL);
	xzamd_forward_init_(&s, XZAMD_FWD_CONCATENATED);
	s.walk_cap = walk_cap;
	for (;;) {
		const uint64_t k = n - fed < piece ? n - fed : piece;
		memcpy(acc + have, xz + fed, k);
		have += k; fed += k;
		uint8_t *d = dup_(acc, have);
		stub_dec_trace_reset();
		const int rc = xzamd_forward_step_(ctx, &s, d, have, fed == n, outbuf + out, OUT_CAP - out, NULL);
		free(d);
		CHECK(rc == XZAMD_OK && s.consumed <= have);
		out += s.produced;
		memmove(acc, acc + s.consumed, have - s.consumed);
		have -= s.consumed;
		if (fed == n) break;
		CHECK(s.stop == XZAMD_FWD_MORE);
	}
	CHECK(s.stop == XZAMD_FWD_END && have == 0 && s.offset == n);
	CHECK(out == dn && memcmp(outbuf, data, dn) == 0 && s.blocks_delivered == nblocks);
	if (walks_out) *walks_out = s.walks;
	xzamd_forward_free_(&s);
	free(acc);
}

static void le32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i)); }

int main(int argc, char **argv)
{
	const uint64_t cap = 3u << 20;
	uint8_t *data = (uint8_t *)malloc(1u << 20), *xz = (uint8_t *)malloc(cap), *cat = (uint8_t *)malloc(cap);
	outbuf = (uint8_t *)malloc(OUT_CAP);
	outbuf2 = (uint8_t *)malloc(OUT_CAP);
	CHECK(data && xz && cat && outbuf && outbuf2);
	xzamd_corpus_lorem(data, 1u << 20);
	stub_dec_enable();
	CHECK(xzamd_ctx_create(&ctx, 0) == XZAMD_OK);
	sbuild s;

	for (int i = 1; i < argc; ++i) reference_file(argv[i]);

	/* a Stream with a filter behind another Stream: its Blocks go through the temporaries of the inverse filters, which a run
	 * addresses from 0 on, while their output lies behind the first Stream's */
	{
		uint64_t len = 0;
		int found = 0;
		for (int pass = 0; pass < 2; ++pass)
			for (int i = 1; i < argc; ++i) {
				const size_t l = strlen(argv[i]);
				const char *want = pass ? "good-1-delta-lzma2.tiff.xz" : "good-1-check-crc32.xz";
				if (l < strlen(want) || strcmp(argv[i] + l - strlen(want), want) != 0) continue;
				FILE *fp = fopen(argv[i], "rb");
				CHECK(fp != NULL);
				len += fread(cat + len, 1, cap - len, fp);
				fclose(fp);
				++found;
			}
		snprintf(g_case, sizeof(g_case), "plain-then-delta");
		if (argc > 1) {
			CHECK(found == 2);
			same_as_backward(cat, len, NULL, 0, 2);
			printf("a {delta, LZMA2} Stream behind a plain one equals the backward reader\n");
		}
	}

	/* Streams of 0, 1, 3, 130 stored Blocks of 1, 4096, 4097 bytes (the last one shorter where there is room), with and
	 * without the sizes in the Block Header, every Check */
	static const uint64_t counts[4] = { 0, 1, 3, 130 }, sizes[3] = { 1, 4096, 4097 };
	static const int checks[4] = { XZAMD_CHECK_NONE, XZAMD_CHECK_CRC32, XZAMD_CHECK_CRC64, XZAMD_CHECK_SHA256 };
	uint64_t cases = 0;
	for (int a = 0; a < 4; ++a)
		for (int b = 0; b < 3; ++b)
			for (int k = 0; k < 4; ++k)
				for (int nosizes = 0; nosizes < 2; ++nosizes) {
					const uint64_t n = counts[a] * sizes[b] - (counts[a] > 1 ? sizes[b] / 2 : 0);
					const uint64_t len = sb_stream(&s, xz, cap, checks[k], nosizes, data, n, sizes[b]);
					CHECK(s.nb == counts[a]);
					snprintf(g_case, sizeof(g_case), "stored-%llux%llu-check%d-nosizes%d", (unsigned long long)counts[a],
							(unsigned long long)sizes[b], checks[k], nosizes);
					const uint64_t w0 = stub_walk_calls();
					same_as_backward(xz, len, data, n, 1);
					CHECK(stub_walk_calls() - w0 == 1);          /* one walk launch per Stream, whatever its Block count */
					++cases;
				}
	printf("stored Streams: %llu cases equal the backward reader\n", (unsigned long long)cases);

	/* two Streams, Stream Padding 0, 4, 8 between and behind them; without XZAMD_FWD_CONCATENATED the read ends behind the first */
	for (uint64_t pad = 0; pad <= 8; pad += 4) {
		uint64_t len = 0, n = 0, first_len = 0;
		for (int i = 0; i < 2; ++i) {
			const uint64_t part = i == 1 ? 1 : 2 * 4096 + 100;
			len += sb_stream(&s, cat + len, cap - len, i ? XZAMD_CHECK_CRC32 : XZAMD_CHECK_CRC64, i, data + n, part, 4096);
			if (i == 0) first_len = len;
			n += part;
			memset(cat + len, 0, pad);
			len += pad;
		}
		snprintf(g_case, sizeof(g_case), "concat-pad%llu", (unsigned long long)pad);
		same_as_backward(cat, len, data, n, 2);
		uint64_t osz = 0;
		xzamd_forward_report rp;
		CHECK(forward(cat, len, 0, &osz, &rp) == XZAMD_OK && osz == 2 * 4096 + 100 && rp.consumed == first_len && rp.streams == 1
				&& rp.stop == XZAMD_FWD_END);
		for (uint64_t piece = 1; piece <= 4099; piece = piece == 1 ? 13 : piece == 13 ? 4099 : 5000)
			fed_in_pieces(cat, len, piece, 0, data, n, 4, NULL);
		/* padding that is no multiple of four, between and behind */
		if (pad == 4) {
			memmove(cat + first_len + 3, cat + first_len + 4, len - first_len - 4);
			CHECK(forward(cat, len - 1, XZAMD_FWD_CONCATENATED, &osz, &rp) == XZAMD_DATA_ERROR && osz == 2 * 4096 + 100 && rp.blocks_delivered == 3);
			CHECK(forward(cat, first_len + 3, XZAMD_FWD_CONCATENATED, &osz, &rp) == XZAMD_DATA_ERROR && osz == 2 * 4096 + 100);
		}
	}
	printf("two Streams with Stream Padding 0 / 4 / 8: equal the backward reader, whole and fed in pieces of 1 / 13 / 4099 bytes\n");

	/* the Stream of the cuts and flips: three Blocks of 4096, 4096, 100 bytes, CRC64; with and without sizes */
	for (int nosizes = 0; nosizes < 2; ++nosizes) {
		const uint64_t N = 2 * 4096 + 100;
		const uint64_t L = sb_stream(&s, xz, cap, XZAMD_CHECK_CRC64, nosizes, data, N, 4096);
		uint64_t osz = 0;
		xzamd_forward_report rp;
		same_as_backward(xz, L, data, N, 1);
		for (uint64_t piece = 1; piece <= 4099; piece = piece == 1 ? 13 : piece == 13 ? 4099 : 5000)
			fed_in_pieces(xz, L, piece, 0, data, N, 3, NULL);

		/* every prefix: exactly the Blocks that lie wholly inside it, XZAMD_BUF_ERROR */
		for (uint64_t cut = 0; cut < L; ++cut) {
			uint64_t nb = 0, un = 0;
			snprintf(g_case, sizeof(g_case), "cut-%llu-nosizes%d", (unsigned long long)cut, nosizes);
			while (nb < 3 && s.bend[nb] <= cut) un += s.usz[nb++];
			CHECK(forward(xz, cut, XZAMD_FWD_CONCATENATED, &osz, &rp) == XZAMD_BUF_ERROR);
			CHECK(rp.stop == XZAMD_FWD_TRUNCATED && rp.blocks_delivered == nb && osz == un && memcmp(outbuf, data, un) == 0);
			CHECK(rp.streams == 0);
		}
		printf("3-Block Stream (sizes in the header: %d): every prefix delivers its whole Blocks with XZAMD_BUF_ERROR\n", !nosizes);

		/* every single-byte flip of Index and Footer, as it is and with the enclosing CRC32 recomputed: all three Blocks are
		 * delivered, then the code of stream_decoder.c -- LZMA_OPTIONS_ERROR for reserved footer flags, LZMA_DATA_ERROR else */
		uint8_t *m = dup_(xz, L);
		static const uint8_t masks[2] = { 0x01, 0x80 };
		uint64_t flips = 0;
		for (uint64_t at = s.index_at; at < L; ++at)
			for (int k = 0; k < 2; ++k)
				for (int fix = 0; fix < 2; ++fix) {
					memcpy(m, xz, L);
					m[at] ^= masks[k];
					const int in_footer = at >= L - 12;
					if (fix && in_footer && at >= L - 8 && at < L - 2) le32(m + L - 12, xzamd_crc32_host_(m + L - 8, 6));
					else if (fix && !in_footer && at < L - 16) le32(m + L - 16, xzamd_crc32_host_(m + s.index_at, L - 16 - s.index_at));
					else if (fix) continue;
					snprintf(g_case, sizeof(g_case), "flip-%llu^%02x-fix%d-nosizes%d", (unsigned long long)(at - s.index_at), masks[k], fix, nosizes);
					const int rc = forward(m, L, XZAMD_FWD_CONCATENATED, &osz, &rp);
					const int want = fix && in_footer && (at == L - 4 || (at == L - 3 && masks[k] == 0x80)) ? XZAMD_OPTIONS_ERROR : XZAMD_DATA_ERROR;
					/* (a first Index byte that is no longer 0x00 reads as the size byte of a Block Header: of 8 bytes, whose CRC32 fails, or
					 * of 516, which the file does not have: the input ends early, as for the reference) */
					if (at == s.index_at && masks[k] == 0x80) CHECK(rc == XZAMD_BUF_ERROR && rp.stop == XZAMD_FWD_TRUNCATED);
					else CHECK(rc == want && rp.stop == XZAMD_FWD_DEFECT && rp.code == (uint32_t)want);
					CHECK(rp.blocks_delivered == 3 && osz == N && memcmp(outbuf, data, N) == 0);
					++flips;
				}
		free(m);
		printf("3-Block Stream (sizes in the header: %d): %llu flips of Index and Footer deliver three Blocks, then the defect's code\n",
				!nosizes, (unsigned long long)flips);
	}

	/* damage inside the Blocks: payload, chunk control byte, stored Check of Block 1 -> Block 0 is delivered */
	{
		const uint64_t N = 2 * 4096 + 100;
		const uint64_t L = sb_stream(&s, xz, cap, XZAMD_CHECK_CRC64, 0, data, N, 4096);
		const uint64_t hs1 = ((uint64_t)xz[s.hpos[1]] + 1) * 4;
		const uint64_t at[3] = { s.hpos[1] + hs1 + 3 + 1000, s.hpos[1] + hs1, s.hpos[2] - 1 };
		for (int i = 0; i < 3; ++i) {
			uint8_t *m = dup_(xz, L);
			uint64_t osz = 0;
			xzamd_forward_report rp;
			snprintf(g_case, sizeof(g_case), "damage-%d", i);
			if (i == 1) m[at[i]] = 0x03; else m[at[i]] ^= 0x10;
			CHECK(forward(m, L, XZAMD_FWD_CONCATENATED, &osz, &rp) == XZAMD_DATA_ERROR);
			CHECK(rp.stop == XZAMD_FWD_DEFECT && rp.blocks_delivered == 1 && osz == 4096 && memcmp(outbuf, data, 4096) == 0);
			CHECK(rp.stop_offset == s.hpos[1]);
			free(m);
		}
		/* an output buffer that holds two Blocks of the three */
		uint8_t *d = dup_(xz, L);
		uint64_t osz = 0;
		xzamd_forward_report rp;
		snprintf(g_case, sizeof(g_case), "out-full");
		CHECK(xzamd_file_decode_forward_device(ctx, d, L, XZAMD_FWD_CONCATENATED, outbuf, 8192 + 50, &osz, &rp, NULL) == XZAMD_BUF_ERROR);
		CHECK(rp.stop == XZAMD_FWD_OUT_FULL && rp.blocks_delivered == 2 && osz == 8192 && memcmp(outbuf, data, 8192) == 0);
		free(d);
		printf("damage inside Block 1 delivers Block 0; a short output buffer delivers the Blocks that fit\n");
	}

	/* a walk table of two rows over five Blocks: three launches */
	for (int nosizes = 0; nosizes < 2; ++nosizes) {
		const uint64_t N = 4 * 4096 + 7;
		const uint64_t L = sb_stream(&s, xz, cap, XZAMD_CHECK_CRC32, nosizes, data, N, 4096);
		uint64_t walks = 0;
		snprintf(g_case, sizeof(g_case), "relaunch-nosizes%d", nosizes);
		CHECK(s.nb == 5);
		fed_in_pieces(xz, L, L, 2, data, N, 5, &walks);
		CHECK(walks == 3);
	}
	printf("a walk table of 2 rows over 5 Blocks: 3 launches\n");

	/* the first twelve bytes: no magic is LZMA_FORMAT_ERROR, a flipped flag byte a data error (CRC32) */
	{
		const uint64_t L = sb_stream(&s, xz, cap, XZAMD_CHECK_CRC64, 0, data, 100, 4096);
		uint64_t osz = 0;
		xzamd_forward_report rp;
		uint8_t *m = dup_(xz, L);
		snprintf(g_case, sizeof(g_case), "header");
		m[0] ^= 1;
		CHECK(forward(m, L, 0, &osz, &rp) == FORMAT_ERROR && osz == 0 && rp.stop == XZAMD_FWD_DEFECT);
		m[0] ^= 1; m[7] ^= 1;
		CHECK(forward(m, L, 0, &osz, &rp) == XZAMD_DATA_ERROR && osz == 0);
		m[6] = 1; m[7] = 4; le32(m + 8, xzamd_crc32_host_(m + 6, 2));
		CHECK(forward(m, L, 0, &osz, &rp) == XZAMD_OPTIONS_ERROR && osz == 0);
		m[6] = 0; m[7] = 2; le32(m + 8, xzamd_crc32_host_(m + 6, 2));
		CHECK(forward(m, L, 0, &osz, &rp) == XZAMD_UNSUPPORTED_CHECK && osz == 0);
		free(m);
	}

	xzamd_ctx_destroy(ctx);
	xzamd_release_parked();
	stub_dec_trace_free();
	free(data); free(xz); free(cat); free(outbuf); free(outbuf2);
	printf("driver_forward: ok\n");
	return 0;
}
