/* driver_auto_delta.c -- TEST INFRASTRUCTURE ONLY: the host side of the automatic per-Block delta filter (XZAMD_F_AUTO_DELTA:
 * xz_amd/csrc/xzamd_host.c, xzamd_frame.c, xzamd_options.c) over the CPU stand-ins of the kernel layer (stub_xzk.c,
 * stub_xzk_delta.c), as a stand-alone program under ASan / UBSan (tests/test_host_auto_delta.py).
 *
 * Five Blocks of 128 KiB -- text, an int32 walk, 24-byte records, random bytes, and a short tail of the int32 walk -- so that one
 * job holds Blocks with and without a filter and Block Headers of two sizes.  Checked: the chain and size of every Block Header,
 * that every Block decodes (LZMA2 through the oracle, then the inverse delta) to its input and carries the right Check, the
 * framing of the Stream (xzamd_file_index_host), XZAMD_F_BLOCKS_ONLY (the same Blocks, bare), a Block sent out stored between
 * two filtered ones (no filter in its header), both encode modes of the host layer (single-phase: preset 1, two-phase: preset
 * 6), the analysis on its own, the two debug fetches, and the combinations the flag declines. */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../include/xz_amd.h"
#include "../../oracle/oracle.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

#define BS (128u << 10)
#define NB 5u
#define TAIL 40001u
#define N (4u * BS + TAIL)

extern int stub_delta_force_stored;
extern int stub_delta_calls[3];

static uint32_t rnd_state = 12345;
static uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

static void make_input(uint8_t *in)
{
	xzamd_corpus_lorem(in, BS);
	uint32_t v = 1u << 28;
	for (uint32_t i = 0; i < BS / 4; ++i) { v += rnd() % 2001u - 1000u; put32(in + BS + 4 * i, v); }
	uint32_t f[6] = { 7u << 24, 3u << 20, 9u << 26, 1u << 16, 5u << 22, 11u << 18 };
	for (uint32_t r = 0; r < BS / 24 + 1; ++r)
		for (uint32_t j = 0; j < 6; ++j) {
			f[j] += (j + 1) * 37u + rnd() % 5u;
			uint8_t w[4];
			put32(w, f[j]);
			for (uint32_t k = 0; k < 4 && (uint64_t)r * 24 + 4 * j + k < BS; ++k) in[2 * BS + r * 24 + 4 * j + k] = w[k];
		}
	for (uint32_t i = 0; i < BS; ++i) in[3 * BS + i] = (uint8_t)(rnd() >> 5);
	for (uint32_t i = 0; i < TAIL; ++i) in[4 * BS + i] = in[BS + i];
}

static uint32_t vli_get(const uint8_t *b, uint32_t *p, uint64_t *v)
{
	*v = 0;
	for (uint32_t s = 0; s < 63; s += 7) {
		const uint8_t c = b[(*p)++];
		*v |= (uint64_t)(c & 0x7F) << s;
		if (!(c & 0x80)) return 1;
	}
	return 0;
}

/* Block `bi` inside `buf`: header size, delta distance of its chain (0: {LZMA2}), sizes; decodes to `want`; Check */
static int block_ok(const uint8_t *buf, const xzamd_block_info *bi, uint32_t dict_size, int check, const uint8_t *want, uint32_t usize_want,
		uint32_t *hs_out, uint32_t *dist_out, int *stored_out)
{
	const uint8_t *h = buf + bi->out_offset;
	const uint32_t hs = (h[0] + 1u) * 4u;
	uint32_t p = 2, dist = 0;
	uint64_t csize = 0, usize = 0, id = 0, ps = 0;
	if ((h[1] & 0xC0) != 0xC0 || !vli_get(h, &p, &csize) || !vli_get(h, &p, &usize)) return 0;
	const uint32_t nf = (h[1] & 3u) + 1u;
	for (uint32_t i = 0; i < nf; ++i) {
		if (!vli_get(h, &p, &id) || !vli_get(h, &p, &ps)) return 0;
		if (i + 1 < nf) {
			if (id != 3 || ps != 1 || nf != 2) return 0;
			dist = h[p] + 1u;
		} else if (id != 0x21 || ps != 1) return 0;
		p += (uint32_t)ps;
	}
	if (p > hs - 4 || orc_crc32(h, hs - 4, 0) != (h[hs - 4] | (uint32_t)h[hs - 3] << 8 | (uint32_t)h[hs - 2] << 16 | (uint32_t)h[hs - 1] << 24)) return 0;
	const uint32_t cb = orc_check_size(check);
	if (usize != usize_want || bi->uncompressed_size != usize || bi->unpadded_size != hs + csize + cb
			|| bi->total_size != ((bi->unpadded_size + 3) & ~3ull)) return 0;
	uint8_t *out = (uint8_t *)malloc(usize + 1);
	uint64_t got = 0;
	int ok = orc_lzma2_decode(h + hs, csize, dict_size, out, usize, &got, NULL) == 0 && got == usize;
	for (uint64_t i = dist; ok && dist && i < usize; ++i) out[i] = (uint8_t)(out[i] + out[i - dist]);
	ok = ok && memcmp(out, want, usize) == 0;
	const uint8_t *ck = h + ((hs + csize + 3) & ~3ull);
	if (ok && check == XZAMD_CHECK_CRC64) {
		uint64_t v = 0;
		for (int i = 7; i >= 0; --i) v = v << 8 | ck[i];
		ok = v == orc_crc64(want, usize, 0);
	} else if (ok && check == XZAMD_CHECK_CRC32) {
		ok = (ck[0] | (uint32_t)ck[1] << 8 | (uint32_t)ck[2] << 16 | (uint32_t)ck[3] << 24) == orc_crc32(want, usize, 0);
	}
	free(out);
	*hs_out = hs; *dist_out = dist;
	*stored_out = csize == usize + ((usize + 65535) / 65536) * 3 + 1 && h[hs] == 0x01;
	return ok;
}

int main(void)
{
	xzamd_ctx *ctx = NULL;
	CHECK(xzamd_ctx_create(&ctx, 0) == XZAMD_OK, "ctx");
	if (!ctx) return 1;
	uint8_t *in = (uint8_t *)malloc(N);
	const uint64_t cap = xzamd_stream_buffer_bound(N, BS);
	uint8_t *out = (uint8_t *)malloc(cap), *bare = (uint8_t *)malloc(cap);
	make_input(in);
	static const uint32_t want_dist[NB] = { 0, 4, 24, 0, 4 };

	/* the analysis on its own, and what it leaves to fetch */
	{
		uint32_t dist[NB], fetched[NB];
		uint64_t nb = 0;
		int rc = xzamd_auto_delta_device(ctx, in, N, BS, dist, NB, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == NB, "analysis: rc %d, %llu Blocks", rc, (unsigned long long)nb);
		CHECK(memcmp(dist, want_dist, sizeof(dist)) == 0, "analysis: %u %u %u %u %u", dist[0], dist[1], dist[2], dist[3], dist[4]);
		CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_DELTA_DIST, fetched, sizeof(fetched)) == XZAMD_OK && memcmp(fetched, dist, sizeof(dist)) == 0,
				"fetch of the choices");
		uint32_t *hist = (uint32_t *)malloc(NB * 11 * 256 * 4);
		CHECK(xzamd_debug_fetch(ctx, XZAMD_DEBUG_DELTA_HIST, hist, NB * 11 * 256 * 4) == XZAMD_OK, "fetch of the histograms");
		for (uint32_t b = 0; b < NB; ++b)
			for (uint32_t k = 0; k < 11; ++k) {
				uint64_t s = 0;
				for (uint32_t v = 0; v < 256; ++v) s += hist[(b * 11 + k) * 256 + v];
				CHECK(s == (b < 4 ? 2 * 4096u : 4096u), "samples of Block %u, candidate %u: %llu", b, k, (unsigned long long)s);
			}
		free(hist);
		rc = xzamd_auto_delta_device(ctx, in, N, BS, dist, NB - 1, &nb, NULL);
		CHECK(rc == XZAMD_BUF_ERROR && nb == NB, "analysis into a short table: rc %d", rc);
		CHECK(xzamd_auto_delta_device(ctx, in, N, 0, dist, NB, &nb, NULL) == XZAMD_OPTIONS_ERROR, "analysis with block_size 0");
		nb = 77;
		CHECK(xzamd_auto_delta_device(ctx, in, 0, BS, dist, NB, &nb, NULL) == XZAMD_OK && nb == 0, "analysis of nothing");
	}

	static const int presets[2] = { 1, 6 }, checks[3] = { XZAMD_CHECK_CRC64, XZAMD_CHECK_CRC32, XZAMD_CHECK_NONE };
	for (int pi = 0; pi < 2; ++pi)
		for (int ci = 0; ci < 3; ++ci)
			for (int forced = -1; forced <= (pi == 0 ? 2 : -1); forced += 3) {       /* forced = 2: Block 2 goes out stored (single-phase stub) */
				xzamd_lzma_options opt;
				xzamd_block_info bi[NB], bb[NB];
				uint64_t size = 0, bsize = 0, nb = 0;
				xzamd_stats st;
				xzamd_lzma_preset(&opt, (uint32_t)presets[pi]);
				const int check = checks[ci];
				stub_delta_force_stored = forced;
				memset(stub_delta_calls, 0, sizeof(stub_delta_calls));
				int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, check, XZAMD_F_AUTO_DELTA, out, cap, &size, bi, NB, &nb, NULL);
				CHECK(rc == XZAMD_OK && nb == NB, "encode (preset %d, check %d): rc %d %s", presets[pi], check, rc, xzamd_last_error(ctx));
				if (rc != XZAMD_OK || nb != NB) continue;
				CHECK(stub_delta_calls[0] == 1 && stub_delta_calls[1] == 1 && stub_delta_calls[2] == 1, "one launch of each per batch");
				xzamd_get_stats(ctx, &st);
				CHECK(st.blocks_stored == (forced >= 0 ? 1u : 0u), "stored Blocks: %llu", (unsigned long long)st.blocks_stored);
				uint32_t hs_plain = 0, hs_delta = 0;
				for (uint32_t b = 0; b < NB; ++b) {
					uint32_t hs = 0, dist = 99;
					int stored = 0;
					const int ok = block_ok(out, &bi[b], opt.dict_size, check, in + (uint64_t)b * BS, b + 1 < NB ? BS : TAIL, &hs, &dist, &stored);
					CHECK(ok, "Block %u (preset %d, check %d, forced %d) does not parse or decode", b, presets[pi], check, forced);
					if (!ok) continue;
					/* (the stub coder's payload is stored chunks too: what tells the Block the layout stored is its header
					 * without the filter, and the count in the stats above) */
					CHECK(stored || (int)b != forced, "Block %u does not have the stored form", b);
					CHECK(dist == ((int)b == forced ? 0u : want_dist[b]), "Block %u: delta %u in its header", b, dist);
					if (b < 4 && (int)b != forced) { if (dist) hs_delta = hs; else hs_plain = hs; }
				}
				CHECK(hs_plain != 0 && hs_delta == hs_plain + 4, "header sizes in one job: %u and %u", hs_plain, hs_delta);
				/* the framing: Stream Header, every Block Header and its padding, Index, Footer */
				{
					xzamd_xz_block xb[NB];
					xzamd_xz_stream xs[1];
					uint64_t ns = 0, nbl = 0, usz = 0;
					rc = xzamd_file_index_host(out, size, xs, 1, &ns, xb, NB, &nbl, &usz);
					CHECK(rc == XZAMD_OK && ns == 1 && nbl == NB && usz == N, "index of the Stream: rc %d", rc);
					for (uint32_t b = 0; rc == XZAMD_OK && b < NB; ++b) {
						const uint32_t d = (int)b == forced ? 0 : want_dist[b];
						CHECK(xb[b].filter_count == (d ? 2u : 1u) && xb[b].filter_ids[0] == (d ? 3u : 0x21u) && xb[b].header_offset == bi[b].out_offset,
								"index row of Block %u", b);
					}
				}
				/* the same Blocks, bare */
				rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, check, XZAMD_F_AUTO_DELTA | XZAMD_F_BLOCKS_ONLY, bare, cap, &bsize, bb, NB, &nb, NULL);
				CHECK(rc == XZAMD_OK && nb == NB && bsize <= size - 12 && memcmp(bare, out + 12, bsize) == 0, "blocks only: rc %d", rc);
				for (uint32_t b = 0; rc == XZAMD_OK && b < NB; ++b)
					CHECK(bb[b].out_offset + 12 == bi[b].out_offset && bb[b].unpadded_size == bi[b].unpadded_size, "blocks only: row %u", b);
				/* without the flag: every Block {LZMA2}, the kernels not called */
				stub_delta_force_stored = -1;
				memset(stub_delta_calls, 0, sizeof(stub_delta_calls));
				rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, check, 0, out, cap, &size, bi, NB, &nb, NULL);
				CHECK(rc == XZAMD_OK && stub_delta_calls[0] + stub_delta_calls[1] + stub_delta_calls[2] == 0, "plain encode: rc %d", rc);
				for (uint32_t b = 0; rc == XZAMD_OK && b < NB; ++b) {
					uint32_t hs = 0, dist = 99;
					int stored = 0;
					CHECK(block_ok(out, &bi[b], opt.dict_size, check, in + (uint64_t)b * BS, b + 1 < NB ? BS : TAIL, &hs, &dist, &stored) && dist == 0
							&& hs == hs_plain, "plain encode: Block %u", b);
				}
			}
	stub_delta_force_stored = -1;

	/* several batches in one call: the choices of every batch reach its own layout */
	{
		xzamd_lzma_options opt;
		xzamd_block_info bi[NB];
		uint64_t size = 0, nb = 0;
		xzamd_lzma_preset(&opt, 6);
		CHECK(xzamd_ctx_set_batch_bytes(ctx, 2 * BS) == XZAMD_OK, "batch bytes");
		memset(stub_delta_calls, 0, sizeof(stub_delta_calls));
		int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_DELTA, out, cap, &size, bi, NB, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == NB && stub_delta_calls[0] == 3, "three batches: rc %d, %d launches", rc, stub_delta_calls[0]);
		for (uint32_t b = 0; rc == XZAMD_OK && b < NB; ++b) {
			uint32_t hs = 0, dist = 99;
			int stored = 0;
			CHECK(block_ok(out, &bi[b], opt.dict_size, XZAMD_CHECK_CRC64, in + (uint64_t)b * BS, b + 1 < NB ? BS : TAIL, &hs, &dist, &stored)
					&& dist == want_dist[b], "three batches: Block %u (delta %u)", b, dist);
		}
		CHECK(xzamd_ctx_set_batch_bytes(ctx, 1ull << 30) == XZAMD_OK, "batch bytes");
	}

	/* what the flag declines: XZAMD_OPTIONS_ERROR and a text */
	{
		xzamd_lzma_options opt;
		xzamd_block_info bi[NB];
		uint64_t size = 0, nb = 0;
		xzamd_lzma_preset(&opt, 6);
		static const uint32_t bad[3] = { XZAMD_F_SEGMENTS, XZAMD_F_SINGLE, XZAMD_F_REPAIR };
		for (int i = 0; i < 3; ++i) {
			const int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_DELTA | bad[i], out, cap, &size, bi, NB, &nb, NULL);
			CHECK(rc == XZAMD_OPTIONS_ERROR && strstr(xzamd_last_error(ctx), "auto delta") != NULL, "flag %u: rc %d '%s'", bad[i], rc, xzamd_last_error(ctx));
		}
		opt.bcj = XZAMD_FILTER_DELTA(4);
		int rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_DELTA, out, cap, &size, bi, NB, &nb, NULL);
		CHECK(rc == XZAMD_OPTIONS_ERROR && strstr(xzamd_last_error(ctx), "auto delta") != NULL, "a chain with a filter: rc %d '%s'", rc, xzamd_last_error(ctx));
		opt.bcj = XZAMD_BCJ_X86;
		rc = xzamd_stream_encode_device(ctx, in, N, BS, &opt, XZAMD_CHECK_CRC64, XZAMD_F_AUTO_DELTA, out, cap, &size, bi, NB, &nb, NULL);
		CHECK(rc == XZAMD_OPTIONS_ERROR, "a chain with x86 BCJ: rc %d", rc);
	}

	xzamd_ctx_destroy(ctx);
	free(in); free(out); free(bare);
	if (failures) { printf("driver_auto_delta: %d failure(s)\n", failures); return 1; }
	printf("driver_auto_delta: ok\n");
	return 0;
}
