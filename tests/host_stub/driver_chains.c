/* driver_chains.c -- TEST INFRASTRUCTURE ONLY: the host code of the bare chunk chains (xz_amd/csrc/xzamd_chains.c: the chain
 * table, verdicts, repair, splice, the framing of XZAMD_F_SINGLE) over the CPU stand-ins of the kernel layer (stub_xzk.c,
 * stub_xzk_dec.c, stub_xzk_chains.c), as a stand-alone program under ASan / UBSan (tests/test_host_chains.py).
 *
 * Two kinds of chains: those the batch encoder writes over the stubs (XZAMD_F_SEGMENTS; the stub coder emits stored chunks), and
 * coded ones made here with the oracle's fast-mode encoder (its Block payload with the end marker cut), which a repair over
 * the stubs can only replace by longer, stored ones -- the way to XZAMD_BUF_ERROR. */
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

#define SEG 65536u
#define NSEG 3u

static xzamd_ctx *ctx;
static xzamd_lzma_options opt;

static int verify(const uint8_t *chains, uint64_t size, const xzamd_block_info *bi, int check, const uint8_t *orig, uint64_t n,
		uint8_t steps[NSEG], xzamd_verify_report *rp)
{
	memset(steps, 0xEE, NSEG);
	return xzamd_chains_verify_device(ctx, chains, size, bi, NSEG, &opt, check, orig, n, steps, NSEG, rp, NULL);
}

#define STEPS_ARE(a, b, c) (steps[0] == (a) && steps[1] == (b) && steps[2] == (c))

/* the concatenated chains and one end marker are one LZMA2 stream that decodes to the data */
static int chains_decode_to(const uint8_t *chains, uint64_t size, const uint8_t *data, uint64_t n)
{
	uint8_t *tmp = (uint8_t *)malloc(size + 1), *out = (uint8_t *)malloc(n + 1);
	uint64_t got = 0;
	memcpy(tmp, chains, size);
	tmp[size] = 0;
	const int r = orc_lzma2_decode(tmp, size + 1, opt.dict_size, out, n, &got, NULL);
	const int ok = r == 0 && got == n && memcmp(out, data, n) == 0;
	free(tmp); free(out);
	return ok;
}

static void stub_coded_chains(const uint8_t *data, uint64_t n)
{
	const uint64_t cap = xzamd_stream_buffer_bound(n, SEG);
	uint8_t *chains = (uint8_t *)malloc(cap), *copy = (uint8_t *)malloc(cap), *other = (uint8_t *)malloc(n);
	xzamd_block_info bi[NSEG], b2[NSEG];
	xzamd_verify_report rp;
	uint8_t steps[NSEG];
	uint64_t size = 0, nb = 0;
	for (int check = 0; check <= 4; check += check ? 3 : 1) {           /* none, CRC32, CRC64 */
		int rc = xzamd_stream_encode_device(ctx, data, n, SEG, &opt, check, XZAMD_F_SEGMENTS, chains, cap, &size, bi, NSEG, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == NSEG, "segments encode (check %d): rc %d, %llu segments", check, rc, (unsigned long long)nb);
		if (rc != XZAMD_OK || nb != NSEG) continue;
		CHECK(chains_decode_to(chains, size, data, n), "the chains of the stub encode do not decode (check %d)", check);
		/* a good table, with and without the original */
		rc = verify(chains, size, bi, check, data, n, steps, &rp);
		CHECK(rc == XZAMD_OK && STEPS_ARE(0, 0, 0) && rp.blocks == NSEG && rp.first_bad_step == XZAMD_VSTEP_NONE && rp.first_bad_block == UINT64_MAX,
				"good chains (check %d): rc %d, steps %u %u %u", check, rc, steps[0], steps[1], steps[2]);
		rc = verify(chains, size, bi, check, NULL, 0, steps, &rp);
		CHECK(rc == XZAMD_OK && STEPS_ARE(0, 0, 0), "good chains without the original (check %d): rc %d", check, rc);
		/* a chain cut one byte short */
		memcpy(b2, bi, sizeof(bi));
		b2[1].total_size -= 1;
		rc = verify(chains, size, b2, check, data, n, steps, &rp);
		CHECK(rc == XZAMD_DATA_ERROR && STEPS_ARE(0, XZAMD_VSTEP_GRAMMAR, 0) && rp.first_bad_block == 1 && rp.first_bad_step == XZAMD_VSTEP_GRAMMAR,
				"chain cut short (check %d): rc %d, steps %u %u %u", check, rc, steps[0], steps[1], steps[2]);
		/* ... and the last one, whose end is the end of the buffer: a row may not name a byte outside it */
		memcpy(b2, bi, sizeof(bi));
		b2[2].total_size += 1;
		rc = verify(chains, size, b2, check, data, n, steps, &rp);
		CHECK(rc == XZAMD_PROG_ERROR, "a row that names a byte behind the buffer: rc %d", rc);
		/* a 0x00 in the middle: the control byte of the second chunk of chain 1 (the stub coder's chunks hold 48 KiB) */
		memcpy(copy, chains, size);
		CHECK(copy[bi[1].out_offset + 3 + 49152] == 0x02, "layout of the stub coder's chunks");
		copy[bi[1].out_offset + 3 + 49152] = 0x00;
		rc = verify(copy, size, bi, check, data, n, steps, &rp);
		CHECK(rc == XZAMD_DATA_ERROR && STEPS_ARE(0, XZAMD_VSTEP_GRAMMAR, 0), "0x00 inside a chain (check %d): rc %d, steps %u %u %u", check, rc,
				steps[0], steps[1], steps[2]);
		/* a chain that does not start with a dictionary reset */
		memcpy(copy, chains, size);
		copy[bi[2].out_offset] = 0x02;
		rc = verify(copy, size, bi, check, data, n, steps, &rp);
		CHECK(rc == XZAMD_DATA_ERROR && STEPS_ARE(0, 0, XZAMD_VSTEP_GRAMMAR), "no dictionary reset (check %d): rc %d", check, rc);
		if (check != XZAMD_CHECK_NONE) {
			/* a wrong CRC in the table */
			memcpy(b2, bi, sizeof(bi));
			b2[2].unpadded_size ^= 0x100;
			rc = verify(chains, size, b2, check, data, n, steps, &rp);
			CHECK(rc == XZAMD_DATA_ERROR && STEPS_ARE(0, 0, XZAMD_VSTEP_CHECK) && rp.first_bad_step == XZAMD_VSTEP_CHECK && rp.first_bad_block == 2,
					"wrong binfo CRC (check %d): rc %d, steps %u %u %u", check, rc, steps[0], steps[1], steps[2]);
		}
		/* a wrong original */
		memcpy(other, data, n);
		other[100] ^= 0x40;
		rc = verify(chains, size, bi, check, other, n, steps, &rp);
		CHECK(rc == XZAMD_DATA_ERROR && STEPS_ARE(XZAMD_VSTEP_COMPARE, 0, 0) && rp.first_bad_step == XZAMD_VSTEP_COMPARE,
				"wrong original (check %d): rc %d, steps %u %u %u", check, rc, steps[0], steps[1], steps[2]);
		rc = verify(chains, size, bi, check, data, n - 1, steps, &rp);
		CHECK(rc == XZAMD_DATA_ERROR && rp.first_bad_step == XZAMD_VSTEP_COMPARE, "original of another size (check %d): rc %d", check, rc);
		/* steps_cap */
		rc = xzamd_chains_verify_device(ctx, chains, size, bi, NSEG, &opt, check, data, n, steps, NSEG - 1, &rp, NULL);
		CHECK(rc == XZAMD_BUF_ERROR && rp.blocks == NSEG, "steps_cap too small: rc %d", rc);
	}
	CHECK(xzamd_chains_verify_device(ctx, chains, size, bi, NSEG, &opt, XZAMD_CHECK_SHA256, data, n, steps, NSEG, NULL, NULL) == XZAMD_OPTIONS_ERROR,
			"SHA-256 cannot be the Check of a segment");
	free(chains); free(copy); free(other);
}

static void oracle_coded_chains(const uint8_t *data, uint64_t n)
{
	orc_enc_params p;
	uint8_t *chains = (uint8_t *)malloc(2 * n + 4096), *copy = (uint8_t *)malloc(2 * n + 4096), *before = (uint8_t *)malloc(2 * n + 4096);
	xzamd_block_info bi[NSEG], b2[NSEG];
	xzamd_verify_report rp;
	xzamd_repair_report rr;
	uint8_t steps[NSEG];
	uint64_t size = 0, ns = 0;
	int rc;
	memset(&p, 0, sizeof(p));
	p.dict_size = 1u << 20; p.lc = 3; p.pb = 2; p.nice_len = 32; p.mf = 4;
	for (uint32_t s = 0; s < NSEG; ++s) {
		const uint64_t off = (uint64_t)s * SEG, len = n - off < SEG ? n - off : SEG;
		uint64_t got = 0;
		rc = orc_lzma2_encode_block(data + off, (uint32_t)len, &p, chains + size, 2 * n + 4096 - size, &got, NULL);
		CHECK(rc == 0 && got > 1 && chains[size + got - 1] == 0x00, "oracle encode of segment %u: %d", s, rc);
		bi[s].out_offset = size; bi[s].total_size = got - 1;        /* (the end marker is cut) */
		bi[s].uncompressed_size = len; bi[s].unpadded_size = orc_crc64(data + off, len, 0);
		size += got - 1;
	}
	CHECK(size < n / 2, "the coded chains are much shorter than the data");
	CHECK(chains_decode_to(chains, size, data, n), "the oracle's chains do not decode");
	rc = verify(chains, size, bi, XZAMD_CHECK_CRC64, data, n, steps, &rp);
	CHECK(rc == XZAMD_OK && STEPS_ARE(0, 0, 0), "good coded chains: rc %d, steps %u %u %u", rc, steps[0], steps[1], steps[2]);

	/* no bad segment: the repair is one pass and changes nothing */
	memcpy(copy, chains, size);
	memcpy(b2, bi, sizeof(bi));
	rc = xzamd_chains_repair_device(ctx, copy, size, size, b2, NSEG, &opt, XZAMD_CHECK_CRC64, data, n, &ns, &rr, NULL);
	CHECK(rc == XZAMD_OK && ns == size && rr.blocks == NSEG && rr.blocks_bad == 0 && rr.passes == 1 && memcmp(copy, chains, size) == 0
			&& memcmp(b2, bi, sizeof(bi)) == 0, "repair of good chains: rc %d", rc);

	/* a flipped byte in the middle of chain 1 */
	memcpy(copy, chains, size);
	copy[bi[1].out_offset + bi[1].total_size / 2] ^= 0x5A;
	rc = verify(copy, size, bi, XZAMD_CHECK_CRC64, data, n, steps, &rp);
	CHECK(rc == XZAMD_DATA_ERROR && steps[0] == 0 && steps[1] != 0 && steps[2] == 0 && rp.first_bad_block == 1,
			"tampered chain: rc %d, steps %u %u %u", rc, steps[0], steps[1], steps[2]);
	/* all or nothing: over the stubs the replacement is stored chunks, longer than the coded chain -- it does not fit */
	memcpy(before, copy, size);
	memcpy(b2, bi, sizeof(bi));
	const uint64_t stored_len = bi[1].uncompressed_size + 3 * ((bi[1].uncompressed_size + 65535) / 65536);
	const uint64_t want = size - bi[1].total_size + stored_len;
	rc = xzamd_chains_repair_device(ctx, copy, size, want - 1, b2, NSEG, &opt, XZAMD_CHECK_CRC64, data, n, &ns, &rr, NULL);
	CHECK(rc == XZAMD_BUF_ERROR && ns == want, "repair into a buffer one byte short: rc %d, new_size %llu, want %llu", rc,
			(unsigned long long)ns, (unsigned long long)want);
	CHECK(memcmp(copy, before, size) == 0 && memcmp(b2, bi, sizeof(bi)) == 0, "XZAMD_BUF_ERROR left chains or binfo changed");
	/* ... and with the byte it goes through */
	rc = xzamd_chains_repair_device(ctx, copy, size, want, b2, NSEG, &opt, XZAMD_CHECK_CRC64, data, n, &ns, &rr, NULL);
	CHECK(rc == XZAMD_OK && ns == want && rr.blocks_bad == 1 && rr.blocks_reencoded + rr.blocks_stored == 1 && rr.passes >= 3
			&& rr.size_before == size && rr.size_after == want, "repair: rc %d (%s)", rc, xzamd_last_error(ctx));
	if (rc == XZAMD_OK) {
		CHECK(b2[0].out_offset == bi[0].out_offset && b2[0].total_size == bi[0].total_size && b2[1].out_offset == bi[1].out_offset
				&& b2[1].total_size == stored_len && b2[2].out_offset == bi[2].out_offset + stored_len - bi[1].total_size
				&& b2[2].total_size == bi[2].total_size, "binfo after the repair");
		for (uint32_t s = 0; s < NSEG; ++s)
			CHECK(b2[s].unpadded_size == bi[s].unpadded_size && b2[s].uncompressed_size == bi[s].uncompressed_size, "CRC / size of segment %u moved", s);
		CHECK(memcmp(copy, chains, bi[1].out_offset) == 0, "chain 0 changed");
		CHECK(memcmp(copy + b2[2].out_offset, chains + bi[2].out_offset, bi[2].total_size) == 0, "chain 2 is not the bytes it was");
		CHECK(copy[b2[1].out_offset] == 0x01, "the replacement starts with a dictionary reset");
		CHECK(chains_decode_to(copy, ns, data, n), "the repaired chains do not decode to the data");
		rc = verify(copy, ns, b2, XZAMD_CHECK_CRC64, data, n, steps, &rp);
		CHECK(rc == XZAMD_OK && STEPS_ARE(0, 0, 0), "repaired chains: rc %d", rc);
	}
	/* the knobs: segments 0 and 2 rejected, straight to the stored rung */
	setenv("XZAMD_TEST_REPAIR_REJECT", "0,2", 1);
	setenv("XZAMD_TEST_REPAIR_RUNG", "2", 1);
	memcpy(copy, chains, size);
	memcpy(b2, bi, sizeof(bi));
	rc = xzamd_chains_repair_device(ctx, copy, size, 2 * n + 4096, b2, NSEG, &opt, XZAMD_CHECK_CRC64, data, n, &ns, &rr, NULL);
	unsetenv("XZAMD_TEST_REPAIR_REJECT");
	unsetenv("XZAMD_TEST_REPAIR_RUNG");
	CHECK(rc == XZAMD_OK && rr.blocks_bad == 2 && rr.blocks_stored == 2 && rr.blocks_reencoded == 0, "forced repair: rc %d (%s)", rc,
			xzamd_last_error(ctx));
	if (rc == XZAMD_OK) {
		CHECK(b2[1].total_size == bi[1].total_size && memcmp(copy + b2[1].out_offset, chains + bi[1].out_offset, bi[1].total_size) == 0,
				"the good chain between two replaced ones is not the bytes it was");
		CHECK(b2[2].out_offset + b2[2].total_size == ns && chains_decode_to(copy, ns, data, n), "forced repair: the chains do not decode");
	}
	/* a table whose chains do not lie back to back is no table of a repair */
	memcpy(b2, bi, sizeof(bi));
	b2[1].out_offset += 1;
	rc = xzamd_chains_repair_device(ctx, copy, size, size, b2, NSEG, &opt, XZAMD_CHECK_CRC64, data, n, &ns, &rr, NULL);
	CHECK(rc == XZAMD_PROG_ERROR, "repair of a table with a gap: rc %d", rc);
	free(chains); free(copy); free(before);
}

static void single_streams(const uint8_t *data, uint64_t n)
{
	const uint64_t cap = xzamd_stream_buffer_bound(n, SEG) + 64;
	uint8_t *xz = (uint8_t *)malloc(cap), *out = (uint8_t *)malloc(n + 1);
	xzamd_block_info bi[NSEG];
	for (int check = 0; check <= 4; check += check ? 3 : 1) {
		uint64_t size = 0, nb = 0, got = 0, blocks = 0;
		int rc = xzamd_stream_encode_device(ctx, data, n, SEG, &opt, check, XZAMD_F_SINGLE, xz, cap, &size, bi, NSEG, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == NSEG, "single (check %d): rc %d (%s)", check, rc, xzamd_last_error(ctx));
		if (rc != XZAMD_OK) continue;
		rc = orc_xz_decode(xz, size, out, n, &got, &blocks);
		CHECK(rc == 0 && got == n && blocks == 1 && memcmp(out, data, n) == 0, "single (check %d): the oracle's decode says %d", check, rc);
		CHECK(bi[0].out_offset == 24 && bi[1].out_offset == 24 + bi[0].total_size, "single: offsets of the segments inside the Stream");
		rc = xzamd_stream_encode_device(ctx, data, 0, SEG, &opt, check, XZAMD_F_SINGLE, xz, cap, &size, bi, NSEG, &nb, NULL);
		CHECK(rc == XZAMD_OK && nb == 0 && size == 32, "single, no input (check %d): rc %d, %llu bytes", check, rc, (unsigned long long)size);
		rc = orc_xz_decode(xz, size, out, n, &got, &blocks);
		CHECK(rc == 0 && got == 0 && blocks == 0, "single, no input (check %d): the oracle's decode says %d", check, rc);
	}
	uint64_t size = 0, nb = 0;
	CHECK(xzamd_stream_encode_device(ctx, data, n, SEG, &opt, 4, XZAMD_F_SINGLE | XZAMD_F_BLOCKS_ONLY, xz, cap, &size, bi, NSEG, &nb, NULL)
			== XZAMD_OPTIONS_ERROR, "single | blocks_only");
	CHECK(xzamd_stream_encode_device(ctx, data, n, SEG, &opt, 4, XZAMD_F_SINGLE | XZAMD_F_SEGMENTS, xz, cap, &size, bi, NSEG, &nb, NULL)
			== XZAMD_OPTIONS_ERROR, "single | segments");
	CHECK(xzamd_stream_encode_device(ctx, data, n, SEG, &opt, XZAMD_CHECK_SHA256, XZAMD_F_SINGLE, xz, cap, &size, bi, NSEG, &nb, NULL)
			== XZAMD_OPTIONS_ERROR, "single with SHA-256");
	CHECK(xzamd_stream_encode_device(ctx, data, n, SEG, &opt, 4, 0x80000000u | XZAMD_F_SEGMENTS | XZAMD_F_REPAIR, xz, cap, &size, bi, NSEG, &nb, NULL)
			== XZAMD_OPTIONS_ERROR, "the internal flag from outside");
	CHECK(xzamd_stream_encode_device(ctx, data, n, SEG, &opt, 4, XZAMD_F_SEGMENTS | XZAMD_F_REPAIR, xz, cap, &size, bi, NSEG, &nb, NULL)
			== XZAMD_OPTIONS_ERROR, "segments | repair");
	CHECK(xzamd_stream_encode_device(ctx, data, n, SEG, &opt, 4, XZAMD_F_SINGLE, xz, 30, &size, bi, NSEG, &nb, NULL) == XZAMD_BUF_ERROR,
			"single into a buffer of 30 bytes");
	free(xz); free(out);
}

int main(void)
{
	const uint64_t n = 2 * SEG + 30001;       /* three segments, the last one short and odd */
	uint8_t *data = (uint8_t *)malloc(n);
	xzamd_corpus_lorem(data, n);
	if (xzamd_lzma_preset(&opt, 6) || xzamd_ctx_create(&ctx, 0) != XZAMD_OK) { printf("driver_chains: no context\n"); return 1; }
	stub_coded_chains(data, n);
	oracle_coded_chains(data, n);
	single_streams(data, n);
	xzamd_ctx_destroy(ctx);
	free(data);
	if (failures) { printf("driver_chains: %d failure(s)\n", failures); return 1; }
	printf("driver_chains: ok\n");
	return 0;
}
