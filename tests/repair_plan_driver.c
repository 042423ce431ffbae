/* Stand-alone driver of the repair's splice layout (xzamd_repair_plan_, xz_amd/csrc/xzamd_repair_plan.c) over xzamd_frame.c:
 * synthetic Block tables, every replacement pattern, the gather carried out on host buffers.  Built with
 * -fsanitize=address,undefined by tests/test_host_repair_plan.py and run as a program; prints "repair_plan_driver: ok". */
#include "../xz_amd/csrc/xzamd_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: case %s: CHECK(%s) failed\n", __FILE__, __LINE__, case_name, #cond); ++failures; return; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void)
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return rng_state;
}
static void fill(uint8_t *p, uint64_t n)
{
	uint64_t i = 0;
	for (; i + 8 <= n; i += 8) { const uint64_t v = rnd(); memcpy(p + i, &v, 8); }
	for (; i < n; ++i) p[i] = (uint8_t)rnd();
}
static uint64_t pad4(uint64_t v) { return (v + 3) & ~3ull; }
static int cmp_seg(const void *a, const void *b)
{
	const xzamd_copy_seg *x = (const xzamd_copy_seg *)a, *y = (const xzamd_copy_seg *)b;
	return x->dst < y->dst ? -1 : x->dst > y->dst;
}

/* repl[b]: XZAMD_RP_*; for CODED, delta[b] is added to the old Unpadded Size */
static void run_case(const char *case_name, uint64_t nb, const uint64_t *usize, const uint64_t *unpadded, const uint32_t *repl,
		const int64_t *delta, int check, int framed)
{
	const uint32_t cbytes = xzamd_check_bytes_(check);
	xzamd_rp_block *blocks = (xzamd_rp_block *)calloc(nb, sizeof(*blocks));
	uint64_t pos = framed ? 12 : 0, utotal = 0, scr_total = 0;
	for (uint64_t b = 0; b < nb; ++b) {
		blocks[b].pos = pos; blocks[b].unpadded = unpadded[b]; blocks[b].usize = usize[b]; blocks[b].uoff = utotal;
		blocks[b].repl = repl[b];
		if (repl[b] == XZAMD_RP_CODED) {
			blocks[b].new_unpadded = (uint64_t)((int64_t)unpadded[b] + delta[b]);
			blocks[b].src = scr_total;
			scr_total += pad4(blocks[b].new_unpadded) + 16;
		} else if (repl[b] == XZAMD_RP_STORED) {
			blocks[b].src = scr_total;
			scr_total += 48;
		}
		pos += pad4(unpadded[b]);
		utotal += usize[b];
	}
	const uint64_t old_blocks_end = pos;
	uint8_t *old = (uint8_t *)malloc(old_blocks_end + 1), *scr = (uint8_t *)malloc(scr_total + 1), *orig = (uint8_t *)malloc(utotal + 1);
	fill(old, old_blocks_end); fill(scr, scr_total); fill(orig, utotal);

	xzamd_rp_plan plan;
	const int rc = xzamd_repair_plan_(blocks, nb, check, framed, &plan);
	CHECK(rc == XZAMD_OK);
	uint64_t first = nb;
	for (uint64_t b = 0; b < nb; ++b) if (repl[b] != XZAMD_RP_KEEP) { first = b; break; }
	CHECK(plan.first == first);
	if (first == nb) { CHECK(plan.nsegs == 0); goto out; }
	CHECK(plan.tail_pos == blocks[first].pos && plan.new_size == plan.tail_pos + plan.tail_len);

	/* new offsets: adjacent; Blocks in front of the first replaced one stay */
	for (uint64_t b = 0; b < nb; ++b) {
		if (b < first) CHECK(blocks[b].new_pos == blocks[b].pos && blocks[b].new_unpadded == blocks[b].unpadded);
		if (b + 1 < nb) CHECK(blocks[b + 1].new_pos == blocks[b].new_pos + pad4(blocks[b].new_unpadded));
		if (repl[b] == XZAMD_RP_KEEP) CHECK(blocks[b].new_unpadded == unpadded[b]);
	}
	const uint64_t new_blocks_end = blocks[nb - 1].new_pos + pad4(blocks[nb - 1].new_unpadded);

	/* Index and Footer: what xzamd_frame_index_footer makes of the new records */
	uint64_t frame_len = 0;
	if (framed) {
		uint64_t *rec = (uint64_t *)malloc(16 * nb);
		const uint64_t cap = 64 + 18 * nb;
		uint8_t *ib = (uint8_t *)malloc(cap);
		for (uint64_t b = 0; b < nb; ++b) { rec[b] = blocks[b].new_unpadded; rec[nb + b] = usize[b]; }
		frame_len = xzamd_frame_index_footer(ib, cap, check, rec, rec + nb, nb);
		const int same = frame_len != 0 && plan.frame_len == frame_len && plan.frame_off + frame_len <= plan.lits_len
				&& memcmp(plan.lits + plan.frame_off, ib, frame_len) == 0;
		free(rec); free(ib);
		CHECK(same);
	} else
		CHECK(plan.frame_len == 0);
	CHECK(plan.new_size == new_blocks_end + frame_len);

	/* the segments tile the tail: no gap, no overlap; every source range lies inside its source */
	qsort(plan.segs, plan.nsegs, sizeof(*plan.segs), cmp_seg);
	uint64_t at = 0;
	for (uint64_t i = 0; i < plan.nsegs; ++i) {
		const xzamd_copy_seg *s = &plan.segs[i];
		CHECK(s->dst == at && s->len != 0 && s->len <= XZAMD_RP_SEG_MAX);
		at += s->len;
		const uint64_t lim = s->kind == 0 ? scr_total : s->kind == 1 ? plan.lits_len : s->kind == 2 ? old_blocks_end : utotal;
		CHECK(s->kind <= 3 && s->src <= lim && s->len <= lim - s->src);
		if (s->kind == 2) CHECK(s->src >= plan.tail_pos);
	}
	CHECK(at == plan.tail_len);

	/* carry the gather out and look at what lies at every Block's new place */
	{
		uint8_t *tail = (uint8_t *)malloc(plan.tail_len + 1);
		memset(tail, 0xEE, plan.tail_len);
		for (uint64_t i = 0; i < plan.nsegs; ++i) {
			const xzamd_copy_seg *s = &plan.segs[i];
			const uint8_t *src = s->kind == 0 ? scr : s->kind == 1 ? plan.lits : s->kind == 2 ? old : orig;
			memcpy(tail + s->dst, src + s->src, s->len);
		}
		int ok = 1;
		for (uint64_t b = first; b < nb && ok; ++b) {
			const uint8_t *p = tail + (blocks[b].new_pos - plan.tail_pos);
			if (repl[b] == XZAMD_RP_KEEP) ok = memcmp(p, old + blocks[b].pos, pad4(unpadded[b])) == 0;
			else if (repl[b] == XZAMD_RP_CODED) ok = memcmp(p, scr + blocks[b].src, pad4(blocks[b].new_unpadded)) == 0;
			else {
				/* stored: header of the chain {LZMA2} with both sizes, chunks 0x01 / 0x02 of 64 KiB, end marker, padding, Check */
				const uint64_t csz = usize[b] + ((usize[b] + 65535) / 65536) * 3 + 1;
				const uint32_t hs = xzamd_block_header_size_(csz, usize[b], NULL);
				uint8_t hdr[64];
				xzamd_block_header_put_(hdr, hs, csz, usize[b], 0x00, NULL);
				ok = blocks[b].new_unpadded == hs + csz + cbytes && memcmp(p, hdr, hs) == 0;
				const uint8_t *q = p + hs;
				for (uint64_t ip = 0; ip < usize[b] && ok; ip += 65536) {
					const uint64_t cs = usize[b] - ip < 65536 ? usize[b] - ip : 65536;
					ok = q[0] == (ip ? 0x02 : 0x01) && q[1] == (uint8_t)((cs - 1) >> 8) && q[2] == (uint8_t)(cs - 1)
							&& memcmp(q + 3, orig + blocks[b].uoff + ip, cs) == 0;
					q += 3 + cs;
				}
				ok = ok && *q++ == 0x00;
				while (ok && ((uint64_t)(q - p) & 3)) ok = *q++ == 0;
				ok = ok && memcmp(q, scr + blocks[b].src, cbytes) == 0 && (uint64_t)(q - p) + cbytes == pad4(blocks[b].new_unpadded);
			}
		}
		free(tail);
		CHECK(ok);
	}
out:
	xzamd_repair_plan_free_(&plan);
	free(blocks); free(old); free(scr); free(orig);
}

/* nb Blocks of mixed sizes; pattern(b) says what replaces Block b */
static void family(const char *name, uint64_t nb, uint32_t (*pattern)(uint64_t b, uint64_t nb), int check, int framed, int64_t d)
{
	uint64_t *usize = (uint64_t *)malloc(8 * nb), *unp = (uint64_t *)malloc(8 * nb);
	uint32_t *repl = (uint32_t *)malloc(4 * nb);
	int64_t *delta = (int64_t *)malloc(8 * nb);
	for (uint64_t b = 0; b < nb; ++b) {
		/* sizes around the varint steps 127 | 128 and 16383 | 16384, some past one raw chunk and one gather piece; the last odd */
		static const uint64_t us[6] = { 100, 16380, 70001, 128, 1100000, 16384 };
		usize[b] = (b % 6 == 4 && b != 4 ? 30000 : us[b % 6]) + (b + 1 == nb ? 7 : 0);      /* (one Block of more than 1 MiB per table) */
		unp[b] = 24 + xzamd_check_bytes_(check) + usize[b] / 3 + (b % 5);
		if (b % 7 == 3) unp[b] = 16383 - (b % 2);         /* one byte more and the record's varint grows */
		repl[b] = pattern(b, nb);
		delta[b] = d;
	}
	run_case(name, nb, usize, unp, repl, delta, check, framed);
	free(usize); free(unp); free(repl); free(delta);
}

static uint32_t p_none(uint64_t b, uint64_t nb) { (void)b; (void)nb; return XZAMD_RP_KEEP; }
static uint32_t p_first(uint64_t b, uint64_t nb) { (void)nb; return b == 0 ? XZAMD_RP_CODED : XZAMD_RP_KEEP; }
static uint32_t p_last(uint64_t b, uint64_t nb) { return b + 1 == nb ? XZAMD_RP_CODED : XZAMD_RP_KEEP; }
static uint32_t p_adjacent(uint64_t b, uint64_t nb) { (void)nb; return b == 1 ? XZAMD_RP_CODED : b == 2 ? XZAMD_RP_STORED : XZAMD_RP_KEEP; }
static uint32_t p_every(uint64_t b, uint64_t nb) { (void)nb; return b & 1 ? XZAMD_RP_STORED : XZAMD_RP_CODED; }
static uint32_t p_middle(uint64_t b, uint64_t nb) { return b == nb / 2 ? XZAMD_RP_CODED : XZAMD_RP_KEEP; }
static uint32_t p_stored_first_last(uint64_t b, uint64_t nb) { return b == 0 || b + 1 == nb ? XZAMD_RP_STORED : XZAMD_RP_KEEP; }

int main(void)
{
	static const int checks[3] = { XZAMD_CHECK_NONE, XZAMD_CHECK_CRC64, XZAMD_CHECK_SHA256 };
	static const struct { const char *name; uint32_t (*p)(uint64_t, uint64_t); } pats[7] = {
		{ "none", p_none }, { "first", p_first }, { "last", p_last }, { "adjacent", p_adjacent }, { "every", p_every },
		{ "middle", p_middle }, { "stored first and last", p_stored_first_last } };
	static const int64_t deltas[3] = { 4001, -9, 1 };     /* replacements larger and smaller than the originals */
	static const uint64_t counts[5] = { 1, 3, 5, 127, 128 };     /* 127 -> 128: the Index's record count grows a byte */
	char name[128];
	for (int ci = 0; ci < 3; ++ci)
		for (int pi = 0; pi < 7; ++pi)
			for (int di = 0; di < 3; ++di)
				for (int ni = 0; ni < 5; ++ni)
					for (int framed = 0; framed < 2; ++framed) {
						snprintf(name, sizeof(name), "check %d, %s, delta %lld, %llu Blocks, framed %d", checks[ci], pats[pi].name,
								(long long)deltas[di], (unsigned long long)counts[ni], framed);
						family(name, counts[ni], pats[pi].p, checks[ci], framed, deltas[di]);
					}
	/* a table that is not adjacent is refused */
	{
		xzamd_rp_block two[2];
		xzamd_rp_plan plan;
		memset(two, 0, sizeof(two));
		two[0].pos = 12; two[0].unpadded = 30; two[1].pos = 40; two[1].unpadded = 30; two[1].repl = XZAMD_RP_CODED; two[1].new_unpadded = 40;
		if (xzamd_repair_plan_(two, 2, XZAMD_CHECK_CRC64, 1, &plan) != XZAMD_PROG_ERROR) { fprintf(stderr, "gap in the table accepted\n"); ++failures; }
		two[1].pos = 44;
		if (xzamd_repair_plan_(two, 2, XZAMD_CHECK_CRC64, 1, &plan) != XZAMD_OK || plan.tail_pos != 44) { fprintf(stderr, "adjacent table refused\n"); ++failures; }
		xzamd_repair_plan_free_(&plan);
	}
	if (failures) { fprintf(stderr, "repair_plan_driver: %d failure(s)\n", failures); return 1; }
	printf("repair_plan_driver: ok\n");
	return 0;
}
