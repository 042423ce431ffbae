/* chains_plan_driver.c -- stand-alone check of the splice layout of a chain repair (xzamd_chains_plan_,
 * xz_amd/csrc/xzamd_repair_plan.c): pure arithmetic, built with -fsanitize=address,undefined and run as a program.
 *
 * A case is a list of segments (uncompressed size, old chain length, replacement).  The driver fills an old buffer, a scratch
 * buffer and an original with distinct byte patterns, asks for the plan, and checks
 *   - the new offsets and sizes: chains back to back from the first one's place, kept lengths unchanged, coded lengths as given,
 *     stored length = usize + 3 per 64 KiB chunk;
 *   - that the segment list covers the rewritten tail exactly once (no gap, no overlap) and every source range lies inside its
 *     source;
 *   - carrying the gather out on host buffers, that every chain's new place holds the bytes it should: kept -- the old ones;
 *     coded -- the scratch's; stored -- 0x01 + 64 KiB, then 0x02 chunks of the original, no end marker. */
#include "../xz_amd/csrc/xzamd_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

typedef struct { uint64_t usize, len; uint32_t repl; uint64_t new_len; } seg_in;

static uint64_t stored_len(uint64_t usize) { return usize + 3 * ((usize + 65535) / 65536); }

static void run_case(const char *name, const seg_in *in, uint64_t n, uint64_t base)
{
	xzamd_cp_chain *ch = (xzamd_cp_chain *)calloc(n, sizeof(*ch));
	uint64_t old_size = base, orig_size = 0, scr_size = 0;
	for (uint64_t i = 0; i < n; ++i) {
		ch[i].pos = old_size; ch[i].len = in[i].len; ch[i].usize = in[i].usize; ch[i].uoff = orig_size;
		ch[i].repl = in[i].repl;
		if (in[i].repl == XZAMD_RP_CODED) { ch[i].src = scr_size + 16; ch[i].new_len = in[i].new_len; scr_size += 16 + in[i].new_len; }
		old_size += in[i].len;
		orig_size += in[i].usize;
	}
	uint8_t *old = (uint8_t *)malloc(old_size + 1), *orig = (uint8_t *)malloc(orig_size + 1), *scr = (uint8_t *)malloc(scr_size + 1);
	for (uint64_t i = 0; i < old_size; ++i) old[i] = (uint8_t)(i * 7 + 1);
	for (uint64_t i = 0; i < orig_size; ++i) orig[i] = (uint8_t)(i * 13 + 5);
	for (uint64_t i = 0; i < scr_size; ++i) scr[i] = (uint8_t)(i * 3 + 2);

	xzamd_rp_plan plan;
	int rc = xzamd_chains_plan_(ch, n, &plan);
	CHECK(rc == XZAMD_OK, "%s: rc %d", name, rc);
	if (rc != XZAMD_OK) goto out;

	uint64_t first = n;
	for (uint64_t i = 0; i < n; ++i) if (in[i].repl != XZAMD_RP_KEEP) { first = i; break; }
	CHECK(plan.first == first, "%s: first %llu, want %llu", name, (unsigned long long)plan.first, (unsigned long long)first);
	if (first == n) {
		CHECK(plan.nsegs == 0 && plan.tail_len == 0, "%s: a plan without a replacement moves nothing", name);
		for (uint64_t i = 0; i < n; ++i)
			CHECK(ch[i].new_pos == ch[i].pos && ch[i].new_len == ch[i].len, "%s: chain %llu changed", name, (unsigned long long)i);
		goto out;
	}
	/* offsets and sizes */
	uint64_t pos = base;
	for (uint64_t i = 0; i < n; ++i) {
		const uint64_t want = in[i].repl == XZAMD_RP_KEEP ? in[i].len : in[i].repl == XZAMD_RP_CODED ? in[i].new_len : stored_len(in[i].usize);
		CHECK(ch[i].new_pos == pos, "%s: chain %llu at %llu, want %llu", name, (unsigned long long)i, (unsigned long long)ch[i].new_pos,
				(unsigned long long)pos);
		CHECK(ch[i].new_len == want, "%s: chain %llu is %llu bytes, want %llu", name, (unsigned long long)i,
				(unsigned long long)ch[i].new_len, (unsigned long long)want);
		if (i < first) CHECK(ch[i].new_pos == ch[i].pos, "%s: chain %llu in front of the first replaced one moved", name, (unsigned long long)i);
		pos += want;
	}
	CHECK(plan.tail_pos == ch[first].pos, "%s: tail_pos", name);
	CHECK(plan.new_size == pos && plan.tail_len == pos - plan.tail_pos, "%s: new_size %llu, want %llu", name,
			(unsigned long long)plan.new_size, (unsigned long long)pos);
	/* the segment list covers the tail exactly once; sources in range; the gather */
	{
		uint8_t *cover = (uint8_t *)calloc(plan.tail_len + 1, 1), *tail = (uint8_t *)calloc(plan.tail_len + 1, 1);
		for (uint64_t s = 0; s < plan.nsegs; ++s) {
			const xzamd_copy_seg *g = &plan.segs[s];
			const uint8_t *src = g->kind == 0 ? scr : g->kind == 1 ? plan.lits : g->kind == 2 ? old : orig;
			const uint64_t lim = g->kind == 0 ? scr_size : g->kind == 1 ? plan.lits_len : g->kind == 2 ? old_size : orig_size;
			CHECK(g->kind <= 3 && g->len != 0 && g->len <= XZAMD_RP_SEG_MAX, "%s: segment %llu: kind / length", name, (unsigned long long)s);
			CHECK(g->src <= lim && g->len <= lim - g->src, "%s: segment %llu reads outside its source", name, (unsigned long long)s);
			CHECK(g->dst <= plan.tail_len && g->len <= plan.tail_len - g->dst, "%s: segment %llu writes outside the tail", name, (unsigned long long)s);
			if (g->kind > 3 || g->src > lim || g->len > lim - g->src || g->dst > plan.tail_len || g->len > plan.tail_len - g->dst) continue;
			for (uint64_t k = 0; k < g->len; ++k) { ++cover[g->dst + k]; tail[g->dst + k] = src[g->src + k]; }
		}
		uint64_t bad = 0;
		for (uint64_t k = 0; k < plan.tail_len; ++k) bad += cover[k] != 1;
		CHECK(bad == 0, "%s: %llu bytes of the tail are not written exactly once", name, (unsigned long long)bad);
		for (uint64_t i = first; i < n; ++i) {
			const uint8_t *p = tail + (ch[i].new_pos - plan.tail_pos);
			if (ch[i].new_pos < plan.tail_pos || ch[i].new_pos - plan.tail_pos + ch[i].new_len > plan.tail_len) continue;
			if (in[i].repl == XZAMD_RP_KEEP) CHECK(memcmp(p, old + ch[i].pos, ch[i].len) == 0, "%s: kept chain %llu", name, (unsigned long long)i);
			else if (in[i].repl == XZAMD_RP_CODED) CHECK(memcmp(p, scr + ch[i].src, ch[i].new_len) == 0, "%s: coded chain %llu", name, (unsigned long long)i);
			else {
				uint64_t o = 0, ip = 0;
				int ok = 1;
				while (ip < in[i].usize) {
					const uint64_t cs = in[i].usize - ip < 65536 ? in[i].usize - ip : 65536;
					ok &= p[o] == (ip ? 0x02 : 0x01) && p[o + 1] == (uint8_t)((cs - 1) >> 8) && p[o + 2] == (uint8_t)(cs - 1);
					ok &= memcmp(p + o + 3, orig + ch[i].uoff + ip, cs) == 0;
					o += 3 + cs; ip += cs;
				}
				CHECK(ok && o == ch[i].new_len, "%s: stored chain %llu", name, (unsigned long long)i);
			}
		}
		free(cover); free(tail);
	}
out:
	xzamd_repair_plan_free_(&plan);
	free(ch); free(old); free(orig); free(scr);
}

#define K XZAMD_RP_KEEP
#define C XZAMD_RP_CODED
#define S XZAMD_RP_STORED
#define RUN(name, base, ...) do { const seg_in segs_[] = { __VA_ARGS__ }; run_case(name, segs_, sizeof(segs_) / sizeof(segs_[0]), base); } while (0)

int main(void)
{
	const uint64_t M = 1u << 20;
	/* first, middle, last replaced; coded shorter / longer than the old chain; stored */
	RUN("first coded shorter", 0, { M, 300000, C, 250000 }, { M, 310000, K, 0 }, { M, 320000, K, 0 }, { 70000, 20000, K, 0 });
	RUN("first coded longer", 24, { M, 300000, C, 333333 }, { M, 310000, K, 0 }, { M, 320000, K, 0 }, { 70000, 20000, K, 0 });
	RUN("middle coded shorter", 24, { M, 300000, K, 0 }, { M, 310000, C, 1000 }, { M, 320000, K, 0 }, { 70000, 20000, K, 0 });
	RUN("middle coded longer", 24, { M, 300000, K, 0 }, { M, 310000, C, 310001 }, { M, 2 * M, K, 0 }, { 70000, 20000, K, 0 });
	RUN("last coded shorter", 0, { M, 300000, K, 0 }, { M, 310000, K, 0 }, { 70000, 20000, C, 19999 });
	RUN("last coded longer", 0, { M, 300000, K, 0 }, { M, 310000, K, 0 }, { 70000, 20000, C, 70006 });
	RUN("first stored", 24, { M, 300000, S, 0 }, { M, 310000, K, 0 }, { 70000, 20000, K, 0 });
	RUN("middle stored", 24, { M, 300000, K, 0 }, { 65536, 100, S, 0 }, { 65537, 100, K, 0 }, { 70000, 20000, K, 0 });
	RUN("last stored (shorter than the old chain)", 24, { M, 300000, K, 0 }, { 65537, 70000, S, 0 });
	/* adjacent replaced segments, every kind next to every kind */
	RUN("adjacent coded", 24, { M, 300000, K, 0 }, { M, 310000, C, 5 }, { M, 320000, C, 400000 }, { 70000, 20000, K, 0 });
	RUN("adjacent coded + stored", 24, { M, 300000, C, 299999 }, { 100000, 310000, S, 0 }, { M, 320000, C, 17 }, { 70000, 20000, S, 0 });
	RUN("all stored", 0, { 65536, 10, S, 0 }, { 65536, 11, S, 0 }, { 1, 4, S, 0 });
	/* a single segment; a segment of 1 byte */
	RUN("single coded", 24, { M, 300000, C, 123 });
	RUN("single stored", 0, { 3 * 65536 + 1, 300000, S, 0 });
	RUN("single kept", 24, { M, 300000, K, 0 });
	RUN("last of 1 byte stored", 24, { M, 300000, K, 0 }, { 1, 9, S, 0 });
	RUN("last of 1 byte coded", 24, { M, 300000, K, 0 }, { 1, 9, C, 4 });
	RUN("1 byte kept behind a replaced one", 24, { M, 300000, C, 300001 }, { 1, 4, K, 0 });
	RUN("single of 1 byte stored", 0, { 1, 9, S, 0 });
	RUN("nothing replaced", 24, { M, 300000, K, 0 }, { M, 310000, K, 0 });
	/* a table that is not adjacent is refused */
	{
		xzamd_cp_chain ch[2];
		xzamd_rp_plan plan;
		memset(ch, 0, sizeof(ch));
		ch[0].pos = 0; ch[0].len = 10; ch[0].usize = 5; ch[0].repl = XZAMD_RP_STORED;
		ch[1].pos = 11; ch[1].len = 10; ch[1].usize = 5; ch[1].uoff = 5;
		CHECK(xzamd_chains_plan_(ch, 2, &plan) == XZAMD_PROG_ERROR, "a gap between two chains");
		xzamd_repair_plan_free_(&plan);
		ch[1].pos = 10; ch[1].repl = 7;
		CHECK(xzamd_chains_plan_(ch, 2, &plan) == XZAMD_PROG_ERROR, "an unknown replacement kind");
		xzamd_repair_plan_free_(&plan);
	}
	if (failures) { printf("chains_plan_driver: %d failure(s)\n", failures); return 1; }
	printf("chains_plan_driver: ok\n");
	return 0;
}
