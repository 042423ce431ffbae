/*
 * xzamd_repair_plan.c -- the splice layout of a repair (DESIGN.md 3.6 "Repair"): from the old Block table, what replaces
 * which Block and the Check to the new offsets, the Index and Stream Footer bytes and the segment list of the gather.
 * Pure arithmetic over xzamd_frame.c: no device call and no context, so a stand-alone program can test it.
 *
 * The Stream is rewritten from the first replaced Block on.  The plan describes that tail: destinations are offsets from
 * tail_pos, because the gather writes a temporary that is copied over the Stream in one piece -- nothing moves in place.
 */
#include "xzamd_internal.h"

#include <stdlib.h>
#include <string.h>

typedef struct {
	xzamd_rp_plan *p;
	uint64_t segs_cap, lits_cap;
	int oom;
} builder;

static void seg_put(builder *B, uint32_t kind, uint64_t src, uint64_t len, uint64_t dst)
{
	xzamd_rp_plan *p = B->p;
	if (len == 0 || B->oom) return;
	if (p->nsegs == B->segs_cap) {
		const uint64_t cap = B->segs_cap ? 2 * B->segs_cap : 64;
		xzamd_copy_seg *s = (xzamd_copy_seg *)realloc(p->segs, cap * sizeof(*s));
		if (!s) { B->oom = 1; return; }
		p->segs = s; B->segs_cap = cap;
	}
	xzamd_copy_seg *s = &p->segs[p->nsegs++];
	s->src = src; s->dst = dst; s->len = len; s->kind = kind; s->pad_ = 0;
}

/* literal bytes: packed back to back, one segment each.  Returns where they lie in lits */
static uint64_t lit_put(builder *B, const uint8_t *bytes, uint64_t n, uint64_t dst)
{
	xzamd_rp_plan *p = B->p;
	if (B->oom) return 0;
	if (p->lits_len + n > B->lits_cap) {
		uint64_t cap = B->lits_cap ? 2 * B->lits_cap : 4096;
		while (cap < p->lits_len + n) cap *= 2;
		uint8_t *l = (uint8_t *)realloc(p->lits, cap);
		if (!l) { B->oom = 1; return 0; }
		p->lits = l; B->lits_cap = cap;
	}
	const uint64_t at = p->lits_len;
	memcpy(p->lits + at, bytes, n);
	p->lits_len += n;
	seg_put(B, 1, at, n, dst);
	return at;
}

void xzamd_repair_plan_free_(xzamd_rp_plan *plan)
{
	free(plan->segs); free(plan->lits);
	memset(plan, 0, sizeof(*plan));
}

int xzamd_repair_plan_(xzamd_rp_block *blocks, uint64_t nb, int check, int framed, xzamd_rp_plan *plan)
{
	const uint32_t cbytes = xzamd_check_bytes_(check);
	builder B = { plan, 0, 0, 0 };
	memset(plan, 0, sizeof(*plan));
	plan->first = nb;
	if (cbytes == 0xFFFFFFFFu) return XZAMD_PROG_ERROR;
	for (uint64_t b = 0; b < nb; ++b) {
		if (b + 1 < nb && blocks[b + 1].pos != blocks[b].pos + ((blocks[b].unpadded + 3) & ~3ull))
			return XZAMD_PROG_ERROR;
		if (blocks[b].repl != XZAMD_RP_KEEP && plan->first == nb) plan->first = b;
		if (blocks[b].repl == XZAMD_RP_KEEP) blocks[b].new_unpadded = blocks[b].unpadded;
		blocks[b].new_pos = blocks[b].pos;
	}
	if (plan->first == nb) return XZAMD_OK;
	plan->tail_pos = blocks[plan->first].pos;

	uint64_t opos = 0;              /* offset from tail_pos */
	for (uint64_t b = plan->first; b < nb; ++b) {
		xzamd_rp_block *K = &blocks[b];
		K->new_pos = plan->tail_pos + opos;
		if (K->repl == XZAMD_RP_KEEP) {
			/* a kept Block moves as it is, in pieces a workgroup copies quickly */
			const uint64_t total = (K->unpadded + 3) & ~3ull;
			for (uint64_t o = 0; o < total; o += XZAMD_RP_SEG_MAX)
				seg_put(&B, 2, K->pos + o, total - o < XZAMD_RP_SEG_MAX ? total - o : XZAMD_RP_SEG_MAX, opos + o);
			opos += total;
		} else if (K->repl == XZAMD_RP_CODED) {
			const uint64_t total = (K->new_unpadded + 3) & ~3ull;
			for (uint64_t o = 0; o < total; o += XZAMD_RP_SEG_MAX)
				seg_put(&B, 0, K->src + o, total - o < XZAMD_RP_SEG_MAX ? total - o : XZAMD_RP_SEG_MAX, opos + o);
			opos += total;
		} else if (K->repl == XZAMD_RP_STORED) {
			/* block_buffer_encoder.c:88-162 as the batch encoder lays a stored Block out: header of the chain {LZMA2}, chunks
			 * 0x01 / 0x02 of 64 KiB of the original, end marker, padding; the Check is the re-encoded Block's (the encoder
			 * computed it over the same bytes) */
			uint8_t small[64];
			const uint64_t usize = K->usize;
			const uint64_t csz = usize + ((usize + 65535) / 65536) * 3 + 1;
			const uint32_t hs = xzamd_block_header_size_(csz, usize, NULL);
			xzamd_block_header_put_(small, hs, csz, usize, 0x00, NULL);
			(void)lit_put(&B, small, hs, opos);
			opos += hs;
			uint8_t ctl = 0x01;
			for (uint64_t ip = 0; ip < usize; ip += 65536) {
				const uint64_t cs = usize - ip < 65536 ? usize - ip : 65536;
				const uint8_t ch[3] = { ctl, (uint8_t)((cs - 1) >> 8), (uint8_t)(cs - 1) };
				ctl = 0x02;
				(void)lit_put(&B, ch, 3, opos);
				seg_put(&B, 3, K->uoff + ip, cs, opos + 3);
				opos += 3 + cs;
			}
			uint32_t tl = 0;
			small[tl++] = 0x00;
			while ((csz + (tl - 1)) & 3) small[tl++] = 0;
			(void)lit_put(&B, small, tl, opos);
			opos += tl;
			seg_put(&B, 0, K->src, cbytes, opos);
			opos += cbytes;
			K->new_unpadded = hs + csz + cbytes;
		} else
			return xzamd_repair_plan_free_(plan), XZAMD_PROG_ERROR;
	}
	if (framed && !B.oom) {
		const uint64_t cap = 32 + nb * 18 + 16;
		uint64_t *rec = (uint64_t *)malloc(sizeof(uint64_t) * 2 * (nb ? nb : 1));
		uint8_t *ib = (uint8_t *)malloc(cap);
		uint64_t w = 0;
		if (rec && ib) {
			for (uint64_t b = 0; b < nb; ++b) { rec[b] = blocks[b].new_unpadded; rec[nb + b] = blocks[b].usize; }
			w = xzamd_frame_index_footer(ib, cap, check, rec, rec + nb, nb);
			if (w) {
				plan->frame_off = lit_put(&B, ib, w, opos);
				plan->frame_len = w;
				opos += w;
			}
		}
		free(rec); free(ib);
		if (!w) B.oom = 1;
	}
	if (B.oom) return xzamd_repair_plan_free_(plan), XZAMD_MEM_ERROR;
	plan->tail_len = opos;
	plan->new_size = plan->tail_pos + opos;
	return XZAMD_OK;
}

/* The splice layout of a chain repair: the segments of a single-Block Stream are bare LZMA2 chunk chains that lie back to back,
 * so a replaced chain only shifts the ones behind it.  Same plan structure, same segment kinds, destinations from tail_pos. */
int xzamd_chains_plan_(xzamd_cp_chain *chains, uint64_t n, xzamd_rp_plan *plan)
{
	builder B = { plan, 0, 0, 0 };
	memset(plan, 0, sizeof(*plan));
	plan->first = n;
	for (uint64_t i = 0; i < n; ++i) {
		if (i + 1 < n && chains[i + 1].pos != chains[i].pos + chains[i].len)
			return XZAMD_PROG_ERROR;
		if (chains[i].repl != XZAMD_RP_KEEP && plan->first == n) plan->first = i;
		if (chains[i].repl == XZAMD_RP_KEEP) chains[i].new_len = chains[i].len;
		chains[i].new_pos = chains[i].pos;
	}
	if (plan->first == n) return XZAMD_OK;
	plan->tail_pos = chains[plan->first].pos;

	uint64_t opos = 0;              /* offset from tail_pos */
	for (uint64_t i = plan->first; i < n; ++i) {
		xzamd_cp_chain *K = &chains[i];
		K->new_pos = plan->tail_pos + opos;
		if (K->repl == XZAMD_RP_KEEP || K->repl == XZAMD_RP_CODED) {
			const uint32_t kind = K->repl == XZAMD_RP_KEEP ? 2u : 0u;
			const uint64_t from = K->repl == XZAMD_RP_KEEP ? K->pos : K->src;
			for (uint64_t o = 0; o < K->new_len; o += XZAMD_RP_SEG_MAX)
				seg_put(&B, kind, from + o, K->new_len - o < XZAMD_RP_SEG_MAX ? K->new_len - o : XZAMD_RP_SEG_MAX, opos + o);
			opos += K->new_len;
		} else if (K->repl == XZAMD_RP_STORED) {
			/* the stored chain as the batch encoder writes it for a segment that does not shrink: 0x01 + 64 KiB of the original,
			 * then 0x02 chunks; no end marker (the Block's own follows the last chain) */
			const uint64_t start = opos;
			uint8_t ctl = 0x01;
			for (uint64_t ip = 0; ip < K->usize; ip += 65536) {
				const uint64_t cs = K->usize - ip < 65536 ? K->usize - ip : 65536;
				const uint8_t ch[3] = { ctl, (uint8_t)((cs - 1) >> 8), (uint8_t)(cs - 1) };
				ctl = 0x02;
				(void)lit_put(&B, ch, 3, opos);
				seg_put(&B, 3, K->uoff + ip, cs, opos + 3);
				opos += 3 + cs;
			}
			K->new_len = opos - start;
		} else
			return xzamd_repair_plan_free_(plan), XZAMD_PROG_ERROR;
	}
	if (B.oom) return xzamd_repair_plan_free_(plan), XZAMD_MEM_ERROR;
	plan->tail_len = opos;
	plan->new_size = plan->tail_pos + opos;
	return XZAMD_OK;
}
