/* xzamd_walk_parse.h -- the forward walk over the Blocks of one .xz Stream, one text for the device (k_dec_walk,
 * lzma_decode.hip) and for the CPU harness (tests/host_stub/stub_xzk_walk.c): the Block table the Index would have given,
 * found from the front.  Restated from
 *   common/stream_decoder.c:150-260         a Block Header size byte of 0x00 is the Index Indicator
 *   common/block_header_decoder.c           the header (xzb_header, xzamd_block_parse.h)
 *   common/block_decoder.c:47-230           the sizes a header carries against what the data says
 *   lzma/lzma2_decoder.c:54-127             the chunk headers: control byte, sizes
 * A Block whose header carries both sizes is hopped over; any other is measured by walking its LZMA2 chunk chain.  The
 * chunk GRAMMAR (dictionary resets, properties) is not looked at here: the unit scan of the decode reports it, Block by
 * Block, as for a table that came from an Index.
 * Every read lies inside [0, size); every iteration of either loop moves its offset forward by at least one byte. */
#ifndef XZAMD_WALK_PARSE_H
#define XZAMD_WALK_PARSE_H

#include "xzamd_block_parse.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define XZW_UNI(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))   /* a loaded byte as a wave-uniform value */
#define XZW_WRITER() (threadIdx.x == 0)                                    /* one lane stores (plain vector stores) */
#else
#define XZW_UNI(v) ((uint32_t)(v))
#define XZW_WRITER() 1
#endif

/* The chunk chain at xz + c0: *csize (the 0x00 end marker included) and *usize.  Returns 0, XZAMD_WALK_INCOMPLETE, or
 * XZAMD_WALK_DEFECT with *code / *step.  The sums stop at the limits of xzb_block (usize < 2^31, csize < 2^32), so
 * nothing here can overflow. */
XZB_FN uint32_t xzw_chain(const uint8_t *xz, uint64_t size, uint64_t c0, uint64_t *csize, uint64_t *usize, uint32_t *code,
		uint32_t *step, uint64_t *hops)
{
	uint64_t c = c0, u = 0;
	for (;;) {
		if (c >= size) return XZAMD_WALK_INCOMPLETE;
		const uint64_t left = size - c;
		/* the six bytes a chunk header can have, loaded side by side: one miss per hop, not one per byte */
		uint32_t b[6];
		for (uint32_t i = 0; i < 6; ++i) b[i] = i < left ? XZW_UNI(xz[c + i]) : 0u;
		const uint32_t ctl = b[0];
		++*hops;
		if (ctl == 0x00) { ++c; break; }
		uint64_t hs, cs, us;
		if (ctl >= 0x80) {
			hs = ctl >= 0xC0 ? 6 : 5;
			us = (((uint64_t)(ctl & 0x1F) << 16) | ((uint64_t)b[1] << 8) | b[2]) + 1;
			cs = (((uint64_t)b[3] << 8) | b[4]) + 1;
		} else if (ctl == 0x01 || ctl == 0x02) {
			hs = 3;
			us = (((uint64_t)b[1] << 8) | b[2]) + 1;
			cs = us;
		} else {
			*code = XZB_DATA_ERROR; *step = XZB_S_CHUNK_CONTROL;
			return XZAMD_WALK_DEFECT;
		}
		if (hs > left) return XZAMD_WALK_INCOMPLETE;
		c += hs + cs;
		u += us;
		if (u >= (1ull << 31) || c - c0 >= (1ull << 32)) {
			*code = XZB_OPTIONS_ERROR; *step = XZB_S_TOO_LARGE;
			return XZAMD_WALK_DEFECT;
		}
	}
	*csize = c - c0;
	*usize = u;
	return 0;
}

/* The Blocks from pos0 (a Block Header or the Index Indicator) on: one row per Block that lies whole inside [0, size) --
 * hpos, unpadded, usize, upos, csz; `end` is left 0 for the host -- until the Index Indicator, the end of the bytes, a full
 * table or a defect.  res->pos = the offset of the Block (or Index) the walk stopped at, res->upos = where its output
 * would go. */
XZB_FN void xzw_walk(const uint8_t *xz, uint64_t size, uint64_t pos0, uint32_t csz, uint64_t upos0, xzamd_hdr_rec *rows,
		uint32_t cap, xzamd_walk_result *res)
{
	uint64_t pos = pos0, upos = upos0, hops = 0;
	uint32_t nrows = 0, stop, code = 0, step = XZB_S_NONE;
	for (;;) {
		if (pos >= size) { stop = XZAMD_WALK_INCOMPLETE; break; }
		const uint64_t left = size - pos;
		const uint32_t b0 = XZW_UNI(xz[pos]);
		++hops;
		if (b0 == 0x00) { stop = XZAMD_WALK_INDEX; break; }
		if (nrows == cap) { stop = XZAMD_WALK_TABLE_FULL; break; }
		const uint32_t hs = (b0 + 1) * 4;
		if (hs > left) { stop = XZAMD_WALK_INCOMPLETE; break; }
		uint64_t h_csize, h_usize, csize, usize;
		uint32_t dict = 0;
		xzamd_dec_chain ch;
		ch.n = 0;
		for (uint32_t i = 0; i < XZAMD_DEC_FILTERS_MAX; ++i) ch.f[i] = 0;
		code = xzb_header(xz + pos, hs, &h_csize, &h_usize, &ch, &dict, &step);
		if (code) { stop = XZAMD_WALK_DEFECT; break; }
		if (h_csize != UINT64_MAX && h_usize != UINT64_MAX) {
			csize = h_csize;
			usize = h_usize;
			if (csize == 0) { code = XZB_DATA_ERROR; step = XZB_S_SIZES; stop = XZAMD_WALK_DEFECT; break; }
		} else {
			const uint32_t r = xzw_chain(xz, size, pos + hs, &csize, &usize, &code, &step, &hops);
			if (r) { stop = r; break; }
			/* block_decoder.c: the one size the header does carry must be what the data has */
			if ((h_csize != UINT64_MAX && h_csize != csize) || (h_usize != UINT64_MAX && h_usize != usize)) {
				code = XZB_DATA_ERROR; step = XZB_S_CHUNK_SIZES; stop = XZAMD_WALK_DEFECT; break;
			}
		}
		if (usize >= (1ull << 31) || csize >= (1ull << 32)) { code = XZB_OPTIONS_ERROR; step = XZB_S_TOO_LARGE; stop = XZAMD_WALK_DEFECT; break; }
		const uint64_t unpadded = (uint64_t)hs + csize + csz;
		const uint64_t padded = (unpadded + 3) & ~3ull;
		if (padded > left) { stop = XZAMD_WALK_INCOMPLETE; code = 0; step = XZB_S_NONE; break; }
		if (XZW_WRITER()) {
			xzamd_hdr_rec *r = &rows[nrows];
			r->hpos = pos; r->unpadded = unpadded; r->usize = usize; r->end = 0; r->upos = upos; r->csz = csz; r->pad_ = 0;
		}
		++nrows;
		pos += padded;
		upos += usize;
	}
	if (stop != XZAMD_WALK_DEFECT) { code = 0; step = XZB_S_NONE; }
	if (XZW_WRITER()) {
		res->stop = stop; res->code = code; res->step = step; res->nrows = nrows;
		res->pos = pos; res->upos = upos; res->hops = hops; res->pad_ = 0;
	}
}

#endif
