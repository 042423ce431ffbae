/* xzamd_block_parse.h -- the per-Block framing checks of the device .xz decoder, one text for the host (xzamd_framing.c)
 * and for the device (k_dec_headers, lzma_decode.hip): Block Header, sizes against the Index, Block
 * Padding, the stored Check.  The checks and their order restate
 *   common/block_header_decoder.c:17-125    size byte, CRC32, reserved flags, the two optional VLIs, padding
 *   common/filter_flags_decoder.c:15-45,    Filter Flags: ids, sizes of properties, LZMA2 dictionary byte, delta distance,
 *   filter_common.c:250-294                 BCJ start offset (0 only); LZMA2 last and only last
 *   common/block_decoder.c:47-230           sizes against the header, Block Padding
 * so that the first defect of a Block gives the same code whoever parses it. */
#ifndef XZAMD_BLOCK_PARSE_H
#define XZAMD_BLOCK_PARSE_H

#include <stdint.h>
#include "kernels_api.h"

#ifdef __HIPCC__
#define XZB_FN __host__ __device__ static inline
#else
#define XZB_FN static inline
#endif

/* codes of include/xz_amd.h (this header is also read by the HIP units, which do not see it) */
#define XZB_OPTIONS_ERROR 8u
#define XZB_DATA_ERROR 9u

/* the check that failed (xzamd_hdr_err.step); xzb_step_msg names them */
enum {
	XZB_S_NONE = 0, XZB_S_BEYOND, XZB_S_INDICATOR, XZB_S_HEADER_SIZE, XZB_S_HEADER_CRC, XZB_S_RESERVED_FLAGS,
	XZB_S_CSIZE_VLI, XZB_S_USIZE_VLI, XZB_S_FILTER_FLAGS, XZB_S_LZMA2_PROPS, XZB_S_DELTA_PROPS, XZB_S_BCJ_PROPS,
	XZB_S_BCJ_START, XZB_S_FILTER_ID, XZB_S_HEADER_PADDING, XZB_S_CHAIN, XZB_S_UNPADDED, XZB_S_SIZES, XZB_S_BLOCK_END,
	XZB_S_BLOCK_PADDING, XZB_S_TOO_LARGE,
	XZB_S_CHUNK_CONTROL, XZB_S_CHUNK_SIZES,         /* the forward walk over a chunk chain (xzamd_walk_parse.h) */
	XZB_S_COUNT
};

XZB_FN int xzb_vli(const uint8_t *p, uint64_t n, uint64_t *pos, uint64_t *v)
{
	/* common/vli_decoder.c:16-86 (single call form) */
	uint64_t r = 0;
	for (unsigned i = 0; i < 9; ++i) {
		if (*pos >= n) return -1;
		const uint8_t b = p[(*pos)++];
		r |= (uint64_t)(b & 0x7F) << (7 * i);
		if (!(b & 0x80)) {
			if (b == 0 && i != 0) return -1;        /* non-minimal encoding */
			*v = r;
			return 0;
		}
	}
	return -1;
}

XZB_FN uint32_t xzb_rd32(const uint8_t *p)
{
	return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

/* CRC32 of a Block Header (at most 1020 bytes): bit by bit, no table to keep in two address spaces */
XZB_FN uint32_t xzb_crc32(const uint8_t *p, uint32_t n)
{
	uint32_t c = 0xFFFFFFFFu;
	for (uint32_t i = 0; i < n; ++i) {
		c ^= p[i];
		for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
	}
	return ~c;
}

/* The hs bytes of a Block Header (hs from its size byte, all readable): CRC32, flags, the optional sizes
 * (UINT64_MAX = absent), the Filter Flags one after another as the reference reads them, header padding, the
 * chain rule.  Fills *ch (zeroed by the caller) and *dict_size.  Returns 0 or the error code; *step = the check. */
XZB_FN uint32_t xzb_header(const uint8_t *bh, uint32_t hs, uint64_t *h_csize, uint64_t *h_usize, xzamd_dec_chain *ch,
		uint32_t *dict_size, uint32_t *step)
{
#define XZB_FAIL(code, s) do { *step = (s); return (code); } while (0)
	if (xzb_rd32(bh + hs - 4) != xzb_crc32(bh, hs - 4)) XZB_FAIL(XZB_DATA_ERROR, XZB_S_HEADER_CRC);
	if (bh[1] & 0x3C) XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_RESERVED_FLAGS);
	uint64_t hp = 2;
	*h_csize = UINT64_MAX;
	*h_usize = UINT64_MAX;
	if ((bh[1] & 0x40) && xzb_vli(bh, hs - 4, &hp, h_csize)) XZB_FAIL(XZB_DATA_ERROR, XZB_S_CSIZE_VLI);
	if ((bh[1] & 0x80) && xzb_vli(bh, hs - 4, &hp, h_usize)) XZB_FAIL(XZB_DATA_ERROR, XZB_S_USIZE_VLI);
	const uint32_t nfilt = (bh[1] & 3u) + 1;
	uint32_t db = 0, lzma2_at = UINT32_MAX, nlzma2 = 0;
	for (uint32_t i = 0; i < nfilt; ++i) {
		uint64_t fid = 0, fps = 0;
		if (xzb_vli(bh, hs - 4, &hp, &fid) || fid >= (1ull << 62) || xzb_vli(bh, hs - 4, &hp, &fps) || hs - 4 - hp < fps)
			XZB_FAIL(XZB_DATA_ERROR, XZB_S_FILTER_FLAGS);
		const uint8_t *props = bh + hp;
		uint32_t entry = 0;
		if (fid == 0x21) {
			if (fps != 1 || props[0] > 40) XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_LZMA2_PROPS);
			db = props[0];
			lzma2_at = i;
			++nlzma2;
		} else if (fid == 0x03) {
			if (fps != 1) XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_DELTA_PROPS);
			entry = 3u | ((uint32_t)props[0] << 8);
		} else if (fid >= 0x04 && fid <= 0x0B) {
			if (fps != 0 && fps != 4) XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_BCJ_PROPS);
			if (fps == 4 && xzb_rd32(props) != 0) XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_BCJ_START);
			entry = (uint32_t)fid;
		} else {
			XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_FILTER_ID);
		}
		if (entry && ch->n < XZAMD_DEC_FILTERS_MAX) ch->f[ch->n++] = entry;
		hp += fps;
	}
	for (uint64_t q = hp; q < hs - 4; ++q)
		if (bh[q] != 0) XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_HEADER_PADDING);
	/* filter_common.c:250-294: LZMA2 ends the chain and stands nowhere else */
	if (nlzma2 != 1 || lzma2_at != nfilt - 1) XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_CHAIN);
	*dict_size = db == 40 ? 0xFFFFFFFFu : ((2u | (db & 1u)) << (db / 2 + 11));
	*step = XZB_S_NONE;
	return 0;
}

/* One whole Block of a file at xz: everything between its first byte and its stored Check, every read inside
 * [r->hpos, r->end).  Fills *B, *ch and the Check bytes (XZAMD_HDR_CHECK_BYTES, zeros behind the Check). */
XZB_FN uint32_t xzb_block(const uint8_t *xz, const xzamd_hdr_rec *r, xzamd_dec_block *B, xzamd_dec_chain *ch, uint8_t *stored,
		uint32_t *step)
{
	B->cpos = 0; B->csize = 0; B->upos = r->upos; B->usize = r->usize; B->dict_size = 0; B->nunits = 0; B->error = 0; B->nrecs = 0;
	ch->n = 0;
	for (uint32_t i = 0; i < XZAMD_DEC_FILTERS_MAX; ++i) ch->f[i] = 0;
	for (uint32_t i = 0; i < XZAMD_HDR_CHECK_BYTES; ++i) stored[i] = 0;
	if (r->hpos > r->end || r->end - r->hpos < 8) XZB_FAIL(XZB_DATA_ERROR, XZB_S_BEYOND);
	const uint64_t avail = r->end - r->hpos;
	const uint8_t *bh = xz + r->hpos;
	if (bh[0] == 0) XZB_FAIL(XZB_DATA_ERROR, XZB_S_INDICATOR);
	const uint32_t hs = ((uint32_t)bh[0] + 1) * 4;
	if (hs > avail) XZB_FAIL(XZB_DATA_ERROR, XZB_S_HEADER_SIZE);
	uint64_t h_csize, h_usize;
	uint32_t dict = 0;
	const uint32_t hc = xzb_header(bh, hs, &h_csize, &h_usize, ch, &dict, step);
	if (hc) return hc;
	if (r->unpadded < (uint64_t)hs + r->csz || r->unpadded > (1ull << 62)) XZB_FAIL(XZB_DATA_ERROR, XZB_S_UNPADDED);
	const uint64_t csize = r->unpadded - hs - r->csz;
	if ((h_csize != UINT64_MAX && h_csize != csize) || (h_usize != UINT64_MAX && h_usize != r->usize) || csize == 0)
		XZB_FAIL(XZB_DATA_ERROR, XZB_S_SIZES);
	const uint64_t padded = (r->unpadded + 3) & ~3ull;
	if (padded > avail) XZB_FAIL(XZB_DATA_ERROR, XZB_S_BLOCK_END);
	B->cpos = r->hpos + hs;
	B->csize = csize;
	B->dict_size = dict;
	const uint8_t *tail = bh + hs + csize;
	const uint32_t padn = (uint32_t)(padded - r->unpadded);
	for (uint32_t i = 0; i < padn; ++i)
		if (tail[i] != 0) XZB_FAIL(XZB_DATA_ERROR, XZB_S_BLOCK_PADDING);
	for (uint32_t i = 0; i < r->csz && i < XZAMD_HDR_CHECK_BYTES; ++i) stored[i] = tail[padn + i];
	if (r->usize >= (1ull << 31) || csize >= (1ull << 32)) XZB_FAIL(XZB_OPTIONS_ERROR, XZB_S_TOO_LARGE);
	*step = XZB_S_NONE;
	return 0;
#undef XZB_FAIL
}

#endif
