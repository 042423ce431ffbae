/*
 * xzamd_frame.c -- the .xz container as the encoder writes it (doc/xz-file-format.txt): CRC32 / CRC64, VLI, Stream
 * Header, Index and Footer, Block Header, the size bounds, stored Blocks made on the host, and the Check of a Block
 * combined from the Checks of its segments.  Plain host code: no
 * device call and no context.
 *
 * Mirrors the container half of the reference
 *   src/liblzma/common/block_header_encoder.c, block_buffer_encoder.c,
 *   index_encoder.c, stream_flags_encoder.c, vli_encoder.c
 */
#include "xzamd_internal.h"

#include <pthread.h>
#include <string.h>

static uint32_t crc32_tab[256];
static pthread_once_t crc32_once = PTHREAD_ONCE_INIT;

static void crc32_init(void)
{
	for (uint32_t i = 0; i < 256; ++i) {
		uint32_t r = i;
		for (int k = 0; k < 8; ++k)
			r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1)));
		crc32_tab[i] = r;
	}
}

static uint32_t crc32_buf(const uint8_t *p, size_t n)
{
	pthread_once(&crc32_once, crc32_init);       /* streams may be framed from several threads */
	uint32_t c = 0xFFFFFFFFu;
	while (n--)
		c = crc32_tab[(c ^ *p++) & 0xFF] ^ (c >> 8);
	return ~c;
}

uint32_t xzamd_crc32_host_(const uint8_t *p, size_t n) { return crc32_buf(p, n); }

void xzamd_le32_(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

static uint32_t vli_len(uint64_t v)
{
	uint32_t n = 0;
	do { ++n; v >>= 7; } while (v);
	return n;
}

static uint32_t vli_put(uint8_t *out, uint64_t v)
{
	uint32_t n = 0;
	for (; v >= 0x80; v >>= 7)
		out[n++] = (uint8_t)(v | 0x80);
	out[n++] = (uint8_t)v;
	return n;
}

uint32_t xzamd_check_bytes_(int check)
{
	switch (check) {
	case XZAMD_CHECK_NONE: return 0;
	case XZAMD_CHECK_CRC32: return 4;
	case XZAMD_CHECK_CRC64: return 8;
	case XZAMD_CHECK_SHA256: return 32;
	default: return 0xFFFFFFFFu;
	}
}

uint64_t xzamd_frame_header(uint8_t *out, int check)
{
	/* stream_flags_encoder.c:29-52 */
	static const uint8_t magic[6] = { 0xFD, 0x37, 0x7A, 0x58, 0x5A, 0x00 };
	memcpy(out, magic, 6);
	out[6] = 0;
	out[7] = (uint8_t)check;
	xzamd_le32_(out + 8, crc32_buf(out + 6, 2));
	return 12;
}

uint64_t xzamd_frame_index_footer(uint8_t *out, uint64_t cap, int check,
		const uint64_t *unpadded, const uint64_t *uncompressed, uint64_t nblocks)
{
	/* index_encoder.c:43-164, stream_flags_encoder.c:56-85 */
	uint64_t need = 1 + vli_len(nblocks);
	for (uint64_t i = 0; i < nblocks; ++i)
		need += vli_len(unpadded[i]) + vli_len(uncompressed[i]);
	const uint64_t padded = (need + 3) & ~3ull;
	if (cap < padded + 4 + 12)
		return 0;
	uint64_t pos = 0;
	out[pos++] = 0x00;
	pos += vli_put(out + pos, nblocks);
	for (uint64_t i = 0; i < nblocks; ++i) {
		pos += vli_put(out + pos, unpadded[i]);
		pos += vli_put(out + pos, uncompressed[i]);
	}
	while (pos < padded)
		out[pos++] = 0;
	xzamd_le32_(out + pos, crc32_buf(out, pos));
	pos += 4;
	uint8_t *f = out + pos;
	xzamd_le32_(f + 4, (uint32_t)(pos / 4 - 1));
	f[8] = 0;
	f[9] = (uint8_t)check;
	xzamd_le32_(f, crc32_buf(f + 4, 6));
	f[10] = 0x59;
	f[11] = 0x5A;
	return pos + 12;
}

uint8_t xzamd_dict_size_byte_(uint32_t d)
{
	/* lzma2_encoder.c:376-400 */
	if (d < 4096) d = 4096;
	--d;
	d |= d >> 2; d |= d >> 3; d |= d >> 4; d |= d >> 8; d |= d >> 16;
	if (d == 0xFFFFFFFFu)
		return 40;
	++d;
	uint32_t top = 31;
	while (!(d >> top)) --top;
	return (uint8_t)(2 * top + ((d >> (top - 1)) & 1) - 24);
}

uint64_t xzamd_block_buffer_bound(uint64_t u)
{
	/* block_buffer_encoder.c:20-69 */
	const uint64_t headers = (1 + 1 + 2 * 9 + 3 + 4 + 64 + 3) & ~3ull;
	const uint64_t lz2 = u + ((u + 65535) / 65536) * 3 + 1;
	return headers + ((lz2 + 3) & ~3ull);
}

/* The filters in front of LZMA2 as xzamd_lzma_options.bcj / bcj2 / bcj3 carry them (0 none, XZAMD_BCJ_*,
 * XZAMD_FILTER_DELTA(dist)), in chain order; NULL = the chain {LZMA2}. */
uint32_t xzamd_prefilter_list_(const xzamd_lzma_options *opt, uint32_t pre[XZAMD_PREFILTERS_MAX])
{
	uint32_t n = 0;
	if (opt != NULL) {
		const uint32_t all[XZAMD_PREFILTERS_MAX] = { opt->bcj, opt->bcj2, opt->bcj3 };
		while (n < XZAMD_PREFILTERS_MAX && all[n] != 0) { pre[n] = all[n]; ++n; }
	}
	return n;
}

int xzamd_prefilter_valid_(uint32_t pre)
{
	return (pre >= XZAMD_BCJ_X86 && pre <= XZAMD_BCJ_RISCV) || ((pre & 0xFF) == 3 && (pre >> 8) <= 255);
}

static uint32_t prefilter_flags_size(const xzamd_lzma_options *opt)
{
	uint32_t pre[XZAMD_PREFILTERS_MAX], s = 0;
	const uint32_t n = xzamd_prefilter_list_(opt, pre);
	for (uint32_t i = 0; i < n; ++i)
		s += (pre[i] & 0xFF) == 3 ? 3 : 2;
	return s;
}

uint32_t xzamd_block_header_size_(uint64_t csize, uint64_t usize, const xzamd_lzma_options *opt)
{
	/* block_header_encoder.c:17-70 for the chains {LZMA2} and {up to three of BCJ | delta, LZMA2} */
	uint32_t s = 1 + 1 + 4 + vli_len(csize) + vli_len(usize) + 3 + prefilter_flags_size(opt);
	return (s + 3) & ~3u;
}

void xzamd_block_header_put_(uint8_t *out, uint32_t hs, uint64_t csize, uint64_t usize, uint8_t dict_byte,
		const xzamd_lzma_options *opt)
{
	/* block_header_encoder.c:73-131 */
	const uint32_t body = hs - 4;
	uint32_t pre[XZAMD_PREFILTERS_MAX];
	const uint32_t npre = xzamd_prefilter_list_(opt, pre);
	memset(out, 0, body);
	out[0] = (uint8_t)(body / 4);
	out[1] = (uint8_t)(0xC0 | npre);   /* both sizes present, number of filters - 1 */
	uint32_t p = 2;
	p += vli_put(out + p, csize);
	p += vli_put(out + p, usize);
	for (uint32_t i = 0; i < npre; ++i) {
		if ((pre[i] & 0xFF) == 3) {      /* delta: id 0x03, one property byte = distance - 1 (delta_encoder.c:99-111) */
			out[p++] = 0x03;
			out[p++] = 0x01;
			out[p++] = (uint8_t)(pre[i] >> 8);
		} else {                         /* filter_flags_encoder.c:30-55: BCJ id, no properties (start offset 0) */
			out[p++] = (uint8_t)(pre[i] & 0xFF);
			out[p++] = 0x00;
		}
	}
	out[p++] = 0x21;
	out[p++] = 0x01;
	out[p++] = dict_byte;
	xzamd_le32_(out + body, crc32_buf(out, body));
}

uint64_t xzamd_stream_buffer_bound(uint64_t in_size, uint64_t block_size)
{
	/* Worst case of the span-parallel layout: every span may add LZMA2 chunk headers of its
	 * own (<= 6 bytes per chunk, at least one chunk per 4 KiB span), on top of the reference's
	 * per-Block header/padding/check and the Index.  in/128 covers 6 bytes per 768 input bytes. */
	if (block_size == 0)
		return 0;
	const uint64_t nb = (in_size + block_size - 1) / block_size;
	uint64_t tot = 12 + 12 + in_size + (in_size >> 7) + nb * (128 + 18) + 4096;
	return (tot + 15) & ~15ull;
}

/* Stored Blocks made on the host (block_buffer_encoder.c:88-162 block_encode_uncompressed: uncompressed LZMA2 chunks
 * of 64 KiB, filter chain reduced to LZMA2), laid out like the device path's XZAMD_F_BLOCKS_ONLY output.  Not an
 * encoder: the error path of the lzma_* front end for a device failure in the middle of a Stream (SURVEY.md section
 * 5: "uncompressed-chunk fallback keeps output valid"), taken only when the client asked for it
 * (XZAMD_STORED_ON_DEVICE_ERROR=1; the default is LZMA_PROG_ERROR).  Checks none / CRC32 / CRC64. */
static uint64_t crc64_tab[256];
static pthread_once_t crc64_once = PTHREAD_ONCE_INIT;
static void crc64_init(void)
{
	for (uint32_t i = 0; i < 256; ++i) {
		uint64_t r = i;
		for (int k = 0; k < 8; ++k) r = (r >> 1) ^ ((r & 1) ? 0xC96C5795D7870F42ull : 0);
		crc64_tab[i] = r;
	}
}

static uint64_t crc64_buf(const uint8_t *p, uint64_t n)
{
	pthread_once(&crc64_once, crc64_init);
	uint64_t c = ~0ull;
	for (uint64_t i = 0; i < n; ++i) c = crc64_tab[(c ^ p[i]) & 0xFF] ^ (c >> 8);
	return ~c;
}

/* ---- Check of a Block from the Checks of its segments (the single-Block Stream) ----
 * crc(A || B) = crc(A) * x^(8 |B|) + crc(B) in GF(2)[x] modulo the polynomial: the registers of CRC32 and CRC64 start and
 * end inverted, and the two inversions cancel in the sum exactly as in zlib's crc32_combine.  Reflected bit order: the
 * top bit of a word is x^0.  x^(8 n) by squaring: 64 products of at most `width` shift-and-add steps, whatever n. */
static uint64_t gf2_mul(uint64_t a, uint64_t b, uint64_t poly, uint64_t top)
{
	uint64_t p = 0;
	for (uint64_t m = top; m != 0; m >>= 1) {
		if (a & m) p ^= b;
		b = (b & 1) ? (b >> 1) ^ poly : b >> 1;
	}
	return p;
}

static uint64_t crc_shift(uint64_t crc, uint64_t len, uint64_t poly, uint64_t top)
{
	uint64_t sq = top >> 1;                           /* x^1 */
	for (int i = 0; i < 3; ++i) sq = gf2_mul(sq, sq, poly, top);      /* x^8: one byte */
	uint64_t xn = top;                                /* x^0 */
	for (; len != 0; len >>= 1) {
		if (len & 1) xn = gf2_mul(sq, xn, poly, top);
		sq = gf2_mul(sq, sq, poly, top);
	}
	return gf2_mul(xn, crc, poly, top);
}

uint32_t xzamd_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
	return (uint32_t)crc_shift(crc_a, len_b, 0xEDB88320u, 1ull << 31) ^ crc_b;
}

uint64_t xzamd_crc64_combine(uint64_t crc_a, uint64_t crc_b, uint64_t len_b)
{
	return crc_shift(crc_a, len_b, 0xC96C5795D7870F42ull, 1ull << 63) ^ crc_b;
}

/* Block Header of the single-Block Stream (block_header_encoder.c:73-131 with both sizes LZMA_VLI_UNKNOWN): 12 bytes,
 * Block Flags = number of filters - 1 = 0, Filter Flags of LZMA2 */
uint32_t xzamd_block_header_nosizes_(uint8_t out[12], uint8_t dict_byte)
{
	memset(out, 0, 12);
	out[0] = 0x02;
	out[1] = 0x00;
	out[2] = 0x21;
	out[3] = 0x01;
	out[4] = dict_byte;
	xzamd_le32_(out + 8, crc32_buf(out, 8));
	return 12;
}

int xzamd_stored_blocks_host_(const uint8_t *in, uint64_t n, uint64_t block_size, int check,
		uint8_t *out, uint64_t out_cap, uint64_t *out_size, xzamd_block_info *binfo, uint64_t binfo_cap, uint64_t *nblocks)
{
	const uint32_t cbytes = xzamd_check_bytes_(check);
	if (block_size == 0 || (check != XZAMD_CHECK_NONE && check != XZAMD_CHECK_CRC32 && check != XZAMD_CHECK_CRC64))
		return XZAMD_OPTIONS_ERROR;
	uint64_t opos = 0, nb = 0;
	for (uint64_t bs = 0; bs < n; bs += block_size, ++nb) {
		const uint64_t usize = n - bs < block_size ? n - bs : block_size;
		const uint64_t csz = usize + ((usize + 65535) / 65536) * 3 + 1;
		const uint32_t hs = xzamd_block_header_size_(csz, usize, NULL);
		const uint64_t pad = (4 - (csz & 3)) & 3;
		if (opos + hs + csz + pad + cbytes > out_cap)
			return XZAMD_BUF_ERROR;
		const uint64_t bstart = opos;
		xzamd_block_header_put_(out + opos, hs, csz, usize, 0x00, NULL);
		opos += hs;
		uint8_t ctl = 0x01;
		for (uint64_t ip = 0; ip < usize; ip += 65536) {
			const uint64_t cs = usize - ip < 65536 ? usize - ip : 65536;
			out[opos++] = ctl;
			out[opos++] = (uint8_t)((cs - 1) >> 8);
			out[opos++] = (uint8_t)(cs - 1);
			memcpy(out + opos, in + bs + ip, cs);
			opos += cs;
			ctl = 0x02;
		}
		out[opos++] = 0x00;
		for (uint64_t i = 0; i < pad; ++i) out[opos++] = 0;
		if (check == XZAMD_CHECK_CRC64) {
			const uint64_t v = crc64_buf(in + bs, usize);
			xzamd_le32_(out + opos, (uint32_t)v);
			xzamd_le32_(out + opos + 4, (uint32_t)(v >> 32));
		} else if (check == XZAMD_CHECK_CRC32) {
			xzamd_le32_(out + opos, crc32_buf(in + bs, usize));
		}
		opos += cbytes;
		if (binfo && nb < binfo_cap) {
			binfo[nb].unpadded_size = hs + csz + cbytes;
			binfo[nb].uncompressed_size = usize;
			binfo[nb].out_offset = bstart;
			binfo[nb].total_size = opos - bstart;
		}
	}
	*out_size = opos;
	if (nblocks) *nblocks = nb;
	return XZAMD_OK;
}
