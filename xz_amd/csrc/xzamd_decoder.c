/*
 * xzamd_decoder.c -- liblzma's .xz Stream decoder ABI on top of the forward reader (xzamd_forward.c):
 *   lzma_stream_decoder          replaces common/stream_decoder.c:443
 *   lzma_stream_decoder_mt       replaces common/stream_decoder_mt.c:1951 (flags and memlimit_stop are used; threads and timeout
 *                                are accepted and unused: the coder is synchronous, the GPU is the parallelism)
 *   lzma_stream_buffer_decode    replaces common/stream_buffer_decoder.c:15
 *   lzma_get_check               replaces common/common.c:437
 * lzma_code / lzma_end / lzma_get_progress of xzamd_stream.c reach this coder through the function pointers at the start of its
 * internal struct (xzamd_coder_hooks), told apart from an encoder stream by `magic`.
 *
 * The coder batches.  lzma_code copies input into a pinned staging buffer; the twelve bytes of a Stream Header are looked at
 * on the host as soon as they are there (LZMA_FORMAT_ERROR, lzma_get_check, the LZMA_TELL_* codes, once per Stream); when the
 * staging holds a batch (XZAMD_DEC_BATCH_KIB, default 512 MiB) or the caller says LZMA_FINISH, the staged bytes are uploaded
 * and one forward step decodes every whole Block among them; the undecoded tail moves to the front, and the decoded bytes are
 * drained through next_out over as many calls as it takes.  A Block larger than the staging doubles it, up to memlimit
 * (LZMA_MEMLIMIT_ERROR).  Errors come behind the bytes in front of them, and latch.
 * Declined: LZMA_IGNORE_CHECK (LZMA_OPTIONS_ERROR at init); a Stream whose Check has no verifier fails where it starts.
 * Without LZMA_CONCATENATED the bytes behind the first Stream that this call handed in are given back; bytes of earlier calls
 * that the staging took cannot be (the reference, which decodes as it reads, never takes them): total_in can then exceed
 * the Stream's length (xz_amd_lzma.h says so).
 */
#include "xzamd_internal.h"
#include "kernels_api.h"
#include "../../include/xz_amd_lzma.h"

#include <stdlib.h>
#include <string.h>

#define BATCH_DEFAULT (512ull << 20)
#define OUT_MIN (1ull << 20)
#define FLAGS_SUPPORTED (LZMA_TELL_NO_CHECK | LZMA_TELL_UNSUPPORTED_CHECK | LZMA_TELL_ANY_CHECK | LZMA_CONCATENATED | LZMA_FAIL_FAST)

typedef struct {
	xzamd_coder_hooks hooks;        /* first: magic, and how lzma_code / lzma_end / lzma_get_progress get here */
	const lzma_allocator *allocator;
	xzamd_ctx *ctx;
	xzamd_forward_state fs;
	uint32_t flags;
	uint64_t memlimit;
	uint64_t batch;                 /* staged bytes that set a step off */
	uint8_t *stage; uint64_t stage_len, stage_cap;          /* pinned: input not yet dealt with */
	void *d_in; uint64_t d_in_cap;
	void *d_out; uint64_t d_out_cap;
	uint8_t *h_out; uint64_t h_out_cap, out_len, out_pos;   /* pinned: decoded bytes not yet drained */
	int grow_out;                   /* the room for the output doubles before the next step */
	int told;                       /* the Stream Header at the front of the staging has been looked at */
	int check;                      /* of the current Stream */
	int first;                      /* no Stream Header has been accepted yet */
	int ended;                      /* the forward reader is done: LZMA_STREAM_END once the output is drained */
	lzma_ret deferred;              /* ... or this code */
	lzma_ret latched;
	int allow_buf_error;
} dec;

static lzma_ret map_rc(int rc)
{
	switch (rc) {
	case XZAMD_OK: return LZMA_OK;
	case XZAMD_UNSUPPORTED_CHECK: return LZMA_UNSUPPORTED_CHECK;
	case XZAMD_MEM_ERROR: return LZMA_MEM_ERROR;
	case 7: return LZMA_FORMAT_ERROR;
	case XZAMD_OPTIONS_ERROR: return LZMA_OPTIONS_ERROR;
	case XZAMD_DATA_ERROR: return LZMA_DATA_ERROR;
	default: return LZMA_PROG_ERROR;        /* device failures */
	}
}

static void dec_free(dec *d)
{
	if (d->ctx) (void)xzk_set_device(xzamd_ctx_device(d->ctx));
	if (d->stage) xzk_host_free(d->stage);
	if (d->h_out) xzk_host_free(d->h_out);
	if (d->d_in) xzk_free(d->d_in);
	if (d->d_out) xzk_free(d->d_out);
	xzamd_forward_free_(&d->fs);
	if (d->ctx) xzamd_ctx_destroy(d->ctx);
	const lzma_allocator *a = d->allocator;
	d->hooks.magic = 0;
	if (a && a->free) a->free(a->opaque, d); else free(d);
}

/* room for `want` staged bytes */
static lzma_ret stage_reserve(dec *d, uint64_t want)
{
	if (want <= d->stage_cap) return LZMA_OK;
	uint64_t cap = d->stage_cap ? d->stage_cap : 65536;
	while (cap < want) cap *= 2;
	void *p = NULL;
	if (xzk_host_alloc(&p, cap)) return LZMA_MEM_ERROR;
	if (d->stage_len) memcpy(p, d->stage, d->stage_len);
	if (d->stage) xzk_host_free(d->stage);
	d->stage = (uint8_t *)p; d->stage_cap = cap;
	return LZMA_OK;
}

static lzma_ret out_reserve(dec *d, uint64_t want)
{
	if (want <= d->d_out_cap) return LZMA_OK;
	if (want > d->memlimit) return LZMA_MEMLIMIT_ERROR;
	void *h = NULL, *g = NULL;
	if (xzk_host_alloc(&h, want)) return LZMA_MEM_ERROR;
	if (xzk_malloc(&g, want + 16)) { xzk_host_free(h); return LZMA_MEM_ERROR; }
	if (d->h_out) xzk_host_free(d->h_out);
	if (d->d_out) xzk_free(d->d_out);
	d->h_out = (uint8_t *)h; d->h_out_cap = want;
	d->d_out = g; d->d_out_cap = want;
	return LZMA_OK;
}

/* The Stream Header at the front of the staging, once per Stream: LZMA_FORMAT_ERROR for a first Stream without the magic, the
 * Check for lzma_get_check, the LZMA_TELL_* code the flags ask for (everything else about it is the forward reader's) */
static lzma_ret header_look(dec *d)
{
	const uint8_t *h = d->stage;
	d->told = 1;
	if (xzamd_fr_header_(h) == XZAMD_FR_MAGIC) return d->first ? LZMA_FORMAT_ERROR : LZMA_OK;
	if (xzamd_fr_header_(h) != 0 || h[6] != 0 || (h[7] & 0xF0)) return LZMA_OK;
	d->first = 0;
	d->check = h[7] & 0x0F;
	const char *msg = "";
	int check = 0;
	const int unsupported = xzamd_fr_flags_(h + 6, &check, &msg) == XZAMD_UNSUPPORTED_CHECK;
	if ((d->flags & LZMA_TELL_NO_CHECK) && d->check == LZMA_CHECK_NONE) return LZMA_NO_CHECK;
	if ((d->flags & LZMA_TELL_UNSUPPORTED_CHECK) && unsupported) return LZMA_UNSUPPORTED_CHECK;
	if (d->flags & LZMA_TELL_ANY_CHECK) return LZMA_GET_CHECK;
	return LZMA_OK;
}

/* one forward step over the staged bytes */
static lzma_ret run_step(dec *d, int final, uint64_t taken_now, uint64_t *give_back)
{
	void *st = xzamd_ctx_stream_(d->ctx);
	lzma_ret r;
	for (;;) {
		if (d->stage_len > d->d_in_cap) {
			if (d->d_in) xzk_free(d->d_in);
			d->d_in = NULL; d->d_in_cap = 0;
			if (xzk_malloc(&d->d_in, d->stage_cap + 16)) return LZMA_MEM_ERROR;
			d->d_in_cap = d->stage_cap;
		}
		if (!d->d_in && xzk_malloc(&d->d_in, 16)) return LZMA_MEM_ERROR;
		/* room for the output: from what is staged (twice its size, OUT_MIN at the least); a Block that needs more says so */
		if (!d->d_out_cap || d->grow_out) {
			/* (grow_out: the step before filled the room, which has been drained since: twice as much, so that data that expands
			 * a lot does not upload its staging once per small piece of output) */
			uint64_t want = 2 * d->stage_len > OUT_MIN ? 2 * d->stage_len : OUT_MIN;
			if (d->grow_out && want < 2 * d->d_out_cap) want = 2 * d->d_out_cap;
			d->grow_out = 0;
			if ((r = out_reserve(d, want < d->memlimit ? want : d->memlimit)) != LZMA_OK) return r;
		}
		if (d->stage_len && (xzk_h2d(d->d_in, d->stage, d->stage_len, st) || xzk_sync(st))) return LZMA_PROG_ERROR;
		const int rc = xzamd_forward_step_(d->ctx, &d->fs, (const uint8_t *)d->d_in, d->stage_len, final, (uint8_t *)d->d_out,
				d->d_out_cap, st);
		if (d->fs.produced) {
			if (xzk_d2h(d->h_out, d->d_out, d->fs.produced, st) || xzk_sync(st)) return LZMA_PROG_ERROR;
			d->out_len = d->fs.produced; d->out_pos = 0;
		}
		const uint64_t left = d->stage_len - d->fs.consumed;
		if (d->fs.consumed) {
			memmove(d->stage, d->stage + d->fs.consumed, left);
			d->stage_len = left;
			d->told = 0;
		}
		if (rc != XZAMD_OK) { d->deferred = map_rc(rc); return LZMA_OK; }
		switch (d->fs.stop) {
		case XZAMD_FWD_END:
			d->ended = 1;
			/* stream_decoder.c without LZMA_CONCATENATED: what follows the Stream is not this coder's */
			*give_back = left < taken_now ? left : taken_now;
			d->stage_len -= *give_back;
			return LZMA_OK;
		case XZAMD_FWD_PAUSE:
			return LZMA_OK;                                 /* in front of a further Stream Header: the host looks at it first */
		case XZAMD_FWD_TRUNCATED:
			d->deferred = LZMA_BUF_ERROR;
			return LZMA_OK;
		case XZAMD_FWD_OUT_FULL:
			if (d->fs.produced) { d->grow_out = 1; return LZMA_OK; }    /* drain, then the rest */
			/* a Block larger than the room: at least twice the room, so that a file of such Blocks grows it a few times only */
			if ((r = out_reserve(d, d->fs.need > 2 * d->d_out_cap || 2 * d->d_out_cap > d->memlimit ? d->fs.need : 2 * d->d_out_cap))
					!= LZMA_OK)
				return r;
			continue;
		default:
			/* more input is needed.  A staging that is full and of which nothing could be used holds a piece larger than
			 * itself: twice the room */
			if (d->fs.consumed == 0 && d->stage_len >= d->batch) {
				if (2 * d->batch > d->memlimit) return LZMA_MEMLIMIT_ERROR;
				d->batch *= 2;
			}
			return LZMA_OK;
		}
	}
}

static lzma_ret dec_code(lzma_stream *strm, lzma_action action)
{
	dec *d = (dec *)strm->internal;
	if (action != LZMA_RUN && action != LZMA_FINISH) return LZMA_PROG_ERROR;
	if (d->latched != LZMA_OK) return d->latched;
	if (xzk_set_device(xzamd_ctx_device(d->ctx))) return d->latched = LZMA_PROG_ERROR;
	const size_t in0 = strm->avail_in, out0 = strm->avail_out;
	uint64_t taken_now = 0;
	lzma_ret ret = LZMA_OK;
	for (;;) {
		/* drain */
		if (d->out_pos < d->out_len) {
			const uint64_t left = d->out_len - d->out_pos;
			const size_t k = left < strm->avail_out ? (size_t)left : strm->avail_out;
			if (k) memcpy(strm->next_out, d->h_out + d->out_pos, k);
			strm->next_out += k; strm->avail_out -= k; strm->total_out += k;
			d->out_pos += k;
			if (d->out_pos < d->out_len) break;             /* no room: the caller comes back */
		}
		if (d->deferred != LZMA_OK) { ret = d->deferred; break; }
		if (d->ended) { ret = LZMA_STREAM_END; break; }
		/* stage */
		if (strm->avail_in && d->stage_len < d->batch) {
			const uint64_t room = d->batch - d->stage_len;
			const size_t k = room < strm->avail_in ? (size_t)room : strm->avail_in;
			if ((ret = stage_reserve(d, d->stage_len + k)) != LZMA_OK) break;
			memcpy(d->stage + d->stage_len, strm->next_in, k);
			d->stage_len += k; taken_now += k;
			strm->next_in += k; strm->avail_in -= k; strm->total_in += k;
		}
		if (!d->told && d->fs.phase == XZAMD_FWD_PHASE_HEADER && d->stage_len >= 12 && (ret = header_look(d)) != LZMA_OK) break;
		const int final = action == LZMA_FINISH && strm->avail_in == 0;
		if (d->stage_len < d->batch && !final) break;           /* nothing to run yet */
		uint64_t give_back = 0;
		if ((ret = run_step(d, final, taken_now, &give_back)) != LZMA_OK) break;
		if (give_back) {
			strm->next_in -= give_back; strm->avail_in += give_back; strm->total_in -= give_back;
			taken_now -= give_back;
		}
		if (!d->ended && d->deferred == LZMA_OK && d->out_len == d->out_pos && d->fs.consumed == 0 && d->fs.stop == XZAMD_FWD_MORE
				&& strm->avail_in == 0)
			break;                                              /* the step wants bytes the caller has not given */
	}
	switch (ret) {
	case LZMA_OK:
		if (strm->avail_in == in0 && strm->avail_out == out0) {
			if (d->allow_buf_error) ret = LZMA_BUF_ERROR;
			else d->allow_buf_error = 1;
		} else {
			d->allow_buf_error = 0;
		}
		break;
	case LZMA_NO_CHECK: case LZMA_UNSUPPORTED_CHECK: case LZMA_GET_CHECK:
		if (ret == d->deferred) d->latched = ret;               /* (the forward reader's verdict, not a notice) */
		d->allow_buf_error = 0;
		break;
	case LZMA_STREAM_END:
		break;
	default:
		d->latched = ret;
		break;
	}
	return ret;
}

static void dec_end(lzma_stream *strm) { dec_free((dec *)strm->internal); }

static void dec_progress(lzma_stream *strm, uint64_t *progress_in, uint64_t *progress_out)
{
	if (progress_in) *progress_in = strm->total_in;
	if (progress_out) *progress_out = strm->total_out;
}

static lzma_ret dec_init(lzma_stream *strm, uint64_t memlimit, uint32_t flags)
{
	if (strm == NULL) return LZMA_PROG_ERROR;
	/* (a coder of this library that is still in the stream ends first, as lzma_next_strm_init does) */
	if (strm->internal != NULL) lzma_end(strm);
	strm->internal = NULL;
	strm->total_in = strm->total_out = 0;
	if (memlimit == 0) return LZMA_PROG_ERROR;
	if ((flags & ~FLAGS_SUPPORTED) || (flags & LZMA_IGNORE_CHECK)) return LZMA_OPTIONS_ERROR;
	const lzma_allocator *a = strm->allocator;
	dec *d = (dec *)(a && a->alloc ? a->alloc(a->opaque, 1, sizeof(*d)) : malloc(sizeof(*d)));
	if (!d) return LZMA_MEM_ERROR;
	memset(d, 0, sizeof(*d));
	d->allocator = a;
	d->hooks.magic = XZAMD_MAGIC_DEC;
	d->hooks.code = dec_code; d->hooks.end = dec_end; d->hooks.progress = dec_progress;
	d->flags = flags; d->memlimit = memlimit;
	d->first = 1;
	d->batch = BATCH_DEFAULT;
	const char *e = getenv("XZAMD_DEC_BATCH_KIB");
	if (e && *e) {
		const unsigned long long kib = strtoull(e, NULL, 10);
		if (kib >= 1 && kib <= (1ull << 32)) d->batch = kib << 10;
	}
	if (d->batch > memlimit) d->batch = memlimit < 4096 ? 4096 : memlimit;
	xzamd_forward_init_(&d->fs, (flags & LZMA_CONCATENATED) ? XZAMD_FWD_CONCATENATED : 0);
	d->fs.pause_at_header = 1;
	/* the device the caller has made current, as the encoders do */
	int dev = 0;
	if (xzk_get_device(&dev)) dev = 0;
	if (xzamd_ctx_create(&d->ctx, dev) != XZAMD_OK) { d->ctx = NULL; dec_free(d); return LZMA_MEM_ERROR; }
	strm->internal = (lzma_internal *)d;
	return LZMA_OK;
}

lzma_ret lzma_stream_decoder(lzma_stream *strm, uint64_t memlimit, uint32_t flags) { return dec_init(strm, memlimit, flags); }

lzma_ret lzma_stream_decoder_mt(lzma_stream *strm, const lzma_mt *options)
{
	if (strm == NULL || options == NULL) return LZMA_PROG_ERROR;
	return dec_init(strm, options->memlimit_stop, options->flags);
}

lzma_check lzma_get_check(const lzma_stream *strm)
{
	if (strm == NULL || strm->internal == NULL || ((const xzamd_coder_hooks *)strm->internal)->magic != XZAMD_MAGIC_DEC)
		return LZMA_CHECK_NONE;
	return (lzma_check)((const dec *)strm->internal)->check;
}

lzma_ret lzma_stream_buffer_decode(uint64_t *memlimit, uint32_t flags, const lzma_allocator *allocator, const uint8_t *in,
		size_t *in_pos, size_t in_size, uint8_t *out, size_t *out_pos, size_t out_size)
{
	/* common/stream_buffer_decoder.c:15-91 */
	if (in_pos == NULL || (in == NULL && *in_pos != in_size) || *in_pos > in_size || out_pos == NULL
			|| (out == NULL && *out_pos != out_size) || *out_pos > out_size || memlimit == NULL)
		return LZMA_PROG_ERROR;
	if (flags & LZMA_TELL_ANY_CHECK) return LZMA_PROG_ERROR;
	lzma_stream s = LZMA_STREAM_INIT;
	s.allocator = allocator;
	lzma_ret r = dec_init(&s, *memlimit, flags);
	if (r != LZMA_OK) return r;
	static uint8_t none[1];
	s.next_in = in ? in + *in_pos : none; s.avail_in = in_size - *in_pos;
	s.next_out = out ? out + *out_pos : none; s.avail_out = out_size - *out_pos;
	do r = dec_code(&s, LZMA_FINISH); while (r == LZMA_OK && s.avail_out != 0 && !((dec *)s.internal)->allow_buf_error);
	if (r == LZMA_STREAM_END) {
		*in_pos = in_size - s.avail_in;
		*out_pos = out_size - s.avail_out;
		r = LZMA_OK;
	} else if (r == LZMA_OK || r == LZMA_BUF_ERROR) {
		/* the input ended early, or the output is too small */
		r = s.avail_out == 0 && ((dec *)s.internal)->out_pos < ((dec *)s.internal)->out_len ? LZMA_BUF_ERROR
				: s.avail_in == 0 ? LZMA_DATA_ERROR : LZMA_BUF_ERROR;
	}
	dec_end(&s);
	return r;
}
