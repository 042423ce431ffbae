/*
 * xzamd_host.c -- the device context and the batch encode of libxz_amd: splits the input into independent .xz Blocks,
 * drives the HIP kernels over device-resident batches of Blocks and reassembles a standards-conformant .xz Stream.
 * The container itself is written by xzamd_frame.c, presets / option checks / encode mode live in xzamd_options.c.
 *
 * Mirrors the scheduler half of the reference MT encoder
 *   src/liblzma/common/stream_encoder_mt.c   (stream_encode_mt :717, worker_encode :219)
 * with threads replaced by one device batch: all Blocks of a batch are
 * encoded by one grid, the ordered output queue (outqueue.c) becomes a prefix
 * sum over span sizes, and the copy-out becomes one gather kernel.
 */
#include "../../include/xz_amd.h"
#include "kernels_api.h"
#include "xzamd_internal.h"
#include "delta_rule.h"
#include "auto_bcj_rule.h"
#include "lclp_rule.h"

#include <stdio.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#define DEFAULT_BATCH ((1ull << 31) - (1ull << 20))   /* positions are 31-bit; more spans per launch = shorter tails */
#define CRC_STRIP 4096u

/* ------------------------------------------------------------------ */
/* context                                                              */
/* ------------------------------------------------------------------ */
typedef struct {
	void *p;
	uint64_t cap;
} dbuf;

/* stage events of one batch (one set per parity of the two-stream pipeline) */
enum { EV_START, EV_CHAINS, EV_FIND, EV_PLAN0, EV_PLAN1, EV_SEED, EV_PART, EV_ITER1, EV_PARSE, EV_FRONT, EV_BACK0, EV_CODE, EV_CRC, EV_ASM, EV_COUNT };
/* (EV_PART: behind the last partial-iteration parse launch, in front of its snapshot walks; recorded only as a start point
 * of the build ahead, no stage of the stats or of the progress) */

/* One batch of Blocks: its geometry, and what its front end (match structures, plan, parse -- the caller's stream) hands
 * to its back end (range coder of the two-phase mode, Block checks, sizes, layout, gather -- the second stream when the
 * two are pipelined). */
typedef struct {
	int active;
	uint64_t b0, nb, in_off, n64;
	uint32_t n;
	uint32_t nspans, nenc;       /* slots of the span plan, encode-span slots (two-phase) */
	uint32_t nout, opb;          /* slots that write coded bytes: in the batch, per Block */
	uint32_t nch;                /* chunk slots of the two-phase coder */
	uint64_t sort_bytes;         /* scratch of the sorts of the structure build */
	int par;                     /* which set of the double-buffered tables / events this batch uses */
	int sha_early;               /* its SHA-256 runs on the second stream from the batch's start */
	int ahead;                   /* its filters and structure build were issued ahead, on the side stream, under the batch before */
	const uint8_t *enc_in;       /* what LZMA2 reads (the filtered copy when a filter runs in front of it) */
	uint64_t max_segs, max_lits;
} batch_run;

/* start points of the build ahead: behind the plan, the last partial parse launch, the partial iterations of the batch before */
enum { AHEAD_PLAN = 1, AHEAD_PART, AHEAD_ITER1 };
#define AHEAD_DEFAULT AHEAD_PLAN      /* measured best: profiles/build_ahead_ab.txt */

/* knobs of the batch encode, read from the environment once per call */
typedef struct {
	int no_overlap;              /* XZAMD_NO_OVERLAP: one stream, no pipelining, no early seeds */
	int back_beside_build;       /* XZAMD_BACK_BESIDE_BUILD: every back end right behind its own front end */
	int build_ahead;             /* XZAMD_BUILD_AHEAD: where the next batch's structure build starts (AHEAD_*; 0: serial) */
	int timing;                  /* XZAMD_TIMING: print what the kernels timed */
	uint32_t tok_limit, log_cap; /* XZAMD_TEST_TOK_PER_BYTE, XZAMD_TEST_LOG_CAP (0: the built-in figures) */
} call_knobs;

/* constants of one xzamd_stream_encode_device call (opos and max_blocks move with its batches) */
typedef struct {
	const xzamd_lzma_options *opt;
	const uint8_t *d_in;
	uint8_t *d_out;
	uint64_t in_size, block_size, out_cap, bound, binfo_cap, total_blocks;
	uint64_t max_blocks;         /* Blocks per batch: key width, 2 GiB, memory budget, even batches; halved when out of memory */
	uint32_t hb, hmask, hbits;   /* hash geometry of the match finder */
	uint32_t span;               /* span size of the fixed plan */
	uint32_t spb, esb, cpb;      /* per Block: span slots, encode-span slots, estimate chunks */
	uint32_t cbytes, hs_fixed;
	uint32_t hs_delta;           /* XZAMD_F_AUTO_DELTA: header size of a Block that got a delta filter (hs_fixed: of one that got none) */
	int auto_delta;
	uint32_t hs_bcj;             /* XZAMD_F_AUTO_BCJ: header size of a Block that got a BCJ filter (x86 and ARM64 take the same two bytes of Filter Flags) */
	int auto_bcj;
	int auto_lclp;               /* XZAMD_F_AUTO_LCLP: every Block is parsed and coded with the lc / lp chosen for it (span args: props_tab) */
	int segments;                  /* XZAMD_F_SEGMENTS: per Block only its chunk chain */
	xzamd_mode m;
	call_knobs k;
	int check, whole, filtered, pipelined, defer, seeds_early;
	int ahead;                   /* != 0 (AHEAD_*): the filters and the structure build of batch i + 1 are issued on the side stream
	                                behind that event of batch i (pipelined two-phase calls on the list-finder path) */
	int resume, verify;          /* XZAMD_F_KEEP_RESUME / _VERIFY on a two-phase encode: resume records are exported; verify the Stream */
	int repair;                  /* XZAMD_F_REPAIR: the verification is the per-Block one, rejected Blocks are replaced */
	uint32_t rec_done;           /* resume records of the batches that are through their back end */
	uint8_t dbyte;
	void *st, *stb;              /* front-end stream (the caller's), back-end stream (the second one when pipelined) */
	void *sta;                   /* side stream of the build ahead */
	uint64_t *rec_unp, *rec_unc;
	xzamd_block_info *binfo;
	uint64_t opos;
} job_env;

struct xzamd_ctx {
	int device;
	void *own_stream;
	void *st2;                   /* back-end stream: range coder, checks and gather of batch i run here while the front end
	                                (match structures, plan, parse) of batch i + 1 runs on the caller's stream */
	void *st3;                   /* the seed pieces of a batch run here, underneath the rest of its match finder; and, in front of them,
	                                the filters and the structure build that are issued ahead of their batch */
	void *st4;                   /* measurement variants (XZAMD_BUILD_AHEAD_STREAM=own|low): a stream of its own for the build ahead */
	void *ev_seed[2][3];            /* seed lists ready (caller's stream), seeds begin / done (st3) */
	void *ev_sha;                /* SHA-256 of the batch (second stream) done */
	uint64_t batch_bytes;
	uint32_t wave_slots;         /* span wavefronts resident at once (CUs x occupancy of the standard span kernel) */
	uint32_t cus;
	uint32_t span_waves;         /* != 0: persistent span kernel with this many wavefronts */
	uint64_t alloc_limit;        /* test hook (XZAMD_TEST_ALLOC_LIMIT_MIB, read once at creation): larger allocations fail; 0 = none */
	char err[256];
	char err_msg_buf[200];
	/* device buffers */
	dbuf keys_a, keys_b, vals_a, vals_b, rank, sorted_pos, prev2, prev3, prev4, prev8, prev16, prev24, prev32, key64_a, key64_b, sa, sa_rank, sort_tmp;
	dbuf scratch, span_bytes, strip_crc, block_crc, segs, lits, trace, errw, errw2, litp, mlen, mdist, bcj[2], bcjt;
	dbuf est, totals, span_tab[2], span_cnt[2], mtop, order;       /* span plan (kernels_api.h); the piece table per pipeline parity: the coder's walk reads it */
	dbuf pinfo[2], snap_sr, part_tab;                                        /* per piece: what its parser leaves for the coder's walk; what a piece of iteration 2 starts with */
	dbuf cb_bnd[2], cb_log[2], cb_hdr[2], cb_start[2], cb_carry[2]; /* carried model walk: [0] over iteration 1's records (front end), [1] the coder's (back end) */
	dbuf sym_len[2], sym_dist[2], prior, enc_tab[2], enc_cnt[2];   /* two-phase mode ([2]: one set per pipeline parity) */
	dbuf tok, chunks, h_chunks;                                    /* coder of the two-phase mode: tokens, chunk table */
	dbuf dhist, ddist[2];                                          /* XZAMD_F_AUTO_DELTA: histograms of the batch, chosen distance per Block (per pipeline parity) */
	dbuf lhist, dprops[2];                                         /* XZAMD_F_AUTO_LCLP: joint histograms of the batch, chosen lc | lp << 8 per Block (per pipeline parity) */
	dbuf bhist, bkind[2];                                          /* XZAMD_F_AUTO_BCJ: histograms of the batch with the site counts behind them, chosen filter id per Block (per pipeline parity) */
	dbuf resume_sr;                                                /* what the token walk of every encode span started from (resume table asked for) */
	/* The resume table of the last encode with XZAMD_F_KEEP_RESUME / _VERIFY (kernels_api.h), kept until the next encode;
	 * not a per-batch buffer: it lives for the call and beyond */
	dbuf resume_tab;
	struct { int valid; uint32_t stride, nrec; uint64_t nblocks, block_size, in_size; } resume;
	xzamd_verify_report report;                                    /* of the last verification */
	xzamd_repair_report repair;                                    /* of the last repair */
	/* pinned host buffers */
	dbuf h_span_bytes, h_block_crc, h_segs, h_lits, h_span_tab, h_span_cnt[2], h_enc_tab[2], h_enc_cnt[2], h_err[2], h_ddist[2], h_bkind[2];
	void *evp[2][EV_COUNT];
	void *ev_total[2];
	uint32_t trace_cap;
	int trace_on;
	int last_par;                /* pipeline parity of the last batch (debug fetches) */
	/* A call made with `defer` returns once the back end of its last batch has been LAUNCHED (second stream); the batch is
	 * carried into the next call, which finishes it underneath the front end of its own first batch, or into
	 * xzamd_encode_finish_.  pend = that batch and the constants of its call. */
	struct { int active; job_env J; batch_run B; } pend;
	int pend_has_result, pend_rc;
	uint64_t pend_out_size;
	uint64_t par_seq;            /* parity of the double-buffered tables: continues across calls while a batch is carried */
	/* progress of the running xzamd_stream_encode_device call, read by other threads (xzamd_ctx_progress_in_) */
	pthread_mutex_t prog_mu;
	int prog_mu_ok;
	uint64_t prog_done;          /* input bytes of the batches that are through their back end */
	uint64_t prog_cur;           /* input bytes of the batch whose launches are all in flight (0: none) */
	int prog_par;                /* its event set */
	xzamd_stats stats;
};

static int fail(xzamd_ctx *c, int code, const char *what, int hip_err)
{
	if (hip_err)
		snprintf(c->err, sizeof(c->err), "%s: %s (%d)", what, xzk_error_string(hip_err), hip_err);
	else
		snprintf(c->err, sizeof(c->err), "%s", what);
	return code;
}

static int pend_complete(xzamd_ctx *c);

static int dgrow(xzamd_ctx *c, dbuf *b, uint64_t bytes, int host)
{
	if (b->cap >= bytes)
		return 0;
	if (c->pend.active) {
		/* a buffer is about to be replaced while the carried batch of the previous call may still be using it */
		int r = pend_complete(c);
		if (r) return r;
	}
	if (b->p) {
		if (host) xzk_host_free(b->p); else xzk_free(b->p);
		b->p = NULL;
		b->cap = 0;
	}
	bytes = (bytes + 255) & ~255ull;
	if (c->alloc_limit && bytes > c->alloc_limit)   /* test hook: exercises the smaller-batch retry */
		return fail(c, XZAMD_MEM_ERROR, "allocation above XZAMD_TEST_ALLOC_LIMIT_MIB", 0);
	int e = host ? xzk_host_alloc(&b->p, bytes) : xzk_malloc(&b->p, bytes);
	if (e)
		return fail(c, XZAMD_MEM_ERROR, host ? "hipHostMalloc" : "hipMalloc", e);
	b->cap = bytes;
	return 0;
}

int xzamd_ctx_create(xzamd_ctx **out, int device)
{
	*out = NULL;
	int ndev = 0;
	if (xzk_device_count(&ndev) || ndev <= 0)
		return XZAMD_DEVICE_ERROR;    /* no GPU: the product path never falls back to the CPU */
	xzamd_ctx *c = (xzamd_ctx *)calloc(1, sizeof(*c));
	if (!c)
		return XZAMD_MEM_ERROR;
	if (device < 0) {
		if (xzk_get_device(&device)) { free(c); return XZAMD_DEVICE_ERROR; }
	}
	if (device >= ndev || xzk_set_device(device)) { free(c); return XZAMD_DEVICE_ERROR; }
	c->device = device;
	if (pthread_mutex_init(&c->prog_mu, NULL)) { free(c); return XZAMD_MEM_ERROR; }
	c->prog_mu_ok = 1;
	/* from here on every failure goes through xzamd_ctx_destroy (streams and events already made are released) */
	if (xzk_stream_create(&c->own_stream)) { c->own_stream = NULL; xzamd_ctx_destroy(c); return XZAMD_DEVICE_ERROR; }
	/* (XZAMD_ST2_LOW=1, measurement knob: the back end's stream at the device's lowest priority) */
	if ((getenv("XZAMD_ST2_LOW") ? xzk_stream_create_low(&c->st2) : xzk_stream_create(&c->st2))) { c->st2 = NULL; xzamd_ctx_destroy(c); return XZAMD_DEVICE_ERROR; }
	if (xzk_event_create(&c->ev_sha)) { c->ev_sha = NULL; xzamd_ctx_destroy(c); return XZAMD_DEVICE_ERROR; }
	if (xzk_stream_create(&c->st3)) { c->st3 = NULL; xzamd_ctx_destroy(c); return XZAMD_DEVICE_ERROR; }
	{
		/* (measurement knob: the build ahead on a fourth stream, at normal or at the device's lowest priority) */
		const char *sv = getenv("XZAMD_BUILD_AHEAD_STREAM");
		const int low = sv && !strcmp(sv, "low");
		if ((low || (sv && !strcmp(sv, "own"))) && (low ? xzk_stream_create_low(&c->st4) : xzk_stream_create(&c->st4))) {
			c->st4 = NULL; xzamd_ctx_destroy(c); return XZAMD_DEVICE_ERROR;
		}
	}
	for (int i = 0; i < 6; ++i)
		if (xzk_event_create(&c->ev_seed[i / 3][i % 3])) { c->ev_seed[i / 3][i % 3] = NULL; xzamd_ctx_destroy(c); return XZAMD_DEVICE_ERROR; }
	for (int i = 0; i < 2 * EV_COUNT; ++i)
		if (xzk_event_create(&c->evp[i / EV_COUNT][i % EV_COUNT])) { c->evp[i / EV_COUNT][i % EV_COUNT] = NULL; xzamd_ctx_destroy(c); return XZAMD_DEVICE_ERROR; }
	for (int i = 0; i < 2; ++i)
		if (xzk_event_create(&c->ev_total[i])) { c->ev_total[i] = NULL; xzamd_ctx_destroy(c); return XZAMD_DEVICE_ERROR; }
	{
		const char *lim = getenv("XZAMD_TEST_ALLOC_LIMIT_MIB");
		c->alloc_limit = (lim && *lim && atoll(lim) > 0) ? (uint64_t)atoll(lim) << 20 : 0;
	}
	c->batch_bytes = DEFAULT_BATCH;
	{
		int cus = 0;
		if (xzk_cu_count(device, &cus) || cus <= 0) cus = 256;
		int occ = 0;
		if (xzk_span_occupancy(1, 64, &occ) || occ <= 0 || occ > 32) occ = 16;     /* the span kernels are built for 4 waves per SIMD */
		c->cus = (uint32_t)cus;
		c->wave_slots = (uint32_t)cus * (uint32_t)occ;
		/* XZAMD_SPAN_WAVES_PER_CU = k: persistent span kernel with k wavefronts per CU (k < 16 leaves
		 * register space for the low-priority stream's kernels); 0 / unset: one wavefront per span */
		const char *pw = getenv("XZAMD_SPAN_WAVES_PER_CU");
		c->span_waves = (pw && atoi(pw) > 0) ? (uint32_t)cus * (uint32_t)atoi(pw) : 0;
	}
	const char *env = getenv("XZAMD_BATCH_MIB");
	if (env && atoll(env) > 0)
		xzamd_ctx_set_batch_bytes(c, (uint64_t)atoll(env) << 20);
	*out = c;
	return XZAMD_OK;
}

#define CTX_NBUF_MAX 96   /* callers' array size for ctx_device_bufs */
static void ctx_device_bufs(xzamd_ctx *c, dbuf **d, size_t *nd)
{
	dbuf *all[] = { &c->keys_a, &c->keys_b, &c->vals_a, &c->vals_b, &c->rank, &c->sorted_pos,
		&c->prev2, &c->prev3, &c->prev4, &c->prev8, &c->prev16, &c->prev24, &c->prev32, &c->key64_a, &c->key64_b, &c->sa, &c->sa_rank, &c->sort_tmp,
		&c->scratch, &c->litp, &c->mlen, &c->mdist, &c->bcj[0], &c->bcj[1], &c->bcjt, &c->est, &c->mtop, &c->order, &c->dhist, &c->bhist, &c->lhist,
		&c->sym_len[0], &c->sym_len[1], &c->sym_dist[0], &c->sym_dist[1], &c->tok, &c->cb_log[0], &c->cb_log[1],
		/* small ones */
		&c->chunks,
		&c->span_bytes, &c->strip_crc, &c->block_crc, &c->segs, &c->lits, &c->trace, &c->errw, &c->errw2,
		&c->totals, &c->span_tab[0], &c->span_tab[1], &c->span_cnt[0], &c->span_cnt[1], &c->prior, &c->enc_tab[0], &c->enc_tab[1], &c->enc_cnt[0], &c->enc_cnt[1],
		&c->pinfo[0], &c->pinfo[1], &c->snap_sr, &c->part_tab, &c->cb_bnd[0], &c->cb_bnd[1], &c->cb_hdr[0], &c->cb_hdr[1], &c->cb_start[0], &c->cb_start[1],
		&c->cb_carry[0], &c->cb_carry[1], &c->resume_sr, &c->ddist[0], &c->ddist[1], &c->bkind[0], &c->bkind[1], &c->dprops[0], &c->dprops[1] };
	_Static_assert(sizeof(all) / sizeof(all[0]) <= CTX_NBUF_MAX, "ctx_device_bufs: raise CTX_NBUF_MAX");
	*nd = sizeof(all) / sizeof(all[0]);
	memcpy(d, all, sizeof(all));
}
#define CTX_NBIG 38      /* the first CTX_NBIG entries of ctx_device_bufs scale with the batch */

void xzamd_ctx_destroy(xzamd_ctx *c)
{
	if (!c)
		return;
	xzk_set_device(c->device);
	if (c->pend.active) {
		/* a deferred call nobody finished (its owner is tearing down): let the kernels end before their buffers go */
		if (c->st2) xzk_sync(c->st2);
		c->pend.active = 0;
	}
	dbuf *d[CTX_NBUF_MAX];
	size_t nd = 0;
	ctx_device_bufs(c, d, &nd);
	for (size_t i = 0; i < nd; ++i)
		if (d[i]->p) xzk_free(d[i]->p);
	if (c->resume_tab.p) xzk_free(c->resume_tab.p);
	dbuf *h[] = { &c->h_span_bytes, &c->h_block_crc, &c->h_segs, &c->h_lits, &c->h_span_tab, &c->h_span_cnt[0], &c->h_span_cnt[1],
		&c->h_enc_tab[0], &c->h_enc_tab[1], &c->h_enc_cnt[0], &c->h_enc_cnt[1], &c->h_err[0], &c->h_err[1], &c->h_chunks, &c->h_ddist[0], &c->h_ddist[1], &c->h_bkind[0], &c->h_bkind[1] };
	for (size_t i = 0; i < sizeof(h) / sizeof(h[0]); ++i)
		if (h[i]->p) xzk_host_free(h[i]->p);
	for (int i = 0; i < 2 * EV_COUNT; ++i)
		if (c->evp[i / EV_COUNT][i % EV_COUNT]) xzk_event_destroy(c->evp[i / EV_COUNT][i % EV_COUNT]);
	for (int i = 0; i < 2; ++i)
		if (c->ev_total[i]) xzk_event_destroy(c->ev_total[i]);
	if (c->ev_sha) xzk_event_destroy(c->ev_sha);
	for (int i = 0; i < 6; ++i)
		if (c->ev_seed[i / 3][i % 3]) xzk_event_destroy(c->ev_seed[i / 3][i % 3]);
	if (c->st4) xzk_stream_destroy(c->st4);
	if (c->st3) xzk_stream_destroy(c->st3);
	if (c->st2) xzk_stream_destroy(c->st2);
	if (c->own_stream) xzk_stream_destroy(c->own_stream);
	if (c->prog_mu_ok) pthread_mutex_destroy(&c->prog_mu);
	free(c);
}

/* lzma_get_progress inside a job (stream_encoder_mt.c:261-267, 1004-1024: the reference's workers publish how far they
 * are inside their Block).  A device batch has no byte position; what it has is stages whose ends are events on the
 * batch's streams.  Input bytes this context has "consumed" of the call it is running = the batches that are complete +
 * the share of the batch in flight that its finished stages stand for (structure build 25 %, finder 15 %, parse 50 %,
 * model pass + range coder 10 %: their shares of a preset-6 job).  Monotonic within a call, 0
 * outside of one; callable from any thread (the events are only queried). */
uint64_t xzamd_ctx_progress_in_(xzamd_ctx *c)
{
	if (!c || !c->prog_mu_ok)
		return 0;
	pthread_mutex_lock(&c->prog_mu);
	uint64_t v = c->prog_done;
	if (c->prog_cur) {
		void **ev = c->evp[c->prog_par];
		uint32_t pct = 0;
		if (xzk_event_query(ev[EV_CHAINS]) == 0) {
			pct = 25;
			if (xzk_event_query(ev[EV_FIND]) == 0) {
				pct = 40;
				if (xzk_event_query(ev[EV_PARSE]) == 0)
					pct = xzk_event_query(ev[EV_CODE]) == 0 ? 100 : 90;
			}
		}
		v += c->prog_cur / 100 * pct;
	}
	pthread_mutex_unlock(&c->prog_mu);
	return v;
}

/* The call's figure stays up until the next call starts or the owner resets it (the lzma_* front end does so in the same
 * critical section in which it books the finished job as a whole). */
void xzamd_ctx_progress_reset_(xzamd_ctx *c)
{
	if (!c || !c->prog_mu_ok)
		return;
	pthread_mutex_lock(&c->prog_mu);
	c->prog_done = c->prog_cur = 0;
	pthread_mutex_unlock(&c->prog_mu);
}

static void progress_set(xzamd_ctx *c, uint64_t done, uint64_t cur, int par)
{
	pthread_mutex_lock(&c->prog_mu);
	c->prog_done = done; c->prog_cur = cur; c->prog_par = par;
	pthread_mutex_unlock(&c->prog_mu);
}

int xzamd_ctx_set_batch_bytes(xzamd_ctx *c, uint64_t bytes)
{
	if (bytes < (1u << 16) || bytes >= (1ull << 31))
		return XZAMD_OPTIONS_ERROR;
	c->batch_bytes = bytes;
	return XZAMD_OK;
}

const char *xzamd_last_error(const xzamd_ctx *c) { return c ? c->err : "no context"; }
/* internal accessors for the other host translation units (xzamd_internal.h) */
void *xzamd_ctx_stream_(xzamd_ctx *c) { return c->own_stream; }
uint32_t xzamd_ctx_wave_slots_(const xzamd_ctx *c) { return c->wave_slots; }
int xzamd_ctx_fail_(xzamd_ctx *c, int code, const char *what) { return fail(c, code, what, 0); }
int xzamd_ctx_device(const xzamd_ctx *c) { return c ? c->device : -1; }
xzamd_verify_report *xzamd_ctx_report_(xzamd_ctx *c) { return &c->report; }
void xzamd_ctx_resume_(xzamd_ctx *c, xzamd_resume_view *v)
{
	memset(v, 0, sizeof(*v));
	if (!c->resume.valid || !c->resume_tab.p) return;
	v->d_rec = (uint8_t *)c->resume_tab.p;
	v->stride = c->resume.stride; v->nrec = c->resume.nrec;
	v->nblocks = c->resume.nblocks; v->block_size = c->resume.block_size; v->in_size = c->resume.in_size;
}
/* The resume export (lzma_kernels.hip) and the verification (xzamd_decode.c) are referred to weakly: a build of this unit
 * on top of a kernel layer without them, or without the decoder, answers the two flags with XZAMD_OPTIONS_ERROR. */
extern int xzk_resume_export(const xzamd_span_args *a, uint32_t nblocks, uint32_t block0, uint8_t *table, uint32_t rec_base,
		uint32_t rec_cap, void *stream) __attribute__((weak));
extern int xzamd_verify_kept_(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size,
		void *stream) __attribute__((weak));
/* ... and the repair (xzamd_repair.c): without it XZAMD_F_REPAIR is XZAMD_OPTIONS_ERROR */
extern int xzamd_repair_encoded_(xzamd_ctx *c, void *d_out, uint64_t size, uint64_t cap, const void *d_in, uint64_t in_size,
		uint64_t block_size, const xzamd_lzma_options *opt, int check, int framed, xzamd_block_info *binfo, uint64_t binfo_cap,
		uint64_t nblocks, uint64_t *new_size, void *stream) __attribute__((weak));
/* ... and the unit of the bare chunk chains (xzamd_chains.c): without it there is no XZAMD_F_SINGLE, and XZAMD_F_SEGMENTS takes
 * none of the three flags */
extern int xzamd_chains_encoded_(xzamd_ctx *c, void *d_out, uint64_t size, uint64_t cap, const void *d_in, uint64_t in_size,
		const xzamd_lzma_options *opt, int check, int repair, xzamd_block_info *binfo, uint64_t nseg, uint64_t *new_size,
		void *stream) __attribute__((weak));
extern int xzamd_single_encode_(xzamd_ctx *c, const void *d_in, uint64_t in_size, uint64_t block_size, const xzamd_lzma_options *opt,
		int check, uint32_t flags, void *d_out, uint64_t out_cap, uint64_t *out_size, xzamd_block_info *binfo, uint64_t binfo_cap,
		uint64_t *nsegments, void *stream) __attribute__((weak));
/* ... and the kernels of the automatic delta filter (lzma_filters.hip): without them XZAMD_F_AUTO_DELTA is XZAMD_OPTIONS_ERROR */
extern int xzk_delta_stats(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t *d_hist, void *stream)
		__attribute__((weak));
extern int xzk_delta_choose(const uint32_t *d_hist, uint32_t nblocks, uint32_t *d_dist, void *stream) __attribute__((weak));
extern int xzk_delta_blocks(const uint8_t *d_in, uint8_t *d_out, uint32_t n, uint32_t block_size, uint32_t nblocks,
		const uint32_t *d_dist, void *stream) __attribute__((weak));
/* ... and of the automatic BCJ filter: without them XZAMD_F_AUTO_BCJ is XZAMD_OPTIONS_ERROR */
extern int xzk_bcj_stats(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t *d_hist, uint32_t *d_nsites,
		void *stream) __attribute__((weak));
extern int xzk_bcj_choose(const uint32_t *d_hist, const uint32_t *d_nsites, uint32_t n, uint32_t block_size, uint32_t nblocks,
		uint32_t *d_kind, uint32_t *d_dist, void *stream) __attribute__((weak));
extern int xzk_bcj_blocks(const uint8_t *d_in, uint8_t *d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, const uint32_t *d_kind,
		int copy, void *stream) __attribute__((weak));
/* ... and of the automatic literal context: without them XZAMD_F_AUTO_LCLP is XZAMD_OPTIONS_ERROR */
extern int xzk_lclp_stats(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t *d_hist, void *stream)
		__attribute__((weak));
extern int xzk_lclp_choose(const uint32_t *d_hist, uint32_t nblocks, uint32_t lc, uint32_t lp, uint32_t *d_props, void *stream)
		__attribute__((weak));
extern int xzk_lclp_read(const uint32_t *d_hist, const uint32_t *d_props, uint32_t nblocks, uint32_t *h_hist, uint32_t *h_props,
		void *stream) __attribute__((weak));
xzamd_repair_report *xzamd_ctx_repair_report_(xzamd_ctx *c) { return &c->repair; }
/* A repair re-encodes Blocks on the context of the call it repairs: the kept table leaves the context meanwhile (the
 * re-encode would free it), the stats of the repaired call come back afterwards */
void xzamd_ctx_save_(xzamd_ctx *c, xzamd_ctx_saved *s)
{
	s->tab = c->resume_tab.p; s->tab_cap = c->resume_tab.cap;
	s->valid = c->resume.valid; s->stride = c->resume.stride; s->nrec = c->resume.nrec;
	s->nblocks = c->resume.nblocks; s->block_size = c->resume.block_size; s->in_size = c->resume.in_size;
	s->stats = c->stats;
	c->resume_tab.p = NULL; c->resume_tab.cap = 0;
	c->resume.valid = 0;
}
void xzamd_ctx_restore_(xzamd_ctx *c, const xzamd_ctx_saved *s)
{
	if (c->resume_tab.p) xzk_free(c->resume_tab.p);
	c->resume_tab.p = s->tab; c->resume_tab.cap = s->tab_cap;
	c->resume.valid = s->valid; c->resume.stride = s->stride; c->resume.nrec = s->nrec;
	c->resume.nblocks = s->nblocks; c->resume.block_size = s->block_size; c->resume.in_size = s->in_size;
	c->stats = s->stats;
}
void xzamd_get_stats(const xzamd_ctx *c, xzamd_stats *out) { *out = c->stats; }
const char *xzamd_version(void) { return "xz_amd 0.1 (gfx950)"; }


int xzamd_trace_enable(xzamd_ctx *c, uint32_t cap)
{
	xzk_set_device(c->device);
	int r = dgrow(c, &c->trace, 16ull * cap + 16, 0);
	if (r) return r;
	c->trace_cap = cap;
	c->trace_on = 1;
	if (xzk_memset(c->trace.p, 0, 16, c->own_stream) || xzk_sync(c->own_stream))
		return XZAMD_DEVICE_ERROR;
	return XZAMD_OK;
}

int xzamd_debug_fetch(xzamd_ctx *c, int what, void *out, uint64_t bytes)
{
	if (!c || !out)
		return XZAMD_PROG_ERROR;
	const dbuf *b = what == XZAMD_DEBUG_SA ? &c->sa : what == XZAMD_DEBUG_SA_RANK ? &c->sa_rank
			: what == XZAMD_DEBUG_LISTS ? &c->mdist : what == XZAMD_DEBUG_LIST_LENS ? &c->mlen
			: what == XZAMD_DEBUG_SPAN_TAB ? &c->span_tab[c->last_par] : what == XZAMD_DEBUG_SPAN_CNT ? &c->span_cnt[c->last_par]
			: what == XZAMD_DEBUG_SPAN_EST ? &c->est : what == XZAMD_DEBUG_LITP ? &c->litp
			: what == XZAMD_DEBUG_SYM_LEN ? &c->sym_len[c->last_par] : what == XZAMD_DEBUG_SYM_DIST ? &c->sym_dist[c->last_par]
			: what == XZAMD_DEBUG_ENC_TAB ? &c->enc_tab[c->last_par] : what == XZAMD_DEBUG_ENC_CNT ? &c->enc_cnt[c->last_par]
			: what == XZAMD_DEBUG_PINFO ? &c->pinfo[c->last_par] : what == XZAMD_DEBUG_SNAP_SR ? &c->snap_sr
			: what == XZAMD_DEBUG_PRIOR ? &c->prior : what == XZAMD_DEBUG_CARRY ? &c->cb_carry[1]
			: what == XZAMD_DEBUG_CB_HDR ? &c->cb_hdr[1] : what == XZAMD_DEBUG_CB_START ? &c->cb_start[1]
			: what == XZAMD_DEBUG_DELTA_HIST ? &c->dhist : what == XZAMD_DEBUG_DELTA_DIST ? &c->ddist[c->last_par]
			: what == XZAMD_DEBUG_BCJ_HIST ? &c->bhist : what == XZAMD_DEBUG_BCJ_KIND ? &c->bkind[c->last_par] : NULL;
	if (what == XZAMD_DEBUG_LCLP_HIST || what == XZAMD_DEBUG_LCLP_PROPS) {
		/* the statistic and the choices of the last batch, through the kernel layer's own read-back */
		const int hist = what == XZAMD_DEBUG_LCLP_HIST;
		const dbuf *l = hist ? &c->lhist : &c->dprops[c->last_par];
		const uint64_t per = hist ? 4ull * XZAMD_LL_HIST_WORDS : 4ull;
		if (!xzk_lclp_read || !l->p || l->cap < bytes || bytes % per)
			return XZAMD_PROG_ERROR;
		xzk_set_device(c->device);
		return xzk_lclp_read(hist ? (const uint32_t *)l->p : NULL, hist ? NULL : (const uint32_t *)l->p, (uint32_t)(bytes / per),
				hist ? (uint32_t *)out : NULL, hist ? NULL : (uint32_t *)out, c->own_stream) ? XZAMD_DEVICE_ERROR : XZAMD_OK;
	}
	if (!b || !b->p || b->cap < bytes)
		return XZAMD_PROG_ERROR;
	xzk_set_device(c->device);
	if (xzk_d2h(out, b->p, bytes, c->own_stream) || xzk_sync(c->own_stream))
		return XZAMD_DEVICE_ERROR;
	return XZAMD_OK;
}

int xzamd_trace_read(xzamd_ctx *c, uint32_t *out, uint32_t cap, uint32_t *count)
{
	if (!c->trace.p)
		return XZAMD_PROG_ERROR;
	xzk_set_device(c->device);
	uint32_t cnt = 0;
	if (xzk_d2h(&cnt, c->trace.p, 4, c->own_stream) || xzk_sync(c->own_stream))
		return XZAMD_DEVICE_ERROR;
	*count = cnt;
	uint32_t n = cnt < cap ? cnt : cap;
	if (n > c->trace_cap) n = c->trace_cap;
	if (n && (xzk_d2h(out, (uint8_t *)c->trace.p + 16, 16ull * n, c->own_stream) || xzk_sync(c->own_stream)))
		return XZAMD_DEVICE_ERROR;
	c->trace_on = 0;
	return XZAMD_OK;
}

/* ------------------------------------------------------------------ */
/* batch encode                                                         */
/* ------------------------------------------------------------------ */
static uint32_t hash_mask_for(uint32_t dict_size, uint32_t hash_bytes)
{
	/* lz/lz_encoder.c:306-327 */
	uint32_t hs = dict_size - 1;
	hs |= hs >> 1; hs |= hs >> 2; hs |= hs >> 4; hs |= hs >> 8;
	hs >>= 1;
	hs |= 0xFFFF;
	if (hs > (1u << 24)) {
		if (hash_bytes == 3) hs = (1u << 24) - 1;
		else hs >>= 1;
	}
	return hs;
}

typedef struct {
	uint8_t *lits; uint64_t lits_len, lits_cap;
	xzamd_copy_seg *segs; uint64_t nsegs, segs_cap;
} plan;

static uint64_t plan_lit(plan *p, const uint8_t *bytes, uint64_t n, uint64_t dst)
{
	/* literal pieces are packed back to back; one segment each */
	memcpy(p->lits + p->lits_len, bytes, n);
	xzamd_copy_seg *s = &p->segs[p->nsegs++];
	s->src = p->lits_len; s->dst = dst; s->len = n; s->kind = 1; s->pad_ = 0;
	p->lits_len += n;
	return dst + n;
}

static uint64_t plan_seg(plan *p, uint32_t kind, uint64_t src, uint64_t n, uint64_t dst)
{
	if (n == 0)
		return dst;
	xzamd_copy_seg *s = &p->segs[p->nsegs++];
	s->src = src; s->dst = dst; s->len = n; s->kind = kind; s->pad_ = 0;
	return dst + n;
}

/* The knobs of the batch encode, read once per call (not per context: they may change between two calls). */
static uint32_t knob_below(const char *s, uint32_t limit)
{
	const unsigned long v = s ? strtoul(s, NULL, 10) : 0;
	return v >= 1 && v < limit ? (uint32_t)v : 0;
}

static void knobs_read(call_knobs *k)
{
	k->no_overlap = getenv("XZAMD_NO_OVERLAP") != NULL;
	k->back_beside_build = getenv("XZAMD_BACK_BESIDE_BUILD") != NULL;
	k->timing = getenv("XZAMD_TIMING") != NULL;
	{
		/* XZAMD_BUILD_AHEAD = 0 | plan | part | iter1: the event of batch i behind which the build of batch i + 1 starts */
		const char *ba = getenv("XZAMD_BUILD_AHEAD");
		k->build_ahead = !ba || !*ba ? AHEAD_DEFAULT : !strcmp(ba, "plan") ? AHEAD_PLAN : !strcmp(ba, "part") ? AHEAD_PART
				: !strcmp(ba, "iter1") ? AHEAD_ITER1 : !strcmp(ba, "0") ? 0 : AHEAD_DEFAULT;
	}
	/* test knobs: a smaller token budget per input byte, fewer logged bits per span and probability (never more: the
	 * buffers are what they are) */
	k->tok_limit = knob_below(getenv("XZAMD_TEST_TOK_PER_BYTE"), XZAMD_TOK_PER_BYTE);
	k->log_cap = knob_below(getenv("XZAMD_TEST_LOG_CAP"), XZAMD_LOG_CAP);
}

/* Checks the arguments and fills the constants of the call: hash geometry, span size, encode mode, Blocks per batch,
 * which streams the two ends of a batch run on. */
static int call_setup(xzamd_ctx *c, job_env *J, const uint8_t *d_in, uint64_t in_size, uint64_t block_size,
		const xzamd_lzma_options *opt, int check, uint32_t flags, uint8_t *d_out, uint64_t out_cap,
		xzamd_block_info *binfo, uint64_t binfo_cap, void *stream, int may_defer)
{
	if (c->pend_has_result)
		return fail(c, XZAMD_PROG_ERROR, "result of the previous deferred call not collected", 0);
	c->err[0] = 0;
	const uint32_t cbytes = xzamd_check_bytes_(check);
	if (flags & XZAMD_F_SEGMENTS)
		flags |= XZAMD_F_BLOCKS_ONLY;
	if ((unsigned)check > 15)
		return fail(c, XZAMD_PROG_ERROR, "check id out of range", 0);
	/* (internal callers only: the three flags act on the chains of the segments, xzamd_chains.c) */
	const int chains = (flags & XZAMD_F_CHAINS_) != 0;
	if (flags & XZAMD_F_AUTO_DELTA) {
		if (!xzk_delta_stats || !xzk_delta_choose || !xzk_delta_blocks)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto delta: this build has no kernels for it", 0);
		if (opt->bcj != 0)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto delta: the chain already has a filter in front of LZMA2", 0);
		if (flags & XZAMD_F_SEGMENTS)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto delta: Blocks only -- the segments of one Block share its chain", 0);
		if (flags & XZAMD_F_REPAIR)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto delta: not with XZAMD_F_REPAIR (the repair plans Block Headers from one chain)", 0);
	}
	if (flags & XZAMD_F_AUTO_BCJ) {
		if (!xzk_bcj_stats || !xzk_bcj_choose || !xzk_bcj_blocks)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto bcj: this build has no kernels for it", 0);
		if (opt->bcj != 0)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto bcj: the chain already has a filter in front of LZMA2", 0);
		if (flags & XZAMD_F_SEGMENTS)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto bcj: Blocks only -- the segments of one Block share its chain", 0);
		if (flags & XZAMD_F_REPAIR)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto bcj: not with XZAMD_F_REPAIR (the repair plans Block Headers from one chain)", 0);
	}
	if (flags & XZAMD_F_AUTO_LCLP) {
		if (!xzk_lclp_stats || !xzk_lclp_choose)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto lclp: this build has no kernels for it", 0);
		if (flags & XZAMD_F_SEGMENTS)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto lclp: Blocks only, not the chunk chains of XZAMD_F_SEGMENTS", 0);
		if (flags & XZAMD_F_REPAIR)
			return fail(c, XZAMD_OPTIONS_ERROR, "auto lclp: not with XZAMD_F_REPAIR (the repair re-encodes Blocks with the job's lc / lp)", 0);
	}
	if (chains && (!(flags & XZAMD_F_SEGMENTS) || !xzamd_chains_encoded_))
		return fail(c, XZAMD_OPTIONS_ERROR, "chains: this build has no unit for bare chunk chains", 0);
	if ((flags & XZAMD_F_REPAIR) && (flags & XZAMD_F_SEGMENTS) && !chains)
		return fail(c, XZAMD_OPTIONS_ERROR, "repair: Blocks only, not the chunk chains of XZAMD_F_SEGMENTS", 0);
	if ((flags & (XZAMD_F_KEEP_RESUME | XZAMD_F_VERIFY)) && (flags & XZAMD_F_BLOCKS_ONLY) && !(flags & XZAMD_F_REPAIR) && !chains)
		return fail(c, XZAMD_OPTIONS_ERROR, "keep_resume / verify need a whole Stream: not with XZAMD_F_BLOCKS_ONLY or XZAMD_F_SEGMENTS", 0);
	if (flags & XZAMD_F_REPAIR) {
		if (!xzamd_repair_encoded_)
			return fail(c, XZAMD_OPTIONS_ERROR, "repair: this build has no repair unit", 0);
		flags |= XZAMD_F_VERIFY;
	}
	if ((flags & (XZAMD_F_KEEP_RESUME | XZAMD_F_VERIFY)) && (!xzk_resume_export || !xzamd_verify_kept_))
		return fail(c, XZAMD_OPTIONS_ERROR, "keep_resume / verify: this build has no resume export or no device decoder", 0);
	if ((flags & XZAMD_F_SEGMENTS) && (check == XZAMD_CHECK_SHA256 || opt->bcj != 0))
		return fail(c, XZAMD_OPTIONS_ERROR, "segments: the chain {LZMA2} and a Check that can be combined from parts (none, CRC32, CRC64)", 0);
	if (cbytes == 0xFFFFFFFFu)
		return fail(c, XZAMD_UNSUPPORTED_CHECK, "checks: none, CRC32, CRC64, SHA-256", 0);
	{
		const char *why = xzamd_options_check(opt);
		if (why)
			return fail(c, XZAMD_OPTIONS_ERROR, why, 0);
	}
	if (block_size == 0)
		block_size = xzamd_mt_block_size(opt);
	if (block_size >= (1ull << 31))
		return fail(c, XZAMD_OPTIONS_ERROR, "block_size must be < 2 GiB", 0);
	void *st = stream ? stream : c->own_stream;
	{
		int e = xzk_set_device(c->device);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "hipSetDevice", e);
	}

	knobs_read(&J->k);
	J->m = xzamd_mode_of_(opt);
	J->hb = opt->gpu_mf & 0x0F;
	J->hmask = hash_mask_for(opt->dict_size, J->hb);
	while ((1ull << J->hbits) <= J->hmask) ++J->hbits;     /* also the widest 32-bit sort key family */
	J->span = (opt->span_size == XZAMD_SPAN_DEFAULT || opt->span_size == XZAMD_SPAN_AUTO) ? J->m.span_default : opt->span_size;
	if (J->span > block_size) J->span = (uint32_t)block_size;
	if (J->span < 4096)
		return fail(c, XZAMD_OPTIONS_ERROR, "span_size must be >= 4096", 0);

	/* batch = whole Blocks, n < 2^31, (nblocks+1) << hbits < 2^32 */
	uint64_t max_blocks = c->batch_bytes / block_size;
	if (max_blocks == 0) max_blocks = 1;
	const uint64_t key_blocks = (1ull << (32 - J->hbits)) - 2;
	if (max_blocks > key_blocks) max_blocks = key_blocks;
	if (max_blocks * block_size >= (1ull << 31))
		max_blocks = ((1ull << 31) - 1) / block_size;
	if (max_blocks == 0)
		return fail(c, XZAMD_OPTIONS_ERROR, "block_size too large for one device batch", 0);

	const uint64_t total_blocks = (in_size + block_size - 1) / block_size;
	if ((flags & (XZAMD_F_REPAIR | (chains ? XZAMD_F_VERIFY : 0u))) && (flags & XZAMD_F_BLOCKS_ONLY) && total_blocks
			&& (!binfo || binfo_cap < total_blocks))
		return fail(c, XZAMD_PROG_ERROR, "repair of bare Blocks: binfo must hold every Block (it is their table)", 0);
	/* A batch must fit the device memory with room to spare: the work buffers take 100 - 165 bytes per input byte
	 * (DESIGN.md section 2), and the runtime allocates kernel scratch (register spills of the parser) lazily at launch --
	 * an allocation that fails there surfaces as an error of some later call, not as a clean out-of-memory here.  So
	 * the batch is capped at 80 % of what is free now plus what this context already holds. */
	{
		double per_byte = xzamd_work_bytes_per_byte_(opt);
		if (flags & XZAMD_F_AUTO_DELTA) per_byte += xzamd_auto_delta_bytes_per_byte_(block_size);
		if (flags & XZAMD_F_AUTO_BCJ) per_byte += xzamd_auto_bcj_bytes_per_byte_(block_size, (flags & XZAMD_F_AUTO_DELTA) != 0);
		if (flags & XZAMD_F_AUTO_LCLP) per_byte += xzamd_auto_lclp_bytes_per_byte_(block_size);
		/* the resume table (only when asked for): one record per encode-span slot, for the whole call */
		if ((flags & (XZAMD_F_KEEP_RESUME | XZAMD_F_VERIFY)) && J->m.two)
			per_byte += (double)(XZAMD_RESUME_BYTES(J->m.model_slots) + 32u) * (double)(block_size / XZAMD_ENC_MIN_LEN + 1) / (double)block_size;
		uint64_t free_b = 0, total_b = 0, held = 0;
		if (xzk_mem_info(&free_b, &total_b) == 0 && total_b != 0) {
			dbuf *d[CTX_NBUF_MAX];
			size_t nd = 0;
			ctx_device_bufs(c, d, &nd);
			for (size_t i = 0; i < nd; ++i) held += d[i]->cap;
			const double budget = 0.80 * (double)(free_b + held);
			uint64_t fit = (uint64_t)(budget / per_byte) / block_size;
			if (fit == 0) fit = 1;
			if (fit < max_blocks) max_blocks = fit;
		}
	}
	/* even batches: a short last launch cannot fill the GPU (one wavefront per span) */
	if (total_blocks > max_blocks) {
		const uint64_t nbatch = (total_blocks + max_blocks - 1) / max_blocks;
		max_blocks = (total_blocks + nbatch - 1) / nbatch;
	}
	const int adaptive = J->m.adaptive, two = J->m.two;
	J->spb = adaptive ? (uint32_t)(block_size / XZAMD_SPAN_MIN_LEN + 2) : (uint32_t)((block_size + J->span - 1) / J->span);   /* span slots per Block */
	J->esb = two ? (uint32_t)(block_size / XZAMD_ENC_MIN_LEN + 1) : 0;      /* encode-span slots per Block */
	J->cpb = (uint32_t)((block_size + XZAMD_EST_CHUNK - 1) / XZAMD_EST_CHUNK);
	J->filtered = opt->bcj != 0;          /* any filter in front of LZMA2: the encoder reads a filtered copy */
	J->auto_delta = (flags & XZAMD_F_AUTO_DELTA) != 0;     /* ... or the copy in which every Block has the filter chosen for it */
	J->auto_bcj = (flags & XZAMD_F_AUTO_BCJ) != 0;
	J->auto_lclp = (flags & XZAMD_F_AUTO_LCLP) != 0;
	/* Two-stream pipeline (two-phase mode): the back end of batch i -- range coder, checks, sizes, gather -- runs on the
	 * second stream while the front end of batch i + 1 -- match structures, plan, parse -- runs on the caller's: the coder
	 * is a few thousand latency-bound wavefronts, the structure build is HBM-bound, they share the GPU well.  The
	 * single-phase kernels read the match structures while they code, so their batches stay serial. */
	const int overlap_ok = two && !J->k.no_overlap;
	J->defer = may_defer && overlap_ok && (flags & XZAMD_F_BLOCKS_ONLY) && total_blocks > 0 && !(flags & (XZAMD_F_REPAIR | XZAMD_F_VERIFY));
	/* a batch carried over from the previous call: it can only be finished underneath this call's front end when this call
	 * runs the same two-stream scheme on the same streams; else it is finished first */
	if (c->pend.active && !(overlap_ok && c->pend.J.st == st))
		(void)pend_complete(c);      /* its result (good or bad) belongs to the deferred call: xzamd_encode_finish_ hands it out;
		                              * nothing of THIS call has failed */
	J->pipelined = overlap_ok && (total_blocks > max_blocks || J->defer || c->pend.active);
	/* two-phase: the lists of the seed regions first, so that the seed pieces (one wavefront per Block, latency
	 * bound) can be parsed on a third stream underneath the rest of the finder (HBM bound) */
	J->seeds_early = overlap_ok && block_size >= XZAMD_SEED_LEN + 1024;
	/* Build ahead: on the list-finder path the structure is read by the finder only, so the build of batch i + 1 can run
	 * under the parse of batch i.  The single-phase kernels read it while they code (never pipelined); a deferred batch is
	 * carried into a call whose input is not known yet, so nothing is built ahead across calls. */
	J->ahead = J->pipelined && opt->gpu_parser ? J->k.build_ahead : 0;
	J->sta = c->st4 ? c->st4 : c->st3;

	J->opt = opt; J->d_in = d_in; J->d_out = d_out; J->in_size = in_size; J->block_size = block_size; J->out_cap = out_cap;
	J->total_blocks = total_blocks; J->max_blocks = max_blocks;
	J->bound = xzamd_block_buffer_bound(block_size);
	J->binfo = binfo; J->binfo_cap = binfo_cap;
	J->cbytes = cbytes; J->hs_fixed = xzamd_block_header_size_(J->bound, block_size, opt);
	if (J->auto_delta) {
		/* the header is per Block: one of two sizes (every delta distance takes the same three bytes of Filter Flags) */
		xzamd_lzma_options view = *opt;
		view.bcj = XZAMD_FILTER_DELTA(1);
		J->hs_delta = xzamd_block_header_size_(J->bound, block_size, &view);
	}
	if (J->auto_bcj) {
		xzamd_lzma_options view = *opt;
		view.bcj = XZAMD_BCJ_X86;
		J->hs_bcj = xzamd_block_header_size_(J->bound, block_size, &view);
	}
	J->check = check;
	J->dbyte = xzamd_dict_size_byte_(opt->dict_size);
	J->st = st; J->stb = J->pipelined ? c->st2 : st;
	J->whole = !(flags & XZAMD_F_BLOCKS_ONLY);
	J->segments = (flags & XZAMD_F_SEGMENTS) != 0;
	J->resume = (flags & (XZAMD_F_KEEP_RESUME | XZAMD_F_VERIFY)) && two;
	J->verify = (flags & XZAMD_F_VERIFY) != 0;
	J->repair = (flags & XZAMD_F_REPAIR) != 0;
	/* the table of the encode before is that encode's: gone with this one (its memory too, unless this call fills it again) */
	c->resume.valid = 0;
	if (c->resume_tab.p && !J->resume && !c->pend.active) {
		xzk_free(c->resume_tab.p);
		c->resume_tab.p = NULL; c->resume_tab.cap = 0;
	}
	if (J->resume) {
		const uint64_t cap = total_blocks * J->esb;
		if (cap >= 0xFFFFFFFFull)
			return fail(c, XZAMD_OPTIONS_ERROR, "too many encode spans for a resume table", 0);
		int r = dgrow(c, &c->resume_tab, (cap ? cap : 1) * XZAMD_RESUME_BYTES(J->m.model_slots), 0);
		if (r) return r;
	}

	memset(&c->stats, 0, sizeof(c->stats));
	c->stats.span_size = adaptive ? 0 : J->span;
	c->stats.wave_slots = c->wave_slots;
	return XZAMD_OK;
}

/* A whole Stream: the per-Block records the Index is made of, and the Stream Header */
static int stream_begin(xzamd_ctx *c, job_env *J)
{
	uint8_t hdr[12];
	J->rec_unp = (uint64_t *)malloc(sizeof(uint64_t) * (J->total_blocks + 1) * 2);
	if (!J->rec_unp)
		return fail(c, XZAMD_MEM_ERROR, "malloc", 0);
	J->rec_unc = J->rec_unp + J->total_blocks + 1;
	if (J->out_cap < 12) { free(J->rec_unp); return fail(c, XZAMD_BUF_ERROR, "output buffer too small", 0); }
	xzamd_frame_header(hdr, J->check);
	int e = xzk_h2d(J->d_out, hdr, 12, J->st);
	if (!e) e = xzk_sync(J->st);
	if (e) { free(J->rec_unp); return fail(c, XZAMD_DEVICE_ERROR, "h2d header", e); }
	J->opos = 12;
	return XZAMD_OK;
}

/* Index and Stream Footer behind the last Block */
static int stream_end(xzamd_ctx *c, job_env *J)
{
	const uint64_t isz_cap = 32 + J->total_blocks * 18 + 16;
	uint8_t *ib = (uint8_t *)malloc(isz_cap);
	if (!ib)
		return fail(c, XZAMD_MEM_ERROR, "malloc", 0);
	int rc = XZAMD_OK;
	const uint64_t w = xzamd_frame_index_footer(ib, isz_cap, J->check, J->rec_unp, J->rec_unc, J->total_blocks);
	if (w == 0 || J->opos + w > J->out_cap) rc = fail(c, XZAMD_BUF_ERROR, "output buffer too small", 0);
	else {
		int e = xzk_h2d(J->d_out + J->opos, ib, w, J->st);
		if (!e) e = xzk_sync(J->st);
		if (e) rc = fail(c, XZAMD_DEVICE_ERROR, "h2d index", e);
		J->opos += w;
	}
	free(ib);
	return rc;
}

/* Geometry of the batch that starts at Block b0: its Blocks and bytes, the slots of its tables, the sorts' scratch. */
static int batch_geometry(xzamd_ctx *c, const job_env *J, uint64_t b0, batch_run *B)
{
	const uint64_t block_size = J->block_size;
	memset(B, 0, sizeof(*B));
	B->b0 = b0;
	B->nb = J->total_blocks - b0 < J->max_blocks ? J->total_blocks - b0 : J->max_blocks;
	B->in_off = b0 * block_size;
	const uint64_t n64 = J->in_size - B->in_off < B->nb * block_size ? J->in_size - B->in_off : B->nb * block_size;
	B->n = (uint32_t)n64;
	B->n64 = B->n;
	uint32_t bb = 0;
	while ((1u << bb) < B->nb + 1) ++bb;
	const uint32_t bits[4] = { 10 + bb, 16 + bb, J->hbits + bb, 32 };   /* 32: the by-position inversions */
	for (int i = 0; i < 4; ++i) {
		uint64_t sbytes = 0;
		int e = xzk_sort_temp_bytes(B->n, bits[i], &sbytes);
		if (e)
			return fail(c, XZAMD_DEVICE_ERROR, "rocprim temp size", e);
		if (sbytes > B->sort_bytes) B->sort_bytes = sbytes;
	}
	if (J->opt->gpu_sa_window) {
		uint64_t sbytes = 0;
		int e = xzk_sa_temp_bytes(B->n, &sbytes);
		if (e)
			return fail(c, XZAMD_DEVICE_ERROR, "rocprim temp size (suffix order)", e);
		if (sbytes > B->sort_bytes) B->sort_bytes = sbytes;
	}
	B->nspans = (uint32_t)(B->nb * J->spb);
	B->nenc = (uint32_t)(B->nb * J->esb);
	B->nout = J->m.two ? B->nenc : B->nspans;            /* slots that write coded bytes */
	B->opb = J->m.two ? J->esb : J->spb;
	B->nch = J->m.two ? XZAMD_CHUNK_SLOTS(B->n, B->nenc) : 0;      /* chunk slots of the two-phase coder */
	/* plan capacity: per Block header + spans + trailer, or the stored form */
	const uint64_t segs_per_block = (J->m.two ? (block_size >> 13) + 2ull * J->esb + 2 : B->opb) + 2 + 2 * ((block_size + 65535) / 65536) + 2;
	B->max_segs = B->nb * segs_per_block + 4;
	B->max_lits = B->nb * (64 + 3 * ((block_size + 65535) / 65536) + 32) + 64;
	return XZAMD_OK;
}

/* Every buffer of the batch at the size the batch needs.  Returns the first failure of dgrow: XZAMD_MEM_ERROR when the
 * device (or the pinned host memory) does not have it -- the batch loop then tries a smaller batch.  With `probe` it only
 * asks whether a buffer would have to grow: a batch is issued ahead only into buffers that are already there. */
static int batch_reserve(xzamd_ctx *c, const job_env *J, const batch_run *B, int probe)
{
	const xzamd_lzma_options *opt = J->opt;
	const int two = J->m.two, par = B->par;
	const uint64_t n = B->n, nb = B->nb, nspans = B->nspans, nenc = B->nenc, nout = B->nout, nch = B->nch;
	const uint64_t mslots = J->m.model_slots;
	const uint64_t spb_crc = (J->block_size + CRC_STRIP - 1) / CRC_STRIP;
	int r = 0;
	/* (nothing more is asked for once one request has failed) */
	/* probe: nothing is allocated or freed; the answer is whether every buffer already has its size (0) or not (1) */
#define NEED(buf, bytes, host) (r = r ? r : probe ? c->buf.cap < (uint64_t)(bytes) : dgrow(c, &c->buf, (bytes), host))
	NEED(keys_a, 4 * n, 0); NEED(keys_b, 4 * n, 0);
	NEED(vals_a, 4 * n, 0); NEED(vals_b, 4 * n, 0);
	NEED(prev2, 4 * n, 0); NEED(prev3, 4 * n, 0);
	if (opt->gpu_sa_window) {
		NEED(prev4, 4 * n, 0); NEED(prev8, 8 * n, 0); NEED(prev16, 8 * n, 0);   /* prev8/16: (rank, distance) pairs */
		NEED(prev24, 4 * n, 0); NEED(prev32, 4 * n, 0);
		NEED(key64_a, 8 * n, 0); NEED(key64_b, 8 * n, 0);
		NEED(sa, 4 * n, 0); NEED(sa_rank, 4 * n, 0);
	} else {
		NEED(rank, 4 * n, 0); NEED(sorted_pos, 4 * n, 0);
	}
	NEED(sort_tmp, B->sort_bytes + 256, 0);
	NEED(scratch, two ? n + (n >> 3) + 64 + 32 * nch : n + (n >> 3) + 32 + XZAMD_SPAN_SLACK * nout, 0);
	NEED(span_bytes, 4 * nout, 0);
	NEED(span_tab[par], 8 * nspans, 0);
	NEED(span_cnt[par], 4 * nb, 0);
	NEED(h_span_tab, 8 * nspans, 1);
	NEED(h_span_cnt[par], 4 * nb + 16, 1);
	if (two) {
		NEED(sym_len[par], 2 * n + 64, 0);
		NEED(sym_dist[par], 4 * n + 64, 0);
		NEED(prior, 4ull * XZAMD_PRIOR_WORDS * nspans, 0);
		NEED(enc_tab[par], 8 * nenc, 0);
		NEED(enc_cnt[par], 4 * nb, 0);
		NEED(h_enc_tab[par], 8 * nenc, 1);
		NEED(h_enc_cnt[par], 4 * nb + 16, 1);
		NEED(tok, 2 * (n * XZAMD_TOK_PER_BYTE + 4096 * nenc + 64), 0);
		NEED(pinfo[par], 4ull * XZAMD_PINFO_WORDS * nspans, 0);
		NEED(snap_sr, 32 * nspans, 0);
		NEED(part_tab, 4 * nspans + 16, 0);
		for (int f = 0; f < 2; ++f) {
			NEED(cb_bnd[f], 4 * mslots * nenc, 0);
			NEED(cb_log[f], 4ull * XZAMD_LOG_WORDS * mslots * nenc, 0);
			NEED(cb_hdr[f], 4 * nenc + 16, 0);
			NEED(cb_start[f], 2 * mslots * nenc + 16, 0);
			NEED(cb_carry[f], 4 * nenc + 16, 0);
		}
		if (J->resume) NEED(resume_sr, 32 * nenc + 32, 0);
		NEED(chunks, nch * sizeof(xzamd_chunk), 0);
		NEED(h_chunks, nch * sizeof(xzamd_chunk), 1);
	}
	if (J->m.adaptive) {
		NEED(est, 8 * nb * J->cpb, 0);
		NEED(totals, 8 * (nb + 2), 0);
		NEED(order, 16 * nspans, 0);
	}
	NEED(strip_crc, 8 * spb_crc * nb, 0);
	NEED(block_crc, 32 * nb, 0);
	NEED(errw, 512, 0);
	NEED(errw2, 512, 0);
	NEED(h_err[par], 1024, 1);
	NEED(litp, nspans * (0x300ull << (opt->lc + opt->lp)) * 4ull, 0);
	if (opt->gpu_parser) {
		/* per-position match lists: 8 x u32 (7 entries + trailer), + 8 x u16 lengths when not packed */
		if (!J->m.list_packed) NEED(mlen, 16 * n, 0);
		NEED(mdist, 32 * n, 0);
		/* + 32: k_span_est reads the summaries eight at a time (16 bytes) and may look past the last position */
		if (opt->gpu_sa_window) NEED(mtop, 2 * n + 32, 0);
	}
	NEED(h_span_bytes, 4 * nout, 1);
	NEED(h_block_crc, 32 * nb, 1);
	NEED(segs, B->max_segs * sizeof(xzamd_copy_seg), 0);
	NEED(lits, B->max_lits, 0);
	NEED(h_segs, B->max_segs * sizeof(xzamd_copy_seg), 1);
	NEED(h_lits, B->max_lits, 1);
	if (J->filtered || J->auto_delta || J->auto_bcj) NEED(bcj[par], n + 16, 0);
	if (J->auto_bcj) {
		NEED(bhist, 4ull * (XZAMD_AB_HIST_WORDS + XZAMD_AB_NCAND) * nb, 0);
		NEED(bkind[par], 4 * nb, 0);
		NEED(h_bkind[par], 4 * nb + 16, 1);
	}
	if (J->auto_delta) {
		NEED(dhist, 4ull * XZAMD_AD_HIST_WORDS * nb, 0);
		NEED(ddist[par], 4 * nb, 0);
		NEED(h_ddist[par], 4 * nb + 16, 1);
	}
	if (J->auto_lclp) {
		NEED(lhist, 4ull * XZAMD_LL_HIST_WORDS * nb, 0);
		NEED(dprops[par], 4 * nb, 0);
	}
	if (opt->bcj2) NEED(bcjt, n + 16, 0);
#undef NEED
	return r;
}

/* What the kernels of a batch's front end and of its coder are called with */
static void span_args_init(const xzamd_ctx *c, const job_env *J, const batch_run *B, xzamd_span_args *a)
{
	const xzamd_lzma_options *opt = J->opt;
	const int par = B->par;
	memset(a, 0, sizeof(*a));
	a->in = B->enc_in;
	a->rank = (const uint32_t *)c->rank.p;
	a->sorted_pos = (const uint32_t *)c->sorted_pos.p;
	a->prev2 = (const uint32_t *)c->prev2.p;
	a->prev3 = (const uint32_t *)c->prev3.p;
	a->sa_window = opt->gpu_sa_window;
	a->parser = opt->gpu_parser;
	a->scratch = (uint8_t *)c->scratch.p;
	a->span_tab = (const uint32_t *)c->span_tab[par].p;
	a->span_cnt = (const uint32_t *)c->span_cnt[par].p;
	a->max_spb = J->spb;
	a->span_bytes = (uint32_t *)c->span_bytes.p;
	a->err = (uint32_t *)c->errw.p;
	a->lit = (uint32_t *)c->litp.p;
	if (c->trace_on) {
		a->trace_count = (uint32_t *)c->trace.p;
		a->trace = (uint32_t *)((uint8_t *)c->trace.p + 16);
		a->trace_cap = c->trace_cap;
	}
	a->n = B->n;
	a->block_size = (uint32_t)J->block_size;
	a->span_size = J->span;
	a->dict_size = opt->dict_size;
	a->nice_len = opt->gpu_nice_len;
	a->depth = opt->gpu_depth;
	a->hash_bytes = J->hb;
	a->lc = opt->lc; a->lp = opt->lp; a->pb = opt->pb;
	a->props_tab = J->auto_lclp ? (const uint32_t *)c->dprops[par].p : NULL;      /* (this batch's parity: front end and coder alike) */
	if (J->m.two) {
		a->sym_len = (uint16_t *)c->sym_len[par].p;
		a->sym_dist = (uint32_t *)c->sym_dist[par].p;
		a->prior = (uint32_t *)c->prior.p;
		a->enc_tab = (const uint32_t *)c->enc_tab[par].p;
		a->enc_cnt = (const uint32_t *)c->enc_cnt[par].p;
		a->max_esb = J->esb;
		a->enc_bits = opt->enc_span_bits;
		a->tok_limit = J->k.tok_limit;
		a->log_cap = J->k.log_cap;
		a->tok = (uint16_t *)c->tok.p;
		a->chunks = (xzamd_chunk *)c->chunks.p;
		a->pinfo = (uint32_t *)c->pinfo[par].p;
		a->snap_sr = (uint32_t *)c->snap_sr.p;
		a->part_tab = (uint32_t *)c->part_tab.p;
		a->model_slots_pad = J->m.model_slots;
		a->resume_sr = J->resume ? (uint32_t *)c->resume_sr.p : NULL;
		/* (the front end's set of the carried-walk buffers; the back end switches to its own) */
		a->cb_bnd = (uint32_t *)c->cb_bnd[0].p; a->cb_log = (uint32_t *)c->cb_log[0].p; a->cb_hdr = (uint32_t *)c->cb_hdr[0].p;
		a->cb_start = (uint16_t *)c->cb_start[0].p; a->cb_carry = (uint32_t *)c->cb_carry[0].p;
	}
	if (opt->gpu_parser) {
		/* the lists the batch match finder writes and the parser streams */
		a->mlen = J->m.list_packed ? NULL : (uint16_t *)c->mlen.p;
		a->list_packed = (uint32_t)J->m.list_packed;
		a->mdist = (uint32_t *)c->mdist.p;
		a->mtop = (uint16_t *)c->mtop.p;
	}
}

/* First half of a batch's back end, enqueued on the back-end stream: model pass + range coder (two-phase), Block checks,
 * D2H of the sizes.  Everything it needs of its batch is in `back_args`, so that the batch loop can enqueue it where it
 * likes: behind the structure build of the NEXT batch, beside its finder (the default for a batch that has one behind it), or
 * right behind the batch's own front end, beside the next batch's sorts (XZAMD_BACK_BESIDE_BUILD=1; the last batch of a call). */
typedef struct {
	int valid;
	xzamd_span_args a;
	batch_run B;
} back_args;

static int back_enqueue(xzamd_ctx *c, const job_env *J, back_args *BA)
{
	const batch_run *B = &BA->B;
	void *stb = J->stb;
	void **ev = c->evp[B->par];
	const int two = J->m.two, check = J->check;
	const uint64_t nb = B->nb, block_size = J->block_size;
	const uint32_t n = B->n;
	int e = 0;
	BA->valid = 0;
	if (stb != J->st) e = xzk_stream_wait_event(stb, ev[EV_FRONT]);
	xzk_event_record(ev[EV_BACK0], stb);
	if (!e) e = xzk_memset(c->errw2.p, 0, 512, stb);
	if (!e && two) {
		xzamd_span_args a2 = BA->a;
		a2.err = (uint32_t *)c->errw2.p;
		a2.cb_bnd = (uint32_t *)c->cb_bnd[1].p; a2.cb_log = (uint32_t *)c->cb_log[1].p; a2.cb_hdr = (uint32_t *)c->cb_hdr[1].p;
		a2.cb_start = (uint16_t *)c->cb_start[1].p; a2.cb_carry = (uint32_t *)c->cb_carry[1].p;
		e = xzk_encode_syms(&a2, (uint32_t)nb, stb);
		/* the batch's resume records, while the coder's buffer set still holds this batch (the batches' back ends run in
		 * order: rec_done counts the records of every batch in front of this one) */
		if (!e && J->resume)
			e = xzk_resume_export(&a2, (uint32_t)nb, (uint32_t)B->b0, (uint8_t *)c->resume_tab.p, J->rec_done,
					(uint32_t)(J->total_blocks * J->esb), stb);
	}
	xzk_event_record(ev[EV_CODE], stb);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "encode_syms launch", e);
	/* Block checks */
	if (check == XZAMD_CHECK_CRC64 || check == XZAMD_CHECK_CRC32) {
		e = xzk_crc_blocks(J->d_in + B->in_off, n, (uint32_t)block_size, (uint32_t)nb, CRC_STRIP,
				check == XZAMD_CHECK_CRC32, (uint64_t *)c->strip_crc.p, (uint64_t *)c->block_crc.p, stb);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "crc64 launch", e);
		e = xzk_d2h(c->h_block_crc.p, c->block_crc.p, 8ull * nb, stb);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "d2h crc", e);
	} else if (check == XZAMD_CHECK_SHA256) {
		e = B->sha_early ? xzk_stream_wait_event(stb, c->ev_sha)
				: xzk_sha256_blocks(J->d_in + B->in_off, n, (uint32_t)block_size, (uint32_t)nb, (uint8_t *)c->block_crc.p, stb);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "sha256 launch", e);
		e = xzk_d2h(c->h_block_crc.p, c->block_crc.p, 32ull * nb, stb);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "d2h sha256", e);
	}
	xzk_event_record(ev[EV_CRC], stb);
	e = two ? xzk_d2h(c->h_chunks.p, c->chunks.p, (uint64_t)B->nch * sizeof(xzamd_chunk), stb)
			: xzk_d2h(c->h_span_bytes.p, c->span_bytes.p, 4ull * B->nout, stb);
	if (!e) e = xzk_d2h((uint8_t *)c->h_err[B->par].p + 512, c->errw2.p, 512, stb);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "d2h sizes", e);
	return XZAMD_OK;
}

/* The back end's kernels are through: what they timed (XZAMD_TIMING) and what their consistency checks found */
static int back_report(xzamd_ctx *c, const job_env *J, const batch_run *B)
{
	int e = xzk_sync(J->stb);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "span encode / d2h sizes", e);
	const uint32_t *herr = (const uint32_t *)c->h_err[B->par].p;       /* front end: parser / single-phase span kernel */
	const uint32_t *herr2 = herr + 128;                                /* back end: coder of the two-phase mode */
	if (J->k.timing && herr[8])
		fprintf(stderr, "[timing span0] total %u round1 %u round2 %u encode %u (x256 clk) rounds %u symbols %u\n",
				herr[8], herr[9], herr[10], herr[11], herr[12], herr[13]);
	if (J->k.timing) {
		const uint64_t *t = (const uint64_t *)(herr + 16);
		if (t[8])
			fprintf(stderr, "[timing opt, Mcycles summed over spans] total %llu | derive %llu round %llu bits %llu lit %llu relax %llu "
					"backtrack %llu encode %llu refresh %llu | nodes %llu symbols %llu windows %llu | span max %llu Mcyc | compound nodes %llu price %llu gather %llu\n",
					(unsigned long long)(t[8] >> 20), (unsigned long long)(t[0] >> 20), (unsigned long long)(t[1] >> 20),
					(unsigned long long)(t[2] >> 20), (unsigned long long)(t[3] >> 20), (unsigned long long)(t[4] >> 20),
					(unsigned long long)(t[5] >> 20), (unsigned long long)(t[6] >> 20), (unsigned long long)(t[7] >> 20),
					(unsigned long long)t[9], (unsigned long long)t[10], (unsigned long long)t[11],
					(unsigned long long)(t[12] >> 20), (unsigned long long)t[13], (unsigned long long)(t[14] >> 20), (unsigned long long)(t[15] >> 20));
		const uint64_t *t2 = (const uint64_t *)(herr2 + 48);
		if (t2[0])
			fprintf(stderr, "[timing coder, Mcycles summed over encode spans] total %llu | encode_symbol %llu of which rc_run %llu | "
					"symbols %llu bits %llu | span max %llu Mcyc\n", (unsigned long long)(t2[0] >> 20), (unsigned long long)(t2[1] >> 20),
					(unsigned long long)(t2[2] >> 20), (unsigned long long)t2[3], (unsigned long long)t2[4], (unsigned long long)(t2[5] >> 20));
	}
	const uint32_t *he = herr[0] ? herr : herr2[0] ? herr2 : NULL;
	if (he) {
		snprintf(c->err_msg_buf, sizeof(c->err_msg_buf),
				"span encoder consistency check %u failed: %u %u %u %u %u %u %u",
				he[0], he[1], he[2], he[3], he[4], he[5], he[6], he[7]);
		return fail(c, XZAMD_PROG_ERROR, c->err_msg_buf, 0);
	}
	return XZAMD_OK;
}

/* Block b of the batch at *opos of the Stream: Block Header, the coded spans in order (or the stored form), padding and
 * Check go into the gather plan; its sizes into the Index records and the caller's table. */
static int layout_block(xzamd_ctx *c, job_env *J, const batch_run *B, plan *pl, uint64_t b, uint64_t *opos_io, int *stored_out)
{
	*stored_out = 0;
	const uint64_t block_size = J->block_size;
	const uint32_t opb = B->opb, cbytes = J->cbytes;
	const int two = J->m.two, check = J->check, par = B->par;
	const uint32_t *sb = (const uint32_t *)c->h_span_bytes.p;
	const xzamd_chunk *hch = (const xzamd_chunk *)c->h_chunks.p;
	const uint32_t *hcnt = (const uint32_t *)c->h_span_cnt[par].p;
	/* the slots that hold coded bytes: the spans of the plan, or (two-phase) the encode spans */
	const uint32_t *otab = (const uint32_t *)(two ? c->h_enc_tab[par].p : c->h_span_tab.p);
	const uint32_t *ocnt = (const uint32_t *)(two ? c->h_enc_cnt[par].p : c->h_span_cnt[par].p);
	const uint64_t *bcrc = (const uint64_t *)c->h_block_crc.p;
	uint64_t opos = *opos_io;
	uint8_t small[64];

	const uint64_t boff = b * block_size;                 /* in batch */
	const uint64_t usize = B->n64 - boff < block_size ? B->n64 - boff : block_size;
	uint64_t payload = 1;                                 /* end marker */
	const uint32_t nsp = ocnt[b];                         /* coded spans of this Block (slots b * opb ...) */
	if (nsp == 0 || nsp > opb || hcnt[b] == 0 || hcnt[b] > J->spb)
		return fail(c, XZAMD_PROG_ERROR, "span plan out of range", 0);
	if (two) {
		/* the chunks of the Block's encode spans, in order (k_model_syms / k_rc_chunks) */
		for (uint32_t s = 0; s < nsp; ++s) {
			const uint32_t slot = (uint32_t)(b * opb + s), st0 = otab[2 * slot], en0 = otab[2 * slot + 1];
			const uint32_t cb = XZAMD_CHUNK_BASE(st0, slot), cc = XZAMD_CHUNK_CAP(en0 - st0);
			uint64_t covered = 0;
			for (uint32_t k = 0; k < cc && hch[cb + k].usize != 0; ++k) {
				if (hch[cb + k].csize == 0 || hch[cb + k].in_start != st0 + covered)
					return fail(c, XZAMD_PROG_ERROR, "chunk table inconsistent", 0);
				payload += hch[cb + k].csize;
				covered += hch[cb + k].usize;
			}
			if (covered != (uint64_t)en0 - st0)
				return fail(c, XZAMD_PROG_ERROR, "chunks do not cover their encode span", 0);
		}
	} else {
		for (uint32_t s = 0; s < nsp; ++s)
			payload += sb[b * opb + s];
	}
	const uint64_t pad = (4 - (payload & 3)) & 3;
	const uint64_t bstart = opos;
	/* the Block's own chain (XZAMD_F_AUTO_DELTA): the job's options with the filter chosen for this Block */
	xzamd_lzma_options bopt = *J->opt;
	uint32_t hs_coded = J->hs_fixed;
	if (J->auto_delta) {
		const uint32_t d = ((const uint32_t *)c->h_ddist[par].p)[b];
		if (d > XZAMD_AD_MAXDIST)
			return fail(c, XZAMD_PROG_ERROR, "automatic delta: distance out of range", 0);
		if (d != 0) { bopt.bcj = XZAMD_FILTER_DELTA(d); hs_coded = J->hs_delta; }
	}
	if (J->auto_bcj) {
		/* (the BCJ rule goes first: where it fires the device has cleared the Block's delta distance) */
		const uint32_t kd = ((const uint32_t *)c->h_bkind[par].p)[b];
		if (kd != 0 && kd != XZAMD_BCJ_X86 && kd != XZAMD_BCJ_ARM64)
			return fail(c, XZAMD_PROG_ERROR, "automatic bcj: filter id out of range", 0);
		if (kd != 0) { bopt.bcj = kd; hs_coded = J->hs_bcj; }
	}
	uint64_t unp;
	uint8_t tail[48];
	uint32_t tl = 0;
	if (J->segments) {
		/* XZAMD_F_SEGMENTS: only the chunk chain -- no header, end marker, padding or Check; whether the segment is stored
		 * is decided exactly as for the Block the MT layout would make of it, so the chains are the same bytes */
		if (J->hs_fixed + payload + pad + cbytes > J->bound) {
			const uint64_t csz = usize + ((usize + 65535) / 65536) * 3;
			if (opos + csz > J->out_cap) return fail(c, XZAMD_BUF_ERROR, "output buffer too small", 0);
			uint8_t ctl = 0x01;
			for (uint64_t ip = 0; ip < usize; ip += 65536) {
				const uint64_t cs = usize - ip < 65536 ? usize - ip : 65536;
				uint8_t ch[3] = { ctl, (uint8_t)((cs - 1) >> 8), (uint8_t)(cs - 1) };
				ctl = 0x02;
				opos = plan_lit(pl, ch, 3, opos);
				opos = plan_seg(pl, 2, boff + ip, cs, opos);
			}
			++c->stats.blocks_stored;
			*stored_out = 1;
		} else {
			if (opos + payload - 1 > J->out_cap) return fail(c, XZAMD_BUF_ERROR, "output buffer too small", 0);
			for (uint32_t s = 0; s < nsp; ++s) {
				const uint64_t slot = b * opb + s, start = otab[2 * slot];
				if (two) {
					const uint32_t cb = XZAMD_CHUNK_BASE((uint32_t)start, (uint32_t)slot), cc = XZAMD_CHUNK_CAP(otab[2 * slot + 1] - (uint32_t)start);
					for (uint32_t k = 0; k < cc && hch[cb + k].usize != 0; ++k)
						opos = plan_seg(pl, 0, XZAMD_CHUNK_OUT(hch[cb + k].in_start, cb + k), hch[cb + k].csize, opos);
				} else
					opos = plan_seg(pl, 0, ((start + (start >> 3) + 15) & ~15ull) + slot * XZAMD_SPAN_SLACK, sb[slot], opos);
			}
		}
		const uint64_t gs = B->b0 + b;
		if (J->binfo && gs < J->binfo_cap) {
			J->binfo[gs].unpadded_size = check == XZAMD_CHECK_CRC64 ? bcrc[b] : check == XZAMD_CHECK_CRC32 ? (uint32_t)bcrc[b] : 0;
			J->binfo[gs].uncompressed_size = usize;
			J->binfo[gs].out_offset = bstart;
			J->binfo[gs].total_size = opos - bstart;
		}
		*opos_io = opos;
		return XZAMD_OK;
	}
	if (hs_coded + payload + pad + cbytes > J->bound) {
		/* stream_encoder_mt.c:298,316-344 -> block_buffer_encoder.c:88-162 */
		const uint64_t csz = usize + ((usize + 65535) / 65536) * 3 + 1;
		const uint32_t hs = xzamd_block_header_size_(csz, usize, NULL);      /* stored Blocks drop the filters in front of LZMA2 */
		if (opos + hs + csz + 3 + cbytes > J->out_cap) return fail(c, XZAMD_BUF_ERROR, "output buffer too small", 0);
		xzamd_block_header_put_(small, hs, csz, usize, 0x00, NULL);
		opos = plan_lit(pl, small, hs, opos);
		uint8_t ctl = 0x01;
		for (uint64_t ip = 0; ip < usize; ip += 65536) {
			const uint64_t cs = usize - ip < 65536 ? usize - ip : 65536;
			uint8_t ch[3] = { ctl, (uint8_t)((cs - 1) >> 8), (uint8_t)(cs - 1) };
			ctl = 0x02;
			opos = plan_lit(pl, ch, 3, opos);
			opos = plan_seg(pl, 2, boff + ip, cs, opos);
		}
		tail[tl++] = 0x00;
		while ((csz + (tl - 1)) & 3) tail[tl++] = 0;
		unp = hs + csz + cbytes;
		++c->stats.blocks_stored;
		*stored_out = 1;
	} else {
		if (opos + hs_coded + payload + pad + cbytes > J->out_cap) return fail(c, XZAMD_BUF_ERROR, "output buffer too small", 0);
		xzamd_block_header_put_(small, hs_coded, payload, usize, J->dbyte, &bopt);
		opos = plan_lit(pl, small, hs_coded, opos);
		for (uint32_t s = 0; s < nsp; ++s) {
			const uint64_t slot = b * opb + s, start = otab[2 * slot];
			if (two) {
				const uint32_t cb = XZAMD_CHUNK_BASE((uint32_t)start, (uint32_t)slot), cc = XZAMD_CHUNK_CAP(otab[2 * slot + 1] - (uint32_t)start);
				for (uint32_t k = 0; k < cc && hch[cb + k].usize != 0; ++k)
					opos = plan_seg(pl, 0, XZAMD_CHUNK_OUT(hch[cb + k].in_start, cb + k), hch[cb + k].csize, opos);
			} else
				opos = plan_seg(pl, 0, ((start + (start >> 3) + 15) & ~15ull) + slot * XZAMD_SPAN_SLACK, sb[slot], opos);
		}
		tail[tl++] = 0x00;
		for (uint64_t i = 0; i < pad; ++i) tail[tl++] = 0;
		unp = hs_coded + payload + cbytes;
	}
	if (check == XZAMD_CHECK_CRC64) {
		const uint64_t v = bcrc[b];
		xzamd_le32_(tail + tl, (uint32_t)v);
		xzamd_le32_(tail + tl + 4, (uint32_t)(v >> 32));
		tl += 8;
	} else if (check == XZAMD_CHECK_CRC32) {
		xzamd_le32_(tail + tl, (uint32_t)bcrc[b]);
		tl += 4;
	} else if (check == XZAMD_CHECK_SHA256) {
		memcpy(tail + tl, (const uint8_t *)c->h_block_crc.p + 32 * b, 32);
		tl += 32;
	}
	opos = plan_lit(pl, tail, tl, opos);
	const uint64_t gi = B->b0 + b;
	if (J->whole) { J->rec_unp[gi] = unp; J->rec_unc[gi] = usize; }
	if (J->binfo && gi < J->binfo_cap) {
		J->binfo[gi].unpadded_size = unp;
		J->binfo[gi].uncompressed_size = usize;
		J->binfo[gi].out_offset = bstart;
		J->binfo[gi].total_size = opos - bstart;
	}
	*opos_io = opos;
	return XZAMD_OK;
}

/* A finished batch in the figures of the call: stage times from the batch's events, Blocks and spans */
static void back_stats(xzamd_ctx *c, const job_env *J, const batch_run *B)
{
	const int par = B->par;
	const uint64_t nb = B->nb;
	const uint32_t *hcnt = (const uint32_t *)c->h_span_cnt[par].p;
	float ms;
	void **ev = c->evp[par];
	/* (a batch that was issued ahead has EV_START and EV_CHAINS on the side stream: its build shares the GPU with the parse of
	 * the batch before, so ms_chains grows with the knob while ms_total shrinks) */
	if (!xzk_event_elapsed_ms(ev[EV_START], ev[EV_CHAINS], &ms)) c->stats.ms_chains += ms;
	if (!xzk_event_elapsed_ms(ev[EV_CHAINS], ev[EV_FRONT], &ms)) c->stats.ms_encode += ms;
	if (J->opt->gpu_parser && !xzk_event_elapsed_ms(ev[EV_CHAINS], ev[EV_FIND], &ms)) c->stats.ms_find += ms;
	if (!xzk_event_elapsed_ms(ev[EV_PLAN0], ev[EV_PLAN1], &ms)) c->stats.ms_plan += ms;
	if (!xzk_event_elapsed_ms(ev[EV_CODE], ev[EV_CRC], &ms)) c->stats.ms_crc += ms;
	if (!xzk_event_elapsed_ms(ev[EV_CRC], ev[EV_ASM], &ms)) c->stats.ms_assemble += ms;
	c->stats.blocks += nb;
	for (uint64_t b = 0; b < nb; ++b) c->stats.spans += hcnt[b];
	if (J->m.two) {
		const uint32_t *ecnt = (const uint32_t *)c->h_enc_cnt[par].p;
		for (uint64_t b = 0; b < nb; ++b) c->stats.enc_spans += ecnt[b];
		if (J->seeds_early) { if (!xzk_event_elapsed_ms(c->ev_seed[par][1], c->ev_seed[par][2], &ms)) c->stats.ms_seed += ms; }
		else if (!xzk_event_elapsed_ms(ev[EV_PLAN1], ev[EV_SEED], &ms)) c->stats.ms_seed += ms;
		if (!xzk_event_elapsed_ms(ev[EV_SEED], ev[EV_PARSE], &ms)) c->stats.ms_parse += ms;
		if (!xzk_event_elapsed_ms(ev[EV_SEED], ev[EV_ITER1], &ms)) c->stats.ms_iter1 += ms;
		if (!xzk_event_elapsed_ms(ev[EV_BACK0], ev[EV_CODE], &ms)) { c->stats.ms_code += ms; c->stats.ms_encode += ms; }
	}
	if (J->m.adaptive) {
		uint64_t tgt;
		memcpy(&tgt, hcnt + 2 * ((nb + 1) / 2), 8);
		c->stats.span_cost_used = tgt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)tgt;
	}
	c->stats.batches += 1;
	c->stats.batches_ahead += B->ahead != 0;
	c->stats.encode_launches += 1;
}

/* Second half of a batch's back end: wait for the sizes, lay the Blocks out (the ordered output queue of the
 * reference, outqueue.c) and gather them into the Stream. */
static int back_finish(xzamd_ctx *c, job_env *J, batch_run *B)
{
	B->active = 0;
	int rc = back_report(c, J, B);
	if (rc != XZAMD_OK) return rc;

	plan pl;
	pl.lits = (uint8_t *)c->h_lits.p; pl.lits_len = 0; pl.lits_cap = B->max_lits;
	pl.segs = (xzamd_copy_seg *)c->h_segs.p; pl.nsegs = 0; pl.segs_cap = B->max_segs;
	uint64_t opos = J->opos;
	for (uint64_t b = 0; b < B->nb; ++b) {
		int stored = 0;
		rc = layout_block(c, J, B, &pl, b, &opos, &stored);
		if (rc != XZAMD_OK) return rc;
		if (J->resume) {
			/* the Block's records; one that went out stored has none of its span starts: its records are void */
			const uint32_t cnt = ((const uint32_t *)c->h_enc_cnt[B->par].p)[b];
			if (stored)
				for (uint32_t k = 0; k < cnt; ++k)
					if (xzk_memset((uint8_t *)c->resume_tab.p + (uint64_t)(J->rec_done + k) * XZAMD_RESUME_BYTES(J->m.model_slots)
							+ XZAMD_RESUME_KIND_OFF, (int)XZAMD_RK_VOID, 1, J->stb))
						return fail(c, XZAMD_DEVICE_ERROR, "memset resume record", 1);
			J->rec_done += cnt;
		}
	}
	J->opos = opos;
	if (pl.nsegs > pl.segs_cap || pl.lits_len > pl.lits_cap) return fail(c, XZAMD_PROG_ERROR, "plan overflow", 0);

	/* gather (the literal pieces and the segment table leave the pinned buffers before the call returns) */
	int e = xzk_h2d(c->segs.p, pl.segs, pl.nsegs * sizeof(xzamd_copy_seg), J->stb);
	if (!e) e = xzk_h2d(c->lits.p, pl.lits, pl.lits_len ? pl.lits_len : 1, J->stb);
	if (!e) e = xzk_assemble((const xzamd_copy_seg *)c->segs.p, (uint32_t)pl.nsegs,
			(const uint8_t *)c->scratch.p, (const uint8_t *)c->lits.p, J->d_in + B->in_off, J->d_out, J->stb);
	xzk_event_record(c->evp[B->par][EV_ASM], J->stb);
	if (!e) e = xzk_sync(J->stb);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "assemble", e);
	back_stats(c, J, B);
	return XZAMD_OK;
}

/* back_finish of a batch of the call that is running: its bytes count as done (prog_done is written by this thread only) */
static int back_finish_own(xzamd_ctx *c, job_env *J, batch_run *B)
{
	const uint64_t n64 = B->n64;
	int rc = back_finish(c, J, B);
	if (rc == XZAMD_OK) progress_set(c, c->prog_done + n64, 0, 0);
	return rc;
}

/* Finish the batch carried over from a deferred call and keep that call's result for xzamd_encode_finish_. */
static int pend_complete(xzamd_ctx *c)
{
	if (!c->pend.active)
		return XZAMD_OK;
	c->pend.active = 0;
	int rc = back_finish(c, &c->pend.J, &c->pend.B);
	if (rc != XZAMD_OK) xzk_sync(c->st2);
	c->pend_rc = rc;
	c->pend_out_size = c->pend.J.opos;
	c->pend_has_result = 1;
	return rc;
}

int xzamd_encode_finish_(xzamd_ctx *c, uint64_t *out_size)
{
	if (!c || !out_size)
		return XZAMD_PROG_ERROR;
	/* the oldest deferred call first: its result is already there when a later call has finished it underneath itself
	 * (and may have left a deferred batch of its own) */
	if (!c->pend_has_result && c->pend.active) {
		xzk_set_device(c->device);
		pend_complete(c);
	}
	if (!c->pend_has_result)
		return fail(c, XZAMD_PROG_ERROR, "no deferred call to finish", 0);
	c->pend_has_result = 0;
	*out_size = c->pend_out_size;
	return c->pend_rc;
}

/* ================= front end of a batch, on the caller's stream ================= */

/* 0. What LZMA2 reads: the input, or -- with filters in front of LZMA2 -- the filtered copy (the Check and stored Blocks
 * read the original).  Also the batch's start event and, where it can run underneath everything else, its SHA-256. */
static int front_input(xzamd_ctx *c, const job_env *J, batch_run *B, void *st)
{
	const uint8_t *in = J->d_in + B->in_off;
	const uint32_t n = B->n, bs = (uint32_t)J->block_size, nb = (uint32_t)B->nb;
	B->enc_in = in;
	xzk_event_record(c->evp[B->par][EV_START], st);
	if (J->check == XZAMD_CHECK_SHA256 && !J->pipelined) {
		/* SHA-256 is a serial hash per Block: on the second stream, underneath everything else of the batch */
		int e3 = xzk_stream_wait_event(c->st2, c->evp[B->par][EV_START]);
		if (!e3) e3 = xzk_sha256_blocks(in, n, bs, nb, (uint8_t *)c->block_crc.p, c->st2);
		if (!e3) e3 = xzk_event_record(c->ev_sha, c->st2);
		if (e3) return fail(c, XZAMD_DEVICE_ERROR, "sha256 launch", e3);
		B->sha_early = 1;
	}
	if (J->filtered) {
		/* the filters run one after another, each over the whole batch (they do not alias: in -> X for one,
		 * in -> T -> X for two, in -> X -> T -> X for three; T is only live inside this sequence) */
		uint32_t pre[XZAMD_PREFILTERS_MAX];
		const uint32_t npre = xzamd_prefilter_list_(J->opt, pre);
		uint8_t *const X = (uint8_t *)c->bcj[B->par].p, *const T = (uint8_t *)c->bcjt.p;
		const uint8_t *src = in;
		for (uint32_t i = 0; i < npre; ++i) {
			uint8_t *dst = ((npre - 1 - i) & 1) ? T : X;
			int e = pre[i] == XZAMD_BCJ_X86
					? xzk_x86_bcj(src, dst, n, bs, nb, st)
					: xzk_prefilter(src, dst, n, bs, nb, pre[i] & 0xFF, (pre[i] >> 8) + 1, st);
			if (e) return fail(c, XZAMD_DEVICE_ERROR, "filter in front of LZMA2", e);
			src = dst;
		}
		B->enc_in = X;
	}
	if (J->auto_delta || J->auto_bcj) {
		/* statistic, choice and filter stay on the device, in stream order in front of the structure build; the choices
		 * travel to the host behind them and are there when the layout (which waits for this stream's tables) reads them.
		 * With both analyses the BCJ choice clears the delta distance of the Blocks it takes before the delta stage copies
		 * or filters every Block, and the BCJ stage then only patches its Blocks in that copy. */
		uint8_t *const X = (uint8_t *)c->bcj[B->par].p;
		uint32_t *const dist = J->auto_delta ? (uint32_t *)c->ddist[B->par].p : NULL;
		uint32_t *const kind = J->auto_bcj ? (uint32_t *)c->bkind[B->par].p : NULL;
		uint32_t *const bh = (uint32_t *)c->bhist.p;
		int e = 0;
		if (dist) e = xzk_delta_stats(in, n, bs, nb, (uint32_t *)c->dhist.p, st);
		if (!e && dist) e = xzk_delta_choose((const uint32_t *)c->dhist.p, nb, dist, st);
		if (!e && kind) e = xzk_bcj_stats(in, n, bs, nb, bh, bh + (uint64_t)XZAMD_AB_HIST_WORDS * nb, st);
		if (!e && kind) e = xzk_bcj_choose(bh, bh + (uint64_t)XZAMD_AB_HIST_WORDS * nb, n, bs, nb, kind, dist, st);
		if (!e && dist) e = xzk_delta_blocks(in, X, n, bs, nb, dist, st);
		if (!e && kind) e = xzk_bcj_blocks(in, X, n, bs, nb, kind, dist == NULL, st);
		if (!e && dist) e = xzk_d2h(c->h_ddist[B->par].p, dist, 4ull * nb, st);
		if (!e && kind) e = xzk_d2h(c->h_bkind[B->par].p, kind, 4ull * nb, st);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "automatic per-Block filter", e);
		B->enc_in = X;
	}
	if (J->auto_lclp) {
		/* the literal context of every Block, from the bytes LZMA2 will code -- behind the filter stage above -- and in stream
		 * order in front of the parse and the coder, which read the table through the span arguments; the host never
		 * needs it (the pair travels in the chunks' properties bytes, not in the Block Header) */
		int e = xzk_lclp_stats(B->enc_in, n, bs, nb, (uint32_t *)c->lhist.p, st);
		if (!e) e = xzk_lclp_choose((const uint32_t *)c->lhist.p, nb, J->opt->lc, J->opt->lp, (uint32_t *)c->dprops[B->par].p, st);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "automatic literal context", e);
	}
	return XZAMD_OK;
}

/* 1. Match-finder structure, on the stream `st` (the caller's, or the side stream of a build ahead). */
static int build_launch(xzamd_ctx *c, const job_env *J, const batch_run *B, void *st)
{
	const xzamd_lzma_options *opt = J->opt;
#define SA(buf) (opt->gpu_sa_window ? c->buf.p : NULL)     /* the suffix-neighbourhood finder's arrays */
	int e = xzk_build_chains(B->enc_in, B->n, (uint32_t)J->block_size, (uint32_t)B->nb, J->hb, J->hmask, J->hbits, opt->gpu_sa_depth,
			(uint32_t *)c->keys_a.p, (uint32_t *)c->keys_b.p, (uint32_t *)c->vals_a.p,
			(uint32_t *)c->vals_b.p, c->sort_tmp.p, B->sort_bytes,
			(uint32_t *)c->rank.p, (uint32_t *)c->sorted_pos.p, (uint32_t *)c->prev2.p, (uint32_t *)c->prev3.p,
			(uint32_t *)SA(prev4), (uint64_t *)SA(prev8), (uint64_t *)SA(prev16), (uint64_t *)SA(key64_a), (uint64_t *)SA(key64_b),
			(uint32_t *)SA(sa), (uint32_t *)SA(sa_rank), (uint32_t *)SA(prev24), (uint32_t *)SA(prev32), st);
#undef SA
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "build_chains", e);
	xzk_event_record(c->evp[B->par][EV_CHAINS], st);
	return XZAMD_OK;
}

/* The structure of the batch is built -- here, or ahead of time on the side stream, in which case the caller's stream only
 * waits for it.  The back end of the previous batch, when it has been left to this batch, starts behind it. */
static int front_build(xzamd_ctx *c, const job_env *J, const batch_run *B, back_args *prev_back)
{
	void **ev = c->evp[B->par];
	int e = 0;
	if (B->ahead) {
		e = xzk_stream_wait_event(J->st, ev[EV_CHAINS]);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "stream wait", e);
	} else {
		int rc = build_launch(c, J, B, J->st);
		if (rc != XZAMD_OK) return rc;
	}
	if (!prev_back->valid)
		return XZAMD_OK;
	e = J->stb != J->st ? xzk_stream_wait_event(J->stb, ev[EV_CHAINS]) : 0;
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "stream wait", e);
	return back_enqueue(c, J, prev_back);
}

/* Build ahead: once the front end of `cur` is enqueued and the batch before it is finished, the filters and
 * the structure build of the batch behind `cur` go on the side stream, behind the start event of `cur` the call has chosen:
 * they fill the snapshot walks and then run beneath the FULL parse.  Everything they write is dead by then -- the structure
 * and the sorts' scratch since the finder and the plan's sort of `cur`, the filtered copy and the delta choices of this
 * parity since the back end of the batch before `cur`, which the host has waited for (audit: DESIGN.md section 2).  Only into
 * buffers that are there: a batch that would grow one is left to the loop, which runs it serially (next->ahead stays 0).
 * The host waits inside the build for the side stream alone (the count of every doubling round). */
static int ahead_issue(xzamd_ctx *c, const job_env *J, const batch_run *cur, batch_run *next)
{
	memset(next, 0, sizeof(*next));
	const uint64_t b0 = cur->b0 + cur->nb;
	if (!J->ahead || b0 >= J->total_blocks)
		return XZAMD_OK;
	batch_run N;
	int rc = batch_geometry(c, J, b0, &N);
	if (rc != XZAMD_OK) return rc;
	N.par = (int)(c->par_seq & 1);
	if (batch_reserve(c, J, &N, 1))
		return XZAMD_OK;
	void **evc = c->evp[cur->par];
	int e = xzk_stream_wait_event(J->sta, evc[J->ahead == AHEAD_PLAN ? EV_PLAN1 : J->ahead == AHEAD_PART ? EV_PART : EV_ITER1]);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "stream wait", e);
	++c->par_seq;
	N.ahead = 1;
	*next = N;                       /* (from here on the side stream holds work of this batch: error paths drain it) */
	rc = front_input(c, J, next, J->sta);
	if (rc == XZAMD_OK) rc = build_launch(c, J, next, J->sta);
	return rc;
}

/* the batch match finder: part 0 = every position, 1 = the seed regions, 2 = the rest */
static int find_part(xzamd_ctx *c, const job_env *J, const xzamd_span_args *a, int part)
{
	return xzk_find_matches(a, (const uint32_t *)c->sa.p, (const uint32_t *)c->sa_rank.p, (const uint32_t *)c->prev4.p,
			(const uint64_t *)c->prev8.p, (const uint64_t *)c->prev16.p,
			(const uint32_t *)c->prev24.p, (const uint32_t *)c->prev32.p, (uint16_t *)a->mlen, (uint32_t *)a->mdist, part, J->st);
}

/* 2a. Batch match finder -> the lists the parser streams.  With seeds_early the lists of the seed regions come first
 * and the seed pieces are parsed on the third stream underneath the rest of the finder. */
static int front_find(xzamd_ctx *c, const job_env *J, const batch_run *B, const xzamd_span_args *a)
{
	const int par = B->par;
	if (xzk_memset(c->errw.p, 0, 512, J->st)) return fail(c, XZAMD_DEVICE_ERROR, "memset", 1);
	if (J->opt->gpu_parser) {
		int e = 0;
		if (J->seeds_early) {
			e = find_part(c, J, a, 1);
			if (!e) e = xzk_event_record(c->ev_seed[par][0], J->st);
			if (!e) e = xzk_stream_wait_event(c->st3, c->ev_seed[par][0]);
			if (!e) e = xzk_event_record(c->ev_seed[par][1], c->st3);
			if (!e) e = xzk_parse_pieces(a, (uint32_t)B->nb, 0, 0, NULL, c->st3);
			if (!e) e = xzk_event_record(c->ev_seed[par][2], c->st3);
		}
		if (!e) e = find_part(c, J, a, J->seeds_early ? 2 : 0);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "find_matches launch", e);
	}
	xzk_event_record(c->evp[par][EV_FIND], J->st);
	return XZAMD_OK;
}

/* 2b. Span plan: cut on the device from the match lists and fetched for the layout, or a table of equal spans
 * written here. */
static int front_plan(xzamd_ctx *c, const job_env *J, const batch_run *B, xzamd_span_args *a)
{
	const xzamd_lzma_options *opt = J->opt;
	const int par = B->par, two = J->m.two;
	const uint64_t nb = B->nb, block_size = J->block_size;
	void *st = J->st;
	void **ev = c->evp[par];
	uint32_t *const htab = (uint32_t *)c->h_span_tab.p, *const hcnt = (uint32_t *)c->h_span_cnt[par].p;
	int e;
	xzk_event_record(ev[EV_PLAN0], st);
	if (J->m.adaptive) {
		uint32_t *launch_order = NULL;
		{
			int occ = 0;
			c->stats.wave_slots = (xzk_span_occupancy(1, opt->gpu_nice_len, &occ) || occ <= 0 || occ > 32)
					? c->wave_slots : c->cus * (uint32_t)occ;
		}
		e = xzk_span_plan(a, (uint32_t)nb, (uint32_t *)c->est.p, (unsigned long long *)c->totals.p,
				(uint32_t *)c->span_tab[par].p, (uint32_t *)c->span_cnt[par].p, opt->span_cost, opt->span_bits,
				XZAMD_SPAN_MIN_LEN, two ? (uint32_t *)c->enc_tab[par].p : NULL, two ? (uint32_t *)c->enc_cnt[par].p : NULL,
				(uint32_t *)c->order.p, c->sort_tmp.p, c->sort_tmp.cap, &launch_order, st);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "span plan launch", e);
		a->order = launch_order;
		/* the host lays the Blocks out from the plan: fetched with the span sizes */
		if (!two) e = xzk_d2h(htab, c->span_tab[par].p, 8ull * B->nspans, st);
		if (!e) e = xzk_d2h(hcnt, c->span_cnt[par].p, 4ull * nb, st);
		if (!e) e = xzk_d2h(hcnt + 2 * ((nb + 1) / 2), (uint8_t *)c->totals.p + 8ull * (nb + 1), 8, st);   /* target used, behind the counts */
		if (!e && two) e = xzk_d2h(c->h_enc_tab[par].p, c->enc_tab[par].p, 8ull * B->nenc, st);
		if (!e && two) e = xzk_d2h(c->h_enc_cnt[par].p, c->enc_cnt[par].p, 4ull * nb, st);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "d2h span plan", e);
	} else {
		const uint32_t span = J->span, spb = J->spb;
		for (uint64_t b = 0; b < nb; ++b) {
			const uint64_t bs = b * block_size, be = B->n64 - bs < block_size ? B->n64 : bs + block_size;
			uint32_t k = 0;
			for (uint64_t p = bs; p < be; p += span, ++k) {
				htab[2 * (b * spb + k)] = (uint32_t)p;
				htab[2 * (b * spb + k) + 1] = (uint32_t)(be - p < span ? be : p + span);
			}
			hcnt[b] = k;
		}
		e = xzk_h2d(c->span_tab[par].p, htab, 8ull * B->nspans, st);
		if (!e) e = xzk_h2d(c->span_cnt[par].p, hcnt, 4ull * nb, st);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "h2d span plan", e);
	}
	xzk_event_record(ev[EV_PLAN1], st);
	return XZAMD_OK;
}

/* 2c. Parse (two-phase: seed pieces, partial iterations, then every other piece in full) or the single-phase span
 * kernel; the front end's error words go to the host behind it. */
static int front_parse(xzamd_ctx *c, const job_env *J, const batch_run *B, xzamd_span_args *a)
{
	const int par = B->par;
	const uint32_t nb = (uint32_t)B->nb;
	void *st = J->st;
	void **ev = c->evp[par];
	uint32_t *const counter = (uint32_t *)c->errw.p + 60;
	int e;
	if (J->m.two) {
		if (J->seeds_early) e = xzk_stream_wait_event(st, c->ev_seed[par][2]);
		else e = xzk_parse_pieces(a, nb, 0, 0, NULL, st);
		xzk_event_record(ev[EV_SEED], st);
		/* partial iterations: the first part of every piece -- from the seed's prior, then from the snapshots -- and the
		 * carried model walk over its records, which leaves every piece the price model the next iteration starts from;
		 * then every piece in full (oracle: parse_block) */
		const uint32_t npart = J->opt->part_iters ? J->opt->part_iters : XZAMD_PART_ITERS_DEFAULT;
		for (uint32_t it = 0; it < npart && !e; ++it) {
			a->iter = XZAMD_ITER_PARTIAL | (it ? XZAMD_ITER_SNAP : 0u);
			if (it) e = xzk_memset(counter, 0, 4, st);
			if (!e) e = xzk_parse_pieces(a, nb, 1, c->span_waves, counter, st);
			if (J->ahead == AHEAD_PART && it + 1 == npart) xzk_event_record(ev[EV_PART], st);
			if (!e) e = xzk_model_snapshots(a, nb, st);
		}
		xzk_event_record(ev[EV_ITER1], st);
		a->iter = XZAMD_ITER_SNAP;
		if (!e) e = xzk_memset(counter, 0, 4, st);
		if (!e) e = xzk_parse_pieces(a, nb, 1, c->span_waves, counter, st);
		xzk_event_record(ev[EV_PARSE], st);
	} else {
		e = xzk_span_encode(a, B->nspans, c->span_waves, counter, st);
		/* single phase: the span kernel parses AND codes; its end is this batch's EV_PARSE for lzma_get_progress (a stage
		 * event that is not recorded for a batch would query as complete: the figure jumped to 90 % at the finder's end) */
		xzk_event_record(ev[EV_PARSE], st);
	}
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "span_encode launch", e);
	e = xzk_d2h(c->h_err[par].p, c->errw.p, 512, st);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "d2h", e);
	xzk_event_record(ev[EV_FRONT], st);
	return XZAMD_OK;
}

/* ================= back end ================= */

/* The previous batch's sizes, layout and gather -- its coder has had the whole front end of `cur` to finish -- then the
 * back end of `cur`: enqueued here, or left to the next batch's front_build (the default for a pipelined batch that has
 * another one behind it: the sorts of the build and the coder's walks slow each other down more than the finder and the
 * walks do; XZAMD_BACK_BESIDE_BUILD=1: always here, beside the next build). */
static int back_stage(xzamd_ctx *c, job_env *J, batch_run *cur, const xzamd_span_args *a, back_args *BA, batch_run *prev)
{
	int rc;
	if (J->pipelined && c->pend.active) {
		/* the last batch of the previous (deferred) call; a failure there is that call's (pend_rc, handed out by
		 * xzamd_encode_finish_), pend_complete has drained the second stream, this call goes on */
		(void)pend_complete(c);
	} else if (J->pipelined && prev->active) {
		rc = back_finish_own(c, J, prev);
		if (rc != XZAMD_OK) return rc;
	}
	BA->valid = 1;
	BA->a = *a;
	BA->B = *cur;
	if (!(!J->k.back_beside_build && J->pipelined && cur->b0 + cur->nb < J->total_blocks)) {
		rc = back_enqueue(c, J, BA);
		if (rc != XZAMD_OK) return rc;
	}
	progress_set(c, c->prog_done, cur->n64, cur->par);     /* every stage event of this batch has been recorded */
	if (J->pipelined) {
		*prev = *cur;
		return XZAMD_OK;
	}
	return back_finish_own(c, J, cur);
}

/* Out of device memory for a batch of which nothing has been launched yet.  The buffers grown so far have full-batch
 * capacity: a retry that kept them would fight for what is left.  An earlier batch may still be in its back end: finish
 * it, then release every per-batch device buffer and let the smaller geometry allocate afresh. */
static int batches_drain_release(xzamd_ctx *c, job_env *J, back_args *BA, batch_run *prev)
{
	int rc;
	c->err[0] = 0;
	if (c->pend.active)
		(void)pend_complete(c);          /* (its result is the deferred call's) */
	if (BA->valid) {                      /* (the earlier batch's back end has not been enqueued yet) */
		rc = back_enqueue(c, J, BA);
		if (rc != XZAMD_OK) return rc;
	}
	if (prev->active) {
		rc = back_finish_own(c, J, prev);
		if (rc != XZAMD_OK) return rc;
	}
	xzk_sync(J->st);
	xzk_sync(c->st2);
	xzk_sync(J->sta);                /* (a build ahead is never in flight here -- it is issued only into buffers that are there, and
	                                  * its batch then skips the reservation -- but the buffers go next: nothing may be running) */
	dbuf *d[CTX_NBUF_MAX];
	size_t nd = 0;
	ctx_device_bufs(c, d, &nd);
	for (size_t i = 0; i < CTX_NBIG && i < nd; ++i)
		if (d[i]->p) { xzk_free(d[i]->p); d[i]->p = NULL; d[i]->cap = 0; }
	return XZAMD_OK;
}

int xzamd_stream_encode_device(xzamd_ctx *c,
		const void *d_in_, uint64_t in_size, uint64_t block_size,
		const xzamd_lzma_options *opt, int check, uint32_t flags,
		void *d_out_, uint64_t out_cap, uint64_t *out_size,
		xzamd_block_info *binfo, uint64_t binfo_cap, uint64_t *nblocks_out,
		void *stream)
{
	if (c && (flags & XZAMD_F_CHAINS_))
		return fail(c, XZAMD_OPTIONS_ERROR, "unknown flag", 0);
	if (c && (flags & XZAMD_F_SINGLE) && (flags & XZAMD_F_AUTO_DELTA))
		return fail(c, XZAMD_OPTIONS_ERROR, "auto delta: Blocks only -- the single Block of XZAMD_F_SINGLE has one chain", 0);
	if (c && (flags & XZAMD_F_SINGLE) && (flags & XZAMD_F_AUTO_BCJ))
		return fail(c, XZAMD_OPTIONS_ERROR, "auto bcj: Blocks only -- the single Block of XZAMD_F_SINGLE has one chain", 0);
	if (c && (flags & XZAMD_F_SINGLE) && (flags & XZAMD_F_AUTO_LCLP))
		return fail(c, XZAMD_OPTIONS_ERROR, "auto lclp: Blocks only, not the single Block of XZAMD_F_SINGLE", 0);
	if (c && (flags & XZAMD_F_SINGLE)) {
		if (!xzamd_single_encode_)
			return fail(c, XZAMD_OPTIONS_ERROR, "single: this build has no unit for bare chunk chains", 0);
		return xzamd_single_encode_(c, d_in_, in_size, block_size, opt, check, flags & ~XZAMD_F_SINGLE, d_out_, out_cap, out_size, binfo,
				binfo_cap, nblocks_out, stream);
	}
	return xzamd_encode_device_(c, d_in_, in_size, block_size, opt, check, flags, d_out_, out_cap, out_size, binfo, binfo_cap,
			nblocks_out, stream, NULL);
}

/* The analysis of XZAMD_F_AUTO_DELTA on its own: statistic and choice of every Block, a device batch at a time */
int xzamd_auto_delta_device(xzamd_ctx *c, const void *d_in_, uint64_t in_size, uint64_t block_size, uint32_t *dist_out, uint64_t cap,
		uint64_t *nblocks_out, void *stream)
{
	if (!c || (!d_in_ && in_size) || !nblocks_out || (!dist_out && cap))
		return XZAMD_PROG_ERROR;
	c->err[0] = 0;
	if (!xzk_delta_stats || !xzk_delta_choose)
		return fail(c, XZAMD_OPTIONS_ERROR, "auto delta: this build has no kernels for it", 0);
	if (block_size == 0 || block_size >= (1ull << 31))
		return fail(c, XZAMD_OPTIONS_ERROR, "block_size must be 1 .. 2 GiB - 1", 0);
	const uint64_t total = (in_size + block_size - 1) / block_size;
	*nblocks_out = total;
	if (total > cap)
		return fail(c, XZAMD_BUF_ERROR, "dist_out too small", 0);
	if (c->pend.active)
		(void)pend_complete(c);      /* (its result is the deferred call's) */
	void *st = stream ? stream : c->own_stream;
	int e = xzk_set_device(c->device);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "hipSetDevice", e);
	uint64_t max_blocks = ((1ull << 31) - 1) / block_size;
	if (max_blocks > (1u << 20)) max_blocks = 1u << 20;      /* (11 KiB of histograms per Block) */
	c->last_par = 0;
	for (uint64_t b0 = 0; b0 < total; b0 += max_blocks) {
		const uint64_t nb = total - b0 < max_blocks ? total - b0 : max_blocks;
		const uint64_t off = b0 * block_size;
		const uint64_t n = in_size - off < nb * block_size ? in_size - off : nb * block_size;
		int r = dgrow(c, &c->dhist, 4ull * XZAMD_AD_HIST_WORDS * nb, 0);
		if (!r) r = dgrow(c, &c->ddist[0], 4 * nb, 0);
		if (r) return r;
		e = xzk_delta_stats((const uint8_t *)d_in_ + off, (uint32_t)n, (uint32_t)block_size, (uint32_t)nb, (uint32_t *)c->dhist.p, st);
		if (!e) e = xzk_delta_choose((const uint32_t *)c->dhist.p, (uint32_t)nb, (uint32_t *)c->ddist[0].p, st);
		if (!e) e = xzk_d2h(dist_out + b0, c->ddist[0].p, 4ull * nb, st);
		if (!e) e = xzk_sync(st);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "automatic delta analysis", e);
	}
	return XZAMD_OK;
}

/* The analysis of XZAMD_F_AUTO_BCJ on its own, in the same form */
int xzamd_auto_bcj_device(xzamd_ctx *c, const void *d_in_, uint64_t in_size, uint64_t block_size, uint32_t *kind_out, uint64_t cap,
		uint64_t *nblocks_out, void *stream)
{
	if (!c || (!d_in_ && in_size) || !nblocks_out || (!kind_out && cap))
		return XZAMD_PROG_ERROR;
	c->err[0] = 0;
	if (!xzk_bcj_stats || !xzk_bcj_choose)
		return fail(c, XZAMD_OPTIONS_ERROR, "auto bcj: this build has no kernels for it", 0);
	if (block_size == 0 || block_size >= (1ull << 31))
		return fail(c, XZAMD_OPTIONS_ERROR, "block_size must be 1 .. 2 GiB - 1", 0);
	const uint64_t total = (in_size + block_size - 1) / block_size;
	*nblocks_out = total;
	if (total > cap)
		return fail(c, XZAMD_BUF_ERROR, "kind_out too small", 0);
	if (c->pend.active)
		(void)pend_complete(c);      /* (its result is the deferred call's) */
	void *st = stream ? stream : c->own_stream;
	int e = xzk_set_device(c->device);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "hipSetDevice", e);
	uint64_t max_blocks = ((1ull << 31) - 1) / block_size;
	if (max_blocks > (1u << 14)) max_blocks = 1u << 14;      /* (64 KiB of histograms per Block) */
	c->last_par = 0;
	for (uint64_t b0 = 0; b0 < total; b0 += max_blocks) {
		const uint64_t nb = total - b0 < max_blocks ? total - b0 : max_blocks;
		const uint64_t off = b0 * block_size;
		const uint64_t n = in_size - off < nb * block_size ? in_size - off : nb * block_size;
		int r = dgrow(c, &c->bhist, 4ull * (XZAMD_AB_HIST_WORDS + XZAMD_AB_NCAND) * nb, 0);
		if (!r) r = dgrow(c, &c->bkind[0], 4 * nb, 0);
		if (r) return r;
		uint32_t *const bh = (uint32_t *)c->bhist.p;
		e = xzk_bcj_stats((const uint8_t *)d_in_ + off, (uint32_t)n, (uint32_t)block_size, (uint32_t)nb, bh, bh + XZAMD_AB_HIST_WORDS * nb, st);
		if (!e) e = xzk_bcj_choose(bh, bh + XZAMD_AB_HIST_WORDS * nb, (uint32_t)n, (uint32_t)block_size, (uint32_t)nb, (uint32_t *)c->bkind[0].p, NULL, st);
		if (!e) e = xzk_d2h(kind_out + b0, c->bkind[0].p, 4ull * nb, st);
		if (!e) e = xzk_sync(st);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "automatic bcj analysis", e);
	}
	return XZAMD_OK;
}

/* The analysis of XZAMD_F_AUTO_LCLP on its own, in the same form: props_out[b] = lc | lp << 8 for a job with (lc, lp) */
int xzamd_auto_lclp_device(xzamd_ctx *c, const void *d_in_, uint64_t in_size, uint64_t block_size, uint32_t lc, uint32_t lp,
		uint32_t *props_out, uint64_t cap, uint64_t *nblocks_out, void *stream)
{
	if (!c || (!d_in_ && in_size) || !nblocks_out || (!props_out && cap))
		return XZAMD_PROG_ERROR;
	c->err[0] = 0;
	if (!xzk_lclp_stats || !xzk_lclp_choose)
		return fail(c, XZAMD_OPTIONS_ERROR, "auto lclp: this build has no kernels for it", 0);
	if (block_size == 0 || block_size >= (1ull << 31))
		return fail(c, XZAMD_OPTIONS_ERROR, "block_size must be 1 .. 2 GiB - 1", 0);
	if (lc > 4 || lp > 4 || lc + lp > 4)
		return fail(c, XZAMD_OPTIONS_ERROR, "lc + lp must be at most 4", 0);
	const uint64_t total = (in_size + block_size - 1) / block_size;
	*nblocks_out = total;
	if (total > cap)
		return fail(c, XZAMD_BUF_ERROR, "props_out too small", 0);
	if (c->pend.active)
		(void)pend_complete(c);      /* (its result is the deferred call's) */
	void *st = stream ? stream : c->own_stream;
	int e = xzk_set_device(c->device);
	if (e) return fail(c, XZAMD_DEVICE_ERROR, "hipSetDevice", e);
	uint64_t max_blocks = ((1ull << 31) - 1) / block_size;
	if (max_blocks > (1u << 12)) max_blocks = 1u << 12;      /* (64 KiB of histograms per Block) */
	c->last_par = 0;
	for (uint64_t b0 = 0; b0 < total; b0 += max_blocks) {
		const uint64_t nb = total - b0 < max_blocks ? total - b0 : max_blocks;
		const uint64_t off = b0 * block_size;
		const uint64_t n = in_size - off < nb * block_size ? in_size - off : nb * block_size;
		int r = dgrow(c, &c->lhist, 4ull * XZAMD_LL_HIST_WORDS * nb, 0);
		if (!r) r = dgrow(c, &c->dprops[0], 4 * nb, 0);
		if (r) return r;
		e = xzk_lclp_stats((const uint8_t *)d_in_ + off, (uint32_t)n, (uint32_t)block_size, (uint32_t)nb, (uint32_t *)c->lhist.p, st);
		if (!e) e = xzk_lclp_choose((const uint32_t *)c->lhist.p, (uint32_t)nb, lc, lp, (uint32_t *)c->dprops[0].p, st);
		if (!e) e = xzk_d2h(props_out + b0, c->dprops[0].p, 4ull * nb, st);
		if (!e) e = xzk_sync(st);
		if (e) return fail(c, XZAMD_DEVICE_ERROR, "automatic literal context analysis", e);
	}
	return XZAMD_OK;
}

/* xzamd_stream_encode_device, and -- with deferred != NULL, XZAMD_F_BLOCKS_ONLY and the two-phase encode -- its pipelined
 * form for callers that run one call after another on the same context (the workers of the lzma_* front end): the call
 * returns when the back end of its LAST batch has been launched (*deferred = 1; *out_size is not set), and that batch is
 * finished by the next call underneath the front end of its own first batch -- the overlap the batches of ONE call have
 * always had -- or by xzamd_encode_finish_, which also hands out the call's out_size and result.  The
 * input, output and binfo buffers of a deferred call stay in use until then. */
int xzamd_encode_device_(xzamd_ctx *c,
		const void *d_in_, uint64_t in_size, uint64_t block_size,
		const xzamd_lzma_options *opt, int check, uint32_t flags,
		void *d_out_, uint64_t out_cap, uint64_t *out_size,
		xzamd_block_info *binfo, uint64_t binfo_cap, uint64_t *nblocks_out,
		void *stream, int *deferred)
{
	if (deferred) *deferred = 0;
	if (!c || !opt || !out_size || (!d_in_ && in_size) || !d_out_)
		return XZAMD_PROG_ERROR;
	job_env J;
	memset(&J, 0, sizeof(J));
	int rc = call_setup(c, &J, (const uint8_t *)d_in_, in_size, block_size, opt, check, flags, (uint8_t *)d_out_, out_cap,
			binfo, binfo_cap, stream, deferred != NULL);
	if (rc != XZAMD_OK)
		return rc;
	if (nblocks_out) *nblocks_out = J.total_blocks;
	if (J.whole) {
		rc = stream_begin(c, &J);
		if (rc != XZAMD_OK)
			return rc;
	}

	batch_run prev;                  /* pipelined: the batch whose back end runs underneath the current front end */
	memset(&prev, 0, sizeof(prev));
	back_args BA;                    /* valid: the back end of `prev` has not been enqueued yet */
	memset(&BA, 0, sizeof(BA));
	batch_run next;                  /* ahead: the batch behind the current one, its build already on the side stream */
	memset(&next, 0, sizeof(next));
	progress_set(c, 0, 0, 0);
	xzk_event_record(c->ev_total[0], J.st);
	for (uint64_t b0 = 0; b0 < J.total_blocks && rc == XZAMD_OK; ) {
		batch_run cur;
		xzamd_span_args a;
		if (next.ahead) {
			/* its geometry, buffers, filters and build were dealt with under the batch before */
			cur = next;
			next.ahead = 0;
		} else {
			rc = batch_geometry(c, &J, b0, &cur);
			if (rc != XZAMD_OK) break;
			cur.par = J.pipelined ? (int)(c->par_seq++ & 1) : 0;
			rc = batch_reserve(c, &J, &cur, 0);
			if (rc == XZAMD_MEM_ERROR && cur.nb > 1) {
				/* out of device memory: this batch again with half the Blocks */
				J.max_blocks = (cur.nb + 1) / 2;
				rc = batches_drain_release(c, &J, &BA, &prev);
				continue;
			}
			if (rc != XZAMD_OK) break;
		}
		cur.active = 1;
		c->last_par = cur.par;

		if (!cur.ahead) rc = front_input(c, &J, &cur, J.st);
		if (rc == XZAMD_OK) rc = front_build(c, &J, &cur, &BA);
		if (rc == XZAMD_OK) {
			span_args_init(c, &J, &cur, &a);
			rc = front_find(c, &J, &cur, &a);
		}
		if (rc == XZAMD_OK) rc = front_plan(c, &J, &cur, &a);
		if (rc == XZAMD_OK) rc = front_parse(c, &J, &cur, &a);
		if (rc == XZAMD_OK) rc = back_stage(c, &J, &cur, &a, &BA, &prev);
		/* Order on the host: the batch before `cur` has just been finished (back_stage: layout and gather, no later than
		 * without the build ahead), and the finder of `cur` is still running, so the build of the next batch is enqueued
		 * before its start event fires.  The host then waits inside that build, where the serial order waited too. */
		if (rc == XZAMD_OK) rc = ahead_issue(c, &J, &cur, &next);
		b0 += cur.nb;
	}
	if (rc == XZAMD_OK && c->pend.active)
		(void)pend_complete(c);      /* (a call without a batch of its own) */
	if (rc == XZAMD_OK && prev.active) {
		if (J.defer) {
			/* the back end of the last batch is in flight on the second stream: whoever comes next finishes it */
			c->pend.J = J;
			c->pend.B = prev;
			c->pend.active = 1;
			prev.active = 0;
			*deferred = 1;
		} else {
			rc = back_finish_own(c, &J, &prev);
		}
	}
	if (rc != XZAMD_OK && c->pend.active)
		pend_complete(c);            /* this call failed before it got there: the carried batch still gets finished */
	xzk_sync(J.st);
	xzk_sync(c->st3);
	if (J.sta != c->st3) xzk_sync(J.sta);     /* (either one: also a build ahead that an error left behind) */
	if (!(deferred && *deferred))
		xzk_sync(c->st2);          /* a back end abandoned by an error path */
	if (rc == XZAMD_OK && J.whole)
		rc = stream_end(c, &J);
	xzk_event_record(c->ev_total[1], J.st);
	xzk_sync(J.st);
	{
		float ms;
		if (!xzk_event_elapsed_ms(c->ev_total[0], c->ev_total[1], &ms)) c->stats.ms_total = ms;
	}
	free(J.rec_unp);
	c->stats.in_bytes = in_size;
	c->stats.out_bytes = J.opos;
	*out_size = (deferred && *deferred) ? 0 : J.opos;
	if (rc == XZAMD_OK && J.resume) {
		c->resume.valid = 1;
		c->resume.stride = XZAMD_RESUME_BYTES(J.m.model_slots); c->resume.nrec = J.rec_done;
		c->resume.nblocks = J.total_blocks; c->resume.block_size = J.block_size; c->resume.in_size = in_size;
	}
	if (rc == XZAMD_OK && J.segments && J.verify) {
		/* the segments of a single-Block Stream: verdicts on their chains, and with XZAMD_F_REPAIR the rejected ones replaced */
		uint64_t ns = J.opos;
		rc = xzamd_chains_encoded_(c, J.d_out, J.opos, J.out_cap, J.d_in, in_size, J.opt, J.check, J.repair, J.binfo, J.total_blocks,
				&ns, J.st);
		if (rc == XZAMD_OK) {
			*out_size = ns;
			c->stats.out_bytes = ns;
		}
		c->stats.ms_verify = c->report.ms_verify;
	} else if (rc == XZAMD_OK && J.repair) {
		/* verified and repaired encode: per-Block verdicts; the Blocks the device decoder rejects are re-encoded and spliced */
		uint64_t ns = J.opos;
		rc = xzamd_repair_encoded_(c, J.d_out, J.opos, J.out_cap, J.d_in, in_size, J.block_size, J.opt, J.check, J.whole, J.binfo,
				J.binfo_cap, J.total_blocks, &ns, J.st);
		if (rc == XZAMD_OK) {
			*out_size = ns;
			c->stats.out_bytes = ns;
		}
		c->stats.ms_verify = c->report.ms_verify;
	} else if (rc == XZAMD_OK && J.verify) {
		/* verified encode: the finished Stream against the input, before the caller sees XZAMD_OK (its message and report stay) */
		rc = xzamd_verify_kept_(c, J.d_out, J.opos, J.d_in, in_size, J.st);
		c->stats.ms_verify = c->report.ms_verify;
	}
	return rc;
}
