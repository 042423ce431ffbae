/* xzamd_internal.h -- shared by the plain-C host translation units only (not part of any ABI). */
#ifndef XZAMD_INTERNAL_H
#define XZAMD_INTERNAL_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/xz_amd.h"
#include "../../include/xz_amd_lzma.h"
#include "kernels_api.h"

uint32_t xzamd_crc32_host_(const uint8_t *p, size_t n);
void *xzamd_ctx_stream_(xzamd_ctx *c);
uint32_t xzamd_ctx_wave_slots_(const xzamd_ctx *c);
int xzamd_ctx_fail_(xzamd_ctx *c, int code, const char *what);
uint64_t xzamd_ctx_progress_in_(xzamd_ctx *c);
void xzamd_ctx_progress_reset_(xzamd_ctx *c);
int xzamd_encode_device_(xzamd_ctx *c, const void *d_in, uint64_t in_size, uint64_t block_size,
		const xzamd_lzma_options *opt, int check, uint32_t flags, void *d_out, uint64_t out_cap, uint64_t *out_size,
		xzamd_block_info *binfo, uint64_t binfo_cap, uint64_t *nblocks_out, void *stream, int *deferred);
int xzamd_encode_finish_(xzamd_ctx *c, uint64_t *out_size);
int xzamd_stored_blocks_host_(const uint8_t *in, uint64_t n, uint64_t block_size, int check,
		uint8_t *out, uint64_t out_cap, uint64_t *out_size, xzamd_block_info *binfo, uint64_t binfo_cap, uint64_t *nblocks);

/* test instrumentation of the device decoder: temporaries allocated for inverse filters, inverse-stage calls, forward-filter
 * launches of verification decodes (process-wide counts) */
void xzamd_debug_decode_counters_(uint64_t out[3]);
/* ... of the last decode launch of the process: units, Blocks, split mode of the scan (0 Block, 1 verification, 2 plain) */
void xzamd_debug_decode_units_(uint64_t out[3]);

/* The device part of a decode (xzamd_decode.c), shared by the single-Stream entries and the file entries (xzamd_file.c). */
typedef struct {
	uint64_t first, count;          /* Blocks [first, first + count) of the job ... */
	int check;                      /* ... carry this Check (the Blocks of one Stream) */
} xzamd_dec_group;
typedef struct {
	const uint8_t *d_xz;
	uint8_t *d_out;                 /* Block b is written at d_out + hb[b].upos */
	const uint8_t *d_expected;      /* the original of all of d_out, or NULL */
	uint64_t nb;
	xzamd_dec_block *hb;            /* parsed Blocks (xzb_block); nunits / error are scratch */
	const xzamd_dec_chain *hc;
	const uint8_t *stored;          /* XZAMD_HDR_CHECK_BYTES per Block: the stored Check */
	const xzamd_dec_group *groups;  /* in Block order, every Block in exactly one group */
	uint32_t ngroups;
	int allow_split;                /* with d_expected: span-parallel units (else unit = Block; compared either way).  Without
	                                 * d_expected the units always start at the dictionary resets */
	uint64_t *mismatches;           /* optional */
	uint64_t *counts;               /* optional: [0] += device-to-host reads, [1] += kernel-launch calls */
	/* verification decode with a resume table (xzamd_stream_verify_device): units at the records instead of at the state resets
	 * that carry properties -- under the geometry rule of allow_split; else the table is ignored */
	const uint8_t *d_rec;           /* optional: nrec records of rec_stride bytes (kernels_api.h) */
	uint32_t rec_stride, nrec;
	xzamd_verify_report *report;    /* optional: units, Blocks, records, the first defect */
	/* COLLECT mode (the per-Block verification, xzamd_verify_table_): one XZAMD_VSTEP_* per Block, in and out.  A Block that
	 * fails a step is marked with it and taken out of the later steps, the run goes on for the others, and the call returns
	 * XZAMD_DATA_ERROR at the end when any Block is marked.  A Block marked on entry (its header was bad) is left out from the
	 * start.  The report names what a run without `steps` would have stopped at. */
	uint8_t *steps;                 /* optional: nb bytes */
	int plain_history;              /* with d_expected: it is only compared with; the units are those of a decode without it (dictionary
	                                 * resets, history = the output itself) */
	int chains;                     /* hb names bare chunk chains (xzamd_chains.c): the scan is xzk_dec_scan_chains, every other stage as it is */
} xzamd_dec_job;

/* The resume table a context keeps of its last encode with XZAMD_F_KEEP_RESUME / XZAMD_F_VERIFY (xzamd_host.c) */
typedef struct {
	uint8_t *d_rec;                 /* NULL: none kept */
	uint32_t stride, nrec;
	uint64_t nblocks, block_size, in_size;   /* the Stream it belongs to: Blocks of block_size bytes but the last */
} xzamd_resume_view;
void xzamd_ctx_resume_(xzamd_ctx *c, xzamd_resume_view *v);
xzamd_verify_report *xzamd_ctx_report_(xzamd_ctx *c);
/* xzamd_stream_verify_device with the context's kept table, on behalf of an encode with XZAMD_F_VERIFY (xzamd_decode.c; the
 * batch encoder refers to it weakly: a build of the host layer without the decoder has no verified encode) */
int xzamd_verify_kept_(xzamd_ctx *c, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size, void *stream);
/* test hook: overwrite a field of record `record` of the kept table -- 0: upos = value, 1: kind = value, 2: state = value,
 * 3: the whole model = 1024s */
int xzamd_debug_resume_poke_(xzamd_ctx *c, uint32_t record, int field, uint32_t value);
/* test hook: the 8 header words of a record of the kept table (hdr_out may be NULL), and how many records it has */
int xzamd_debug_resume_peek_(xzamd_ctx *c, uint32_t record, uint32_t hdr_out[8], uint32_t *nrec_out);
int xzamd_dec_run_(xzamd_ctx *c, void *st, const xzamd_dec_job *j);
const char *xzamd_block_step_msg_(uint32_t step);

/* ---- per-Block verification and repair (xzamd_framing.c, xzamd_decode.c, xzamd_repair.c, xzamd_repair_plan.c; DESIGN.md 3.6 "Repair") ---- */
/* Header, Footer and Index of the single Stream at d_xz -> one record per Block (malloc'ed, the caller frees) and the Check.
 * A defect here is a defect of the whole Stream: the code of xzamd_stream_decode_device. */
int xzamd_stream_table_(xzamd_ctx *c, const uint8_t *d_xz, uint64_t xz_size, xzamd_hdr_rec **recs, uint64_t *nb, int *check,
		void *stream);
/* The collecting verification of the Blocks `recs` name inside d_xz (a Stream, or bare Blocks): Block Headers (k_dec_headers),
 * unit scan, decode, inverse filters, Checks and -- with d_original, whose byte recs[b].upos is the Block's first -- the
 * per-Block comparison.  steps[b] = XZAMD_VSTEP_* of the first step Block b failed.  XZAMD_VT_KEPT: the units of the context's
 * resume table when it fits.  XZAMD_VT_PRECISE: a Block that fails at "decode" or "check" with the original as history goes
 * through once more with its own output as history, so that the step names a defect of the Stream and not one of the original
 * (a Block-sequential decode; the repair, which re-encodes a bad Block whatever its step, does without).
 * XZAMD_OK: every Block good; XZAMD_DATA_ERROR: some Block bad; else a failure of the call. */
#define XZAMD_VT_KEPT 1
#define XZAMD_VT_PRECISE 2
int xzamd_verify_table_(xzamd_ctx *c, const uint8_t *d_xz, uint64_t xz_size, const xzamd_hdr_rec *recs, uint64_t nb, int check,
		const uint8_t *d_original, uint64_t original_size, int mode, uint8_t *steps, xzamd_verify_report *report, void *stream);
/* The collecting run of a prepared job (job->steps set, utotal = the sum of its uncompressed sizes) as xzamd_verify_table_ makes
 * it: the kept table when it fits (XZAMD_VT_KEPT), the second look at "decode" / "check" verdicts (XZAMD_VT_PRECISE) */
int xzamd_verify_job_(xzamd_ctx *c, void *st, xzamd_dec_job *job, uint64_t utotal, int mode, xzamd_verify_report *rp);
/* What an encode on the context would overwrite while a repair re-encodes Blocks on it: the kept resume table (taken out of
 * the context, so that the re-encode neither frees nor replaces it) and the stats of the call being repaired */
typedef struct {
	void *tab; uint64_t tab_cap;
	int valid; uint32_t stride, nrec; uint64_t nblocks, block_size, in_size;
	xzamd_stats stats;
} xzamd_ctx_saved;
void xzamd_ctx_save_(xzamd_ctx *c, xzamd_ctx_saved *s);
void xzamd_ctx_restore_(xzamd_ctx *c, const xzamd_ctx_saved *s);
xzamd_repair_report *xzamd_ctx_repair_report_(xzamd_ctx *c);
/* XZAMD_F_REPAIR on behalf of the batch encoder, which refers to it weakly (xzamd_repair.c): per-Block verification of the
 * Stream (framed) or the bare Blocks (their table: binfo) just written to d_out, repair of the rejected ones.  binfo (optional
 * when framed) is rewritten for the Blocks that moved. */
int xzamd_repair_encoded_(xzamd_ctx *c, void *d_out, uint64_t size, uint64_t cap, const void *d_in, uint64_t in_size,
		uint64_t block_size, const xzamd_lzma_options *opt, int check, int framed, xzamd_block_info *binfo, uint64_t binfo_cap,
		uint64_t nblocks, uint64_t *new_size, void *stream);

/* The splice layout of a repair: pure arithmetic, no device call (xzamd_repair_plan.c). */
#define XZAMD_RP_KEEP 0u
#define XZAMD_RP_CODED 1u       /* replaced by a re-encoded Block that lies whole in the scratch buffer */
#define XZAMD_RP_STORED 2u      /* replaced by the stored form: uncompressed LZMA2 chunks of the original, filters dropped */
#define XZAMD_RP_SEG_MAX (1ull << 20)   /* a kept run moves in pieces of this size (the gather runs one workgroup per segment) */
typedef struct {
	uint64_t pos;           /* in: of the Block Header in the old Stream */
	uint64_t unpadded;      /* in: old Unpadded Size */
	uint64_t usize;         /* in */
	uint64_t uoff;          /* in: of the Block's first byte in the original */
	uint32_t repl;          /* in: XZAMD_RP_* */
	uint32_t pad_;
	uint64_t src;           /* in: CODED: scratch offset of the re-encoded Block; STORED: scratch offset of the Block's Check bytes */
	uint64_t new_unpadded;  /* CODED: in; KEEP, STORED: out */
	uint64_t new_pos;       /* out */
} xzamd_rp_block;
/* segment kinds of the plan: 0 scratch, 1 lits, 2 the old Stream, 3 the original; dst = offset from tail_pos */
typedef struct {
	uint64_t first;         /* first replaced Block (nb: none, nothing else is filled in) */
	uint64_t tail_pos;      /* the Stream is rewritten from here on: blocks[first].pos */
	uint64_t tail_len;      /* new bytes from tail_pos to the end */
	uint64_t new_size;      /* tail_pos + tail_len */
	xzamd_copy_seg *segs; uint64_t nsegs;
	uint8_t *lits; uint64_t lits_len;
	uint64_t frame_off, frame_len;   /* framed: Index + Stream Footer inside lits */
} xzamd_rp_plan;
/* blocks: nb Blocks in Stream order, adjacent (pos[b + 1] = pos[b] + Unpadded Size rounded up to four).  framed: Index and
 * Stream Footer follow the last Block.  Returns XZAMD_OK, XZAMD_MEM_ERROR or XZAMD_PROG_ERROR (a table that is not adjacent). */
int xzamd_repair_plan_(xzamd_rp_block *blocks, uint64_t nb, int check, int framed, xzamd_rp_plan *plan);
void xzamd_repair_plan_free_(xzamd_rp_plan *plan);

/* ---- bare chunk chains: the segments of a single-Block Stream (xzamd_chains.c; DESIGN.md 3.6 "Chains") ---- */
/* The splice layout of a chain repair (xzamd_repair_plan.c): chains lie back to back (pos[i + 1] = pos[i] + len[i]), every chain
 * behind the first replaced one moves, nothing else is written -- no header, padding, Check, Index or Footer.  CODED: the
 * re-encoded chain lies at scratch offset src, new_len bytes.  STORED: 0x01 + 64 KiB of the original, then 0x02 chunks, no end
 * marker; new_len is computed.  The plan's segment kinds and destinations are those of xzamd_repair_plan_. */
typedef struct {
	uint64_t pos;           /* in: of the chain's first byte */
	uint64_t len;           /* in: its old length */
	uint64_t usize;         /* in */
	uint64_t uoff;          /* in: of the segment's first byte in the original */
	uint32_t repl;          /* in: XZAMD_RP_* */
	uint32_t pad_;
	uint64_t src;           /* in, CODED */
	uint64_t new_len;       /* CODED: in; KEEP, STORED: out */
	uint64_t new_pos;       /* out */
} xzamd_cp_chain;
int xzamd_chains_plan_(xzamd_cp_chain *chains, uint64_t n, xzamd_rp_plan *plan);
/* The collecting verification of the chains binfo names inside d_chains (binfo as XZAMD_F_SEGMENTS fills it in): steps[i] =
 * XZAMD_VSTEP_* of segment i.  mode: XZAMD_VT_*.  XZAMD_OK / XZAMD_DATA_ERROR / a failure of the call. */
int xzamd_chains_verify_(xzamd_ctx *c, const uint8_t *d_chains, uint64_t size, const xzamd_block_info *binfo, uint64_t nseg,
		uint32_t dict_size, int check, const uint8_t *d_original, uint64_t original_size, int mode, uint8_t *steps,
		xzamd_verify_report *rp, void *st);
/* XZAMD_F_VERIFY / XZAMD_F_REPAIR on behalf of an XZAMD_F_SEGMENTS encode, which the batch encoder refers to weakly: verdicts
 * on the chains just written to d_out, and with `repair` the replacement of the rejected ones (binfo and *new_size rewritten) */
int xzamd_chains_encoded_(xzamd_ctx *c, void *d_out, uint64_t size, uint64_t cap, const void *d_in, uint64_t in_size,
		const xzamd_lzma_options *opt, int check, int repair, xzamd_block_info *binfo, uint64_t nseg, uint64_t *new_size, void *stream);
/* XZAMD_F_SINGLE on behalf of xzamd_stream_encode_device (weak reference): the framed single-Block Stream */
int xzamd_single_encode_(xzamd_ctx *c, const void *d_in, uint64_t in_size, uint64_t block_size, const xzamd_lzma_options *opt,
		int check, uint32_t flags, void *d_out, uint64_t out_cap, uint64_t *out_size, xzamd_block_info *binfo, uint64_t binfo_cap,
		uint64_t *nsegments, void *stream);
/* Internal flag of xzamd_encode_device_ (xzamd_stream_encode_device refuses it): with XZAMD_F_SEGMENTS, the flags
 * XZAMD_F_KEEP_RESUME / _VERIFY / _REPAIR are allowed and act on the chains (xzamd_chains_encoded_) */
#define XZAMD_F_CHAINS_ 0x80000000u
/* xzamd_repair.c: what the Block repair and the chain repair share */
void xzamd_repair_rung1_options_(const xzamd_lzma_options *opt, xzamd_lzma_options *o);
void xzamd_repair_knob_reject_(uint8_t *steps, uint64_t n);
int xzamd_repair_knob_rung2_(void);

double xzamd_work_bytes_per_byte_(const xzamd_lzma_options *opt);   /* device work buffers per input byte of a batch */
double xzamd_auto_delta_bytes_per_byte_(uint64_t block_size);       /* ... what XZAMD_F_AUTO_DELTA adds to them */
double xzamd_auto_bcj_bytes_per_byte_(uint64_t block_size, int with_auto_delta);      /* ... and XZAMD_F_AUTO_BCJ */
double xzamd_auto_lclp_bytes_per_byte_(uint64_t block_size);        /* ... and XZAMD_F_AUTO_LCLP */

/* Shared by the host units only.  The version script exports every xzamd_* name; these stay inside the library. */
#define XZAMD_HIDDEN __attribute__((visibility("hidden")))

/* xzamd_frame.c: the container pieces the batch encoder lays out itself */
XZAMD_HIDDEN void xzamd_le32_(uint8_t *p, uint32_t v);
XZAMD_HIDDEN uint32_t xzamd_check_bytes_(int check);               /* 0xFFFFFFFF: not a Check this library writes */
XZAMD_HIDDEN uint8_t xzamd_dict_size_byte_(uint32_t dict_size);
XZAMD_HIDDEN uint32_t xzamd_prefilter_list_(const xzamd_lzma_options *opt, uint32_t pre[XZAMD_PREFILTERS_MAX]);
XZAMD_HIDDEN int xzamd_prefilter_valid_(uint32_t pre);
XZAMD_HIDDEN uint32_t xzamd_block_header_size_(uint64_t csize, uint64_t usize, const xzamd_lzma_options *opt);
XZAMD_HIDDEN uint32_t xzamd_block_header_nosizes_(uint8_t out[12], uint8_t dict_byte);
XZAMD_HIDDEN void xzamd_block_header_put_(uint8_t *out, uint32_t hs, uint64_t csize, uint64_t usize, uint8_t dict_byte,
		const xzamd_lzma_options *opt);

/* xzamd_framing.c: container bytes -> the tables a decoder run consumes */
typedef struct {
	const uint8_t *host;    /* the container in host memory, or */
	const uint8_t *dev;     /* in device memory, read through st */
	void *st;
	uint64_t size;
	uint64_t reads;         /* device-to-host reads so far */
} xzamd_src;
XZAMD_HIDDEN int xzamd_src_read_(xzamd_src *s, uint64_t off, void *buf, uint64_t n);
/* Header, Footer and Index of the single Stream `s` -> one record per Block (malloc'ed, the caller frees) and the Check.
 * An Index record with an Uncompressed Size above usize_max is a data error.  Returns 0 or the code; *msg. */
XZAMD_HIDDEN int xzamd_stream_walk_(xzamd_src *s, uint64_t usize_max, xzamd_hdr_rec **recs, uint64_t *nb, int *check, const char **msg);
/* The framing of every Stream of a file (walked from its end, Stream Padding included): Streams and Index records */
typedef struct {
	xzamd_xz_stream *streams;   /* file order */
	uint64_t nstreams;
	xzamd_hdr_rec *recs;        /* one per Block of the file, file order; upos = offset in the decoded file */
	uint32_t *rec_stream;
	uint64_t nrecs;
	uint64_t usize;
} xzamd_walk;
XZAMD_HIDDEN int xzamd_file_walk_(xzamd_src *s, xzamd_walk *w, const char **msg);
XZAMD_HIDDEN void xzamd_walk_free_(xzamd_walk *w);
/* The Block table of n records: xzb_block per Block, on the host for a container in host memory, as k_dec_headers else.
 * err[b] is the verdict on Block b (code 0: good); hb / hc / stored of a bad Block are not to be used.  Returns 0, or the
 * code of a failure of the call itself (memory, device) with *msg. */
typedef struct {
	xzamd_dec_block *hb;
	xzamd_dec_chain *hc;
	uint8_t *stored;            /* XZAMD_HDR_CHECK_BYTES per Block */
	xzamd_hdr_err *err;
} xzamd_blocks;
XZAMD_HIDDEN int xzamd_block_table_(xzamd_src *s, const xzamd_hdr_rec *recs, uint64_t n, xzamd_blocks *B, uint64_t *launches,
		const char **msg);
/* the code of the first bad Block of the table in file order (0: none) and the text of its defect */
XZAMD_HIDDEN int xzamd_blocks_first_bad_(const xzamd_blocks *B, uint64_t n, const char **msg);
XZAMD_HIDDEN void xzamd_blocks_free_(xzamd_blocks *B);

/* the primitives of the framing reader: 0, or 1 = bad magic bytes, 2 = bad CRC32 (Stream Header, Stream Footer); Stream Flags
 * -> the Check, or XZAMD_OPTIONS_ERROR / XZAMD_UNSUPPORTED_CHECK with *msg; the size of a Check */
#define XZAMD_FR_MAGIC 1
#define XZAMD_FR_CRC 2
XZAMD_HIDDEN int xzamd_fr_header_(const uint8_t h[12]);
XZAMD_HIDDEN int xzamd_fr_footer_(const uint8_t f[12], uint64_t *index_size);
XZAMD_HIDDEN int xzamd_fr_flags_(const uint8_t f[2], int *check, const char **msg);
XZAMD_HIDDEN uint32_t xzamd_fr_check_size_(int check);

/* xzamd_forward.c: the forward framing reader (DESIGN.md 3.6 "Forward reading").  One resumable step over the bytes of a
 * file that are there so far: d_buf[0 .. size) continues the file at the first byte the steps before did not consume.
 * A step reads Stream Headers, walks Blocks (xzk_dec_walk), decodes the whole ones into d_out (Checks verified), checks Index
 * and Footer against the Blocks it met and passes Stream Padding, until the bytes or the room end.  It sets
 *   consumed    bytes of d_buf that are dealt with for good: the next step's buffer starts behind them
 *   produced    bytes written at d_out (the Blocks in front of a defect included, nothing behind it)
 *   stop        XZAMD_FWD_MORE: more input is needed (never with `final`); XZAMD_FWD_END; XZAMD_FWD_TRUNCATED (`final` only);
 *               XZAMD_FWD_OUT_FULL: the next Block does not fit behind `produced` (need: its size); XZAMD_FWD_DEFECT: code / step;
 *               XZAMD_FWD_PAUSE (with pause_at_header only): the next byte is the first of a further Stream Header
 * and returns XZAMD_OK unless the call itself failed (device, memory) or stop is XZAMD_FWD_DEFECT: then the defect's code. */
#define XZAMD_FWD_MORE 0u
#define XZAMD_FWD_PAUSE 5u
#define XZAMD_FWD_PHASE_HEADER 0u   /* xzamd_forward_state.phase: the next byte is the first of a Stream Header */
typedef struct {
	uint32_t phase;                 /* XZF_* (xzamd_forward.c) */
	uint32_t flags;                 /* XZAMD_FWD_CONCATENATED */
	int check;                      /* of the Stream being read */
	int first_stream;
	uint64_t *unp, *usz;            /* Unpadded Size and Uncompressed Size of the Stream's Blocks so far */
	uint64_t npairs, pairs_cap;
	uint64_t padding;               /* Stream Padding bytes passed so far */
	uint32_t walk_cap;              /* rows per walk launch (0: XZAMD_FWD_WALK_CAP) */
	uint32_t pause_at_header;       /* stop with XZAMD_FWD_PAUSE in front of every Stream Header but the first */
	/* totals over all steps */
	uint64_t offset;                /* file offset of the next step's d_buf[0] */
	uint64_t streams, blocks, blocks_delivered;
	/* of the last step */
	uint64_t consumed, produced, need;
	uint32_t stop, code, step;
	uint32_t pad2_;
	uint64_t reads, launches, walks; /* device-to-host reads, kernel-launch calls, of them walk launches: totals */
} xzamd_forward_state;
#define XZAMD_FWD_WALK_CAP 4096u
void xzamd_forward_init_(xzamd_forward_state *s, uint32_t flags);
void xzamd_forward_free_(xzamd_forward_state *s);
int xzamd_forward_step_(xzamd_ctx *c, xzamd_forward_state *s, const uint8_t *d_buf, uint64_t size, int final, uint8_t *d_out,
		uint64_t out_cap, void *stream);
/* test instrumentation of the last xzamd_file_decode_forward_device call: [0] device-to-host reads, [1] kernel-launch calls,
 * [2] Blocks delivered, [3] walk launches */
void xzamd_debug_forward_counters_(uint64_t out[4]);

/* How lzma_code / lzma_end / lzma_get_progress (xzamd_stream.c) reach a coder that lives in another unit: the coder's internal
 * struct starts with this, and `magic` tells it from the encoder's (XZAMD_MAGIC_DEC: the decoder of xzamd_decoder.c).  No call
 * into that unit, so a program without it links as before. */
#define XZAMD_MAGIC_DEC 0x585A414D44444543ull
typedef struct {
	uint64_t magic;
	lzma_ret (*code)(lzma_stream *strm, lzma_action action);
	void (*end)(lzma_stream *strm);
	void (*progress)(lzma_stream *strm, uint64_t *progress_in, uint64_t *progress_out);
} xzamd_coder_hooks;

/* xzamd_options.c: the encode mode of an option set */
typedef struct {
	int adaptive;            /* cost-balanced spans, cut on the device */
	int two;                 /* two-phase: parse pieces record symbols, encode spans code them */
	int list_packed;         /* match lists without the separate lengths */
	uint32_t model_slots;    /* probabilities of the model, padded */
	uint32_t span_default;   /* span size when the options name none */
} xzamd_mode;
XZAMD_HIDDEN xzamd_mode xzamd_mode_of_(const xzamd_lzma_options *opt);
#endif
