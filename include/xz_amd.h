/*
 * xz_amd.h -- public C ABI of the MI355X-native LZMA2 Block encoder (libxz_amd.so).
 *
 * Plain C: pointers and sizes only, no HIP or torch types in any signature.
 * `stream` arguments are a hipStream_t passed as void* (NULL = the library's
 * own stream).
 *
 * Two levels, both replacing reference interfaces (paths relative to the
 * XZ Utils 5.8.3 tree):
 *
 *  (1) Device-resident batch encode -- what every worker thread of the
 *      reference does for one Block, done here for all Blocks at once:
 *        worker_encode()            src/liblzma/common/stream_encoder_mt.c:219-361
 *        block_encode()             src/liblzma/common/block_encoder.c:47-135
 *        lzma2_encode()             src/liblzma/lzma/lzma2_encoder.c:135-259
 *        lzma_lzma_encode()         src/liblzma/lzma/lzma_encoder.c:313-436
 *        lzma_mf_hc3/hc4_find/skip  src/liblzma/lz/lz_encoder_mf.c:305-441
 *      -> xzamd_stream_encode_device()
 *
 *  (2) The liblzma streaming API itself (declared in xz_amd_lzma.h):
 *        lzma_stream_encoder_mt()   stream_encoder_mt.c:1196
 *        lzma_code()/lzma_end()     common/common.c:203,379
 *        lzma_get_progress()        common/common.c:406
 *        lzma_stream_encoder()      common/stream_encoder.c:341   (one Block per Stream, coded in segments:
 *        lzma_easy_encoder()        common/easy_encoder.c          XZAMD_F_SEGMENTS below)
 */
#ifndef XZ_AMD_H
#define XZ_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xzamd_ctx xzamd_ctx;

/* Return codes: the lzma_ret values of api/lzma/base.h:55-271 (same numbers). */
#define XZAMD_OK              0
#define XZAMD_STREAM_END      1
#define XZAMD_UNSUPPORTED_CHECK 3
#define XZAMD_MEM_ERROR       5
#define XZAMD_OPTIONS_ERROR   8
#define XZAMD_DATA_ERROR      9
#define XZAMD_BUF_ERROR      10
#define XZAMD_PROG_ERROR     11
/* HIP runtime / kernel failure (mapped to LZMA_PROG_ERROR at the lzma_* level). */
#define XZAMD_DEVICE_ERROR  100

#define XZAMD_CHECK_NONE   0
#define XZAMD_CHECK_CRC32  1
#define XZAMD_CHECK_CRC64  4
#define XZAMD_CHECK_SHA256 10

#define XZAMD_MF_HC3 0x03   /* lzma_match_finder values, api/lzma/lzma12.h:58-112 */
#define XZAMD_MF_HC4 0x04
#define XZAMD_MF_BT4 0x14

#define XZAMD_MODE_FAST   1 /* lzma_mode, api/lzma/lzma12.h:138-157 */
#define XZAMD_MODE_NORMAL 2

#define XZAMD_PRESET_EXTREME 0x80000000u

/* One span per Block: output is byte-identical to the reference MT encoder
 * for fast-mode HC3/HC4 chains (presets 0-3). */
#define XZAMD_SPAN_WHOLE_BLOCK 0xFFFFFFFFu
#define XZAMD_SPAN_DEFAULT 0u
/* Same as XZAMD_SPAN_DEFAULT (kept for callers of the round-2 interface: the span plan is derived from the
 * batch and the GPU's wave slots either way). */
#define XZAMD_SPAN_AUTO 1u

/* LZMA2 options: the encoder-relevant subset of lzma_options_lzma
 * (api/lzma/lzma12.h:216-525) plus the GPU span size. */
typedef struct {
	uint32_t dict_size;
	uint32_t lc, lp, pb;
	uint32_t mode;       /* as requested by the preset (informational) */
	uint32_t nice_len;
	uint32_t mf;         /* requested match finder */
	uint32_t depth;      /* 0 = reference default (lz_encoder.c:359-365) */
	/* --- what the device path actually runs --- */
	uint32_t gpu_mf;     /* XZAMD_MF_HC3 / XZAMD_MF_HC4 */
	uint32_t gpu_nice_len;
	uint32_t gpu_depth;  /* candidates taken from the main (3/4-byte hash) chain (exact finder only) */
	uint32_t span_size;  /* bytes per independently coded span; XZAMD_SPAN_*.  With the optimal parser (gpu_parser = 1) an EXPLICIT
	                        span size (also: XZAMD_SPAN_KIB in the environment) selects the single-phase kernel -- every span codes
	                        with its own model, 8 wavefronts per CU: a test and measurement mode, several times slower than the
	                        default (XZAMD_SPAN_DEFAULT / _AUTO: cost-balanced parse pieces + the two-phase encode) */
	uint32_t gpu_sa_window; /* 0 = exact HC3/HC4 semantics of the reference; else the suffix-neighbourhood
	                        finder (the BT4 successor): recency records among this many slots (<= 5) on
	                        either side of a position in 32-byte-prefix suffix order, plus the nearest
	                        equal hash2 / hash4 and equal 8 / 16 bytes; needs gpu_mf = HC4 and
	                        gpu_parser = 1 */
	uint32_t gpu_parser; /* 0 = lzma_lzma_optimum_fast semantics, 1 = windowed optimal parser (384-node DP over
	                        per-position match lists incl. the reference's compound edges; pb > 2 needs the two-phase
	                        mode, i.e. no explicit span size, else XZAMD_OPTIONS_ERROR) */
	uint32_t bcj;        /* 0 = chain {LZMA2}; XZAMD_BCJ_* / XZAMD_FILTER_DELTA(d) = that filter in front of LZMA2
	                        (the FIRST filter of the chain when bcj2 / bcj3 below name more) */
	uint32_t gpu_sa_depth; /* suffix-neighbourhood finder: prefix bytes the suffix order compares, 32 / 64 / 128 / 256
	                        (0 = 32); one rank-doubling round more per step.  Presets: 32 for nice_len <= 32, 64 up to
	                        nice_len 64, 256 above (what lz_encoder_mf.c:450-512 orders by is the whole suffix) */
	uint32_t span_cost;  /* != 0 with span_size XZAMD_SPAN_DEFAULT / _AUTO and the optimal parser: cost-balanced spans.
	                        The match lists give every 4 KiB an estimate of the parser's work (one unit per position it
	                        has to visit: positions under a match of nice_len bytes or more are skipped); a Block is cut
	                        into spans of equal estimated work of about span_cost units, each at least 64 KiB long (a batch that
	                        fills the GPU: 0.8 .. 2 x span_cost, chosen so that the rounds of the launch are full; the target
	                        used is reported in xzamd_stats.span_cost_used).  0: spans of span_size bytes */
	uint32_t span_bits;  /* with span_cost: a Block whose estimated coded size is `bits` (greedy parse over the match lists)
	                        gets at most bits / span_bits spans (no span longer than 1 MiB): a piece start costs output bytes
	                        whatever the data, so what bounds their number is the Block's OUTPUT (highly compressible Blocks:
	                        fewer, longer spans) */
	uint32_t enc_span_bits; /* != 0 with cost-balanced spans: TWO-PHASE encode.  The spans of the plan are
	                        parse PIECES: the optimal parser runs over each with an adaptive price model that codes nothing
	                        (the first 64 KiB of a Block are the seed piece, parsed from the flat model; what it leaves is
	                        the prior of the partial iteration; the full one starts every piece from a snapshot, part_iters) and
	                        records (length, distance) / literal symbols; the coder then walks them per ENCODE SPAN, in parallel,
	                        with ONE continuous model per Block (the model is carried from span to span exactly; a
	                        state reset only at the Block start, behind a stored piece, or where the carry falls back).
	                        A Block of estimated coded size `bits` gets max(1, min(size / 256 KiB, bits / enc_span_bits))
	                        encode spans, closed at piece ends.  0: single phase, every span of the plan resets the state */
	uint32_t bcj2, bcj3; /* second and third filter in front of LZMA2, same values as `bcj`, applied in that order (a chain
	                        holds at most 4 filters, LZMA2 last: common/filter_common.c:250-334); bcj3 needs bcj2 needs bcj */
	uint32_t part_iters; /* two-phase: PARTIAL parse iterations in front of the full one (0 = XZAMD_PART_ITERS_DEFAULT, at most 8).
	                        Each parses the first eighth (of its estimated work; >= 16 KiB) of every piece -- the first from the seed's prior, the others
	                        from the snapshots of the walk before -- and the carried model walk over its records leaves every
	                        piece the price model the next iteration starts from.  One costs about 15 % of the
	                        parse; more of them walk record tables out of the regime the Block's first 64 KiB suggest */
} xzamd_lzma_options;
#define XZAMD_PART_ITERS_DEFAULT 1u
#define XZAMD_PART_ITERS_MAX 8u
#define XZAMD_PREFILTERS_MAX 3u
#define XZAMD_SPAN_COST_DEFAULT 131072u   /* text: 128 KiB spans */
#define XZAMD_SPAN_BITS_DEFAULT 400000u
#ifndef XZAMD_ENC_SPAN_BITS_DEFAULT
#define XZAMD_ENC_SPAN_BITS_DEFAULT 800000u    /* about 100 KB of output per encode span (round 5: 1,600,000) */
#endif
#define XZAMD_SPAN_MIN_LEN 65536u         /* shortest cost-balanced span */
#define XZAMD_BCJ_X86 4u    /* LZMA_FILTER_X86, api/lzma/bcj.h:20 */
#define XZAMD_BCJ_ARM64 0x0Au   /* LZMA_FILTER_ARM64, api/lzma/bcj.h (simple/arm64.c), start offset 0 */
#define XZAMD_BCJ_RISCV 0x0Bu   /* LZMA_FILTER_RISCV (simple/riscv.c) */
#define XZAMD_BCJ_POWERPC 5u    /* LZMA_FILTER_POWERPC (simple/powerpc.c) */
#define XZAMD_BCJ_IA64 6u       /* LZMA_FILTER_IA64 (simple/ia64.c) */
#define XZAMD_BCJ_ARM 7u        /* LZMA_FILTER_ARM (simple/arm.c) */
#define XZAMD_BCJ_ARMTHUMB 8u   /* LZMA_FILTER_ARMTHUMB (simple/armthumb.c) */
#define XZAMD_BCJ_SPARC 9u      /* LZMA_FILTER_SPARC (simple/sparc.c) */
#define XZAMD_FILTER_DELTA(dist) (3u | (((uint32_t)(dist) - 1u) << 8))   /* LZMA_FILTER_DELTA, dist 1..256 (delta/delta_encoder.c) */
#define XZAMD_SA_WINDOW_MAX 5u

/* lzma_lzma_preset() (lzma/lzma_encoder_presets.c:17-63) + the device mapping.
 * Returns nonzero for an invalid preset. */
int xzamd_lzma_preset(xzamd_lzma_options *opt, uint32_t preset);
/* For hand-made option sets: fill in what a BT2/BT3/BT4 + normal-mode request runs on the device (suffix-
 * neighbourhood finder, suffix depth from gpu_nice_len, windowed optimal parser, cost-balanced spans). */
void xzamd_sn_defaults(xzamd_lzma_options *opt);
/* NULL when the device path runs this option set, else the reason it does not (static string). */
const char *xzamd_options_check(const xzamd_lzma_options *opt);
/* Give back the device / pinned buffers lzma_end() keeps parked for the next stream of the process. */
void xzamd_release_parked(void);
/* lzma_mt_block_size() for a plain LZMA2 chain (lzma2_encoder.c:403-413). */
uint64_t xzamd_mt_block_size(const xzamd_lzma_options *opt);
/* lzma_block_buffer_bound64() (common/block_buffer_encoder.c:55-69). */
uint64_t xzamd_block_buffer_bound(uint64_t uncompressed_size);
/* Upper bound for the whole .xz Stream produced from in_size bytes. */
uint64_t xzamd_stream_buffer_bound(uint64_t in_size, uint64_t block_size);

/* Context = one GPU (device ordinal, -1 = current) + its work buffers. */
int xzamd_ctx_create(xzamd_ctx **ctx, int device);
void xzamd_ctx_destroy(xzamd_ctx *ctx);
/* Bytes of input processed per device batch (default 2 GiB - 1 MiB; must be < 2 GiB: positions are 31-bit).
 */
int xzamd_ctx_set_batch_bytes(xzamd_ctx *ctx, uint64_t bytes);
const char *xzamd_last_error(const xzamd_ctx *ctx);
int xzamd_ctx_device(const xzamd_ctx *ctx);          /* device ordinal the context lives on */

typedef struct {
	uint64_t in_bytes, out_bytes;
	uint64_t blocks, spans, batches;
	uint64_t blocks_stored;      /* Blocks that took the uncompressed fallback */
	/* HIP-event time per stage, summed over batches (milliseconds) */
	float ms_chains;             /* hash keys + radix sorts + link kernels */
	float ms_encode;             /* k_find (when the optimal parser runs) + k_span_encode */
	float ms_crc;
	float ms_assemble;
	float ms_total;              /* first launch -> last kernel done */
	uint32_t encode_launches;
	float ms_find;               /* the k_find part of ms_encode */
	uint32_t span_size;          /* bytes per span the last encode used (0: cost-balanced spans) */
	float ms_find_overlapped;    /* k_find of batches whose structure + lists were made underneath the previous span kernel */
	uint32_t span_cost_used;     /* cost-balanced spans: work target of the LAST batch (>= span_cost) */
	float ms_plan;               /* span plan (k_span_est + k_span_cut) */
	uint32_t wave_slots;         /* span wavefronts the GPU holds at once (CUs x occupancy of the span kernel) */
	uint64_t enc_spans;          /* two-phase: encode spans (= state resets + 1 per Block); `spans` counts the parse pieces */
	float ms_seed;               /* two-phase: the seed pieces (one wavefront per Block, part of ms_encode) */
	float ms_parse;              /* two-phase: every other piece */
	float ms_code;               /* two-phase: the coder's walk (bounds, chain, tokens) + the range coder, second stream */
	float ms_iter1;              /* two-phase: the part of ms_parse spent in the partial iteration(s) and the carried walk over their records;
	                                ms_parse - ms_iter1 = the full parse (k_parse_pieces, iteration 2): the dominant kernel */
	float ms_verify;             /* XZAMD_F_VERIFY: the verification of the finished Stream (wall time, not part of ms_total) */
	uint32_t batches_ahead;      /* batches whose filters and structure build were issued ahead, under the parse of the batch before
	                                (XZAMD_BUILD_AHEAD).  Their ms_chains spans a build that shares the GPU with that parse: it grows
	                                while ms_total shrinks.  (The field takes the place of padding: the layout is what it was.) */
} xzamd_stats;
/* Stats of the last xzamd_stream_encode_device call of the context.  Under the lzma_* front end consecutive jobs of a
 * worker are pipelined (the back end of a job's last batch finishes underneath the next job's front end): there the stage
 * times, blocks, spans and batches of that carried batch are booked to the call that finishes it, i.e. the figures are
 * running per-context totals shifted by one batch, not per-job figures. */
void xzamd_get_stats(const xzamd_ctx *ctx, xzamd_stats *out);

/* Encode in_size bytes resident in device memory (d_in) into a complete,
 * standards-conformant .xz Stream in device memory (d_out): Stream Header,
 * one Block per block_size bytes (Block Header with both sizes, LZMA2 data,
 * padding, Check), Index, Stream Footer -- exactly the layout
 * lzma_stream_encoder_mt produces (stream_encoder_mt.c:717-883).
 *
 * flags: XZAMD_F_BLOCKS_ONLY emits only the Blocks (no header/index/footer)
 * and reports per-Block sizes through `binfo` so several GPUs can each encode
 * a shard and one of them frames the Stream.
 *
 * block_size 0 = xzamd_mt_block_size(opt). check = XZAMD_CHECK_*.
 * Returns XZAMD_OK or an error code. */
#define XZAMD_F_BLOCKS_ONLY 1u
/* XZAMD_F_SEGMENTS (implies XZAMD_F_BLOCKS_ONLY): every block_size bytes of the input are a SEGMENT of one larger Block
 * that the caller frames (the single-Block Stream of lzma_stream_encoder).  Per segment only its LZMA2
 * chunk chain is written -- the bytes between the Block Header and the end marker of the Block the MT layout would make
 * of it: no header, no 0x00 end marker, no padding, no Check.  Every chain starts with a dictionary reset, so the
 * chains of consecutive segments followed by one 0x00 are one valid LZMA2 stream.  binfo[i] then carries:
 * total_size = length of the chain, uncompressed_size, out_offset, and unpadded_size = the segment's Check value
 * (CRC32 zero-extended / CRC64; 0 for XZAMD_CHECK_NONE) for xzamd_crc32_combine / xzamd_crc64_combine.
 * Chain {LZMA2} and Checks none / CRC32 / CRC64 only (else XZAMD_OPTIONS_ERROR). */
#define XZAMD_F_SEGMENTS 2u

/* XZAMD_F_KEEP_RESUME: the two-phase encode (presets 4-9, default spans) exports one RESUME RECORD per encode span -- Block,
 * offset inside the Block, lc / lp / pb, coder state, rep distances and the coder's model at the span start -- into a table
 * the context keeps until its next encode or xzamd_ctx_destroy: what xzamd_stream_verify_device needs to decode every encode
 * span as a unit of its own.  About encode spans x (32 + 2 x model size) bytes of device memory (16 KB per >= 256 KiB of
 * input at lc + lp = 3), allocated only when asked for.  The single-phase modes (presets 0-3, explicit span sizes) write no
 * records: their spans reset the state and carry the properties, which the verification decode cuts at anyway.  The bytes of
 * the Stream do not depend on the flag.
 * XZAMD_F_VERIFY (implies XZAMD_F_KEEP_RESUME): VERIFIED ENCODE.  Behind the last batch the finished Stream in d_out goes
 * through xzamd_stream_verify_device against d_in before the call returns: chunk-grammar scan, span-parallel decode, Checks,
 * comparison with the input.  Any defect returns XZAMD_DATA_ERROR, xzamd_last_error names the Block and the step,
 * xzamd_get_verify_report has the details, and *out_size is still set: the caller never gets XZAMD_OK for a Stream the device
 * decoder rejects or that differs from the input.  Nothing is rewritten; the caller decides what to do with the Stream
 * (xzamd_stream_verify_blocks_device names every bad Block, xzamd_stream_repair_device replaces them; XZAMD_F_REPAIR does both).
 * (Known at this version: a Block whose first piece is stored raw -- e.g. 512 KiB of random bytes in front of text -- can come
 * out with its first LZMA chunk lacking the properties byte, which every decoder rejects; XZAMD_F_VERIFY is what reports it,
 * XZAMD_F_REPAIR delivers a valid Stream for it; the same holds for the segments of XZAMD_F_SINGLE.)
 * Either flag with XZAMD_F_BLOCKS_ONLY or XZAMD_F_SEGMENTS is XZAMD_OPTIONS_ERROR: there is no container to read.
 * XZAMD_F_REPAIR (implies XZAMD_F_VERIFY): VERIFIED AND REPAIRED ENCODE.  The verification is the per-Block one
 * (xzamd_stream_verify_blocks_device); every Block it rejects is re-encoded from its slice of d_in and spliced into d_out as
 * xzamd_stream_repair_device does, with the call's own options, before the call returns: XZAMD_OK, *out_size = the repaired size,
 * binfo rewritten for the Blocks that moved, xzamd_get_repair_report says what happened, xzamd_get_verify_report describes the
 * final, passing verification.  A Stream without a bad Block is byte for byte that of a call without the flag.
 * XZAMD_F_REPAIR | XZAMD_F_BLOCKS_ONLY is allowed (binfo must then hold every Block: the Block table is read from it and from
 * the Block Headers in d_out; the splice rewrites the bare Blocks and binfo).  XZAMD_F_REPAIR | XZAMD_F_SEGMENTS is
 * XZAMD_OPTIONS_ERROR: the chunk chains of a single-Block Stream are not Blocks -- they are verified and replaced through
 * XZAMD_F_SINGLE below, or on their own with xzamd_chains_verify_device / xzamd_chains_repair_device.  A call with
 * XZAMD_F_REPAIR never defers its back end.
 * XZAMD_F_SINGLE: the call writes the complete SINGLE-BLOCK Stream lzma_stream_encoder / lzma_easy_encoder of this library write
 * (DESIGN.md 3.7), on the device: Stream Header, the 12-byte Block Header without sizes, the chunk chains of the segments of
 * block_size bytes (exactly what XZAMD_F_SEGMENTS writes), 0x00 and Block Padding, the Check folded from the segments' CRCs, an
 * Index of one record, Stream Footer.  binfo describes the SEGMENTS as under XZAMD_F_SEGMENTS, with offsets inside the Stream;
 * *nblocks = their number.  An empty input gives a Stream without a Block.  XZAMD_F_SINGLE | XZAMD_F_KEEP_RESUME, | XZAMD_F_VERIFY
 * and | XZAMD_F_REPAIR are valid and act on the chains BEFORE they are framed (the resume records name segments): with
 * XZAMD_F_VERIFY a defect is XZAMD_DATA_ERROR, *out_size is still set to the framed Stream and the report's first_bad_block is
 * the segment; with XZAMD_F_REPAIR the rejected segments are replaced (xzamd_chains_repair_device), the delivered Stream is
 * valid and xzamd_get_repair_report counts segments.  With XZAMD_F_BLOCKS_ONLY or XZAMD_F_SEGMENTS, with SHA-256 or with a filter
 * in front of LZMA2: XZAMD_OPTIONS_ERROR.  Not covered: xzamd_stream_verify_device on the framed Stream cuts no units at the
 * kept records of a Stream of several segments (they name segments, the Stream has one Block): it verifies with one unit per
 * segment, at the dictionary resets. */
#define XZAMD_F_KEEP_RESUME 4u
#define XZAMD_F_VERIFY 8u
#define XZAMD_F_REPAIR 16u
#define XZAMD_F_SINGLE 32u
/* XZAMD_F_AUTO_DELTA: AUTOMATIC PER-BLOCK DELTA FILTER for the chain {LZMA2} (DESIGN.md 3.5 "Automatic delta").  For every
 * Block the device counts byte histograms of a sample of the Block (4 KiB of every 64 KiB) as it is and after delta(d), d in
 * {1, 2, 3, 4, 6, 8, 12, 16, 24, 32}, prices each with an integer order-0 entropy, and gives the Block the filter delta(d) with
 * the lowest price when that is at least half a bit per byte below the unfiltered one; else the Block stays {LZMA2}.  The
 * chain is written into each Block Header, so the Blocks of one Stream may differ: plain .xz, read by any decoder.  Blocks
 * that go out stored carry no filter, as always.  Nothing but the flag is needed; the choice costs no host synchronisation.
 * Allowed with XZAMD_F_BLOCKS_ONLY, _KEEP_RESUME and _VERIFY, every Check and every preset.  XZAMD_OPTIONS_ERROR with a filter
 * already in front of LZMA2 (opt->bcj != 0), with XZAMD_F_SEGMENTS or XZAMD_F_SINGLE (a single Block has one chain), with
 * XZAMD_F_REPAIR (the repair plans the headers of the Blocks it replaces from one chain for the whole Stream), and over a kernel
 * layer without the entry points.  Without the flag no byte this library writes changes. */
#define XZAMD_F_AUTO_DELTA 64u
/* XZAMD_F_AUTO_BCJ: AUTOMATIC PER-BLOCK BCJ FILTER for the chain {LZMA2} (DESIGN.md 3.5 "Automatic BCJ").  For every Block the
 * device finds the call sites of two candidates over the whole Block -- x86 (E8 / E9 whose operand's top byte is 00 / FF) and
 * ARM64 (BL at a 4-byte offset of the Block) -- counts 4096-bucket hashed histograms of their operands as stored and as the
 * filter would store them (made absolute), prices both with the integer order-0 entropy of the automatic delta, and gives the
 * Block the filter when it has at least 256 sites, one per 2 KiB or denser, and the absolute operands are at least half a bit
 * per site cheaper; of two candidates that qualify the one that saves more, x86 on a tie; else the Block stays {LZMA2}.  The
 * Block is then filtered exactly as the fixed chain {x86, LZMA2} / {ARM64, LZMA2} filters it, and the chain is written into
 * its Block Header: plain .xz, read by any decoder.  Together with XZAMD_F_AUTO_DELTA both analyses run; a Block takes the
 * BCJ filter when that rule fires and else what the delta rule says -- never two filters.  Blocks that go out stored carry no
 * filter.  Allowed and declined (XZAMD_OPTIONS_ERROR) exactly where XZAMD_F_AUTO_DELTA is: not with a filter already in front
 * of LZMA2, XZAMD_F_SEGMENTS, XZAMD_F_SINGLE or XZAMD_F_REPAIR, nor over a kernel layer without the entry points; with
 * XZAMD_F_VERIFY every Block is its own verification unit.  Without the flag no byte and no launch changes. */
#define XZAMD_F_AUTO_BCJ 128u
/* XZAMD_F_AUTO_LCLP: AUTOMATIC PER-BLOCK LITERAL CONTEXT (DESIGN.md 3.5 "Automatic literal context").  For every Block the
 * device counts one joint histogram [offset & 7][byte in front >> 5][byte] over the sample set of the automatic delta, of the
 * bytes LZMA2 codes (behind the Block's filters, chosen or fixed), prices every (lc, lp) with lc <= 3, lp <= 3 and
 * lc + lp <= opt->lc + opt->lp by the integer order-0 entropy of the bytes under its contexts plus 12 bits per used (context,
 * byte) cell, and parses and codes the Block with the cheapest pair when that is at least an eighth of a bit per byte below
 * the job's own; else with opt->lc / opt->lp.  pb is never chosen.  The pair stands in the properties byte of the Block's
 * LZMA2 chunks, not in its Block Header: plain .xz, read by any decoder.  A job with lc or lp of 4 keeps its pair everywhere.
 * Allowed with every filter chain, XZAMD_F_AUTO_DELTA / _AUTO_BCJ, XZAMD_F_BLOCKS_ONLY, _KEEP_RESUME and _VERIFY (the resume
 * records carry the Block's pair), every Check and every preset.  XZAMD_OPTIONS_ERROR with XZAMD_F_SEGMENTS, XZAMD_F_SINGLE or
 * XZAMD_F_REPAIR, and over a kernel layer without the entry points.  Without the flag no byte this library writes changes. */
#define XZAMD_F_AUTO_LCLP 256u

typedef struct {
	uint64_t unpadded_size;      /* Index record field 1 (block_util.c:45-76) */
	uint64_t uncompressed_size;  /* Index record field 2 */
	uint64_t out_offset;         /* where the Block starts in d_out */
	uint64_t total_size;         /* header + data + padding + check */
} xzamd_block_info;

int xzamd_stream_encode_device(xzamd_ctx *ctx,
		const void *d_in, uint64_t in_size, uint64_t block_size,
		const xzamd_lzma_options *opt, int check, uint32_t flags,
		void *d_out, uint64_t out_cap, uint64_t *out_size,
		xzamd_block_info *binfo, uint64_t binfo_cap, uint64_t *nblocks,
		void *stream);

/* The analysis of XZAMD_F_AUTO_DELTA on its own: dist_out[b] (host memory, cap entries) = the delta distance the rule picks
 * for Block b of the in_size bytes at d_in cut into Blocks of block_size bytes, 0 = no filter; *nblocks = their number.
 * XZAMD_BUF_ERROR when cap is too small (*nblocks is set), XZAMD_OPTIONS_ERROR for block_size 0 or >= 2 GiB or over a kernel
 * layer without the entry points.  The histograms and choices stay fetchable (XZAMD_DEBUG_DELTA_HIST / _DIST) for inputs of
 * one device batch. */
int xzamd_auto_delta_device(xzamd_ctx *ctx, const void *d_in, uint64_t in_size, uint64_t block_size, uint32_t *dist_out,
		uint64_t cap, uint64_t *nblocks, void *stream);

/* The analysis of XZAMD_F_AUTO_BCJ on its own, in the same form: kind_out[b] = the filter id the rule picks for Block b
 * (XZAMD_BCJ_X86, XZAMD_BCJ_ARM64), 0 = no filter.  The same errors; the histograms, site counts and choices stay fetchable
 * (XZAMD_DEBUG_BCJ_HIST / _KIND) for inputs of one device batch. */
int xzamd_auto_bcj_device(xzamd_ctx *ctx, const void *d_in, uint64_t in_size, uint64_t block_size, uint32_t *kind_out,
		uint64_t cap, uint64_t *nblocks, void *stream);

/* The analysis of XZAMD_F_AUTO_LCLP on its own, in the same form, on the bytes at d_in as they are: props_out[b] =
 * lc | lp << 8 the rule picks for Block b of a job with (lc, lp).  The same errors, and XZAMD_OPTIONS_ERROR for lc + lp > 4; the
 * histograms and choices stay fetchable (XZAMD_DEBUG_LCLP_HIST / _PROPS) for inputs of one device batch. */
int xzamd_auto_lclp_device(xzamd_ctx *ctx, const void *d_in, uint64_t in_size, uint64_t block_size, uint32_t lc, uint32_t lp,
		uint32_t *props_out, uint64_t cap, uint64_t *nblocks, void *stream);

/* Device .xz decoder (the reference's stream_decoder_mt.c / lzma2_decoder.c / lzma_decoder.c path, SURVEY.md
 * 8f.3): decode a single-Stream .xz file resident in device memory into d_out (trailing bytes, Stream Padding or a second
 * Stream are an error here: xzamd_file_decode_device reads those).  Filter chains, per Block: {LZMA2} and
 * {up to three of: delta (0x03) | x86, PowerPC, IA-64, ARM, ARM-Thumb, SPARC, ARM64, RISC-V BCJ (0x04 .. 0x0B), LZMA2};
 * declined with XZAMD_OPTIONS_ERROR: a BCJ start offset other than 0, any other filter id, any chain the reference's
 * lzma_validate_chain refuses.  A Stream with a filtered Block needs one or two temporaries of the uncompressed size.
 * Checks none / CRC32 / CRC64 / SHA-256 are verified, any other Check id is XZAMD_UNSUPPORTED_CHECK.  Blocks decode in parallel; inside a
 * Block a decode unit (one wavefront) starts at every LZMA2 chunk that resets the dictionary (control 0x01 or >= 0xE0): nothing in front
 * of it can be referenced, so a Block of many segments (lzma_stream_encoder's) decodes segment-parallel and a Block with one reset (the MT
 * encoders') is one unit; at most usize / 4096 + 8 units per Block, further resets stay inside the last unit.  With d_expected (the original
 * data, device memory, expected_size bytes: a Stream of another uncompressed size is XZAMD_DATA_ERROR) it is a VERIFICATION decode: every chunk chain that starts with a state
 * reset + properties (our spans) is its own unit, history is read from d_expected, and the decoded bytes are
 * compared with it afterwards (*mismatches).  For a filtered Stream the history is the filtered original (made with the
 * encoder's forward kernels when the Blocks are equally long but the last and share one chain; otherwise unit = Block).  Returns XZAMD_OK, 7 (LZMA_FORMAT_ERROR: not an .xz Stream),
 * XZAMD_OPTIONS_ERROR (unsupported chain), XZAMD_DATA_ERROR (corrupt / mismatch), XZAMD_BUF_ERROR (out_cap). */
int xzamd_stream_decode_device(xzamd_ctx *ctx, const void *d_xz, uint64_t xz_size, void *d_out, uint64_t out_cap,
		uint64_t *out_size, const void *d_expected, uint64_t expected_size, uint64_t *mismatches, uint64_t *nblocks,
		void *stream);

/* Verification of a Stream against its original, both in device memory: xzamd_stream_decode_device with d_expected into a
 * temporary of original_size bytes, with the resume table the context keeps (XZAMD_F_KEEP_RESUME) when it fits the Stream
 * -- as many Blocks of the same sizes as the encode it was kept from (nothing else is compared: ANOTHER Stream of that
 * geometry verified while the table is kept meets records that are not its own and is XZAMD_DATA_ERROR, a false alarm;
 * verify a Stream with the context that encoded it, or after an encode without the flag).  Then a decode unit starts at
 * the Block's first chunk and at every LZMA2 chunk start whose offset a record names, from the record's model instead of a
 * state reset: units = encode spans.  A record that no chunk start meets is XZAMD_DATA_ERROR (step "grammar"); a record whose
 * contents are wrong makes its unit fail or decode other bytes, which the comparison with the original reports -- the table
 * can cause a false alarm, never a false pass.  Without a fitting table (or for a filtered Stream of Blocks that differ in
 * length or chain) the units are those of xzamd_stream_decode_device, and the report says so.  *report may be NULL. */
#define XZAMD_VSTEP_NONE 0u
#define XZAMD_VSTEP_GRAMMAR 1u      /* container framing, LZMA2 chunk grammar, resume records against the chunk starts */
#define XZAMD_VSTEP_DECODE 2u       /* range coder, distances, chunk sizes */
#define XZAMD_VSTEP_CHECK 3u        /* the stored Check of a Block */
#define XZAMD_VSTEP_COMPARE 4u      /* decoded bytes differ from the original */
typedef struct {
	uint64_t units;              /* decode units (wavefronts' work items) */
	uint64_t blocks;
	uint64_t records_used;       /* resume records a unit started from */
	uint64_t first_bad_block;    /* UINT64_MAX: none, or not attributable to a Block (framing, comparison) */
	uint64_t mismatching_words;  /* 32-bit words of the decoded bytes that differ from the original */
	uint32_t table_used;         /* 1: the units were cut at the kept table's records */
	uint32_t first_bad_step;     /* XZAMD_VSTEP_* */
	float ms_verify;             /* wall time of the call */
	uint32_t reserved_;
} xzamd_verify_report;
int xzamd_stream_verify_device(xzamd_ctx *ctx, const void *d_xz, uint64_t xz_size, const void *d_original, uint64_t original_size,
		xzamd_verify_report *report, void *stream);
/* The report of the context's last verification (xzamd_stream_verify_device, xzamd_stream_verify_blocks_device, or an encode
 * with XZAMD_F_VERIFY / XZAMD_F_REPAIR). */
void xzamd_get_verify_report(const xzamd_ctx *ctx, xzamd_verify_report *out);

/* PER-BLOCK VERIFICATION: xzamd_stream_verify_device that does not stop at the first defect.  A Block that fails a step is
 * marked with that step and taken out of the later ones; the others go on.  block_steps receives one XZAMD_VSTEP_* per Block
 * (XZAMD_VSTEP_NONE = good).  A Block Header that fails its CRC32 or disagrees with the Index makes its Block bad at step
 * "grammar" (the Index gives its extent); a damaged Stream Header, Footer or Index fails the whole call as before
 * (first_bad_block = UINT64_MAX).  The steps speak about the Stream: a verification unit reads its history from the original,
 * so a Block that fails at "decode" or "check" goes through once more on its own (history = its own output) and that run decides
 * -- a wrong original shows as "compare".  The comparison counts differing bytes per Block.  The report's first_bad_step /
 * first_bad_block name the defect xzamd_stream_verify_device would have stopped at (steps in their order, the lowest Block of
 * a step; a comparison defect names its Block here).  d_original may be NULL: grammar, decode and Check only.
 * One Stream; the kept resume table is used when it fits, as by xzamd_stream_verify_device.
 * XZAMD_OK: every Block good.  XZAMD_DATA_ERROR: some Block bad, block_steps filled in.  XZAMD_BUF_ERROR: steps_cap too small,
 * *nblocks set. */
int xzamd_stream_verify_blocks_device(xzamd_ctx *ctx, const void *d_xz, uint64_t xz_size,
		const void *d_original, uint64_t original_size, uint8_t *block_steps, uint64_t steps_cap,
		uint64_t *nblocks, xzamd_verify_report *report, void *stream);

/* REPAIR: hand back a valid Stream for one the device decoder rejects, at the price of re-encoding the rejected Blocks only.
 * 1. per-Block verdicts (above); none bad: XZAMD_OK, the Stream untouched.
 * 2. every bad Block is re-encoded from its slice of the original (uncompressed offset and size from the Index), runs of
 *    adjacent bad Blocks of equal size in one call of the batch encoder.  Rung 1: `opt` single-phase -- an explicit span size
 *    of 256 KiB, every span starts with a state reset and the properties (an option set xzamd_options_check refuses that way,
 *    i.e. the optimal parser with pb > 2: the fast parser with the same dict_size / lc / lp / pb / filters) -- and verified
 *    again.  Rung 2, for what rung 1 leaves rejected: the stored form, uncompressed LZMA2 chunks with the filters dropped.
 * 3. splice: every Block behind the first repaired one moves, Index and Stream Footer are rebuilt.  The Check kind is the
 *    Stream's; the spliced Stream goes through the per-Block verification once more.
 * All or nothing: on any error the xz_size bytes at d_xz are what they were.  XZAMD_BUF_ERROR: the repaired Stream needs
 * *new_size > xz_cap bytes.  A kept resume table stays usable: the records of repaired Blocks become void. */
typedef struct {
	uint64_t blocks, blocks_bad, blocks_reencoded, blocks_stored;   /* reencoded: accepted from rung 1; stored: rung 2 */
	uint64_t size_before, size_after;
	uint32_t passes;             /* verification passes run (>= 1) */
	float ms_repair;             /* wall time, verification passes included */
	float ms_verify_passes, ms_reencode, ms_splice;      /* its parts */
	uint32_t reserved_;
} xzamd_repair_report;
int xzamd_stream_repair_device(xzamd_ctx *ctx, void *d_xz, uint64_t xz_size, uint64_t xz_cap,
		const void *d_original, uint64_t original_size, const xzamd_lzma_options *opt,
		uint64_t *new_size, xzamd_repair_report *report, void *stream);
/* The report of the context's last repair (xzamd_stream_repair_device or an encode with XZAMD_F_REPAIR). */
void xzamd_get_repair_report(const xzamd_ctx *ctx, xzamd_repair_report *out);

/* BARE CHUNK CHAINS: the segments of an XZAMD_F_SEGMENTS encode (the payload of the single-Block Stream of lzma_stream_encoder),
 * verified and repaired as the Blocks of a Stream are.  binfo[i] is what XZAMD_F_SEGMENTS fills in: out_offset and total_size =
 * where chain i lies in d_chains (`size` bytes) and how long it is, uncompressed_size, unpadded_size = the segment's Check value
 * (none: 0, CRC32 zero-extended, CRC64); segment i covers the original from the sum of the sizes in front of it.  opt gives the
 * dictionary size (and, for the repair, what to re-encode with).  Checks none / CRC32 / CRC64.
 * xzamd_chains_verify_device: one XZAMD_VSTEP_* per segment in seg_steps.  A chain is exactly total_size bytes, starts with a
 * dictionary reset and holds no 0x00 end marker ("grammar" otherwise); it decodes as a unit of its own, with d_original also cut
 * at its state resets or -- when the context keeps the resume table of the encode that made the chains -- at the records, which
 * name segments; the decoded bytes are checked against the row's CRC ("check") and the original ("compare").  d_original may be
 * NULL.  Codes as xzamd_stream_verify_blocks_device: XZAMD_OK, XZAMD_DATA_ERROR (some segment bad), XZAMD_BUF_ERROR (steps_cap <
 * nsegments).
 * xzamd_chains_repair_device: the chains must lie back to back and end at `size`.  Every rejected segment is re-encoded from its
 * slice of the original -- rung 1: opt single-phase, 256 KiB spans (the fast parser for an option set that cannot run that way);
 * rung 2: the stored chain, 0x01 + 64 KiB, then 0x02 chunks -- and spliced in: every chain behind the first replaced one moves,
 * binfo[i].out_offset / total_size are rewritten, the CRC and the uncompressed size stay.  The spliced chains pass the verdicts
 * once more before the call returns.  All or nothing: on any error chains and binfo are what they were.  XZAMD_BUF_ERROR: the
 * repaired chains need *new_size > cap bytes.  Codes and report as xzamd_stream_repair_device (its counts are segments). */
int xzamd_chains_verify_device(xzamd_ctx *ctx, const void *d_chains, uint64_t size, const xzamd_block_info *binfo, uint64_t nsegments,
		const xzamd_lzma_options *opt, int check, const void *d_original, uint64_t original_size, uint8_t *seg_steps,
		uint64_t steps_cap, xzamd_verify_report *report, void *stream);
int xzamd_chains_repair_device(xzamd_ctx *ctx, void *d_chains, uint64_t size, uint64_t cap, xzamd_block_info *binfo, uint64_t nsegments,
		const xzamd_lzma_options *opt, int check, const void *d_original, uint64_t original_size, uint64_t *new_size,
		xzamd_repair_report *report, void *stream);

/* ---- whole .xz files: concatenated Streams, Stream Padding, file index, range decode ----
 * An .xz file is one or more Streams, each followed by Stream Padding (zero bytes, a multiple of four): what `xz -d`
 * and every liblzma client with LZMA_CONCATENATED read.  The file is walked from its end, as the reference's
 * common/file_info.c does: Stream Padding, Stream Footer, Backward Size, Index; the padded Block sizes of the Index give
 * the place of the Stream Header; in front of it lies the padding of the Stream before.  All framing of all Streams is
 * validated before a Block is looked at, all Blocks before the first decode kernel runs.
 * Codes (common/stream_decoder.c with LZMA_CONCATENATED): 7 (LZMA_FORMAT_ERROR) only for a file shorter than 32 bytes or
 * without the Header Magic at offset 0; XZAMD_DATA_ERROR for every other framing defect (padding that is no multiple of
 * four, bad magic of a Footer or of a later Header, a Backward Size or Block sizes that do not land on a Stream Header,
 * Header and Footer that disagree); XZAMD_OPTIONS_ERROR for Stream Flags of an unknown version; XZAMD_UNSUPPORTED_CHECK
 * for a Check without a verifier in any Stream; inside a Block the codes of xzamd_stream_decode_device.
 * Streams may differ in Check and in filter chains; Streams without Blocks are legal. */
typedef struct {
	uint64_t offset;                /* of the Stream Header in the file */
	uint64_t size;                  /* Stream Header .. Stream Footer */
	uint64_t padding;               /* Stream Padding behind it */
	uint64_t first_block;           /* index of its first Block in the Block list */
	uint64_t block_count;
	uint64_t uncompressed_offset;   /* of its first byte in the decoded file */
	uint64_t uncompressed_size;
	uint32_t check;                 /* XZAMD_CHECK_* */
	uint32_t reserved_;
} xzamd_xz_stream;

typedef struct {
	uint64_t header_offset;         /* of the Block Header in the file */
	uint64_t unpadded_size;         /* Index record */
	uint64_t total_size;            /* Unpadded Size rounded up to four: header + data + padding + check */
	uint64_t uncompressed_size;     /* Index record */
	uint64_t uncompressed_offset;   /* of its first byte in the decoded file */
	uint32_t stream;                /* index of its Stream */
	uint32_t filter_count;
	uint32_t filter_ids[4];         /* in Block Header order, LZMA2 (0x21) last */
} xzamd_xz_block;

/* List the Streams and Blocks of a file (xz --list, lzma_file_info_decoder) and validate all of its framing: Stream
 * Headers / Footers / Padding, Indexes, every Block Header, sizes against the Index, Block Padding.  *nstreams, *nblocks,
 * *uncompressed_size are always filled in once the framing is valid; XZAMD_BUF_ERROR when a capacity is too small
 * (streams / blocks may be NULL with capacity 0).  The host variant reads host memory and needs neither a GPU nor a
 * context; the device variant reads device memory: three small reads per Stream, and one kernel (one thread per Block)
 * for all Block Headers. */
int xzamd_file_index_host(const void *xz, uint64_t xz_size, xzamd_xz_stream *streams, uint64_t streams_cap, uint64_t *nstreams,
		xzamd_xz_block *blocks, uint64_t blocks_cap, uint64_t *nblocks, uint64_t *uncompressed_size);
int xzamd_file_index_device(xzamd_ctx *ctx, const void *d_xz, uint64_t xz_size, xzamd_xz_stream *streams, uint64_t streams_cap,
		uint64_t *nstreams, xzamd_xz_block *blocks, uint64_t blocks_cap, uint64_t *nblocks, uint64_t *uncompressed_size);

/* xzamd_stream_decode_device for a whole file: any number of Streams plus Stream Padding.  The Blocks of all Streams form
 * one table and go through one scan and one decode launch; the Checks are verified per Stream.  With d_expected the
 * span-parallel units of the verification decode are kept for a file of one Stream; a file of several Streams decodes
 * Block by Block; the result is compared with the original either way.  *nblocks = Blocks of all Streams. */
int xzamd_file_decode_device(xzamd_ctx *ctx, const void *d_xz, uint64_t xz_size, void *d_out, uint64_t out_cap,
		uint64_t *out_size, const void *d_expected, uint64_t expected_size, uint64_t *mismatches, uint64_t *nblocks,
		void *stream);

/* Decode uncompressed bytes [uoffset, uoffset + ulen) of a file by decoding only the Blocks that hold them (and
 * verifying their Checks): random access into an .xz file of small Blocks.  The range is clipped at the end of the file
 * like pread: *out_size = bytes written at d_out (0 for an offset at or behind the end, or ulen 0: nothing is decoded).
 * Stream framing and Indexes are validated for the whole file, Block framing for the Blocks that are decoded: a defect
 * of another Block does not fail the call.  A range that starts and ends on Block boundaries decodes straight into
 * d_out, any other into a temporary of the touched Blocks from which the range is copied.  *blocks_decoded = Blocks
 * touched.  XZAMD_BUF_ERROR (with *out_size set) when out_cap is smaller than the clipped range. */
int xzamd_file_decode_range_device(xzamd_ctx *ctx, const void *d_xz, uint64_t xz_size, uint64_t uoffset, uint64_t ulen,
		void *d_out, uint64_t out_cap, uint64_t *out_size, uint64_t *blocks_decoded, void *stream);

/* ---- forward decode: a file read from its front, without its Index ----
 * xzamd_file_decode_device needs the last byte of a file before it can decode the first.  This entry reads as the
 * reference's lzma_stream_decoder does (common/stream_decoder.c, index_hash.c): Stream Header, then Block after Block -- a
 * kernel of one wavefront finds them, by the sizes in their headers or, where a header has none, by walking the LZMA2
 * chunk headers -- and only then the Index and the Stream Footer, which must be exactly what these Blocks call for.  So a
 * truncated file, or one that is damaged in or behind a Block, decodes as far as its last whole good Block:
 *   XZAMD_OK          the whole input was read (without XZAMD_FWD_CONCATENATED: up to the end of the first Stream;
 *                     report->consumed tells where that is)
 *   XZAMD_BUF_ERROR   the input ends early (report->stop = XZAMD_FWD_TRUNCATED: every complete Block in front of the end is
 *                     delivered, a partial last Block is not), or out_cap is too small (XZAMD_FWD_OUT_FULL: the Blocks that
 *                     fit are delivered)
 *   any other code    that of the first defect (report->stop = XZAMD_FWD_DEFECT, report->code / step); the Blocks in front
 *                     of it are delivered, their Checks verified
 * *out_size = the bytes delivered at d_out, whatever the code.  Codes as xzamd_file_decode_device gives them, but 7
 * (LZMA_FORMAT_ERROR) only for twelve first bytes without the Header Magic.  One walk launch and a constant number of small
 * reads per Stream, whatever its Block count. */
#define XZAMD_FWD_CONCATENATED 1u   /* read Stream Padding and further Streams (LZMA_CONCATENATED) */
#define XZAMD_FWD_END 1u
#define XZAMD_FWD_TRUNCATED 2u
#define XZAMD_FWD_DEFECT 3u
#define XZAMD_FWD_OUT_FULL 4u
typedef struct {
	uint64_t streams;               /* Streams read to the end of their Footer */
	uint64_t blocks;                /* Blocks met whole */
	uint64_t blocks_delivered;      /* ... of them decoded, verified and counted in *out_size */
	uint64_t consumed;              /* bytes of the input dealt with */
	uint64_t stop_offset;           /* of the Block or framing piece the read stopped at */
	uint32_t stop;                  /* XZAMD_FWD_* */
	uint32_t code;                  /* XZAMD_FWD_DEFECT: the code returned */
	uint32_t step;                  /* ... and, for a defect of a Block Header or chunk chain, which check failed */
	uint32_t reserved_;
} xzamd_forward_report;
int xzamd_file_decode_forward_device(xzamd_ctx *ctx, const void *d_xz, uint64_t xz_size, uint32_t flags,
		void *d_out, uint64_t out_cap, uint64_t *out_size, xzamd_forward_report *report, void *stream);

/* Host-side framing helpers for the multi-GPU path: Stream Header (12 bytes),
 * Index + Stream Footer from gathered Block records. Return bytes written. */
uint64_t xzamd_frame_header(uint8_t *out, int check);
uint64_t xzamd_frame_index_footer(uint8_t *out, uint64_t out_cap, int check,
		const uint64_t *unpadded, const uint64_t *uncompressed, uint64_t nblocks);

/* CRC of the concatenation A || B from crc(A), crc(B) and the length of B: crc(A) is advanced over len_b zero bytes
 * (multiplication by x^(8 len_b) in GF(2)[x] modulo the polynomial, by squaring) and crc(B) is added.  CRC32 = the
 * IEEE 802.3 polynomial (zlib.crc32, check/crc32_fast.c), CRC64 = ECMA-182 as liblzma writes it (check/crc64_fast.c). */
uint32_t xzamd_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
uint64_t xzamd_crc64_combine(uint64_t crc_a, uint64_t crc_b, uint64_t len_b);

/* Debug hook for the parity tests: when set, the next encode records every
 * LZMA symbol (span, pos, back, len as 4 x u32) into a device buffer of
 * `cap` symbols; xzamd_trace_read copies it out. Not for production use. */
int xzamd_trace_enable(xzamd_ctx *ctx, uint32_t cap);
int xzamd_trace_read(xzamd_ctx *ctx, uint32_t *out, uint32_t cap, uint32_t *count);

/* Debug hook for the parity tests: copy a work buffer of the LAST batch of the last encode to the host
 * (suffix order slot -> position, position -> slot, the 8 x u32 match-list records, their u16 lengths). */
#define XZAMD_DEBUG_SA 1
#define XZAMD_DEBUG_SA_RANK 2
#define XZAMD_DEBUG_LISTS 3
#define XZAMD_DEBUG_LIST_LENS 4
#define XZAMD_DEBUG_SPAN_TAB 5      /* span plan: (first byte, end) per span slot, slots = Block * (block_size / 64 KiB + 2) + k */
#define XZAMD_DEBUG_SPAN_CNT 6      /* spans per Block */
#define XZAMD_DEBUG_LITP 8          /* literal-coder slices of the span slots (timing builds leave a per-span record there) */
#define XZAMD_DEBUG_SPAN_EST 7      /* per 4 KiB chunk: work estimates of every Block, then the bit estimates */
#define XZAMD_DEBUG_SYM_LEN 9       /* two-phase: u16 per position, valid at symbol starts (0 = literal) */
#define XZAMD_DEBUG_SYM_DIST 10     /* two-phase: u32 per position (distance / literal bytes) */
#define XZAMD_DEBUG_ENC_TAB 11      /* two-phase: (first byte, end) per encode-span slot, slots = Block * (block_size / 256 KiB + 1) + j */
#define XZAMD_DEBUG_ENC_CNT 12      /* encode spans per Block */
#define XZAMD_DEBUG_PINFO 13        /* two-phase: 16 x u32 per piece slot ([0..7] iteration 1, [8..15] iteration 2: state | ok << 31, rep distances, raw) */
#define XZAMD_DEBUG_SNAP_SR 14      /* 8 x u32 per piece slot: state and rep distances a piece starts iteration 2 with */
#define XZAMD_DEBUG_PRIOR 15        /* 1856 x u32 per piece slot: the non-literal probabilities of the piece's price model (after the run: as adapted) */
#define XZAMD_DEBUG_CARRY 16        /* the coder's walk, per encode-span slot: 0 = reset + properties, 1 = carried, 2 = flat start */
#define XZAMD_DEBUG_CB_HDR 17       /* the coder's bounds walk, per encode-span slot: XZAMD_CB_* flags */
#define XZAMD_DEBUG_CB_START 18     /* the coder's walk: the model at the span start, u16 per probability (padded to 64) */
#define XZAMD_DEBUG_DELTA_HIST 19   /* XZAMD_F_AUTO_DELTA / xzamd_auto_delta_device, last batch: 11 x 256 x u32 per Block (candidates none, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32) */
#define XZAMD_DEBUG_DELTA_DIST 20   /* ... the chosen distance per Block, u32 (0 = no filter) */
#define XZAMD_DEBUG_BCJ_HIST 21     /* XZAMD_F_AUTO_BCJ / xzamd_auto_bcj_device, last batch of nb Blocks: nb x 2 x 2 x 4096 x u32 ([Block][x86, ARM64][operand as stored, absolute][bucket]), then nb x 2 x u32 site counts */
#define XZAMD_DEBUG_BCJ_KIND 22     /* ... the chosen filter id per Block, u32 (0 = no filter) */
#define XZAMD_DEBUG_LCLP_HIST 23    /* XZAMD_F_AUTO_LCLP / xzamd_auto_lclp_device, last batch: 8 x 8 x 256 x u32 per Block ([offset & 7][byte in front >> 5][byte]); whole Blocks only */
#define XZAMD_DEBUG_LCLP_PROPS 24   /* ... the chosen lc | lp << 8 per Block, u32 */
int xzamd_debug_fetch(xzamd_ctx *ctx, int what, void *host_out, uint64_t bytes);

/* Seeded synthetic corpora used by bench.py and the tests (host memory). */
void xzamd_corpus_lorem(uint8_t *out, uint64_t n);                 /* tests/create_compress_files.c:110-152 continued */
void xzamd_corpus_text(uint8_t *out, uint64_t n, uint64_t seed, int threads);   /* Zipf/Markov "enwik-style" */
/* ustar stream of the source trees under `roots` (':'-separated directories of the box,
 * walked in strcmp order), cycled to n bytes with a per-cycle byte-level perturbation.  Returns the number of
 * files in one cycle (0: nothing readable, out is zero-filled). */
uint64_t xzamd_corpus_tar(uint8_t *out, uint64_t n, const char *roots, uint64_t seed);
#define XZAMD_TAR_ROOTS "/opt/rocm/include:/usr/include:/usr/lib/python3:/usr/lib/python3.10"

const char *xzamd_version(void);

#ifdef __cplusplus
}
#endif
#endif
