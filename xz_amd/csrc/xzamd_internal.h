/* xzamd_internal.h -- shared by the plain-C host translation units only (not part of any ABI). */
#ifndef XZAMD_INTERNAL_H
#define XZAMD_INTERNAL_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/xz_amd.h"
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

/* The device part of a decode (xzamd_decode.c), shared by the single-Stream entry and the file entries (xzamd_file.c). */
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

double xzamd_work_bytes_per_byte_(const xzamd_lzma_options *opt);   /* device work buffers per input byte of a batch */

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
