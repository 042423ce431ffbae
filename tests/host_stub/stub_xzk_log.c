/* stub_xzk_log.c -- TEST INFRASTRUCTURE ONLY: a log of the kernel-layer calls of the batch encode with the stream each one is
 * enqueued on, for tests/host_stub/driver_build_ahead.c (tests/test_host_build_ahead.py).  The program is linked with the
 * linker's --wrap for every function below: the stand-ins of stub_xzk.c / stub_xzk_delta.c run unchanged behind the log line.
 * One line per call, in the order the host enqueues them (the stand-in streams are synchronous):
 *     op <name> <stream> [<event> | <input pointer> <n>]
 * Streams, events and pointers are printed as they are: the checker only compares them. */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../xz_amd/csrc/kernels_api.h"
#include <stdio.h>

int stub_log_on;

#define LOG(...) do { if (stub_log_on) { printf("op " __VA_ARGS__); printf("\n"); } } while (0)

int __real_xzk_stream_wait_event(void *st, void *ev);
int __wrap_xzk_stream_wait_event(void *st, void *ev) { LOG("wait %p %p", st, ev); return __real_xzk_stream_wait_event(st, ev); }
int __real_xzk_event_record(void *ev, void *st);
int __wrap_xzk_event_record(void *ev, void *st) { LOG("record %p %p", st, ev); return __real_xzk_event_record(ev, st); }
int __real_xzk_sync(void *st);
int __wrap_xzk_sync(void *st) { LOG("sync %p", st); return __real_xzk_sync(st); }

int __real_xzk_build_chains(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks,
		uint32_t hash_bytes, uint32_t hash_mask, uint32_t hash_bits, uint32_t sa_depth,
		uint32_t *keys_a, uint32_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, void *sort_tmp, uint64_t sort_tmp_bytes,
		uint32_t *rank, uint32_t *sorted_pos, uint32_t *prev2, uint32_t *prev3,
		uint32_t *prev4, uint64_t *rp8, uint64_t *rp16, uint64_t *key64_a, uint64_t *key64_b,
		uint32_t *sa, uint32_t *sa_rank, uint32_t *prev24, uint32_t *prev32, void *stream);
int __wrap_xzk_build_chains(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks,
		uint32_t hash_bytes, uint32_t hash_mask, uint32_t hash_bits, uint32_t sa_depth,
		uint32_t *keys_a, uint32_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, void *sort_tmp, uint64_t sort_tmp_bytes,
		uint32_t *rank, uint32_t *sorted_pos, uint32_t *prev2, uint32_t *prev3,
		uint32_t *prev4, uint64_t *rp8, uint64_t *rp16, uint64_t *key64_a, uint64_t *key64_b,
		uint32_t *sa, uint32_t *sa_rank, uint32_t *prev24, uint32_t *prev32, void *stream)
{
	LOG("build %p %p %u", stream, (const void *)d_in, n);
	return __real_xzk_build_chains(d_in, n, block_size, nblocks, hash_bytes, hash_mask, hash_bits, sa_depth, keys_a, keys_b, vals_a, vals_b,
			sort_tmp, sort_tmp_bytes, rank, sorted_pos, prev2, prev3, prev4, rp8, rp16, key64_a, key64_b, sa, sa_rank, prev24, prev32, stream);
}

int __real_xzk_find_matches(const xzamd_span_args *a, const uint32_t *sa, const uint32_t *sa_rank, const uint32_t *prev4,
		const uint64_t *rp8, const uint64_t *rp16, const uint32_t *prev24, const uint32_t *prev32,
		uint16_t *mlen, uint32_t *mdist, int part, void *stream);
int __wrap_xzk_find_matches(const xzamd_span_args *a, const uint32_t *sa, const uint32_t *sa_rank, const uint32_t *prev4,
		const uint64_t *rp8, const uint64_t *rp16, const uint32_t *prev24, const uint32_t *prev32,
		uint16_t *mlen, uint32_t *mdist, int part, void *stream)
{
	LOG("find %p %p %u", stream, (const void *)a->in, a->n);
	return __real_xzk_find_matches(a, sa, sa_rank, prev4, rp8, rp16, prev24, prev32, mlen, mdist, part, stream);
}

int __real_xzk_span_plan(const xzamd_span_args *a, uint32_t nblocks, uint32_t *est, unsigned long long *totals,
		uint32_t *span_tab, uint32_t *span_cnt, uint32_t cost_min, uint32_t bits_min, uint32_t min_len,
		uint32_t *enc_tab, uint32_t *enc_cnt, uint32_t *order_bufs, void *sort_tmp, uint64_t sort_tmp_bytes, uint32_t **order_out, void *stream);
int __wrap_xzk_span_plan(const xzamd_span_args *a, uint32_t nblocks, uint32_t *est, unsigned long long *totals,
		uint32_t *span_tab, uint32_t *span_cnt, uint32_t cost_min, uint32_t bits_min, uint32_t min_len,
		uint32_t *enc_tab, uint32_t *enc_cnt, uint32_t *order_bufs, void *sort_tmp, uint64_t sort_tmp_bytes, uint32_t **order_out, void *stream)
{
	LOG("plan %p %p %u", stream, (const void *)a->in, a->n);
	return __real_xzk_span_plan(a, nblocks, est, totals, span_tab, span_cnt, cost_min, bits_min, min_len, enc_tab, enc_cnt, order_bufs,
			sort_tmp, sort_tmp_bytes, order_out, stream);
}

int __real_xzk_parse_pieces(const xzamd_span_args *a, uint32_t nblocks, int phase, uint32_t waves, uint32_t *counter, void *stream);
int __wrap_xzk_parse_pieces(const xzamd_span_args *a, uint32_t nblocks, int phase, uint32_t waves, uint32_t *counter, void *stream)
{
	LOG("%s %p %p %u", phase == 0 ? "seeds" : (a->iter & XZAMD_ITER_PARTIAL) ? "parse_part" : "parse_full", stream, (const void *)a->in, a->n);
	return __real_xzk_parse_pieces(a, nblocks, phase, waves, counter, stream);
}

int __real_xzk_model_snapshots(const xzamd_span_args *a, uint32_t nblocks, void *stream);
int __wrap_xzk_model_snapshots(const xzamd_span_args *a, uint32_t nblocks, void *stream)
{
	LOG("snapshots %p %p %u", stream, (const void *)a->in, a->n);
	return __real_xzk_model_snapshots(a, nblocks, stream);
}

int __real_xzk_encode_syms(const xzamd_span_args *a, uint32_t nblocks, void *stream);
int __wrap_xzk_encode_syms(const xzamd_span_args *a, uint32_t nblocks, void *stream)
{
	LOG("code %p %p %u", stream, (const void *)a->in, a->n);
	return __real_xzk_encode_syms(a, nblocks, stream);
}

int __real_xzk_assemble(const xzamd_copy_seg *d_segs, uint32_t nsegs, const uint8_t *d_scratch, const uint8_t *d_lits, const uint8_t *d_in,
		uint8_t *d_out, void *stream);
int __wrap_xzk_assemble(const xzamd_copy_seg *d_segs, uint32_t nsegs, const uint8_t *d_scratch, const uint8_t *d_lits, const uint8_t *d_in,
		uint8_t *d_out, void *stream)
{
	LOG("gather %p %p %u", stream, (const void *)d_in, nsegs);
	return __real_xzk_assemble(d_segs, nsegs, d_scratch, d_lits, d_in, d_out, stream);
}

int __real_xzk_delta_stats(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t *d_hist, void *stream);
int __wrap_xzk_delta_stats(const uint8_t *d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t *d_hist, void *stream)
{
	LOG("delta_stats %p %p %u", stream, (const void *)d_in, n);
	return __real_xzk_delta_stats(d_in, n, block_size, nblocks, d_hist, stream);
}
int __real_xzk_delta_choose(const uint32_t *d_hist, uint32_t nblocks, uint32_t *d_dist, void *stream);
int __wrap_xzk_delta_choose(const uint32_t *d_hist, uint32_t nblocks, uint32_t *d_dist, void *stream)
{
	LOG("delta_choose %p %p %u", stream, (const void *)d_dist, nblocks);
	return __real_xzk_delta_choose(d_hist, nblocks, d_dist, stream);
}
/* (the filtered copy is what the build, the finder, the parse and the coder of the batch read: its pointer names the buffer) */
int __real_xzk_delta_blocks(const uint8_t *d_in, uint8_t *d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, const uint32_t *d_dist,
		void *stream);
int __wrap_xzk_delta_blocks(const uint8_t *d_in, uint8_t *d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, const uint32_t *d_dist,
		void *stream)
{
	LOG("delta_blocks %p %p %u", stream, (const void *)d_out, n);
	return __real_xzk_delta_blocks(d_in, d_out, n, block_size, nblocks, d_dist, stream);
}
