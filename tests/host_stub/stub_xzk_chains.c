/* stub_xzk_chains.c -- TEST INFRASTRUCTURE ONLY: what the host code of the bare chunk chains (xz_amd/csrc/xzamd_chains.c) needs of
 * the kernel layer on top of stub_xzk.c and stub_xzk_dec.c, on the CPU (tests/test_host_chains.py, driven by driver_chains.c):
 *   xzk_dec_scan_chains      the bare-chain grammar in plain C -- a chain is exactly csize bytes, starts with a dictionary reset,
 *                            holds no 0x00 end marker and ends at c == csize with u == usize -- one unit per chain, like the scan
 *                            of stub_xzk_dec.c
 *   __wrap_xzk_dec_units     stub_xzk_dec.c decodes a Block's data with the oracle's decoder, which wants the end marker a chain
 *                            does not have: the program is linked with --wrap=xzk_dec_units, and this stand-in decodes every
 *                            chain from a copy with the 0x00 appended
 *   xzk_resume_void_blocks   nothing to do: no encode over the stubs keeps a resume table */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "../../xz_amd/csrc/kernels_api.h"
#include "../../oracle/oracle.h"
#include <stdlib.h>
#include <string.h>

int xzk_dec_scan_chains(const uint8_t *d_chains, xzamd_dec_block *d_blocks, uint32_t nchains, xzamd_dec_unit *d_units,
		uint32_t units_cap, int split, const uint8_t *d_rec, uint32_t rec_stride, uint32_t nrec, void *stream)
{
	(void)split; (void)d_rec; (void)rec_stride; (void)nrec; (void)stream;
	for (uint32_t b = 0; b < nchains; ++b) {
		xzamd_dec_block *B = &d_blocks[b];
		const uint8_t *p = d_chains + B->cpos;
		uint64_t c = 0, u = 0;
		uint32_t err = 0;
		int need_dict_reset = 1, need_props = 1;
		while (c < B->csize && !err) {
			const uint32_t ctl = p[c];
			uint64_t hs, cs, us;
			if (ctl == 0x00) { err = 6; break; }            /* no end marker inside a chain */
			if (ctl >= 0x80) {
				if (c + 5 > B->csize) { err = 5; break; }
				us = ((((uint64_t)ctl & 0x1F) << 16) | ((uint64_t)p[c + 1] << 8) | p[c + 2]) + 1;
				cs = (((uint64_t)p[c + 3] << 8) | p[c + 4]) + 1;
				hs = 5;
				if (ctl >= 0xE0) need_dict_reset = 0;
				if (need_dict_reset) { err = 2; break; }
				if (ctl >= 0xC0) {
					if (c + 6 > B->csize) { err = 5; break; }
					if (p[c + 5] > (4 * 5 + 4) * 9 + 8 || (p[c + 5] % 45u) / 9u + p[c + 5] % 9u > 4u) { err = 4; break; }
					hs = 6;
					need_props = 0;
				}
				if (need_props) { err = 3; break; }
			} else if (ctl == 0x01 || ctl == 0x02) {
				if (c + 3 > B->csize) { err = 5; break; }
				if (ctl == 0x01) { need_dict_reset = 0; need_props = 1; }
				if (need_dict_reset) { err = 2; break; }
				us = (((uint64_t)p[c + 1] << 8) | p[c + 2]) + 1;
				cs = us;
				hs = 3;
			} else { err = 1; break; }
			if (c + hs + cs > B->csize || u + us > B->usize) { err = 6; break; }
			c += hs + cs;
			u += us;
		}
		if (!err && (c != B->csize || u != B->usize)) err = 6;
		xzamd_dec_unit *U = &d_units[(uint64_t)b * units_cap];
		memset(U, 0, sizeof(*U));
		U->cpos = B->cpos; U->block = b; U->rec = XZAMD_RESUME_NONE;
		B->nunits = err ? 0 : 1; B->error = err; B->nrecs = 0;
	}
	return 0;
}

int __wrap_xzk_dec_units(const uint8_t *d_xz, const xzamd_dec_block *d_blocks, uint32_t nblocks, const xzamd_dec_unit *d_units,
		uint32_t units_cap, const uint32_t *d_unit_first, uint32_t total_units, uint8_t *d_out, const uint8_t *d_expected,
		uint16_t *d_lit_pool, uint32_t waves, uint32_t *d_counter, uint32_t *d_block_err, int per_unit,
		const uint8_t *d_rec, uint32_t rec_stride, void *stream)
{
	(void)d_units; (void)units_cap; (void)total_units; (void)d_expected; (void)d_lit_pool; (void)waves; (void)d_counter; (void)per_unit;
	(void)d_rec; (void)rec_stride; (void)stream;
	for (uint32_t b = 0; b < nblocks; ++b) {
		const xzamd_dec_block *B = &d_blocks[b];
		uint64_t got = 0;
		if (d_unit_first[b + 1] == d_unit_first[b]) continue;      /* taken out of the decode by the host */
		uint8_t *tmp = (uint8_t *)malloc(B->csize + 1);
		if (!tmp) return 2;
		memcpy(tmp, d_xz + B->cpos, B->csize);
		tmp[B->csize] = 0x00;
		if (orc_lzma2_decode(tmp, B->csize + 1, B->dict_size, d_out + B->upos, B->usize, &got, NULL) || got != B->usize)
			d_block_err[b] = 1;
		free(tmp);
	}
	return 0;
}

int xzk_resume_void_blocks(uint8_t *d_table, uint32_t rec_stride, uint32_t nrec, const uint8_t *d_bad, uint32_t nblocks, void *stream)
{
	(void)d_table; (void)rec_stride; (void)nrec; (void)d_bad; (void)nblocks; (void)stream;
	return 0;
}
