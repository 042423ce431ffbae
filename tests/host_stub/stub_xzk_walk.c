/* stub_xzk_walk.c -- TEST INFRASTRUCTURE ONLY: the forward walk of the kernels_api.h layer on the CPU (next to stub_xzk.c and
 * stub_xzk_dec.c), so that the forward reader (xzamd_forward.c) runs without a GPU and under sanitizers
 * (tests/test_host_forward.py, driven by driver_forward.c).  The walk is xzw_walk (xzamd_walk_parse.h), the text the device
 * compiles too; "device" memory is host memory.  Counts its calls. */
#include "../../xz_amd/csrc/kernels_api.h"
#include "../../xz_amd/csrc/xzamd_walk_parse.h"

static uint64_t g_walks;
uint64_t stub_walk_calls(void) { return g_walks; }

int xzk_dec_walk(const uint8_t *d_xz, uint64_t size, uint64_t pos0, uint32_t csz, uint64_t upos0, xzamd_hdr_rec *d_rows, uint32_t cap,
		xzamd_walk_result *d_res, void *stream)
{
	(void)stream;
	if (!d_xz || !d_rows || !d_res || cap == 0 || pos0 > size) return 1;
	++g_walks;
	xzw_walk(d_xz, size, pos0, csz, upos0, d_rows, cap, d_res);
	return 0;
}
