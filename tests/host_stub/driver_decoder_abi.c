/* driver_decoder_abi.c -- TEST INFRASTRUCTURE ONLY: a liblzma client of the decoder ABI (xzamd_decoder.c: lzma_stream_decoder,
 * lzma_stream_decoder_mt, lzma_stream_buffer_decode, lzma_get_check through lzma_code / lzma_end of xzamd_stream.c) over the CPU
 * stand-ins of the kernel layer.  A program of its own, so that it can be built with sanitizers and simply run
 * (tests/test_host_decoder_abi.py).
 * usage: driver_decoder_abi FILE.xz OUT IN_PIECE OUT_PIECE FLAGS MT
 *   feeds FILE.xz IN_PIECE bytes per lzma_code call (0: all at once) with OUT_PIECE bytes of room (0: all of it), LZMA_FINISH
 *   once the last byte is handed over; writes the decoded bytes to OUT and prints one line:
 *   ret=R total_in=N total_out=N notices=a,b,... checks=c,... buffer=R2/in_pos/out_pos */
#include "../../xz_amd/csrc/xzamd_internal.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver_decoder_abi: %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
#define OUT_CAP (8u << 20)

void stub_dec_enable(void);
void stub_dec_trace_reset(void);
void stub_dec_trace_free(void);

int main(int argc, char **argv)
{
	CHECK(argc == 7);
	FILE *f = fopen(argv[1], "rb");
	CHECK(f != NULL);
	uint8_t *big = (uint8_t *)malloc(OUT_CAP);
	CHECK(big != NULL);
	const size_t n = fread(big, 1, OUT_CAP, f);
	fclose(f);
	uint8_t *xz = (uint8_t *)malloc(n ? n : 1);             /* an allocation of exactly the file's size */
	CHECK(xz != NULL);
	memcpy(xz, big, n);
	const size_t in_piece = strtoull(argv[3], NULL, 10), out_piece = strtoull(argv[4], NULL, 10);
	const uint32_t flags = (uint32_t)strtoul(argv[5], NULL, 16);
	const int mt = atoi(argv[6]);
	stub_dec_enable();

	lzma_stream s = LZMA_STREAM_INIT;
	if (mt) {
		lzma_mt o;
		memset(&o, 0, sizeof(o));
		o.flags = flags; o.threads = 4; o.timeout = 300; o.memlimit_threading = UINT64_MAX; o.memlimit_stop = UINT64_MAX;
		CHECK(lzma_stream_decoder_mt(&s, &o) == LZMA_OK);
	} else {
		CHECK(lzma_stream_decoder(&s, UINT64_MAX, flags) == LZMA_OK);
	}
	char notices[256] = "", checks[256] = "";
	size_t fed = 0, done = 0;
	lzma_ret r;
	for (;;) {
		if (s.avail_in == 0 && fed < n) {
			const size_t k = in_piece && in_piece < n - fed ? in_piece : n - fed;
			s.next_in = xz + fed; s.avail_in = k;
			fed += k;
		}
		const size_t room = out_piece && out_piece < OUT_CAP - done ? out_piece : OUT_CAP - done;
		s.next_out = big + done; s.avail_out = room;
		stub_dec_trace_reset();
		r = lzma_code(&s, fed == n ? LZMA_FINISH : LZMA_RUN);
		done += room - s.avail_out;
		if (r == LZMA_NO_CHECK || r == LZMA_UNSUPPORTED_CHECK || r == LZMA_GET_CHECK) {
			/* a notice, or -- LZMA_UNSUPPORTED_CHECK only -- this coder's verdict on a Stream it cannot verify.  A verdict has
			 * latched: a call that offers neither input nor room and does not finish gets it again, where a coder that only
			 * gave notice has nothing to do and says LZMA_OK */
			if (r == LZMA_UNSUPPORTED_CHECK) {
				lzma_stream probe = s;
				probe.avail_in = 0; probe.avail_out = 0;
				const lzma_ret pr = lzma_code(&probe, LZMA_RUN);
				CHECK(pr == LZMA_OK || pr == LZMA_UNSUPPORTED_CHECK);
				CHECK(probe.total_in == s.total_in && probe.total_out == s.total_out && probe.internal == s.internal);
				if (pr == LZMA_UNSUPPORTED_CHECK) break;
			}
			CHECK(strlen(notices) + 8 < sizeof(notices));
			sprintf(notices + strlen(notices), "%s%d", notices[0] ? "," : "", (int)r);
			sprintf(checks + strlen(checks), "%s%d", checks[0] ? "," : "", (int)lzma_get_check(&s));
			continue;
		}
		if (r != LZMA_OK) break;
	}
	uint64_t pin = 0, pout = 0;
	lzma_get_progress(&s, &pin, &pout);
	CHECK(pin == s.total_in && pout == s.total_out && s.total_out == done);
	const lzma_ret again = lzma_code(&s, LZMA_FINISH);         /* the end and errors latch */
	CHECK(again == r || (r == LZMA_STREAM_END && again == LZMA_STREAM_END));
	f = fopen(argv[2], "wb");
	CHECK(f != NULL && fwrite(big, 1, done, f) == done);
	fclose(f);
	printf("ret=%d total_in=%llu total_out=%llu notices=%s checks=%s", (int)r, (unsigned long long)s.total_in,
			(unsigned long long)s.total_out, notices, checks);
	lzma_end(&s);
	CHECK(s.internal == NULL);

	/* the one-shot entry on the same file */
	uint64_t memlimit = UINT64_MAX;
	size_t in_pos = 0, out_pos = 0;
	stub_dec_trace_reset();
	const lzma_ret rb = lzma_stream_buffer_decode(&memlimit, flags & LZMA_CONCATENATED, NULL, xz, &in_pos, n, big, &out_pos, OUT_CAP);
	printf(" buffer=%d/%llu/%llu\n", (int)rb, (unsigned long long)in_pos, (unsigned long long)out_pos);
	/* declined at init */
	CHECK(lzma_stream_decoder(&s, UINT64_MAX, LZMA_IGNORE_CHECK) == LZMA_OPTIONS_ERROR && s.internal == NULL);
	CHECK(lzma_stream_decoder(&s, 0, 0) == LZMA_PROG_ERROR);
	xzamd_release_parked();
	stub_dec_trace_free();
	free(xz); free(big);
	return 0;
}
