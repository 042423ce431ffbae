"""The host side of the automatic per-Block BCJ filter (XZAMD_F_AUTO_BCJ; xz_amd/csrc/xzamd_host.c, DESIGN.md 3.5 "Automatic
BCJ") without a GPU: tests/host_stub/driver_auto_bcj.c over the CPU stand-ins of the kernel layer (stub_xzk.c and the others
as they are, stub_xzk_delta.c for the automatic delta, stub_xzk_autobcj.c for the three new entry points), built with
-fsanitize=address,undefined and run as a program.  It covers the per-Block header planning -- Blocks with no filter, a delta
filter and both BCJ filters in one job, a stored Block, XZAMD_F_BLOCKS_ONLY, several batches in one call -- the precedence of
the BCJ rule over the delta rule, the analysis entry point, the debug fetches and the combinations the flag declines.  The
Stream of a job with three kinds of Block Header (none, delta, x86) is written out and read here with Python's lzma."""
import lzma
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ("xzamd_host.c", "xzamd_frame.c", "xzamd_options.c", "xzamd_stream.c", "corpus.c", "xzamd_framing.c", "xzamd_decode.c", "xzamd_file.c",
        "xzamd_repair.c", "xzamd_repair_plan.c", "xzamd_chains.c")
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in CSRC] + \
      [os.path.join(ROOT, "tests", "host_stub", f) for f in ("stub_xzk.c", "stub_xzk_dec.c", "stub_xzk_chains.c", "stub_xzk_delta.c",
                                                             "stub_xzk_autobcj.c", "driver_auto_bcj.c")] + \
      [os.path.join(ROOT, "oracle", f) for f in ("lzma2_dec.c", "xz_container.c", "lzma_fast_enc.c")]


def test_auto_bcj_host_layer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "driver_auto_bcj")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *SRC, "-Wl,--wrap=xzk_dec_units",
                    "-Wl,--wrap=xzk_span_encode", "-lm", "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k in ("LD_PRELOAD", "XZAMD_BATCH_MIB", "XZAMD_AUTO_DELTA", "XZAMD_AUTO_BCJ", "XZAMD_NO_OVERLAP"):
        env.pop(k, None)
    raw_path = str(tmp_path / "input")
    p = subprocess.run([exe, raw_path], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "driver_auto_bcj: ok" in p.stdout, (p.stdout[-4000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
    with open(raw_path, "rb") as f:
        data = f.read()
    with open(raw_path + ".xz", "rb") as f:
        stream = f.read()
    assert len(data) == 4 * (128 << 10) + 40001
    assert lzma.decompress(stream, format=lzma.FORMAT_XZ) == data
