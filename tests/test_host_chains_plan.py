"""The splice layout of a chain repair (xzamd_chains_plan_, xz_amd/csrc/xzamd_repair_plan.c) without a GPU: pure
arithmetic, driven by a stand-alone program (tests/chains_plan_driver.c) that is built with -fsanitize=address,undefined
and run as a program.  The segments of a single-Block Stream are bare LZMA2 chunk chains that lie back to back, so a
replaced chain shifts every chain behind it and nothing else is written.  The driver covers: the first, a middle and
the last segment replaced; coded replacements shorter and longer than the old chain, and the stored chain; adjacent
replaced segments of both kinds; a single segment; a segment of 1 byte (kept, coded, stored).  For each case it checks
the new offsets and sizes, that the segment list covers the rewritten tail exactly once with every source range inside
its source, and -- carrying the gather out on host buffers -- that every chain's new place holds the bytes it should."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in ("xzamd_repair_plan.c", "xzamd_frame.c")] + \
      [os.path.join(ROOT, "tests", "chains_plan_driver.c")]


def test_chain_splice_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chains_plan_driver")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "chains_plan_driver: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
