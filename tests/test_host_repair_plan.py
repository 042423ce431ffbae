"""The splice layout of the repair (xzamd_repair_plan_, xz_amd/csrc/xzamd_repair_plan.c) without a GPU: pure arithmetic
over xzamd_frame.c, driven by a stand-alone program (tests/repair_plan_driver.c) that is built with
-fsanitize=address,undefined and run as a program.  The driver covers: replacements larger and smaller than the
originals; the first, the last, adjacent and every Block replaced (coded and stored); 1, 3, 5, 127 and 128 Blocks (the
Index's record count grows a byte at 128) and Unpadded Sizes on either side of 16383 | 16384; Checks none, CRC64 and
SHA-256; with and without Index and Footer.  It asserts that the segment lists tile the rewritten tail without gap or
overlap, that every source range lies inside its source, that the Index and Footer are what xzamd_frame_index_footer
makes of the new records, and -- carrying the gather out on host buffers -- that every Block's new place holds the bytes
it should (kept: the old ones; coded: the scratch's; stored: header, chunks of the original, end marker, padding, Check)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in ("xzamd_repair_plan.c", "xzamd_frame.c")] + \
      [os.path.join(ROOT, "tests", "repair_plan_driver.c")]


def test_splice_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "repair_plan_driver")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "repair_plan_driver: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
