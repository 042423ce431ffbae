"""The host code of the device decoder (xzamd_decode.c, xzamd_file.c: container framing, Block tables, the staging of a
run, the per-Block verdicts) without a GPU: a characterisation test.

tests/host_stub/driver_decode.c drives every decoder entry point over the CPU stand-ins of the kernel layer
(tests/host_stub/stub_xzk.c + stub_xzk_dec.c: the Block Header kernel is xzb_block, the LZMA2 decode is the oracle's) and
prints, one line per case, return codes, Block counts, per-Block steps, report fields and an id of the trace of the
kernel-layer calls with their scalar arguments (each distinct trace once, at the end; the format is described in the driver).  The program is built with -fsanitize=address,undefined and run as a program; its output must equal
tests/golden/decode_host_trace.txt.  The cases: every reference fixture; Streams of 0 / 1 / 3 / 130 stored Blocks of 1 / 4096 /
4097 bytes with every Check; two and three Streams with Stream Padding 0 / 4 / 8; every single-byte flip (two masks, with and
without the enclosing CRC32 recomputed) of the Stream Header, Stream Footer, Index and one Block Header of a 3-Block Stream
through three entries; verification against right, flipped and short originals, flipped payload, chunk control byte and
stored Check; a forced overflow of the unit table; Blocks of no bytes; ranges.  A change of the host code that moves the
golden file changes behaviour: re-record it (driver_decode `ls tests/golden/ref_files*/*.xz | sort`) only when that is the
intent, and say so."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ("xzamd_host.c", "xzamd_frame.c", "xzamd_options.c", "xzamd_stream.c", "corpus.c", "xzamd_framing.c", "xzamd_decode.c", "xzamd_file.c")
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in CSRC] + \
      [os.path.join(ROOT, "tests", "host_stub", f) for f in ("stub_xzk.c", "stub_xzk_dec.c", "driver_decode.c")] + \
      [os.path.join(ROOT, "oracle", f) for f in ("lzma2_dec.c", "xz_container.c")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "decode_host_trace.txt")


def test_decoder_host_trace_under_sanitizers(tmp_path):
    exe = str(tmp_path / "driver_decode")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *SRC, "-o", exe], check=True)
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_files*", "*.xz")),
                   key=lambda p: os.path.relpath(p, ROOT))
    assert files
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe, *files], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "driver_decode: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
    want = open(GOLDEN).read()
    if p.stdout != want:
        got_l, want_l = p.stdout.splitlines(), want.splitlines()
        i = next((k for k, (a, b) in enumerate(zip(got_l, want_l)) if a != b), min(len(got_l), len(want_l)))
        raise AssertionError(f"output differs from {os.path.basename(GOLDEN)} at line {i + 1}:\n"
                             f"got:  {got_l[i - 3:i + 4]}\nwant: {want_l[i - 3:i + 4]}")
