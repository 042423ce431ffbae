"""The forward reader of the device decoder (xzamd_forward.c: an .xz file read from its front, without its Index) without a
GPU.

tests/host_stub/driver_forward.c drives it over the CPU stand-ins of the kernel layer -- the walk is xzw_walk
(xzamd_walk_parse.h), the text k_dec_walk compiles too; the Block Header kernel is xzb_block, the LZMA2 decode is the oracle's
-- in a program built with -fsanitize=address,undefined and run as a program.  The cases and what is asserted of them:
every reference fixture, Streams of 0 / 1 / 3 / 130 stored Blocks of 1 / 4096 / 4097 bytes with and without the sizes in the
Block Header and with every Check, two Streams with Stream Padding 0 / 4 / 8 -- an intact file gives the bytes and the Block
count xzamd_file_decode_device gives over the same stubs, with one walk launch per Stream; every prefix of a 3-Block Stream
gives exactly the Blocks that lie wholly inside it, with XZAMD_BUF_ERROR (a cut inside the first Stream Header: nothing);
every single-byte flip of its Index and Footer delivers the three Blocks and then the reference's code; a walk table of 2
rows over 5 Blocks launches three times; the step fed in buffers of 1, 13 and 4099 bytes gives the same bytes."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ("xzamd_host.c", "xzamd_frame.c", "xzamd_options.c", "xzamd_stream.c", "corpus.c", "xzamd_framing.c", "xzamd_decode.c",
        "xzamd_file.c", "xzamd_forward.c")
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in CSRC] + \
      [os.path.join(ROOT, "tests", "host_stub", f) for f in ("stub_xzk.c", "stub_xzk_dec.c", "stub_xzk_walk.c", "driver_forward.c")] + \
      [os.path.join(ROOT, "oracle", f) for f in ("lzma2_dec.c", "xz_container.c")]


def test_forward_reader_under_sanitizers(tmp_path):
    exe = str(tmp_path / "driver_forward")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *SRC, "-o", exe], check=True)
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_files*", "*.xz")),
                   key=lambda p: os.path.relpath(p, ROOT))
    assert files
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe, *files], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "driver_forward: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
    # every fixture was looked at, and at least 15 good-* files decoded in full
    lines = [l for l in p.stdout.splitlines() if ": backward " in l]
    assert len(lines) == len(files)
    assert sum(1 for l in lines if l.startswith(("ref_files/good-", "ref_files_concat/good-", "ref_files_filters/good-"))
               and "forward 0 " in l) >= 15, p.stdout[:4000]
