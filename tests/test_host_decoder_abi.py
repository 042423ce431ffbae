"""The liblzma decoder ABI (xzamd_decoder.c: lzma_stream_decoder, lzma_stream_decoder_mt, lzma_stream_buffer_decode,
lzma_get_check, driven through lzma_code / lzma_end) without a GPU: tests/host_stub/driver_decoder_abi.c is a liblzma client
over the CPU stand-ins of the kernel layer, built with -fsanitize=address,undefined and run as a program, once per case.

Feed and drain schedules (in, out): (1, 1) on a file below 2 KiB, (7, 4096), (4093, 65536), (all, all).  XZAMD_DEC_BATCH_KIB=96,
so that the 64 KiB Blocks, an Index, a Stream Header and Stream Padding of the larger file come to lie across batches.
Checked: the output, the final code, total_in and total_out, each LZMA_TELL_* notice once per Stream with lzma_get_check, and
the one-shot entry.  Where oracle/_ref is built, the same schedules go through the reference's liblzma: output bytes, final
code and final totals must be equal (the per-call sequence is not compared: this coder batches)."""
import os
import subprocess

import numpy as np
import pytest

import _forward as fw
import _oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ("xzamd_host.c", "xzamd_frame.c", "xzamd_options.c", "xzamd_stream.c", "corpus.c", "xzamd_framing.c", "xzamd_decode.c",
        "xzamd_file.c", "xzamd_forward.c", "xzamd_decoder.c")
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in CSRC] + \
      [os.path.join(ROOT, "tests", "host_stub", f) for f in ("stub_xzk.c", "stub_xzk_dec.c", "stub_xzk_walk.c", "driver_decoder_abi.c")] + \
      [os.path.join(ROOT, "oracle", f) for f in ("lzma2_dec.c", "xz_container.c")]
TELL = 0x01 | 0x04          # LZMA_TELL_NO_CHECK | LZMA_TELL_ANY_CHECK
CONCAT = 0x08
STREAM_END, BUF_ERROR, DATA_ERROR = 1, 10, 9


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("abi") / "driver_decoder_abi")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def files():
    """name -> (file bytes, decoded bytes, Streams as (Check, has Blocks))"""
    a, b, c = _rand(700, 1), _rand(5 * 65536 + 4097, 2), _rand(65536 + 1, 3)
    small = fw.stored_stream(a[:300], 128, check=1) + b"\0" * 4 + fw.stored_stream(a[300:], 400, check=0, sizes=False)
    assert len(small) < 2048
    large = fw.stored_stream(b, 65536, check=1) + b"\0" * 8 + fw.stored_stream(c, 1 << 20, check=0, sizes=False) \
        + fw.stored_stream(b"", 1, check=1) + b"\0" * 4
    return {"small": (small, a, [1, 0]), "large": (large, b + c, [1, 0, 1])}


def _run(exe, tmp_path, raw, in_piece, out_piece, flags, mt=0):
    src, dst = tmp_path / "in.xz", tmp_path / "out.bin"
    src.write_bytes(raw)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               XZAMD_DEC_BATCH_KIB="96")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe, str(src), str(dst), str(in_piece), str(out_piece), f"{flags:x}", str(mt)], capture_output=True,
                       text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
    f = dict(kv.split("=") for kv in p.stdout.split())
    ints = lambda s: [int(v) for v in s.split(",") if v]
    return dict(ret=int(f["ret"]), total_in=int(f["total_in"]), total_out=int(f["total_out"]), notices=ints(f["notices"]),
                checks=ints(f["checks"]), buffer=tuple(int(v) for v in f["buffer"].split("/")), out=dst.read_bytes())


SCHEDULES = [("small", 1, 1), ("small", 7, 4096), ("large", 7, 4096), ("large", 4093, 65536), ("large", 0, 0), ("small", 0, 0)]


# lzma_stream_decoder_mt is the same coder behind another init: two schedules of it
CASES = [(*sch, 0) for sch in SCHEDULES] + [("large", 4093, 65536, 1), ("large", 0, 0, 1), ("small", 0, 0, 1)]


@pytest.mark.parametrize("name,in_piece,out_piece,mt", CASES)
def test_schedules(exe, files, tmp_path, name, in_piece, out_piece, mt):
    raw, data, checks = files[name]
    got = _run(exe, tmp_path, raw, in_piece, out_piece, CONCAT | TELL, mt)
    assert got["ret"] == STREAM_END and got["out"] == data
    assert got["total_in"] == len(raw) and got["total_out"] == len(data)
    # once per Stream: LZMA_NO_CHECK (2) for Check none, LZMA_GET_CHECK (4) for any other
    assert got["notices"] == [2 if c == 0 else 4 for c in checks] and got["checks"] == checks
    assert got["buffer"] == (0, len(raw), len(data))
    if o.have_ref():
        notices = []
        r, ref, tin, tout = fw.stream_decode(fw.ref_lib(), raw, 8 << 20, CONCAT | TELL, in_piece or None, out_piece or None, notices,
                                             mt=bool(mt))
        assert (r, ref, tin, tout) == (got["ret"], got["out"], got["total_in"], got["total_out"])
        assert notices == got["notices"]




@pytest.mark.parametrize("in_piece,out_piece", [(7, 4096), (0, 0)])
def test_truncated_damaged_and_trailing_input(exe, files, tmp_path, in_piece, out_piece):
    raw, data, _ = files["large"]
    L = fw.ref_lib() if o.have_ref() else None
    # cut inside the last Block of the first Stream: the four whole Blocks, then LZMA_BUF_ERROR
    cut = 12 + 4 * (65536 + 24) + 1000
    got = _run(exe, tmp_path, raw[:cut], in_piece, out_piece, CONCAT)
    assert got["ret"] == BUF_ERROR and got["out"] == data[: 4 * 65536] and got["total_in"] == cut
    assert got["buffer"][0] == DATA_ERROR            # stream_buffer_decoder.c: input that ends early
    if L:
        r, ref, tin, _ = fw.stream_decode(L, raw[:cut], 8 << 20, CONCAT, in_piece or None, out_piece or None)
        assert r == BUF_ERROR and tin == cut and ref[: len(got["out"])] == got["out"]
    # a flipped payload byte in Block 2: Blocks 0 and 1, then LZMA_DATA_ERROR
    bad = bytearray(raw)
    bad[12 + 2 * (65536 + 24) + 5000] ^= 1
    got = _run(exe, tmp_path, bytes(bad), in_piece, out_piece, CONCAT)
    assert got["ret"] == DATA_ERROR and got["out"] == data[: 2 * 65536] and got["buffer"][0] == DATA_ERROR
    if L:
        r, ref, _, _ = fw.stream_decode(L, bytes(bad), 8 << 20, CONCAT, in_piece or None, out_piece or None)
        assert r == DATA_ERROR and ref[: len(got["out"])] == got["out"]
    # not an .xz file
    got = _run(exe, tmp_path, b"\xfd7zXY\0" + raw[6:], in_piece, out_piece, CONCAT)
    assert got["ret"] == 7 and got["out"] == b""
    if (in_piece, out_piece) == (0, 0):
        # without LZMA_CONCATENATED what follows the first Stream stays with the caller
        first = len(fw.stored_stream(data[: 5 * 65536 + 4097], 65536, check=1))
        got = _run(exe, tmp_path, raw, 0, 0, 0)
        assert got["ret"] == STREAM_END and got["out"] == data[: 5 * 65536 + 4097] and got["total_in"] == first
        assert got["buffer"] == (0, first, 5 * 65536 + 4097)
        if L:
            r, ref, tin, tout = fw.stream_decode(L, raw, 8 << 20, 0)
            assert (r, ref, tin, tout) == (got["ret"], got["out"], got["total_in"], got["total_out"])


UNSUPPORTED_CHECK = 3
TELL_UNSUPPORTED = 0x02     # LZMA_TELL_UNSUPPORTED_CHECK


@pytest.mark.parametrize("in_piece,out_piece", [(1, 1), (7, 4096), (0, 0)])
def test_tell_unsupported_check(exe, tmp_path, in_piece, out_piece):
    """A Stream whose Check (id 2) has no verifier, behind a Stream with CRC32.  With LZMA_TELL_UNSUPPORTED_CHECK the notice comes
    once, when that Stream's header is looked at, with lzma_get_check = 2 -- as from the reference.  Then this coder fails the
    Stream where it starts (documented: the reference decodes it unverified): LZMA_UNSUPPORTED_CHECK again, as its verdict,
    which latches (the driver calls once more), behind the bytes of the Stream in front."""
    a = _rand(900, 4)
    raw = fw.stored_stream(a[:500], 200, check=1) + b"\0" * 4 + fw.stored_stream(a[500:], 300, check=2)
    got = _run(exe, tmp_path, raw, in_piece, out_piece, CONCAT | TELL_UNSUPPORTED)
    assert got["notices"] == [UNSUPPORTED_CHECK] and got["checks"] == [2]
    assert got["ret"] == UNSUPPORTED_CHECK and got["out"] == a[:500] and got["total_out"] == 500
    assert got["buffer"][0] == UNSUPPORTED_CHECK
    # without the flag: no notice, the same verdict behind the same bytes
    quiet = _run(exe, tmp_path, raw, in_piece, out_piece, CONCAT)
    assert quiet["notices"] == [] and quiet["ret"] == UNSUPPORTED_CHECK and quiet["out"] == a[:500] and quiet["total_out"] == 500
    # the Stream alone: the notice is the first thing the client hears
    alone = _run(exe, tmp_path, fw.stored_stream(a[500:], 300, check=2), in_piece, out_piece, TELL_UNSUPPORTED | TELL)
    assert alone["notices"] == [UNSUPPORTED_CHECK] and alone["checks"] == [2] and alone["ret"] == UNSUPPORTED_CHECK and alone["out"] == b""
    if o.have_ref():
        notices = []
        r, ref, _, _ = fw.stream_decode(fw.ref_lib(), raw, 8 << 20, CONCAT | TELL_UNSUPPORTED, in_piece or None, out_piece or None, notices)
        assert notices == got["notices"] and r == STREAM_END and ref == a
