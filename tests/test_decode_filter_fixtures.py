"""The yardsticks of tests/test_gpu_decode_filters.py, checked without a GPU against the real liblzma (oracle/_ref):
the fixture files of tests/golden/ref_files_filters are what their names say, the numpy model of the delta filter is
the reference's delta filter, the hand-made Streams of the "declined" cases are refused by the reference for the
reason the test means (or, for a BCJ start offset, decoded: that one is this project's own limit), and the chunked
walk behind the RISC-V inverse kernel equals the reference's decoder."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import _filters as f
import _oracle as o


@pytest.fixture(scope="module", autouse=True)
def _need_ref():
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")


def test_fixture_files_are_what_their_names_say():
    files = sorted(glob.glob(os.path.join(f.FIX, "*.xz")))
    good = [p for p in files if os.path.basename(p).startswith("good-")]
    assert len(good) >= 5 and len(files) - len(good) >= 3
    for p in files:
        raw = open(p, "rb").read()
        assert len(raw) < (1 << 20)
        r, out = o.ref_decode(raw, 1 << 20)
        if os.path.basename(p).startswith("good-"):
            assert r == 1, (p, r)                         # LZMA_STREAM_END
            assert any(fid != f.LZMA2 for fid, _ in f.block_filter_flags(raw)), p      # a chain, not {LZMA2}
        else:
            assert r in (8, 9), (p, r)                    # LZMA_OPTIONS_ERROR / LZMA_DATA_ERROR


@pytest.mark.parametrize("dist", [1, 2, 3, 4, 7, 16, 64, 255, 256])
def test_numpy_delta_model_is_the_reference_delta_filter(dist):
    rng = np.random.default_rng(dist)
    for n in (1, dist - 1, dist, dist + 1, 1000, f.TILE + 1, 3 * f.TILE + 5):
        if n <= 0:
            continue
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        filtered = f.np_delta_forward(data, dist)
        assert filtered == f.ref_forward(data, [(f.DELTA, dist)]), (dist, n)
        assert f.np_delta_inverse(filtered, dist) == data, (dist, n)
        # and through whole Streams of the reference encoder and decoder
        xz = o.ref_encode_mt_chain(data, 1, f.DELTA, dist, threads=1, block_size=max(n // 2, 1))
        r, back = o.ref_decode(xz, n + 16)
        assert r == 1 and back == data, (dist, n)


def test_hand_made_streams_mean_what_the_gpu_test_says():
    data = o.corpus_x86(50000, 3)
    raw = o.ref_encode_mt_chain(data, 1, f.BCJ["x86"], 1, threads=1, block_size=1 << 20)
    check, flags, nf, payload, chk, usize = f.parse_single_block(raw)
    assert nf == 2 and flags[:2] == b"\x04\x00" and usize == len(data)
    lz2 = flags[2:]
    # the writer reproduces a Stream the reference decodes
    r, out = o.ref_decode(f.single_block_stream(check, flags, nf, payload, chk, usize), len(data) + 16)
    assert r == 1 and out == data
    r, out = o.ref_decode(f.single_block_stream(check, b"\x04\x04\0\0\0\0" + lz2, 2, payload, chk, usize), len(data) + 16)
    assert r == 1 and out == data                         # size-4 properties, offset 0
    # start offset 4: fine for the reference (it decodes other bytes, so the Check fails), declined by the device
    r, _ = o.ref_decode(f.single_block_stream(check, b"\x04\x04\x04\0\0\0" + lz2, 2, payload, chk, usize), len(data) + 16)
    assert r == 9
    for name, ff, n in (("id 0x0C", b"\x0c\x00" + lz2, 2), ("LZMA2 then delta", lz2 + b"\x03\x01\x00", 2),
                        ("delta props size 2", b"\x03\x02\x00\x00" + lz2, 2)):
        r, _ = o.ref_decode(f.single_block_stream(check, ff, n, payload, chk, usize), len(data) + 16)
        assert r == 8, (name, r)
    r, _ = o.ref_decode(f.single_block_stream(check, flags, nf, payload, chk, usize, header_pad=b"\0\0\0\x01"), len(data) + 16)
    assert r == 8                                         # non-zero header padding


# ---- RISC-V, decoder direction: restatement + chunk rule (what unf_riscv in lzma_decode.hip does) ----------------
from test_bcj_riscv_walk import _not_pair, _rd32, _special, _sync, riscv_like      # noqa: E402  (same tests decide the jumps)

M = 0xFFFFFFFF


def _unconvert(b, out, pos):
    b0 = b[pos]
    if b0 == 0xEF:
        b1 = b[pos + 1]
        if b1 & 0x0D:
            return 2
        b2, b3 = b[pos + 2], b[pos + 3]
        addr = ((((b1 & 0xF0) << 13) | (b2 << 9) | (b3 << 1)) - pos) & M
        out[pos + 1] = (b1 & 0x0F) | ((addr >> 8) & 0xF0)
        out[pos + 2] = ((addr >> 16) & 0x0F) | ((addr >> 7) & 0x10) | ((addr << 4) & 0xE0)
        out[pos + 3] = ((addr >> 4) & 0x7F) | ((addr >> 13) & 0x80)
        return 4
    if (b0 & 0x7F) != 0x17:
        return 2
    inst = _rd32(b, pos)
    if inst & 0xE80:
        inst2 = _rd32(b, pos + 4)
        if _not_pair(inst, inst2):
            return 6
        addr = ((inst & 0xFFFFF000) + (inst2 >> 20)) & M
        inst = (0x17 | (2 << 7) | (inst2 << 12)) & M
        inst2 = addr
    else:
        if not _special(inst):
            return 4
        rs1 = inst >> 27
        addr = (int.from_bytes(bytes(b[pos + 4:pos + 8]), "big") - pos) & M
        inst2 = ((inst >> 12) | (addr << 20)) & M
        inst = (0x17 | (rs1 << 7) | ((addr + 0x800) & 0xFFFFF000)) & M
    out[pos:pos + 4] = list(inst.to_bytes(4, "little"))
    out[pos + 4:pos + 8] = list(inst2.to_bytes(4, "little"))
    return 8


def chunked_unwalk(data, chunk):
    b, out = list(data), list(data)
    if len(b) < 8:
        return bytes(out)
    limit = len(b) - 8
    for k in range((len(b) + chunk - 1) // chunk):
        s = k * chunk
        if s > limit:
            continue
        e = s + chunk
        pos = 0
        if k:
            q = s
            while q <= limit and q < e and not _sync(b, q, limit):
                q += 2
            if not (q <= limit and q < e):
                continue
            pos = q
        while pos <= limit:
            if pos >= e and _sync(b, pos, limit):
                break
            pos += _unconvert(b, out, pos)
    return bytes(out)


@pytest.mark.parametrize("n", [0, 5, 8, 9, 17, 100, 1000, 4097, 12000])
def test_riscv_decoder_walk_in_chunks_equals_the_reference(n):
    lib = C.CDLL(os.path.join(o.ORACLE_DIR, "_ref", "liblzma_ref.so"))
    for fn in (lib.lzma_bcj_riscv_decode, lib.lzma_bcj_riscv_encode):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_uint32, C.c_char_p, C.c_size_t]

    def run(fn, data):
        buf = C.create_string_buffer(bytes(data), max(len(data), 1))
        fn(0, buf, len(data))
        return buf.raw[:len(data)]
    changed = 0
    for seed in range(3):
        plain = riscv_like(n, 100 * n + seed)
        for data in (plain, run(lib.lzma_bcj_riscv_encode, plain)):       # arbitrary bytes and real encoder output
            want = run(lib.lzma_bcj_riscv_decode, data)
            changed += sum(x != y for x, y in zip(data, want))
            for chunk in (16, 64, 2048):
                assert chunked_unwalk(data, chunk) == want, (n, seed, chunk)
    if n >= 1000:
        assert changed > n // 20
