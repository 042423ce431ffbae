"""The liblzma decoder ABI on the device: lzma_stream_decoder / lzma_stream_decoder_mt / lzma_stream_buffer_decode of
libxz_amd.so by ctypes, on the feed and drain schedules of test_host_decoder_abi.py and with two batch sizes -- the output is
the original, and output, final code and totals are those of the real liblzma (oracle/_ref) on the same schedule."""
import ctypes as C
import os
import subprocess

import pytest

import _forward as fw
import _oracle as o

pytestmark = pytest.mark.gpu

BS = 65536
CONCAT, TELL = 0x08, 0x01 | 0x04
STREAM_END, DATA_ERROR, BUF_ERROR = 1, 9, 10


@pytest.fixture(scope="module")
def libs():
    import xz_amd
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    xz_amd.lib()                                 # (loads torch's HIP runtime first)
    ours = fw.bind(C.CDLL(xz_amd.LIB_PATH))      # a handle of its own: the argument types set here stay out of xz_amd.lib()
    ours.lzma_stream_buffer_decode.restype = C.c_int
    ours.lzma_stream_buffer_decode.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t),
                                               C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t]
    return ours, fw.ref_lib()


@pytest.fixture(scope="module")
def inputs():
    """name -> (file, data): a file of three Streams (the reference's encoder at preset 1, 64 KiB Blocks, Checks CRC64 / none /
    CRC32, Stream Padding 8 and 4) and one below 2 KiB"""
    import torch
    import xz_amd
    a, b, c = o.corpus_mixed(5 * BS + 4097, 81), o.corpus_mixed(BS + 1, 82), o.corpus_lorem(3000)
    enc = xz_amd.Encoder()
    own, _ = enc.encode(torch.frombuffer(bytearray(c), dtype=torch.uint8).cuda(), preset=1, block_size=BS, check=1)
    own = own.cpu().numpy().tobytes()
    enc.close()
    large = o.ref_encode_mt(a, 1, block_size=BS) + b"\0" * 8 + o.ref_encode_mt(b, 0, block_size=BS, check=0) + own + b"\0" * 4
    small = o.ref_encode_mt(c[:900], 1, block_size=512, check=1) + b"\0" * 4 + o.ref_encode_mt(c[900:1500], 1, check=0)
    assert len(small) < 2048
    return {"large": (large, a + b + c, [4, 0, 1]), "small": (small, c[:1500], [1, 0])}


SCHEDULES = [("small", 1, 1), ("small", 7, 4096), ("large", 7, 4096), ("large", 4093, 65536), ("large", None, None)]


@pytest.mark.parametrize("batch_kib", [96, 1024])
@pytest.mark.parametrize("name,in_piece,out_piece", SCHEDULES)
def test_schedules_equal_the_reference(libs, inputs, monkeypatch, name, in_piece, out_piece, batch_kib):
    ours, ref = libs
    raw, data, checks = inputs[name]
    monkeypatch.setenv("XZAMD_DEC_BATCH_KIB", str(batch_kib))
    n1, n2 = [], []
    got = fw.stream_decode(ours, raw, len(data) + 4096, CONCAT | TELL, in_piece, out_piece, n1)
    want = fw.stream_decode(ref, raw, len(data) + 4096, CONCAT | TELL, in_piece, out_piece, n2)
    assert got[0] == STREAM_END and got[1] == data and got[2:] == (len(raw), len(data))
    assert got == want
    assert n1 == n2 == [2 if c == 0 else 4 for c in checks]


@pytest.mark.parametrize("in_piece,out_piece", [(7, 4096), (None, None)])
def test_tell_unsupported_check(libs, monkeypatch, in_piece, out_piece):
    """A Stream whose Check (id 2) has no verifier behind a Stream of the reference's encoder: with LZMA_TELL_UNSUPPORTED_CHECK the
    notice comes once, with lzma_get_check = 2, as from the reference; then this coder's verdict on that Stream (the reference
    decodes it unverified), which latches, behind the bytes of the Stream in front."""
    ours, ref = libs
    monkeypatch.setenv("XZAMD_DEC_BATCH_KIB", "96")
    a, b = o.corpus_mixed(BS + 5, 83), o.corpus_lorem(900)
    raw = o.ref_encode_mt(a, 1, block_size=BS, check=1) + b"\0" * 4 + fw.stored_stream(b, 300, check=2)
    n1, n2, c1, c2 = [], [], [], []
    got = fw.stream_decode(ours, raw, len(a) + 4096, CONCAT | 0x02, in_piece, out_piece, n1, checks_out=c1)
    want = fw.stream_decode(ref, raw, len(a) + 4096, CONCAT | 0x02, in_piece, out_piece, n2, checks_out=c2)
    assert n1 == n2 == [3] and c1 == c2 == [2]
    assert want[0] == STREAM_END and want[1] == a + b
    assert got[0] == 3 and got[1] == a and got[3] == len(a)
    # without the flag: no notice from either; the verdict is the first and only LZMA_UNSUPPORTED_CHECK
    n1 = []
    got = fw.stream_decode(ours, raw, len(a) + 4096, CONCAT, in_piece, out_piece, n1)
    assert got[0] == 3 and got[1] == a and n1 == [3]        # (the helper lists the first answer; the second one ends its run)


def test_decoder_mt_truncation_and_damage(libs, inputs, monkeypatch):
    ours, ref = libs
    raw, data, _ = inputs["large"]
    monkeypatch.setenv("XZAMD_DEC_BATCH_KIB", "96")
    got = fw.stream_decode(ours, raw, len(data) + 4096, CONCAT, 4093, 65536, mt=True)
    assert got == fw.stream_decode(ref, raw, len(data) + 4096, CONCAT, 4093, 65536, mt=True) and got[1] == data
    # truncated: LZMA_BUF_ERROR behind the whole Blocks; the reference hands out the bytes of the partial Block as well
    cut = len(raw) // 3
    got = fw.stream_decode(ours, raw[:cut], len(data) + 4096, CONCAT, 4093, 65536)
    want = fw.stream_decode(ref, raw[:cut], len(data) + 4096, CONCAT, 4093, 65536)
    assert got[0] == want[0] == BUF_ERROR and got[2] == want[2] == cut
    assert len(got[1]) % BS == 0 and len(want[1]) - BS < len(got[1]) <= len(want[1]) and want[1][: len(got[1])] == got[1]
    # damaged: the reference's code behind the Blocks in front of the damage
    bad = bytearray(raw)
    bad[cut] ^= 0x40
    got = fw.stream_decode(ours, bytes(bad), len(data) + 4096, CONCAT, None, None)
    want = fw.stream_decode(ref, bytes(bad), len(data) + 4096, CONCAT, None, None)
    assert got[0] == want[0] == DATA_ERROR and len(got[1]) % BS == 0 and want[1][: len(got[1])] == got[1]
    assert len(got[1]) >= len(want[1]) - BS


def test_buffer_decode(libs, inputs):
    ours, ref = libs
    raw, data, _ = inputs["large"]
    for L in (ours, ref):
        out = C.create_string_buffer(len(data) + 16)
        memlimit, ipos, opos = C.c_uint64((1 << 64) - 1), C.c_size_t(0), C.c_size_t(0)
        r = L.lzma_stream_buffer_decode(C.byref(memlimit), CONCAT, None, raw, C.byref(ipos), len(raw), out, C.byref(opos), len(data) + 16)
        assert (r, ipos.value, opos.value) == (0, len(raw), len(data)) and out.raw[: len(data)] == data


def test_symbol_versions():
    import xz_amd
    syms = subprocess.run(["nm", "-D", xz_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for want in ("lzma_stream_decoder@@XZ_5.0", "lzma_stream_buffer_decode@@XZ_5.0", "lzma_get_check@@XZ_5.0", "lzma_stream_decoder_mt@@XZ_5.4"):
        assert want in syms, want
