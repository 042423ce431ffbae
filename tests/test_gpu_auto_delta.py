"""Automatic per-Block delta filter on the device (XZAMD_F_AUTO_DELTA, DESIGN.md 3.5 "Automatic delta"): the histograms and
choices of the kernels against the numpy model of the rule (tests/_auto_delta.py) bit for bit, Streams whose Blocks carry
different chains through the reference decoder and the device decoders, no drift against the existing paths, the gain on
numeric classes, the combinations the flag declines, and XZAMD_AUTO_DELTA=1 through lzma_code."""
import lzma

import numpy as np
import pytest

import _auto_delta as ad
import _corpora as cp
import _filters as fl
import _oracle as o
import _single_block as sb

pytestmark = pytest.mark.gpu

OPTIONS_ERROR = 8
K = 1024


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    e = xz_amd.Encoder()
    yield e
    e.close()


def _text(n, seed=5):
    import xz_amd
    return xz_amd.corpus_text(n, seed=seed).tobytes()


def _rnd(n, s):
    return np.random.default_rng(s).integers(0, 256, n, dtype=np.uint8).tobytes()


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _chain(raw, off):
    """delta distance in the Block Header at `off` (0: the chain is {LZMA2})"""
    ff = fl.block_filter_flags(raw[off - 12:])
    assert ff[-1][0] == fl.LZMA2 and len(ff) <= 2
    if len(ff) == 1:
        return 0
    assert ff[0][0] == fl.DELTA and len(ff[0][1]) == 1
    return ff[0][1][0] + 1


# ---- (a) exactness ----
@pytest.mark.parametrize("case", ["one_byte", "one_block_4096", "three_blocks_and_a_byte", "mixed_batch"])
def test_choices_and_histograms_are_the_model(enc, case):
    if case == "one_byte":
        data, bs = b"\x5a", 4096
    elif case == "one_block_4096":
        data, bs = cp.int32_walk(4096), 4096
    elif case == "three_blocks_and_a_byte":
        data, bs = cp.int32_walk(3 * 69632 + 1), 69632
    else:
        data, bs = _text(65536) + cp.int32_walk(65536) + bytes(65536) + _rnd(65536, 3), 65536
    data = bytes(data)
    want, want_hist = ad.choose_blocks(data, bs)
    got = enc.choose_delta(_cuda(data), bs)
    hist, dist = enc.delta_histograms(len(want))
    print(case, "model", want, "device", got)
    assert got == want and dist.tolist() == want
    assert hist.dtype == want_hist.dtype and np.array_equal(hist, want_hist)
    if case == "mixed_batch":
        assert want == [0, 4, 0, 0]


# ---- (b) a Stream whose Blocks differ ----
_MIXED = None


def _mixed():
    global _MIXED
    if _MIXED is None:
        _MIXED = _text(256 * K) + bytes(cp.int32_walk(256 * K)) + bytes(cp.structs24(256 * K)) + _rnd(256 * K, 9)
    return _MIXED


@pytest.mark.parametrize("preset", [1, 6])
@pytest.mark.parametrize("check", [4, 10])
def test_mixed_stream(enc, preset, check):
    import xz_amd
    data = _mixed()
    d = _cuda(data)
    out, binfo = enc.encode(d, preset=preset, block_size=256 * K, check=check, auto_delta=True, verify=True)    # verified encode: passes
    raw = _bytes(out)
    assert [_chain(raw, b.out_offset) for b in binfo] == [0, 4, 24, 0]
    # the random Block goes out as uncompressed chunks (from the coder, or as a stored Block from the layout) and has no filter
    assert binfo[3].unpadded_size > 256 * K and raw[binfo[3].out_offset + (raw[binfo[3].out_offset] + 1) * 4] == 0x01
    rr, dec = o.ref_decode(raw, len(data) + 16)
    assert rr == 1 and dec == data
    assert lzma.decompress(raw, format=lzma.FORMAT_XZ) == data          # the system's liblzma: what `xz -d` runs
    _, blocks, usz = xz_amd.file_index(raw)
    assert usz == len(data) and [b["filter_ids"] for b in blocks] == [(0x21,), (3, 0x21), (3, 0x21), (0x21,)]
    x = _cuda(raw)
    assert _bytes(enc.decode(x, len(data))[0]) == data
    assert _bytes(enc.decode_file(x, len(data))[0]) == data
    fwd, rep = enc.decode_forward(x, len(data))
    assert _bytes(fwd) == data and rep["blocks_delivered"] == 4
    # without the verification, as bare Blocks: the same bytes without the framing
    out3, b3 = enc.encode(d, preset=preset, block_size=256 * K, check=check, auto_delta=True, blocks_only=True)
    assert _bytes(out3) == raw[12: 12 + out3.numel()] and [b.out_offset + 12 for b in b3] == [b.out_offset for b in binfo]


# ---- (c) no drift ----
def test_no_drift_against_the_existing_paths(enc):
    import xz_amd
    walk = bytes(cp.int32_walk(1 << 20))
    auto, _ = enc.encode(_cuda(walk), preset=6, block_size=256 * K, auto_delta=True)
    opts = xz_amd.preset_options(6)
    opts.bcj = xz_amd.filter_delta(4)
    named, _ = enc.encode(_cuda(walk), opts=opts, block_size=256 * K)
    assert _bytes(auto) == _bytes(named)
    text = _text(1 << 20)
    auto, _ = enc.encode(_cuda(text), preset=6, block_size=256 * K, auto_delta=True)
    plain, _ = enc.encode(_cuda(text), preset=6, block_size=256 * K)
    assert _bytes(auto) == _bytes(plain)
    # several batches in one call (pipelined back ends): the same Stream
    enc.set_batch_bytes(512 * K)
    try:
        auto2, _ = enc.encode(_cuda(walk), preset=6, block_size=256 * K, auto_delta=True)
        assert _bytes(auto2) == _bytes(named)
    finally:
        enc.set_batch_bytes((1 << 31) - (1 << 20))


# ---- (d) gain ----
@pytest.mark.parametrize("name,dist", [("pcm16", 4), ("structs24", 24), ("f64sine", 8), ("int32walk", 4)])
def test_gain_on_numeric_classes(enc, name, dist):
    """One Block of 1 MiB at preset 6: smaller than the plain Stream, and within the README's 1.025 x of the reference on the
    same chain {delta(dist), LZMA2}."""
    data = bytes(ad.CLASSES[name](1 << 20))
    auto, binfo = enc.encode(_cuda(data), preset=6, block_size=1 << 20, auto_delta=True)
    plain, _ = enc.encode(_cuda(data), preset=6, block_size=1 << 20)
    ref = o.ref_encode_mt_chain(data, 6, fl.DELTA, delta_dist=dist, block_size=1 << 20)
    raw = _bytes(auto)
    print(f"{name}: auto {len(raw)} plain {plain.numel()} ratio {len(raw) / plain.numel():.4f} | reference delta({dist}) {len(ref)} "
          f"ratio {len(raw) / len(ref):.4f}")
    assert _chain(raw, binfo[0].out_offset) == dist
    rr, dec = o.ref_decode(raw, len(data) + 16)
    assert rr == 1 and dec == data
    assert len(raw) < plain.numel()
    assert len(raw) <= 1.025 * len(ref)


# ---- (e) what the flag declines ----
def test_declined_combinations(enc):
    import xz_amd
    d = _cuda(_text(128 * K))
    for kw in (dict(flags=xz_amd.F_SEGMENTS), dict(single=True), dict(repair=True)):
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, preset=6, block_size=64 * K, auto_delta=True, **kw)
        assert ei.value.code == OPTIONS_ERROR and "auto delta" in str(ei.value), kw
    for bcj in (xz_amd.filter_delta(4), xz_amd.BCJ_X86):
        opts = xz_amd.preset_options(6)
        opts.bcj = bcj
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, opts=opts, block_size=64 * K, auto_delta=True)
        assert ei.value.code == OPTIONS_ERROR and "auto delta" in str(ei.value)
    # the context is still good
    out, _ = enc.encode(d, preset=6, block_size=64 * K, auto_delta=True, keep_resume=True)
    assert o.ref_decode(_bytes(out), 128 * K + 16) == (1, _text(128 * K))


# ---- (f) through lzma_code ----
def test_env_variable_through_lzma_code(enc, monkeypatch):
    import xz_amd
    data = bytes(cp.int32_walk(2 << 20))
    bs = 512 * K
    monkeypatch.setenv("XZAMD_AUTO_DELTA", "1")
    pieces, _ = sb.lzma_encode(data, 6, piece=8 * K, mt_block_size=bs)
    whole, _ = sb.lzma_encode(data, 6, mt_block_size=bs)
    assert pieces == whole
    _, blocks, usz = xz_amd.file_index(whole)
    assert usz == len(data) and len(blocks) == 4
    assert [_chain(whole, b["header_offset"]) for b in blocks] == [4, 4, 4, 4]
    rr, dec = o.ref_decode(whole, len(data) + 16)
    assert rr == 1 and dec == data
    # ignored, not an error, where the mode does not apply: with XZAMD_REPAIR=1 the jobs are repaired ones, every Block {LZMA2}
    monkeypatch.setenv("XZAMD_REPAIR", "1")
    rep, _ = sb.lzma_encode(data[:bs], 6, mt_block_size=bs)
    monkeypatch.delenv("XZAMD_REPAIR")
    assert [_chain(rep, b["header_offset"]) for b in xz_amd.file_index(rep)[1]] == [0]
    assert o.ref_decode(rep, bs + 16) == (1, data[:bs])
    monkeypatch.delenv("XZAMD_AUTO_DELTA")
    off, _ = sb.lzma_encode(data, 6, mt_block_size=bs)
    assert [_chain(off, b["header_offset"]) for b in xz_amd.file_index(off)[1]] == [0, 0, 0, 0]
    plain, _ = enc.encode(_cuda(data), preset=6, block_size=bs)
    assert off == _bytes(plain)
