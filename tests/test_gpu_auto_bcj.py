"""Automatic per-Block BCJ filter on the device (XZAMD_F_AUTO_BCJ, DESIGN.md 3.5 "Automatic BCJ"): the histograms, site counts
and choices of the kernels against the numpy model of the rule (tests/_auto_bcj.py) bit for bit; byte identity with the
fixed chains {x86, LZMA2} / {ARM64, LZMA2} / {LZMA2}, Stream-wide where every Block chooses the same and Block by Block on mixed
input; independence of the batch size; the decoders; precedence over the automatic delta; the size on real code; the combinations the flag declines; and
XZAMD_AUTO_BCJ=1 through lzma_code."""
import lzma

import numpy as np
import pytest

import _auto_bcj as ab
import _corpora as cp
import _filters as fl
import _oracle as o
import _single_block as sb

pytestmark = pytest.mark.gpu

OPTIONS_ERROR = 8
K = 1024
X86, ARM64 = 4, 0x0A


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    e = xz_amd.Encoder()
    yield e
    e.close()


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _fixed(enc, d, kind, **kw):
    """(Stream, block infos) of the fixed chain {kind, LZMA2}, kind 0: {LZMA2}"""
    import xz_amd
    opts = xz_amd.preset_options(kw.pop("preset"))
    opts.bcj = kind
    out, binfo = enc.encode(d, opts=opts, **kw)
    return _bytes(out), binfo


def _chain(raw, off):
    """BCJ filter id in the Block Header at `off` (0: the chain is {LZMA2})"""
    ff = fl.block_filter_flags(raw[off - 12:])
    assert ff[-1][0] == fl.LZMA2 and len(ff) <= 2
    if len(ff) == 1:
        return 0
    assert ff[0][1] == b""
    return ff[0][0]


_MIX = None


def _mix():
    """1 MiB: synth_x86 | text | synth_arm64 | random, 256 KiB each"""
    global _MIX
    if _MIX is None:
        _MIX = ab.synth_x86(256 * K, 11) + ab.text(256 * K) + ab.synth_arm64(256 * K, 12) + ab.rnd(256 * K, 13)
    return _MIX


# ---- model agreement ----
@pytest.mark.parametrize("bs", [64 * K, 65537, 200001])
def test_choices_and_histograms_are_the_model(enc, bs):
    data = _mix()
    want, want_hist, want_n = ab.choose_blocks(data, bs)
    got = enc.choose_bcj(_cuda(data), bs)
    hist, ns, kind = enc.bcj_histograms(len(want))
    print("Block size", bs, "model", want, "device", got)
    # (at 200001 bytes the ARM64 code starts 2 mod 4 into its Blocks: no BL is on the Block's grid, and none is chosen)
    assert {X86, 0} <= set(want) and (ARM64 in want) == (bs != 200001)
    assert got == want and kind.tolist() == want
    assert np.array_equal(ns, want_n)
    assert hist.dtype == want_hist.dtype and np.array_equal(hist, want_hist)


# ---- byte identity where every Block chooses the same ----
@pytest.mark.parametrize("preset", [1, 6])
@pytest.mark.parametrize("kind", [X86, ARM64])
def test_uniform_input_is_the_fixed_chain(enc, kind, preset):
    data = ab.synth_x86(1 << 20, 21) if kind == X86 else ab.synth_arm64(1 << 20, 22)
    d = _cuda(data)
    assert enc.choose_bcj(d, 256 * K) == [kind] * 4
    auto, _ = enc.encode(d, preset=preset, block_size=256 * K, auto_bcj=True)
    named, _ = _fixed(enc, d, kind, preset=preset, block_size=256 * K)
    assert _bytes(auto) == named


@pytest.mark.parametrize("what", ["text", "random"])
def test_refused_input_is_the_plain_stream(enc, what):
    data = ab.text(1 << 20) if what == "text" else ab.rnd(1 << 20, 23)
    d = _cuda(data)
    auto, _ = enc.encode(d, preset=6, block_size=256 * K, auto_bcj=True)
    plain, _ = enc.encode(d, preset=6, block_size=256 * K)
    assert _bytes(auto) == _bytes(plain)


# ---- a Stream whose Blocks differ ----
_MIXED = {}


def _mixed(enc, preset):
    """(data, Block size, Stream of encode(auto_bcj, verify), its block infos, the model's choices) on 256 KiB: synth_x86 |
    text | synth_arm64 | random in Blocks of 64 KiB; encoded once per preset"""
    if preset not in _MIXED:
        bs = 64 * K
        data = ab.synth_x86(bs, 11) + ab.text(bs) + ab.synth_arm64(bs, 12) + ab.rnd(bs, 13)
        want = ab.choose_blocks(data, bs)[0]
        assert want == [X86, 0, ARM64, 0]
        out, binfo = enc.encode(_cuda(data), preset=preset, block_size=bs, auto_bcj=True, verify=True)    # verified encode: passes
        _MIXED[preset] = (data, bs, _bytes(out), binfo, want)
    return _MIXED[preset]


@pytest.mark.parametrize("preset", [1, 6])
def test_mixed_stream_blocks_are_the_fixed_chains(enc, preset):
    data, bs, raw, binfo, want = _mixed(enc, preset)
    d = _cuda(data)
    assert [_chain(raw, b.out_offset) for b in binfo] == want
    # every Block (header, payload, Check) is the Block at the same index of the fixed-chain Stream of its kind
    fixed = {k: _fixed(enc, d, k, preset=preset, block_size=bs) for k in (0, X86, ARM64)}
    for i, (b, k) in enumerate(zip(binfo, want)):
        fraw, fb = fixed[k]
        assert b.total_size == fb[i].total_size and b.unpadded_size == fb[i].unpadded_size, (i, k)
        assert raw[b.out_offset: b.out_offset + b.total_size] == fraw[fb[i].out_offset: fb[i].out_offset + fb[i].total_size], (i, k)


@pytest.mark.parametrize("preset", [1, 6])
def test_mixed_stream_does_not_depend_on_the_batch(enc, preset):
    data, bs, raw, binfo, _ = _mixed(enc, preset)
    d = _cuda(data)
    for batch in (bs, 2 * bs):
        enc.set_batch_bytes(batch)
        try:
            again, _ = enc.encode(d, preset=preset, block_size=bs, auto_bcj=True)
        finally:
            enc.set_batch_bytes((1 << 31) - (1 << 20))
        assert _bytes(again) == raw, batch
    bare, b3 = enc.encode(d, preset=preset, block_size=bs, auto_bcj=True, blocks_only=True)
    assert _bytes(bare) == raw[12: 12 + bare.numel()] and [b.out_offset + 12 for b in b3] == [b.out_offset for b in binfo]


def test_mixed_stream_decodes(enc):
    """The reference decoder (ARM64 is in the Stream, which the system's liblzma may not know: Python's lzma reads the mixed
    Streams without ARM64 in test_bcj_goes_before_delta and test_env_variable_through_lzma_code) and the device decoders."""
    import xz_amd
    data, _, raw, _, _ = _mixed(enc, 6)
    rr, dec = o.ref_decode(raw, len(data) + 16)
    assert rr == 1 and dec == data
    _, blocks, usz = xz_amd.file_index(raw)
    assert usz == len(data) and [b["filter_ids"] for b in blocks] == [(X86, 0x21), (0x21,), (ARM64, 0x21), (0x21,)]
    x = _cuda(raw)
    assert _bytes(enc.decode(x, len(data))[0]) == data
    assert _bytes(enc.decode_file(x, len(data))[0]) == data
    fwd, rep = enc.decode_forward(x, len(data))
    assert _bytes(fwd) == data and rep["blocks_delivered"] == 4


# ---- with the automatic delta ----
def test_bcj_goes_before_delta(enc):
    """pcm16 | synth_x86 | text: delta, x86 and none, in that order"""
    bs = 64 * K
    data = bytes(cp.NUMERIC_CLASSES["pcm16"](bs)) + ab.synth_x86(bs, 31) + ab.text(bs)
    d = _cuda(data)
    dist = enc.choose_delta(d, bs)
    assert dist[0] == 4 and dist[2] == 0                 # (whatever the delta rule says of the code Block, the BCJ rule goes first)
    assert enc.choose_bcj(d, bs) == [0, X86, 0]
    out, binfo = enc.encode(d, preset=6, block_size=bs, auto_bcj=True, auto_delta=True, verify=True)
    raw = _bytes(out)
    chains = [fl.block_filter_flags(raw[b.out_offset - 12:]) for b in binfo]
    assert [[f[0] for f in c] for c in chains] == [[fl.DELTA, fl.LZMA2], [X86, fl.LZMA2], [fl.LZMA2]]
    assert chains[0][0][1] == bytes([3])                 # delta distance 4
    assert lzma.decompress(raw, format=lzma.FORMAT_XZ) == data
    # Block by Block the Streams of the single analyses: delta alone for Block 0, BCJ alone for Blocks 1 and 2
    da, dinfo = enc.encode(d, preset=6, block_size=bs, auto_delta=True)
    ba, binfo2 = enc.encode(d, preset=6, block_size=bs, auto_bcj=True)
    da, ba = _bytes(da), _bytes(ba)
    for i, (src, info) in enumerate(((da, dinfo), (ba, binfo2), (ba, binfo2))):
        b, s = binfo[i], info[i]
        assert raw[b.out_offset: b.out_offset + b.total_size] == src[s.out_offset: s.out_offset + s.total_size], i
    assert _bytes(enc.decode(_cuda(raw), len(data))[0]) == data


# ---- size on real code ----
def test_size_on_real_code(enc):
    """No fixed percentage is asserted: the measured gain is in DESIGN.md section 5."""
    data = ab.x86_code(1 << 20)
    d = _cuda(data)
    auto, binfo = enc.encode(d, preset=6, block_size=1 << 20, auto_bcj=True)
    plain, _ = enc.encode(d, preset=6, block_size=1 << 20)
    raw = _bytes(auto)
    kind = _chain(raw, binfo[0].out_offset)
    print(f"x86_code: chain {kind}, auto {len(raw)} plain {plain.numel()} ratio {len(raw) / plain.numel():.4f}")
    assert kind == ab.choose(data)[0]
    assert len(raw) <= plain.numel()
    assert lzma.decompress(raw, format=lzma.FORMAT_XZ) == data


# ---- what the flag declines ----
def test_declined_combinations(enc):
    import xz_amd
    d = _cuda(ab.text(128 * K))
    for kw in (dict(flags=xz_amd.F_SEGMENTS), dict(single=True), dict(repair=True)):
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, preset=6, block_size=64 * K, auto_bcj=True, **kw)
        assert ei.value.code == OPTIONS_ERROR and "auto bcj" in str(ei.value), kw
    for bcj in (xz_amd.filter_delta(4), xz_amd.BCJ_X86):
        opts = xz_amd.preset_options(6)
        opts.bcj = bcj
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, opts=opts, block_size=64 * K, auto_bcj=True)
        assert ei.value.code == OPTIONS_ERROR and "auto bcj" in str(ei.value)
    # the context is still good
    out, _ = enc.encode(d, preset=6, block_size=64 * K, auto_bcj=True, keep_resume=True)
    assert lzma.decompress(_bytes(out), format=lzma.FORMAT_XZ) == ab.text(128 * K)


# ---- through lzma_code ----
def test_env_variable_through_lzma_code(enc, monkeypatch):
    import xz_amd
    bs = 64 * K
    data = ab.synth_x86(2 * bs, 41) + ab.text(bs)
    monkeypatch.setenv("XZAMD_AUTO_BCJ", "1")
    pieces, _ = sb.lzma_encode(data, 6, piece=8 * K, mt_block_size=bs)
    whole, _ = sb.lzma_encode(data, 6, mt_block_size=bs)
    assert pieces == whole
    _, blocks, usz = xz_amd.file_index(whole)
    assert usz == len(data) and [_chain(whole, b["header_offset"]) for b in blocks] == [X86, X86, 0]
    assert lzma.decompress(whole, format=lzma.FORMAT_XZ) == data
    auto, _ = enc.encode(_cuda(data), preset=6, block_size=bs, auto_bcj=True)
    assert whole == _bytes(auto)
    monkeypatch.delenv("XZAMD_AUTO_BCJ")
    off, _ = sb.lzma_encode(data, 6, mt_block_size=bs)
    plain, _ = enc.encode(_cuda(data), preset=6, block_size=bs)
    assert off == _bytes(plain)
