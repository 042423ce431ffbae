"""Automatic per-Block literal context on the device (XZAMD_F_AUTO_LCLP, DESIGN.md 3.5 "Automatic literal context"): the joint
histograms and choices of the kernels against the numpy model (tests/_auto_lclp.py) and the C rule (xz_amd/csrc/lclp_rule.h
through tests/host_stub/stub_xzk_lclp.c) bit for bit; Streams whose Blocks differ in lc / lp through the reference decoder,
the properties byte of their chunks, and every Block against the oracle run on that Block alone with its pair; no change on
text; the statistic behind the automatic delta; verified encode; sizes; declined flags; XZAMD_AUTO_LCLP=1 through lzma_code."""
import ctypes as C
import lzma
import os
import subprocess

import numpy as np
import pytest

import _auto_delta as ad
import _auto_lclp as ll
import _corpora as cp
import _oracle as o
import _single_block as sb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS_ERROR = 8
M = 1 << 20
RAGGED = 300 << 10


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    e = xz_amd.Encoder()
    yield e
    e.close()


@pytest.fixture(scope="module")
def crule(tmp_path_factory):
    """the C rule on one Block: (lc, lp)"""
    so = str(tmp_path_factory.mktemp("lclp") / "lclp_rule.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-DSTUB_LCLP_RULE_ONLY",
                    os.path.join(ROOT, "tests", "host_stub", "stub_xzk_lclp.c"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.stub_lclp_block.restype = C.c_uint32
    lib.stub_lclp_block.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(block, lc=3, lp=0):
        hist = np.zeros(ll.HIST_SHAPE, dtype=np.uint32)
        cand = np.zeros(15, dtype=np.uint32)
        S = np.zeros(15, dtype=np.uint64)
        nc = C.c_uint32(0)
        v = lib.stub_lclp_block(bytes(block), len(block), lc, lp, hist.ctypes.data, cand.ctypes.data, S.ctypes.data, C.byref(nc))
        return (v & 255, v >> 8)
    return run


def _text(n, seed=5):
    import xz_amd
    return xz_amd.corpus_text(n, seed=seed).tobytes()


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


_MIXED = {}


def _mixed():
    """text, float32 walk, RGBA, 32-byte records, and a ragged 300 KiB of RGBA: five Blocks of 1 MiB (above XZAMD_SEED_LEN + 512:
    the two-phase path) -- with the model's choices and histograms, computed once"""
    if not _MIXED:
        data = _text(M) + bytes(ll.f32_walk(M)) + bytes(cp.rgba_image(M)) + bytes(ll.flow_records(M)) + bytes(cp.rgba_image(RAGGED, seed=121))
        _MIXED["data"] = data
        _MIXED["pairs"], _MIXED["hists"] = ll.choose_blocks(data, M)
    return _MIXED["data"], _MIXED["pairs"], _MIXED["hists"]


def _chunk_props(raw, binfo):
    """per Block: the properties bytes of its LZMA2 chunks that carry one, and the Block's LZMA2 data"""
    out = []
    for b in binfo:
        p = b.out_offset + (raw[b.out_offset] + 1) * 4
        start, props = p, []
        while raw[p] != 0:
            c = raw[p]
            if c < 0x80:
                assert c in (1, 2)
                p += 3 + ((raw[p + 1] << 8) | raw[p + 2]) + 1
            else:
                csize = ((raw[p + 3] << 8) | raw[p + 4]) + 1
                if c >= 0xC0:
                    props.append(raw[p + 5])
                p += (6 if c >= 0xC0 else 5) + csize
        out.append((props, raw[start:p + 1]))
    return out


# ---- (a) kernel against rule ----
@pytest.mark.parametrize("case", ["mixed", "short_block", "one_byte", "window_and_a_byte", "job_2_2"])
def test_kernel_against_rule(enc, crule, case):
    lc, lp = (2, 2) if case == "job_2_2" else (3, 0)
    if case in ("mixed", "job_2_2"):
        data, want, want_hist = _mixed()
        bs = M
        if case == "job_2_2":
            want, want_hist = ll.choose_blocks(data, bs, lc, lp)
    else:
        data = bytes(ll.f32_walk(M))[:{"short_block": 1000, "one_byte": 1, "window_and_a_byte": 65536 + 4096 + 1}[case]]
        bs = M
        want, want_hist = ll.choose_blocks(data, bs)
    got = enc.choose_lclp(_cuda(data), bs, lc, lp)
    hist, props = enc.lclp_stats(len(want))
    print(case, "model", want, "device", got)
    assert hist.dtype == want_hist.dtype and np.array_equal(hist, want_hist)
    assert got == want and props == want
    assert got == [crule(data[i:i + bs], lc, lp) for i in range(0, len(data), bs)]
    if case == "mixed":
        assert got[0] == (3, 0) and got[1] == (0, 2) and got[2] == (0, 2) and got[4][1] >= 2 and got[3] != (3, 0)


# ---- (b) a Stream whose Blocks differ in lc / lp ----
@pytest.mark.parametrize("preset", [6, 1])
def test_mixed_stream(enc, preset):
    import xz_amd
    data, pairs, _ = _mixed()
    d = _cuda(data)
    opts = xz_amd.preset_options(preset)
    out, binfo = enc.encode(d, opts=opts, block_size=M, auto_lclp=True)
    raw = _bytes(out)
    st = enc.stats()
    assert len(binfo) == 5
    rr, dec = o.ref_decode(raw, len(data) + 16)
    assert rr == 1 and dec == data
    assert lzma.decompress(raw, format=lzma.FORMAT_XZ) == data
    # the pair of every Block stands in the properties byte of its chunks
    blocks = _chunk_props(raw, binfo)
    for b, (props, _) in enumerate(blocks):
        lc, lp = pairs[b]
        assert props and set(props) == {(opts.pb * 5 + lp) * 9 + lc}, (b, pairs[b], props)
    # ... and every Block is what the oracle writes for that Block alone with its pair
    payloads = []
    for b, (lc, lp) in enumerate(pairs):
        o2 = xz_amd.preset_options(preset)
        o2.lc, o2.lp = lc, lp
        two = bool(o2.gpu_parser and o2.gpu_sa_window and o2.span_cost and o2.enc_span_bits)
        prm = o.params_for_gpu_options(o2, span_cost_used=st.span_cost_used) if two else o.params_for_gpu_options(o2)
        payloads.append(o.orc_encode_block(data[b * M:(b + 1) * M], prm))
        assert blocks[b][1] == payloads[b], ("Block", b, pairs[b], o.first_diff(blocks[b][1], payloads[b]))
    prm0 = o.params_for_gpu_options(opts)
    assert o.first_diff(raw, o.orc_xz_stream(data, prm0, M, payloads=payloads)) == -1
    # the device decoders read it too
    x = _cuda(raw)
    assert _bytes(enc.decode(x, len(data))[0]) == data
    # several batches in one call (both pipeline parities): the same Stream
    enc.set_batch_bytes(2 * M)
    try:
        out2, _ = enc.encode(d, opts=opts, block_size=M, auto_lclp=True)
        assert _bytes(out2) == raw
    finally:
        enc.set_batch_bytes((1 << 31) - (1 << 20))


# ---- (c) text: nothing changes ----
def test_all_text_is_byte_identical(enc):
    text = _text(4 * M + RAGGED, seed=9)
    d = _cuda(text)
    assert enc.choose_lclp(d, M) == [(3, 0)] * 5
    for preset in (6, 1):
        flagged, _ = enc.encode(d, preset=preset, block_size=M, auto_lclp=True)
        plain, _ = enc.encode(d, preset=preset, block_size=M)
        assert _bytes(flagged) == _bytes(plain)


# ---- (d) stacking with the automatic delta ----
def test_statistic_behind_the_automatic_delta(enc):
    pcm = bytes(cp.pcm16_stereo(2 * M))
    data = pcm[:M] + _text(M, seed=11) + pcm[M:] + _text(RAGGED, seed=12)
    d = _cuda(data)
    dists, _ = ad.choose_blocks(data, M)
    assert dists == [4, 0, 4, 0]
    # what LZMA2 sees: every Block behind its own delta filter
    filt = bytearray()
    for b, dist in enumerate(dists):
        x = np.frombuffer(data[b * M:(b + 1) * M], dtype=np.uint8).astype(np.int64)
        y = x.copy()
        if dist:
            y[dist:] = (x[dist:] - x[:-dist]) & 255
        filt += y.astype(np.uint8).tobytes()
    want, want_hist = ll.choose_blocks(bytes(filt), M)
    out, binfo = enc.encode(d, preset=6, block_size=M, auto_delta=True, auto_lclp=True, verify=True)
    hist, props = enc.lclp_stats(4)
    print("delta", dists, "model on the filtered bytes", want, "device", props)
    assert np.array_equal(hist, want_hist) and props == want
    assert want[0] != (3, 0) and want[1] == (3, 0)      # a delta-filtered 16-bit PCM Block is aligned data
    raw = _bytes(out)
    rr, dec = o.ref_decode(raw, len(data) + 16)
    assert rr == 1 and dec == data
    for b, (pr, _) in enumerate(_chunk_props(raw, binfo)):
        assert set(pr) == {(2 * 5 + want[b][1]) * 9 + want[b][0]}, (b, want[b], pr)
    plain, _ = enc.encode(d, preset=6, block_size=M, auto_delta=True)
    print(f"auto_delta + auto_lclp {len(raw)} against auto_delta alone {plain.numel()}: {len(raw) / plain.numel():.4f}")
    # ... and behind a filter named by the caller
    import xz_amd
    opts = xz_amd.preset_options(6)
    opts.bcj = xz_amd.filter_delta(4)
    out3, _ = enc.encode(_cuda(pcm), opts=opts, block_size=M, auto_lclp=True)
    assert enc.lclp_stats(2)[1] == [want[0], want[2]]
    assert o.ref_decode(_bytes(out3), len(pcm) + 16) == (1, pcm)


# ---- (e) verified encode ----
@pytest.mark.parametrize("preset", [6, 1])
def test_verified_encode(enc, preset):
    data, pairs, _ = _mixed()
    d = _cuda(data)
    out, _ = enc.encode(d, preset=preset, block_size=M, auto_lclp=True, verify=True)        # raises on a defect
    rep = enc.verify_report()
    print(rep)
    assert rep["first_bad_block"] is None
    assert enc.verify_blocks(out, d) == ["none"] * 5
    plain, _ = enc.encode(d, preset=preset, block_size=M, auto_lclp=True)
    assert _bytes(plain) == _bytes(out)
    # the kept resume table carries every Block's own pair: verification with it passes
    kept, _ = enc.encode(d, preset=preset, block_size=M, auto_lclp=True, keep_resume=True)
    enc.verify(kept, d)


# ---- (f) size ----
def test_size_on_float_and_pixel_blocks(enc):
    """The device encoder's own gain (the calibration is the reference's): no larger than the plain Stream on the float32 and
    RGBA Blocks.  The measured ratios go to stdout; profiles/auto_lclp_ab.txt records a run."""
    data, pairs, _ = _mixed()
    d = _cuda(data)
    for preset in (6, 1):
        _, fb = enc.encode(d, preset=preset, block_size=M, auto_lclp=True)
        _, pb = enc.encode(d, preset=preset, block_size=M)
        for b, name in enumerate(["text", "f32walk", "rgba", "flow32", "rgba-ragged"]):
            print(f"preset {preset} {name} {pairs[b]}: flagged {fb[b].unpadded_size} plain {pb[b].unpadded_size} "
                  f"ratio {fb[b].unpadded_size / pb[b].unpadded_size:.4f}")
        assert fb[0].unpadded_size == pb[0].unpadded_size
        for b in (1, 2, 4):
            assert fb[b].unpadded_size <= pb[b].unpadded_size, (preset, b)


# ---- (g) what the flag declines, and the presets ----
def _small():
    """192 KiB of the float32 walk and 64 KiB of text, in Blocks of 128 KiB, with the model's choices"""
    data, _, _ = _mixed()
    small = data[M:M + (192 << 10)] + data[:64 << 10]
    want, _ = ll.choose_blocks(small, 128 << 10)
    assert want[0] != (3, 0)
    return small, want


def test_declined_combinations(enc):
    import xz_amd
    small, _ = _small()
    d = _cuda(small)
    for kw in (dict(flags=xz_amd.F_SEGMENTS), dict(single=True), dict(repair=True)):
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, preset=6, block_size=128 << 10, auto_lclp=True, **kw)
        assert ei.value.code == OPTIONS_ERROR and "auto lclp" in str(ei.value), kw
    # a job with lc = 4 keeps its pair: the plain Stream
    opts = xz_amd.preset_options(6)
    opts.lc = 4
    out, _ = enc.encode(d, opts=opts, block_size=128 << 10, auto_lclp=True)
    plain, _ = enc.encode(d, opts=opts, block_size=128 << 10)
    assert _bytes(out) == _bytes(plain)


@pytest.mark.parametrize("preset,pb", [(p, 2) for p in range(10)] + [(6, 3), (6, 4), (6, 0)])
def test_every_preset_and_pb(enc, preset, pb):
    """Every preset, and pb 3 / 4 (the parser keeps its pb = 2 view): the Stream decodes, every Block has its pair"""
    import xz_amd
    small, want = _small()
    opts = xz_amd.preset_options(preset)
    opts.pb = pb
    out, binfo = enc.encode(_cuda(small), opts=opts, block_size=128 << 10, auto_lclp=True, verify=True)
    raw = _bytes(out)
    assert o.ref_decode(raw, len(small) + 16) == (1, small)
    assert [set(p) for p, _ in _chunk_props(raw, binfo)] == [{(pb * 5 + lp) * 9 + lc} for lc, lp in want]


# ---- (h) through lzma_code ----
def test_env_variable_through_lzma_code(enc, monkeypatch):
    data, pairs, _ = _mixed()
    data = data[:3 * M]
    monkeypatch.setenv("XZAMD_AUTO_LCLP", "1")
    whole, _ = sb.lzma_encode(data, 6, mt_block_size=M)
    monkeypatch.delenv("XZAMD_AUTO_LCLP")
    flagged, _ = enc.encode(_cuda(data), preset=6, block_size=M, auto_lclp=True)
    assert whole == _bytes(flagged)
    assert o.ref_decode(whole, len(data) + 16) == (1, data)
    off, _ = sb.lzma_encode(data, 6, mt_block_size=M)
    plain, _ = enc.encode(_cuda(data), preset=6, block_size=M)
    assert off == _bytes(plain) and off != whole
