"""Per-Block verification and repair (DESIGN.md 3.6 "Repair"): verify_blocks names every bad Block of a Stream, repair
re-encodes the Blocks the device decoder rejects and splices them in, encode(repair=True) does both before it returns, and
XZAMD_REPAIR=1 does it for the jobs of lzma_stream_encoder_mt.  Unless said otherwise: preset 6 with enc_span_bits =
200000, Blocks of 1 MiB, corpus_text(seed=5); the judge of every Stream is the reference decoder (o.ref_decode)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _oracle as o

pytestmark = pytest.mark.gpu

OPTIONS_ERROR, DATA_ERROR, BUF_ERROR = 8, 9, 10
K = 1024
BS = 1 << 20
N3 = 2 * BS + 300 * K + 7             # three Blocks, the last one odd-length
FBS = 300001                          # foreign Stream: four Blocks of 1 MiB at offsets that are no multiple of 4


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    e = xz_amd.Encoder()
    yield e
    e.close()


@pytest.fixture(scope="module")
def text():
    import xz_amd
    return xz_amd.corpus_text(5 << 20, seed=5).tobytes()


@pytest.fixture(scope="module")
def foreign(text):
    """(Stream of the reference's MT encoder, its data, its Blocks)"""
    import xz_amd
    data = text[:1 << 20]
    xz = bytes(o.ref_encode_mt(data, 6, block_size=FBS))
    blocks = xz_amd.file_index(xz)[1]
    assert [b["uncompressed_size"] for b in blocks] == [FBS, FBS, FBS, (1 << 20) - 3 * FBS]
    return xz, data, blocks


def rnd(n, s):
    return np.random.default_rng(s).integers(0, 256, n, dtype=np.uint8).tobytes()


def _opts(**kw):
    import xz_amd
    op = xz_amd.preset_options(6)
    op.enc_span_bits = 200000
    for k, v in kw.items():
        setattr(op, k, v)
    return op


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _ref_ok(xz, data):
    rr, dec = o.ref_decode(xz, len(data) + 16)
    return rr == 1 and dec == data


def _index(xz):
    import xz_amd
    return xz_amd.file_index(xz)[1]


def _block_bytes(xz, blk):
    return xz[blk["header_offset"]: blk["header_offset"] + blk["total_size"]]


def _payload_middle(xz, blk, check_bytes=8):
    """offset of the middle byte of the Block's LZMA2 data"""
    ho = blk["header_offset"]
    hs = (xz[ho] + 1) * 4
    return ho + hs + (blk["unpadded_size"] - hs - check_bytes) // 2


def _tamper(xz, offsets):
    t = bytearray(xz)
    for p in offsets:
        t[p] ^= 0x5A
    return bytes(t)


def _controls(xz, blk):
    """control bytes of the Block's LZMA2 chunks, in order"""
    ho = blk["header_offset"]
    p = ho + (xz[ho] + 1) * 4
    out = []
    while xz[p] != 0:
        ctl = xz[p]
        out.append(ctl)
        if ctl >= 0x80:
            p += (6 if ctl >= 0xC0 else 5) + ((xz[p + 3] << 8) | xz[p + 4]) + 1
        else:
            assert ctl in (1, 2)
            p += 3 + ((xz[p + 1] << 8) | xz[p + 2]) + 1
    return out


def _first_lzma_control(xz, blk):
    return next((c for c in _controls(xz, blk) if c >= 0x80), None)


def _encode_kept(enc, data):
    """encode with keep_resume on `enc`: (Stream bytes, its Blocks)"""
    xz, _ = enc.encode(_cuda(data), opts=_opts(), block_size=BS, keep_resume=True)
    xz = _bytes(xz)
    return xz, _index(xz)


def _repair(enc, xz, data, slack=1 << 20, **kw):
    """Encoder.repair on a copy of xz in a buffer with `slack` spare bytes: (repaired bytes, report, the buffer)"""
    import torch
    buf = torch.zeros(len(xz) + slack, dtype=torch.uint8, device="cuda")
    buf[: len(xz)] = _cuda(xz)
    view, rep = enc.repair(buf, len(xz), _cuda(data), **kw)
    print("repair report", rep)
    return _bytes(view), rep, buf


# ---- 1, 2: verdicts ----------------------------------------------------------------------------------------------

def test_verdicts_own_stream(enc, text):
    data = text[:N3]
    xz, blocks = _encode_kept(enc, data)
    assert len(blocks) == 3
    d = _cuda(data)
    assert enc.verify_blocks(_cuda(xz), d) == ["none"] * 3
    rep = enc.verify_report()
    assert rep["first_bad_step"] == "none" and rep["first_bad_block"] is None and rep["table_used"]
    check_at = blocks[2]["header_offset"] + blocks[2]["total_size"] - 8
    bad = _tamper(xz, [_payload_middle(xz, blocks[1]), check_at])
    steps = enc.verify_blocks(_cuda(bad), d)
    rep = enc.verify_report()
    print("steps", steps, "report", rep)
    assert steps[0] == "none" and steps[1] in ("decode", "compare") and steps[2] == "check"
    assert rep["first_bad_block"] == 1 and rep["blocks"] == 3
    # ... and without the original: grammar, decode and Check only
    steps = enc.verify_blocks(_cuda(bad))
    assert steps[0] == "none" and steps[2] == "check"


def test_verdicts_foreign_stream_at_odd_offsets(enc, foreign):
    """The original is tampered with, not the Stream: the verdict must be "compare" for exactly the Blocks that differ.  A
    verification unit reads its history from the original, so without the second run of the per-Block verification (history
    = the Block's own output) the device gave "decode" for the first byte of Block 3 and "check" for a middle byte of Block 2
    (measured on the MI355X with the first-pass verdicts alone; the last byte of Block 1, which nothing reads as history,
    gave "compare" as expected)."""
    xz, data, blocks = foreign
    dxz = _cuda(xz)
    assert enc.verify_blocks(dxz, _cuda(data)) == ["none"] * 4
    t = bytearray(data)
    t[2 * FBS - 1] ^= 1                 # last byte of Block 1
    t[3 * FBS] ^= 0x80                  # first byte of Block 3
    assert enc.verify_blocks(dxz, _cuda(bytes(t))) == ["none", "compare", "none", "compare"]
    assert enc.verify_report()["first_bad_step"] == "compare"
    t = bytearray(data)
    t[2 * FBS + 12345] ^= 0xFF
    assert enc.verify_blocks(dxz, _cuda(bytes(t))) == ["none", "none", "compare", "none"]
    assert enc.verify_blocks(dxz) == ["none"] * 4
    # a Block Header that fails its CRC32: bad at "grammar", the other Blocks are still looked at
    h = _tamper(xz, [blocks[2]["header_offset"] + 2])
    assert enc.verify_blocks(_cuda(h), _cuda(data)) == ["none", "none", "grammar", "none"]
    assert enc.verify_report()["first_bad_block"] == 2


# ---- 3 - 6: repair of a tampered Stream --------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [(1,), (0,), (2,), (0, 1), (0, 1, 2)])
def test_repair_tampered(enc, text, bad):
    import xz_amd
    data = text[:N3]
    xz, blocks = _encode_kept(enc, data)
    broken = _tamper(xz, [_payload_middle(xz, blocks[b]) for b in bad])
    assert not _ref_ok(broken, data)
    fixed, rep, buf = _repair(enc, broken, data, opts=_opts())
    assert _ref_ok(fixed, data)
    nblocks = _index(fixed)                       # xzamd_file_index_host accepts the result
    assert len(nblocks) == 3
    for b in range(3):
        if b not in bad:
            assert _block_bytes(fixed, nblocks[b]) == _block_bytes(xz, blocks[b]), b
        else:
            assert _first_lzma_control(fixed, nblocks[b]) >= 0xE0
    assert rep["blocks"] == 3 and rep["blocks_bad"] == len(bad) and rep["blocks_reencoded"] == len(bad)
    assert rep["blocks_stored"] == 0 and rep["passes"] >= 2
    assert rep["size_before"] == len(broken) and rep["size_after"] == len(fixed)
    # the kept table still fits: the records of the repaired Blocks are void, the others open units
    vr = enc.verify(buf[: len(fixed)], _cuda(data))
    print("verify with the kept table", vr)
    assert vr["table_used"] and vr["first_bad_step"] == "none"
    kinds = [enc.debug_resume_peek(r) for r in range(enc.debug_resume_records())]
    assert all((h["kind"] == 3) == (h["block"] in bad) for h in kinds)


def test_repair_stored_rung(enc, text, monkeypatch):
    data = text[:N3]
    xz, blocks = _encode_kept(enc, data)
    broken = _tamper(xz, [_payload_middle(xz, blocks[1])])
    monkeypatch.setenv("XZAMD_TEST_REPAIR_RUNG", "2")
    fixed, rep, _ = _repair(enc, broken, data, slack=2 << 20, opts=_opts())
    assert rep["blocks_bad"] == 1 and rep["blocks_stored"] == 1 and rep["blocks_reencoded"] == 0
    nblocks = _index(fixed)
    assert _controls(fixed, nblocks[1])[0] == 0x01
    assert nblocks[1]["total_size"] > BS
    assert _block_bytes(fixed, nblocks[0]) == _block_bytes(xz, blocks[0])
    assert _block_bytes(fixed, nblocks[2]) == _block_bytes(xz, blocks[2])
    assert _ref_ok(fixed, data)


def test_repair_foreign_stream(enc, foreign):
    import xz_amd
    xz, data, blocks = foreign
    broken = _tamper(xz, [_payload_middle(xz, blocks[1])])
    assert not _ref_ok(broken, data)
    fixed, rep, _ = _repair(enc, broken, data, opts=xz_amd.preset_options(6))
    assert rep["blocks_bad"] == 1 and rep["blocks_reencoded"] == 1
    assert _ref_ok(fixed, data)
    nblocks = _index(fixed)
    for b in (0, 2, 3):
        assert _block_bytes(fixed, nblocks[b]) == _block_bytes(xz, blocks[b]), b


def test_repair_is_all_or_nothing(enc, text, monkeypatch):
    import xz_amd
    data = text[:N3]
    xz, blocks = _encode_kept(enc, data)
    broken = _tamper(xz, [_payload_middle(xz, blocks[1])])
    monkeypatch.setenv("XZAMD_TEST_REPAIR_RUNG", "2")        # the stored Block is larger than the coded one
    buf = _cuda(broken)
    with pytest.raises(xz_amd.XzAmdError) as ei:
        enc.repair(buf, len(broken), _cuda(data), opts=_opts())
    assert ei.value.code == BUF_ERROR and ei.value.new_size > len(broken)
    assert _bytes(buf) == broken


# ---- 7: in-encode repair, forced ---------------------------------------------------------------------------------

def _forced(enc, data, monkeypatch, opts=None, **kw):
    """encode(repair=True) with Blocks 0 and 2 rejected by the test knob, and the plain encode of the same call"""
    opts = opts or _opts()
    plain, pinfo = enc.encode(_cuda(data), opts=opts, block_size=BS, **kw)
    plain = _bytes(plain)
    monkeypatch.setenv("XZAMD_TEST_REPAIR_REJECT", "0,2")
    try:
        xz, binfo = enc.encode(_cuda(data), opts=opts, block_size=BS, repair=True, **kw)
    finally:
        monkeypatch.delenv("XZAMD_TEST_REPAIR_REJECT", raising=False)
    rep = enc.repair_report()
    print("repair report", rep, "verify report", enc.verify_report())
    return _bytes(xz), binfo, rep, plain, pinfo


def test_encode_repair_forced(enc, text, monkeypatch):
    data = text[:N3]
    xz, binfo, rep, plain, _ = _forced(enc, data, monkeypatch)
    assert _ref_ok(xz, data)
    assert rep["blocks_bad"] == 2 and rep["blocks_reencoded"] == 2 and rep["passes"] >= 2
    assert enc.verify_report()["first_bad_step"] == "none"
    blocks, pblocks = _index(xz), _index(plain)
    assert _block_bytes(xz, blocks[1]) == _block_bytes(plain, pblocks[1])
    assert xz != plain
    # binfo describes the repaired Stream
    assert [(b.out_offset, b.unpadded_size, b.total_size) for b in binfo] == \
           [(k["header_offset"], k["unpadded_size"], k["total_size"]) for k in blocks]
    assert enc.stats().out_bytes == len(xz)


def test_encode_repair_forced_batches(text, monkeypatch):
    import xz_amd
    data = text[:5 << 20]
    e = xz_amd.Encoder()
    try:
        e.set_batch_bytes(2 << 20)
        xz, _, rep, plain, _ = _forced(e, data, monkeypatch)
        assert e.stats().batches == 3
    finally:
        e.close()
    assert _ref_ok(xz, data) and rep["blocks"] == 5 and rep["blocks_bad"] == 2
    blocks, pblocks = _index(xz), _index(plain)
    for b in (1, 3, 4):
        assert _block_bytes(xz, blocks[b]) == _block_bytes(plain, pblocks[b]), b


def test_encode_repair_forced_delta(enc, text, monkeypatch):
    import xz_amd
    data = text[:N3]
    xz, _, rep, plain, _ = _forced(enc, data, monkeypatch, opts=_opts(bcj=xz_amd.filter_delta(4)))
    assert _ref_ok(xz, data) and rep["blocks_bad"] == 2
    blocks = _index(xz)
    assert all(b["filter_ids"] == (3, 0x21) for b in blocks)
    assert _block_bytes(xz, blocks[1]) == _block_bytes(plain, _index(plain)[1])


def test_encode_repair_forced_blocks_only(enc, text, monkeypatch):
    import xz_amd
    L = xz_amd.lib()
    data = text[:N3]
    raw, binfo, rep, plain, pinfo = _forced(enc, data, monkeypatch, blocks_only=True)
    assert rep["blocks_bad"] == 2 and len(binfo) == 3
    hdr = (C.c_uint8 * 12)()
    assert L.xzamd_frame_header(hdr, xz_amd.CHECK_CRC64) == 12
    unp = (C.c_uint64 * 3)(*[b.unpadded_size for b in binfo])
    unc = (C.c_uint64 * 3)(*[b.uncompressed_size for b in binfo])
    tail = (C.c_uint8 * 256)()
    w = L.xzamd_frame_index_footer(tail, 256, xz_amd.CHECK_CRC64, unp, unc, 3)
    assert w > 0 and binfo[0].out_offset == 0 and binfo[2].out_offset + binfo[2].total_size == len(raw)
    assert _ref_ok(bytes(hdr) + raw + bytes(tail[:w]), data)
    assert raw[binfo[1].out_offset: binfo[1].out_offset + binfo[1].total_size] == \
           plain[pinfo[1].out_offset: pinfo[1].out_offset + pinfo[1].total_size]


def _records16(n, seed):
    """n bytes of 16-byte records: a counter, two slowly changing fields, four noisy bytes (as in test_model_sizes)"""
    rng = np.random.default_rng(seed)
    k = (n + 15) // 16
    rec = np.zeros((k, 16), dtype=np.uint8)
    rec[:, 0:4] = np.arange(k, dtype="<u4").view(np.uint8).reshape(k, 4)
    rec[:, 4:8] = (np.cumsum(rng.integers(0, 3, k)).astype("<u4")).view(np.uint8).reshape(k, 4)
    rec[:, 8:12] = (1000000 + np.cumsum(rng.integers(-2, 3, k))).astype("<u4").view(np.uint8).reshape(k, 4)
    rec[:, 12:16] = rng.integers(0, 16, (k, 4), dtype=np.uint8)
    return rec.tobytes()[:n]


def test_encode_repair_forced_pb4_falls_back_to_the_fast_parser(enc, monkeypatch):
    data = _records16(600 * K, 3)
    xz, _, rep, plain, _ = _forced(enc, data, monkeypatch, opts=_opts(lc=0, lp=4, pb=4))
    assert _ref_ok(xz, data)
    assert rep["blocks"] == 1 and rep["blocks_bad"] == 1 and rep["blocks_reencoded"] == 1 and rep["blocks_stored"] == 0
    assert xz != plain


# ---- 8: the real defect ------------------------------------------------------------------------------------------

def _defect_inputs(text):
    lorem = o.corpus_lorem(1 << 20)
    lorem = lorem if isinstance(lorem, bytes) else bytes(lorem)
    return {
        "A": (rnd(512 * K, 1) + lorem[:512 * K], BS),
        "B": (text[:BS] + rnd(512 * K, 1) + lorem[:512 * K] + text[BS:BS + 300 * K], BS),
        "D": (rnd(384 * K, 2) + text[:640 * K], BS),
        "E": (rnd(640 * K, 2) + text[:384 * K], BS),
        "C": (rnd(BS, 1) + lorem, 0),
    }


def test_encode_repair_real_defect(enc, text):
    """Blocks that begin with >= ~320 KiB of incompressible bytes: the two-phase encoder writes their first LZMA chunk
    without the properties byte.  The oracle gives LZMA_DATA_ERROR on all five inputs at the default span cost (checked on
    the CPU); the device picks span_cost_used itself, so at least 4 of the 5 must be rejected by encode(verify=True) here --
    fewer would mean the device no longer shows the defect on these inputs (a parity finding, not a reason to skip)."""
    import xz_amd
    rejected = []
    for name, (data, bs) in _defect_inputs(text).items():
        d = _cuda(data)
        bad = []
        try:
            enc.encode(d, preset=6, block_size=bs, verify=True)
        except xz_amd.XzAmdError as e:
            assert e.code == DATA_ERROR, (name, e)
            assert not _ref_ok(_bytes(e.stream), data), name           # the reference rejects it too
            steps = enc.verify_blocks(e.stream.clone(), d)
            bad = [b for b, s in enumerate(steps) if s != "none"]
            rejected.append(name)
        xz, _ = enc.encode(d, preset=6, block_size=bs, repair=True)
        xz = _bytes(xz)
        rep = enc.repair_report()
        print(name, "bad Blocks", bad, "repair report", rep)
        assert _ref_ok(xz, data), name
        if bad:
            assert rep["blocks_bad"] == len(bad) >= 1, name
            blocks = _index(xz)
            for b in bad:
                assert _first_lzma_control(xz, blocks[b]) >= 0xC0, (name, b)
        else:
            assert rep["blocks_bad"] == 0, name
    assert len(rejected) >= 4, f"the device no longer shows the stored-prefix defect on these inputs: rejected {rejected}"


# ---- 9: flags ----------------------------------------------------------------------------------------------------

def test_flags(enc, text):
    import xz_amd
    d = _cuda(text[:N3])
    with pytest.raises(xz_amd.XzAmdError) as ei:
        enc.encode(d, opts=_opts(), block_size=BS, flags=xz_amd.F_REPAIR | xz_amd.F_SEGMENTS, check=xz_amd.CHECK_CRC32)
    assert ei.value.code == OPTIONS_ERROR
    plain, _ = enc.encode(d, opts=_opts(), block_size=BS)
    plain = _bytes(plain)
    xz, _ = enc.encode(d, opts=_opts(), block_size=BS, repair=True)
    rep = enc.repair_report()
    assert _bytes(xz) == plain and rep["blocks_bad"] == 0 and rep["passes"] == 1 and rep["blocks"] == 3
    assert enc.verify_report()["table_used"]


# ---- 10: the lzma_* front end ------------------------------------------------------------------------------------

def _lzma_code_encode(L, data, preset, block_size, piece):
    """lzma_stream_encoder_mt / lzma_code, `piece` bytes per LZMA_RUN call, then LZMA_FINISH"""
    tools = os.path.join(o.ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from bench_lzma_code import Mt, Stream
    ib = C.create_string_buffer(data, len(data))
    ob = C.create_string_buffer(len(data) + (1 << 20))
    s = Stream()
    m = Mt(threads=1, preset=preset, check=4, block_size=block_size, timeout=0)
    assert L.lzma_stream_encoder_mt(C.byref(s), C.byref(m)) == 0
    s.next_out = C.cast(ob, C.c_void_p).value
    s.avail_out = len(ob)
    pos = 0
    while pos < len(data):
        k = min(piece, len(data) - pos)
        s.next_in = C.cast(ib, C.c_void_p).value + pos
        s.avail_in = k
        while s.avail_in:
            assert L.lzma_code(C.byref(s), 0) == 0
        pos += k
    r = L.lzma_code(C.byref(s), 3)
    while r == 0:
        r = L.lzma_code(C.byref(s), 3)
    assert r == 1
    out = ob.raw[: s.total_out]
    L.lzma_end(C.byref(s))
    return out


def test_front_end_repairs_its_jobs(enc, text, monkeypatch):
    import xz_amd
    L = xz_amd.lib()
    data, bs = _defect_inputs(text)["B"]
    plain, _ = enc.encode(_cuda(data), preset=6, block_size=bs)
    plain = _bytes(plain)
    monkeypatch.delenv("XZAMD_REPAIR", raising=False)
    assert _lzma_code_encode(L, data, 6, bs, 100000) == plain          # unset: today's Stream
    monkeypatch.setenv("XZAMD_REPAIR", "1")
    try:
        out = _lzma_code_encode(L, data, 6, bs, 100000)
    finally:
        monkeypatch.delenv("XZAMD_REPAIR", raising=False)
    assert _ref_ok(out, data)
    blocks, pblocks = _index(out), _index(plain)
    assert len(blocks) == 3
    assert _block_bytes(out, blocks[0]) == _block_bytes(plain, pblocks[0])
