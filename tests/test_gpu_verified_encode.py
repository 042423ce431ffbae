"""Verified encode ("Units at resume records"): the two-phase encoder exports one resume record per encode
span, the verification decode opens a unit at every record, and an encode with verify=True checks its own Stream on the
device before it returns.  Unless said otherwise: preset 6 with enc_span_bits = 200000, Blocks of 1 MiB, corpus_text(seed=5)."""
import numpy as np
import pytest

import _oracle as o

pytestmark = pytest.mark.gpu

OPTIONS_ERROR, DATA_ERROR = 8, 9
BS = 1 << 20
N3 = 2 * BS + 300 * 1024 + 7          # three Blocks, the last one short


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


def _verified(enc, data, opts, block_size=BS):
    """encode(verify=True) that must pass: (Stream bytes, report, stats)"""
    xz, _ = enc.encode(_cuda(data), opts=opts, block_size=block_size, verify=True)
    rep, st = enc.verify_report(), enc.stats()
    print("verify report", rep, "enc_spans", st.enc_spans, "blocks", st.blocks, "ms_verify", st.ms_verify)
    assert rep["first_bad_step"] == "none" and rep["first_bad_block"] is None and rep["mismatching_words"] == 0
    return _bytes(xz), rep, st


def test_units_are_the_encode_spans(enc, text):
    data = text[:N3]
    d = _cuda(data)
    xz, _ = enc.encode(d, opts=_opts(), block_size=BS, verify=True)
    rep, st = enc.verify_report(), enc.stats()
    print("verify report", rep, "enc_spans", st.enc_spans, "ms_verify", st.ms_verify)
    assert _ref_ok(_bytes(xz), data)
    assert st.blocks == 3 and st.enc_spans >= st.blocks + 4
    assert rep["units"] == st.enc_spans and rep["records_used"] == st.enc_spans and rep["table_used"]
    assert rep["blocks"] == 3 and rep["mismatching_words"] == 0 and rep["first_bad_step"] == "none"
    assert st.ms_verify > 0
    # the same Stream without the table: the carried spans reset nothing, the Block is the unit
    dec, nb = enc.decode(xz, len(data), expected=d)
    assert nb == 3 and _bytes(dec) == data
    assert enc.debug_decode_units()[:2] == (3, 3)


def _records16(n, seed):
    """n bytes of 16-byte records: a counter, two slowly changing fields, four noisy bytes"""
    rng = np.random.default_rng(seed)
    k = (n + 15) // 16
    rec = np.zeros((k, 16), dtype=np.uint8)
    rec[:, 0:4] = np.arange(k, dtype="<u4").view(np.uint8).reshape(k, 4)
    rec[:, 4:8] = (np.cumsum(rng.integers(0, 3, k)).astype("<u4")).view(np.uint8).reshape(k, 4)
    rec[:, 8:12] = (1000000 + np.cumsum(rng.integers(-2, 3, k))).astype("<u4").view(np.uint8).reshape(k, 4)
    rec[:, 12:16] = rng.integers(0, 16, (k, 4), dtype=np.uint8)
    return rec.tobytes()[:n]


@pytest.mark.parametrize("lc,lp,pb", [(0, 4, 4), (4, 0, 0)])
def test_model_sizes(enc, lc, lp, pb):
    data = _records16(600 * 1024, 3)
    xz, rep, st = _verified(enc, data, _opts(lc=lc, lp=lp, pb=pb))
    assert _ref_ok(xz, data)
    assert st.blocks == 1 and st.enc_spans >= 2
    assert rep["table_used"] and rep["units"] == st.enc_spans


def test_stored_pieces_inside_a_block(enc, text):
    noise = np.random.default_rng(7).integers(0, 256, 400 * 1024, dtype=np.uint8).tobytes()
    data = text[:300 * 1024] + noise + text[300 * 1024:600 * 1024]
    xz, rep, st = _verified(enc, data, _opts())
    assert _ref_ok(xz, data)
    assert st.blocks == 1 and st.blocks_stored == 0 and st.enc_spans >= 2
    assert rep["table_used"] and rep["units"] == st.enc_spans
    kinds = [enc.debug_resume_peek(r)["kind"] for r in range(enc.debug_resume_records())]
    print("record kinds", kinds)
    assert 2 in kinds                 # a span behind a stored piece: flat start, no properties


def test_stored_block_has_void_records(enc, text):
    """An incompressible Block between text Blocks goes out in the stored form (at 4 MiB the raw chunks of its pieces, cut at
    piece ends, exceed the Block bound; at 1 MiB they do not): its encode spans start at no chunk, so its records are void,
    the Block is one unit, and the Blocks around it keep their span units."""
    bs = 4 << 20
    noise = np.random.default_rng(11).integers(0, 256, bs, dtype=np.uint8).tobytes()
    data = text[:bs] + noise + text[bs:bs + 300 * 1024]
    xz, rep, st = _verified(enc, data, _opts(), block_size=bs)
    assert _ref_ok(xz, data)
    assert st.blocks == 3 and st.blocks_stored == 1
    recs = [enc.debug_resume_peek(r) for r in range(enc.debug_resume_records())]
    print("records (block, kind)", [(h["block"], h["kind"]) for h in recs])
    assert len(recs) == st.enc_spans
    void = [h for h in recs if h["kind"] == 3]
    assert void and all(h["block"] == 1 for h in void) and all(h["kind"] == 3 for h in recs if h["block"] == 1)
    assert rep["table_used"] and rep["records_used"] == len(recs) - len(void) and rep["units"] == rep["records_used"] + 1
    assert rep["records_used"] >= 4 + 1           # the spans of the two text Blocks


def test_carry_fallback(enc, text, monkeypatch):
    data = text[:N3]
    monkeypatch.setenv("XZAMD_TEST_LOG_CAP", "8")
    try:
        xz, rep, st = _verified(enc, data, _opts())
        kinds = [enc.debug_resume_peek(r)["kind"] for r in range(enc.debug_resume_records())]
    finally:
        monkeypatch.delenv("XZAMD_TEST_LOG_CAP", raising=False)
    print("record kinds", kinds)
    assert kinds.count(0) > 3         # reset spans behind the first of a Block
    assert rep["table_used"] and rep["units"] == st.enc_spans


@pytest.mark.parametrize("prefix", [512 * 1024, 1 << 20])
def test_stored_prefix_is_never_ok_and_undecodable(enc, prefix):
    """A Block that starts with stored pieces: the encoder may write the first LZMA chunk behind them without its
    properties byte.  verify=True either passes with a Stream the reference decodes, or reports Block 0."""
    import xz_amd
    data = np.random.default_rng(1).integers(0, 256, prefix, dtype=np.uint8).tobytes() + o.corpus_lorem(1 << 20)
    try:
        xz, _ = enc.encode(_cuda(data), opts=xz_amd.preset_options(6), verify=True)
    except xz_amd.XzAmdError as e:
        rep = enc.verify_report()
        print("verify failed:", e, rep, "reference:", o.ref_decode(_bytes(e.stream), len(data) + 16)[0])
        assert e.code == DATA_ERROR and rep["first_bad_block"] == 0 and rep["first_bad_step"] != "none"
        assert len(e.stream) > 32
        return
    assert _ref_ok(_bytes(xz), data)


def test_tampered_stream(enc, text):
    import xz_amd
    data = text[:N3]
    d = _cuda(data)
    xz, binfo = enc.encode(d, opts=_opts(), block_size=BS, keep_resume=True)
    rep = enc.verify(xz, d)
    assert rep["table_used"] and rep["units"] == enc.stats().enc_spans and rep["first_bad_step"] == "none"
    bad = xz.clone()
    bad[binfo[1].out_offset + binfo[1].total_size // 2] ^= 0x10
    with pytest.raises(xz_amd.XzAmdError) as ei:
        enc.verify(bad, d)
    rep = enc.verify_report()
    print("tampered:", ei.value, rep)
    assert ei.value.code == DATA_ERROR and rep["first_bad_block"] == 1
    assert enc.verify(xz, d)["first_bad_step"] == "none"


def _carried_record(enc):
    for r in range(enc.debug_resume_records()):
        h = enc.debug_resume_peek(r)
        if h["kind"] == 1:
            return r, h
    raise AssertionError("no carried record")


@pytest.mark.parametrize("field", ["upos", "model", "state"])
def test_tampered_table(enc, text, field):
    import xz_amd
    data = text[:N3]
    d = _cuda(data)
    xz, _ = enc.encode(d, opts=_opts(), block_size=BS, keep_resume=True)
    r, h = _carried_record(enc)
    enc.debug_resume_poke(r, field, h["upos"] + 1 if field == "upos" else (h["state"] + 1) % 12)
    try:
        rep = enc.verify(xz, d)
    except xz_amd.XzAmdError as e:
        rep = enc.verify_report()
        print(field, "->", e, rep)
        assert e.code == DATA_ERROR and rep["first_bad_step"] != "none"
        if field == "upos":
            assert rep["first_bad_step"] == "grammar" and rep["first_bad_block"] == h["block"]
        return
    # a wrong record that happens to decode: only acceptable when the bytes are the original's (the comparison ran)
    print(field, "-> OK", rep)
    assert field != "upos" and rep["mismatching_words"] == 0 and rep["table_used"]


def test_several_batches(text):
    import xz_amd
    e = xz_amd.Encoder()
    try:
        e.set_batch_bytes(2 << 20)
        data = text[:5 << 20]
        xz, rep, st = _verified(e, data, _opts())
        assert st.batches == 3 and st.blocks == 5
        assert rep["table_used"] and rep["units"] == st.enc_spans == e.debug_resume_records()
        blocks = [e.debug_resume_peek(r)["block"] for r in range(e.debug_resume_records())]
        assert blocks == sorted(blocks) and set(blocks) == set(range(5))
        assert _ref_ok(xz, data)
    finally:
        e.close()


@pytest.mark.parametrize("preset", [1, 3])
def test_single_phase_presets_have_no_records(enc, text, preset):
    import xz_amd
    data = text[:N3]
    xz, rep, st = _verified(enc, data, xz_amd.preset_options(preset))
    assert enc.debug_resume_records() == 0 and not rep["table_used"] and rep["records_used"] == 0
    assert rep["units"] == st.spans and st.spans > st.blocks


def test_filter_chain(enc, text):
    import xz_amd
    data = text[:BS + 100 * 1024]
    xz, rep, st = _verified(enc, data, _opts(bcj=xz_amd.filter_delta(4)))
    assert rep["table_used"] and rep["units"] == st.enc_spans
    assert _ref_ok(xz, data)


def test_flags(enc, text):
    import xz_amd
    data = text[:N3]
    d = _cuda(data)
    for flags in (xz_amd.F_VERIFY | xz_amd.F_BLOCKS_ONLY, xz_amd.F_KEEP_RESUME | xz_amd.F_SEGMENTS):
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, opts=_opts(), block_size=BS, flags=flags)
        assert ei.value.code == OPTIONS_ERROR
    plain, _ = enc.encode(d, opts=_opts(), block_size=BS)
    plain = _bytes(plain)
    assert enc.debug_resume_records() == 0
    kept, _ = enc.encode(d, opts=_opts(), block_size=BS, keep_resume=True)
    assert _bytes(kept) == plain and enc.debug_resume_records() == enc.stats().enc_spans
