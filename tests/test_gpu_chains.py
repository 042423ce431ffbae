"""Verified and repaired encode of single-Block Streams (DESIGN.md 3.6 "Chains", 3.7): encode(single=True) writes the Stream
lzma_easy_encoder writes, verify_chains / repair_chains judge and replace the bare chunk chains of its segments,
encode(single=True, verify / repair) does so before the Stream is framed, and XZAMD_REPAIR=1 does it for the jobs of
lzma_stream_encoder / lzma_easy_encoder.  Unless said otherwise: preset 6, segments of 1 MiB, corpus_text(seed=5).  The judge
of every Stream is Python's lzma module (stock liblzma)."""
import lzma
import os
import shutil
import subprocess

import numpy as np
import pytest

import _single_block as sb

pytestmark = pytest.mark.gpu

OPTIONS_ERROR, DATA_ERROR, BUF_ERROR = 8, 9, 10
K = 1024
BS = 1 << 20
N4 = 3 * BS + 300 * K + 7             # four segments, the last one odd-length


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


def rnd(n, s):
    return np.random.default_rng(s).integers(0, 256, n, dtype=np.uint8).tobytes()


def _opts(**kw):
    import xz_amd
    op = xz_amd.preset_options(6)
    op.enc_span_bits = 200000           # several encode spans per segment of 1 MiB
    for k, v in kw.items():
        setattr(op, k, v)
    return op


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _ref_ok(xz, data):
    """stock liblzma decodes the Stream to `data`"""
    try:
        return lzma.decompress(xz, format=lzma.FORMAT_XZ) == data
    except lzma.LZMAError:
        return False


def _chains(xz):
    """[(offset, length, control bytes)] of the chunk chains of a single-Block Stream: the LZMA2 data behind the 24 bytes of
    Stream Header and Block Header, cut at every chunk that resets the dictionary, up to the end marker"""
    p, out = 24, []
    while xz[p] != 0:
        ctl = xz[p]
        if ctl == 0x01 or ctl >= 0xE0:
            out.append([p, 0, []])
        assert out, "the first chunk does not reset the dictionary"
        out[-1][2].append(ctl)
        if ctl >= 0x80:
            p += (6 if ctl >= 0xC0 else 5) + ((xz[p + 3] << 8) | xz[p + 4]) + 1
        else:
            assert ctl in (1, 2)
            p += 3 + ((xz[p + 1] << 8) | xz[p + 2]) + 1
        out[-1][1] = p - out[-1][0]
    return [tuple(c) for c in out]


def _seg_bytes(xz, b):
    return xz[b.out_offset: b.out_offset + b.total_size]


def _single(enc, data, **kw):
    kw.setdefault("opts", _opts())
    kw.setdefault("block_size", BS)
    out, binfo = enc.encode(_cuda(data), single=True, **kw)
    return _bytes(out), binfo


class _Info:
    """a block info that can be edited"""

    def __init__(self, b):
        self.unpadded_size, self.uncompressed_size = b.unpadded_size, b.uncompressed_size
        self.out_offset, self.total_size = b.out_offset, b.total_size


def _tamper(raw, offsets):
    t = bytearray(raw)
    for p in offsets:
        t[p] ^= 0x5A
    return bytes(t)


# ---- 1: framing --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("check", [1, 4, 0])
@pytest.mark.parametrize("case", ["last_of_1_byte", "one_segment", "empty", "segment_4k", "batches"])
def test_framing_is_that_of_lzma_easy_encoder(text, monkeypatch, case, check):
    import xz_amd
    seg = 256 * K
    data = {"last_of_1_byte": text[:2 * seg + 1], "one_segment": text[:200 * K], "empty": b"", "segment_4k": text[:3 * 4096 + 1712],
            "batches": text[:2 * BS + 300 * K + 7]}[case]
    if case == "segment_4k":
        seg = 4096                      # below the 64 KiB seed piece
    if case == "batches":
        seg = 512 * K
        monkeypatch.setenv("XZAMD_BATCH_MIB", "1")
    monkeypatch.setenv("XZAMD_SEGMENT_KIB", str(seg >> 10))
    want, _ = sb.lzma_encode(data, 6, check=check)
    e = xz_amd.Encoder()
    try:
        got, binfo = e.encode(_cuda(data), preset=6, block_size=seg, check=check, single=True)
        got = _bytes(got)
        if case == "batches":
            assert e.stats().batches >= 3
    finally:
        e.close()
    assert got == want
    assert _ref_ok(got, data)
    assert len(binfo) == (len(data) + seg - 1) // seg
    if data:
        assert [(b.out_offset, b.total_size) for b in binfo] == [(c[0], c[1]) for c in _chains(got)]
        assert sum(b.uncompressed_size for b in binfo) == len(data) and binfo[-1].uncompressed_size == (len(data) - 1) % seg + 1


# ---- 2: verdicts -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def four(enc, text):
    """(data, chains, block infos) of a 4-segment encode (no resume table kept)"""
    import xz_amd
    data = text[:N4]
    out, binfo = enc.encode(_cuda(data), opts=_opts(), block_size=BS, flags=xz_amd.F_SEGMENTS)
    return data, _bytes(out), binfo


@pytest.mark.parametrize("k", [0, 2, 3])
def test_verdicts_name_the_tampered_segment(enc, four, k):
    data, raw, binfo = four
    assert enc.verify_chains(_cuda(raw), binfo, _cuda(data), opts=_opts()) == ["none"] * 4
    broken = _tamper(raw, [binfo[k].out_offset + binfo[k].total_size // 2])
    steps = enc.verify_chains(_cuda(broken), binfo, _cuda(data), opts=_opts())
    print("steps", steps, enc.verify_report())
    assert steps[k] != "none" and [s for i, s in enumerate(steps) if i != k] == ["none"] * 3
    assert enc.verify_report()["first_bad_block"] == k
    # without the original: grammar, decode and the segment's CRC
    steps = enc.verify_chains(_cuda(broken), binfo, None, opts=_opts())
    assert steps[k] != "none" and [s for i, s in enumerate(steps) if i != k] == ["none"] * 3


def test_verdicts_truncated_chain_and_wrong_crc_and_wrong_original(enc, four):
    data, raw, binfo = four
    cut = [_Info(b) for b in binfo]
    cut[1].total_size -= 1
    assert enc.verify_chains(_cuda(raw), cut, _cuda(data), opts=_opts()) == ["none", "grammar", "none", "none"]
    # a 0x00 where a chunk should start (the first control byte of chain 2), and a chain that runs into the next one
    assert enc.verify_chains(_cuda(raw[: binfo[2].out_offset] + b"\0" + raw[binfo[2].out_offset + 1:]), binfo,
                             _cuda(data), opts=_opts())[2] == "grammar"
    longer = [_Info(b) for b in binfo]
    longer[0].total_size += 1
    assert enc.verify_chains(_cuda(raw), longer, _cuda(data), opts=_opts())[0] == "grammar"
    crc = [_Info(b) for b in binfo]
    crc[3].unpadded_size ^= 1
    assert enc.verify_chains(_cuda(raw), crc, _cuda(data), opts=_opts()) == ["none", "none", "none", "check"]
    other = bytearray(data)
    other[BS + 5000] ^= 0x20
    assert enc.verify_chains(_cuda(raw), binfo, _cuda(bytes(other)), opts=_opts()) == ["none", "compare", "none", "none"]


def test_verdict_units(enc, text):
    import xz_amd
    data = text[:N4]
    d = _cuda(data)
    out, binfo = enc.encode(d, opts=_opts(), block_size=BS, flags=xz_amd.F_SEGMENTS)
    spans = enc.stats().enc_spans
    assert spans > 4
    # no table kept: a unit at the first chunk of every chain and at every later state reset that carries the properties
    assert enc.debug_resume_records() == 0
    assert enc.verify_chains(out, binfo, d, opts=_opts()) == ["none"] * 4
    rep = enc.verify_report()
    resets = sum(1 + sum(1 for c in ctl[1:] if c >= 0xC0) for _, _, ctl in _chains(b"\0" * 24 + _bytes(out) + b"\0"))
    print("verify report", rep, "state resets", resets)
    assert not rep["table_used"] and rep["units"] == resets and 4 <= resets < spans and rep["blocks"] == 4
    # with the table of encode(single, keep_resume): units = encode spans; the records name segments
    xz, sinfo = enc.encode(d, opts=_opts(), block_size=BS, single=True, keep_resume=True)
    assert enc.debug_resume_records() == spans
    assert [(b.out_offset - 24, b.total_size) for b in sinfo] == [(b.out_offset, b.total_size) for b in binfo]
    assert enc.verify_chains(xz[24:], [_shift(b, -24) for b in sinfo], d, opts=_opts()) == ["none"] * 4
    rep = enc.verify_report()
    print("verify report", rep)
    assert rep["table_used"] and rep["units"] == spans and 0 < rep["records_used"] <= spans
    # a defect is still named with the table
    broken = _cuda(_tamper(_bytes(xz), [sinfo[2].out_offset + sinfo[2].total_size // 2]))
    steps = enc.verify_chains(broken[24:], [_shift(b, -24) for b in sinfo], d, opts=_opts())
    assert steps[2] != "none" and steps[:2] + steps[3:] == ["none"] * 3 and enc.verify_report()["table_used"]


def _shift(b, by):
    i = _Info(b)
    i.out_offset += by
    return i


def test_incompressible_segment_verifies(enc, text):
    """A segment of random bytes between two of text.  At these sizes (segments of 1 MiB and of 512 KiB, bytes uniform below
    256 ... 224: measured) the two-phase coder stores every piece of such a segment raw and the chain stays within the bound, so
    the segment does not take the stored form of the layout (blocks_stored stays 0): its chain is uncompressed chunks all the
    same, and it verifies as "none" with the units of the kept table around it."""
    data = text[:BS] + rnd(BS, 7) + text[BS:BS + 300 * K]
    d = _cuda(data)
    xz, binfo = enc.encode(d, opts=_opts(), block_size=BS, single=True, keep_resume=True)
    raw = _bytes(xz)
    ctl = _chains(raw)[1][2]
    assert ctl[0] == 0x01 and set(ctl[1:]) == {0x02} and binfo[1].total_size > BS
    print("blocks_stored", enc.stats().blocks_stored, "records", enc.debug_resume_records())
    assert enc.verify_chains(xz[24:], [_shift(b, -24) for b in binfo], d, opts=_opts()) == ["none"] * 3
    rep = enc.verify_report()
    print("verify report", rep)
    assert rep["table_used"] and rep["first_bad_step"] == "none" and rep["units"] >= 3
    assert _ref_ok(raw, data)


# ---- 3: repair, forced -------------------------------------------------------------------------------------------

def _forced(enc, data, monkeypatch, opts=None, rung2=False, **kw):
    """encode(single=True, repair=True) with segments 0 and 2 rejected by the test knob, and the plain single encode"""
    opts = opts or _opts()
    plain, pinfo = _single(enc, data, opts=opts, **kw)
    monkeypatch.setenv("XZAMD_TEST_REPAIR_REJECT", "0,2")
    if rung2:
        monkeypatch.setenv("XZAMD_TEST_REPAIR_RUNG", "2")
    try:
        xz, binfo = _single(enc, data, opts=opts, repair=True, **kw)
    finally:
        monkeypatch.delenv("XZAMD_TEST_REPAIR_REJECT", raising=False)
        monkeypatch.delenv("XZAMD_TEST_REPAIR_RUNG", raising=False)
    rep = enc.repair_report()
    print("repair report", rep, "verify report", enc.verify_report())
    return xz, binfo, rep, plain, pinfo


@pytest.mark.parametrize("rung2", [False, True])
def test_encode_single_repair_forced(enc, text, monkeypatch, rung2):
    data = text[:N4]
    xz, binfo, rep, plain, pinfo = _forced(enc, data, monkeypatch, rung2=rung2)
    assert _ref_ok(xz, data)
    assert rep["blocks"] == 4 and rep["blocks_bad"] == 2 and rep["passes"] >= 2
    assert (rep["blocks_reencoded"], rep["blocks_stored"]) == ((0, 2) if rung2 else (2, 0))
    assert enc.verify_report()["first_bad_step"] == "none"
    assert xz != plain
    for k in (1, 3):
        assert _seg_bytes(xz, binfo[k]) == _seg_bytes(plain, pinfo[k]), k
        assert (binfo[k].unpadded_size, binfo[k].uncompressed_size) == (pinfo[k].unpadded_size, pinfo[k].uncompressed_size)
    chains = _chains(xz)
    assert [(b.out_offset, b.total_size) for b in binfo] == [(c[0], c[1]) for c in chains]
    for k in (0, 2):
        if rung2:
            assert chains[k][2][0] == 0x01 and set(chains[k][2][1:]) == {0x02}
            assert binfo[k].total_size == BS + 3 * 16
        else:
            assert chains[k][2][0] >= 0xE0 and _seg_bytes(xz, binfo[k]) != _seg_bytes(plain, pinfo[k])
    if rung2:
        assert len(xz) > len(plain)


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


def test_encode_single_repair_forced_pb4_falls_back_to_the_fast_parser(enc, monkeypatch):
    data = _records16(600 * K, 3)
    xz, binfo, rep, plain, _ = _forced(enc, data, monkeypatch, opts=_opts(lc=0, lp=4, pb=4))
    assert _ref_ok(xz, data)
    assert rep["blocks"] == 1 and rep["blocks_bad"] == 1 and rep["blocks_reencoded"] == 1 and rep["blocks_stored"] == 0
    assert xz != plain and [(b.out_offset, b.total_size) for b in binfo] == [(c[0], c[1]) for c in _chains(xz)]


# ---- 4: no-op ----------------------------------------------------------------------------------------------------

def test_repair_without_a_bad_segment_changes_nothing(enc, text):
    data = text[:N4]
    plain, pinfo = _single(enc, data)
    xz, binfo = _single(enc, data, repair=True)
    rep = enc.repair_report()
    assert xz == plain and rep["blocks_bad"] == 0 and rep["passes"] == 1 and rep["blocks"] == 4
    assert [(b.out_offset, b.total_size) for b in binfo] == [(b.out_offset, b.total_size) for b in pinfo]
    assert enc.verify_report()["table_used"]
    xz, _ = _single(enc, data, verify=True)
    assert xz == plain and enc.verify_report()["first_bad_step"] == "none"


# ---- 5: all or nothing -------------------------------------------------------------------------------------------

def test_repair_chains_is_all_or_nothing(enc, four, monkeypatch):
    import torch
    import xz_amd
    data, raw, binfo = four
    broken = _tamper(raw, [binfo[1].out_offset + binfo[1].total_size // 2])
    monkeypatch.setenv("XZAMD_TEST_REPAIR_RUNG", "2")        # the stored chain is larger than the coded one
    need = len(raw) - binfo[1].total_size + BS + 3 * 16
    buf = torch.zeros(need - 1, dtype=torch.uint8, device="cuda")
    buf[: len(broken)] = _cuda(broken)
    infos = [_Info(b) for b in binfo]
    with pytest.raises(xz_amd.XzAmdError) as ei:
        enc.repair_chains(buf, len(broken), infos, _cuda(data), opts=_opts())
    assert ei.value.code == BUF_ERROR and ei.value.new_size == need
    assert _bytes(buf[: len(broken)]) == broken
    assert [(b.out_offset, b.total_size, b.unpadded_size, b.uncompressed_size) for b in ei.value.block_infos] == \
           [(b.out_offset, b.total_size, b.unpadded_size, b.uncompressed_size) for b in binfo]
    # ... and with the one byte more it goes through
    buf = torch.zeros(need, dtype=torch.uint8, device="cuda")
    buf[: len(broken)] = _cuda(broken)
    view, ninfo, rep = enc.repair_chains(buf, len(broken), infos, _cuda(data), opts=_opts())
    assert view.numel() == need and rep["blocks_bad"] == 1 and rep["blocks_stored"] == 1
    fixed = _bytes(view)
    assert _seg_bytes(fixed, ninfo[0]) == _seg_bytes(raw, binfo[0])
    for k in (2, 3):
        assert _seg_bytes(fixed, ninfo[k]) == _seg_bytes(raw, binfo[k]) and ninfo[k].out_offset > binfo[k].out_offset
    assert enc.verify_chains(view, ninfo, _cuda(data), opts=_opts()) == ["none"] * 4


# ---- 6: the real defect ------------------------------------------------------------------------------------------

def _defect_inputs(text):
    """inputs A, D, E of tests/test_gpu_repair.py (its generator, copied): Blocks of 1 MiB that begin with incompressible bytes"""
    import _oracle as o
    lorem = o.corpus_lorem(1 << 20)
    lorem = lorem if isinstance(lorem, bytes) else bytes(lorem)
    return {
        "A": (rnd(512 * K, 1) + lorem[:512 * K], BS),
        "B": (text[:BS] + rnd(512 * K, 1) + lorem[:512 * K] + text[BS:BS + 300 * K], BS),
        "D": (rnd(384 * K, 2) + text[:640 * K], BS),
        "E": (rnd(640 * K, 2) + text[:384 * K], BS),
    }


_REJECTED = {}                         # input name -> the unrepaired single-Block Stream was rejected by liblzma


@pytest.mark.parametrize("name", ["A", "D", "E"])
def test_encode_single_real_defect(enc, text, name):
    """A segment that begins with >= ~320 KiB of incompressible bytes: the two-phase encoder writes its first LZMA chunk
    without the properties byte, and the chain is byte for byte the payload of the MT Block that shows the defect
    (profiles/repair_small_streams.txt: all five MT twins rejected on the device).  Whether or not an input shows it, verify
    and repair must agree with stock liblzma; test_real_defect_is_still_shown counts the rejections."""
    import xz_amd
    data, bs = _defect_inputs(text)[name]
    d = _cuda(data)
    plain, _ = enc.encode(d, preset=6, block_size=bs, single=True)
    plain = _bytes(plain)
    bad = not _ref_ok(plain, data)
    _REJECTED[name] = bad
    print(name, "unrepaired Stream rejected by liblzma:", bad)
    if bad:
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, preset=6, block_size=bs, single=True, verify=True)
        assert ei.value.code == DATA_ERROR
        assert _bytes(ei.value.stream) == plain                          # *out_size is still the framed Stream
        assert enc.verify_report()["first_bad_block"] == 0
    else:
        enc.encode(d, preset=6, block_size=bs, single=True, verify=True)
    xz, binfo = enc.encode(d, preset=6, block_size=bs, single=True, repair=True)
    xz = _bytes(xz)
    rep = enc.repair_report()
    print(name, "repair report", rep)
    assert _ref_ok(xz, data)
    assert rep["blocks_bad"] == (1 if bad else 0)
    if bad:
        first_lzma = next(c for c in _chains(xz)[0][2] if c >= 0x80)
        assert first_lzma >= 0xC0


def test_real_defect_is_still_shown():
    """At least 2 of the 3 unrepaired Streams above must have been rejected by stock liblzma -- fewer would mean the inputs no
    longer show the defect: a finding, not a reason to pass.  (Measured: all three rejected.)"""
    assert len(_REJECTED) == 3, "runs behind test_encode_single_real_defect[A, D, E]"
    rejected = [n for n, bad in _REJECTED.items() if bad]
    assert len(rejected) >= 2, f"the device no longer shows the stored-prefix defect on these inputs: rejected {rejected}"


# ---- 7: the lzma_* front end -------------------------------------------------------------------------------------

def test_front_end_repairs_the_segments_of_its_jobs(enc, text, monkeypatch):
    """lzma_easy_encoder / lzma_code with XZAMD_REPAIR=1: input B, segment 1 is the one with the defect"""
    data, bs = _defect_inputs(text)["B"]
    monkeypatch.setenv("XZAMD_SEGMENT_KIB", str(bs >> 10))
    monkeypatch.delenv("XZAMD_REPAIR", raising=False)
    plain, pinfo = enc.encode(_cuda(data), preset=6, block_size=bs, single=True)
    plain = _bytes(plain)
    out0, _ = sb.lzma_encode(data, 6, piece=100000)
    assert out0 == plain                                                 # unset: today's bytes
    defect = not _ref_ok(plain, data)
    print("unrepaired Stream rejected by liblzma:", defect)
    monkeypatch.setenv("XZAMD_REPAIR", "1")
    try:
        out, _ = sb.lzma_encode(data, 6, piece=100000)
    finally:
        monkeypatch.delenv("XZAMD_REPAIR", raising=False)
    assert defect, "input B no longer shows the stored-prefix defect in its second segment"
    assert _ref_ok(out, data)
    chains, pchains = _chains(out), _chains(plain)
    assert len(chains) == len(pchains) == 3
    for k in (0, 2):
        assert out[chains[k][0]: chains[k][0] + chains[k][1]] == plain[pchains[k][0]: pchains[k][0] + pchains[k][1]], k
    assert out[chains[1][0]: chains[1][0] + chains[1][1]] != plain[pchains[1][0]: pchains[1][0] + pchains[1][1]]
    assert next(c for c in chains[1][2] if c >= 0x80) >= 0xC0


def test_front_end_repairs_under_flushes(text, monkeypatch):
    """the same input with a LZMA_SYNC_FLUSH in the middle of the bad segment and a LZMA_FULL_FLUSH later: a short segment, two
    Blocks, Checks folded from the rewritten segment tables"""
    data, bs = _defect_inputs(text)["B"]
    monkeypatch.setenv("XZAMD_SEGMENT_KIB", str(bs >> 10))
    monkeypatch.setenv("XZAMD_REPAIR", "1")
    mid = bs + 200 * K                                                   # inside the bad segment
    try:
        flushed, cuts = sb.lzma_encode(data, 6, piece=100000, flushes=[(mid, sb.SYNC_FLUSH), (2 * bs + 100 * K, sb.FULL_FLUSH)])
    finally:
        monkeypatch.delenv("XZAMD_REPAIR", raising=False)
    assert _ref_ok(flushed, data)
    assert len(sb.parse_blocks(flushed)) == 2
    d = lzma.LZMADecompressor(format=lzma.FORMAT_XZ)
    assert d.decompress(flushed[: cuts[0]]) == data[:mid]                # everything up to the flush is decodable


# ---- 8: the command line -----------------------------------------------------------------------------------------

def test_xz_T1_under_the_interposer_with_repair(tmp_path, text):
    """`xz -T1 -6` under LD_PRELOAD=libxz_amd_preload.so with XZAMD_REPAIR=1 on input A (one segment: the file is shorter than
    the default segment); the stock `xz -d`, without the preload, restores it"""
    import xz_amd
    xz = shutil.which("xz")
    if not xz:
        pytest.skip("no xz binary")
    pre = os.path.join(os.path.dirname(xz_amd.LIB_PATH), "libxz_amd_preload.so")
    assert os.path.exists(pre), "libxz_amd_preload.so not built"
    data, _ = _defect_inputs(text)["A"]
    src = tmp_path / "input.bin"
    src.write_bytes(data)
    env = dict(os.environ, LD_PRELOAD=pre, XZ_AMD_VERBOSE="1", XZAMD_REPAIR="1")
    p = subprocess.run(["timeout", "-k", "10", "120", xz, "-T1", "-6", "-c", str(src)], capture_output=True, env=env, timeout=150)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"-> GPU" in p.stderr, p.stderr.decode()[-2000:]
    env2 = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    d = subprocess.run([xz, "-dc"], input=p.stdout, capture_output=True, timeout=120, env=env2)
    assert d.returncode == 0 and d.stdout == data, d.stderr.decode()[-2000:]
    assert _ref_ok(p.stdout, data)


# ---- 9: flags ----------------------------------------------------------------------------------------------------

def test_flags(enc, text):
    import xz_amd
    d = _cuda(text[:300 * K])
    bad = [dict(single=True, blocks_only=True), dict(single=True, flags=xz_amd.F_SEGMENTS), dict(single=True, check=xz_amd.CHECK_SHA256),
           dict(single=True, opts=_opts(bcj=xz_amd.BCJ_X86)), dict(single=True, flags=0x80000000),
           # pinned as errors before this feature, and still errors
           dict(flags=xz_amd.F_REPAIR | xz_amd.F_SEGMENTS, check=xz_amd.CHECK_CRC32), dict(flags=xz_amd.F_KEEP_RESUME | xz_amd.F_SEGMENTS),
           dict(flags=xz_amd.F_VERIFY | xz_amd.F_SEGMENTS), dict(flags=0x80000000 | xz_amd.F_REPAIR | xz_amd.F_SEGMENTS)]
    for kw in bad:
        kw.setdefault("opts", _opts())
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, block_size=BS, **kw)
        assert ei.value.code == OPTIONS_ERROR, kw
