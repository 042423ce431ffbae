"""The device LZMA2 decoder (k_dec_scan, k_dec_units) against the real liblzma on crafted symbol streams.

tests/_lzma2_craft.py writes LZMA2 data symbol by symbol -- every model geometry, every chunk succession, the size
extremes, distances and copy lengths around every limit, range-coder framing defects; each case valid up to one chosen
point.  tests/golden/lzma2_craft.json holds what the real liblzma said about each (tests/golden/make_craft_golden.py,
checked on the CPU by tests/test_lzma2_craft.py).  Here the cases go to the device, assembled into a few multi-Block
Streams with known-good control Blocks between the bad ones: the same verdict, the same bytes, the step that names the
defect ("grammar" for what the chunk scan must catch, "decode" for what only decoding shows), and no leak of a bad Block
into its neighbours.  Every rejected case stands behind a good Block of more than 4 KiB and reaches at most a few bytes
past its limit; the far-distance cases are ordinary hostile input the decoder documents as rejected.
"""
import ctypes as C
import hashlib
import json
import os

import pytest

import _lzma2_craft as craft

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzma2_craft.json")
SLACK = 4096
FILL = 0xA5
DATA_ERROR = 9


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    e = xz_amd.Encoder()
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def accepted(golden):
    """name -> the reference accepts the case.  The plaintext of an accepted case is the reference's output (by its
    recorded size and SHA-256), so every byte compared below is liblzma's."""
    acc = {}
    for c in craft.cases():
        g = golden["cases"][c.name]
        assert hashlib.sha256(c.stream()).hexdigest() == g["stream_sha256"], c.name
        acc[c.name] = g["ret"] == 1
        if acc[c.name]:
            assert (len(c.plain), hashlib.sha256(c.plain).hexdigest()) == (g["size"], g["sha256"]), c.name
    acc["control"] = True
    assert set("ABCDEFG") == {c.section for c in craft.cases()} and len(acc) >= 381
    return acc


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _good_stream(accepted, check):
    """(Stream, plaintext, Blocks) of every accepted case"""
    cs = [c for c in craft.cases() if accepted[c.name]]
    raw, _ = craft.frame([c.block() for c in cs], check)
    return raw, b"".join(c.plain for c in cs), len(cs)


def _small_stream():
    """The two unit-table overflow Blocks between controls: no Block above 8 KiB, so the unit table has 9 rows a Block"""
    by, ctl = craft.by_name(), craft.control()
    cs = [ctl, by["C-4k-block-48-dict-resets"], ctl, by["C-4k-block-48-C0-chunks"], ctl]
    assert max(c.usize for c in cs) // 4096 + 8 == 9
    raw, _ = craft.frame([c.block() for c in cs], craft.CHECK_CRC32)
    return raw, b"".join(c.plain for c in cs), len(cs)


def _want_step(c, accepted):
    return "none" if accepted[c.name] else c.step if not c.record_only else "decode"


# ---------------------------------------------------------------- accepted cases, plain decode
@pytest.mark.parametrize("check", [craft.CHECK_NONE, craft.CHECK_CRC32, craft.CHECK_SHA256])
def test_accepted_cases_decode_to_the_reference_bytes(enc, accepted, check):
    import torch
    import xz_amd
    raw, want, nblocks = _good_stream(accepted, check)
    xz = _cuda(raw)
    got, nb = enc.decode(xz, len(want) + SLACK)
    assert nb == nblocks and _bytes(got) == want
    got, nb = enc.decode_file(xz, len(want) + SLACK)
    assert nb == nblocks and _bytes(got) == want
    # the C entry on a tensor of the test's own: nothing behind the decoded size is written
    out = torch.full((len(want) + SLACK,), FILL, dtype=torch.uint8, device="cuda")
    osz, mm, nbk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    torch.cuda.synchronize()
    rc = xz_amd.lib().xzamd_stream_decode_device(enc._ctx, C.c_void_p(xz.data_ptr()), xz.numel(), C.c_void_p(out.data_ptr()),
                                                 out.numel(), C.byref(osz), None, 0, C.byref(mm), C.byref(nbk), None)
    assert (rc, osz.value, nbk.value) == (0, len(want), nblocks)
    assert _bytes(out[: osz.value]) == want
    assert bool((out[osz.value:] == FILL).all())


def test_full_unit_table_of_a_plain_decode(enc):
    """48 dictionary resets in a Block whose unit table has 9 rows: further resets stay inside the last unit"""
    raw, want, nblocks = _small_stream()
    got, nb = enc.decode(_cuda(raw), len(want) + SLACK)
    assert nb == nblocks and _bytes(got) == want
    units, blocks, split = enc.debug_decode_units()
    assert (blocks, split) == (nblocks, 2) and units == 3 + 9 + 1


# ---------------------------------------------------------------- accepted cases, verification decode
def test_accepted_cases_verify_as_good(enc, accepted):
    raw, want, nblocks = _good_stream(accepted, craft.CHECK_NONE)
    xz, orig = _cuda(raw), _cuda(want)
    got, nb = enc.decode(xz, len(want) + SLACK, expected=orig)
    assert nb == nblocks and _bytes(got) == want
    assert enc.verify_blocks(xz, orig) == ["none"] * nblocks
    assert enc.verify_blocks(xz) == ["none"] * nblocks


def test_unit_table_overflow_of_a_verification_decode_is_no_defect(enc):
    """more than 9 state resets in a Block: the scan reports DEC_UNIT_OVERFLOW, the host decodes one unit per Block"""
    raw, want, nblocks = _small_stream()
    xz, orig = _cuda(raw), _cuda(want)
    got, nb = enc.decode(xz, len(want) + SLACK, expected=orig)
    assert nb == nblocks and _bytes(got) == want
    assert enc.debug_decode_units() == (nblocks, nblocks, 0)
    assert enc.verify_blocks(xz, orig) == ["none"] * nblocks
    assert enc.verify_blocks(xz) == ["none"] * nblocks


# ---------------------------------------------------------------- all cases in one Stream
@pytest.fixture(scope="module")
def everything(accepted):
    """(Stream, original with zeros for the rejected Blocks, [(case, is_control)])"""
    seq = craft.interleave(craft.cases(), accepted)
    for k, (c, _) in enumerate(seq):
        if not accepted[c.name]:
            assert k > 0 and seq[k - 1][1] and k + 1 < len(seq)      # never first or last, a control Block in front
    raw, _ = craft.frame([c.block(b"") for c, _ in seq], craft.CHECK_NONE)
    orig = b"".join(c.plain if accepted[c.name] else b"\0" * c.usize for c, _ in seq)
    return raw, orig, seq


@pytest.mark.parametrize("with_original", [False, True])
def test_every_case_gets_the_reference_verdict_and_its_step(enc, accepted, everything, with_original):
    raw, orig, seq = everything
    steps = enc.verify_blocks(_cuda(raw), _cuda(orig) if with_original else None)
    assert len(steps) == len(seq)
    wrong = [(c.name, got, _want_step(c, accepted)) for (c, _), got in zip(seq, steps) if got != _want_step(c, accepted)]
    assert wrong == []
    assert sum(1 for s in steps if s != "none") == sum(1 for v in accepted.values() if not v)


# ---------------------------------------------------------------- forward decode up to a defect
@pytest.mark.parametrize("name", craft.FORWARD_CASES)
def test_forward_decode_delivers_the_blocks_in_front_of_the_defect(enc, golden, name):
    import xz_amd
    g = golden["forward"][name]
    raw, front = craft.forward_stream(name)
    assert hashlib.sha256(raw).hexdigest() == g["stream_sha256"]
    assert (len(front), hashlib.sha256(front).hexdigest()) == (g["front_size"], g["front_sha256"])
    with pytest.raises(xz_amd.XzAmdError) as e:
        enc.decode_forward(_cuda(raw), len(front) + 65536)
    assert e.value.code == g["ret"] == DATA_ERROR
    assert _bytes(e.value.partial) == front and e.value.report["blocks_delivered"] == 3


# ---------------------------------------------------------------- bare chains
@pytest.mark.parametrize("dict_size", [8 * craft.MIB, 4 * craft.MIB, 8192, 4096])
def test_bare_chains_get_the_same_verdicts(enc, accepted, dict_size):
    """the same LZMA2 data without its end marker, as the segments of a single-Block Stream are verified"""
    import xz_amd
    cs = [c for c in craft.cases() if c.dict_size == dict_size]
    assert cs
    chain_ok = {c.name: (accepted[c.name] if c.chain_intent == c.intent else c.chain_intent == "accept") for c in cs}
    chain_ok["control"] = True
    seq = craft.interleave(cs, chain_ok)
    buf, rows = craft.bare_chains([c.chain for c, _ in seq], [c.usize for c, _ in seq])
    orig = b"".join(c.plain if chain_ok[c.name] else b"\0" * c.usize for c, _ in seq)
    want = ["none" if chain_ok[c.name] else c.step if not c.record_only else "decode" for c, _ in seq]
    if dict_size == 8 * craft.MIB:
        assert "grammar" in want and "decode" in want and want[[c.name for c, _ in seq].index("B-bad-data-behind-end-marker")] == "grammar"
    opts = xz_amd.preset_options(6)
    opts.dict_size = dict_size
    for original in (None, _cuda(orig)):
        steps = enc.verify_chains(_cuda(buf), rows, original, opts=opts, check=xz_amd.CHECK_NONE)
        wrong = [(c.name, got, w) for (c, _), got, w in zip(seq, steps, want) if got != w]
        assert wrong == []
