"""The device on the composite Blocks of tests/_composite.py: inputs whose compressibility changes at the
boundaries the back end cuts at, so that the stored-piece loop of k_model_walk, its three reset flags, the carry kinds of
k_model_chain and the control bytes of k_rc_chunks are all exercised.  One case = one named input at one setting, Blocks of
1 MiB.  Per case:

  parity    the Stream is byte-identical to the oracle's; at the stressed preset-6 plan also the stored-piece flags and the
            carry kinds, stage by stage;
  validity  the verdict of the independent chunk walker (tests/_lzma2_grammar.py) per Block equals the record that
            tests/test_composite_oracle.py pins for the oracle (_composite.EXPECTED_DEFECT); the reference decoder returns
            the input where every Block passes and rejects the Stream where one has the stored-prefix defect;
  verify    verify_blocks says "grammar" for exactly the flagged Blocks, with and without the original, and
            encode(verify=True) raises XZAMD_DATA_ERROR exactly when one is flagged;
  repair    encode(repair=True) gives a Stream whose every Block passes the walker, that decodes to the input, reports
            blocks_bad = the number of flagged Blocks, and is the plain Stream when that number is 0.

The assertions read "valid, or exactly this shape and reported": on the day the defect is fixed only the record changes.
"""
import numpy as np
import pytest

import _composite as cp
import _lzma2_grammar as g
import _oracle as o

pytestmark = pytest.mark.gpu

DATA_ERROR = 9
BS = cp.MIB


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    e = xz_amd.Encoder()
    yield e
    e.close()


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _two_phase(opts):
    return bool(opts.gpu_parser and opts.gpu_sa_window and opts.span_cost and opts.enc_span_bits)


def _stages(enc, data, prm, nb):
    """stored-piece flags and carry kinds of the encode that just ran against the oracle's, Block by Block"""
    spb, esb = BS // 65536 + 2, BS // (256 << 10) + 1
    cnt = enc.debug_fetch(6, nb)
    ecnt = enc.debug_fetch(12, nb)
    gpi = enc.debug_fetch(13, 16 * nb * spb).reshape(nb, spb, 16)
    gcarry = enc.debug_fetch(16, nb * esb).reshape(nb, esb)
    for b in range(nb):
        blk = data[b * BS:(b + 1) * BS]
        starts, estarts = o.orc_piece_plan(blk, prm)
        assert cnt[b] == len(starts) and ecnt[b] == len(estarts), ("plan", b)
        _, _, oprice, ocarry = o.orc_two_phase_debug(blk, prm, len(starts), len(estarts))
        plen = np.diff(np.append(starts, len(blk)))
        oraw = (plen >= 32768) & (oprice // 128 >= plen)
        assert (gpi[b, :cnt[b], 8 + 5] == oraw).all(), ("stored pieces", b, gpi[b, :cnt[b], 8 + 5], oraw)
        assert (gcarry[b, 1:ecnt[b]] == ocarry[1:]).all(), ("carry kinds", b, gcarry[b, :ecnt[b]], ocarry)


@pytest.mark.parametrize("setting", cp.SETTINGS)
@pytest.mark.parametrize("name", list(cp.NAMED))
def test_composite_block(enc, name, setting):
    import xz_amd
    data = cp.named(name)
    d = _cuda(data)
    opts = cp.options_for(setting)
    nb = (len(data) + BS - 1) // BS
    flagged = [k in cp.expected_defect(setting, BS, name) for k in range(nb)]

    # ---- parity
    out, _ = enc.encode(d, opts=opts, block_size=BS)
    got = _bytes(out)
    st = enc.stats()
    if _two_phase(opts):
        assert st.span_cost_used == opts.span_cost
        prm = o.params_for_gpu_options(opts, span_cost_used=st.span_cost_used)
    else:
        prm = o.params_for_gpu_options(opts)
    if setting == "p6-stress":
        _stages(enc, data, prm, nb)
    want = o.orc_xz_stream(data, prm, BS)
    assert o.first_diff(got, want) == -1, "parity"

    # ---- independent validity
    walks = g.walk_stream(got)
    verdicts = [g.verdict(w) for w in walks]
    print(name, setting, verdicts, [f"{c.control:02X}" for c in walks[0].chunks[:12]])
    assert verdicts == [g.DEFECT if f else g.OK for f in flagged], ("validity", walks)
    rr, dec = o.ref_decode(got, len(data) + 16)
    if any(flagged):
        assert rr == DATA_ERROR, rr
    else:
        assert rr == 1 and dec == data

    # ---- verify
    steps = ["grammar" if f else "none" for f in flagged]
    assert enc.verify_blocks(out, d) == steps
    assert enc.verify_blocks(out) == steps
    if any(flagged):
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.encode(d, opts=opts, block_size=BS, verify=True)
        assert ei.value.code == DATA_ERROR
        assert _bytes(ei.value.stream) == got
    else:
        assert _bytes(enc.encode(d, opts=opts, block_size=BS, verify=True)[0]) == got

    # ---- repair
    fixed, _ = enc.encode(d, opts=opts, block_size=BS, repair=True)
    fixed = _bytes(fixed)
    rep = enc.repair_report()
    assert all(w.ok for w in g.walk_stream(fixed)), g.walk_stream(fixed)
    rr, dec = o.ref_decode(fixed, len(data) + 16)
    assert rr == 1 and dec == data
    assert rep["blocks"] == nb and rep["blocks_bad"] == sum(flagged), rep
    if not any(flagged):
        assert fixed == got


# Single-Block Streams (encode(single=True): the chunk chain of a segment is the payload of the MT Block of the same bytes).
# Preset 6 with its default plan, segments of 1 MiB; what the oracle says of them (EXPECTED_DEFECT["p6"]):
#   r256k+t         one segment, valid: 256 KiB of random bytes in front of text
#   r320k+t         one segment, stored-prefix defect: 320 KiB in front of text
#   r512k+z         one segment, stored-prefix defect: 512 KiB in front of zeros
#   r512k+t512k+l   two segments: the first has the defect (512 KiB in front of text), the second is valid
SINGLE = ("r256k+t", "r320k+t", "r512k+z", "r512k+t512k+l")


class _Info:
    def __init__(self, b, shift=0):
        self.unpadded_size, self.uncompressed_size = b.unpadded_size, b.uncompressed_size
        self.out_offset, self.total_size = b.out_offset + shift, b.total_size


def _chain_walks(raw, infos):
    return [g.walk(raw[b.out_offset: b.out_offset + b.total_size] + b"\0", b.uncompressed_size) for b in infos]


@pytest.mark.parametrize("name", SINGLE)
def test_composite_single_block_chains(enc, name):
    import torch
    import xz_amd
    data = cp.named(name)
    d = _cuda(data)
    opts = cp.options_for("p6")
    nseg = (len(data) + BS - 1) // BS
    flagged = [k in cp.expected_defect("p6", BS, name) for k in range(nseg)]
    assert any(flagged) == (name != SINGLE[0])
    xz, binfo = enc.encode(d, opts=opts, block_size=BS, single=True)
    assert len(binfo) == nseg
    infos = [_Info(b, -24) for b in binfo]
    size = infos[-1].out_offset + infos[-1].total_size         # the chains lie back to back behind the 24 header bytes
    assert infos[0].out_offset == 0 and _bytes(xz)[24 + size] == 0
    raw = _bytes(xz)[24: 24 + size]
    walks = _chain_walks(raw, infos)
    print(name, [g.verdict(w) for w in walks])
    assert [g.verdict(w) for w in walks] == [g.DEFECT if f else g.OK for f in flagged], walks
    for original in (d, None):
        steps = enc.verify_chains(xz[24: 24 + size], infos, original, opts=opts)
        assert steps == ["grammar" if f else "none" for f in flagged], steps
    buf = torch.zeros(len(raw) + (1 << 20), dtype=torch.uint8, device="cuda")
    buf[: len(raw)] = _cuda(raw)
    view, ninfo, rep = enc.repair_chains(buf, len(raw), infos, d, opts=opts)
    fixed = _bytes(view)
    assert rep["blocks_bad"] == sum(flagged), rep
    assert all(w.ok for w in _chain_walks(fixed, ninfo)), _chain_walks(fixed, ninfo)
    assert sum(b.total_size for b in ninfo) == len(fixed)
    rr, dec = o.ref_raw_decode(fixed + b"\0", opts.dict_size, len(data) + 16)
    assert rr == 1 and dec == data
    if not any(flagged):
        assert fixed == raw
