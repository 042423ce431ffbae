"""The rule of the automatic per-Block literal context (DESIGN.md 3.5 "Automatic literal context") on the CPU: the C statement
(xz_amd/csrc/lclp_rule.h, through the stand-in tests/host_stub/stub_xzk_lclp.c) against the numpy model (tests/_auto_lclp.py)
on every calibration class and on the edge Blocks, and the calibration itself against the reference encoder: liblzma through
Python's lzma module, raw {LZMA2 preset 6} with every candidate pair (the helpers of _oracle take no per-option preset encode).
The sizes measured when the constants were chosen are in tests/golden/auto_lclp_ref.json."""
import ctypes as C
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import _auto_lclp as ll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 1 << 20
GOLDEN = os.path.join(ROOT, "tests", "golden", "auto_lclp_ref.json")
_data, _sizes = {}, {}


@pytest.fixture(scope="module")
def crule(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lclp") / "lclp_rule.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-DSTUB_LCLP_RULE_ONLY",
                    os.path.join(ROOT, "tests", "host_stub", "stub_xzk_lclp.c"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.stub_lclp_block.restype = C.c_uint32
    lib.stub_lclp_block.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(block, lc=3, lp=0):
        """((lc, lp) chosen, [candidates], [costs], histogram) of one Block by the C rule"""
        block = bytes(block)
        hist = np.zeros(ll.HIST_SHAPE, dtype=np.uint32)
        cand = np.zeros(15, dtype=np.uint32)
        S = np.zeros(15, dtype=np.uint64)
        nc = C.c_uint32(0)
        v = lib.stub_lclp_block(block, len(block), lc, lp, hist.ctypes.data, cand.ctypes.data, S.ctypes.data, C.byref(nc))
        k = nc.value
        return (v & 255, v >> 8), [(int(c) & 255, int(c) >> 8) for c in cand[:k]], [int(s) for s in S[:k]], hist
    return run


def _class(name):
    if name not in _data:
        _data[name] = bytes(ll.CLASSES[name](SIZE))
        assert len(_data[name]) == SIZE
    return _data[name]


def _agree(crule, block, lc=3, lp=0):
    chosen, cand, S, hist = crule(block, lc, lp)
    mh = ll.joint_hist(block)
    mchosen, mS, ns = ll.rule(mh, lc, lp)
    assert (hist == mh).all()
    assert cand == ll.candidates(lc, lp)
    assert S == mS and chosen == mchosen
    assert int(hist.sum()) == ns == len(ll.ad.sample_offsets(len(block)))
    return chosen


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "xz_amd", "csrc", "lclp_rule.h")).read()
    assert f"#define XZAMD_LL_CELL {ll.CELL}u" in text and f"#define XZAMD_LL_MARGIN {ll.MARGIN}u" in text
    g = json.load(open(GOLDEN))
    assert g["cell"] == ll.CELL and g["margin"] == ll.MARGIN


def test_candidates():
    c = ll.candidates(3, 0)
    assert len(c) == 10 and c[0] == (3, 0) and {(0, 2), (1, 2), (0, 3)} <= set(c)
    assert all(a + b <= 3 and b <= 3 for a, b in c)
    assert len(ll.candidates(2, 2)) == 13 and ll.candidates(2, 2)[0] == (2, 2)
    assert ll.candidates(0, 0) == [(0, 0)]
    assert ll.candidates(4, 0) == [(4, 0)] and ll.candidates(0, 4) == [(0, 4)]      # pairs the statistic cannot price


@pytest.mark.parametrize("name", sorted(ll.CLASSES))
def test_c_rule_equals_model(crule, name):
    chosen = _agree(crule, _class(name))
    print(f"{name}: chosen {chosen}")
    if name in ll.TEXT_CLASSES:
        assert chosen == (3, 0)
    # another job's pair: more candidates, another candidate 0
    _agree(crule, _class(name)[:300 << 10], 2, 2)
    _agree(crule, _class(name)[:70000], 0, 1)


def test_edge_blocks(crule):
    f32 = _class("f32walk")
    pairs0, hists0 = ll.choose_blocks(b"", 4096)
    assert pairs0 == [] and hists0.shape == (0, 8, 8, 256)
    # empty Block: no samples, the job's pair; one byte; shorter than a sample window; exactly one; one more; ragged
    for n in (0, 1, 2, 7, 8, 9, 4095, 4096, 4097, 65535, 65536, 65536 + 31, 65536 + 4096 + 5, 300 << 10):
        for lc, lp in ((3, 0), (1, 2), (2, 2), (4, 0), (0, 4), (1, 3)):
            chosen = _agree(crule, f32[:n], lc, lp)
            if n <= 1 or lc == 4 or lp == 4:
                assert chosen == (lc, lp)
    # prev of offset 0 is 0, of the first byte of a later window the byte in front of the window
    b = bytes([0xFF]) * (65536 + 1)
    h = ll.joint_hist(b)
    assert h[0, 0, 0xFF] == 1 and h[0, 7, 0xFF] == 4096 // 8 and int(h.sum()) == 4097
    _agree(crule, b)
    # all bytes equal: no candidate is cheaper than the job's by the margin
    assert _agree(crule, bytes(100000)) == (3, 0)
    # Blocks of a cut input: the last one ragged
    pairs, hists = ll.choose_blocks(f32[:(1 << 20) - 12345], 256 << 10)
    assert len(pairs) == 4 and hists.shape == (4, 8, 8, 256) and int(hists[3].sum()) == len(ll.ad.sample_offsets((256 << 10) - 12345))


def test_rule_ties_and_margin():
    # a histogram where lp carries everything: byte = offset & 3, so (0, 2) has zero plug-in cost
    x = (np.arange(8192) & 3).astype(np.uint8).tobytes()
    chosen, S, ns = ll.rule(ll.joint_hist(x))
    cands = ll.candidates(3, 0)
    # (0, 2), (1, 2) and (0, 3) all cost cells only; (0, 2) uses the fewest
    assert chosen == (0, 2) and S[cands.index((0, 2))] == 4 * ll.CELL and ns == 4096
    # ties go to fewer literal coders, then to the smaller lp: one byte value only -> every pair costs its used cells
    h = np.zeros(ll.HIST_SHAPE, dtype=np.uint32)
    h[:, 0, 5] = 1000
    S = [ll.cost(h, c, p) for c, p in ll.candidates(3, 0)]
    assert S[0] == ll.CELL and min(S) == ll.CELL and ll.rule(h)[0] == (3, 0)        # (0, 0) ties and is cheaper by nothing
    h2 = np.zeros(ll.HIST_SHAPE, dtype=np.uint32)
    h2[0, 0, 1] = h2[1, 0, 2] = 4000        # two positions, two bytes: lp >= 1 separates them, 1 bit per byte saved
    chosen2, S2, ns2 = ll.rule(h2)
    assert ns2 == 8000 and chosen2 == (0, 1) and S2[0] - S2[ll.candidates(3, 0).index((0, 1))] == 8000 * 256 + 0 * ll.CELL


# ---- calibration against the reference ----------------------------------------------------------------------------------
def _ref_size(data, lc, lp):
    f = [{"id": lzma.FILTER_LZMA2, "preset": 6, "lc": lc, "lp": lp, "pb": 2}]
    return len(lzma.compress(data, format=lzma.FORMAT_RAW, filters=f))


def _sizes_of(name):
    """reference sizes of 1 MiB of the class under every candidate of the default job: encoded once"""
    if name not in _sizes:
        _sizes[name] = {c: _ref_size(_class(name), *c) for c in ll.candidates(3, 0)}
    return _sizes[name]


@pytest.mark.parametrize("name", sorted(ll.CLASSES))
def test_calibration_against_reference(name):
    sizes = _sizes_of(name)
    chosen = ll.rule(ll.joint_hist(_class(name)))[0]
    default, best = sizes[(3, 0)], min(sizes.values())
    noise = 6 * ((SIZE + 65535) // 65536)           # one LZMA2 chunk header per 64 KiB
    print(f"{name}: chosen {chosen} {sizes[chosen]} ({sizes[chosen] / default:.4f}), default {default}, best "
          f"{min(sizes, key=sizes.get)} {best} ({best / default:.4f}); all: "
          + " ".join(f"{c}={s / default:.4f}" for c, s in sizes.items()))
    assert sizes[chosen] <= default + noise
    if name in ll.GAIN_CLASSES:
        assert default - sizes[chosen] >= (default - best) / 2 and chosen != (3, 0)
    if name in ll.TEXT_CLASSES:
        assert chosen == (3, 0)
    # the sizes recorded when the constants were chosen satisfy the same bounds (the liblzma of the day may differ a little)
    g = json.load(open(GOLDEN))["classes"][name]
    gs = {tuple(int(v) for v in k.split(",")): s for k, s in g["sizes"].items()}
    assert set(gs) == set(sizes) and tuple(g["choice"]) == chosen
    assert gs[chosen] <= gs[(3, 0)] + noise
    if name in ll.GAIN_CLASSES:
        assert gs[(3, 0)] - gs[chosen] >= (gs[(3, 0)] - min(gs.values())) / 2
