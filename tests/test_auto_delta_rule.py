"""The rule of the automatic per-Block delta filter (DESIGN.md 3.5 "Automatic delta") through its numpy model
(tests/_auto_delta.py), on the CPU: what it picks for 1 MiB of each of the 20 corpus classes it was calibrated on, that the
reference encoder (the liblzma of oracle/_ref, preset 6) agrees -- no chosen filter makes its output larger, no declined
one would have made it smaller -- the committed log table, and the edge inputs."""
import math

import numpy as np
import pytest

import _auto_delta as ad
import _oracle as o

SIZE = 1 << 20
_cache = {}


def _class(name):
    """(data, chosen, d*) of 1 MiB of a class: generated and analysed once"""
    if name not in _cache:
        data = bytes(ad.CLASSES[name](SIZE))
        assert len(data) == SIZE
        chosen, dstar, _ = ad.choose(data)
        _cache[name] = (data, chosen, dstar)
    return _cache[name]


def test_twenty_classes():
    assert len(ad.CLASSES) == 20 and set(ad.EXPECTED) == set(ad.CLASSES)
    assert sorted(k for k, v in ad.EXPECTED.items() if v) == sorted(
        ["f32sine", "f32two", "pcm16", "int32walk", "rgba", "f32mesh", "f64sine", "structs24", "relocs"])


def test_log_table_is_the_formula():
    want = [int(math.floor(256 * math.log2(1 + m / 256) + 0.5)) for m in range(256)]
    assert ad.T.tolist() == want
    # L on exact powers of two and around them; L(0) = 0
    assert ad.log256([0, 1, 2, 3, 4, 255, 256, 257, 1 << 20, (1 << 20) + (1 << 12)]).tolist() == [
        0, 0, 256, 256 + 150, 512, 7 * 256 + 255, 2048, 2048 + 1, 20 * 256, 20 * 256 + 1]


@pytest.mark.parametrize("name", sorted(ad.CLASSES))
def test_choice_per_class(name):
    _, chosen, _ = _class(name)
    print(f"{name}: chosen {chosen}, expected {ad.EXPECTED[name]}")
    assert chosen == ad.EXPECTED[name]


@pytest.mark.parametrize("name", sorted(ad.CLASSES))
def test_reference_agrees(name):
    if not o.have_ref():
        pytest.skip("reference liblzma not built (oracle/_ref)")
    data, chosen, dstar = _class(name)
    plain = len(o.ref_encode_mt(data, 6))
    filt = len(o.ref_encode_mt_chain(data, 6, 3, delta_dist=dstar))
    print(f"{name}: chosen {chosen}, d* {dstar}, reference plain {plain}, with delta({dstar}) {filt}, ratio {filt / plain:.3f}")
    if chosen:
        assert chosen == dstar and filt <= plain
    else:
        assert filt >= plain


def test_edge_inputs():
    rng = np.random.default_rng(5)
    walk = np.cumsum(rng.integers(-1000, 1001, 70000), dtype=np.int64).astype(np.int32).tobytes()
    # empty: no Block, nothing to choose; one byte: Ns = 1, every S is 0
    dists, hists = ad.choose_blocks(b"", 4096)
    assert dists == [] and hists.shape == (0, 11, 256)
    assert ad.choose(b"\x07")[0] == 0
    # the sample set: whole below 4096 bytes, 4096 of 4097, 4096 + 31 of 65536 + 31
    for n, ns in ((1, 1), (4095, 4095), (4096, 4096), (4097, 4096), (65536 + 31, 4096 + 31), (3 * 65536, 3 * 4096)):
        assert len(ad.sample_offsets(n)) == ns
        h = ad.histograms(walk[:n])
        assert (h.sum(axis=1) == ns).all()
    assert ad.sample_offsets(65536 + 31)[-1] == 65536 + 30
    # 4095 bytes and 4096 + 1 bytes of an int32 walk: delta 4 either way (x[i - d] of a sample may lie outside the sample set)
    assert ad.choose(walk[:4095])[0] == 4 and ad.choose(walk[:4097])[0] == 4 and ad.choose(walk[:65536 + 31])[0] == 4
    # all bytes equal: S(0) = 0, nothing can win
    for v in (0, 0x55):
        chosen, _, h = ad.choose(bytes([v]) * 100000)
        S, ns = ad.costs(h)
        assert chosen == 0 and S[0] == 0 and ns == 2 * 4096
    assert ad.costs(ad.histograms(bytes(70000)))[0] == [0] * 11
    # the rule itself: ties go to the smaller distance; the margin is inclusive; no samples, no filter
    assert ad.rule([1000, 500, 300, 400, 300, 900, 300, 900, 900, 900, 900], 1) == (2, 2)
    assert ad.rule([300 + 128 * 7, 500, 300, 400, 300, 900, 300, 900, 900, 900, 900], 7) == (2, 2)
    assert ad.rule([300 + 128 * 7 - 1, 500, 300, 400, 300, 900, 300, 900, 900, 900, 900], 7) == (0, 2)
    assert ad.rule([0] * 11, 0) == (0, 1)
