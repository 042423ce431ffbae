"""Automatic per-Block delta filter at Block sizes that are no multiple of 16 (DESIGN.md 3.5 "Edge classes and their tests"):
k_delta_stats on partial windows, on fewer than 16 bytes per thread and on Block starts off the 16-byte grid, and
k_delta_blocks on 16-byte groups that straddle two Blocks whose distances differ.  The choices and histograms are compared
with the numpy model (tests/_auto_delta.py) bit for bit; what the filter stage wrote is read back out of every Block with
the system's liblzma (the `lzma` module) and compared with the numpy delta encoder.  The inputs and the conditions that keep
these tests from passing vacuously (mixed distances, neighbours that differ) are checked on the CPU in test_checks_model.py."""
import lzma

import numpy as np
import pytest

import _auto_delta as ad
import _checks as ck
import _filters as fl
import _oracle as o

pytestmark = pytest.mark.gpu


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


def _check_blocks(raw, offsets, data, bs, want):
    """Every Block Header's chain is the model's choice, and the Block's LZMA2 payload holds the delta encoder's bytes."""
    assert len(offsets) == len(want)
    for b, (off, d) in enumerate(zip(offsets, want)):
        block = data[b * bs: (b + 1) * bs]
        assert ck.block_chain(raw, off) == ([(fl.DELTA, d)] if d else []), (b, d)
        got, exp = ck.block_payload_filtered(raw, off), fl.np_delta_forward(block, d) if d else block
        assert got == exp, f"Block {b} (distance {d}): the filtered bytes differ first at {o.first_diff(got, exp)} of {len(exp)}"


def _run(enc, data, bs, want, want_hist):
    d = _cuda(data)
    got = enc.choose_delta(d, bs)
    hist, dist = enc.delta_histograms(len(want))
    print("Block size", bs, "model", want, "device", got)
    assert got == want and dist.tolist() == want
    assert hist.dtype == want_hist.dtype and np.array_equal(hist, want_hist)
    out, binfo = enc.encode(d, preset=1, block_size=bs, check=4, auto_delta=True)
    raw = _bytes(out)
    _check_blocks(raw, [b.out_offset for b in binfo], data, bs, want)
    assert lzma.decompress(raw, format=lzma.FORMAT_XZ) == data
    x = _cuda(raw)
    assert _bytes(enc.decode(x, len(data))[0]) == data
    assert _bytes(enc.decode_file(x, len(data))[0]) == data
    fwd, rep = enc.decode_forward(x, len(data))
    assert _bytes(fwd) == data and rep["blocks_delivered"] == len(want)
    bare, b2 = enc.encode(d, preset=1, block_size=bs, check=4, auto_delta=True, blocks_only=True)
    _check_blocks(_bytes(bare), [b.out_offset for b in b2], data, bs, want)


@pytest.mark.parametrize("bs,tail", ck.RAGGED_CASES)
def test_ragged_block_sizes(enc, bs, tail):
    data, bs = ck.ragged_input(bs, tail)
    want, want_hist = ad.choose_blocks(data, bs)
    assert len(set(want)) >= 3 and any(a != b for a, b in zip(want, want[1:]))
    _run(enc, data, bs, want, want_hist)


def test_neighbours_of_every_distance_pair(enc):
    """(d, 0), (0, d) and (d1, d2) for d in {1, 3, 24, 32} at seams on every offset modulo 16: the per-byte distance lookup of a
    straddling group sees every pairing."""
    data, bs, made = ck.pair_input()
    want, want_hist = ad.choose_blocks(data, bs)
    assert want[:-1] == made[:-1]
    _run(enc, data, bs, want, want_hist)
