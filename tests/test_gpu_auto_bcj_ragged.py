"""Automatic per-Block BCJ filter at its length and alignment edges (DESIGN.md 3.5 "Edge classes and their tests"): x86 sites
in the last five bytes of a Block and across its end, sites straddling the 16-byte groups of the threads of k_bcj_stats and
the seams of its tiles and workgroups by every number of bytes, Block sizes that are no multiple of 4 (later Blocks start off
the batch's 4-byte grid while ARM64 alignment stays Block-relative), last Blocks of 1, 4, 5 and 17 bytes, and an empty input.
Choices, histograms and site counts are compared with the numpy model (tests/_auto_bcj.py) bit for bit, every Block of the
Stream with the Block of the fixed-chain Stream of its kind."""
import numpy as np
import pytest

import _auto_bcj as ab
import _oracle as o

pytestmark = pytest.mark.gpu

X86, ARM64 = 4, 0x0A
TILE, RUN = 4096, 65536            # bytes per workgroup step and per workgroup of k_bcj_stats


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


def _run(enc, data, bs):
    """model == device for the analysis; every Block of the auto Stream == the Block of the fixed-chain Stream of its kind"""
    import xz_amd
    d = _cuda(data)
    want, want_hist, want_n = ab.choose_blocks(data, bs)
    got = enc.choose_bcj(d, bs)
    hist, ns, kind = enc.bcj_histograms(len(want))
    print("Block size", bs, "model", want, "device", got, "sites", want_n.tolist())
    assert got == want and kind.tolist() == want
    assert np.array_equal(ns, want_n) and np.array_equal(hist, want_hist)
    out, binfo = enc.encode(d, preset=1, block_size=bs, auto_bcj=True)
    raw = _bytes(out)
    fixed = {}
    for k in set(want):
        opts = xz_amd.preset_options(1)
        opts.bcj = k
        s, fb = enc.encode(d, opts=opts, block_size=bs)
        fixed[k] = (_bytes(s), fb)
    for i, (b, k) in enumerate(zip(binfo, want)):
        fraw, fb = fixed[k]
        assert raw[b.out_offset: b.out_offset + b.total_size] == fraw[fb[i].out_offset: fb[i].out_offset + fb[i].total_size], (i, k)
    rr, dec = o.ref_decode(raw, len(data) + 16)
    assert rr == 1 and dec == data
    assert _bytes(enc.decode(_cuda(raw), len(data))[0]) == data
    return want, want_n


def _plant(x, pos, top=0x00):
    x[pos] = 0xE8
    x[pos + 4] = top


def test_sites_at_the_block_end(enc):
    """Block 0 ends with a site at len - 5 (its operand ends on the last byte: counted); Block 1 has E8 at len - 4 and Block 2
    starts with 00, so a statistic that read across the Block end would count a site the model does not."""
    bs = 70001
    x = np.frombuffer(ab.synth_x86(3 * bs, 51), dtype=np.uint8).copy()
    x[bs - 10: bs] = 0x11
    _plant(x, bs - 5)
    x[2 * bs - 10: 2 * bs + 1] = 0x11
    x[2 * bs - 4] = 0xE8
    x[2 * bs] = 0x00
    data = x.tobytes()
    i0 = ab.sites(data[:bs], 0)[0]
    i1 = ab.sites(data[bs: 2 * bs], 0)[0]
    assert i0[-1] == bs - 5 and i1[-1] < bs - 10
    want, _ = _run(enc, data, bs)
    assert want == [X86, X86, X86]


def test_sites_across_thread_groups_and_tile_seams(enc):
    """x86 sites planted so that 0 .. 5 of their bytes lie behind every kind of seam: the 16-byte groups, the 4 KiB tiles and
    the 64 KiB runs of the workgroups; text around them, so that they are the only sites."""
    bs = 3 * RUN + 4096 + 7
    x = np.frombuffer(ab.text(2 * bs), dtype=np.uint8).copy()
    want_pos = []
    for m in range(1, bs // TILE + 1):
        pos = m * TILE - (m % 6)                      # m = 16, 32, 48: the run seams, with 4, 2 and 0 bytes in front
        if pos + 5 <= bs:
            _plant(x, pos, 0xFF if m & 1 else 0x00)
            want_pos.append(pos)
    for g in range(16):                               # every offset modulo 16 inside one tile
        pos = 1000 * 16 + 48 * g + g
        _plant(x, pos)
        want_pos.append(pos)
    data = x.tobytes()
    assert sorted(ab.sites(data[:bs], 0)[0].tolist()) == sorted(want_pos)
    assert {p % 16 for p in want_pos} == set(range(16))
    _run(enc, data, bs)


@pytest.mark.parametrize("tail", [1, 4, 5, 17])
def test_block_size_off_the_grid_and_short_last_blocks(enc, tail):
    """Blocks of 70001 bytes (1 mod 4): x86, ARM64, text, ARM64 -- every Block generated on its own, so the BL sites sit on the
    Block's 4-byte grid and, from the second Block on, off the batch's -- and a last Block of `tail` bytes that holds a site
    where one fits."""
    bs = 70001
    last = {1: b"\xe8", 4: b"\x01\x00\x00\x94", 5: b"\xe8\x10\x00\x00\x00",
            17: b"\x01\x00\x00\x94" * 3 + b"\xe8\x10\x00\x00\x00"}[tail]
    assert len(last) == tail
    data = ab.synth_x86(bs, 61) + ab.synth_arm64(bs, 62) + ab.text(bs) + ab.synth_arm64(bs, 63) + last
    want, ns = _run(enc, data, bs)
    assert want == [X86, ARM64, 0, ARM64, 0]
    assert ns[4].tolist() == {1: [0, 0], 4: [0, 1], 5: [1, 0], 17: [1, 3]}[tail]


def test_empty_input(enc):
    d = _cuda(b"")
    assert enc.choose_bcj(d, 65536) == []
    auto, binfo = enc.encode(d, preset=6, block_size=65536, auto_bcj=True)
    plain, _ = enc.encode(d, preset=6, block_size=65536)
    assert _bytes(auto) == _bytes(plain) and binfo == []
