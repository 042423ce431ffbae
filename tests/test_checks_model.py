"""The helpers of the edge tests (tests/_checks.py) pinned on the CPU, and the conditions without which the device tests that
use them would pass vacuously: the crafted Streams are accepted by the system's liblzma and refused after one flipped Check
bit, the system's forward filters are the models the other tests use, the ragged auto-delta inputs make neighbouring Blocks
pick different distances, and the seam inputs make the x86 filter convert in most Blocks."""
import lzma

import numpy as np
import pytest

import _auto_delta as ad
import _checks as ck
import _filters as fl
import _oracle as o

CHECKS = [1, 4, 10]


def test_crc64_check_value():
    assert ck.crc64(b"123456789") == 0x995DC9BBDF1939FA
    assert ck.crc64(b"") == 0
    assert ck.check_bytes(4, b"123456789") == bytes.fromhex("fa3919dfbbc95d99")


@pytest.mark.parametrize("n", [0, 1, 7, 8, 4095, 4096, 4097, 65536])
def test_crc64_is_the_oracles(n):
    d = np.random.default_rng(n).integers(0, 256, max(n, 1), dtype=np.uint8)[:n]
    got = ck.crc64(d.tobytes())
    if n:
        assert got == o.orc().orc_crc64(o._ptr(np.ascontiguousarray(d)), n, 0)
        if o.have_ref():
            assert got == o.ref().ref_crc64(o._ptr(np.ascontiguousarray(d)), n, 0)
    else:
        assert got == 0


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("name", list(ck.SIZE_LISTS))
def test_crafted_streams_are_accepted_and_flipped_ones_refused(name, check):
    sizes = ck.SIZE_LISTS[name]
    data, raw = ck.crafted(name, check)
    assert lzma.decompress(raw, format=lzma.FORMAT_XZ) == data
    fields = ck.check_fields(raw)
    assert len(fields) == len(sizes) and all(sz == ck.CHECK_SIZE[check] for _, sz in fields)
    at = 0
    for (off, sz), n in zip(fields, sizes):
        assert raw[off: off + sz] == ck.check_bytes(check, data[at: at + n])
        at += n
    for b in ck.flip_subset(sizes):
        off, sz = fields[b]
        for where, bit in ((off, 0), (off + sz - 1, 7)):
            with pytest.raises(lzma.LZMAError):
                lzma.decompress(ck.flip(raw, where, bit), format=lzma.FORMAT_XZ)


def test_every_byte_of_a_sha256_check_counts():
    data, raw = ck.crafted("sha_edges", 10)
    off, sz = ck.check_fields(raw)[4]
    assert sz == 32
    for i in range(32):
        with pytest.raises(lzma.LZMAError):
            lzma.decompress(ck.flip(raw, off + i, i % 8), format=lzma.FORMAT_XZ)


@pytest.mark.parametrize("dist", [1, 2, 3, 24, 32, 256])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 4099])
def test_sys_forward_delta_is_the_numpy_model(n, dist):
    d = ck._rnd(n, 7 * n + dist)
    assert ck.sys_forward(d, [(fl.DELTA, dist)]) == fl.np_delta_forward(d, dist)


def test_sys_forward_x86_is_the_reference_filter():
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    for n in (0, 4, 5, 6, 100, 5000):
        d = bytes(o.corpus_x86(n, seed=n + 1))[:n]
        assert ck.sys_forward(d, [(fl.BCJ["x86"], 0)]) == (o.ref_x86_filter(d) if n else b"")
    data, bs = ck.x86_seam_blocks("encoder", 50, 3)
    for at in range(0, len(data), bs):
        assert ck.sys_forward(data[at: at + bs], [(4, 0)]) == o.ref_x86_filter(data[at: at + bs])


def test_block_payload_filtered_reads_a_stored_block():
    data, raw = ck.crafted("ragged", 4)
    at, pos = 0, 12
    for n, (off, _) in zip(ck.SIZE_LISTS["ragged"], ck.check_fields(raw)):
        assert ck.block_payload_filtered(raw, pos) == data[at: at + n] and ck.block_chain(raw, pos) == []
        at += n
        pos = off + 8


# ---- the conditions of test_gpu_auto_delta_ragged.py ----
@pytest.mark.parametrize("bs,tail", ck.RAGGED_CASES)
def test_ragged_auto_delta_inputs_mix_distances(bs, tail):
    data, bs = ck.ragged_input(bs, tail)
    assert len(data) == 6 * bs + tail and bs % 16 != 0
    want, _ = ad.choose_blocks(data, bs)
    print(bs, tail, want)
    assert len(want) == 7 and len(set(want)) >= 3
    assert sum(a != b for a, b in zip(want, want[1:])) >= 4          # neighbours that differ, at seams off the 16-byte grid
    assert want[:6] == [0, 4, 24, 4, 0, 8]


def test_all_tails_appear():
    assert {t for _, t in ck.RAGGED_CASES} == {1, 15, 16, 17, 31, 33}
    assert {b for b, _ in ck.RAGGED_CASES} == {4097, 65537, 65636, 69631, 200001}


def test_pair_input_takes_the_distances_it_is_made_for():
    data, bs, made = ck.pair_input()
    want, _ = ad.choose_blocks(data, bs)
    assert want[:-1] == made[:-1]
    pairs = set(zip(want[:-1], want[1:-1]))
    for d in ck.PAIR_DISTS:
        assert (d, 0) in pairs and (0, d) in pairs
    assert sum(1 for a, b in pairs if a and b and a != b) >= 4
    assert {(k * bs) % 16 for k in range(1, len(want))} == set(range(16))     # every offset of a seam inside a 16-byte group


# ---- the conditions of test_gpu_bcj_seams.py ----
def test_x86_seam_blocks_are_converted():
    for kind, count, floor in (("encoder", 2000, 1000), ("decoder", 200, 100)):
        data, bs = ck.x86_seam_blocks(kind, count, 11)
        assert len(data) == count * bs
        changed = sum(ck.sys_forward(data[at: at + bs], [(4, 0)]) != data[at: at + bs] for at in range(0, len(data), bs))
        print(kind, "Blocks the system's x86 filter changes:", changed, "of", count)
        assert changed >= floor


def test_riscv_seam_blocks_are_converted():
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    for kind, count in (("encoder", 300), ("decoder", 100)):
        data, bs = ck.riscv_seam_blocks(kind, count, 12)
        changed = sum(fl.ref_forward(data[at: at + bs], [(0x0B, 0)]) != data[at: at + bs] for at in range(0, len(data), bs))
        print(kind, "Blocks the reference's RISC-V filter changes:", changed, "of", count)
        assert changed >= count // 2
