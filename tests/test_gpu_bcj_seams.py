"""The x86 and RISC-V walks at the seams between their owners (DESIGN.md 3.5 "Edge classes and their tests"): every 2048 bytes
in the encoder (BCJ_CHUNK of k_x86_bcj / k_riscv_bcj), every 64 bytes and at every 16384 (a tile = a workgroup) in the decoder
(unf_x86 / unf_riscv).  The Blocks (tests/_checks.py) are quiet but for clusters of opcode bytes laid across the seams: the
last synchronisation point just in front of a seam, none for some bytes behind it, conversions whose operands span it, and a
prev_mask history the next owner must not see.  What the device's filter stage wrote is read out of every Block with the
system's liblzma and compared with the system's own filter (RISC-V: the reference's, oracle/_ref); the inverse walks decode
the device's Streams and Streams whose payloads the system made.  test_checks_model.py shows on the CPU that the filters do
convert in these Blocks."""
import lzma
import zlib

import pytest

import _checks as ck
import _filters as fl
import _oracle as o

pytestmark = pytest.mark.gpu

X86, RISCV = 4, 0x0B


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


def _device_stream(enc, data, bs, fid):
    import xz_amd
    opts = xz_amd.preset_options(1)
    opts.bcj = fid
    out, binfo = enc.encode(_cuda(data), opts=opts, block_size=bs, check=1)
    assert len(binfo) == len(data) // bs
    return _bytes(out), binfo


def _forward_and_back(enc, data, bs, fid, forward, decode):
    """per Block: the filter stage's bytes are `forward` of the Block; then the Stream through `decode` (the system's decoder,
    or the reference's for a filter the system's does not know) and the device's three entries"""
    raw, binfo = _device_stream(enc, data, bs, fid)
    changed = 0
    for b, bi in enumerate(binfo):
        block = data[b * bs: (b + 1) * bs]
        assert ck.block_chain(raw, bi) == [(fid, 0)]
        got, exp = ck.block_payload_filtered(raw, bi), forward(block)
        assert got == exp, f"Block {b}: the filtered bytes differ first at {o.first_diff(got, exp)}"
        changed += exp != block
    print("Blocks with conversions:", changed, "of", len(binfo))
    assert changed >= len(binfo) // 2
    assert decode(raw) == data
    x = _cuda(raw)
    assert _bytes(enc.decode(x, len(data))[0]) == data
    assert _bytes(enc.decode_file(x, len(data))[0]) == data
    assert _bytes(enc.decode_forward(x, len(data))[0]) == data


@pytest.mark.parametrize("kind,count", [("encoder", 2000), ("decoder", 200)])
def test_x86_walk_at_its_seams(enc, kind, count):
    data, bs = ck.x86_seam_blocks(kind, count, 11)
    _forward_and_back(enc, data, bs, X86, lambda blk: ck.sys_forward(blk, [(X86, 0)]), lambda raw: lzma.decompress(raw, format=lzma.FORMAT_XZ))


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_x86_blocks_the_system_filtered_decode(enc, kind):
    """200 single-Block Streams {x86, LZMA2} whose payloads the `lzma` module made, laid end to end as one file: one decode of
    all of them; the first few through the forward reader (which takes a file Stream by Stream) and on their own"""
    data, bs = ck.x86_seam_blocks(kind, 200, 13)
    spec = [{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA2, "preset": 0}]       # preset 0: a dictionary of 256 KiB, byte 0x0C
    streams = []
    for at in range(0, len(data), bs):
        block = data[at: at + bs]
        payload = lzma.compress(block, format=lzma.FORMAT_RAW, filters=spec)
        streams.append(fl.single_block_stream(1, b"\x04\x00\x21\x01\x0c", 2, payload, zlib.crc32(block).to_bytes(4, "little"), bs))
    whole = b"".join(streams)
    assert lzma.decompress(whole, format=lzma.FORMAT_XZ) == data
    out, nb = enc.decode_file(_cuda(whole), len(data))
    assert nb == 200 and _bytes(out) == data
    out, rep = enc.decode_forward(_cuda(b"".join(streams[:8])), 8 * bs)
    assert _bytes(out) == data[: 8 * bs] and rep["streams"] == 8
    for b in range(4):
        assert _bytes(enc.decode(_cuda(streams[b]), bs)[0]) == data[b * bs: (b + 1) * bs]


@pytest.mark.parametrize("kind,count", [("encoder", 300), ("decoder", 100)])
def test_riscv_walk_at_its_seams(enc, kind, count):
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    data, bs = ck.riscv_seam_blocks(kind, count, 12)
    _forward_and_back(enc, data, bs, RISCV, lambda blk: fl.ref_forward(blk, [(RISCV, 0)]), lambda raw: o.ref_decode(raw, len(data) + 16)[1])
    # the inverse walk on a Stream the reference made
    ref = o.ref_encode_mt_chain(data, 0, RISCV, threads=1, block_size=bs, check=1)
    assert _bytes(enc.decode(_cuda(ref), len(data))[0]) == data
