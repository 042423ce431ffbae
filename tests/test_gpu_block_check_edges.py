"""Block Checks at their length edges (DESIGN.md 3.5 "Edge classes and their tests").
Encode side: k_sha256_blocks on Blocks whose padding fits the last chunk, spills into a second one or meets a chunk boundary,
and on more than one wavefront of Blocks; k_crc_strips / k_crc_fold on 64, 65, 66 and 129 strips and on a last strip of one
byte.  The Check fields of the Streams are compared with zlib, hashlib and a table CRC64 (tests/_checks.py), and every Stream
goes through the system's liblzma (the `lzma` module), which verifies all Checks.
Decode side: Streams made in Python with real Checks (stored LZMA2 chunks only, so that nothing but the Check stage can go
wrong) in the shapes the launch grouping of the device decoder tells apart: uniform groups, ragged groups, empty Blocks, several
Streams with different Checks.  Good Streams decode through every entry; a Check with one flipped bit is refused, at the Block
that carries it.  test_checks_model.py shows on the CPU that the `lzma` module accepts the same Streams and refuses the same
flips."""
import lzma

import pytest

import _checks as ck

pytestmark = pytest.mark.gpu

DATA_ERROR = 9
CHECKS = [1, 4, 10]
K = 1024


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


_TEXT = None


def _data(n):
    """text with noise: compressible, so that the Blocks are coded ones, and no period a CRC could hide behind"""
    global _TEXT
    if _TEXT is None:
        import numpy as np
        import xz_amd
        a = xz_amd.corpus_text(600 * K, seed=21).copy()
        rng = np.random.default_rng(22)
        at = rng.integers(0, len(a), len(a) // 16)
        a[at] = rng.integers(0, 256, len(at), dtype=np.uint8)
        _TEXT = a.tobytes()
    while len(_TEXT) < n:
        _TEXT += _TEXT
    return _TEXT[:n]


def _encoded_checks(enc, data, bs, check, preset=1, python_crc64_limit=64 * K):
    """Encode, then: every Block's Check field (the last bytes of the Block the block infos locate) is the Check of its data,
    and the system's decoder takes the Stream."""
    out, binfo = enc.encode(_cuda(data), preset=preset, block_size=bs, check=check)
    raw = _bytes(out)
    csz = ck.CHECK_SIZE[check]
    assert len(binfo) == (len(data) + bs - 1) // bs
    for b, bi in enumerate(binfo):
        block = data[b * bs: (b + 1) * bs]
        assert bi.uncompressed_size == len(block) and bi.total_size == (bi.unpadded_size + 3) & ~3
        if check == 4 and len(block) > python_crc64_limit:
            continue                                    # (the table CRC64 is too slow: liblzma below is the arbiter)
        end = bi.out_offset + bi.total_size
        assert raw[end - csz: end] == ck.check_bytes(check, block), f"Check {check} of Block {b} ({len(block)} bytes)"
    assert lzma.decompress(raw, format=lzma.FORMAT_XZ) == data, f"Check {check}, Block size {bs}, {len(data)} bytes"


# ---- encode side ----
@pytest.mark.parametrize("check", CHECKS)
def test_encoded_checks_of_short_last_blocks(enc, check):
    """a last Block of r bytes: r mod 64 = 55 | 56 (the SHA-256 padding fits | spills), 63 | 64 | 65, 119 | 120, and one strip"""
    for r in (1, 55, 56, 63, 64, 65, 119, 120, 4095):
        _encoded_checks(enc, _data(4096 + r), 4096, check, preset=0 if r & 1 else 1)


def test_encoded_sha256_of_131_blocks(enc):
    """three wavefronts of lanes, the last one partial, and a last Block whose padding spills"""
    _encoded_checks(enc, _data(130 * 4096 + 56), 4096, 10)


@pytest.mark.parametrize("check", [1, 4])
@pytest.mark.parametrize("bs", [4097, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 17, 128 * 4096 + 1])
def test_encoded_crc_at_the_fold_edges(enc, bs, check):
    """2, 64, 65, 66 and 129 strips of 4096 bytes per Block (one per lane | two per lane with lanes left empty | three), a last
    strip of one byte, and a last Block of one byte"""
    _encoded_checks(enc, _data(2 * bs + 1), bs, check)


# ---- decode side ----
def _decodes(enc, raw, data, nblocks):
    x = _cuda(raw)
    out, nb = enc.decode(x, len(data))
    assert _bytes(out) == data and nb == nblocks
    out, nb = enc.decode_file(x, len(data))
    assert _bytes(out) == data and nb == nblocks
    out, rep = enc.decode_forward(x, len(data))
    assert _bytes(out) == data and rep["blocks_delivered"] == nblocks and rep["code"] == 0
    assert enc.verify_blocks(x) == ["none"] * nblocks


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("name", list(ck.SIZE_LISTS))
def test_crafted_streams_decode_and_flipped_checks_are_refused(enc, name, check):
    import xz_amd
    sizes = ck.SIZE_LISTS[name]
    data, raw = ck.crafted(name, check)
    _decodes(enc, raw, data, len(sizes))
    fields = ck.check_fields(raw)
    bad = ck.flip_subset(sizes)
    hurt = raw
    for i, b in enumerate(bad):
        off, sz = fields[b]
        hurt = ck.flip(hurt, off + (i * 5) % sz, (i * 3) % 8)
    x = _cuda(hurt)
    steps = enc.verify_blocks(x)
    assert steps == ["check" if b in bad else "none" for b in range(len(sizes))]
    rep = enc.verify_report()
    assert rep["first_bad_block"] == bad[0] and rep["first_bad_step"] == "check"
    for call in (enc.decode, enc.decode_file):
        with pytest.raises(xz_amd.XzAmdError) as ei:
            call(x, len(data))
        assert ei.value.code == DATA_ERROR and f"Block {bad[0]}: Block Check mismatch" in str(ei.value)
    with pytest.raises(xz_amd.XzAmdError) as ei:
        enc.decode_forward(x, len(data))
    assert ei.value.code == DATA_ERROR and ei.value.report["blocks_delivered"] == bad[0]
    assert _bytes(ei.value.partial) == data[: sum(sizes[: bad[0]])]
    # one flip at a time, in a Block behind the first: that Block alone
    if len(bad) > 1:
        off, sz = fields[bad[-1]]
        steps = enc.verify_blocks(_cuda(ck.flip(raw, off + sz - 1, 7)))
        assert steps == ["check" if b == bad[-1] else "none" for b in range(len(sizes))]


def test_every_byte_of_a_sha256_check_is_compared(enc):
    sizes = ck.SIZE_LISTS["sha_edges"]
    data, raw = ck.crafted("sha_edges", 10)
    off, sz = ck.check_fields(raw)[4]
    assert sz == 32
    for i in range(32):
        steps = enc.verify_blocks(_cuda(ck.flip(raw, off + i, i % 8)))
        assert steps == ["check" if b == 4 else "none" for b in range(len(sizes))], f"byte {i} of the Check"


def test_concatenated_streams_with_different_checks(enc):
    """CRC32 x 3 Blocks, SHA-256 x 5, CRC64 x 2 with Stream Padding between them: the results of every group land at the
    group's first Block in the tables of the run"""
    import xz_amd
    parts = [(1, [4096, 4096, 100]), (10, [64, 64, 64, 64, 56]), (4, [8192, 1])]
    data, raw, spans = b"", b"", []
    for i, (check, sizes) in enumerate(parts):
        d = ck._rnd(sum(sizes), 300 + i)
        one = ck.stored_stream_checked(d, sizes, check)
        assert lzma.decompress(one, format=lzma.FORMAT_XZ) == d       # (the module reads no Stream Padding: one Stream at a time)
        spans.append((len(raw), len(raw) + len(one)))
        raw += one + bytes(4 * i + 4 if i < 2 else 0)
        data += d
    x = _cuda(raw)
    out, nb = enc.decode_file(x, len(data))
    assert _bytes(out) == data and nb == 10
    out, rep = enc.decode_forward(x, len(data))
    assert _bytes(out) == data and rep["blocks_delivered"] == 10 and rep["streams"] == 3
    # the third Block of the second Stream is Block 5 of the file; then the last Block of the last Stream: Block 9
    for stream, block, overall in ((1, 2, 5), (2, 1, 9), (0, 0, 0)):
        off, sz = ck.check_fields(raw, spans[stream][0])[block]
        hurt = ck.flip(raw, off + sz // 2, 4)
        with pytest.raises(lzma.LZMAError):
            lzma.decompress(hurt[spans[stream][0]: spans[stream][1]], format=lzma.FORMAT_XZ)
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.decode_file(_cuda(hurt), len(data))
        assert ei.value.code == DATA_ERROR and f"Block {overall}: Block Check mismatch" in str(ei.value)
        with pytest.raises(xz_amd.XzAmdError) as ei:
            enc.decode_forward(_cuda(hurt), len(data))
        assert ei.value.code == DATA_ERROR and ei.value.report["blocks_delivered"] == overall
        at = sum(sum(s) for _, s in parts[:stream]) + sum(parts[stream][1][:block])
        assert _bytes(ei.value.partial) == data[:at]
