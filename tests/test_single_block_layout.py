"""The layout the single-Block encoder writes, pinned without a GPU: a one-Block .xz Stream whose Block Header carries no
sizes and whose LZMA2 data is a concatenation of chunk chains that each start with a dictionary reset (made here from
Python's lzma raw encodings) is a valid file for stock liblzma and for the host file index; and the Check of such a
Block can be combined from the Checks of its segments (xzamd_crc32_combine / xzamd_crc64_combine)."""
import lzma
import zlib

import numpy as np
import pytest

import _single_block as sb


def test_segmented_one_block_stream_is_valid(product_lib):
    import xz_amd
    fx = sb.four_segments()
    assert len(fx.data) == 220000
    assert lzma.decompress(fx.raw) == fx.data
    # both kinds of dictionary reset occur: 0xE0 | x (LZMA chunk) and 0x01 (uncompressed chunk: the random segment)
    firsts = [fx.raw[off] for off in fx.seg_off]
    assert firsts[2] == 0x01 and all(c >= 0xE0 for c in (firsts[0], firsts[1], firsts[3])), firsts
    assert fx.raw[12:14] == b"\x02\x00"                  # Block Header of 12 bytes, Block Flags: one filter, no sizes
    streams, blocks, usize = xz_amd.file_index(fx.raw)
    assert usize == 220000 and len(streams) == 1 and streams[0]["block_count"] == 1 and streams[0]["check"] == 4
    assert len(blocks) == 1
    b = blocks[0]
    assert (b["header_offset"], b["unpadded_size"], b["uncompressed_size"]) == (12, fx.unpadded, 220000)
    assert b["total_size"] == (fx.unpadded + 3) // 4 * 4 and b["filter_ids"] == (0x21,)


@pytest.mark.parametrize("len_b", [0, 1, 4095, 70000])
def test_crc_combine(product_lib, len_b):
    import xz_amd
    rng = np.random.default_rng(len_b + 5)
    a = bytes(rng.integers(0, 256, size=12345, dtype=np.uint8))
    b = bytes(rng.integers(0, 256, size=len_b, dtype=np.uint8))
    assert xz_amd.crc32_combine(zlib.crc32(a), zlib.crc32(b), len_b) == zlib.crc32(a + b)
    assert xz_amd.crc32_combine(0, zlib.crc32(b), len_b) == zlib.crc32(b)         # an empty first part
    whole = sb.liblzma_crc64(a + b)
    assert whole == sb.crc64(a + b)
    assert xz_amd.crc64_combine(sb.liblzma_crc64(a), sb.liblzma_crc64(b), len_b) == whole
    assert xz_amd.crc64_combine(0, sb.liblzma_crc64(b), len_b) == sb.liblzma_crc64(b)


def test_crc_combine_over_many_parts(product_lib):
    """Folded left to right over parts of 0, 1, 4095 and 70,000 bytes, as the encoder folds its segments."""
    import xz_amd
    rng = np.random.default_rng(3)
    parts = [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (4095, 0, 70000, 1, 70000, 0)]
    c32 = c64 = 0
    for p in parts:
        c32 = xz_amd.crc32_combine(c32, zlib.crc32(p), len(p))
        c64 = xz_amd.crc64_combine(c64, sb.crc64(p), len(p))
    whole = b"".join(parts)
    assert c32 == zlib.crc32(whole) and c64 == sb.liblzma_crc64(whole)
