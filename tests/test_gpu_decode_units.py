"""Plain device decode with units at dictionary resets: a Block whose LZMA2 data holds several dictionary resets (the
single-Block encoder's segments; here made with Python's lzma on the host) decodes one wavefront per unit, through
all three entry points, with its Check verified; a Block of one reset stays one unit."""
import lzma

import pytest

import _oracle as o
import _single_block as sb

pytestmark = pytest.mark.gpu

DATA_ERROR = 9


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


def _code(call):
    import xz_amd
    try:
        call()
    except xz_amd.XzAmdError as e:
        assert e.code
        return e.code
    return 0


def test_four_segments_through_all_entry_points(enc):
    fx = sb.four_segments()
    t = _cuda(fx.raw)
    got, nb = enc.decode(t, len(fx.data) + 16)
    assert nb == 1 and o.first_diff(_bytes(got), fx.data) == -1
    assert enc.debug_decode_units() == (4, 1, 2)
    got, nb = enc.decode_file(t, len(fx.data) + 16)
    assert nb == 1 and o.first_diff(_bytes(got), fx.data) == -1
    assert enc.debug_decode_units() == (4, 1, 2)
    # a range inside the third segment (the random one: stored chunks)
    lo = fx.seg_upos[2] + 12345
    got, nb = enc.decode_range(t, lo, 40000)
    assert nb == 1 and _bytes(got) == fx.data[lo:lo + 40000]
    # the verification decode keeps its own units (state resets with properties; the original as history)
    ver, _ = enc.decode(t, len(fx.data) + 16, expected=_cuda(fx.data))
    assert _bytes(ver) == fx.data and enc.debug_decode_units()[2] == 1


def test_stored_check_is_verified(enc):
    fx = sb.four_segments()
    bad = bytearray(fx.raw)
    check_at = 24 + fx.csize + (-fx.csize % 4)
    bad[check_at] ^= 1
    with pytest.raises(lzma.LZMAError):
        lzma.decompress(bytes(bad))
    assert _code(lambda: enc.decode(_cuda(bad), len(fx.data) + 16)) == DATA_ERROR


def test_mt_stream_is_one_unit_per_block(enc):
    import xz_amd
    data = xz_amd.corpus_text(4 * 65536 - 7, seed=4).tobytes()
    xz, binfo = enc.encode(_cuda(data), preset=6, block_size=65536)
    assert len(binfo) == 4
    got, nb = enc.decode(xz, len(data) + 16)
    assert nb == 4 and _bytes(got) == data
    assert enc.debug_decode_units() == (4, 4, 2)


def test_more_resets_than_the_unit_table_holds(enc):
    """60 segments of 2 KiB in a Block of 120 KiB: the table holds 120 KiB / 4096 + 8 = 38 units; the resets beyond stay
    inside the last unit, and the Block decodes all the same."""
    fx = sb.many_segments(60, 2048)
    assert lzma.decompress(fx.raw) == fx.data
    got, nb = enc.decode(_cuda(fx.raw), len(fx.data) + 16)
    assert nb == 1 and o.first_diff(_bytes(got), fx.data) == -1
    assert enc.debug_decode_units() == (len(fx.data) // 4096 + 8, 1, 2)
    fits = sb.many_segments(40, 4096)                   # 160 KiB / 4096 + 8 = 48 >= 40: a unit per segment
    got, _ = enc.decode(_cuda(fits.raw), len(fits.data) + 16)
    assert _bytes(got) == fits.data and enc.debug_decode_units() == (40, 1, 2)


def test_flipped_byte_in_the_range_coder_data_of_segment_3(enc):
    fx = sb.four_segments()
    bad = bytearray(fx.raw)
    assert bad[fx.seg_off[3]] >= 0xE0
    bad[fx.seg_off[3] + 6 + fx.seg_len[3] // 2] ^= 0x10
    with pytest.raises(lzma.LZMAError):
        lzma.decompress(bytes(bad))
    assert _code(lambda: enc.decode(_cuda(bad), len(fx.data) + 16)) == DATA_ERROR
    assert _code(lambda: enc.decode_file(_cuda(bad), len(fx.data) + 16)) == DATA_ERROR


def test_segment_without_its_dictionary_reset_decodes_in_the_unit_before(enc):
    """Segment 3's first control byte 0xE0 | x -> 0xC0 | x (state reset and properties, no dictionary reset): no error of
    the unit scan; the chunks now belong to segment 2's unit and decode against real history.  Whatever stock liblzma
    makes of the file is the expectation."""
    fx = sb.four_segments()
    mod = bytearray(fx.raw)
    ctl = mod[fx.seg_off[3]]
    assert ctl >= 0xE0
    mod[fx.seg_off[3]] = 0xC0 | (ctl & 0x1F)
    try:
        want = lzma.decompress(bytes(mod))
    except lzma.LZMAError:
        want = None
    if want is None:
        assert _code(lambda: enc.decode(_cuda(mod), len(fx.data) + 16)) == DATA_ERROR
    else:
        got, _ = enc.decode(_cuda(mod), len(fx.data) + 16)
        assert o.first_diff(_bytes(got), want) == -1
    assert enc.debug_decode_units() == (3, 1, 2)
