"""Device decoder for whole .xz files: concatenated Streams and Stream Padding (Encoder.decode_file), the file index
with the Block Headers parsed by k_dec_headers (Encoder.file_index) against the host parser (xz_amd.file_index), the
number of device-to-host reads per file, and range decode (Encoder.decode_range) -- against the real liblzma
(oracle/_ref) and the single-Stream entry (Encoder.decode)."""
import glob
import os
import zlib

import pytest

import _filters as f
import _oracle as o
import _xzfiles as x

pytestmark = pytest.mark.gpu

DATA_ERROR = 9


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    e = xz_amd.Encoder()
    yield e
    e.close()


@pytest.fixture(scope="module")
def built():
    return x.built_files()


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


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


def _host_code(raw):
    import xz_amd
    return _code(lambda: xz_amd.file_index(raw))


BS_OWN = 1 << 17
BUILT = ["checks-p0", "checks-p1", "delta-p0", "delta-p1"]


# ---------------------------------------------------------------- whole-file decode
@pytest.mark.parametrize("name", BUILT)
def test_decodes_built_files(enc, built, name):
    fl = built[name]
    r, want = x.ref_concat_decode(fl.raw, len(fl.data) + 16)
    assert r == 0 and want == fl.data
    nblocks = len(x.expected_layout(fl)[1])
    t = _cuda(fl.raw)
    got, nb = enc.decode_file(t, len(want) + 16)
    assert nb == nblocks and o.first_diff(_bytes(got), want) == -1
    ver, nb = enc.decode_file(t, len(want) + 16, expected=_cuda(want))        # raises on mismatches != 0
    assert nb == nblocks and o.first_diff(_bytes(ver), want) == -1
    other = bytearray(want)
    other[len(want) // 2] ^= 1
    assert _code(lambda: enc.decode_file(t, len(want) + 16, expected=_cuda(other))) == DATA_ERROR


@pytest.mark.parametrize("name", BUILT)
def test_flipped_payload_byte_in_the_middle_stream(enc, built, name):
    fl = built[name]
    bad = bytearray(fl.raw)
    s1 = fl.parts[1][0]
    first_header = (s1[12] + 1) * 4
    bad[fl.stream_offset(1) + 12 + first_header + (len(s1) - 12 - first_header) // 3] ^= 0x20
    assert x.ref_concat_decode(bytes(bad), len(fl.data) + 16)[0] == DATA_ERROR
    assert _code(lambda: enc.decode_file(_cuda(bad), len(fl.data) + 16)) == DATA_ERROR


def test_own_streams_concatenated(enc):
    """The device encoder's own Streams, presets 1 and 6, with four bytes of Stream Padding between them."""
    data = [o.corpus_mixed(150000, 31), o.corpus_lorem(100001)]
    parts = []
    for d, preset in zip(data, (1, 6)):
        xz, _ = enc.encode(_cuda(d), preset=preset, block_size=BS_OWN)
        parts.append(_bytes(xz))
    raw = parts[0] + b"\0" * 4 + parts[1]
    whole = data[0] + data[1]
    r, want = x.ref_concat_decode(raw, len(whole) + 16)
    assert r == 0 and want == whole
    nblocks = sum((len(d) + BS_OWN - 1) // BS_OWN for d in data)
    got, nb = enc.decode_file(_cuda(raw), len(whole) + 16)
    assert nb == nblocks and o.first_diff(_bytes(got), whole) == -1
    ver, _ = enc.decode_file(_cuda(raw), len(whole) + 16, expected=_cuda(whole))
    assert o.first_diff(_bytes(ver), whole) == -1
    # one Stream alone: the span-parallel verification decode of the single-Stream entry, same result
    one, nb1 = enc.decode_file(_cuda(parts[1]), len(data[1]) + 16, expected=_cuda(data[1]))
    assert nb1 == (len(data[1]) + BS_OWN - 1) // BS_OWN and _bytes(one) == data[1]


def test_good_concat_fixtures_decode_to_nothing(enc):
    for name in ("good-0pad-empty.xz", "good-0cat-empty.xz", "good-0catpad-empty.xz"):
        raw = open(os.path.join(x.CONCAT, name), "rb").read()
        got, nb = enc.decode_file(_cuda(raw), 16)
        assert got.numel() == 0 and nb == 0


def test_single_stream_entry_is_unchanged(enc):
    """Encoder.decode reads one Stream: Stream Padding behind it is refused as before this file reader existed.  The code
    is the one a run of the parent commit's library gave for this file on an MI355X: "xzamd_stream_decode_device failed
    (7): bad magic bytes" (the twelve bytes at the end of the file are not a Stream Footer)."""
    raw = open(os.path.join(x.CONCAT, "good-0pad-empty.xz"), "rb").read()
    import xz_amd
    with pytest.raises(xz_amd.XzAmdError) as ei:
        enc.decode(_cuda(raw), 16)
    assert ei.value.code == 7 and "(7)" in str(ei.value)


# ---------------------------------------------------------------- device parser against host parser
def _good_fixtures():
    out = []
    for p in sorted(glob.glob(os.path.join(x.GOLD, "ref_files*", "*.xz"))):
        raw = open(p, "rb").read()
        if _host_code(raw) == 0:
            out.append((os.path.basename(p), raw))
    return out


def test_device_index_equals_host_index(enc, built):
    import xz_amd
    cases = [(n, built[n].raw) for n in BUILT] + _good_fixtures()
    assert len(cases) >= 4 + 30
    for name, raw in cases:
        assert enc.file_index(_cuda(raw)) == xz_amd.file_index(raw), name


def test_device_codes_equal_host_codes(enc, built):
    bad = []
    for p in sorted(glob.glob(os.path.join(x.GOLD, "ref_files*", "*.xz"))):
        raw = open(p, "rb").read()
        if _host_code(raw) != 0:
            bad.append((os.path.basename(p), raw))
    assert len(bad) >= 10
    for n in ("checks-p0", "delta-p1"):
        bad += [(f"{n}/{k}", raw) for k, raw in x.corruptions(built[n]).items()]
    bad.append(("first byte", b"\xfc" + built["checks-p0"].raw[1:]))
    for name, raw in bad:
        want = _host_code(raw)
        assert want != 0, name
        t = _cuda(raw)
        assert _code(lambda: enc.file_index(t)) == want, name
        assert _code(lambda: enc.decode_file(t, 1 << 20)) == want, name
        assert _code(lambda: enc.decode_range(t, 0, 16)) == want, name          # every defect here is in the framing or in Block 0


def test_decode_refuses_what_the_reference_refuses(enc):
    """Every file of the reference's collection held here, through decode_file: the reference's verdict, but for the
    declined BCJ start offset."""
    n = 0
    for p in sorted(glob.glob(os.path.join(x.GOLD, "ref_files*", "*.xz"))):
        raw = open(p, "rb").read()
        r, want = x.ref_concat_decode(raw, 1 << 20)
        t = _cuda(raw)
        if r == 0 and any(4 <= fid <= 0x0B and len(props) == 4 and props != b"\0\0\0\0" for fid, props in f.block_filter_flags(raw)):
            assert _code(lambda: enc.decode_file(t, 1 << 20)) == 8, p
        elif r == 0:
            got, _ = enc.decode_file(t, 1 << 20)
            assert _bytes(got) == want, p
            n += 1
        else:
            assert _code(lambda: enc.decode_file(t, 1 << 20)) == r, p
    assert n >= 20          # 13 + 4 + 3 good files of the three fixture folders that this decoder reads


def _header_corruptions(raw, blocks):
    """name -> Stream with one defect in the framing of ONE Block (not the first), Block Header CRC32 recomputed where
    the defect is not the CRC32 itself."""
    out = {}

    def patched(k, edit, fix_crc=True):
        b = bytearray(raw)
        h = blocks[k]["header_offset"]
        hs = (b[h] + 1) * 4
        edit(b, h, hs)
        if fix_crc:
            b[h + hs - 4: h + hs] = zlib.crc32(bytes(b[h: h + hs - 4])).to_bytes(4, "little")
        return bytes(b)

    def flip(off, v):
        def e(b, h, hs):
            b[h + off if off >= 0 else h + hs + off] ^= v
        return e

    k = 1
    h = blocks[k]["header_offset"]
    hs = (raw[h] + 1) * 4
    assert raw[h + 1] & 0x40, "the reference's threaded encoder writes the Compressed Size"
    _, p = f._vli_get(raw, h + 2)
    _, idpos = f._vli_get(raw, p)                       # behind Compressed Size and Uncompressed Size: the first filter id
    assert raw[h + 1] & 0x83 == 0x80 and raw[idpos: idpos + 2] == b"\x21\x01"
    assert raw[h + hs - 5] == 0 and idpos + 3 <= hs + h - 5, "no Header Padding to spoil"
    out["header-crc"] = patched(k, flip(-1, 0x01), fix_crc=False)
    out["reserved-flag"] = patched(k, flip(1, 0x04))
    out["filter-id-0x0c"] = patched(k, lambda b, h, hs: b.__setitem__(idpos, 0x0C))
    out["header-padding"] = patched(k, flip(-5, 0x01))
    out["compressed-size"] = patched(k, flip(2, 0x01))
    kp = [i for i, bl in enumerate(blocks) if i and bl["unpadded_size"] % 4]
    assert kp, "no Block with Block Padding"
    bl = blocks[kp[0]]
    csz = x.CHECK_SIZE[raw[7] & 0x0F]
    b = bytearray(raw)
    b[bl["header_offset"] + bl["total_size"] - csz - 1] = 0x01
    out["block-padding"] = bytes(b)
    return out


def test_block_framing_codes_equal_the_single_stream_entry(enc):
    import xz_amd
    data = o.corpus_mixed(5 * x.BS + 777, 41)
    raw = o.ref_encode_mt(data, 1, block_size=x.BS)
    _, blocks, _ = xz_amd.file_index(raw)
    assert len(blocks) == 6
    cases = _header_corruptions(raw, blocks)
    assert len(cases) == 6
    seen = set()
    for name, bad in cases.items():
        t = _cuda(bad)
        want = _code(lambda: enc.decode(t, len(data) + 16))
        assert want in (8, 9), name
        seen.add(want)
        assert _code(lambda: enc.file_index(t)) == want, name
        assert _code(lambda: enc.decode_file(t, len(data) + 16)) == want, name
        assert _host_code(bad) == want, name
    assert seen == {8, 9}


# ---------------------------------------------------------------- reads per file
def test_reads_and_launches_do_not_grow_with_the_blocks(enc):
    import xz_amd
    bs = 16384
    d32 = o.corpus_mixed(32 * bs - 5, 51)
    one = o.ref_encode_mt(d32[:bs], 1, block_size=bs)
    many = o.ref_encode_mt(d32, 1, block_size=bs)
    counts = {}
    for name, raw, data, nblocks in (("1", one, d32[:bs], 1), ("32", many, d32, 32), ("2 streams", one + many, d32[:bs] + d32, 33),
                                     ("3 streams", one + many + b"\0" * 8 + one, d32[:bs] + d32 + d32[:bs], 34)):
        got, nb = enc.decode_file(_cuda(raw), len(data) + 16)
        assert nb == nblocks and _bytes(got) == data
        counts[name] = xz_amd.Encoder.debug_file_counters()
        assert counts[name][2] == nblocks
    assert counts["1"][:2] == counts["32"][:2], counts
    assert counts["1"][0] > 0 and counts["1"][1] > 0
    # what a Stream adds: the same from the second to the third as from the first to the second
    r1, r2, r3 = (counts[k][0] for k in ("32", "2 streams", "3 streams"))
    assert 0 < r2 - r1 == r3 - r2 <= 4, counts
    l1, l2, l3 = (counts[k][1] for k in ("32", "2 streams", "3 streams"))
    assert 0 <= l2 - l1 == l3 - l2 <= 2, counts


# ---------------------------------------------------------------- range decode
@pytest.fixture(scope="module")
def ranged():
    data = o.corpus_mixed(8 * x.BS, 61)
    half = len(data) // 2
    s0 = o.ref_encode_mt(data[:half], 1, block_size=x.BS, check=4)
    s1 = o.ref_encode_mt(data[half:], 0, block_size=x.BS, check=1)
    raw = s0 + b"\0" * 4 + s1
    r, want = x.ref_concat_decode(raw, len(data) + 16)
    assert r == 0 and want == data
    return raw, data


B = x.BS
RANGES = [("inside one Block", B + 100, 1000, 1), ("exactly one Block", 2 * B, B, 1), ("across a Block boundary", B - 7, 20, 2), ("across the Stream boundary", 4 * B - 1000, 3000, 2),
          ("three Blocks over the Stream boundary", 3 * B - 1, B + 2, 3), ("the last byte", 8 * B - 1, 1, 1),
          ("the whole file", 0, 8 * B, 8), ("length 0", 3 * B, 0, 0), ("offset at the end", 8 * B, 10, 0),
          ("past the end", 7 * B + 5, 2 * B, 1), ("far behind the end", 1 << 40, 10, 0)]


@pytest.mark.parametrize("name,off,length,nblocks", RANGES, ids=[r[0] for r in RANGES])
def test_range_decode(enc, ranged, name, off, length, nblocks):
    import xz_amd
    raw, data = ranged
    got, nb = enc.decode_range(_cuda(raw), off, length)
    want = data[off: off + length]
    assert nb == nblocks and _bytes(got) == want
    assert xz_amd.Encoder.debug_file_counters()[2] == nblocks


def test_range_decode_looks_only_at_its_blocks(enc, ranged):
    import xz_amd
    raw, data = ranged
    _, blocks, _ = xz_amd.file_index(raw)
    assert len(blocks) == 8
    bad = bytearray(raw)
    bad[blocks[5]["header_offset"] + blocks[5]["total_size"] - 1] ^= 0x80          # last byte of the Check of Block 5
    t = _cuda(bad)
    assert _code(lambda: enc.decode_file(t, len(data) + 16)) == DATA_ERROR
    got, nb = enc.decode_range(t, 2 * B + 5, 3 * B - 5)                              # Blocks 2 .. 4
    assert nb == 3 and _bytes(got) == data[2 * B + 5: 5 * B]
    got, nb = enc.decode_range(t, 6 * B, 2 * B)                                      # Blocks 6, 7
    assert nb == 2 and _bytes(got) == data[6 * B:]
    assert _code(lambda: enc.decode_range(t, 5 * B + 10, 10)) == DATA_ERROR          # inside Block 5
    assert _code(lambda: enc.decode_range(t, 4 * B, 3 * B)) == DATA_ERROR            # Blocks 4 .. 6
    # the framing of a Block outside the range is not looked at either; Stream framing always is
    bad = bytearray(raw)
    bad[blocks[6]["header_offset"] + 1] ^= 0x04
    got, nb = enc.decode_range(_cuda(bad), 100, 100)
    assert nb == 1 and _bytes(got) == data[100:200]
    assert _code(lambda: enc.decode_range(_cuda(raw + b"\0"), 100, 100)) == DATA_ERROR
