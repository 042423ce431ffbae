"""File index of whole .xz files on the host (xz_amd.file_index -> xzamd_file_index_host): concatenated Streams, Stream
Padding, the walk from the end of the file and its error codes, against the verdict of the real liblzma
(lzma_stream_buffer_decode with LZMA_CONCATENATED, oracle/_ref) -- not Python's lzma module, which ignores trailing
data it cannot decode."""
import glob
import os

import pytest

import _filters as f
import _oracle as o
import _xzfiles as x

OK, UNSUPPORTED_CHECK, FORMAT_ERROR, OPTIONS_ERROR, DATA_ERROR, BUF_ERROR = 0, 3, 7, 8, 9, 10


@pytest.fixture(scope="module", autouse=True)
def _ref(product_lib):
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")


def _index(raw):
    """(code, streams, blocks, uncompressed size)"""
    import xz_amd
    try:
        s, b, u = xz_amd.file_index(raw)
        return OK, s, b, u
    except xz_amd.XzAmdError as e:
        assert e.code
        return e.code, None, None, None


def _fixture(name):
    return open(os.path.join(x.CONCAT, name), "rb").read()


@pytest.mark.parametrize("name,nstreams,padding", [("good-0pad-empty.xz", 1, 4), ("good-0cat-empty.xz", 2, 0),
                                                   ("good-0catpad-empty.xz", 2, 4)])
def test_good_concat_fixtures(name, nstreams, padding):
    raw = _fixture(name)
    r, dec = x.ref_concat_decode(raw, 64)
    assert r == OK and dec == b""
    code, streams, blocks, usize = _index(raw)
    assert code == OK and usize == 0 and blocks == []
    assert len(streams) == nstreams and sum(s["padding"] for s in streams) == padding
    assert sum(s["size"] + s["padding"] for s in streams) == len(raw)
    assert all(s["size"] == 32 and s["block_count"] == 0 for s in streams)


@pytest.mark.parametrize("name", ["bad-0pad-empty.xz", "bad-0catpad-empty.xz", "bad-0cat-alone.xz", "bad-0cat-header_magic.xz"])
def test_bad_concat_fixtures(name):
    raw = _fixture(name)
    r, _ = x.ref_concat_decode(raw, 64)
    assert r == DATA_ERROR
    assert _index(raw)[0] == DATA_ERROR         # bad-0cat-header_magic: the magic of a LATER Stream is no format error


def test_format_error_belongs_to_the_first_bytes():
    raw = bytearray(open(os.path.join(x.GOLD, "ref_files", "good-0-empty.xz"), "rb").read())
    raw[0] ^= 1
    assert x.ref_concat_decode(bytes(raw), 64)[0] == FORMAT_ERROR
    assert _index(bytes(raw))[0] == FORMAT_ERROR
    assert _index(b"\xfd7zXZ\0" + b"\0" * 25)[0] == FORMAT_ERROR        # 31 bytes: shorter than an empty Stream
    assert _index(b"")[0] == FORMAT_ERROR


# Files of the reference's collection whose only defect lies in the LZMA2 data or in the Check value: the index reads no
# compressed data, so it lists them; decoding refuses them (tests/test_gpu_decode_file.py).  bad-2-index-1.xz belongs here:
# its Index records are consistent with each other and land on the Stream Header, its Block Headers carry no sizes, so
# only the end of the LZMA2 chunk chain shows that the Unpadded Sizes are wrong.
DATA_DEFECTS = {f"bad-1-lzma2-{i}.xz" for i in range(1, 12)} | {"bad-1-check-crc64.xz", "bad-2-index-1.xz"}


def test_every_reference_fixture():
    """Framing defects give the reference's code; good files list Blocks whose sizes sum to the reference's output.  One
    limit of the device decoder cuts through the good files: a BCJ start offset other than 0 is declined with
    XZAMD_OPTIONS_ERROR (found by reading the Block Header, not by the file's name)."""
    files = sorted(glob.glob(os.path.join(x.GOLD, "ref_files", "*.xz")) + glob.glob(os.path.join(x.GOLD, "ref_files_filters", "*.xz"))
                   + glob.glob(os.path.join(x.CONCAT, "*.xz")))
    assert len(files) >= 43
    ngood = nframing = ndata = 0
    for p in files:
        raw = open(p, "rb").read()
        name = os.path.basename(p)
        r, dec = x.ref_concat_decode(raw, 1 << 20)
        code, streams, blocks, usize = _index(raw)
        if r == OK:
            if any(4 <= fid <= 0x0B and len(props) == 4 and props != b"\0\0\0\0" for fid, props in f.block_filter_flags(raw)):
                assert code == OPTIONS_ERROR, name
                continue
            assert code == OK, (name, code)
            assert usize == len(dec) == sum(b["uncompressed_size"] for b in blocks), name
            assert sum(s["size"] + s["padding"] for s in streams) == len(raw), name
            assert sum(b["total_size"] for b in blocks) == sum(s["size"] - 24 - x.index_size(raw[s["offset"]: s["offset"] + s["size"]])
                                                               for s in streams), name
            ngood += 1
        elif name in DATA_DEFECTS:
            assert code == OK and r == DATA_ERROR, (name, code, r)
            ndata += 1
        else:
            assert code == r, (name, code, r)
            nframing += 1
    assert ngood >= 19 and nframing >= 9 and ndata == 13


@pytest.fixture(scope="module")
def built():
    return x.built_files()


@pytest.mark.parametrize("name", ["checks-p0", "checks-p1", "delta-p0", "delta-p1"])
def test_built_files_list_what_their_parts_hold(built, name):
    fl = built[name]
    want = b"".join(o.ref_decode(s, len(d) + 16)[1] for s, d, _ in fl.parts)
    assert want == fl.data
    r, dec = x.ref_concat_decode(fl.raw, len(fl.data) + 16)
    assert r == OK and dec == want
    code, streams, blocks, usize = _index(fl.raw)
    assert code == OK and usize == len(fl.data)
    es, eb = x.expected_layout(fl)
    assert streams == es
    assert len(blocks) == len(eb)
    for got, exp in zip(blocks, eb):
        assert {k: got[k] for k in exp} == exp
        assert got["total_size"] == (got["unpadded_size"] + 3) & ~3
        assert got["filter_ids"] == ((3, 0x21) if name.startswith("delta") and got["stream"] == 1 else (0x21,))
    for i, s in enumerate(streams):
        mine = blocks[s["first_block"]: s["first_block"] + s["block_count"]]
        assert mine[0]["header_offset"] == s["offset"] + 12
        for a, b in zip(mine, mine[1:]):
            assert b["header_offset"] == a["header_offset"] + a["total_size"]
        # the Blocks end where the Index of their Stream starts
        assert mine[-1]["header_offset"] + mine[-1]["total_size"] == s["offset"] + s["size"] - 12 - x.index_size(fl.parts[i][0])


def test_capacities(built):
    import ctypes as C
    import xz_amd
    raw = built["checks-p0"].raw
    ns, nb, usz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    lib = xz_amd.lib()
    rc = lib.xzamd_file_index_host(raw, len(raw), None, 0, C.byref(ns), None, 0, C.byref(nb), C.byref(usz))
    assert rc == BUF_ERROR and (ns.value, nb.value, usz.value) == (3, 6, len(built["checks-p0"].data))
    streams, blocks = (xz_amd.XzStream * 3)(), (xz_amd.XzBlock * 5)()
    assert lib.xzamd_file_index_host(raw, len(raw), streams, 3, C.byref(ns), blocks, 5, C.byref(nb), C.byref(usz)) == BUF_ERROR


CORRUPTIONS = ["pad3-middle", "pad5-middle", "pad3-end", "pad5-end", "footer-crc", "backward-size", "truncated-first-alone",
               "truncated-first"]


@pytest.mark.parametrize("kind", CORRUPTIONS)
@pytest.mark.parametrize("name", ["checks-p0", "delta-p1"])
def test_single_corruptions_give_the_reference_code(built, name, kind):
    raw = x.corruptions(built[name])[kind]
    r, _ = x.ref_concat_decode(raw, len(built[name].data) + 16)
    assert r not in (OK, BUF_ERROR)
    assert _index(raw)[0] == r


def test_unsupported_check_in_any_stream(built):
    """A Check id without a verifier is reported, not skipped -- in whichever Stream it stands (the reference without
    LZMA_TELL_UNSUPPORTED_CHECK decodes such a Stream and does not verify it)."""
    import zlib
    a = built["checks-p0"].parts[1][0]
    empty = open(os.path.join(x.GOLD, "ref_files", "good-0-empty.xz"), "rb").read()
    sf = bytes([0, 2])                                                  # a reserved Check id: four bytes, no verifier
    foot = empty[-8:-4] + sf
    odd = empty[:6] + sf + zlib.crc32(sf).to_bytes(4, "little") + empty[12:-12] + zlib.crc32(foot).to_bytes(4, "little") + foot + b"YZ"
    for raw in (a + odd, odd + a, a + odd + b"\0" * 4 + a):
        assert x.ref_concat_decode(raw, 1 << 10)[0] == OK
        assert _index(raw)[0] == UNSUPPORTED_CHECK
