"""Helpers shared by the whole-file decoder tests (test_file_index.py, test_gpu_decode_file.py): the verdict of the real
liblzma (oracle/_ref) with LZMA_CONCATENATED, files built from Streams of the reference encoder, and single corruptions
of them."""
import ctypes as C
import os
import zlib

import numpy as np

import _oracle as o

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONCAT = os.path.join(GOLD, "ref_files_concat")
LZMA_CONCATENATED = 0x08
BS = 65536
CHECK_SIZE = {0: 0, 1: 4, 4: 8, 10: 32}

_lz = None


def ref_concat_decode(raw, out_cap):
    """(lzma_ret, decoded bytes) of lzma_stream_buffer_decode with flags = LZMA_CONCATENATED: what `xz -d` says."""
    global _lz
    if _lz is None:
        _lz = C.CDLL(os.path.join(o.ORACLE_DIR, "_ref", "liblzma_ref.so"))
        _lz.lzma_stream_buffer_decode.restype = C.c_int
        _lz.lzma_stream_buffer_decode.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p, C.c_char_p,
                                                  C.POINTER(C.c_size_t), C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t),
                                                  C.c_size_t]
    raw = bytes(raw)
    out = C.create_string_buffer(max(out_cap, 1))
    memlimit = C.c_uint64((1 << 64) - 1)
    ipos, opos = C.c_size_t(0), C.c_size_t(0)
    r = _lz.lzma_stream_buffer_decode(C.byref(memlimit), LZMA_CONCATENATED, None, raw, C.byref(ipos), len(raw), out,
                                      C.byref(opos), out_cap)
    return r, out.raw[: opos.value]


class Built:
    """A file of several Streams: .raw, .parts [(Stream bytes, its data, padding behind it)], .data."""

    def __init__(self, parts):
        self.parts = parts
        self.raw = b"".join(s + b"\0" * pad for s, _, pad in parts)
        self.data = b"".join(d for _, d, _ in parts)

    def stream_offset(self, i):
        return sum(len(s) + pad for s, _, pad in self.parts[:i])


_INPUTS = None


def inputs():
    """The three inputs of the issue: 1 B, 64 KiB exactly, 200 KiB."""
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = (b"x", o.corpus_mixed(BS, 21), o.corpus_mixed(200 << 10, 22))
    return _INPUTS


_BUILT = {}


def built_files():
    """name -> Built.  Per preset (0, 1): three Streams with the Checks none, CRC32 and SHA-256 (Stream Padding 0 / 4 /
    8 between them over the two presets, 4 at the end), and one {delta, LZMA2} Stream between two plain ones."""
    if not _BUILT:
        a, b, c = inputs()
        for preset, gaps in ((0, (0, 4)), (1, (8, 4))):
            _BUILT[f"checks-p{preset}"] = Built([
                (o.ref_encode_mt(c, preset, block_size=BS, check=0), c, gaps[0]),
                (o.ref_encode_mt(a, preset, block_size=BS, check=1), a, gaps[1]),
                (o.ref_encode_mt(b, preset, block_size=BS, check=10), b, 4)])
            _BUILT[f"delta-p{preset}"] = Built([
                (o.ref_encode_mt(b, preset, block_size=BS), b, 0),
                (o.ref_encode_mt_chain(c, preset, 3, 4, block_size=BS), c, 4),
                (o.ref_encode_mt(a, preset, block_size=BS), a, 0)])
    return _BUILT


def index_size(stream):
    return (int.from_bytes(stream[-8:-4], "little") + 1) * 4


def corruptions(f):
    """name -> bytes: single corruptions of the framing of a Built file of three Streams."""
    s0, s1, s2 = (p[0] for p in f.parts)
    p0, p1, p2 = (p[2] for p in f.parts)
    z = lambda n: b"\0" * n
    out = {}
    out["pad3-middle"] = s0 + z(3) + s1 + z(p1) + s2 + z(p2)
    out["pad5-middle"] = s0 + z(p0) + s1 + z(5) + s2 + z(p2)
    out["pad3-end"] = s0 + z(p0) + s1 + z(p1) + s2 + z(3)
    out["pad5-end"] = s0 + z(p0) + s1 + z(p1) + s2 + z(5)
    bad = bytearray(s1)
    bad[-12] ^= 0x10                                            # first byte of the Stream Footer: its CRC32
    out["footer-crc"] = s0 + z(p0) + bytes(bad) + z(p1) + s2 + z(p2)
    foot = (int.from_bytes(s1[-8:-4], "little") + 1).to_bytes(4, "little") + s1[-4:-2]
    bad = s1[:-12] + zlib.crc32(foot).to_bytes(4, "little") + foot + b"YZ"
    out["backward-size"] = s0 + z(p0) + bad + z(p1) + s2 + z(p2)
    cut = (len(s0) * 3 // 5) & ~3
    assert cut >= 32
    out["truncated-first-alone"] = s0[:cut]
    out["truncated-first"] = s0[:cut] + z(p0) + s1 + z(p1) + s2 + z(p2)
    return out


def expected_layout(f):
    """(streams, blocks) a correct index of a Built file lists, from the parts alone."""
    streams, blocks = [], []
    uoff = 0
    for i, (s, d, pad) in enumerate(f.parts):
        nb = max(1, (len(d) + BS - 1) // BS) if len(d) else 0
        streams.append(dict(offset=f.stream_offset(i), size=len(s), padding=pad, first_block=len(blocks), block_count=nb,
                            uncompressed_offset=uoff, uncompressed_size=len(d), check=s[7] & 0x0F))
        for b in range(nb):
            blocks.append(dict(stream=i, uncompressed_offset=uoff + b * BS, uncompressed_size=min(BS, len(d) - b * BS)))
        uoff += len(d)
    return streams, blocks


def as_np(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)
