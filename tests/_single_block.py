"""Helpers of the single-Block tests: a segmented one-Block .xz Stream made with Python's lzma module (raw LZMA2 encodings
whose end markers are cut, concatenated behind a Block Header without sizes), a parser for such Streams, and a ctypes
driver for lzma_easy_encoder / lzma_stream_encoder_mt of libxz_amd.so."""
import ctypes as C
import lzma
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT_SIZE = 1 << 20
DICT_BYTE = 16                       # 1 MiB (lzma2_encoder.c:376-400)
RUN, SYNC_FLUSH, FULL_FLUSH, FINISH, FULL_BARRIER = 0, 1, 2, 3, 4

_T64 = []
for _i in range(256):
    _r = _i
    for _ in range(8):
        _r = (_r >> 1) ^ (0xC96C5795D7870F42 if _r & 1 else 0)
    _T64.append(_r)


def crc64(data, crc=0):
    c = crc ^ 0xFFFFFFFFFFFFFFFF
    for b in data:
        c = _T64[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFFFFFFFFFF


def liblzma_crc64(data):
    """The CRC64 liblzma itself writes: the Check field of a one-Block Stream from lzma.compress (no data: no Block)."""
    if len(data) == 0:
        return 0
    raw = lzma.compress(data, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, preset=0)
    index_size = (struct.unpack("<I", raw[-8:-4])[0] + 1) * 4
    end = len(raw) - 12 - index_size
    return struct.unpack("<Q", raw[end - 8:end])[0]


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def stream_header(check):
    flags = bytes([0, check])
    return b"\xfd7zXZ\0" + flags + struct.pack("<I", zlib.crc32(flags))


def index_footer(records, check):
    idx = b"\0" + vli(len(records)) + b"".join(vli(u) + vli(n) for u, n in records)
    idx += b"\0" * (-len(idx) % 4)
    idx += struct.pack("<I", zlib.crc32(idx))
    body = struct.pack("<I", len(idx) // 4 - 1) + bytes([0, check])
    return idx + struct.pack("<I", zlib.crc32(body)) + body + b"YZ"


def block_header_nosizes(dict_byte=DICT_BYTE):
    h = bytes([0x02, 0x00, 0x21, 0x01, dict_byte, 0, 0, 0])
    return h + struct.pack("<I", zlib.crc32(h))


def raw_chain(data):
    """The LZMA2 chunk chain of `data` (Python's lzma, raw), end marker cut: starts with a dictionary reset."""
    raw = lzma.compress(data, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": 6, "dict_size": DICT_SIZE}])
    assert raw[-1] == 0 and (raw[0] == 0x01 or raw[0] >= 0xE0)
    return raw[:-1]


class Segmented:
    """raw = the file; data = what it decodes to; seg_off[i] = file offset of segment i's chunk chain; seg_upos[i]"""

    def __init__(self, segments):
        chains = [raw_chain(s) for s in segments]
        self.data = b"".join(segments)
        payload = b"".join(chains) + b"\0"
        pos = 24
        self.seg_off, self.seg_upos, self.seg_len = [], [], []
        u = 0
        for s, c in zip(segments, chains):
            self.seg_off.append(pos)
            self.seg_upos.append(u)
            self.seg_len.append(len(c))
            pos += len(c)
            u += len(s)
        self.csize = len(payload)
        self.unpadded = 12 + len(payload) + 8
        self.raw = (stream_header(4) + block_header_nosizes() + payload + b"\0" * (-len(payload) % 4)
                    + struct.pack("<Q", crc64(self.data)) + index_footer([(self.unpadded, len(self.data))], 4))


def periodic(n, period, seed):
    rng = np.random.default_rng(seed)
    base = bytes(rng.integers(0, 256, size=period, dtype=np.uint8))
    return (base * (n // period + 1))[:n]


def text(n):
    import _oracle as o
    return o.corpus_lorem(n)


_FOUR = None


def four_segments():
    """30,000 B periodic, 60,000 B periodic, 70,000 B random (comes out as 0x01 / 0x02 chunks), 60,000 B text."""
    global _FOUR
    if _FOUR is None:
        rnd = bytes(np.random.default_rng(11).integers(0, 256, size=70000, dtype=np.uint8))
        _FOUR = Segmented([periodic(30000, 300, 1), periodic(60000, 777, 2), rnd, text(60000)])
    return _FOUR


def many_segments(count, size):
    t = text(count * size)
    return Segmented([t[i * size:(i + 1) * size] for i in range(count)])


def parse_blocks(raw):
    """[(header offset, header size, LZMA2 data, uncompressed size)] of a single-Stream file, from its Index."""
    import xz_amd
    streams, blocks, _ = xz_amd.file_index(raw)
    assert len(streams) == 1
    csz = {0: 0, 1: 4, 4: 8, 10: 32}[streams[0]["check"]]
    out = []
    for b in blocks:
        ho = b["header_offset"]
        hs = (raw[ho] + 1) * 4
        out.append((ho, hs, raw[ho + hs: ho + b["unpadded_size"] - csz], b["uncompressed_size"]))
    return out


# ---- ctypes driver of the liblzma entry points of libxz_amd.so ----
def _structs():
    t = os.path.join(ROOT, "tools")
    if t not in sys.path:
        sys.path.insert(0, t)
    from bench_lzma_code import Mt, Stream
    return Mt, Stream


def lzma_encode(data, preset, check=4, piece=None, flushes=(), mt_block_size=None):
    """Encode through lzma_code.  mt_block_size None: lzma_easy_encoder; else lzma_stream_encoder_mt with that Block size.
    piece: bytes per lzma_code(LZMA_RUN) call (None: everything with the closing action).  flushes: [(position, action)].
    Returns (output, [bytes handed out when each flush returned LZMA_STREAM_END])."""
    import xz_amd
    Mt, Stream = _structs()
    L = xz_amd.lib()
    ib = C.create_string_buffer(bytes(data), max(len(data), 1))
    ob = C.create_string_buffer(len(data) + len(data) // 8 + (1 << 16))
    s = Stream()
    if mt_block_size is None:
        L.lzma_easy_encoder.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        rc = L.lzma_easy_encoder(C.byref(s), preset, check)
    else:
        m = Mt(threads=1, preset=preset, check=check, block_size=mt_block_size, timeout=0)
        rc = L.lzma_stream_encoder_mt(C.byref(s), C.byref(m))
    assert rc == 0, rc
    s.next_out, s.avail_out = C.cast(ob, C.c_void_p).value, len(ob)
    base = C.cast(ib, C.c_void_p).value
    pos, cuts = 0, []
    for stop, action in list(flushes) + [(len(data), FINISH)]:
        if piece is not None:
            while stop - pos > 0:
                k = min(piece, stop - pos)
                s.next_in, s.avail_in = base + pos, k
                while s.avail_in:
                    assert L.lzma_code(C.byref(s), RUN) == 0
                pos += k
        s.next_in, s.avail_in = base + pos, stop - pos
        pos = stop
        r = L.lzma_code(C.byref(s), action)
        while r == 0:
            r = L.lzma_code(C.byref(s), action)
        assert r == 1 and s.avail_in == 0, r
        cuts.append(s.total_out)
    out = ob.raw[: s.total_out]
    L.lzma_end(C.byref(s))
    return out, cuts[:-1]
