"""Helpers of the forward-decode tests (test_gpu_decode_forward.py): the real liblzma's streaming decoder
(lzma_stream_decoder / lzma_code of oracle/_ref) on a feed and drain schedule, and Streams rewritten so that their Block
Headers carry no sizes (what lzma_stream_encoder and `xz -T1` write)."""
import ctypes as C
import os
import zlib

import _oracle as o
import _xzfiles as x

LZMA_RUN, LZMA_FINISH = 0, 3
LZMA_OK, LZMA_STREAM_END, LZMA_BUF_ERROR = 0, 1, 10
LZMA_CONCATENATED = 0x08


class LzmaStream(C.Structure):
    """lzma_stream (api/lzma/base.h)"""
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_size_t), ("total_in", C.c_uint64),
                ("next_out", C.c_void_p), ("avail_out", C.c_size_t), ("total_out", C.c_uint64),
                ("allocator", C.c_void_p), ("internal", C.c_void_p),
                ("rp1", C.c_void_p), ("rp2", C.c_void_p), ("rp3", C.c_void_p), ("rp4", C.c_void_p),
                ("seek_pos", C.c_uint64), ("ri2", C.c_uint64), ("ri3", C.c_size_t), ("ri4", C.c_size_t),
                ("re1", C.c_int), ("re2", C.c_int)]


class LzmaMt(C.Structure):
    """lzma_mt (api/lzma/container.h)"""
    _fields_ = [("flags", C.c_uint32), ("threads", C.c_uint32), ("block_size", C.c_uint64),
                ("timeout", C.c_uint32), ("preset", C.c_uint32), ("filters", C.c_void_p),
                ("check", C.c_int), ("re1", C.c_int), ("re2", C.c_int), ("re3", C.c_int),
                ("ri1", C.c_uint32), ("ri2", C.c_uint32), ("ri3", C.c_uint32), ("ri4", C.c_uint32),
                ("memlimit_threading", C.c_uint64), ("memlimit_stop", C.c_uint64),
                ("ri7", C.c_uint64), ("ri8", C.c_uint64),
                ("rp1", C.c_void_p), ("rp2", C.c_void_p), ("rp3", C.c_void_p), ("rp4", C.c_void_p)]


def bind(L):
    """argument types of the decoder ABI on a loaded liblzma (the reference's, or libxz_amd.so)"""
    L.lzma_stream_decoder.restype = C.c_int
    L.lzma_stream_decoder.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
    L.lzma_stream_decoder_mt.restype = C.c_int
    L.lzma_stream_decoder_mt.argtypes = [C.c_void_p, C.c_void_p]
    L.lzma_code.restype = C.c_int
    L.lzma_code.argtypes = [C.c_void_p, C.c_int]
    L.lzma_end.restype = None
    L.lzma_end.argtypes = [C.c_void_p]
    L.lzma_get_check.restype = C.c_int
    L.lzma_get_check.argtypes = [C.c_void_p]
    return L


_lz = None


def ref_lib():
    global _lz
    if _lz is None:
        _lz = bind(C.CDLL(os.path.join(o.ORACLE_DIR, "_ref", "liblzma_ref.so")))
    return _lz


def stream_decode(L, raw, out_cap, flags=LZMA_CONCATENATED, in_piece=None, out_piece=None, notices_out=None, mt=False, checks_out=None):
    """`raw` through L.lzma_stream_decoder / lzma_code: in_piece bytes per call (None: all at once), out_piece bytes of
    room per call (None: out_cap), LZMA_FINISH once the last input byte has been handed over.
    Returns (final lzma_ret, decoded bytes, total_in, total_out).  notices_out / checks_out: every LZMA_NO_CHECK,
    LZMA_UNSUPPORTED_CHECK and LZMA_GET_CHECK answer on the way (an LZMA_UNSUPPORTED_CHECK straight behind another ends the run: it
    is the coder's verdict) and lzma_get_check at each."""
    raw = bytes(raw)
    s = LzmaStream()
    if mt:
        opt = LzmaMt(flags=flags, threads=2, memlimit_threading=(1 << 64) - 1, memlimit_stop=(1 << 64) - 1)
        r = L.lzma_stream_decoder_mt(C.byref(s), C.byref(opt))
    else:
        r = L.lzma_stream_decoder(C.byref(s), (1 << 64) - 1, flags)
    assert r == 0, r
    notices, last = [], 0
    src = C.create_string_buffer(raw, max(len(raw), 1))
    dst = C.create_string_buffer(max(out_cap, 1))
    ibase, obase = C.addressof(src), C.addressof(dst)
    fed = done = 0
    try:
        while True:
            if s.avail_in == 0 and fed < len(raw):
                k = len(raw) - fed if in_piece is None else min(in_piece, len(raw) - fed)
                s.next_in, s.avail_in = ibase + fed, k
                fed += k
            room = out_cap - done if out_piece is None else min(out_piece, out_cap - done)
            s.next_out, s.avail_out = obase + done, room
            r = L.lzma_code(C.byref(s), LZMA_FINISH if fed == len(raw) else LZMA_RUN)
            done += room - s.avail_out
            if r in (2, 3, 4) and not (r == 3 and last == 3):      # LZMA_NO_CHECK / _UNSUPPORTED_CHECK / _GET_CHECK: notices
                notices.append(r)
                if checks_out is not None:
                    checks_out.append(L.lzma_get_check(C.byref(s)))
                last = r
                continue
            last = 0
            if r != LZMA_OK or (room == 0 and done == out_cap):
                break
        if notices_out is not None:
            notices_out.extend(notices)
        return r, dst.raw[:done], s.total_in, s.total_out
    finally:
        L.lzma_end(C.byref(s))


def _vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _vli_get(b, pos):
    """(value, offset behind it) of the variable-length integer at b[pos]"""
    v = shift = 0
    while True:
        c = b[pos]
        pos += 1
        v |= (c & 0x7F) << shift
        shift += 7
        if not c & 0x80:
            return v, pos


def index_footer(check, pairs):
    """Index and Stream Footer of Blocks with the (Unpadded Size, Uncompressed Size) `pairs`."""
    idx = b"\0" + _vli(len(pairs)) + b"".join(_vli(u) + _vli(n) for u, n in pairs)
    idx += b"\0" * (-len(idx) % 4)
    idx += zlib.crc32(idx).to_bytes(4, "little")
    tail = (len(idx) // 4 - 1).to_bytes(4, "little") + bytes([0, check])
    return idx + zlib.crc32(tail).to_bytes(4, "little") + tail + b"YZ"


def blocks_of(stream):
    """[(header offset, header size, Compressed Size, Uncompressed Size, end of the Filter Flags)] of a Stream whose Block
    Headers carry both sizes (what the threaded encoders write)."""
    out, pos = [], 12
    while stream[pos] != 0:
        hs = (stream[pos] + 1) * 4
        assert stream[pos + 1] & 0xC0 == 0xC0, "a Block Header without sizes"
        csize, p = _vli_get(stream, pos + 2)
        usize, p = _vli_get(stream, p)
        q = p
        for _ in range((stream[pos + 1] & 3) + 1):
            _, q = _vli_get(stream, q)
            n, q = _vli_get(stream, q)
            q += n
        out.append((pos, hs, csize, usize, p, q))
        pos += ((hs + csize + 3) & ~3) + x.CHECK_SIZE[stream[7] & 0x0F]
    return out, pos


def strip_sizes(stream):
    """The same Stream with Block Headers that carry neither Compressed Size nor Uncompressed Size; Index and Footer
    rebuilt for the shorter headers."""
    stream = bytes(stream)
    check = stream[7] & 0x0F
    csz = x.CHECK_SIZE[check]
    blocks, _ = blocks_of(stream)
    out, pairs = bytearray(stream[:12]), []
    for pos, hs, csize, usize, fstart, fend in blocks:
        body = bytes([stream[pos + 1] & 0x03]) + stream[fstart:fend]
        hs2 = (1 + len(body) + 4 + 3) & ~3
        hdr = bytes([hs2 // 4 - 1]) + body + b"\0" * (hs2 - 5 - len(body))
        hdr += zlib.crc32(hdr).to_bytes(4, "little")
        out += hdr + stream[pos + hs: pos + hs + csize]
        out += b"\0" * (-(hs2 + csize) % 4)
        old_check = pos + ((hs + csize + 3) & ~3)
        out += stream[old_check: old_check + csz]
        pairs.append((hs2 + csize + csz, usize))
    return bytes(out) + index_footer(check, pairs)


def stored_stream(data, block_size, check=1, sizes=True):
    """An .xz Stream of stored Blocks (uncompressed LZMA2 chunks) made here, without any encoder.  check: none (0), CRC32 (1),
    or any other id -- its Check field then holds zeros of the id's size, for ids no decoder here verifies (2, 3: four
    bytes) or that a test never lets a decoder get as far as."""
    csz = (0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64)[check]
    flags = bytes([0, check])
    out = bytearray(b"\xfd7zXZ\0" + flags + zlib.crc32(flags).to_bytes(4, "little"))
    pairs = []
    for at in range(0, len(data), block_size):
        blk = data[at: at + block_size]
        chain = bytearray()
        for c in range(0, len(blk), 65536):
            piece = blk[c: c + 65536]
            chain += bytes([1 if c == 0 else 2]) + (len(piece) - 1).to_bytes(2, "big") + piece
        chain += b"\0"
        body = (bytes([0xC0]) + _vli(len(chain)) + _vli(len(blk)) if sizes else bytes([0])) + b"\x21\x01\x10"
        hs = (1 + len(body) + 4 + 3) & ~3
        hdr = bytes([hs // 4 - 1]) + body + b"\0" * (hs - 5 - len(body))
        hdr += zlib.crc32(hdr).to_bytes(4, "little")
        out += hdr + chain + b"\0" * (-(hs + len(chain)) % 4)
        out += zlib.crc32(blk).to_bytes(4, "little") if check == 1 else b"\0" * csz
        pairs.append((hs + len(chain) + csz, len(blk)))
    return bytes(out) + index_footer(check, pairs)
