"""Helpers shared by the filter-chain decoder tests: the reference's forward filters (through the real liblzma of
oracle/_ref), a numpy model of the delta filter, inputs on which the BCJ filters convert something, and a writer of
single-Block .xz Streams with hand-made Filter Flags."""
import ctypes as C
import os
import zlib

import numpy as np

import _oracle as o

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_files_filters")
BCJ = {"x86": 4, "powerpc": 5, "ia64": 6, "arm": 7, "armthumb": 8, "sparc": 9, "arm64": 0x0A, "riscv": 0x0B}
DELTA = 3
LZMA2 = 0x21
TILE = 16384            # bytes of a Block one wavefront of the delta scan handles (XZAMD_UNF_TILE)

_lz = None


class _Filter(C.Structure):
    _fields_ = [("id", C.c_uint64), ("options", C.c_void_p)]


def _liblzma():
    global _lz
    if _lz is None:
        _lz = C.CDLL(os.path.join(o.ORACLE_DIR, "_ref", "liblzma_ref.so"))
        _lz.lzma_raw_buffer_encode.argtypes = [C.POINTER(_Filter), C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p,
                                               C.POINTER(C.c_size_t), C.c_size_t]
        _lz.lzma_raw_buffer_decode.argtypes = [C.POINTER(_Filter), C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t,
                                               C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t]
        _lz.lzma_lzma_preset.argtypes = [C.c_void_p, C.c_uint32]
    return _lz


def ref_forward(data, chain):
    """What the reference's encoder-side filters make of one Block: chain = [(filter id, delta distance), ...] in
    Block Header order.  {chain, LZMA2} raw-encoded, then raw-decoded as {LZMA2} alone."""
    lz = _liblzma()
    data = bytes(data)
    opt = C.create_string_buffer(512)
    assert lz.lzma_lzma_preset(opt, 0) == 0
    dl = [C.create_string_buffer(64) for _ in chain]
    enc = (_Filter * (len(chain) + 2))()
    for i, (fid, dist) in enumerate(chain):
        enc[i].id = fid
        if fid == DELTA:
            C.memmove(dl[i], np.array([0, dist], dtype=np.uint32).tobytes(), 8)      # LZMA_DELTA_TYPE_BYTE, dist
            enc[i].options = C.addressof(dl[i])
    enc[len(chain)].id = LZMA2
    enc[len(chain)].options = C.addressof(opt)
    enc[len(chain) + 1].id = (1 << 64) - 1          # LZMA_VLI_UNKNOWN
    dec = (_Filter * 2)()
    dec[0].id, dec[0].options = LZMA2, C.addressof(opt)
    dec[1].id = (1 << 64) - 1
    cap = len(data) + len(data) // 4 + 65536
    tmp = C.create_string_buffer(cap)
    tpos = C.c_size_t(0)
    assert lz.lzma_raw_buffer_encode(enc, None, data, len(data), tmp, C.byref(tpos), cap) == 0
    out = C.create_string_buffer(max(len(data), 1))
    ipos, opos = C.c_size_t(0), C.c_size_t(0)
    assert lz.lzma_raw_buffer_decode(dec, None, tmp, C.byref(ipos), tpos.value, out, C.byref(opos), len(data)) == 0
    assert opos.value == len(data)
    return out.raw[: len(data)]


def np_delta_forward(data, dist):
    """delta encoder of one Block: byte minus the byte `dist` before it, zero history."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    f = a.copy()
    if len(a) > dist:
        f[dist:] = a[dist:] - a[:-dist]
    return f.tobytes()


def np_delta_inverse(data, dist):
    """delta decoder of one Block: dist interleaved prefix sums modulo 256 (np.cumsum per residue class)."""
    f = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty_like(f)
    for r in range(min(dist, len(f))):
        out[r::dist] = np.cumsum(f[r::dist], dtype=np.uint8)
    return out.tobytes()


def ramp_noise(n, seed, width):
    """int16 / int32 ramp plus small noise: what a delta filter is for."""
    rng = np.random.default_rng(seed)
    dt = np.int16 if width == 2 else np.int32
    k = n // width + 1
    v = (np.arange(k, dtype=np.int64) * 37 + rng.integers(-3, 4, k)).astype(dt)
    return v.tobytes()[:n]


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _vli_get(b, p):
    v, s = 0, 0
    while True:
        c = b[p]
        p += 1
        v |= (c & 0x7F) << s
        s += 7
        if not c & 0x80:
            return v, p


CHECK_SIZE = {0: 0, 1: 4, 4: 8, 10: 32}


def parse_single_block(raw):
    """(check id, filter-flags bytes, number of filters, LZMA2 payload, check bytes, uncompressed size) of a
    single-Block Stream."""
    check = raw[7] & 0x0F
    isz = (int.from_bytes(raw[-8:-4], "little") + 1) * 4
    idx = raw[len(raw) - 12 - isz: len(raw) - 12]
    assert idx[0] == 0 and idx[1] == 1, "one Block expected"
    unpadded, p = _vli_get(idx, 2)
    usize, p = _vli_get(idx, p)
    hs = (raw[12] + 1) * 4
    flags = raw[13]
    p = 14
    if flags & 0x40:
        _, p = _vli_get(raw, p)
    if flags & 0x80:
        _, p = _vli_get(raw, p)
    nf = (flags & 3) + 1
    q = p
    for _ in range(nf):
        _, q = _vli_get(raw, q)
        ps, q = _vli_get(raw, q)
        q += ps
    csize = unpadded - hs - CHECK_SIZE[check]
    payload = raw[12 + hs: 12 + hs + csize]
    pad = (-csize) % 4
    chk = raw[12 + hs + csize + pad: 12 + hs + csize + pad + CHECK_SIZE[check]]
    return check, bytes(raw[p:q]), nf, bytes(payload), bytes(chk), usize


def block_filter_flags(raw):
    """[(filter id, properties bytes), ...] of the first Block Header of a Stream."""
    flags = raw[13]
    p = 14
    if flags & 0x40:
        _, p = _vli_get(raw, p)
    if flags & 0x80:
        _, p = _vli_get(raw, p)
    out = []
    for _ in range((flags & 3) + 1):
        fid, p = _vli_get(raw, p)
        ps, p = _vli_get(raw, p)
        out.append((fid, bytes(raw[p:p + ps])))
        p += ps
    return out


def single_block_stream(check, filter_flags, nf, payload, chk, usize, header_pad=b""):
    """A single-Block .xz Stream around an LZMA2 payload with the given Filter Flags bytes (CRC32s computed here)."""
    body = bytes([0xC0 | (nf - 1)]) + vli(len(payload)) + vli(usize) + filter_flags + header_pad
    body += b"\0" * ((-(len(body) + 1)) % 4)
    hdr = bytes([(len(body) + 1 + 4) // 4 - 1]) + body
    hdr += zlib.crc32(hdr).to_bytes(4, "little")
    sflags = bytes([0, check])
    out = b"\xfd7zXZ\0" + sflags + zlib.crc32(sflags).to_bytes(4, "little")
    out += hdr + payload + b"\0" * ((-len(payload)) % 4) + chk
    idx = b"\0\x01" + vli(len(hdr) + len(payload) + len(chk)) + vli(usize)
    idx += b"\0" * ((-len(idx)) % 4)
    idx += zlib.crc32(idx).to_bytes(4, "little")
    foot = (len(idx) // 4 - 1).to_bytes(4, "little") + sflags
    out += idx + zlib.crc32(foot).to_bytes(4, "little") + foot + b"YZ"
    return out
