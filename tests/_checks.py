"""Helpers of the edge tests of filters and Block Checks (test_checks_model.py, test_gpu_auto_delta_ragged.py,
test_gpu_block_check_edges.py, test_gpu_bcj_seams.py).  The arbiter of these tests is Python's `lzma` module, that is the
system's liblzma: nothing here comes from the kernels under test.  CPU only."""
import hashlib
import lzma
import zlib

import _filters as fl
import _forward as fw

CHECK_SIZE = {0: 0, 1: 4, 4: 8, 10: 32}
_CRC64_POLY = 0xC96C5795D7870F42           # ECMA-182, reflected
_CRC64_TAB = None


def crc64(data):
    """CRC64 of the .xz format, one table lookup per byte.  Slow: for Blocks of at most 64 KiB; the arbiter for larger
    Blocks is lzma.decompress of the whole Stream."""
    global _CRC64_TAB
    if _CRC64_TAB is None:
        tab = []
        for i in range(256):
            r = i
            for _ in range(8):
                r = (r >> 1) ^ (_CRC64_POLY if r & 1 else 0)
            tab.append(r)
        _CRC64_TAB = tab
    tab = _CRC64_TAB
    crc = 0xFFFFFFFFFFFFFFFF
    for c in bytes(data):
        crc = tab[(crc ^ c) & 0xFF] ^ (crc >> 8)
    return crc ^ 0xFFFFFFFFFFFFFFFF


def check_bytes(check, block):
    """The Check field of a Block with the data `block`: none (0), CRC32 (1), CRC64 (4), SHA-256 (10)."""
    block = bytes(block)
    if check == 0:
        return b""
    if check == 1:
        return zlib.crc32(block).to_bytes(4, "little")
    if check == 4:
        return crc64(block).to_bytes(8, "little")
    if check == 10:
        return hashlib.sha256(block).digest()
    raise ValueError(f"no Check {check} here")


def stored_stream_checked(data, sizes, check):
    """An .xz Stream of stored Blocks (uncompressed LZMA2 chunks) of the lengths `sizes`, which sum to len(data), with real
    Checks.  A length of zero gives a Block whose chunk chain is the end marker alone.  (_forward.stored_stream: the same
    with one Block size and zero-filled Checks.)"""
    data = bytes(data)
    assert sum(sizes) == len(data)
    flags = bytes([0, check])
    out = bytearray(b"\xfd7zXZ\0" + flags + zlib.crc32(flags).to_bytes(4, "little"))
    pairs, at = [], 0
    for n in sizes:
        blk = data[at: at + n]
        at += n
        chain = bytearray()
        for c in range(0, n, 65536):
            piece = blk[c: c + 65536]
            chain += bytes([1 if c == 0 else 2]) + (len(piece) - 1).to_bytes(2, "big") + piece
        chain += b"\0"
        body = bytes([0xC0]) + fl.vli(len(chain)) + fl.vli(n) + b"\x21\x01\x10"
        hs = (1 + len(body) + 4 + 3) & ~3
        hdr = bytes([hs // 4 - 1]) + body + b"\0" * (hs - 5 - len(body))
        hdr += zlib.crc32(hdr).to_bytes(4, "little")
        chk = check_bytes(check, blk)
        out += hdr + chain + b"\0" * (-(hs + len(chain)) % 4) + chk
        pairs.append((hs + len(chain) + len(chk), n))
    return bytes(out) + fw.index_footer(check, pairs)


def check_fields(raw, at=0):
    """[(offset in raw, size)] of the Check fields of the Blocks of the Stream that starts at raw[at] (Block Headers with
    both sizes, as stored_stream_checked and the device encoder write them)."""
    csz = CHECK_SIZE[raw[at + 7] & 0x0F]
    out, pos = [], at + 12
    while raw[pos] != 0:
        hs = (raw[pos] + 1) * 4
        assert raw[pos + 1] & 0xC0 == 0xC0, "a Block Header without sizes"
        csize, _ = fl._vli_get(raw, pos + 2)
        pos += (hs + csize + 3) & ~3
        out.append((pos, csz))
        pos += csz
    return out


def flip(raw, offset, bit=0):
    """raw with one bit of the byte at `offset` inverted"""
    out = bytearray(raw)
    out[offset] ^= 1 << bit
    return bytes(out)


_SYS_IDS = {fl.DELTA: lzma.FILTER_DELTA, 4: lzma.FILTER_X86, 5: lzma.FILTER_POWERPC, 6: lzma.FILTER_IA64, 7: lzma.FILTER_ARM,
            8: lzma.FILTER_ARMTHUMB, 9: lzma.FILTER_SPARC}


def sys_forward(block, chain):
    """What the system's encoder-side filters make of one Block: chain = [(filter id, delta distance), ...] in Block Header
    order (as _filters.ref_forward takes it).  {chain, LZMA2} raw-encoded by the `lzma` module, then raw-decoded as {LZMA2}
    alone.  ARM64 and RISC-V, which the module refuses, go to _filters.ref_forward (needs oracle/_ref)."""
    block = bytes(block)
    if not chain:
        return block
    if any(fid not in _SYS_IDS for fid, _ in chain):
        return fl.ref_forward(block, chain)
    spec = [{"id": lzma.FILTER_DELTA, "dist": d} if fid == fl.DELTA else {"id": _SYS_IDS[fid]} for fid, d in chain]
    tail = {"id": lzma.FILTER_LZMA2, "preset": 0}
    coded = lzma.compress(block, format=lzma.FORMAT_RAW, filters=spec + [tail])
    out = lzma.decompress(coded, format=lzma.FORMAT_RAW, filters=[tail])
    assert len(out) == len(block)
    return out


def _dict_size(props):
    return 0xFFFFFFFF if props == 40 else (2 | (props & 1)) << (props // 2 + 11)


def block_payload_filtered(raw, where):
    """The bytes the filters in front of LZMA2 produced for one Block: its LZMA2 payload decoded by the `lzma` module with
    {LZMA2} alone.  `where`: the offset of the Block Header in raw, or a block info (out_offset) / file-index entry
    (header_offset) that names it.  The Block Header must carry its Compressed Size."""
    off = where if isinstance(where, int) else where["header_offset"] if isinstance(where, dict) else where.out_offset
    hs = (raw[off] + 1) * 4
    assert raw[off + 1] & 0x40, "a Block Header without Compressed Size"
    csize, _ = fl._vli_get(raw, off + 2)
    ff = fl.block_filter_flags(bytes(12) + bytes(raw[off: off + hs]))
    assert ff[-1][0] == fl.LZMA2 and len(ff[-1][1]) == 1
    d = lzma.LZMADecompressor(format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": max(_dict_size(ff[-1][1][0]), 4096)}])
    out = d.decompress(bytes(raw[off + hs: off + hs + csize]))
    assert d.eof and not d.unused_data, "the payload is not one whole LZMA2 chunk chain"
    return out


def block_chain(raw, where):
    """[(filter id, delta distance)] of the filters in front of LZMA2 in the Block Header at `where` (see above)."""
    off = where if isinstance(where, int) else where["header_offset"] if isinstance(where, dict) else where.out_offset
    ff = fl.block_filter_flags(bytes(12) + bytes(raw[off: off + (raw[off] + 1) * 4]))
    assert ff[-1][0] == fl.LZMA2
    return [(fid, props[0] + 1 if fid == fl.DELTA else 0) for fid, props in ff[:-1]]


# ---- inputs shared by the CPU conditions (test_checks_model.py) and the device tests ----
RAGGED_CASES = [(4097, 1), (65537, 15), (65636, 16), (69631, 17), (200001, 31), (4097, 33)]     # (Block size, tail bytes)
PAIR_BLOCK = 4099                       # odd, so that the seams of consecutive Blocks fall on every offset modulo 16
PAIR_DISTS = (1, 3, 24, 32)


def _rnd(n, seed):
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def ragged_input(bs, tail):
    """Six classes of bs bytes each laid end to end -- every one a Block of its own at Block size bs -- and a last Block
    of `tail` bytes.  Returns (data, Block size)."""
    import _corpora as cp
    parts = [cp.logs(bs), cp.int32_walk(bs), cp.structs24(bs), cp.pcm16_stereo(bs), _rnd(bs, 1000 + bs), cp.f64_sine(bs)]
    parts = [bytes(p)[:bs] for p in parts]
    assert all(len(p) == bs for p in parts)
    return b"".join(parts) + bytes(cp.int32_walk(64))[:tail], bs


def period_ramp(n, d, seed):
    """d interleaved byte ramps with steps of 1..3: the delta filter of distance d leaves three values, every other
    candidate distance a wider spread."""
    import numpy as np
    rng = np.random.default_rng(seed)
    rows = (n + d - 1) // d
    steps = rng.integers(1, 4, (rows, d), dtype=np.int64)
    steps[0] = rng.integers(0, 256, d)
    return (np.cumsum(steps, axis=0) & 255).astype(np.uint8).reshape(-1)[:n].tobytes()


def pair_input():
    """Blocks of PAIR_BLOCK bytes whose neighbours take (d, 0), (0, d) and (d1, d2) for the distances of PAIR_DISTS.
    Returns (data, Block size, the distance every Block is made for)."""
    want, parts = [], []
    for d in PAIR_DISTS:                                 # d, 0, d
        want += [d, 0, d]
    want += list(PAIR_DISTS) + [PAIR_DISTS[0], 0]        # ... d, 1, 3, 24, 32, 1, 0: every ordered pair of neighbours once
    for i, d in enumerate(want):
        parts.append(period_ramp(PAIR_BLOCK, d, 50 + i) if d else _rnd(PAIR_BLOCK, 70 + i))
    return b"".join(parts) + period_ramp(17, 1, 99), PAIR_BLOCK, want + [None]


SEAM_BLOCK = 3 * 2048 + 7               # three chunks of the encoder's walks (BCJ_CHUNK) and a few bytes
TILE_BLOCK = 2 * 16384 + 7              # two tiles of the decoder's walks (XZAMD_UNF_TILE) and a few bytes
_X86_ALPHABET = (0xE8, 0xE9, 0x00, 0xFF, 0x01, 0xFE, 0x7F, 0x80)


def _seams(kind):
    if kind == "encoder":               # the owners of k_x86_bcj / k_riscv_bcj change here
        return SEAM_BLOCK, (2048, 4096)
    # the owners of unf_x86 / unf_riscv change every 64 bytes; a tile (= a workgroup) ends at 16384
    return TILE_BLOCK, (16384 - 64, 16384, 16384 + 64, 2 * 16384 - 64, 2 * 16384)


def x86_seam_blocks(kind, count, seed):
    """`count` Blocks on a quiet background (bytes 0x01..0xDF: no E8, E9, 00, FF) with, at every seam of the walk of
    `kind` ("encoder": 2048 and 4096; "decoder": multiples of 64 around 16384 k), a window of 5..30 bytes from
    {E8, E9, 00, FF, 01, FE, 7F, 80} that starts 0..30 bytes in front of the seam.  Returns (data, Block size)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    bs, seams = _seams(kind)
    a = rng.integers(0x01, 0xE0, (count, bs), dtype=np.uint8)
    alphabet = np.array(_X86_ALPHABET, dtype=np.uint8)
    for b in range(count):
        for s in seams:
            start = s - int(rng.integers(0, 31))
            n = int(rng.integers(5, 31))
            n = min(n, bs - start)
            a[b, start:start + n] = alphabet[rng.integers(0, len(alphabet), n)]
    return a.tobytes(), bs


def _riscv_cluster(rng, n):
    """n bytes of back-to-back RISC-V instructions the filter looks at: JAL, AUIPC pairs, AUIPCs without a partner, the special
    form, AUIPCs with rd x0 / x2 that are not special, and two-byte gaps."""
    out = bytearray()
    r32 = lambda: int(rng.integers(0, 1 << 32))
    while len(out) < n:
        k = int(rng.integers(0, 6))
        if k == 0:
            out += bytes([0xEF, r32() & 0xF2, r32() & 0xFF, r32() & 0xFF])
        elif k in (1, 2):
            rd = int(rng.choice([1, 3, 5, 6, 10, 31]))
            inst = (r32() & ~0xFFF) | (rd << 7) | 0x17
            inst2 = r32() if k == 2 else (r32() & ~(0x1F << 15) & ~3) | (rd << 15) | 3
            out += inst.to_bytes(4, "little") + (inst2 & 0xFFFFFFFF).to_bytes(4, "little")
        elif k == 3:
            inst = (r32() & ~0x3FFF) | 0x3117
            if rng.random() < 0.2:
                inst &= 0x07FFFFFF                        # "rs1" x0: not the special form
            out += inst.to_bytes(4, "little") + r32().to_bytes(4, "little")
        elif k == 4:
            out += ((r32() & ~0xFFF) | (int(rng.choice([0, 2])) << 7) | 0x17).to_bytes(4, "little")
        else:
            out += bytes([0x13, 0x05])
    return bytes(out[:n])


def riscv_seam_blocks(kind, count, seed):
    """The same for RISC-V: a background without JAL (EF) and AUIPC (17, 97) opcode bytes, and around every seam a cluster of
    8..40 bytes of instructions the filter converts or steps over, mostly at an even offset."""
    import numpy as np
    rng = np.random.default_rng(seed)
    bs, seams = _seams(kind)
    quiet = np.array([v for v in range(256) if v != 0xEF and (v & 0x7F) != 0x17], dtype=np.uint8)
    a = quiet[rng.integers(0, len(quiet), (count, bs))]
    for b in range(count):
        for s in seams:
            start = s - 2 * int(rng.integers(0, 16)) - int(rng.random() < 0.15)
            n = min(int(rng.integers(8, 41)), bs - start)
            a[b, start:start + n] = np.frombuffer(_riscv_cluster(rng, n), dtype=np.uint8)
    return a.tobytes(), bs


# Block lengths of the crafted Streams of the Check tests: uniform groups (one launch), ragged ones (a launch per Block), empty
# Blocks, the padding edges of SHA-256 and the lane edges of the CRC fold (64, 65 and 66 strips of 4096 bytes)
SIZE_LISTS = {
    "uniform_4096": [4096] * 3 + [1],
    "uniform_64": [64] * 70 + [56],
    "ragged": [4095, 4097, 8192, 0, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 17],
    "empty": [0],
    "empty_twice": [0, 0],
    "empty_last": [100, 100, 0],
    "empty_first": [0, 0, 5],
    "sha_edges": [55, 56, 63, 64, 65, 119, 120, 0, 128],
}
_STREAMS = {}


def crafted(name, check):
    """(data, Stream) of SIZE_LISTS[name] with the Check `check`; made once."""
    if (name, check) not in _STREAMS:
        sizes = SIZE_LISTS[name]
        data = _rnd(sum(sizes), 4000 + len(sizes))
        _STREAMS[name, check] = (data, stored_stream_checked(data, sizes, check))
    return _STREAMS[name, check]


def flip_subset(sizes):
    """Blocks whose Check the tests damage: the first, the last, one in the middle and every empty one."""
    n = len(sizes)
    return sorted({0, n - 1, n // 2} | {i for i, s in enumerate(sizes) if s == 0})
