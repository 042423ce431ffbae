"""An independent walker over the chunks of an LZMA2 payload (test infrastructure only).

Written from the file-format description; it imports nothing from oracle/ and nothing from the library, so it can judge both.
``walk(payload, block_usize)`` lists the chunks and gives two verdicts that are kept apart on purpose:

(a) ``decoder_error``: what an LZMA2 decoder enforces before it looks at a single range-coded bit -- the first chunk resets
    the dictionary (control 0x01 or >= 0xE0), controls 0x03..0x7F do not exist, an LZMA chunk needs properties since the last
    dictionary reset (a control >= 0xC0 brings them, and its properties byte must be a legal lc/lp/pb), every chunk lies
    inside the payload, and the payload ends with the 0x00 marker and nothing behind it.
(b) ``convention_error``: what the reference encoder and this project's encoder promise on top of that -- an LZMA chunk
    behind a stored chunk resets the coder state (control >= 0xA0), an LZMA chunk holds at most 2 MiB and takes at most
    64 KiB, a stored chunk holds at most 64 KiB, and the uncompressed sizes add up to the Block's size.

``is_stored_prefix_defect`` names the one shape of an invalid Block this project is known to write: the
Block's first LZMA chunk has control 0xA0 -- a state reset without properties -- and everything in front of it is stored.
``blocks_of(stream)`` cuts the Blocks of a one-Stream .xz file out by its Index.
"""
import collections
import zlib

STORED, LZMA = "stored", "lzma"

Chunk = collections.namedtuple("Chunk", "control kind usize csize offset")
# control: the control byte; kind: STORED / LZMA; usize: uncompressed bytes; csize: bytes of data behind the chunk header;
# offset: of the control byte in the payload

LZMA_CHUNK_USIZE_MAX = 1 << 21
LZMA_CHUNK_CSIZE_MAX = 1 << 16
STORED_CHUNK_MAX = 1 << 16


def control_class(ctl):
    """0x01 / 0x02 for stored chunks; 0x80, 0xA0, 0xC0, 0xE0 for LZMA chunks (their low five bits are size bits)"""
    return ctl & 0xE0 if ctl >= 0x80 else ctl


class Walk:
    """chunks: every chunk up to the one at which rule (a) failed (that one included, where its header could be read);
    decoder_error / convention_error: None or (index of the chunk, text)."""

    def __init__(self, chunks, decoder_error, convention_error):
        self.chunks, self.decoder_error, self.convention_error = chunks, decoder_error, convention_error

    @property
    def decoder_ok(self):
        return self.decoder_error is None

    @property
    def ok(self):
        return self.decoder_error is None and self.convention_error is None

    def __repr__(self):
        ctl = " ".join(f"{c.control:02X}" for c in self.chunks[:24]) + (" ..." if len(self.chunks) > 24 else "")
        return f"Walk({len(self.chunks)} chunks [{ctl}], decoder_error={self.decoder_error}, convention_error={self.convention_error})"


def _props_ok(byte):
    if byte > (4 * 5 + 4) * 9 + 8:
        return False
    lc, lp = byte % 9, byte // 9 % 5
    return lc + lp <= 4


def walk(payload, block_usize=None):
    """Walk the chunks of one LZMA2 payload (end marker included).  block_usize: the Block's uncompressed size for the
    sum rule of (b); None leaves that rule out."""
    payload = bytes(payload)
    n = len(payload)
    chunks = []
    conv = None
    p = 0
    need_dict_reset = True
    need_props = True
    behind_stored = False
    total = 0

    def result(err):
        c = conv
        if err is None and c is None and block_usize is not None and total != block_usize:
            c = (len(chunks), f"uncompressed sizes add up to {total}, the Block holds {block_usize}")
        return Walk(chunks, err, c)

    while True:
        k = len(chunks)
        if p >= n:
            return result((k, "payload ends without the end marker"))
        ctl = payload[p]
        if ctl == 0x00:
            if p + 1 != n:
                return result((k, f"{n - p - 1} bytes behind the end marker"))
            return result(None)
        if ctl >= 0xE0 or ctl == 0x01:
            need_props = True
            need_dict_reset = False
        elif need_dict_reset:
            chunks.append(Chunk(ctl, LZMA if ctl >= 0x80 else STORED, 0, 0, p))
            return result((k, f"first chunk {ctl:#04x} does not reset the dictionary"))
        if ctl >= 0x80:
            hdr = 6 if ctl >= 0xC0 else 5
            if p + hdr > n:
                return result((k, "chunk header runs past the payload"))
            usize = ((ctl & 0x1F) << 16) + (payload[p + 1] << 8) + payload[p + 2] + 1
            csize = (payload[p + 3] << 8) + payload[p + 4] + 1
            chunks.append(Chunk(ctl, LZMA, usize, csize, p))
            if ctl >= 0xC0:
                if not _props_ok(payload[p + 5]):
                    return result((k, f"properties byte {payload[p + 5]:#04x}"))
                need_props = False
            elif need_props:
                return result((k, f"LZMA chunk {ctl:#04x} in front of any properties"))
            if conv is None and behind_stored and ctl < 0xA0:
                conv = (k, f"LZMA chunk {ctl:#04x} behind a stored chunk carries no state reset")
            if conv is None and (usize > LZMA_CHUNK_USIZE_MAX or csize > LZMA_CHUNK_CSIZE_MAX):
                conv = (k, f"LZMA chunk of {usize} -> {csize} bytes")
            behind_stored = False
        elif ctl > 0x02:
            chunks.append(Chunk(ctl, STORED, 0, 0, p))
            return result((k, f"control {ctl:#04x} does not exist"))
        else:
            hdr = 3
            if p + hdr > n:
                return result((k, "chunk header runs past the payload"))
            usize = csize = (payload[p + 1] << 8) + payload[p + 2] + 1
            chunks.append(Chunk(ctl, STORED, usize, csize, p))
            if conv is None and usize > STORED_CHUNK_MAX:
                conv = (k, f"stored chunk of {usize} bytes")
            behind_stored = True
        if p + hdr + csize > n:
            return result((k, "chunk data runs past the payload"))
        total += usize
        p += hdr + csize


def is_stored_prefix_defect(w):
    """w: a Walk (or its chunk list with the failing chunk last).  True when rule (a) fails at the Block's first LZMA chunk,
    that chunk is of class 0xA0, and every chunk in front of it is stored."""
    if isinstance(w, Walk):
        if w.decoder_error is None:
            return False
        k, chunks = w.decoder_error[0], w.chunks
    else:
        chunks = list(w)
        k = len(chunks) - 1
    if k < 1 or k >= len(chunks):
        return False
    return control_class(chunks[k].control) == 0xA0 and all(c.kind == STORED for c in chunks[:k])


# ---------------------------------------------------------------- .xz framing
Block = collections.namedtuple("Block", "offset header_size unpadded_size uncompressed_size payload")


def _vli(buf, p):
    v = shift = 0
    while True:
        b = buf[p]
        p += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            return v, p
        shift += 7
        assert shift < 63, "overlong variable-length integer"


_CHECK_BYTES = {0: 0, 1: 4, 4: 8, 10: 32}


def blocks_of(stream):
    """The Blocks of a .xz file that holds one Stream, by its Index: [Block(offset, header_size, unpadded_size,
    uncompressed_size, payload)] with payload = the LZMA2 data between Block Header and Check (the last filter of every
    Block must be LZMA2, which is all this project writes)."""
    s = bytes(stream)
    assert s[:6] == b"\xFD7zXZ\0" and s[-2:] == b"YZ", "not one whole .xz Stream"
    assert zlib.crc32(s[6:8]) == int.from_bytes(s[8:12], "little") and s[-4:-2] == s[6:8]
    assert zlib.crc32(s[-8:-2]) == int.from_bytes(s[-12:-8], "little")
    check = _CHECK_BYTES[s[7] & 0x0F]
    isize = (int.from_bytes(s[-8:-4], "little") + 1) * 4
    ip = len(s) - 12 - isize
    index = s[ip: ip + isize]
    assert index[0] == 0 and zlib.crc32(index[:-4]) == int.from_bytes(index[-4:], "little")
    count, p = _vli(index, 1)
    out = []
    off = 12
    for _ in range(count):
        unpadded, p = _vli(index, p)
        usize, p = _vli(index, p)
        hs = (s[off] + 1) * 4
        assert s[off] != 0 and zlib.crc32(s[off: off + hs - 4]) == int.from_bytes(s[off + hs - 4: off + hs], "little")
        out.append(Block(off, hs, unpadded, usize, s[off + hs: off + unpadded - check]))
        off += (unpadded + 3) & ~3
    assert off == ip, "the Index does not cover the Blocks"
    return out


def walk_stream(stream):
    """[Walk] of every Block of a one-Stream .xz file"""
    return [walk(b.payload, b.uncompressed_size) for b in blocks_of(stream)]


OK, DEFECT, INVALID = "ok", "stored-prefix", "invalid"


def verdict(w):
    """OK: rules (a) and (b) hold; DEFECT: the known stored-prefix shape; INVALID: anything else"""
    return OK if w.ok else DEFECT if is_stored_prefix_defect(w) else INVALID


def verdicts(stream):
    """[verdict] of every Block of a one-Stream .xz file"""
    return [verdict(w) for w in walk_stream(stream)]
