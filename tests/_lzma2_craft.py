"""Symbol-level LZMA2 writer, a small .xz framer, and the list of crafted decoder cases (test infrastructure only).

Written from the file-format description: an LZMA model for any (lc, lp, pb), a range encoder, the four symbol kinds
``("L", byte)``, ``("M", dist, len)``, ``("R", rep_index, len)``, ``("S",)`` and the LZMA2 chunk headers.  The writer keeps
the decoder's view of the data since the last dictionary reset, so position states, literal contexts and match bytes come
out as the decoder will compute them -- also for symbols that are illegal on purpose.  Every header field of a chunk can
be overridden after it was coded, so a case can be wrong in exactly one place.

``cases()`` builds the whole deterministic case list (sections A to G of tests/test_lzma2_craft.py); every case has a
name, a seed and an intended verdict.  The truth is never the intent: tests/golden/lzma2_craft.json records what the real
liblzma says about the very bytes of every case (tests/golden/make_craft_golden.py).
"""
import functools
import hashlib
import random
import struct
import zlib

CHECK_NONE, CHECK_CRC32, CHECK_SHA256 = 0, 1, 10
_CHECK_BYTES = {CHECK_NONE: 0, CHECK_CRC32: 4, CHECK_SHA256: 32}
DEFAULT_PROPS = (3, 0, 2)
MIB = 1 << 20


# ---------------------------------------------------------------- range encoder
class RangeEncoder:
    def __init__(self):
        self.low = 0
        self.range = 0xFFFFFFFF
        self.cache = 0
        self.cache_size = 1
        self.out = bytearray()

    def shift_low(self):
        low = self.low
        if low < 0xFF000000 or low >= 0x100000000:
            carry = low >> 32
            out = self.out
            out.append((self.cache + carry) & 0xFF)
            if self.cache_size > 1:
                out.extend(bytes([(0xFF + carry) & 0xFF]) * (self.cache_size - 1))
            self.cache_size = 0
            self.cache = (low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (low & 0x00FFFFFF) << 8

    def bit(self, probs, i, b):
        p = probs[i]
        bound = (self.range >> 11) * p
        if b:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)
        else:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        while self.range < 0x1000000:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.shift_low()

    def direct(self, value, nbits):
        for i in range(nbits - 1, -1, -1):
            self.range >>= 1
            if (value >> i) & 1:
                self.low += self.range
            while self.range < 0x1000000:
                self.range = (self.range << 8) & 0xFFFFFFFF
                self.shift_low()

    def tree(self, probs, base, nbits, value):
        m = 1
        for i in range(nbits - 1, -1, -1):
            b = (value >> i) & 1
            self.bit(probs, base + m, b)
            m = (m << 1) | b

    def tree_rev(self, probs, base, nbits, value):
        m = 1
        for i in range(nbits):
            b = (value >> i) & 1
            self.bit(probs, base + m, b)
            m = (m << 1) | b

    def pending_size(self):
        """size of the payload if it were flushed now"""
        return len(self.out) + self.cache_size + 4

    def finish(self):
        for _ in range(5):
            self.shift_low()
        return bytes(self.out)


# ---------------------------------------------------------------- LZMA model
class _LenCoder:
    def __init__(self):
        self.choice = [1024, 1024]
        self.low = [1024] * (16 * 8)
        self.mid = [1024] * (16 * 8)
        self.high = [1024] * 256

    def encode(self, rc, length, ps):
        v = length - 2
        if v < 8:
            rc.bit(self.choice, 0, 0)
            rc.tree(self.low, ps * 8, 3, v)
        elif v < 16:
            rc.bit(self.choice, 0, 1)
            rc.bit(self.choice, 1, 0)
            rc.tree(self.mid, ps * 8, 3, v - 8)
        else:
            rc.bit(self.choice, 0, 1)
            rc.bit(self.choice, 1, 1)
            rc.tree(self.high, 0, 8, v - 16)


class Model:
    def __init__(self, lc, lp, pb):
        self.lc, self.lp, self.pb = lc, lp, pb
        self.reset()

    def reset(self):
        self.literal = [1024] * (0x300 << (self.lc + self.lp))
        self.is_match = [1024] * (12 * 16)
        self.is_rep = [1024] * 12
        self.is_rep0 = [1024] * 12
        self.is_rep1 = [1024] * 12
        self.is_rep2 = [1024] * 12
        self.is_rep0_long = [1024] * (12 * 16)
        self.dist_slot = [1024] * (4 * 64)
        self.dist_special = [1024] * 115
        self.dist_align = [1024] * 16
        self.match_len = _LenCoder()
        self.rep_len = _LenCoder()
        self.state = 0
        self.reps = [0, 0, 0, 0]


def dist_slot_of(dist):
    if dist < 4:
        return dist
    n = dist.bit_length() - 1
    return 2 * n + ((dist >> (n - 1)) & 1)


def slot_base(slot):
    if slot < 4:
        return slot
    return (2 | (slot & 1)) << ((slot >> 1) - 1)


def props_byte(lc, lp, pb):
    return (pb * 5 + lp) * 9 + lc


# ---------------------------------------------------------------- chunks
class Chunk:
    """One LZMA2 chunk.  `usize` / `csize` are the DECLARED sizes; every field may be changed after the chunk was coded."""

    def __init__(self, control, usize, body, csize=None, props=None):
        self.control = control        # 0x01 / 0x02 / 0x80 / 0xA0 / 0xC0 / 0xE0 (high bits of the size are added on output)
        self.usize = usize
        self.csize = csize            # None: an uncompressed chunk
        self.props = props            # properties byte (control >= 0xC0)
        self.body = bytearray(body)
        self.control_byte = None      # overrides the whole first byte
        self.tail = b""               # bytes behind the chunk's payload

    def to_bytes(self):
        if self.csize is None:
            first = self.control if self.control_byte is None else self.control_byte
            head = bytes([first]) + struct.pack(">H", (self.usize - 1) & 0xFFFF)
        else:
            first = (self.control | (((self.usize - 1) >> 16) & 0x1F)) if self.control_byte is None else self.control_byte
            head = bytes([first]) + struct.pack(">HH", (self.usize - 1) & 0xFFFF, (self.csize - 1) & 0xFFFF)
            if self.props is not None:
                head += bytes([self.props])
        return head + bytes(self.body) + bytes(self.tail)


class EndMarker:
    tail = b""

    def to_bytes(self):
        return b"\x00" + bytes(self.tail)


class Writer:
    """The LZMA2 data of one Block, chunk by chunk."""

    def __init__(self):
        self.chunks = []
        self.plain = bytearray()      # what a decoder that accepts everything would have written
        self.hist = bytearray()       # ... since the last dictionary reset
        self.prefix = bytearray()     # ... before it: what a decoder without a dictionary-reset test would still reach
        self.model = Model(*DEFAULT_PROPS)
        self.rc = None

    def _dict_reset(self):
        self.prefix += self.hist
        self.hist = bytearray()

    def _behind(self, back):
        """the byte `back` positions in front of the next one for a decoder that tests no distance: across the last
        dictionary reset it reads the Block's earlier data, in front of the Block zero"""
        k = len(self.hist) - back
        if k >= 0:
            return self.hist[k]
        k += len(self.prefix)
        return self.prefix[k] if k >= 0 else 0

    # -- symbols
    def _sym(self, s):
        m, rc, hist = self.model, self.rc, self.hist
        pos = len(hist)
        ps = pos & ((1 << m.pb) - 1)
        st = m.state
        kind = s[0]
        if kind == "L":
            byte = s[1]
            rc.bit(m.is_match, st * 16 + ps, 0)
            prev = hist[-1] if pos else 0
            base = 0x300 * (((pos & ((1 << m.lp) - 1)) << m.lc) + (prev >> (8 - m.lc)))
            lit = m.literal
            sym = 1
            if st < 7:
                for i in range(7, -1, -1):
                    b = (byte >> i) & 1
                    rc.bit(lit, base + sym, b)
                    sym = (sym << 1) | b
            else:
                r0 = m.reps[0]
                mb = self._behind(r0 + 1)
                off = 0x100
                for i in range(7, -1, -1):
                    mb <<= 1
                    mbit = mb & off
                    b = (byte >> i) & 1
                    rc.bit(lit, base + off + mbit + sym, b)
                    sym = (sym << 1) | b
                    off &= mbit if b else ~mbit
            hist.append(byte)
            m.state = 0 if st <= 3 else (st - 3 if st <= 9 else st - 6)
            return
        rc.bit(m.is_match, st * 16 + ps, 1)
        reps = m.reps
        if kind == "M":
            dist, length = s[1], s[2]
            rc.bit(m.is_rep, st, 0)
            m.match_len.encode(rc, length, ps)
            slot = dist_slot_of(dist)
            rc.tree(m.dist_slot, min(length - 2, 3) * 64, 6, slot)
            if slot >= 4:
                fb = (slot >> 1) - 1
                base = (2 | (slot & 1)) << fb
                rem = dist - base
                if slot < 14:
                    rc.tree_rev(m.dist_special, base - slot - 1, fb, rem)
                else:
                    rc.direct(rem >> 4, fb - 4)
                    rc.tree_rev(m.dist_align, 0, 4, rem & 15)
            m.reps = [dist, reps[0], reps[1], reps[2]]
            m.state = 7 if st < 7 else 10
        elif kind == "S":
            rc.bit(m.is_rep, st, 1)
            rc.bit(m.is_rep0, st, 0)
            rc.bit(m.is_rep0_long, st * 16 + ps, 0)
            m.state = 9 if st < 7 else 11
            length = 1
        else:
            idx, length = s[1], s[2]
            rc.bit(m.is_rep, st, 1)
            if idx == 0:
                rc.bit(m.is_rep0, st, 0)
                rc.bit(m.is_rep0_long, st * 16 + ps, 1)
            else:
                rc.bit(m.is_rep0, st, 1)
                if idx == 1:
                    rc.bit(m.is_rep1, st, 0)
                else:
                    rc.bit(m.is_rep1, st, 1)
                    rc.bit(m.is_rep2, st, idx - 2)
                d = reps.pop(idx)
                reps.insert(0, d)
            m.rep_len.encode(rc, length, ps)
            m.state = 8 if st < 7 else 11
        # the copy, as a decoder without a distance test would do it
        d = m.reps[0] + 1
        if d > pos:
            for _ in range(length):
                hist.append(self._behind(d))
        elif d >= length:
            hist.extend(hist[pos - d: pos - d + length])
        else:
            pat = bytes(hist[pos - d:])
            hist.extend((pat * (length // d + 1))[:length])

    # -- chunks
    def lz_chunk(self, symbols, control, props=None, stop=None):
        """Code `symbols` (any iterable; it may look at the writer while it is consumed) as one LZMA chunk.  `props`:
        (lc, lp, pb), needed for 0xC0 / 0xE0 unless the model in use is to stay.  `stop(writer)`: end the chunk early."""
        if control >= 0xE0:
            self._dict_reset()
        if control >= 0xC0:
            if props is not None:
                self.model = Model(*props)
            else:
                self.model.reset()
        elif control >= 0xA0:
            self.model.reset()
        m = self.model
        self.rc = RangeEncoder()
        u0 = len(self.hist)
        for s in symbols:
            self._sym(s)
            if stop is not None and stop(self):
                break
        body = self.rc.finish()
        usize = len(self.hist) - u0
        self.plain += self.hist[u0:]
        ch = Chunk(control, usize, body, csize=len(body), props=props_byte(m.lc, m.lp, m.pb) if control >= 0xC0 else None)
        self.chunks.append(ch)
        return ch

    def raw_chunk(self, data, control):
        if control == 0x01:
            self._dict_reset()
        self.hist += data
        self.plain += data
        ch = Chunk(control, len(data), data)
        self.chunks.append(ch)
        return ch

    def end(self):
        e = EndMarker()
        self.chunks.append(e)
        return e

    def payload(self):
        return b"".join(c.to_bytes() for c in self.chunks)

    def declared_usize(self):
        return sum(c.usize for c in self.chunks if isinstance(c, Chunk))


# ---------------------------------------------------------------- .xz framing
def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def dict_byte(dict_size):
    for b in range(40):
        if (2 | (b & 1)) << (b // 2 + 11) == dict_size:
            return b
    raise ValueError("no LZMA2 dictionary size: %d" % dict_size)


def _check_of(check, plain):
    if check == CHECK_CRC32:
        return struct.pack("<I", zlib.crc32(plain) & 0xFFFFFFFF)
    if check == CHECK_SHA256:
        return hashlib.sha256(plain).digest()
    return b""


class Block:
    """What the framer needs of one Block: its LZMA2 data (end marker included where there is one), the declared sizes."""

    def __init__(self, payload, usize, dict_size, plain=b"", header_sizes=True):
        self.payload, self.usize, self.dict_size, self.plain, self.header_sizes = payload, usize, dict_size, plain, header_sizes


class Row:
    """A row of the bare-chain table (the fields of xzamd_block_info)."""

    def __init__(self, unpadded_size, uncompressed_size, out_offset, total_size):
        self.unpadded_size, self.uncompressed_size = unpadded_size, uncompressed_size
        self.out_offset, self.total_size = out_offset, total_size


def frame(blocks, check=CHECK_NONE):
    """One .xz Stream of `blocks`.  Returns (stream bytes, [(offset of the LZMA2 data, its length)] per Block)."""
    flags = bytes([0, check])
    out = bytearray(b"\xFD7zXZ\x00" + flags + struct.pack("<I", zlib.crc32(flags) & 0xFFFFFFFF))
    records, where = [], []
    for b in blocks:
        body = bytearray([0, 0xC0 if b.header_sizes else 0x00])
        if b.header_sizes:
            body += vli(len(b.payload)) + vli(b.usize)
        body += bytes([0x21, 0x01, dict_byte(b.dict_size)])
        while (len(body) + 4) % 4:
            body.append(0)
        body[0] = (len(body) + 4) // 4 - 1
        out += body + struct.pack("<I", zlib.crc32(bytes(body)) & 0xFFFFFFFF)
        where.append((len(out), len(b.payload)))
        out += b.payload
        out += b"\0" * (-len(b.payload) % 4)
        out += _check_of(check, b.plain)
        records.append((len(body) + 4 + len(b.payload) + _CHECK_BYTES[check], b.usize))
    index = bytearray(b"\x00" + vli(len(records)))
    for unpadded, usize in records:
        index += vli(unpadded) + vli(usize)
    index += b"\0" * (-len(index) % 4)
    index += struct.pack("<I", zlib.crc32(bytes(index)) & 0xFFFFFFFF)
    out += index
    tail = struct.pack("<I", len(index) // 4 - 1) + flags
    out += struct.pack("<I", zlib.crc32(tail) & 0xFFFFFFFF) + tail + b"YZ"
    return bytes(out), where


def bare_chains(chains, usizes):
    """(buffer, rows) of bare chunk chains laid end to end (Check none: the CRC field of a row is 0)."""
    buf, rows = bytearray(), []
    for ch, us in zip(chains, usizes):
        rows.append(Row(0, us, len(buf), len(ch)))
        buf += ch
    return bytes(buf), rows


# ---------------------------------------------------------------- cases
class Case:
    """One crafted Block.  intent: "accept" (`plain` is the intended plaintext) or "reject" (then `step` is the
    verification step that must name it: "grammar" or "decode").  `record_only`: the verdict is whatever the reference says.
    `chain` / `chain_intent`: the same data as a bare chunk chain (no end marker) and its intended verdict."""

    def __init__(self, name, section, seed, payload, usize, intent, plain=None, step=None, dict_size=8 * MIB,
                 header_sizes=True, record_only=False, chain=None, chain_intent=None, big=False):
        self.name, self.section, self.seed = name, section, seed
        self.payload, self.usize, self.intent, self.plain, self.step = payload, usize, intent, plain, step
        self.dict_size, self.header_sizes, self.record_only, self.big = dict_size, header_sizes, record_only, big
        if chain is None:
            chain = payload[:-1] if payload.endswith(b"\x00") else payload
        self.chain = chain
        self.chain_intent = chain_intent if chain_intent is not None else intent

    def block(self, plain=None):
        return Block(self.payload, self.usize, self.dict_size, self.plain if plain is None else plain, self.header_sizes)

    def stream(self):
        """the case alone, as a one-Block Stream with Check none: what the reference judges"""
        return frame([self.block(b"")], CHECK_NONE)[0]


LENS = (2, 3, 9, 10, 17, 18, 273)


def literals(rng, n):
    return [("L", rng.randrange(256)) for _ in range(n)]


def random_symbols(w, rng, n, long_share=0.04, max_len=273):
    """n seeded legal symbols of all four kinds (the first ones literals when there is no history yet)"""
    for _ in range(n):
        have = len(w.hist)
        k = rng.random()
        if have < 4 or k < 0.32:
            yield ("L", rng.randrange(256) if rng.random() < 0.7 else (w.hist[-1] if have else 0))
            continue
        length = 273 if rng.random() < long_share else rng.choice(LENS[:-1]) if rng.random() < 0.8 else rng.randrange(2, 274)
        length = min(length, max_len)
        if k < 0.62:
            far = rng.random() < 0.5
            yield ("M", rng.randrange(have) if far else rng.randrange(min(have, 16)), length)
        elif k < 0.84:
            idx = rng.randrange(4)
            yield ("R", idx, length) if w.model.reps[idx] < have else ("L", rng.randrange(256))
        else:
            yield ("S",) if w.model.reps[0] < have else ("L", rng.randrange(256))


def fill_to(w, rng, total):
    """cheap symbols (a few literals, then long matches) until the chunk being coded has `total` bytes"""
    start = len(w.hist)
    n = 0
    while True:
        left = total - (len(w.hist) - start)
        if left <= 0:
            return
        if n < 12 or left == 1 or len(w.hist) < 2:
            yield ("L", rng.randrange(256))
        elif rng.random() < 0.5:
            yield ("M", rng.randrange(min(len(w.hist), 4096)), min(left, 273))
        else:
            yield ("R", 0, min(left, 273)) if w.model.reps[0] < len(w.hist) else ("L", rng.randrange(256))
        n += 1


class _Maker:
    def __init__(self):
        self.cases = []
        self.names = set()

    def add(self, name, section, seed, w, intent, step=None, usize=None, payload=None, **kw):
        assert name not in self.names, name
        self.names.add(name)
        payload = w.payload() if payload is None else payload
        usize = w.declared_usize() if usize is None else usize
        plain = bytes(w.plain)          # (of a rejected case: what a decoder without any test would have written)
        if intent == "accept":
            assert len(plain) == usize, (name, len(plain), usize)
        self.cases.append(Case(name, section, seed, payload, usize, intent, plain, step, **kw))


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _new(name):
    return Writer(), random.Random(_seed(name)), _seed(name)


def _section_a(mk):
    for pb in range(5):
        for lp in range(5):
            for lc in range(5 - lp):
                name = "A-geom-lc%d-lp%d-pb%d" % (lc, lp, pb)
                w, rng, seed = _new(name)
                w.lz_chunk(random_symbols(w, rng, 200), 0xE0, (lc, lp, pb))
                w.lz_chunk(random_symbols(w, rng, 100), 0x80)
                w.end()
                mk.add(name, "A", seed, w, "accept")
    name = "A-props-change-mid-block"
    w, rng, seed = _new(name)
    w.lz_chunk(random_symbols(w, rng, 150), 0xE0, (0, 0, 0))
    w.lz_chunk(random_symbols(w, rng, 150), 0xC0, (4, 0, 2))          # a larger literal table ...
    w.lz_chunk(random_symbols(w, rng, 150), 0xC0, (1, 0, 4))          # ... and back to a smaller one
    w.lz_chunk(random_symbols(w, rng, 100), 0xC0, (0, 4, 0))
    w.lz_chunk(random_symbols(w, rng, 100), 0xC0, (2, 1, 1))
    w.end()
    mk.add(name, "A", seed, w, "accept")
    for how in ("E0", "01-C0"):
        name = "A-dict-reset-odd-offset-" + how
        w, rng, seed = _new(name)
        w.lz_chunk(fill_to(w, rng, 1001), 0xE0, (0, 4, 4))
        if how == "E0":
            w.lz_chunk(random_symbols(w, rng, 200), 0xE0, (0, 4, 4))
        else:
            w.raw_chunk(bytes(rng.randrange(256) for _ in range(13)), 0x01)
            w.lz_chunk(random_symbols(w, rng, 200), 0xC0, (0, 4, 4))
        w.lz_chunk(random_symbols(w, rng, 60), 0x80)
        w.end()
        mk.add(name, "A", seed, w, "accept")
        # Position states and literal positions that count from the Block start only permute contexts that were all reset
        # together, so no stream tells such a decoder apart.  What does restart observably is the byte in front of the first
        # literal: zero, whatever stood in front of the reset.  The first literal trains the context of a zero byte; the
        # literals behind it (all below 0x10, lc = 4) use that context again.
        name = "A-dict-reset-first-literal-context-" + how
        w, rng, seed = _new(name)
        w.lz_chunk(literals(rng, 40) + [("L", 0xFF)], 0xE0, (4, 0, 0))
        lits = [("L", rng.randrange(16)) for _ in range(60)]
        if how == "E0":
            w.lz_chunk(lits, 0xE0, (4, 0, 0))
        else:
            w.raw_chunk(b"\xFF", 0x01)
            w.lz_chunk(lits, 0xC0, (4, 0, 0))
            w.raw_chunk(b"\xFE\xFF", 0x01)
            w.lz_chunk(lits, 0xE0, (4, 0, 0))
        w.end()
        mk.add(name, "A", seed, w, "accept")


def _any_chunk(w, rng, control, n=24):
    if control < 0x80:
        return w.raw_chunk(bytes(rng.randrange(256) for _ in range(rng.randrange(1, 90))), control)
    return w.lz_chunk(random_symbols(w, rng, n, max_len=40), control, (rng.randrange(4), 0, rng.randrange(5)) if control >= 0xC0 else None)


def _section_b(mk):
    ctl = (0x01, 0x02, 0x80, 0xA0, 0xC0, 0xE0)
    for a in ctl:
        for b in ctl:
            if a == 0x01 and b in (0x80, 0xA0):
                continue
            name = "B-pair-%02X-%02X" % (a, b)
            w, rng, seed = _new(name)
            _any_chunk(w, rng, 0xE0)
            _any_chunk(w, rng, a)
            _any_chunk(w, rng, b)
            w.end()
            mk.add(name, "B", seed, w, "accept")
    # 0x80 directly behind 0x02, the coder in a match state
    for what, rep0 in (("literal-matchbyte-in-raw", 2), ("literal-matchbyte-before-raw", 30), ("rep-match", 5)):
        name = "B-80-behind-02-" + what
        w, rng, seed = _new(name)
        w.lz_chunk(literals(rng, 48) + [("M", rep0, 7)], 0xE0, (3, 0, 2))
        assert w.model.state >= 7
        w.raw_chunk(bytes(rng.randrange(256) for _ in range(9)), 0x02)
        first = [("R", 0, 12)] if what == "rep-match" else [("L", rng.randrange(256))]
        w.lz_chunk(first + list(literals(rng, 3)) + [("M", 40, 9), ("L", 7), ("S",)], 0x80)
        w.end()
        mk.add(name, "B", seed, w, "accept")
    # illegal chains
    for c in (0x02, 0x80, 0xA0, 0xC0):
        name = "B-bad-first-chunk-%02X" % c
        w, rng, seed = _new(name)
        if c == 0x02:
            w.raw_chunk(bytes(rng.randrange(256) for _ in range(40)), c)
        else:
            w.lz_chunk(literals(rng, 30), c, DEFAULT_PROPS if c == 0xC0 else None)
        w.end()
        mk.add(name, "B", seed, w, "reject", "grammar")
    for c in (0x80, 0xA0):
        name = "B-bad-01-then-%02X" % c
        w, rng, seed = _new(name)
        w.lz_chunk(literals(rng, 30), 0xE0, DEFAULT_PROPS)
        w.raw_chunk(bytes(rng.randrange(256) for _ in range(20)), 0x01)
        w.lz_chunk(literals(rng, 20), c)
        w.end()
        mk.add(name, "B", seed, w, "reject", "grammar")
    for c in (0x03, 0x40, 0x7F):
        name = "B-bad-control-%02X" % c
        w, rng, seed = _new(name)
        w.lz_chunk(literals(rng, 30), 0xE0, DEFAULT_PROPS)
        w.raw_chunk(bytes(rng.randrange(256) for _ in range(20)), 0x02).control_byte = c
        w.end()
        mk.add(name, "B", seed, w, "reject", "grammar")
    for geom in (None, (4, 1, 0), (8, 0, 0), (2, 3, 4)):
        # a byte above 224 names no geometry; the others are coded under the geometry their byte names, so that a decoder
        # which took the byte would go on to decode the chunk without a flaw
        pbyte = 225 if geom is None else props_byte(*geom)
        name = "B-bad-props-%d" % pbyte
        w, rng, seed = _new(name)
        w.lz_chunk(literals(rng, 30), 0xE0, DEFAULT_PROPS)
        w.lz_chunk(random_symbols(w, rng, 40, max_len=20), 0xC0, geom or DEFAULT_PROPS).props = pbyte
        w.end()
        mk.add(name, "B", seed, w, "reject", "grammar")

    def small(name):
        w, rng, seed = _new(name)
        w.lz_chunk(random_symbols(w, rng, 40, max_len=30), 0xE0, DEFAULT_PROPS)
        w.raw_chunk(bytes(rng.randrange(256) for _ in range(20)), 0x02)
        return w, rng, seed

    name = "B-bad-no-end-marker"
    w, rng, seed = small(name)
    mk.add(name, "B", seed, w, "reject", "grammar", chain=w.payload(), chain_intent="accept")
    name = "B-bad-data-behind-end-marker"
    w, rng, seed = small(name)
    w.end().tail = b"\x5A"
    mk.add(name, "B", seed, w, "reject", "grammar", chain=w.payload())
    name = "B-bad-block-csize-plus-1"
    w, rng, seed = small(name)
    w.end().tail = b"\x00"
    mk.add(name, "B", seed, w, "reject", "grammar", chain=w.payload()[:-1])
    name = "B-bad-block-csize-minus-1"
    w, rng, seed = small(name)
    w.end()
    mk.add(name, "B", seed, w, "reject", "grammar", payload=w.payload()[:-1], chain=w.payload()[:-2])
    for d in (1, -1):
        name = "B-bad-block-usize-%s-1" % ("plus" if d > 0 else "minus")
        w, rng, seed = small(name)
        w.end()
        mk.add(name, "B", seed, w, "reject", "grammar", usize=w.declared_usize() + d)
    name = "B-empty-block"
    w, rng, seed = _new(name)
    w.end()
    mk.add(name, "B", seed, w, "accept")


def _section_c(mk):
    name = "C-lzma-chunk-of-1-byte"
    w, rng, seed = _new(name)
    w.lz_chunk([("L", 0x41)], 0xE0, DEFAULT_PROPS)
    w.lz_chunk([("L", 0x42)], 0x80)
    w.lz_chunk(random_symbols(w, rng, 30), 0xA0)
    w.lz_chunk([("S",)], 0x80)
    w.end()
    mk.add(name, "C", seed, w, "accept")
    name = "C-max-usize-chunk"
    w, rng, seed = _new(name)
    ch = w.lz_chunk(fill_to(w, rng, 2 * MIB), 0xE0, DEFAULT_PROPS)
    assert ch.usize == 2 * MIB and ch.to_bytes()[:3] == b"\xFF\xFF\xFF"
    w.end()
    mk.add(name, "C", seed, w, "accept", big=True)
    name = "C-max-csize-chunk"
    w, rng, seed = _new(name)

    def lits():
        while w.rc.pending_size() < 65536 - 48:
            yield ("L", rng.randrange(256))
        while True:                     # one literal in one context: well under a byte each, so no size is stepped over
            yield ("L", 0x55)
    ch = w.lz_chunk(lits(), 0xE0, DEFAULT_PROPS, stop=lambda wr: wr.rc.pending_size() >= 65536)
    assert ch.csize == 65536, ch.csize
    w.lz_chunk(literals(rng, 5), 0x80)
    w.end()
    mk.add(name, "C", seed, w, "accept")
    name = "C-bad-csize-below-5"
    w, rng, seed = _new(name)
    w.lz_chunk(literals(rng, 30), 0xE0, DEFAULT_PROPS)
    ch = w.lz_chunk([("L", 0)], 0x80)
    ch.body = ch.body[:4]
    ch.csize = 4
    w.end()
    mk.add(name, "C", seed, w, "reject", "decode")
    for how in ("dict-resets", "C0-chunks"):
        name = "C-4k-block-48-" + how
        w, rng, seed = _new(name)
        for k in range(48):
            n = 85 if k < 47 else 4096 - 47 * 85
            if how == "C0-chunks":
                ctl = 0xE0 if k == 0 else 0xC0
            else:
                ctl = 0xE0 if k % 3 != 1 else 0x01
            if ctl == 0x01:
                w.raw_chunk(bytes(rng.randrange(256) for _ in range(n)), ctl)
            else:
                w.lz_chunk(fill_to(w, rng, n), ctl, (k % 4, 0, k % 5))
        w.end()
        assert w.declared_usize() == 4096
        mk.add(name, "C", seed, w, "accept")


def _section_d(mk):
    name = "D-distance-0"
    w, rng, seed = _new(name)
    w.lz_chunk([("L", 0x61), ("M", 0, 5), ("L", 0x62), ("M", 0, 273)], 0xE0, DEFAULT_PROPS)
    w.end()
    mk.add(name, "D", seed, w, "accept")
    for over in (0, 1):
        name = "D-distance-all-data" + ("-plus-1" if over else "")
        w, rng, seed = _new(name)
        w.lz_chunk(literals(rng, 40) + [("M", 39 + over, 4), ("L", 1)], 0xE0, DEFAULT_PROPS)
        w.end()
        mk.add(name, "D", seed, w, "reject" if over else "accept", "decode" if over else None)
        for how in ("E0", "01-C0"):
            name = "D-distance-behind-reset-%s%s" % (how, "-plus-1" if over else "")
            w, rng, seed = _new(name)
            w.lz_chunk(fill_to(w, rng, 300), 0xE0, DEFAULT_PROPS)
            if how == "E0":
                w.lz_chunk(literals(rng, 10) + [("M", 9 + over, 3), ("L", 1)], 0xE0, DEFAULT_PROPS)
            else:
                w.raw_chunk(bytes(rng.randrange(256) for _ in range(10)), 0x01)
                w.lz_chunk([("M", 9 + over, 3), ("L", 1)], 0xC0, DEFAULT_PROPS)
            w.end()
            mk.add(name, "D", seed, w, "reject" if over else "accept", "decode" if over else None)
    for dsz in (4096, 8192):
        for over in (0, 1):
            name = "D-distance-dict-%d%s" % (dsz, "" if over else "-minus-1")
            w, rng, seed = _new(name)
            w.lz_chunk(fill_to(w, rng, dsz + 900), 0xE0, DEFAULT_PROPS)
            w.lz_chunk([("L", 3), ("M", dsz - 1 + over, 6), ("L", 4)], 0x80)
            w.end()
            mk.add(name, "D", seed, w, "accept", dict_size=dsz, record_only=bool(over))
    name = "D-every-distance-slot"
    w, rng, seed = _new(name)
    w.lz_chunk(fill_to(w, rng, 2 * MIB), 0xE0, DEFAULT_PROPS)
    syms = [("L", 9)]
    for slot in range(43):
        base = slot_base(slot)
        top = min(slot_base(slot + 1) - 1, 2 * MIB) if slot >= 4 else base
        syms += [("M", rng.randrange(base, top + 1), 2 + slot % 5), ("L", slot)]
    syms += [("M", 2 * MIB, 4)]
    w.lz_chunk(syms, 0x80)
    w.end()
    mk.add(name, "D", seed, w, "accept", dict_size=4 * MIB, big=True)
    for dist, tag in ((0xFFFFFFFF, "end-marker"), (0xFFFFFFFE, "slot-63"), (3 << 20, "slot-43-small-dict")):
        name = "D-bad-distance-" + tag
        w, rng, seed = _new(name)
        w.lz_chunk(literals(rng, 40) + [("M", dist, 4), ("L", 1)], 0xE0, DEFAULT_PROPS)
        w.end()
        mk.add(name, "D", seed, w, "reject", "decode", dict_size=4096 if "small" in tag else 8 * MIB)


def _section_e(mk):
    lens = (2, 63, 64, 65, 128, 129, 273)
    for dist in (0, 1, 2, 62, 63, 64, 65, 127, 128, 272, 273):
        name = "E-copy-distance-%d" % dist
        w, rng, seed = _new(name)
        syms = literals(rng, 300)
        for n in lens:
            syms += [("M", dist, n), ("L", rng.randrange(256)), ("L", rng.randrange(256)), ("R", 0, n), ("L", rng.randrange(256))]
        w.lz_chunk(syms, 0xE0, DEFAULT_PROPS)
        w.end()
        mk.add(name, "E", seed, w, "accept")
    for over in (0, 1):
        name = "E-match-ends-at-chunk-end" + ("-plus-1" if over else "")
        w, rng, seed = _new(name)
        ch = w.lz_chunk(literals(rng, 70) + [("M", 64, 65 + over)], 0xE0, DEFAULT_PROPS)
        ch.usize -= over
        w.lz_chunk(literals(rng, 8), 0x80)
        w.end()
        mk.add(name, "E", seed, w, "reject" if over else "accept", "decode" if over else None)
    for sym, tag in ((("S",), "short-rep"), (("R", 0, 4), "rep-match")):
        for where in ("block-start", "behind-reset"):
            name = "E-bad-%s-first-at-%s" % (tag, where)
            w, rng, seed = _new(name)
            if where == "behind-reset":
                w.lz_chunk(fill_to(w, rng, 200), 0xE0, DEFAULT_PROPS)
            w.lz_chunk([sym] + literals(rng, 10), 0xE0, DEFAULT_PROPS)
            w.end()
            mk.add(name, "E", seed, w, "reject", "decode")


def _section_f(mk):
    def base(name):
        w, rng, seed = _new(name)
        w.lz_chunk(random_symbols(w, rng, 40), 0xE0, DEFAULT_PROPS)
        ch = w.lz_chunk(random_symbols(w, rng, 60), 0x80)
        w.lz_chunk(random_symbols(w, rng, 20), 0x80)
        w.end()
        return w, seed, ch

    name = "F-untouched"
    w, seed, ch = base(name)
    mk.add(name, "F", seed, w, "accept")
    name = "F-bad-first-payload-byte"
    w, seed, ch = base(name)
    ch.body[0] = 1
    mk.add(name, "F", seed, w, "reject", "decode")
    name = "F-bad-csize-plus-1-pad"
    w, seed, ch = base(name)
    ch.body.append(0)
    ch.csize += 1
    mk.add(name, "F", seed, w, "reject", "decode")
    for k in (1, 2, 3, 4):
        name = "F-bad-csize-minus-%d-cut" % k
        w, seed, ch = base(name)
        ch.body = ch.body[:-k]
        ch.csize -= k
        mk.add(name, "F", seed, w, "reject", "decode")
    name = "F-bad-final-code"
    w, seed, ch = base(name)
    ch.body[-1] ^= 0x01
    mk.add(name, "F", seed, w, "reject", "decode")


def _section_g(mk, count=200):
    for i in range(count):
        name = "G-mix-%03d" % i
        w, rng, seed = _new(name)
        target = rng.randrange(1024, 16 * 1024 + 1)
        have_props = False
        first = True
        while len(w.plain) < target:
            if first:
                ctl = rng.choice((0x01, 0xE0, 0xE0))
            else:
                ok = [0x01, 0x02, 0xC0, 0xE0] + ([0x80, 0xA0, 0x80] if have_props else [])
                ctl = rng.choice(ok)
            first = False
            left = target - len(w.plain)
            if ctl < 0x80:
                w.raw_chunk(bytes(rng.randrange(256) for _ in range(rng.randrange(1, min(left, 700) + 1))), ctl)
                if ctl == 0x01:
                    have_props = False
            else:
                props = None
                if ctl >= 0xC0:
                    lp = rng.randrange(5)
                    props = (rng.randrange(5 - lp), lp, rng.randrange(5))
                    have_props = True
                w.lz_chunk(random_symbols(w, rng, rng.randrange(4, 40), long_share=0.15, max_len=min(273, max(left, 2))), ctl, props)
        w.end()
        mk.add(name, "G", seed, w, "accept", header_sizes=i % 2 == 0)


def control_block():
    """A known-good Block of a little over 4 KiB: stands in front of every rejected case and between them."""
    w, rng, _ = _new("control")
    w.lz_chunk(random_symbols(w, rng, 120), 0xE0, DEFAULT_PROPS)
    w.raw_chunk(bytes(rng.randrange(256) for _ in range(100)), 0x02)
    w.lz_chunk(fill_to(w, rng, max(4200 - len(w.plain), 16)), 0x80)
    w.end()
    mk = _Maker()
    mk.add("control", "-", _seed("control"), w, "accept")
    return mk.cases[0]


@functools.lru_cache(maxsize=None)
def cases():
    """The whole case list, in a fixed order (built once per process)."""
    mk = _Maker()
    for section in (_section_a, _section_b, _section_c, _section_d, _section_e, _section_f, _section_g):
        section(mk)
    return tuple(mk.cases)


@functools.lru_cache(maxsize=None)
def control():
    return control_block()


# ---------------------------------------------------------------- Streams of several cases
FORWARD_CASES = ("B-bad-01-then-80", "B-bad-props-13", "D-distance-behind-reset-E0-plus-1", "E-match-ends-at-chunk-end-plus-1",
                 "F-bad-csize-plus-1-pad")


def by_name():
    return {c.name: c for c in cases()}


def forward_stream(name):
    """(Stream, the bytes in front of the defect): control, a good case, control, the rejected case `name`, control; CRC32"""
    ctl, good, bad = control(), by_name()["F-untouched"], by_name()[name]
    assert bad.intent == "reject"
    raw, _ = frame([ctl.block(), good.block(), ctl.block(), bad.block(b""), ctl.block()], CHECK_CRC32)
    return raw, ctl.plain + good.plain + ctl.plain


def interleave(cs, accepted):
    """`cs` with a control Block in front of every case that is not accepted (`accepted`: name -> bool), after every eighth
    accepted one and at the end: [(case, is_control)]"""
    ctl, out, run = control(), [], 0
    for c in cs:
        if not accepted[c.name] or run == 8:
            out.append((ctl, True))
            run = 0
        out.append((c, False))
        run = run + 1 if accepted[c.name] else 8
    out.append((ctl, True))
    return out
