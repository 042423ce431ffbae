"""Composite Blocks: inputs whose compressibility changes inside a Block (test infrastructure only; numpy only).

The encoder's back end decides per parse piece whether to store it, and cuts at 32 KiB (the shortest piece that may be
stored), 64 KiB (the end of the seed piece) and 256 KiB (the shortest encode span).  The named inputs below put the switch
between incompressible and compressible bytes at and one byte to either side of those boundaries and just in front of the
Block's end; ``draw(seed)`` makes random ones from the same segment kinds.  Everything is seeded and deterministic.

A segment is ``(kind, length)`` or ``(kind, length, seed)``; the kinds:
  "r"  uniform random bytes (incompressible)
  "l"  lorem-ipsum words picked by a small generator
  "t"  the same text read backwards (other words, other line structure: corpus_text itself lives in the library)
  "z"  zeros
  "p"  period 3
  "a"  random bytes over a 4-symbol alphabet: compress to a quarter, but cost a decision per byte
"""
import functools

import numpy as np

K = 1024
MIB = 1 << 20

_WORDS = ("lorem ipsum dolor sit amet consectetur adipisicing elit sed do eiusmod tempor incididunt ut labore et dolore magna "
          "aliqua ut enim ad minim veniam quis nostrud exercitation ullamco laboris nisi ut aliquip ex ea commodo consequat duis "
          "aute irure dolor in reprehenderit in voluptate velit esse cillum dolore eu fugiat nulla pariatur excepteur sint "
          "occaecat cupidatat non proident sunt in culpa qui officia deserunt mollit anim id est laborum").split()


@functools.lru_cache(maxsize=None)
def _lorem(n):
    rng = np.random.default_rng(4242)
    parts, total, w = [], 0, 0
    picks = rng.integers(0, len(_WORDS), n // 3 + 16)
    for k in picks:
        s = _WORDS[int(k)] + (".\n" if w % 11 == 10 else " ")
        parts.append(s)
        total += len(s)
        w += 1
        if total >= n:
            break
    return "".join(parts).encode("ascii")[:n]


def segment(kind, n, seed=1):
    if kind == "r":
        return np.random.default_rng(1000 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "l":
        return _lorem(max(n, 1 << 16))[:n]
    if kind == "t":
        return _lorem(max(n, 1 << 16))[:n][::-1]
    if kind == "z":
        return bytes(n)
    if kind == "p":
        return (b"\x17\xA5\x3C" * (n // 3 + 1))[:n]
    if kind == "a":
        return (np.random.default_rng(2000 + seed).integers(0, 4, n, dtype=np.uint8) * 61 + 7).astype(np.uint8).tobytes()
    raise ValueError(kind)


def build(segments):
    return b"".join(segment(*s) for s in segments)


KINDS = "rltzpa"
LENGTHS = (1, 5, 100, 4096, 32767, 32768, 65535, 65536, 65537, 100000, 200000, 262144, 300000, 400000, 524288, 700000)
DRAW_MAX = 3 * MIB // 2


def draw_segments(seed):
    """1-6 segments, kinds and lengths drawn independently; segments that would take the input past 1.5 MiB are left out
    (the first one always stays)"""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, 7))
    segs, total = [], 0
    for i in range(k):
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        n = int(LENGTHS[int(rng.integers(0, len(LENGTHS)))])
        s = int(rng.integers(1, 1000))
        if segs and total + n > DRAW_MAX:
            continue
        segs.append((kind, n, s))
        total += n
    return segs


def draw(seed):
    """one random composite input: bytes"""
    return build(draw_segments(seed))


def describe(segments):
    return "+".join(f"{s[0]}{s[1]}" for s in segments)


# name -> segments.  Offsets in the comments are from the Block's start at Blocks of 1 MiB (every input but the last is one
# such Block; at Blocks of 300000 bytes the first Block sees the same switch where it lies below 300000).  The compressible
# tails are short (64 ... 96 KiB) where the boundary under test lies in front of them: the device tests pay per byte.  Behind the
# prefixes of 256 and 320 KiB they are 256 KiB, so that a second encode span exists behind the first.
NAMED = {
    "all-random": [("r", 400 * K)],                                      # a wholly incompressible Block: stored pieces only
    "random-then-1": [("r", 300 * K), ("z", 1)],                         # incompressible with one compressible byte behind it (switch at end - 1)
    "head-then-random": [("l", 64 * K), ("r", 300 * K)],                 # compressible head, then stored pieces to the Block's end
    "alternate-3": [("r", 100 * K), ("l", 100 * K), ("r", 100 * K, 2), ("t", 100 * K)],   # three alternations, none on a boundary
    "r32k-1+l": [("r", 32767), ("l", 96 * K)],                           # 32 KiB - 1: one byte too short to make a piece that may be stored
    "r32k+l": [("r", 32768), ("l", 96 * K)],                             # 32 KiB: the shortest piece that may be stored (plen >= 32768)
    "r32k+1+l": [("r", 32769), ("l", 96 * K)],                           # 32 KiB + 1
    "r64k-1+t": [("r", 65535), ("t", 96 * K)],                           # 64 KiB - 1: the seed piece ends one byte into the text
    "r64k+t": [("r", 65536), ("t", 96 * K)],                             # 64 KiB: the seed piece is exactly the incompressible part
    "r64k+1+t": [("r", 65537), ("t", 96 * K)],                           # 64 KiB + 1: one random byte in the piece behind the seed piece
    "r64k+t512k": [("r", 65536), ("t", 512 * K)],                        # the stored seed piece in front of two encode spans, the second with a carried model (stressed plan)
    "l64k+r64k+l": [("l", 65536), ("r", 65536), ("l", 64 * K)],          # a stored piece that starts at the seed piece's end, behind an adapted model
    "r256k-1+l": [("r", 262143), ("l", 96 * K)],                         # 256 KiB - 1: the switch one byte in front of the shortest encode span's end
    "r256k+l": [("r", 262144), ("l", 96 * K)],                           # 256 KiB: the switch at the end of the shortest encode span
    "r256k+1+l": [("r", 262145), ("l", 96 * K)],                         # 256 KiB + 1
    "l256k+r+l": [("l", 262144), ("r", 64 * K), ("l", 64 * K)],          # compressible up to 256 KiB, a stored stretch behind it, text again
    "l+r5": [("l", 128 * K), ("r", 5)],                                  # switch at end - 5, into incompressible
    "r+l5": [("r", 300 * K), ("l", 5)],                                  # switch at end - 5, out of incompressible
    "z+r1": [("z", 128 * K), ("r", 1)],                                  # switch at end - 1, one random byte behind a long run
    "r256k+t": [("r", 256 * K), ("t", 256 * K)],                         # prefix 256 KiB in front of text
    "r320k+t": [("r", 320 * K), ("t", 256 * K)],                         # prefix 320 KiB in front of text
    "r512k+t": [("r", 512 * K), ("t", 64 * K)],                          # prefix 512 KiB in front of text
    "r256k+z": [("r", 256 * K), ("z", 256 * K)],                         # prefix 256 KiB in front of zeros
    "r320k+z": [("r", 320 * K), ("z", 256 * K)],                         # prefix 320 KiB in front of zeros
    "r512k+z": [("r", 512 * K), ("z", 64 * K)],                          # prefix 512 KiB in front of zeros
    "r256k+p": [("r", 256 * K), ("p", 256 * K)],                         # prefix 256 KiB in front of period 3
    "r320k+p": [("r", 320 * K), ("p", 256 * K)],                         # prefix 320 KiB in front of period 3
    "r512k+p": [("r", 512 * K), ("p", 64 * K)],                          # prefix 512 KiB in front of period 3
    "a+r+a": [("a", 128 * K), ("r", 64 * K), ("a", 64 * K, 2)],          # 4-symbol noise around a stored stretch: many decisions per byte
    "r512k+t512k+l": [("r", 512 * K), ("t", 512 * K), ("l", 64 * K)],    # two Blocks of 1 MiB: prefix 512 KiB in the first, plain text in the second
}

assert all(sum(s[1] for s in v) < DRAW_MAX for v in NAMED.values())


@functools.lru_cache(maxsize=None)
def named(name):
    return build(NAMED[name])


# ---------------------------------------------------------------- encoder settings the composite tests run
SETTINGS = ("p6", "p9e", "p4", "p6-stress", "p1", "p3")
BLOCK_SIZES = (MIB, 300000)


def options_for(setting):
    """xz_amd.LzmaOptions of a setting: the preset's defaults; "p6-stress" is preset 6 with the stressed plan of the stage
    tests (small parse pieces, no bit bound on them, several encode spans per Block)"""
    import xz_amd
    preset = {"p6": 6, "p9e": 9 | 0x80000000, "p4": 4, "p6-stress": 6, "p1": 1, "p3": 3}[setting]
    opts = xz_amd.preset_options(preset)
    if setting == "p6-stress":
        opts.span_cost = 50000
        opts.span_bits = 0
        opts.enc_span_bits = 300000
    return opts


# Which Blocks of the named inputs show the stored-prefix defect, per setting and Block size: recorded from the
# oracle on the CPU when the list was written (tests/test_composite_oracle.py asserts equality with it, and the device
# test expects the same of the device).  {setting: {block size: {name: Block numbers}}}; everything not listed is valid.
# At Blocks of 300000 bytes no Block is long enough to show it.
EXPECTED_DEFECT = {
    "p6": {
        MIB: {"r320k+t": (0,), "r512k+t": (0,), "r512k+z": (0,), "r512k+p": (0,), "r512k+t512k+l": (0,)},
        300000: {},
    },
    "p9e": {
        MIB: {"r320k+t": (0,), "r512k+t": (0,), "r512k+z": (0,), "r512k+p": (0,), "r512k+t512k+l": (0,)},
        300000: {},
    },
    "p4": {
        MIB: {"r512k+t": (0,), "r512k+z": (0,), "r512k+p": (0,), "r512k+t512k+l": (0,)},
        300000: {},
    },
    "p6-stress": {
        MIB: {"r256k+t": (0,), "r320k+t": (0,), "r512k+t": (0,), "r256k+z": (0,), "r320k+z": (0,),
              "r512k+z": (0,), "r256k+p": (0,), "r320k+p": (0,), "r512k+p": (0,), "r512k+t512k+l": (0,)},
        300000: {},
    },
    "p1": {
        MIB: {},
        300000: {},
    },
    "p3": {
        MIB: {},
        300000: {},
    },
}


def expected_defect(setting, block_size, name):
    """Block numbers of a named input that are expected to show the defect"""
    return tuple(EXPECTED_DEFECT[setting][block_size].get(name, ()))
