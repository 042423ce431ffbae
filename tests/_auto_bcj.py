"""numpy model of the automatic per-Block BCJ filter (DESIGN.md 3.5 "Automatic BCJ"; the C statement of the same rule is
xz_amd/csrc/auto_bcj_rule.h): call sites of the two candidates over the whole Block, the hashed histograms of their operands
as stored and made absolute, the costs and the rule.  Integers only, so that the device has to agree bit for bit.  Also the
inputs the tests share: real x86-64 code found on the machine, two synthetic instruction streams, random bytes with planted
sites."""
import glob
import os
import struct
import sys
import sysconfig

import numpy as np
import pytest

from _auto_delta import log256

KINDS = (4, 0x0A)                    # x86, ARM64 (.xz filter ids), in the order of the rule's preference on a tie
BUCKETS = 4096
NMIN, DENS, MARGIN = 256, 2048, 128
M32 = 0xFFFFFFFF


def _u8(block):
    return np.frombuffer(bytes(block), dtype=np.uint8).astype(np.int64)


def sites(block, cand):
    """(offsets i, operands as stored, operands made absolute) of candidate `cand` (0: x86, 1: ARM64) in one Block."""
    x = _u8(block)
    n = len(x)
    if cand == 0:
        if n < 5:
            z = np.zeros(0, dtype=np.int64)
            return z, z, z
        i = np.arange(n - 4, dtype=np.int64)                       # i + 4 < n
        ok = ((x[:n - 4] & 0xFE) == 0xE8) & ((x[4:] == 0x00) | (x[4:] == 0xFF))
        i = i[ok]
        rel = x[i + 1] | x[i + 2] << 8 | x[i + 3] << 16 | x[i + 4] << 24
        return i, rel, (rel + i + 5) & M32
    nw = n // 4                                                     # i mod 4 == 0 and i + 3 < n
    w = x[:4 * nw].reshape(nw, 4)
    w = w[:, 0] | w[:, 1] << 8 | w[:, 2] << 16 | w[:, 3] << 24
    k = np.nonzero((w >> 26) == 0x25)[0].astype(np.int64)
    rel = w[k] & 0x03FFFFFF
    return 4 * k, rel, (rel + k) & 0x03FFFFFF


def bucket(v):
    """h(v) = (v * 2654435761 mod 2^32) >> 20"""
    return ((np.asarray(v, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(M32)) >> np.uint64(20)


def histograms(block):
    """(uint32 [2, 2, 4096]: [candidate][stored, absolute][bucket], uint32 [2]: sites per candidate)"""
    h = np.zeros((len(KINDS), 2, BUCKETS), dtype=np.uint32)
    ns = np.zeros(len(KINDS), dtype=np.uint32)
    for c in range(len(KINDS)):
        i, rel, ab = sites(block, c)
        ns[c] = len(i)
        h[c, 0] = np.bincount(bucket(rel).astype(np.int64), minlength=BUCKETS).astype(np.uint32)
        h[c, 1] = np.bincount(bucket(ab).astype(np.int64), minlength=BUCKETS).astype(np.uint32)
    return h, ns


def cost(hist_row, n):
    """S = N * L(N) - sum_v hist[v] * L(hist[v]) in 1/256 bit (Python int)"""
    h = hist_row.astype(np.int64)
    return int(n) * int(log256(np.array([int(n)]))[0]) - int((h * log256(h)).sum())


def rule(S_rel, S_abs, N, length):
    """The filter id of the candidate that fires with the larger S_rel - S_abs (ties: the earlier candidate), else 0."""
    kind, best = 0, 0
    for k in range(len(KINDS)):
        if N[k] < NMIN or N[k] * DENS < length:
            continue
        if S_abs[k] + MARGIN * N[k] > S_rel[k]:
            continue
        save = S_rel[k] - S_abs[k]
        if kind == 0 or save > best:
            kind, best = KINDS[k], save
    return kind


def choose(block):
    """(filter id, histograms, site counts, S_rel list, S_abs list) of one Block."""
    h, ns = histograms(block)
    S_rel = [cost(h[k, 0], ns[k]) for k in range(len(KINDS))]
    S_abs = [cost(h[k, 1], ns[k]) for k in range(len(KINDS))]
    return rule(S_rel, S_abs, [int(v) for v in ns], len(block)), h, ns, S_rel, S_abs


def choose_blocks(data, block_size):
    """What the device must answer for `data` cut into Blocks: ([filter id per Block], uint32 [nb, 2, 2, 4096], uint32 [nb, 2])."""
    data = bytes(data)
    out, hs, nss = [], [], []
    for off in range(0, len(data), block_size):
        k, h, ns, _, _ = choose(data[off:off + block_size])
        out.append(k)
        hs.append(h)
        nss.append(ns)
    if not out:
        return out, np.zeros((0, len(KINDS), 2, BUCKETS), dtype=np.uint32), np.zeros((0, len(KINDS)), dtype=np.uint32)
    return out, np.stack(hs), np.stack(nss)


# ---- inputs ----
def _exec_segment(path):
    """(file offset, size) of the largest executable PT_LOAD segment of an x86-64 ELF file, or None."""
    try:
        with open(path, "rb") as f:
            eh = f.read(64)
            if len(eh) < 64 or eh[:4] != b"\x7fELF" or eh[4] != 2 or eh[5] != 1 or struct.unpack_from("<H", eh, 18)[0] != 62:
                return None
            phoff, = struct.unpack_from("<Q", eh, 32)
            phentsize, phnum = struct.unpack_from("<HH", eh, 54)
            best = None
            for k in range(phnum):
                f.seek(phoff + k * phentsize)
                ph = f.read(56)
                if len(ph) < 56:
                    break
                p_type, p_flags, p_offset, _, _, p_filesz = struct.unpack_from("<IIQQQQ", ph, 0)
                if p_type == 1 and (p_flags & 1) and (best is None or p_filesz > best[1]):
                    best = (p_offset, p_filesz)
            return best
    except OSError:
        return None


def x86_binaries():
    """[(path, offset, size)] of the executable segments of the interpreter, its libpython and the ROCm clang binaries, largest
    first; every file once."""
    paths = [sys.executable]
    libdir, ldlib = sysconfig.get_config_var("LIBDIR"), sysconfig.get_config_var("LDLIBRARY")
    if libdir and ldlib:
        paths.append(os.path.join(libdir, ldlib))
    paths += sorted(glob.glob("/opt/rocm/llvm/bin/clang*"))
    seen, out = set(), []
    for p in paths:
        rp = os.path.realpath(p)
        if rp in seen or not os.path.isfile(rp):
            continue
        seen.add(rp)
        seg = _exec_segment(rp)
        if seg:
            out.append((rp, seg[0], seg[1]))
    return sorted(out, key=lambda t: -t[2])


_x86_cache = {}


def x86_code(n):
    """n bytes from the middle of the executable segment of the largest binary of x86_binaries(); skips with fewer."""
    if n not in _x86_cache:
        bins = x86_binaries()
        if not bins or bins[0][2] < n:
            pytest.skip(f"no x86-64 executable segment of {n} bytes on this machine")
        path, off, size = bins[0]
        with open(path, "rb") as f:
            f.seek(off + ((size - n) // 2 & ~4095))
            _x86_cache[n] = f.read(n)
        assert len(_x86_cache[n]) == n
    return _x86_cache[n]


def _zipf_targets(rng, n, count, nfun, align):
    """`count` call targets: function starts spread over [0, n), picked by a Zipf law over their rank"""
    starts = (np.sort(rng.integers(0, max(n // align, 1), nfun)) * align).astype(np.int64)
    w = 1.0 / np.arange(1, nfun + 1)
    return starts[rng.permutation(nfun)][rng.choice(nfun, size=count, p=w / w.sum())]


def synth_x86(n, seed):
    """Deterministic stream of pseudo-instructions: 2 - 7 byte instructions of a skewed byte alphabet without E8 / E9, and about
    every eighth one a CALL rel32 (E8) to one of 300 function starts, Zipf-distributed."""
    rng = np.random.default_rng(seed)
    alphabet = np.array([b for b in range(256) if b not in (0xE8, 0xE9)], dtype=np.uint8)
    fill = alphabet[np.minimum(rng.geometric(0.06, n + 16) - 1, len(alphabet) - 1)]
    out = fill[:n].copy()
    ncall = n // 20 + 1
    gaps = rng.integers(2, 8, (ncall, 8)).sum(axis=1) + 5
    pos = np.cumsum(gaps) - gaps[0]
    pos = pos[pos + 5 <= n]
    tg = _zipf_targets(rng, n, len(pos), 300, 16)
    rel = (tg - (pos + 5)) & M32
    out[pos] = 0xE8
    for k in range(4):
        out[pos + 1 + k] = (rel >> (8 * k)) & 255
    return out.tobytes()


def synth_arm64(n, seed):
    """Deterministic stream of 4-byte pseudo-instructions (top bytes of common A64 data-processing and load / store forms,
    neither BL nor ADRP), about every eighth one a BL to one of 300 function starts, Zipf-distributed.  A tail of n mod 4 bytes
    is zeros."""
    rng = np.random.default_rng(seed)
    nw = n // 4
    tops = np.array([0xAA, 0xF9, 0xB9, 0x91, 0xD1, 0x52, 0x2A, 0x54, 0xA9, 0x39], dtype=np.int64)
    low = np.minimum(rng.geometric(0.002, nw) - 1, (1 << 24) - 1).astype(np.int64)
    w = tops[rng.integers(0, len(tops), nw)] << 24 | low
    gaps = rng.integers(3, 14, nw // 8 + 1)
    pos = np.cumsum(gaps) - gaps[0]
    pos = pos[pos < nw]
    tg = _zipf_targets(rng, 4 * nw, len(pos), 300, 4) >> 2
    w[pos] = 0x94000000 | ((tg - pos) & 0x03FFFFFF)
    return w.astype("<u4").tobytes() + bytes(n - 4 * nw)


def planted_random(n, seed, every=64):
    """Random bytes with E8 .. .. .. 00 planted every `every` bytes (the site density of code): the operands never repeat, so
    only the entropy test of the rule can refuse this."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    pos = np.arange(0, n - 5, every)
    x[pos] = 0xE8
    x[pos + 4] = 0x00
    return x.tobytes()


def text(n, seed=5):
    """n bytes of word-like ASCII text (numpy only: the CPU tests have no use for the library's corpus)"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(l)).astype(np.uint8)) for l in rng.integers(2, 10, 500)]
    idx = np.minimum(rng.geometric(0.02, n // 3 + 8) - 1, 499)
    return b" ".join(words[i] for i in idx)[:n].ljust(n, b".")


def cjk_e8(n, seed=6):
    """UTF-8 of CJK ideographs U+8000 .. U+8FFF: every character is E8 xx xx"""
    rng = np.random.default_rng(seed)
    cps = 0x8000 + np.minimum(rng.geometric(0.003, n // 3 + 1) - 1, 0xFFF)
    return "".join(map(chr, cps)).encode("utf-8")[:n].ljust(n, b" ")


def float32(n, seed=7):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(0, 1, n // 4 + 1)).astype("<f4").tobytes()[:n]


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
