"""numpy model of the automatic per-Block literal context (DESIGN.md 3.5 "Automatic literal context"; the C statement of
the same rule is xz_amd/csrc/lclp_rule.h): sample set, joint histogram, candidates, marginals, costs and the rule.  Integers
only, so that the device has to agree bit for bit.  Also the corpus classes the rule was calibrated on."""
import numpy as np

import _auto_delta as ad
import _corpora as cp

CELL, MARGIN = 3072, 32         # XZAMD_LL_CELL, XZAMD_LL_MARGIN (1/256 bit per used cell / per sampled byte)
HIST_SHAPE = (8, 8, 256)        # [pos & 7][prev >> 5][byte]


def joint_hist(block):
    """uint32 [8, 8, 256]: H[i & 7][x[i - 1] >> 5][x[i]] over the sample set of the automatic delta (x[-1] = 0)."""
    x = np.frombuffer(bytes(block), dtype=np.uint8).astype(np.int64)
    idx = ad.sample_offsets(len(x))
    h = np.zeros(HIST_SHAPE, dtype=np.uint32)
    if len(idx) == 0:
        return h
    prev = np.zeros(len(idx), dtype=np.int64)
    ok = idx >= 1
    prev[ok] = x[idx[ok] - 1]
    flat = ((idx & 7) * 8 + (prev >> 5)) * 256 + x[idx]
    return np.bincount(flat, minlength=8 * 8 * 256).astype(np.uint32).reshape(HIST_SHAPE)


def candidates(lc, lp):
    """The (lc, lp) pairs the rule looks at for a job with (lc, lp): its own first, then every other pair with no more
    literal coders, lc <= 3 and lp <= 3, by lp then lc.  A job pair the statistic cannot price (lc or lp above 3) stands alone."""
    out = [(lc, lp)]
    if lc > 3 or lp > 3:
        return out
    for p in range(4):
        for c in range(4):
            if c + p <= lc + lp and (c, p) != (lc, lp):
                out.append((c, p))
    return out


def marginal(hist, lc, lp):
    """int64 [1 << lp, 1 << lc, 256]: the histogram of the bytes under the contexts of (lc, lp): the low lp bits of the
    offset, the high lc bits of the byte in front."""
    h = hist.astype(np.int64).reshape(8 >> lp, 1 << lp, 1 << lc, 8 >> lc, 256)
    return h.sum(axis=(0, 3))


def cost(hist, lc, lp):
    """sum over the contexts of N * L(N) - sum_v c * L(c), plus CELL per used (context, byte) cell; in 1/256 bit."""
    m = marginal(hist, lc, lp).reshape(-1, 256)
    n = m.sum(axis=1)
    return int((n * ad.log256(n)).sum()) - int((m * ad.log256(m)).sum()) + CELL * int((m != 0).sum())


def rule(hist, lc=3, lp=0):
    """((lc, lp) chosen, [cost per candidate], Ns).  The cheapest candidate -- ties: fewer literal coders, then the smaller
    lp -- when it beats the job's own pair by MARGIN / 256 bit per sampled byte, else the job's own."""
    cands = candidates(lc, lp)
    ns = int(hist.astype(np.int64).sum())
    if len(cands) == 1:
        return cands[0], [0], ns
    S = [cost(hist, c, p) for c, p in cands]
    best = 0
    for k in range(1, len(cands)):
        kb, kk = (S[best], sum(cands[best]), cands[best][1]), (S[k], sum(cands[k]), cands[k][1])
        if kk < kb:
            best = k
    chosen = cands[best] if ns and S[best] + MARGIN * ns <= S[0] else cands[0]
    return chosen, S, ns


def choose_blocks(data, block_size, lc=3, lp=0):
    """What the device must answer for `data` cut into Blocks: ([(lc, lp) per Block], uint32 [nblocks, 8, 8, 256])."""
    data = bytes(data)
    out, hs = [], []
    for off in range(0, len(data), block_size):
        h = joint_hist(data[off:off + block_size])
        out.append(rule(h, lc, lp)[0])
        hs.append(h)
    return out, (np.stack(hs) if hs else np.zeros((0,) + HIST_SHAPE, dtype=np.uint32))


# ---- the classes of the calibration -------------------------------------------------------------------------------------
def f32_walk(n, seed=130):
    """float32 random walk: cumulative sum of N(0, 1) steps."""
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(0.0, 1.0, n // 4 + 1)).astype("<f4").tobytes()[:n]


def flow_records(n, seed=131):
    """32-byte flow records {u32 src, u32 dst, u16 sport, u16 dport, u8 proto, u8 flags, u16 zero, u32 packets, u32 bytes,
    u64 microsecond timestamp}: 64 hosts in two subnets, ephemeral source ports, a few services, a rising clock."""
    rng = np.random.default_rng(seed)
    m = n // 32 + 1
    rec = np.zeros(m, dtype=[("src", "<u4"), ("dst", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("proto", "u1"),
                             ("flags", "u1"), ("zero", "<u2"), ("packets", "<u4"), ("bytes", "<u4"), ("ts", "<u8")])
    rec["src"] = 0x0A000000 + rng.integers(0, 64, m)
    rec["dst"] = 0xC0A80100 + rng.integers(0, 64, m)
    rec["sport"] = rng.integers(32768, 61000, m)
    rec["dport"] = np.array([80, 443, 53, 22, 8080, 5432], dtype=np.uint16)[rng.integers(0, 6, m)]
    rec["proto"] = np.array([6, 6, 6, 17], dtype=np.uint8)[rng.integers(0, 4, m)]
    rec["flags"] = rng.integers(0, 32, m)
    pk = rng.geometric(0.05, m)
    rec["packets"] = pk
    rec["bytes"] = pk * rng.integers(40, 1500, m)
    rec["ts"] = 1_700_000_000_000_000 + np.cumsum(rng.integers(1, 5000, m))
    return rec.tobytes()[:n]


def word_text(n, seed=132):
    """Words drawn from a short English list, lines of about 70 characters."""
    rng = np.random.default_rng(seed)
    words = cp._WORDS
    pick = rng.integers(0, len(words), n // 3 + 16)
    out, col = bytearray(), 0
    for i in pick:
        w = words[i]
        out += w
        col += len(w) + 1
        if col > 70:
            out += b"\n"
            col = 0
        else:
            out += b" "
        if len(out) >= n:
            break
    return bytes(out[:n])


def utf16_text(n, seed=133):
    """The word text as UTF-16LE."""
    return word_text(n // 2 + 1, seed).decode("ascii").encode("utf-16-le")[:n]


CLASSES = {"f32walk": f32_walk, "rgba": cp.rgba_image, "flow32": flow_records, "f64sine": cp.f64_sine,
           "words": word_text, "utf16": utf16_text, "logs": cp.logs, "int32walk": cp.int32_walk}
# The rule must leave the text classes at the job's pair.  (The int32 walk of _corpora is no such class: the reference itself
# is 1.1 % smaller with lp = 2 on it, so it only stands under the bound that holds for every class.)
TEXT_CLASSES = ("words", "utf16", "logs")
GAIN_CLASSES = ("f32walk", "rgba")                   # ... and reach half of the best candidate's saving on these
