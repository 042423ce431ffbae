"""numpy model of the automatic per-Block delta filter (DESIGN.md 3.5 "Automatic delta"; the C statement of the same rule
is xz_amd/csrc/delta_rule.h): candidates, sample set, histograms, the integer log L, the costs S and the rule.  Integers
only, so that the device has to agree bit for bit.  Also the 20 corpus classes the rule was calibrated on."""
import numpy as np

import _corpora as cp

DISTS = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32)      # 0 = no filter
PERIOD, WINDOW, MARGIN = 65536, 4096, 128

# T[m] = floor(256 * log2(1 + m / 256) + 0.5): the committed constants (test_auto_delta_rule checks them against the formula)
T = np.array([
    0, 1, 3, 4, 6, 7, 9, 10, 11, 13, 14, 16, 17, 18, 20, 21, 22, 24, 25, 26, 28, 29, 30, 32, 33, 34, 36, 37, 38, 40, 41, 42,
    44, 45, 46, 47, 49, 50, 51, 52, 54, 55, 56, 57, 59, 60, 61, 62, 63, 65, 66, 67, 68, 69, 71, 72, 73, 74, 75, 77, 78, 79, 80, 81,
    82, 84, 85, 86, 87, 88, 89, 90, 92, 93, 94, 95, 96, 97, 98, 99, 100, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112,
    113, 114, 116, 117, 118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 130, 131, 132, 133, 134, 135, 136, 137,
    138, 139, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149, 150, 151, 152, 153, 154, 155, 155, 156, 157, 158, 159, 160,
    161, 162, 163, 164, 165, 166, 167, 168, 169, 169, 170, 171, 172, 173, 174, 175, 176, 177, 178, 178, 179, 180, 181, 182,
    183, 184, 185, 185, 186, 187, 188, 189, 190, 191, 192, 192, 193, 194, 195, 196, 197, 198, 198, 199, 200, 201, 202, 203,
    203, 204, 205, 206, 207, 208, 208, 209, 210, 211, 212, 212, 213, 214, 215, 216, 216, 217, 218, 219, 220, 220, 221, 222,
    223, 224, 224, 225, 226, 227, 228, 228, 229, 230, 231, 231, 232, 233, 234, 234, 235, 236, 237, 238, 238, 239, 240, 241,
    241, 242, 243, 244, 244, 245, 246, 247, 247, 248, 249, 249, 250, 251, 252, 252, 253, 254, 255, 255], dtype=np.int64)


def sample_offsets(blen):
    """Offsets i of a Block of blen bytes with (i mod PERIOD) < WINDOW (a Block shorter than WINDOW: all of it)."""
    i = np.arange(blen, dtype=np.int64)
    return i[(i % PERIOD) < WINDOW]


def histograms(block):
    """uint32 [11, 256]: hist[k][v] counts (x[i] - (x[i - d] if i >= d else 0)) & 255 over the sample set, d = DISTS[k]."""
    x = np.frombuffer(bytes(block), dtype=np.uint8).astype(np.int64)
    idx = sample_offsets(len(x))
    h = np.zeros((len(DISTS), 256), dtype=np.uint32)
    for k, d in enumerate(DISTS):
        prev = np.zeros(len(idx), dtype=np.int64)
        if d:
            ok = idx >= d
            prev[ok] = x[idx[ok] - d]
        h[k] = np.bincount((x[idx] - prev) & 255, minlength=256).astype(np.uint32)
    return h


def log256(c):
    """L(c) of an integer array: 256 * floor(log2 c) + T[the 8 bits below the leading one], L(0) = 0."""
    c = np.asarray(c, dtype=np.int64)
    out = np.zeros(c.shape, dtype=np.int64)
    pos = c > 0
    cp_ = c[pos]
    e = np.zeros(cp_.shape, dtype=np.int64)
    for s in range(1, 40):                          # floor(log2) by comparison: no floating point
        e += (cp_ >> s) > 0
    m = np.where(e >= 8, cp_ >> np.maximum(e - 8, 0), cp_ << np.maximum(8 - e, 0)) & 255
    out[pos] = 256 * e + T[m]
    return out


def costs(hist):
    """S[k] = Ns * L(Ns) - sum_v hist[k][v] * L(hist[k][v]) in 1/256 bit (Python ints), and Ns."""
    h = hist.astype(np.int64)
    ns = int(h[0].sum())
    lns = int(log256(np.array([ns]))[0])
    return [ns * lns - int((h[k] * log256(h[k])).sum()) for k in range(len(DISTS))], ns


def rule(S, ns):
    """The distance of the cheapest filter (ties: the smaller distance) when it beats no filter by MARGIN / 256 bit per sampled
    byte, else 0; and that cheapest filter's distance d* either way."""
    best = 1
    for k in range(2, len(DISTS)):
        if S[k] < S[best]:
            best = k
    chosen = DISTS[best] if ns and S[best] + MARGIN * ns <= S[0] else 0
    return chosen, DISTS[best]


def choose(block):
    """(chosen distance, d*, histograms) of one Block."""
    h = histograms(block)
    S, ns = costs(h)
    chosen, dstar = rule(S, ns)
    return chosen, dstar, h


def choose_blocks(data, block_size):
    """What the device must answer for `data` cut into Blocks: ([distance per Block], uint32 [nblocks, 11, 256])."""
    data = bytes(data)
    out, hs = [], []
    for off in range(0, len(data), block_size):
        c, _, h = choose(data[off:off + block_size])
        out.append(c)
        hs.append(h)
    return out, (np.stack(hs) if hs else np.zeros((0, len(DISTS), 256), dtype=np.uint32))


# the 20 classes of the calibration (tests/_corpora.py) and what the rule must pick for each
CLASSES = dict(cp.NUMERIC_CLASSES)
CLASSES.update(cp.REVIEW_CLASSES)
CLASSES["relocs"] = cp.KNOWN_OUTSIDE["relocs"][0]
CLASSES["logs"] = cp.logs
CLASSES["json"] = cp.json_records
EXPECTED = {"f32sine": 4, "f32two": 4, "pcm16": 4, "int32walk": 4, "rgba": 4, "f32mesh": 12, "f64sine": 8, "structs24": 24,
            "relocs": 24}
for _name in CLASSES:
    EXPECTED.setdefault(_name, 0)
