"""The rule of the automatic per-Block BCJ filter (DESIGN.md 3.5 "Automatic BCJ") on the CPU: xz_amd/csrc/auto_bcj_rule.h,
compiled into tests/host_stub/rule_auto_bcj.c, against the numpy model (tests/_auto_bcj.py) integer for integer; what the
rule picks for text, random bytes, CJK text made of E8 xx xx, float32, real x86-64 code, the two synthetic instruction
streams and random bytes with planted sites; that the reference encoder (the liblzma of oracle/_ref, preset 6) agrees; and
the edge inputs."""
import os
import subprocess

import numpy as np
import pytest

import _auto_bcj as ab
import _oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 256 << 10
X86, ARM64 = 4, 0x0A
EXPECTED = {"text": 0, "random": 0, "cjk": 0, "float32": 0, "synth_x86": X86, "synth_arm64": ARM64, "planted": 0, "x86_code": X86}
_cache = {}


def _class(name):
    if name not in _cache:
        _cache[name] = {"text": lambda: ab.text(SIZE), "random": lambda: ab.rnd(SIZE, 1), "cjk": lambda: ab.cjk_e8(SIZE),
                        "float32": lambda: ab.float32(SIZE), "synth_x86": lambda: ab.synth_x86(SIZE, 1),
                        "synth_arm64": lambda: ab.synth_arm64(SIZE, 2), "planted": lambda: ab.planted_random(SIZE, 3),
                        "x86_code": lambda: ab.x86_code(1 << 20)}[name]()
    return _cache[name]


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rule_auto_bcj")
    exe = str(d / "rule_auto_bcj")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_stub", "rule_auto_bcj.c"), "-o", exe], check=True)
    return exe, d


def _c_rule(rule_exe, data, bs):
    """([(kind, N0, N1, S_rel0, S_abs0, S_rel1, S_abs1) per Block], uint32 [nb, 2, 2, 4096]) from the C header"""
    exe, d = rule_exe
    src, hist = str(d / "in.bin"), str(d / "hist.bin")
    with open(src, "wb") as f:
        f.write(data)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    p = subprocess.run([exe, src, str(bs), hist], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-3000:]
    rows = [tuple(int(v) for v in line.split()) for line in p.stdout.splitlines()]
    return rows, np.fromfile(hist, dtype=np.uint32).reshape(len(rows), 2, 2, ab.BUCKETS)


def _model_rows(data, bs):
    rows, hs = [], []
    for off in range(0, len(data), bs):
        k, h, ns, sr, sa = ab.choose(data[off:off + bs])
        rows.append((k, int(ns[0]), int(ns[1]), sr[0], sa[0], sr[1], sa[1]))
        hs.append(h)
    return rows, hs


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_c_header_is_the_model_and_picks_the_expected(rule_exe, name):
    data = _class(name)
    rows, hist = _c_rule(rule_exe, data, len(data))
    want, want_hist = _model_rows(data, len(data))
    kind, n0, n1, sr0, sa0, sr1, sa1 = rows[0]
    print(f"{name}: kind {kind}, sites {n0} / {n1}, x86 {(sr0 - sa0) / 256 / max(n0, 1):+.2f} bit/site, ARM64 {(sr1 - sa1) / 256 / max(n1, 1):+.2f}")
    assert rows == want and np.array_equal(hist[0], want_hist[0])
    assert kind == EXPECTED[name]
    if name in ("text", "cjk", "float32"):
        assert n0 < ab.NMIN                                       # no x86 sites to speak of
    if name == "planted":
        # the count and the density would let it through: the entropy test is what refuses
        assert n0 >= ab.NMIN and n0 * ab.DENS >= len(data) and sa0 + ab.MARGIN * n0 > sr0


def test_c_header_is_the_model_block_by_block(rule_exe):
    """Blocks of 65537 and 200001 bytes over a mix: offsets are Block-relative, the last Block is short"""
    data = ab.synth_x86(SIZE, 11) + ab.text(SIZE) + ab.synth_arm64(SIZE, 12) + ab.rnd(SIZE, 13)
    for bs in (65537, 200001):
        rows, hist = _c_rule(rule_exe, data, bs)
        want, want_hist = _model_rows(data, bs)
        assert rows == want and np.array_equal(hist, np.stack(want_hist))
        assert [r[0] for r in rows] == ab.choose_blocks(data, bs)[0] and {X86, 0} <= {r[0] for r in rows}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_reference_agrees(name):
    """The calibration's two conditions on these classes: a filter that is taken does not lose with the
    reference encoder and is the better of the two; no candidate that is refused would have gained 1 % or more."""
    if not o.have_ref():
        pytest.skip("reference liblzma not built (oracle/_ref)")
    data = _class(name)
    kind, _, ns, _, _ = ab.choose(data)
    plain = len(o.ref_encode_mt(data, 6, block_size=len(data)))
    sizes = {k: len(o.ref_encode_mt_chain(data, 6, k, block_size=len(data))) for k in (X86, ARM64)}
    print(f"{name}: chosen {kind}, reference plain {plain}, x86 {sizes[X86]} ({sizes[X86] / plain:.4f}), ARM64 {sizes[ARM64]} ({sizes[ARM64] / plain:.4f})")
    if kind:
        assert sizes[kind] < plain and sizes[kind] == min(sizes.values())
    else:
        assert min(sizes.values()) > 0.99 * plain


def test_edge_inputs(rule_exe):
    # lengths 0, 1, 4, 5: no Block at all; nothing; one ARM64 site; one x86 site
    assert ab.choose_blocks(b"", 4096)[0] == []
    assert _c_rule(rule_exe, b"", 4096)[0] == []
    for blk, n in ((b"\xe8", [0, 0]), (b"\x01\x00\x00\x94", [0, 1]), (b"\xe8\x00\x00\x00", [0, 0]), (b"\xe8\x01\x00\x00\x00", [1, 0]),
                   (b"\xe8\x01\x00\x00\xff", [1, 0]), (b"\xe9\x01\x00\x00\x00", [1, 0]), (b"\xe8\x01\x00\x00\x01", [0, 0])):
        k, h, ns, _, _ = ab.choose(blk)
        rows, hist = _c_rule(rule_exe, blk, 4096)
        assert k == 0 and ns.tolist() == n and rows == [(0, n[0], n[1], 0, 0, 0, 0)] and np.array_equal(hist[0], h), blk
    # an operand that would cross the Block end is no site: E8 at len - 4, the next Block starting with 00
    two = bytes(100) + b"\xe8\x01\x02\x03" + b"\x00" * 104
    assert ab.sites(two[:104], 0)[0].tolist() == [] and ab.sites(two, 0)[0].tolist() == [100]
    rows, _ = _c_rule(rule_exe, two, 104)
    assert [r[1] for r in rows] == [0, 0]
    # the operands: stored and absolute, Block-relative
    i, rel, a = ab.sites(b"\x90" * 7 + b"\xe8\xf4\xff\xff\xff", 0)
    assert (i.tolist(), rel.tolist(), a.tolist()) == ([7], [0xFFFFFFF4], [0])
    i, rel, a = ab.sites(bytes(8) + (0x94000000 | 0x03FFFFFE).to_bytes(4, "little") + (0x97FFFFFF).to_bytes(4, "little"), 1)
    assert (i.tolist(), rel.tolist(), a.tolist()) == ([8, 12], [0x03FFFFFE, 0x03FFFFFF], [0, 2])
    # ARM64 sites at i mod 4 != 0 are none: the same BL stream shifted by 1, 2, 3 bytes
    code = ab.synth_arm64(65536, 9)
    n_aligned = len(ab.sites(code, 1)[0])
    assert n_aligned > 2000 and ab.choose(code)[0] == ARM64
    for shift in (1, 2, 3):
        shifted = bytes(shift) + code
        k, _, ns, _, _ = ab.choose(shifted)
        rows, _ = _c_rule(rule_exe, shifted, len(shifted))
        assert k == 0 and ns[1] < n_aligned // 8 and rows[0][:3] == (0, int(ns[0]), int(ns[1]))
    # the hash: 12 bits, the constants of the C header
    assert ab.bucket([0, 1, 0xFFFFFFFF, 0x12345678]).tolist() == [0, 2654435761 >> 20, ((0xFFFFFFFF * 2654435761) & ab.M32) >> 20,
                                                                  ((0x12345678 * 2654435761) & ab.M32) >> 20]


def test_rule_thresholds():
    n, length = 1000, 1 << 20
    big = 10 ** 9
    # the margin is inclusive; one unit short refuses
    assert ab.rule([big, 0], [big - ab.MARGIN * n, 0], [n, 0], length) == X86
    assert ab.rule([big, 0], [big - ab.MARGIN * n + 1, 0], [n, 0], length) == 0
    # enough sites, dense enough
    assert ab.rule([big, 0], [0, 0], [ab.NMIN, 0], ab.NMIN * ab.DENS) == X86
    assert ab.rule([big, 0], [0, 0], [ab.NMIN - 1, 0], 1000) == 0
    assert ab.rule([big, 0], [0, 0], [ab.NMIN, 0], ab.NMIN * ab.DENS + 1) == 0
    # two candidates fire: the larger saving, x86 on a tie
    assert ab.rule([big, big], [big // 2, big // 2 - 1], [n, n], length) == ARM64
    assert ab.rule([big, big], [big // 2, big // 2], [n, n], length) == X86
    assert ab.rule([big, big], [big // 2 - 1, big // 2], [n, n], length) == X86
    assert ab.rule([0, 0], [0, 0], [0, 0], 0) == 0
