"""Device decoder with filter chains: {up to three of BCJ | delta, LZMA2}, Block-parallel and as a verification decode,
against the input, the REAL reference encoder / decoder (oracle/_ref), the reference's fixture files and plain
arithmetic (tests/test_decode_filter_fixtures.py checks these yardsticks themselves on the CPU)."""
import glob
import os
import time

import numpy as np
import pytest

import _filters as f
import _oracle as o
from test_gpu_parity import _arm64_like, _bcj_like

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    e = xz_amd.Encoder()
    yield e
    e.close()


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _opts(preset, chain):
    import xz_amd
    opts = xz_amd.preset_options(preset)
    vals = [xz_amd.filter_delta(d) if fid == f.DELTA else fid for fid, d in chain]
    opts.bcj, opts.bcj2, opts.bcj3 = (vals + [0, 0, 0])[:3]
    return opts


N = 393216          # 3 x 131072


def _input(chain):
    """corpus_x86 for x86, corpus_mixed + an int16 / int32 ramp with noise for delta and the fixed-width filters, plus
    a stretch with planted branches of every BCJ architecture in the chain."""
    parts = []
    for fid, _ in chain:
        if fid == f.BCJ["x86"]:
            parts.append(o.corpus_x86(150000, 7))
        elif fid == f.BCJ["arm64"]:
            parts.append(_arm64_like(60000, 3))
        elif fid != f.DELTA:
            name = [k for k, v in f.BCJ.items() if v == fid][0]
            parts.append(_bcj_like(name, 40000 if name == "riscv" else 60000, 5))
    parts += [f.ramp_noise(60000, 1, 2), f.ramp_noise(60000, 2, 4)]
    head = b"".join(parts)
    return (head + o.corpus_mixed(N - len(head), 11))[:N]


def _ragged_block_size(chain):
    """A Block size whose last Block is neither a multiple of 4 nor of any delta distance of the chain."""
    bs = 100003
    while True:
        last = N % bs
        if last and last % 4 and all(d == 1 or last % d for fid, d in chain if fid == f.DELTA):
            return bs
        bs += 1


CHAINS = ([(k, [(v, 1)]) for k, v in sorted(f.BCJ.items())]
          + [(f"delta{d}", [(f.DELTA, d)]) for d in (1, 2, 3, 4, 7, 16, 255, 256)]
          + [("delta4+x86", [(f.DELTA, 4), (f.BCJ["x86"], 1)]),
             ("x86+delta1+arm64", [(f.BCJ["x86"], 1), (f.DELTA, 1), (f.BCJ["arm64"], 1)]),
             ("delta256+delta1+delta3", [(f.DELTA, 256), (f.DELTA, 1), (f.DELTA, 3)])])


@pytest.mark.parametrize("name,chain", CHAINS, ids=[c[0] for c in CHAINS])
def test_decodes_own_streams_of_every_chain(enc, name, chain):
    import xz_amd
    data = _input(chain)
    if o.have_ref():
        # the case proves something only if every filter of the chain changes bytes
        cur = data
        for i, (fid, d) in enumerate(chain):
            nxt = f.ref_forward(cur, [(fid, d)])
            assert nxt != cur, (name, i)
            cur = nxt
    t = _cuda(data)
    for preset in (1, 6):
        for bs in (N // 3, _ragged_block_size(chain)):
            xz, _ = enc.encode(t, opts=_opts(preset, chain), block_size=bs)
            xz = xz.clone()
            nblocks = (N + bs - 1) // bs
            got, nb = enc.decode(xz, N + 16)
            assert nb == nblocks and o.first_diff(_bytes(got), data) == -1, (name, preset, bs)
            ver, nb2 = enc.decode(xz, N + 16, expected=t)
            assert nb2 == nblocks and o.first_diff(_bytes(ver), data) == -1, (name, preset, bs)
            bad = xz.clone()
            bad[xz.numel() // 2] ^= 0x40
            with pytest.raises(xz_amd.XzAmdError):
                enc.decode(bad, N + 16)
            other = t.clone()
            other[N // 3 + 5] ^= 1
            with pytest.raises(xz_amd.XzAmdError):
                enc.decode(xz, N + 16, expected=other)


@pytest.mark.parametrize("name,chain", CHAINS, ids=[c[0] for c in CHAINS])
def test_decodes_reference_streams_of_every_chain(enc, name, chain):
    """Streams of the real liblzma MT encoder (BT4) with the same chains."""
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    data = _input(chain)
    t = _cuda(data)
    for preset, bs in ((6, 150001), (1, 1 << 17)):
        if len(chain) == 1:
            raw = o.ref_encode_mt_chain(data, preset, chain[0][0], chain[0][1], threads=2, block_size=bs)
        else:
            raw = o.ref_encode_mt_chain_n(data, preset, chain, threads=2, block_size=bs)
        got, nb = enc.decode(_cuda(raw), N + 16)
        assert nb == (N + bs - 1) // bs and o.first_diff(_bytes(got), data) == -1, (name, preset)
        ver, _ = enc.decode(_cuda(raw), N + 16, expected=t)
        assert o.first_diff(_bytes(ver), data) == -1, (name, preset)


def _has_start_offset(raw):
    return any(4 <= fid <= 0x0B and len(props) == 4 and props != b"\0\0\0\0" for fid, props in f.block_filter_flags(raw))


def test_reference_fixture_files_with_chains(enc):
    """Every good file decodes to what the reference decoder gives, every other file is refused.  One limit of this
    decoder cuts through the good files: a BCJ filter with a non-zero start offset is declined with
    XZAMD_OPTIONS_ERROR (8) by design (good-1-arm64-lzma2-2.xz carries one); such a file must be declined, not
    mis-decoded -- found by reading its Block Header, not by its name."""
    import xz_amd
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    files = sorted(glob.glob(os.path.join(f.FIX, "*.xz")))
    ndec = ndeclined = nrefused = 0
    for p in files:
        raw = open(p, "rb").read()
        r, want = o.ref_decode(raw, 1 << 20)
        if os.path.basename(p).startswith("good-"):
            assert r == 1, p
            if _has_start_offset(raw):
                with pytest.raises(xz_amd.XzAmdError) as ei:
                    enc.decode(_cuda(raw), 1 << 20)
                assert "(8)" in str(ei.value), (p, str(ei.value))
                ndeclined += 1
                continue
            got, nb = enc.decode(_cuda(raw), 1 << 20)
            assert _bytes(got) == want, p
            ver, _ = enc.decode(_cuda(raw), 1 << 20, expected=_cuda(want))
            assert _bytes(ver) == want, p
            ndec += 1
        else:
            with pytest.raises(xz_amd.XzAmdError):
                enc.decode(_cuda(raw), 1 << 20)
            nrefused += 1
    assert ndec >= 4 and ndeclined <= 1 and nrefused >= 3


def test_x86_without_synchronisation_points(enc):
    """Inputs on which the chunk owners of the x86 inverse kernel find no synchronisation point, so that one thread
    walks the Block serially: 1 MiB of E8, 1 MiB of E8 00 00 00 00, corpus_x86 at its densest, and a Block boundary
    that cuts an instruction.  Device decode == reference decode of the same Stream, byte for byte.
    Sizes as the issue states them (1 MiB); seen on an MI355X, per decode: 1 MiB of E8 0.33 s,
    1 MiB of E8 00 00 00 00 1.4 s, the densest corpus 0.47 s, the cut instruction 0.37 s (all printed)."""
    import xz_amd
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    cut = bytearray(o.corpus_x86(300000, 9))
    cut[99998:100003] = bytes([0xE8, 0x10, 0x20, 0x00, 0x00])        # Block size 100000 cuts this CALL
    cases = {"all_e8": (bytes([0xE8]) * (1 << 20), 1 << 20), "e8_zero": (bytes([0xE8, 0, 0, 0, 0]) * ((1 << 20) // 5), 1 << 20),
             "densest": (o.corpus_x86(600000, 5, density=2), 1 << 20), "cut": (bytes(cut), 100000)}
    for name, (data, bs) in cases.items():
        for src in ("ref", "own"):
            if src == "ref":
                raw = o.ref_encode_mt_x86(data, 1, threads=2, block_size=bs)
            else:
                xz, _ = enc.encode(_cuda(data), opts=_opts(1, [(f.BCJ["x86"], 1)]), block_size=bs)
                raw = _bytes(xz)
            r, want = o.ref_decode(raw, len(data) + 16)
            assert r == 1 and want == data
            t0 = time.time()
            got, _ = enc.decode(_cuda(raw), len(data) + 16)
            print(f"x86 serial case {name}/{src}: {len(data)} B decoded in {time.time() - t0:.3f} s")
            assert o.first_diff(_bytes(got), want) == -1, (name, src)


def _stored_lzma2(data):
    """LZMA2 payload of uncompressed chunks (first one resets the dictionary)."""
    out, first = b"", True
    for i in range(0, len(data), 65536):
        c = data[i:i + 65536]
        out += bytes([1 if first else 2]) + (len(c) - 1).to_bytes(2, "big") + c
        first = False
    return out + b"\0"


@pytest.mark.parametrize("dist", [1, 3, 64, 255, 256])
def test_delta_against_arithmetic(enc, dist):
    """Random bytes (the scan, not the LZMA2 stage, carries the information), Block lengths around the distance and
    around the scan's tile.  The filtered bytes come from numpy (byte minus the byte dist before it; np.cumsum per
    residue class, uint8, gives the input back) and are put into a hand-made {delta, LZMA2} Stream of stored chunks:
    the device must return the input.  The same lengths as Blocks of the reference encoder's Streams and, from 4096
    bytes on (the encoder's smallest Block), of our own."""
    rng = np.random.default_rng(1000 + dist)
    for L in (1, dist - 1, dist, f.TILE - 1, f.TILE + 1, 3 * f.TILE + 5):
        if L <= 0:
            continue
        blk = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        filtered = f.np_delta_forward(blk, dist)
        assert f.np_delta_inverse(filtered, dist) == blk
        flags = bytes([3, 1, dist - 1, 0x21, 1, 0])
        s = f.single_block_stream(0, flags, 2, _stored_lzma2(filtered), b"", L)
        got, nb = enc.decode(_cuda(s), L + 16)
        assert nb == 1 and o.first_diff(_bytes(got), blk) == -1, (dist, L)
        data = rng.integers(0, 256, 2 * L + (L + 1) // 2, dtype=np.uint8).tobytes()      # Blocks of L, L and about L / 2
        t = _cuda(data)
        streams = []
        if o.have_ref():
            streams.append(o.ref_encode_mt_chain(data, 1, f.DELTA, dist, threads=1, block_size=L))
        if L >= 4096:
            xz, _ = enc.encode(t, opts=_opts(1, [(f.DELTA, dist)]), block_size=L)
            streams.append(_bytes(xz))
        for raw in streams:
            got, nb = enc.decode(_cuda(raw), len(data) + 16)
            assert nb == (len(data) + L - 1) // L and o.first_diff(_bytes(got), data) == -1, (dist, L)
            ver, _ = enc.decode(_cuda(raw), len(data) + 16, expected=t)
            assert o.first_diff(_bytes(ver), data) == -1, (dist, L)


def test_declined_not_misdecoded(enc):
    """Hand-made Block Headers around a good LZMA2 payload (CRC32s recomputed)."""
    import xz_amd
    data = o.corpus_x86(50000, 3)
    xz, _ = enc.encode(_cuda(data), opts=_opts(1, [(f.BCJ["x86"], 1)]), block_size=1 << 20)
    raw = _bytes(xz)
    check, flags, nf, payload, chk, usize = f.parse_single_block(raw)
    assert nf == 2 and flags[:2] == b"\x04\x00"
    lz2 = flags[2:]

    def code(stream):
        try:
            enc.decode(_cuda(stream), len(data) + 16)
        except xz_amd.XzAmdError as e:
            return int(str(e).split("(")[1].split(")")[0])
        return 0

    assert code(f.single_block_stream(check, flags, nf, payload, chk, usize)) == 0                    # the writer itself
    got, _ = enc.decode(_cuda(f.single_block_stream(check, b"\x04\x04\0\0\0\0" + lz2, 2, payload, chk, usize)), len(data) + 16)
    assert _bytes(got) == data                                                                        # offset 0 in size-4 properties
    assert code(f.single_block_stream(check, b"\x04\x04\x04\0\0\0" + lz2, 2, payload, chk, usize)) == 8      # start offset 4
    assert code(f.single_block_stream(check, b"\x0c\x00" + lz2, 2, payload, chk, usize)) == 8                # unknown id
    assert code(f.single_block_stream(check, lz2 + b"\x03\x01\x00", 2, payload, chk, usize)) == 8            # LZMA2 not last
    assert code(f.single_block_stream(check, flags, nf, payload, chk, usize, header_pad=b"\0\0\0\x01")) == 8
    s = f.single_block_stream(check, b"\x03\x02\x00\x00" + lz2, 2, payload, chk, usize)                      # delta, properties size 2
    mine = code(s)
    assert mine in (8, 9)
    if o.have_ref():
        r, _ = o.ref_decode(s, len(data) + 16)
        assert r in (8, 9) and r == mine
    # five filters cannot be written (two bits); four non-LZMA2 filters are a chain without LZMA2
    assert code(f.single_block_stream(check, b"\x03\x01\x00" * 4, 4, payload, chk, usize)) == 8


def test_plain_streams_allocate_and_launch_nothing_new(enc):
    import xz_amd
    data = o.corpus_mixed(300000, 2)
    t = _cuda(data)
    xz, _ = enc.encode(t, preset=1, block_size=1 << 17)
    xz = xz.clone()
    before = xz_amd.Encoder.debug_decode_counters()
    got, _ = enc.decode(xz, len(data) + 16)
    ver, _ = enc.decode(xz, len(data) + 16, expected=t)
    assert _bytes(got) == data and _bytes(ver) == data
    assert xz_amd.Encoder.debug_decode_counters() == before
    # ... and the counters do count: one temporary + one stage for {delta, LZMA2}; two + three for a chain of three;
    # a verification decode adds the filtered history and one forward launch per filter
    xz, _ = enc.encode(t, opts=_opts(1, [(f.DELTA, 2)]), block_size=1 << 17)
    enc.decode(xz.clone(), len(data) + 16)
    c1 = xz_amd.Encoder.debug_decode_counters()
    assert (c1[0] - before[0], c1[1] - before[1], c1[2] - before[2]) == (1, 1, 0)
    xz, _ = enc.encode(t, opts=_opts(1, [(f.DELTA, 2), (f.BCJ["arm"], 1), (f.BCJ["x86"], 1)]), block_size=1 << 17)
    enc.decode(xz.clone(), len(data) + 16, expected=t)
    c2 = xz_amd.Encoder.debug_decode_counters()
    assert (c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]) == (3, 3, 3)


def test_streams_that_mix_chains_from_block_to_block(enc):
    """A foreign Stream may change the chain from Block to Block: Blocks of our own Streams with different chains (and
    lengths) put behind one another, Index rebuilt."""
    import zlib
    rng = np.random.default_rng(5)
    pieces = [([], 70001), ([(f.DELTA, 3)], 40000), ([(f.BCJ["x86"], 1), (f.DELTA, 2)], 16384), ([], 5),
              ([(f.BCJ["arm64"], 1)], 33333), ([(f.DELTA, 256), (f.DELTA, 1), (f.BCJ["sparc"], 1)], 50001)]
    body, records, whole = b"", [], b""
    for chain, n in pieces:
        data = (o.corpus_x86(n, 3) if n % 2 else _arm64_like(n, 4))
        data = bytes(np.frombuffer(data, dtype=np.uint8) ^ rng.integers(0, 2, n, dtype=np.uint8))
        xz, _ = enc.encode(_cuda(data), opts=_opts(1, chain), block_size=1 << 20)
        raw = _bytes(xz)
        isz = (int.from_bytes(raw[-8:-4], "little") + 1) * 4
        block = raw[12: len(raw) - 12 - isz]
        idx = raw[len(raw) - 12 - isz: len(raw) - 12]
        unpadded, p = f._vli_get(idx, 2)
        body += block
        records.append((unpadded, n))
        whole += data
    idx = b"\0" + f.vli(len(records)) + b"".join(f.vli(u) + f.vli(n) for u, n in records)
    idx += b"\0" * ((-len(idx)) % 4)
    idx += zlib.crc32(idx).to_bytes(4, "little")
    sflags = bytes([0, 4])
    foot = (len(idx) // 4 - 1).to_bytes(4, "little") + sflags
    stream = b"\xfd7zXZ\0" + sflags + zlib.crc32(sflags).to_bytes(4, "little") + body + idx + zlib.crc32(foot).to_bytes(4, "little") + foot + b"YZ"
    if o.have_ref():
        r, want = o.ref_decode(stream, len(whole) + 16)
        assert r == 1 and want == whole
    got, nb = enc.decode(_cuda(stream), len(whole) + 16)
    assert nb == len(pieces) and o.first_diff(_bytes(got), whole) == -1
    ver, _ = enc.decode(_cuda(stream), len(whole) + 16, expected=_cuda(whole))
    assert o.first_diff(_bytes(ver), whole) == -1
