"""The structure build of batch i + 1 issued ahead, under the parse of batch i (XZAMD_BUILD_AHEAD, DESIGN.md 3.5 "Build
ahead"): for every start point the Stream equals the one of the serial schedule (knob at 0) byte for byte, and the system's
liblzma (the `lzma` module) decodes it to the input.

Shape: Blocks of 256 KiB and batches of 1 MiB (XZAMD_BATCH_MIB=1), i.e. four Blocks per batch; the Block size is above
XZAMD_SEED_LEN + 1024, so the seed pieces run on the third stream, behind the build that now shares it.  The encode with the knob
at 0 comes first and leaves every buffer at its size, so the encodes behind it issue every batch but the first ahead
(stats().batches_ahead says so).  That reference Stream is made once per case and shared by the start points.  The order of
the launches itself is checked on the CPU (test_host_build_ahead.py)."""
import functools
import lzma
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BS = 256 << 10
MIB = 1 << 20
KNOBS = ("plan", "part", "iter1")
SHA256 = 10


def _make_encoder(limit_mib=None):
    import xz_amd
    saved = {k: os.environ.get(k) for k in ("XZAMD_BATCH_MIB", "XZAMD_TEST_ALLOC_LIMIT_MIB")}
    os.environ["XZAMD_BATCH_MIB"] = "1"
    if limit_mib is not None:
        os.environ["XZAMD_TEST_ALLOC_LIMIT_MIB"] = str(limit_mib)
    else:
        os.environ.pop("XZAMD_TEST_ALLOC_LIMIT_MIB", None)
    try:
        return xz_amd.Encoder()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def enc():
    e = _make_encoder()
    yield e
    e.close()


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _encode(enc, monkeypatch, knob, t, **kw):
    monkeypatch.setenv("XZAMD_BUILD_AHEAD", knob)
    out, _ = enc.encode(t, block_size=BS, **kw)
    st = enc.stats()
    return out.cpu().numpy().tobytes(), st.batches, st.batches_ahead


@functools.lru_cache(maxsize=None)
def _corpus():
    import xz_amd
    return xz_amd.corpus_text(3 * MIB, seed=7).tobytes()


def _text(n):
    return _corpus()[:n]


def _opcode_clusters(n):
    """quiet bytes with clusters of CALL / JMP opcodes, small and sign-extended displacements: the x86 filter converts many"""
    rng = np.random.default_rng(5)
    data = rng.integers(0, 24, n, dtype=np.uint8)
    at = rng.integers(0, n - 64, n // 400)
    for j in range(4):
        data[at + 5 * j] = np.where(rng.integers(0, 2, at.size) == 1, 0xE8, 0xE9)
        data[at + 5 * j + 4] = np.where(rng.integers(0, 2, at.size) == 1, 0x00, 0xFF)
    return data.tobytes()


def _int32_walk(n):
    rng = np.random.default_rng(11)
    return ((1 << 28) + np.cumsum(rng.integers(-1000, 1001, n // 4, dtype=np.int64))).astype("<u4").tobytes()


def _bcj_opts():
    import xz_amd
    opts = xz_amd.preset_options(6)
    opts.bcj = 4
    return opts


RAGGED = 2 * MIB + 300001
# name: (input, batches, batches a start point issues ahead, arguments of encode)
CASES = {
    "three_full_batches": (lambda: _text(3 * MIB), 3, 2, lambda: {}),
    "ragged_last_batch_and_block": (lambda: _text(RAGGED), 3, 2, lambda: {}),
    # five Blocks, the last one a single byte; the batch loop deals them evenly: 3 + 2
    "one_byte_block_in_the_second_batch": (lambda: _text(MIB + 1), 2, 1, lambda: {}),
    "x86_bcj_filtered_copy_by_parity": (lambda: _opcode_clusters(RAGGED), 3, 2, lambda: {"opts": _bcj_opts()}),
    "auto_delta_on_an_int32_walk": (lambda: _int32_walk(RAGGED - 1), 3, 2, lambda: {"auto_delta": True}),
    "check_sha256": (lambda: _text(RAGGED), 3, 2, lambda: {"check": SHA256}),
    "verified_encode": (lambda: _text(RAGGED), 3, 2, lambda: {"verify": True}),
    "single_phase_preset": (lambda: _text(RAGGED), 3, 0, lambda: {"preset": 1}),
}
_reference = {}


def _serial(enc, monkeypatch, name):
    """the case's input on the device and its Stream with the knob at 0, checked once: the batches, nothing ahead, the
    system's decoder; this encode also brings every buffer of the case to its size"""
    if name not in _reference:
        make, nbatches, _, kw = CASES[name]
        data = make()
        t = _cuda(data)
        base, nb, na = _encode(enc, monkeypatch, "0", t, **kw())
        assert (nb, na) == (nbatches, 0)
        assert lzma.decompress(base, format=lzma.FORMAT_XZ) == data
        _reference[name] = (t, base)
    return _reference[name]


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", list(CASES))
def test_same_stream_as_the_serial_schedule(enc, monkeypatch, name, knob):
    for k in ("XZAMD_NO_OVERLAP", "XZAMD_BACK_BESIDE_BUILD"):
        monkeypatch.delenv(k, raising=False)
    _, nbatches, ahead, kw = CASES[name]
    t, base = _serial(enc, monkeypatch, name)
    got, nb, na = _encode(enc, monkeypatch, knob, t, **kw())
    assert (nb, na) == (nbatches, ahead), (nb, na)
    assert got == base, f"XZAMD_BUILD_AHEAD={knob}: the Stream differs from the serial schedule's"


def test_the_filter_cases_filter(enc):
    """(what keeps the two filter cases from passing vacuously) the x86 filter changes Blocks of its input, and the device picks
    a delta filter for the walk"""
    import _checks as ck
    data = _opcode_clusters(RAGGED)
    changed = sum(ck.sys_forward(data[at: at + BS], [(4, 0)]) != data[at: at + BS] for at in range(0, len(data), BS))
    assert changed >= 8
    assert all(d == 4 for d in enc.choose_delta(_cuda(_int32_walk(RAGGED - 1)), BS)[:-1])


@pytest.mark.parametrize("knob", KNOBS)
def test_two_calls_of_different_sizes(enc, monkeypatch, knob):
    """nothing of a call's last build ahead survives the call: a job of three batches, then one of two on the same context,
    each against the serial schedule of its own size (the next start point's first call is the way back up)"""
    t3, want3 = _serial(enc, monkeypatch, "three_full_batches")
    t1, want1 = _serial(enc, monkeypatch, "one_byte_block_in_the_second_batch")
    got3, nb, na = _encode(enc, monkeypatch, knob, t3)
    assert got3 == want3 and (nb, na) == (3, 2)
    got1, nb, na = _encode(enc, monkeypatch, knob, t1)
    assert got1 == want1 and (nb, na) == (2, 1)


@pytest.fixture(scope="module")
def limited():
    """A context whose first batch (1 MiB: 32 MiB of match lists) does not fit under a limit of 20 MiB: every call tries it,
    releases the buffers and goes on in batches of two Blocks"""
    e = _make_encoder(limit_mib=20)
    yield e
    e.close()


@pytest.mark.parametrize("knob", KNOBS)
def test_allocation_limit_path(limited, monkeypatch, knob):
    """the two batches that allocate are serial, the two behind them are issued ahead; the Stream is the serial schedule's"""
    if "limited" not in _reference:
        data = _text(2 * MIB)
        t = _cuda(data)
        base, nb, na = _encode(limited, monkeypatch, "0", t)
        assert (nb, na) == (4, 0)
        assert lzma.decompress(base, format=lzma.FORMAT_XZ) == data
        _reference["limited"] = (t, base)
    t, base = _reference["limited"]
    got, nb, na = _encode(limited, monkeypatch, knob, t)
    assert (nb, na) == (4, 2) and got == base, (nb, na)
