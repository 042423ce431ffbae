"""The Pareto filter of k_find_sn (a sort of the 16 candidates of a position inside their DPP row, a prefix maximum, a
population count) against the oracle's find_sn: every 32-byte match-list record of inputs made to stress the filter,
and the whole Stream for the unpacked list format, which orc_list_dump does not speak.  Every input is at most 300 KB."""
import numpy as np
import pytest

import _oracle as o
from test_gpu_parity import gpu_encode

LADDER_STEPS = (40, 33, 27, 22, 18, 14, 11, 9, 7, 5, 4, 3, 2)


def ladder():
    """400 rounds of: the prefixes of a random 48-letter phrase of 40 .. 2 bytes, each followed by 3 random bytes, then
    the whole phrase.  A position inside the phrase sees the longer prefixes further back and the shorter ones nearer:
    more survivors than LIST_K, the nearest one the shortest."""
    rng = np.random.default_rng(1)
    phrase = rng.integers(97, 123, size=48, dtype=np.uint8)
    out = []
    for _ in range(400):
        for k in LADDER_STEPS:
            out.append(phrase[:k])
            out.append(rng.integers(0, 256, size=3, dtype=np.uint8))
        out.append(phrase)
    data = np.concatenate(out).tobytes()
    assert len(data) == 112800
    return data


def same_position():
    """The suffix neighbour and the 8-, 16-, 24- and 32-byte heads all name one position."""
    rng = np.random.default_rng(2)
    return bytes(rng.integers(0, 256, size=5000, dtype=np.uint8)) * 20


def short_matches():
    """hash2 candidates of length 2-3 beside lanes whose minimum is 4."""
    rng = np.random.default_rng(3)
    return bytes(rng.integers(0, 16, size=100000, dtype=np.uint8))


def edge_pairs():
    """32-byte strings repeated at a distance of exactly 4096 (eligible with dict_size 4096) and of 4097 (not eligible)
    between random bytes: the 60 KB of the ladder alone hold no match at the distance of the dictionary size itself."""
    rng = np.random.default_rng(4)
    rnd = lambda k: rng.integers(0, 256, size=k, dtype=np.uint8)
    out = []
    for _ in range(6):
        a, b = rnd(32), rnd(32)
        out += [a, rnd(4096 - 32), a, rnd(1), b, rnd(4097 - 32), b]
    return np.concatenate(out).tobytes()


def _opts(preset=6, dict_size=None):
    import xz_amd
    opts = xz_amd.preset_options(preset)
    if dict_size is not None:
        opts.dict_size = dict_size
    return opts


_want = {}


def oracle_lists(name, data, opts, bs):
    """The oracle's records of every Block, computed once per (input, options, Block size) and shared."""
    key = (name, opts.dict_size, opts.gpu_nice_len, opts.gpu_sa_depth, bs)
    if key not in _want:
        prm = o.params_for_gpu_options(opts)
        w = np.concatenate([o.orc_list_dump(data[b0:b0 + bs], prm) for b0 in range(0, len(data), bs)])
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def test_ladder_fills_the_lists():
    """The ladder's condition, on the oracle's lists alone: at least 1,000 positions with LIST_K = 7 entries (measured:
    3,515 at the preset-6 options, 4,224 with nice_len 273 and the 256-byte suffix order)."""
    data = ladder()
    for preset in (6, 9 | 0x80000000):
        opts = _opts(preset, dict_size=1 << 23)                      # (orc_list_dump speaks the packed format)
        full = int(((oracle_lists("ladder", data, opts, 1 << 20)[:, 7] & 0xFF) == 7).sum())
        print("ladder, preset", hex(preset), "positions with 7 entries:", full)
        assert full >= 1000, (hex(preset), full)


def test_dictionary_edge_is_reached():
    """dict_size 4096 on edge_pairs: entries at the distance of the dictionary size itself, none beyond."""
    want = oracle_lists("edge_pairs", edge_pairs(), _opts(6, dict_size=4096), 1 << 20)
    cnt = want[:, 7] & 0xFF
    d1 = np.concatenate([want[cnt > k, k] & 0x7FFFFF for k in range(7)])
    print("dictionary edge: entries at distance 4096:", int((d1 == 4095).sum()), "largest distance", int(d1.max()) + 1)
    assert d1.max() == 4095 and (d1 == 4095).sum() >= 100


@pytest.fixture(scope="module")
def enc():
    import torch
    import xz_amd
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    e = xz_amd.Encoder(0)
    yield e
    e.close()


def check_lists(enc, name, data, opts, bs):
    gpu_encode(enc, data, opts, bs)
    n = len(data)
    got = enc.debug_fetch(3, 8 * n).reshape(n, 8).copy()
    want = oracle_lists(name, data, opts, bs)
    cnt = got[:, 7] & 0xFF
    for k in range(7):
        got[cnt <= k, k] = 0                    # entries past the count are undefined on the device
    bad = np.nonzero((got != want).any(axis=1))[0]
    bad = bad[bad % bs != 0]                    # position 0 of a Block: no earlier data, never read by the parser
    assert len(bad) == 0, (name, bs, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", [("ladder", ladder), ("same_position", same_position), ("short", short_matches)])
def test_records_identical_to_oracle(enc, name, make):
    check_lists(enc, name, make(), _opts(6), 1 << 20)


@pytest.mark.gpu
def test_records_with_nice_273_identical_to_oracle(enc):
    """nice_len 273 and the 256-byte suffix order of preset 9e, in the packed format: the > nice_len extension and len2
    are taken from the lane that holds the sorted entry, not from the lane that fetched the candidate."""
    check_lists(enc, "ladder", ladder(), _opts(9 | 0x80000000, dict_size=1 << 23), 1 << 20)


@pytest.mark.gpu
def test_records_at_the_dictionary_edge_identical_to_oracle(enc):
    """dict_size 4096 on 60 KB of the ladder, and on edge_pairs, which has matches at a distance of exactly 4096 (eligible)
    and of 4097 (not)."""
    check_lists(enc, "ladder60k", ladder()[:60000], _opts(6, dict_size=4096), 1 << 20)
    check_lists(enc, "edge_pairs", edge_pairs(), _opts(6, dict_size=4096), 1 << 20)


@pytest.mark.gpu
@pytest.mark.parametrize("bs", [65536, 100000])
def test_records_across_block_ends_identical_to_oracle(enc, bs):
    """Several Blocks, a ragged last one, an input length (112,800) that is no multiple of the 256 positions of a run;
    with 100,000-byte Blocks a run and a row of 64 positions straddle a Block end."""
    data = ladder()
    assert len(data) % 256 and len(data) % bs and (bs % 256 == 0 or bs % 64)
    check_lists(enc, "ladder", data, _opts(6), bs)
    check_lists(enc, "same_position", same_position(), _opts(6), bs)


@pytest.mark.gpu
@pytest.mark.parametrize("preset,dict_size", [(6, 1 << 24), (9 | 0x80000000, None)])
def test_unpacked_lists_whole_stream_identical_to_oracle(enc, preset, dict_size):
    """Dictionaries above 8 MiB: entries are distance - 1 with the lengths in the u16 side array, and the row sort runs
    on (distance, length) pairs.  The whole Stream against the oracle's, then through the reference decoder."""
    data = ladder()
    opts = _opts(preset, dict_size)
    assert opts.dict_size > 1 << 23
    for bs in (1 << 20, 100000):
        got, _ = gpu_encode(enc, data, opts, bs)
        want = o.orc_xz_stream(data, o.params_for_gpu_options(opts, span_cost_used=enc.stats().span_cost_used), bs)
        assert o.first_diff(got, want) == -1, (hex(preset), bs)
        if o.have_ref():
            rr, rdec = o.ref_decode(got, len(data) + 16)
            assert rr == 1 and rdec == data
