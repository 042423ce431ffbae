"""The parse kernel is one instance per stage (SEED, PART_PRIOR, PART_SNAP, FULL) and list format (packed / unpacked):
every instance against the oracle, and the Block lengths at which the stages' branches switch.

Options as in test_two_phase_stages_identical_to_oracle: span_cost 50000, span_bits 0, enc_span_bits 300000 (many
pieces and several encode spans per Block).  part_iters = 1 runs SEED, PART_PRIOR, FULL; part_iters = 2 adds PART_SNAP.
The oracle side of a case is computed once per module and shared."""
import functools

import numpy as np
import pytest

import _oracle as o

pytestmark = pytest.mark.gpu

SEED_LEN, PREROLL = 65536, 2048
MIN_EARLY_SEED_BLOCK = SEED_LEN + 2 * 256            # XZAMD_SEED_LEN + 2 x FIND_RUN: the smallest Block size of the early-seed path
# second-Block lengths: the seed piece is the whole Block (<= 65,536); one byte behind the seed; a piece behind the seed
# ends at / one byte behind the pre-roll length (every piece behind the seed has a pre-roll, none of these a warm-up walk:
# that needs piece start - Block start > 65,536 + 2,048); the shortest Block in which a piece can start there; 1 byte
SECOND_BLOCK_LENGTHS = [SEED_LEN - 1, SEED_LEN, SEED_LEN + 1, SEED_LEN + PREROLL, SEED_LEN + PREROLL + 1,
                        2 * SEED_LEN + PREROLL + 1, 1]


@pytest.fixture(scope="module")
def enc():
    import torch
    import xz_amd
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    e = xz_amd.Encoder(0)
    yield e
    e.close()


def gpu_encode(enc, data, opts, block_size):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out, _ = enc.encode(t, opts=opts, block_size=block_size)
    return out.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def mixed_corpus():
    """The corpus of test_two_phase_stages_identical_to_oracle: text, lorem, zeros, random bytes, a repeated page, tar."""
    import xz_amd
    rng = np.random.default_rng(7)
    lorem = o.corpus_lorem(900000)
    return (xz_amd.corpus_text(1500000, seed=3).tobytes() + lorem[:700000] + b"\0" * 300000
            + bytes(rng.integers(0, 256, size=150000, dtype=np.uint8)) + (lorem[:3000] * 150) + xz_amd.corpus_tar(1200000).tobytes())


def options(preset, part_iters):
    import xz_amd
    opts = xz_amd.preset_options(preset)
    opts.span_cost = 50000
    opts.span_bits = 0
    opts.enc_span_bits = 300000
    opts.part_iters = part_iters
    return opts


@functools.lru_cache(maxsize=None)
def oracle_payload(preset, part_iters, start, length):
    """The oracle's payload of one Block (Blocks are independent: a Block several cases share is encoded once)."""
    prm = o.params_for_gpu_options(options(preset, part_iters))
    assert prm.enc_bits == 300000 and prm.part_iters == part_iters
    return o.orc_encode_block(mixed_corpus()[start:start + length], prm)


def oracle_stream(preset, part_iters, start, length, bs):
    prm = o.params_for_gpu_options(options(preset, part_iters))
    pay = [oracle_payload(preset, part_iters, start + i, min(bs, length - i)) for i in range(0, length, bs)]
    return o.orc_xz_stream(mixed_corpus()[start:start + length], prm, bs, payloads=pay)


def _walk_symbols(sl, sd, gsl, gsd, n):
    """First symbol start at which the recorded parses differ (None: identical)."""
    p = 0
    while p < n:
        if sl[p] != gsl[p] or sd[p] != gsd[p]:
            return p
        p += max(1, int(sl[p]) & 0x7FFF)           # bit 15 = "coded as a match" flag
    return None


MATRIX_START, MATRIX_LEN, MATRIX_BS = 1000000, (5 << 19) + 12345, 1 << 20      # 2.5 MiB + a ragged last Block


@pytest.mark.parametrize("part_iters", [1, 2])
@pytest.mark.parametrize("preset,packed", [(6, True), (7, False)])
def test_every_instance_identical_to_oracle(enc, preset, packed, part_iters):
    """Dispatch matrix: both list formats (preset 6: 8 MiB dictionary, packed records; preset 7: 16 MiB, unpacked) x
    part_iters 1 and 2.  The Stream equals the oracle's and decodes through the reference decoder; the recorded symbols
    of the middle Block (lorem, zero pages, random bytes, a repeated page) equal the oracle's parse."""
    opts = options(preset, part_iters)
    assert (opts.dict_size <= (1 << 23)) == packed
    data = mixed_corpus()[MATRIX_START:MATRIX_START + MATRIX_LEN]
    bs = MATRIX_BS
    want = oracle_stream(preset, part_iters, MATRIX_START, MATRIX_LEN, bs)
    got = gpu_encode(enc, data, opts, bs)
    gsl = enc.debug_fetch(9, len(data), "uint16")
    gsd = enc.debug_fetch(10, len(data), "uint32")
    assert o.first_diff(got, want) == -1, (preset, part_iters)
    rr, rdec = o.ref_decode(got, len(data) + 16)
    assert rr == 1 and rdec == data
    b = 1
    blk = data[b * bs:(b + 1) * bs]
    sl, sd = o.orc_parse_dump(blk, o.params_for_gpu_options(opts))
    bad = _walk_symbols(sl, sd, gsl[b * bs:b * bs + len(blk)], gsd[b * bs:b * bs + len(blk)], len(blk))
    assert bad is None, ("symbol records", b, bad)


def _length_cases():
    # a second Block cannot be longer than the Block size: the smallest size takes the lengths that fit in it
    return [(bs, n) for bs in (MIN_EARLY_SEED_BLOCK, 1 << 20) for n in SECOND_BLOCK_LENGTHS if n <= bs]


@pytest.mark.parametrize("bs,second", _length_cases())
def test_stage_branch_lengths_identical_to_oracle(enc, bs, second):
    """Two Blocks, the second of a length at which a stage's branches switch: the seed piece is the whole Block, a piece
    with a pre-roll but no warm-up walk, the first piece that takes the walk, a 1-byte Block.  Block sizes: the smallest
    the early-seed path accepts and 1 MiB.  With part_iters 1 and 2 (every stage)."""
    start = 200000
    n = bs + second
    data = mixed_corpus()[start:start + n]
    for part_iters in (1, 2):
        want = oracle_stream(6, part_iters, start, n, bs)
        got = gpu_encode(enc, data, options(6, part_iters), bs)
        assert o.first_diff(got, want) == -1, (bs, second, part_iters)
        rr, rdec = o.ref_decode(got, n + 16)
        assert rr == 1 and rdec == data
