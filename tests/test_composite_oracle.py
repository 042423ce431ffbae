"""The oracle over the composite Blocks of tests/_composite.py, on the CPU.

The parity tests pin the device to the oracle; this pins the oracle's design to two judges that share no code with it:
the chunk walker of tests/_lzma2_grammar.py and the reference decoder.  Every Block of every Stream must be either
  * valid: the walker's rules (a) and (b) hold, and the reference decodes the Stream to the input; or
  * the known stored-prefix defect (first LZMA chunk 0xA0 behind stored chunks only), and then the
    reference rejects the Stream.
The second branch cannot hide a failure: which Blocks of the named inputs show the defect is recorded in
_composite.EXPECTED_DEFECT and compared for equality, at least three named Blocks must show it, and at most 6 of the 60
random draws may.

Measured when this was written (oracle alone): 30 named inputs x 6 settings x 2 Block sizes = 360 Streams, 24 of them
with one defect Block (p6 5, p9e 5, p4 4, p6-stress 10, p1 / p3 0; all at Blocks of 1 MiB), no other invalid Block.
Random draws: seeds 1..240 gave 4 defect draws (85, 111, 132, 171); the 60 seeds used here, 61..120, hold two of them.

The oracle runs at about 1 MiB/s and a core, so the Streams are made once, by a few worker processes.
"""
import concurrent.futures as cf
import multiprocessing
import os

import pytest

import _composite as cp
import _lzma2_grammar as g
import _oracle as o

DRAW_SEEDS = tuple(range(61, 121))
DRAW_DEFECT_CAP = 6


def _draw_plan(seed):
    """setting and Block size of a random draw: all twelve combinations in turn"""
    return cp.SETTINGS[seed % len(cp.SETTINGS)], cp.BLOCK_SIZES[seed // len(cp.SETTINGS) % len(cp.BLOCK_SIZES)]


def _judge(job):
    """(walker verdict per Block, the reference decoder returned the input) of one oracle Stream"""
    kind, key, setting, bs = job
    data = cp.named(key) if kind == "named" else cp.draw(key)
    prm = o.params_for_gpu_options(cp.options_for(setting))
    xz = o.orc_xz_stream(data, prm, bs)
    rr, dec = o.ref_decode(xz, len(data) + 16)
    return g.verdicts(xz), (rr == 1 and dec == data), rr


@pytest.fixture(scope="module")
def judged():
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    o.orc()
    jobs = [("named", n, s, bs) for n in cp.NAMED for s in cp.SETTINGS for bs in cp.BLOCK_SIZES]
    jobs += [("draw", seed) + _draw_plan(seed) for seed in DRAW_SEEDS]
    workers = max(1, min(8, len(os.sched_getaffinity(0))))
    with cf.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("fork")) as ex:
        return dict(zip(jobs, ex.map(_judge, jobs, chunksize=2)))


def _check(job, res):
    """valid, or exactly the known shape and rejected: anything else fails"""
    verdicts, decoded, rr = res
    assert g.INVALID not in verdicts, (job, verdicts)
    if g.DEFECT in verdicts:
        assert not decoded and rr == 9, (job, verdicts, rr)          # LZMA_DATA_ERROR
    else:
        assert decoded, (job, verdicts, rr)


def test_named_blocks_are_valid_or_the_recorded_defect(judged):
    shown = 0
    per_setting = {}
    for job, res in judged.items():
        if job[0] != "named":
            continue
        _, name, setting, bs = job
        _check(job, res)
        bad = tuple(k for k, v in enumerate(res[0]) if v == g.DEFECT)
        assert len(res[0]) == (len(cp.named(name)) + bs - 1) // bs
        assert bad == cp.expected_defect(setting, bs, name), (job, res[0])
        shown += len(bad)
        per_setting[setting] = per_setting.get(setting, 0) + len(bad)
    print("defect Blocks per setting", per_setting)
    assert shown >= 3


def test_the_record_names_only_inputs_and_settings_that_exist():
    assert set(cp.EXPECTED_DEFECT) == set(cp.SETTINGS)
    for per_bs in cp.EXPECTED_DEFECT.values():
        assert set(per_bs) == set(cp.BLOCK_SIZES)
        for names in per_bs.values():
            assert set(names) <= set(cp.NAMED)


def test_random_draws_are_valid_or_the_defect_within_the_cap(judged):
    defect = []
    for job, res in judged.items():
        if job[0] != "draw":
            continue
        _check(job, res)
        if g.DEFECT in res[0]:
            defect.append((job[1], job[2], job[3], cp.describe(cp.draw_segments(job[1]))))
    print("defect draws", defect)
    assert len(DRAW_SEEDS) == 60 and len(defect) <= DRAW_DEFECT_CAP


def test_generator_is_deterministic_and_within_its_bounds():
    assert 24 <= len(cp.NAMED) and all(len(cp.named(n)) < 3 * cp.MIB // 2 for n in cp.NAMED)
    for seed in (1, 61, 120):
        segs = cp.draw_segments(seed)
        assert 1 <= len(segs) <= 6 and all(s[1] in cp.LENGTHS for s in segs)
        assert cp.draw(seed) == cp.build(segs) and len(cp.draw(seed)) == sum(s[1] for s in segs)
    assert cp.draw(61) != cp.draw(62)
    used = {s[0] for seed in DRAW_SEEDS for s in cp.draw_segments(seed)}
    assert used == set(cp.KINDS)
