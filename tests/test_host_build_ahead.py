"""The batch loop with the structure build of batch i + 1 issued ahead (XZAMD_BUILD_AHEAD; xz_amd/csrc/xzamd_host.c,
DESIGN.md 3.5 "Build ahead") without a GPU.  tests/host_stub/driver_build_ahead.c runs the real host code over the CPU
stand-ins of the kernel layer; tests/host_stub/stub_xzk_log.c (linked in through the linker's --wrap) prints every
kernel-layer call with the stream it is enqueued on, stream waits, event records and host synchronisations included.  The
program is built with -fsanitize=address,undefined and run as a program.

The checker below turns the log of one encode into a happens-before graph -- order on a stream, event record -> the
stream waits on that event that follow, and a host synchronisation of a stream -> everything the host enqueues later -- and
asserts, for a job of four batches and every start point:
  * the filters and the build of batch i + 1 come after the finder and the plan of batch i (the structure, the sorts'
    scratch, the histograms) and after every reader of the filtered copy of batch i - 1 (the same buffer: one per parity);
  * the finder of batch i + 1 comes after its build;
  * the coder of batch i comes after EV_CHAINS of batch i + 1 and after EV_FRONT of batch i;
  * every stage event is recorded once per batch;
  * the build starts behind the event the knob names;
  * with the knob at 0 nothing of the build leaves the caller's stream;
and for the fallbacks -- a context that has to allocate, the forced allocation limit, a single-phase preset -- that
nothing is issued ahead there.  Every Stream equals the one of the knob at 0 and (chain {LZMA2}) decodes through the oracle.

Two limits of this checker.  The log carries no event names, so EV_CHAINS and EV_FRONT of a batch are found by position: the
record that follows the build on its stream, and the second record on the caller's stream behind the full parse launch (EV_PARSE,
then EV_FRONT, as front_parse records them); a change of that order has to be followed here.  And the stand-in build is
synchronous, so the host synchronisation INSIDE the real build is not in the graph: that build_sa_doubling (lzma_build.hip)
synchronises only the stream it is given -- the side stream of a build ahead -- is established by reading it, not by this test."""
import os
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ("xzamd_host.c", "xzamd_frame.c", "xzamd_options.c", "xzamd_stream.c", "corpus.c", "xzamd_framing.c", "xzamd_decode.c", "xzamd_file.c",
        "xzamd_repair.c", "xzamd_repair_plan.c", "xzamd_chains.c")
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in CSRC] + \
      [os.path.join(ROOT, "tests", "host_stub", f) for f in ("stub_xzk.c", "stub_xzk_dec.c", "stub_xzk_chains.c", "stub_xzk_delta.c",
                                                             "stub_xzk_log.c", "driver_build_ahead.c")] + \
      [os.path.join(ROOT, "oracle", f) for f in ("lzma2_dec.c", "xz_container.c", "lzma_fast_enc.c")]
WRAPPED = ("stream_wait_event", "event_record", "sync", "build_chains", "find_matches", "span_plan", "span_encode", "parse_pieces",
           "model_snapshots", "encode_syms", "assemble", "delta_stats", "delta_choose", "delta_blocks", "dec_units")
WRITERS = ("delta_stats", "delta_choose", "delta_blocks", "build")
PARSE = ("parse_part", "snapshots", "parse_full")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """{(case, knob): (ops, end)} of one run of the driver; ops = [(kind, stream, arg, ...)], end = the figures of its end line"""
    exe = str(tmp_path_factory.mktemp("build_ahead") / "driver_build_ahead")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *SRC,
                    *["-Wl,--wrap=xzk_" + w for w in WRAPPED], "-lm", "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k in ("LD_PRELOAD", "XZAMD_BATCH_MIB", "XZAMD_AUTO_DELTA", "XZAMD_NO_OVERLAP", "XZAMD_BUILD_AHEAD", "XZAMD_BUILD_AHEAD_STREAM",
              "XZAMD_BACK_BESIDE_BUILD", "XZAMD_TEST_ALLOC_LIMIT_MIB", "DRIVER_ALLOC_LIMIT_MIB"):
        env.pop(k, None)
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "driver_build_ahead: ok" in p.stdout, (p.stdout[-4000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
    out, cur, ops = {}, None, []
    for line in p.stdout.splitlines():
        w = line.split()
        if w[:1] == ["case"]:
            cur, ops = (w[1], w[2]), []
        elif w[:1] == ["op"]:
            ops.append(tuple(w[1:]))
        elif w[:1] == ["end"]:
            out[cur] = (ops, [int(x) for x in w[1:]])
    return out


class Graph:
    """happens-before over the log of one encode"""

    def __init__(self, ops):
        self.ops = ops
        self.anc = []                      # bit j of anc[i]: op j happens before op i
        last_on, last_rec, last_sync = {}, {}, None
        for i, op in enumerate(ops):
            kind, st = op[0], op[1]
            preds = []
            if st in last_on:
                preds.append(last_on[st])
            if last_sync is not None:
                preds.append(last_sync)
            if kind == "wait" and op[2] in last_rec:
                preds.append(last_rec[op[2]])
            m = 0
            for q in preds:
                m |= self.anc[q] | (1 << q)
            self.anc.append(m)
            if kind == "sync":
                last_sync = i              # (it has the stream's last op among its predecessors; later ops have it among theirs)
            else:
                last_on[st] = i
            if kind == "record":
                last_rec[op[2]] = i

    def before(self, a, b):
        return bool(self.anc[b] >> a & 1)

    def idx(self, *kinds):
        return [i for i, op in enumerate(self.ops) if op[0] in kinds]


def batches_of(g):
    """the ops of every batch, by kind: the k-th build, plan, coder ... is batch k's; finder launches lie between two builds
    in the log (ahead or not), parse launches between two plans"""
    builds, plans = g.idx("build"), g.idx("plan")
    nb = len(builds)
    assert nb == len(plans) == len(g.idx("code")) == len(g.idx("gather"))
    B = []
    for k in range(nb):
        hi_b = builds[k + 1] if k + 1 < nb else len(g.ops)
        hi_p = plans[k + 1] if k + 1 < nb else len(g.ops)
        b = {"build": [builds[k]], "plan": [plans[k]], "code": [g.idx("code")[k]],
             "find": [i for i in g.idx("find") if builds[k] < i < hi_b],
             "parse": [i for i in g.idx(*PARSE) if plans[k] < i < hi_p]}
        for kind in ("seeds", "delta_stats", "delta_choose", "delta_blocks"):
            all_ = g.idx(kind)
            assert len(all_) in (0, nb), kind
            b[kind] = [all_[k]] if all_ else []
        assert b["find"] and b["parse"] and g.ops[b["parse"][-1]][0] == "parse_full"
        B.append(b)
    return B


def check_order(ops, knob, ahead_from):
    """ahead_from: the first batch whose build must be on the side stream (None: none is)"""
    g = Graph(ops)
    B = batches_of(g)
    caller = g.ops[B[0]["find"][-1]][1]
    for k, b in enumerate(B):
        writers = [i for kind in WRITERS for i in b[kind]]
        side = {g.ops[i][1] for i in writers} - {caller}
        if ahead_from is None or k < ahead_from:
            assert not side, f"batch {k}: build or filters off the caller's stream ({knob})"
        else:
            assert len(side) == 1 and all(g.ops[i][1] != caller for i in writers), f"batch {k} was not issued ahead ({knob})"
        for f in b["find"]:
            assert g.before(b["build"][0], f), f"finder of batch {k} not behind its build"
        assert all(i < b["parse"][-1] for i in b["find"] + b["plan"])
        if k >= 1:
            p = B[k - 1]
            for w in writers:
                for r in p["find"] + p["plan"] + p["delta_choose"]:
                    assert g.before(r, w), f"batch {k}: {g.ops[w][0]} not behind {g.ops[r][0]} of batch {k - 1} ({knob})"
            # the coder of the batch before: behind this batch's EV_CHAINS (the record that follows the build on its stream)
            # and behind its own EV_FRONT (the second record on the caller's stream behind the full parse: EV_PARSE, EV_FRONT)
            ev_chains = b["build"][0] + 1
            assert g.ops[ev_chains][0] == "record" and g.ops[ev_chains][1] == g.ops[b["build"][0]][1]
            recs = [i for i in g.idx("record") if i > p["parse"][-1] and g.ops[i][1] == caller]
            assert g.before(ev_chains, p["code"][0]) and g.before(recs[1], p["code"][0]), f"coder of batch {k - 1} ({knob})"
            if ahead_from is not None and k >= ahead_from:
                # the start point: the first thing on the side stream is a wait for an event of the batch before
                # (and the record of the batch's EV_START behind it)
                first = min(writers)
                assert g.ops[first - 2][0] == "wait" and g.ops[first - 1][0] == "record"
                assert g.ops[first - 2][1] == g.ops[first - 1][1] == g.ops[first][1]
                rec = max(i for i in g.idx("record") if i < first and g.ops[i][2] == g.ops[first - 2][2])
                assert g.ops[rec][1] == caller
                parts = [i for i in p["parse"] if g.ops[i][0] == "parse_part"]
                snaps = [i for i in p["parse"] if g.ops[i][0] == "snapshots"]
                lo, hi = {"plan": (p["plan"][0], parts[0]), "default": (p["plan"][0], parts[0]), "part": (parts[-1], snaps[-1]),
                          "iter1": (snaps[-1], p["parse"][-1])}[knob]
                assert lo < rec < hi, f"batch {k}: build ahead starts behind the wrong event ({knob})"
        if k >= 2 and b["delta_blocks"]:
            # the filtered copy and the choices of this parity: last read by batch k - 2
            p = B[k - 2]
            w, w0 = b["delta_blocks"][0], p["delta_blocks"][0]
            assert g.ops[w][2] == g.ops[w0][2], "one filtered copy per parity"
            for r in p["build"] + p["find"] + p["seeds"] + p["parse"] + p["code"]:
                assert g.ops[r][2] == g.ops[w][2] or g.ops[r][0] == "snapshots", "the readers read the filtered copy"
                assert g.before(r, w), f"batch {k}: filter writes the copy that {g.ops[r][0]} of batch {k - 2} reads ({knob})"
            assert g.before(w0, b["delta_choose"][0])
    return g, B


def stage_events(ops):
    """how often every event was recorded, without the two that bracket the call"""
    c = Counter(op[2] for op in ops if op[0] == "record")
    return {e: n for e, n in c.items() if n != 1}


@pytest.mark.parametrize("job", ["warm", "plain"])
def test_four_batches_every_start_point(cases, job):
    base_events = None
    for knob in ("0", "plan", "part", "iter1") + (("default",) if job == "warm" else ()):
        ops, end = cases[(job, knob)]
        assert end[0] == 0 and end[2] == 4 and end[3] == 1 and end[4] in (1, -1) and (job != "plain" or end[4] == 1), (job, knob, end)
        check_order(ops, knob, None if knob == "0" else 1)
        assert end[5] == (0 if knob == "0" else 3), "batches_ahead of the stats"
        ev = stage_events(ops)
        assert set(ev.values()) == {2}, "every stage event once per batch (two batches per parity)"
        if knob == "0":
            base_events = len(ev)
        else:
            # the same events as the serial schedule; EV_PART only where the build waits for it
            assert len(ev) == base_events + (2 if knob == "part" else 0), (knob, len(ev), base_events)


def test_knob_zero_is_the_serial_schedule(cases):
    ops, _ = cases[("warm", "0")]
    streams = {op[1] for op in ops if op[0] not in ("sync",)}
    g = Graph(ops)
    caller = ops[g.idx("find")[0]][1]
    for i in g.idx(*WRITERS):
        assert ops[i][1] == caller
    # the side stream carries the seed pieces and nothing else: a wait, two records and the launch per batch
    third = {ops[i][1] for i in g.idx("seeds")}
    assert len(third) == 1 and len(streams) == 3
    assert Counter(op[0] for op in ops if op[1] in third and op[0] != "sync") == Counter({"wait": 4, "record": 8, "seeds": 4})


def test_fallbacks_issue_nothing_ahead(cases):
    # a context that has never run: the first batch allocates, the second grows the tables of its parity -- serial; then ahead
    ops, end = cases[("cold", "part")]
    assert end[0] == 0 and end[2] == 4 and end[5] == 2
    check_order(ops, "part", 2)
    # a job of another size on the same context: three batches, the last one a single byte
    for knob, ahead in (("0", None), ("part", 1)):
        ops, end = cases[("short", knob)]
        assert end[0] == 0 and end[2] == 3 and end[3] == 1 and end[4] == 1
        check_order(ops, knob, ahead)
    # the forced allocation limit: the first batch (four Blocks) does not fit and is halved; the two batches that allocate
    # are serial, the two behind them find their buffers there
    for knob in ("0", "part"):
        ops, end = cases[("alloc_limit", knob)]
        assert end[0] == 0 and end[2] == 4 and end[3] == 1, end
        check_order(ops, knob, None if knob == "0" else 2)
    # a single-phase preset: no plan / pieces / coder in the log, every build on the one stream the call uses
    for knob in ("0", "part"):
        ops, end = cases[("single_phase", knob)]
        assert end[0] == 0 and end[2] == 4 and end[3] == 1 and end[4] == 1 and end[5] == 0
        builds = [op for op in ops if op[0] == "build"]
        assert len(builds) == 4 and len({op[1] for op in builds}) == 1
        assert {op[1] for op in ops if op[0] in ("wait", "record")} == {builds[0][1]} or not any(op[0] == "wait" for op in ops)
    assert cases[("single_phase", "0")][0] == cases[("single_phase", "part")][0]
