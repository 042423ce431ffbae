#!/usr/bin/env python3
"""Timings of the verified encode: verification decode of one Stream with units = Blocks (what
decode(expected=) does with a two-phase Stream) next to Encoder.verify with the kept resume table (units = encode spans),
and what keeping the table / verifying costs the encode.  XZ_AMD_LIB selects the library build; the `blocks` mode uses
nothing a build without the verified encode lacks, so the same figure can be taken with an older library.

usage: tools/bench_verify.py blocks [MiB=1024] [preset=6] [reps=3]   encode, then decode(expected=) timed
       tools/bench_verify.py table  [MiB=1024] [preset=6] [reps=3]   encode(keep_resume), then Encoder.verify timed
       tools/bench_verify.py encode [MiB=1024] [preset=6] [reps=3]   encode plain / keep_resume / verify, alternating
       tools/bench_verify.py all    [MiB=1024] [preset=6] [reps=3]   the three in one process
Prints one line per figure: median, the runs, MB/s of the uncompressed size."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import xz_amd  # noqa: E402


def timed(f, reps, warm=1):
    import torch
    times = []
    for _ in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times[warm:], r


def line(what, runs, nbytes, extra=""):
    med = statistics.median(runs)
    print(f"{what}: median {med * 1e3:.1f} ms = {nbytes / med / 1e6:.1f} MB/s (runs {' '.join(f'{x * 1e3:.1f}' for x in runs)} ms; "
          f"spread {(max(runs) - min(runs)) * 1e3:.1f} ms){extra}", flush=True)
    return med


def main():
    import torch
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd not in ("blocks", "table", "encode", "all"):
        sys.exit(__doc__)
    a = sys.argv[2:]
    mib = int(a[0]) if a else 1024
    preset = int(a[1]) if len(a) > 1 else 6
    reps = int(a[2]) if len(a) > 2 else 3
    data = xz_amd.corpus_text(mib << 20, seed=1000)
    d = torch.from_numpy(data).cuda()
    n = data.size
    enc = xz_amd.Encoder(0)
    opts = xz_amd.preset_options(preset)
    print(f"lib {'XZ_AMD_LIB' if os.environ.get('XZ_AMD_LIB') else 'in-tree'} ({os.path.basename(xz_amd.LIB_PATH)}); {mib} MiB corpus_text, preset {preset}, default Blocks", flush=True)
    if cmd in ("blocks", "all"):
        xz, binfo = enc.encode(d, opts=opts)
        runs, _ = timed(lambda: enc.decode(xz, n, expected=d), reps)
        units = enc.debug_decode_units()
        line(f"(a) decode(expected=), units {units[0]} of {units[1]} Blocks, split {units[2]}", runs, n)
    if cmd in ("table", "all"):
        xz, binfo = enc.encode(d, opts=opts, keep_resume=True)
        st = enc.stats()
        runs, rep = timed(lambda: enc.verify(xz, d), reps)
        line(f"(b) Encoder.verify, units {rep['units']} (encode spans {st.enc_spans}, Blocks {rep['blocks']}), table_used {rep['table_used']}",
             runs, n, f"; table {enc.debug_resume_records()} records")
    if cmd in ("encode", "all"):
        kinds = (("plain", {}), ("keep_resume", {"keep_resume": True}), ("verify", {"verify": True}))
        runs = {k: [] for k, _ in kinds}
        vms = []
        enc.encode(d, opts=opts)                    # warm-up: buffers allocated
        for _ in range(reps):
            for k, kw in kinds:
                r, _ = timed(lambda: enc.encode(d, opts=opts, **kw), 1, warm=0)
                runs[k] += r
                if k == "verify":
                    vms.append(enc.stats().ms_verify)
        m0 = line("(c) encode, no flag", runs["plain"], n)
        m1 = line("(c) encode, keep_resume", runs["keep_resume"], n)
        print(f"(c) export cost: {(m1 - m0) * 1e3:+.1f} ms = {(m1 / m0 - 1) * 100:+.2f} %", flush=True)
        line("(d) encode, verify=True", runs["verify"], n, f"; ms_verify {' '.join(f'{x:.1f}' for x in vms)}")
    enc.close()


if __name__ == "__main__":
    main()
