#!/usr/bin/env python3
"""Timings of the repair (DESIGN.md 3.6 "Repair"), input resident in HBM: what encode(repair=True) costs when nothing is
rejected (next to the plain and the verify=True encode), and what a repair costs when XZAMD_TEST_REPAIR_REJECT rejects one
and then four Blocks -- ms_repair split into verification passes, re-encode and splice, and the size of every repaired
Block next to its two-phase size.  XZ_AMD_LIB selects the library build (the `ask` figures of an older library: plain and
verify only).

usage: tools/bench_repair.py ask    [MiB=1024] [preset=6] [reps=3] [block MiB=24]   plain / verify / repair, alternating
       tools/bench_repair.py reject [MiB=1024] [preset=6] [reps=3] [block MiB=24]   1 and 4 Blocks rejected
       tools/bench_repair.py all    [MiB=1024] [preset=6] [reps=3] [block MiB=24]
       tools/bench_repair.py single [MiB=1024] [preset=6] [reps=3]    the single-Block path: lzma_easy_encoder through one
                                                                      lzma_code(LZMA_FINISH), host to host, default segments
                                                                      (XZAMD_SEGMENT_KIB), without and -- where the library
                                                                      honours it there -- with XZAMD_REPAIR=1, alternating
Prints one line per figure: median, the runs, MB/s of the uncompressed size."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import xz_amd  # noqa: E402
from bench_verify import line, timed  # noqa: E402


def single(mib, preset, reps):
    """XZAMD_REPAIR is read by lzma_easy_encoder at init: one process can time both settings side by side"""
    import numpy as np
    from bench_single_block import easy_encode
    L = xz_amd.lib()
    data = xz_amd.corpus_text(mib << 20, seed=1000)
    out = np.empty(data.size // 2 + (1 << 20), dtype=np.uint8)
    has = hasattr(L, "xzamd_chains_repair_device")
    print(f"lib {'XZ_AMD_LIB' if os.environ.get('XZ_AMD_LIB') else 'in-tree'} ({os.path.basename(xz_amd.LIB_PATH)}); {mib} MiB corpus_text, "
          f"preset {preset}, lzma_easy_encoder, XZAMD_SEGMENT_KIB={os.environ.get('XZAMD_SEGMENT_KIB', '-')}; repair of segments "
          f"{'present' if has else 'absent'}", flush=True)
    os.environ.pop("XZAMD_REPAIR", None)
    os.environ.pop("XZAMD_TEST_REPAIR_REJECT", None)
    easy_encode(L, data, preset, out)                               # warm-up: buffers allocated and parked
    kinds = [("XZAMD_REPAIR unset", None)] + ([("XZAMD_REPAIR=1", "1")] if has else [])
    runs = {k: [] for k, _ in kinds}
    sizes = {}
    for _ in range(reps):
        for k, v in kinds:
            if v is None:
                os.environ.pop("XZAMD_REPAIR", None)
            else:
                os.environ["XZAMD_REPAIR"] = v
            dt, sizes[k] = easy_encode(L, data, preset, out)
            runs[k].append(dt)
    os.environ.pop("XZAMD_REPAIR", None)
    m0 = line(f"(s) lzma_easy_encoder, {kinds[0][0]}", runs[kinds[0][0]], data.size, f"; {sizes[kinds[0][0]]} bytes")
    for k, _ in kinds[1:]:
        m = line(f"(s) lzma_easy_encoder, {k}", runs[k], data.size, f"; {sizes[k]} bytes")
        print(f"(s) cost of {k}: {(m - m0) * 1e3:+.1f} ms = {(m / m0 - 1) * 100:+.2f} %", flush=True)
    xz_amd.lib().xzamd_release_parked()


def main():
    import torch
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "single":
        a = sys.argv[2:]
        return single(int(a[0]) if a else 1024, int(a[1]) if len(a) > 1 else 6, int(a[2]) if len(a) > 2 else 3)
    if cmd not in ("ask", "reject", "all"):
        sys.exit(__doc__)
    a = sys.argv[2:]
    mib = int(a[0]) if a else 1024
    preset = int(a[1]) if len(a) > 1 else 6
    reps = int(a[2]) if len(a) > 2 else 3
    bs = (int(a[3]) if len(a) > 3 else 24) << 20
    data = xz_amd.corpus_text(mib << 20, seed=1000)
    d = torch.from_numpy(data).cuda()
    n = data.size
    enc = xz_amd.Encoder(0)
    opts = xz_amd.preset_options(preset)
    has_repair = hasattr(xz_amd.lib(), "xzamd_stream_repair_device")
    print(f"lib {'XZ_AMD_LIB' if os.environ.get('XZ_AMD_LIB') else 'in-tree'} ({os.path.basename(xz_amd.LIB_PATH)}); {mib} MiB corpus_text, "
          f"preset {preset}, Blocks of {bs >> 20} MiB; repair {'present' if has_repair else 'absent'}", flush=True)
    os.environ.pop("XZAMD_TEST_REPAIR_REJECT", None)
    plain, pinfo = enc.encode(d, opts=opts, block_size=bs)          # warm-up: buffers allocated
    plain_sizes = [b.total_size for b in pinfo]
    if cmd in ("ask", "all"):
        kinds = [("plain", {}), ("verify", {"verify": True})] + ([("repair", {"repair": True})] if has_repair else [])
        runs = {k: [] for k, _ in kinds}
        extra = {k: [] for k, _ in kinds}
        for _ in range(reps):
            for k, kw in kinds:
                r, _ = timed(lambda: enc.encode(d, opts=opts, block_size=bs, **kw), 1, warm=0)
                runs[k] += r
                if k != "plain":
                    extra[k].append(enc.stats().ms_verify)
        m0 = line("(a) encode, no flag", runs["plain"], n)
        for k, _ in kinds[1:]:
            m = line(f"(a) encode, {k}=True", runs[k], n, f"; ms_verify {' '.join(f'{x:.1f}' for x in extra[k])}")
            print(f"(a) cost of {k}: {(m - m0) * 1e3:+.1f} ms = {(m / m0 - 1) * 100:+.2f} %", flush=True)
    if cmd in ("reject", "all") and has_repair:
        nb = len(pinfo)
        for rejected in ([nb // 2], [0, nb // 3, nb // 2, nb - 1]):
            os.environ["XZAMD_TEST_REPAIR_REJECT"] = ",".join(str(b) for b in rejected)
            reports = []

            def run():
                out = enc.encode(d, opts=opts, block_size=bs, repair=True)
                reports.append(enc.repair_report())
                return out
            runs, (xz, binfo) = timed(run, reps)
            os.environ.pop("XZAMD_TEST_REPAIR_REJECT", None)
            rep = reports[-1]
            line(f"(b) encode, repair=True, Blocks {rejected} rejected", runs, n)
            for key in ("ms_repair", "ms_verify_passes", "ms_reencode", "ms_splice"):
                print(f"    {key}: {' '.join(f'{r[key]:.1f}' for r in reports[1:])}", flush=True)
            print(f"    passes {rep['passes']}, bad {rep['blocks_bad']}, re-encoded {rep['blocks_reencoded']}, stored {rep['blocks_stored']}, "
                  f"Stream {rep['size_before']} -> {rep['size_after']} bytes", flush=True)
            for b in rejected:
                print(f"    Block {b}: two-phase {plain_sizes[b]} bytes, single-phase {binfo[b].total_size} bytes "
                      f"({(binfo[b].total_size / plain_sizes[b] - 1) * 100:+.2f} %)", flush=True)
    enc.close()


if __name__ == "__main__":
    main()
