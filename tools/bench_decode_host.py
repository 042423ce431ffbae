#!/usr/bin/env python3
"""Host-side cost of the device decoder's entries: what the framing in front of the kernels takes, on Streams of stored-size
extremes.  One process is one round; XZ_AMD_LIB selects the library build, so that two builds can be compared in alternating
processes (profiles/decode_host_ab.txt).

usage: tools/bench_decode_host.py [label]
  (a) decode of a one-Block 64 KiB Stream                   us per call, median of 5 batches of 100 calls
  (b) decode of 256 MiB in 4,096 Blocks of 64 KiB           ms, median of 3 calls
  (c) decode_file and verify_blocks (with the original) of (b)
Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import xz_amd  # noqa: E402


def timed(f, reps, calls=1, warm=1):
    import torch
    times = []
    for _ in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / calls)
    return statistics.median(times[warm:])


def main():
    import torch
    label = sys.argv[1] if len(sys.argv) > 1 else ("XZ_AMD_LIB" if os.environ.get("XZ_AMD_LIB") else "in-tree")
    bs = 65536
    data = xz_amd.corpus_text(256 << 20, seed=1000)
    d = torch.from_numpy(data).cuda()
    n = data.size
    enc = xz_amd.Encoder(0)
    opts = xz_amd.preset_options(1)
    small, _ = enc.encode(d[:bs], opts=opts, block_size=bs)
    small = small.clone()
    big, _ = enc.encode(d, opts=opts, block_size=bs)
    big = big.clone()
    _, nb = enc.decode(big, n)
    assert nb == n // bs and enc.decode(small, bs)[1] == 1
    res = {"label": label, "lib": os.path.basename(xz_amd.LIB_PATH)}
    res["a_decode_1x64KiB_us"] = round(timed(lambda: enc.decode(small, bs), 5, calls=100) * 1e6, 2)
    res["b_decode_4096x64KiB_ms"] = round(timed(lambda: enc.decode(big, n), 3) * 1e3, 3)
    res["c_decode_file_ms"] = round(timed(lambda: enc.decode_file(big, n), 3) * 1e3, 3)
    res["c_verify_blocks_ms"] = round(timed(lambda: enc.verify_blocks(big, d), 3) * 1e3, 3)
    enc.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
