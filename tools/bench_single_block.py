#!/usr/bin/env python3
"""Timings around the single-Block encoder (lzma_easy_encoder) and the plain device decode with units at dictionary
resets.  XZ_AMD_LIB selects the library build, so that two builds can be compared in alternating processes.

usage: tools/bench_single_block.py make OUT.xz [MiB=32] [preset=6]   one Block written by lzma_easy_encoder (segments:
                                                                     XZAMD_SEGMENT_KIB) from MiB of the text corpus
       tools/bench_single_block.py decode FILE.xz [reps=5]           plain device decode of a file, wall clock per run
       tools/bench_single_block.py decode-mt [MiB=64] [block MiB=1] [reps=5]   the same for an MT Stream encoded here
       tools/bench_single_block.py encode [MiB=1024] [preset=6] [reps=2]       host-to-host rate of lzma_easy_encoder next
                                                                     to lzma_stream_encoder_mt (one lzma_code(LZMA_FINISH))
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import xz_amd  # noqa: E402
from bench_lzma_code import Mt, Stream  # noqa: E402


def lzma_code_finish(L, s, data, out):
    s.next_in, s.avail_in = data.ctypes.data, data.size
    s.next_out, s.avail_out = out.ctypes.data, out.size
    t0 = time.perf_counter()
    rc = L.lzma_code(C.byref(s), 3)
    while rc == 0:
        rc = L.lzma_code(C.byref(s), 3)
    dt = time.perf_counter() - t0
    assert rc == 1, rc
    return dt


def easy_encode(L, data, preset, out):
    s = Stream()
    L.lzma_easy_encoder.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    assert L.lzma_easy_encoder(C.byref(s), preset, 4) == 0
    dt = lzma_code_finish(L, s, data, out)
    n = s.total_out
    L.lzma_end(C.byref(s))
    return dt, n


def mt_encode(L, data, preset, out):
    s = Stream()
    m = Mt(threads=1, preset=preset, check=4)
    assert L.lzma_stream_encoder_mt(C.byref(s), C.byref(m)) == 0
    dt = lzma_code_finish(L, s, data, out)
    n = s.total_out
    L.lzma_end(C.byref(s))
    return dt, n


def timed_decodes(enc, t, cap, reps, what):
    import torch
    times = []
    for _ in range(reps + 1):                      # the first run is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, nb = enc.decode(t, cap)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    units = enc.debug_decode_units() if hasattr(xz_amd.lib(), "xzamd_debug_decode_units_") else ("-", nb, "-")
    runs = times[1:]
    print(f"{what}: lib {os.path.basename(os.path.dirname(xz_amd.LIB_PATH))}/{os.path.basename(xz_amd.LIB_PATH)} "
          f"{out.numel() >> 20} MiB, {nb} Block(s), units {units[0]}: median {statistics.median(runs):.4f} s "
          f"(runs {' '.join(f'{x:.4f}' for x in runs)}; warm-up {times[0]:.4f})", flush=True)
    return out


def main():
    cmd = sys.argv[1]
    a = sys.argv[2:]
    L = xz_amd.lib()
    if cmd == "make":
        mib = int(a[1]) if len(a) > 1 else 32
        preset = int(a[2]) if len(a) > 2 else 6
        data = xz_amd.corpus_text(mib << 20, seed=1000)
        out = np.empty(data.size // 2 + (1 << 20), dtype=np.uint8)
        dt, n = easy_encode(L, data, preset, out)
        out[:n].tofile(a[0])
        print(f"made {a[0]}: {mib} MiB -> {n} B, preset {preset}, XZAMD_SEGMENT_KIB={os.environ.get('XZAMD_SEGMENT_KIB', '-')}, {dt:.3f} s", flush=True)
    elif cmd == "decode":
        import torch
        reps = int(a[1]) if len(a) > 1 else 5
        raw = np.fromfile(a[0], dtype=np.uint8)
        _, _, usize = xz_amd.file_index(raw.tobytes())
        enc = xz_amd.Encoder(0)
        timed_decodes(enc, torch.from_numpy(raw).cuda(), usize + 16, reps, "plain decode of " + os.path.basename(a[0]))
        enc.close()
    elif cmd == "decode-mt":
        import torch
        mib = int(a[0]) if a else 64
        bmib = int(a[1]) if len(a) > 1 else 1
        reps = int(a[2]) if len(a) > 2 else 5
        data = xz_amd.corpus_text(mib << 20, seed=1000)
        enc = xz_amd.Encoder(0)
        xz, _ = enc.encode(torch.from_numpy(data).cuda(), preset=6, block_size=bmib << 20)
        out = timed_decodes(enc, xz, data.size + 16, reps, f"plain decode, MT Stream of {bmib} MiB Blocks")
        assert (out.cpu().numpy() == data).all()
        enc.close()
    elif cmd == "encode":
        mib = int(a[0]) if a else 1024
        preset = int(a[1]) if len(a) > 1 else 6
        reps = int(a[2]) if len(a) > 2 else 2
        data = xz_amd.corpus_text(mib << 20, seed=1000)
        out = np.empty(data.size // 2 + (1 << 20), dtype=np.uint8)
        for r in range(reps):
            for name, f in (("lzma_stream_encoder_mt", mt_encode), ("lzma_easy_encoder", easy_encode)):
                dt, n = f(L, data, preset, out)
                print(f"{name} host->host preset {preset} {mib} MiB: {dt*1e3:.1f} ms = {data.size/dt/1e6:.1f} MB/s, "
                      f"ratio {n/data.size:.4f}", flush=True)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
