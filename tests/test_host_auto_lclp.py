"""The host side of the automatic per-Block literal context (XZAMD_F_AUTO_LCLP; xz_amd/csrc/xzamd_host.c, DESIGN.md 3.5
"Automatic literal context") without a GPU: tests/host_stub/driver_auto_lclp.c over the CPU stand-ins of the kernel layer
(stub_xzk.c and the others as they are, plus stub_xzk_lclp.c for the three new entry points), built with
-fsanitize=address,undefined and run as a program.  It covers the analysis entry point and its errors, the two debug fetches,
the props table in the span arguments of every parse and coder launch -- the table of the launch's own batch, with one batch and
with three (both pipeline parities), NULL without the flag -- and the combinations the flag declines; a second build without the
stand-ins is a kernel layer that lacks the entry points: the flag and the analysis are XZAMD_OPTIONS_ERROR there."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ("xzamd_host.c", "xzamd_frame.c", "xzamd_options.c", "xzamd_stream.c", "corpus.c", "xzamd_framing.c", "xzamd_decode.c", "xzamd_file.c",
        "xzamd_repair.c", "xzamd_repair_plan.c", "xzamd_chains.c")
WRAPS = ("xzk_parse_pieces", "xzk_model_snapshots", "xzk_encode_syms", "xzk_span_encode")


def _sources(with_kernels):
    stubs = ("stub_xzk.c", "stub_xzk_dec.c", "stub_xzk_chains.c") + (("stub_xzk_lclp.c",) if with_kernels else ()) + ("driver_auto_lclp.c",)
    return [os.path.join(ROOT, "xz_amd", "csrc", f) for f in CSRC] + [os.path.join(ROOT, "tests", "host_stub", f) for f in stubs] + \
           [os.path.join(ROOT, "oracle", f) for f in ("lzma2_dec.c", "xz_container.c", "lzma_fast_enc.c")]


@pytest.mark.parametrize("with_kernels", [True, False], ids=["stub_kernels", "no_kernels"])
def test_auto_lclp_host_layer_under_sanitizers(tmp_path, with_kernels):
    exe = str(tmp_path / "driver_auto_lclp")
    extra = [f"-Wl,--wrap={w}" for w in WRAPS] if with_kernels else ["-DDRIVER_NO_LCLP_KERNELS"]
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *_sources(with_kernels), "-Wl,--wrap=xzk_dec_units",
                    *extra, "-lm", "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k in ("LD_PRELOAD", "XZAMD_BATCH_MIB", "XZAMD_AUTO_DELTA", "XZAMD_AUTO_BCJ", "XZAMD_AUTO_LCLP", "XZAMD_NO_OVERLAP"):
        env.pop(k, None)
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "driver_auto_lclp: ok" in p.stdout, (p.stdout[-4000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
