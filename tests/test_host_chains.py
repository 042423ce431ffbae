"""The host code of the bare chunk chains (xz_amd/csrc/xzamd_chains.c, DESIGN.md 3.6 "Chains") without a GPU: the chain table
made from the block infos of an XZAMD_F_SEGMENTS encode, the per-segment verdicts, the repair with its all-or-nothing splice and
the framing of XZAMD_F_SINGLE, over the CPU stand-ins of the kernel layer -- tests/host_stub/stub_xzk.c and stub_xzk_dec.c as
they are, plus stub_xzk_chains.c, which restates the bare-chain grammar for xzk_dec_scan_chains in plain C (and, because the
decode stand-in of stub_xzk_dec.c hands a Block's data to a decoder that wants the end marker a chain lacks, takes the place of
xzk_dec_units through the linker's --wrap).  tests/host_stub/driver_chains.c is built with -fsanitize=address,undefined and run
as a program.  It checks: verdicts for a good table (Checks none, CRC32, CRC64, with and without the original); a chain cut one
byte short, a 0x00 in the middle of a chain and a chain without a dictionary reset ("grammar"); a wrong CRC in the table
("check"); a wrong original ("compare"); a table that names bytes outside the buffer; a repair that finds nothing to do; the
repair of a tampered coded chain (made with the oracle's encoder) into a buffer one byte short -- XZAMD_BUF_ERROR with the needed
size, chains and table untouched -- and into one that fits: offsets and lengths rewritten, CRCs kept, the other chains the bytes
they were, the whole decodable; the test knobs (segments 0 and 2 rejected, stored rung); the single-Block Stream through the
oracle's container decoder, the empty one, and the flag combinations that are errors."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ("xzamd_host.c", "xzamd_frame.c", "xzamd_options.c", "xzamd_stream.c", "corpus.c", "xzamd_framing.c", "xzamd_decode.c", "xzamd_file.c",
        "xzamd_repair.c", "xzamd_repair_plan.c", "xzamd_chains.c")
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in CSRC] + \
      [os.path.join(ROOT, "tests", "host_stub", f) for f in ("stub_xzk.c", "stub_xzk_dec.c", "stub_xzk_chains.c", "driver_chains.c")] + \
      [os.path.join(ROOT, "oracle", f) for f in ("lzma2_dec.c", "xz_container.c", "lzma_fast_enc.c")]


def test_chain_host_layer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "driver_chains")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *SRC, "-Wl,--wrap=xzk_dec_units", "-lm",
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k in ("LD_PRELOAD", "XZAMD_TEST_REPAIR_REJECT", "XZAMD_TEST_REPAIR_RUNG", "XZAMD_BATCH_MIB"):
        env.pop(k, None)
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "driver_chains: ok" in p.stdout, (p.stdout[-4000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
