"""The single-Block encoder's host code without a GPU: lzma_easy_encoder / lzma_stream_encoder of xzamd_stream.c over
xzamd_host.c, xzamd_frame.c and xzamd_options.c, compiled on top of the CPU stand-in for the kernel layer
(tests/host_stub/stub_xzk.c, unchanged) and driven by a stand-alone program (tests/host_stub/driver_single.c) -- built
once plain and once with -fsanitize=address,undefined, and run as a program.  300,000 bytes, 64 KiB segments, fed 1 byte,
4097 bytes at a time and all at once; with LZMA_SYNC_FLUSH behind byte 100,000; with LZMA_FULL_FLUSH behind byte
200,000.  Python's lzma (stock liblzma) is the judge of what comes out."""
import lzma
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "xz_amd", "csrc", f) for f in ("xzamd_stream.c", "xzamd_host.c", "xzamd_frame.c", "xzamd_options.c", "corpus.c")] + \
      [os.path.join(ROOT, "tests", "host_stub", f) for f in ("stub_xzk.c", "driver_single.c")]
FEEDS = ("1", "4097", "all")
N = 300000


def _sanitizer_usable(flag, tmp):
    src = os.path.join(tmp, "p.c")
    open(src, "w").write("int main(void){return 0;}\n")
    exe = os.path.join(tmp, "p")
    r = subprocess.run(["gcc", flag, src, "-o", exe], capture_output=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def outdir(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("single_" + request.param)
    flags = []
    if request.param == "asan_ubsan":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        if not shutil.which("gcc") or not _sanitizer_usable(flags[0], str(tmp)):
            pytest.skip(f"{flags[0]} not usable here")
    exe = str(tmp / "driver_single")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-pthread", *flags, *SRC, "-o", exe], check=True)
    out = tmp / "out"
    out.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    for k in ("XZAMD_SEGMENT_KIB", "XZAMD_TEST_WORKERS", "XZAMD_BATCH_MIB"):
        env.pop(k, None)
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "driver_single: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-6000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-6000:]
    return out


def _read(outdir, name):
    return open(outdir / name, "rb").read()


def _blocks(raw):
    import xz_amd
    return xz_amd.file_index(raw)[1]


def test_output_decodes_and_does_not_depend_on_the_feeding(outdir, product_lib):
    data = _read(outdir, "input.bin")
    assert len(data) == N
    for kind in ("plain", "sync", "full"):
        outs = [_read(outdir, f"{kind}_{f}.xz") for f in FEEDS]
        assert lzma.decompress(outs[0]) == data, kind
        assert outs[1] == outs[0] and outs[2] == outs[0], kind
    assert lzma.decompress(_read(outdir, "barrier.xz")) == data


def test_one_block_whose_header_has_no_sizes(outdir, product_lib):
    raw = _read(outdir, "plain_all.xz")
    blocks = _blocks(raw)
    assert len(blocks) == 1 and blocks[0]["uncompressed_size"] == N and blocks[0]["header_offset"] == 12
    assert raw[12] == 0x02 and raw[13] == 0x00 and raw[14:16] == b"\x21\x01"      # 12 bytes; Block Flags: one filter, no sizes
    # the stub codes stored chunks: segments of 64 KiB start with control 0x01 (dictionary reset), nothing else does
    pos, resets, u = 24, [], 0
    while raw[pos] != 0:
        assert raw[pos] in (1, 2)
        if raw[pos] == 1:
            resets.append(u)
        k = ((raw[pos + 1] << 8) | raw[pos + 2]) + 1
        pos += 3 + k
        u += k
    assert u == N and resets == list(range(0, N, 65536))


def test_sync_flush_hands_out_a_decodable_prefix(outdir, product_lib):
    data = _read(outdir, "input.bin")
    for f in FEEDS:
        raw = _read(outdir, f"sync_{f}.xz")
        cut = int(_read(outdir, f"sync_{f}.cut"))
        d = lzma.LZMADecompressor()
        assert d.decompress(raw[:cut]) == data[:100000] and not d.eof
        assert d.decompress(raw[cut:]) == data[100000:] and d.eof
    # still one Block; the flush starts a segment at byte 100,000 (costs ratio, not correctness)
    assert len(_blocks(_read(outdir, "sync_all.xz"))) == 1
    assert len(_read(outdir, "sync_all.xz")) > len(_read(outdir, "plain_all.xz"))


def test_full_flush_yields_two_blocks(outdir, product_lib):
    for name in ("full_all.xz", "barrier.xz"):
        raw = _read(outdir, name)
        blocks = _blocks(raw)
        assert [b["uncompressed_size"] for b in blocks] == [200000, 100000], name
        for b in blocks:
            ho = b["header_offset"]
            assert raw[ho] == 0x02 and raw[ho + 1] == 0x00, name               # no size fields in either header


def test_empty_input_is_a_stream_without_blocks(outdir):
    assert _read(outdir, "empty.xz") == lzma.compress(b"", check=lzma.CHECK_CRC64)

# (An {x86, LZMA2} chain and SHA-256 giving LZMA_OPTIONS_ERROR at init, and the other option checks, are CHECKs of the
# driver itself: it exits non-zero when one of them answers differently.)
