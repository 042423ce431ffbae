"""lzma_easy_encoder / lzma_stream_encoder on the device: the single-Block Stream (one Block, header without sizes, LZMA2
data made of segments) against stock liblzma, against the MT path's own Block payloads, and through the interposer."""
import lzma
import os
import shutil
import subprocess

import pytest

import _oracle as o
import _single_block as sb

pytestmark = pytest.mark.gpu

SEG = 256 << 10
N = (1 << 20) + 5            # four full segments and a ragged one of 5 bytes


@pytest.fixture(scope="module")
def corpus():
    import xz_amd
    return xz_amd.corpus_text(N, seed=21).tobytes()


@pytest.fixture()
def seg_env(monkeypatch):
    monkeypatch.setenv("XZAMD_SEGMENT_KIB", str(SEG >> 10))
    return monkeypatch


def _block_data(raw):
    blocks = sb.parse_blocks(raw)
    assert len(blocks) == 1
    ho, hs, data, usize = blocks[0]
    assert (ho, hs) == (12, 12) and raw[12:14] == b"\x02\x00"
    return data


@pytest.mark.parametrize("preset", [1, 6])
def test_stream_decodes_and_equals_the_mt_payloads(seg_env, corpus, preset):
    import xz_amd
    L = xz_amd.lib()
    got, _ = sb.lzma_encode(corpus, preset)
    assert lzma.decompress(got) == corpus
    xz = shutil.which("xz")
    if xz:
        d = subprocess.run([xz, "-dc"], input=got, capture_output=True, timeout=120)
        assert d.returncode == 0 and d.stdout == corpus
    # the Block's data = the LZMA2 payloads of the Blocks the MT front end writes for the same input, options and
    # block_size = the segment size, end markers dropped, one 0x00 behind the last
    mt, _ = sb.lzma_encode(corpus, preset, mt_block_size=SEG)
    payloads = [p for _, _, p, _ in sb.parse_blocks(mt)]
    assert len(payloads) == 5 and all(p[-1] == 0 for p in payloads)
    want = b"".join(p[:-1] for p in payloads) + b"\0"
    data = _block_data(got)
    assert o.first_diff(data, want) == -1
    # fed in pieces; one and three workers with jobs of four segments: the same bytes
    pieces, _ = sb.lzma_encode(corpus, preset, piece=100003)
    assert pieces == got
    seg_env.setenv("XZAMD_BATCH_MIB", "1")
    for workers in ("1", "3"):
        L.xzamd_release_parked()
        seg_env.setenv("XZAMD_TEST_WORKERS", workers)
        w, _ = sb.lzma_encode(corpus, preset, piece=300000)
        assert w == got, workers
    seg_env.delenv("XZAMD_TEST_WORKERS")
    seg_env.delenv("XZAMD_BATCH_MIB")
    L.xzamd_release_parked()


def test_sync_flush_prefix_decodes(seg_env, corpus):
    got, cuts = sb.lzma_encode(corpus, 6, flushes=[(300000, sb.SYNC_FLUSH)])
    d = lzma.LZMADecompressor()
    assert d.decompress(got[:cuts[0]]) == corpus[:300000] and not d.eof
    assert lzma.decompress(got) == corpus and len(sb.parse_blocks(got)) == 1
    fed, cuts2 = sb.lzma_encode(corpus, 6, piece=77777, flushes=[(300000, sb.SYNC_FLUSH)])
    assert fed == got and cuts2 == cuts


def test_full_flush_and_crc32(seg_env, corpus):
    got, _ = sb.lzma_encode(corpus, 1, check=1, flushes=[(400000, sb.FULL_FLUSH)])
    assert lzma.decompress(got) == corpus
    assert [u for _, _, _, u in sb.parse_blocks(got)] == [400000, N - 400000]
    none, _ = sb.lzma_encode(corpus[:300001], 1, check=0)
    assert lzma.decompress(none) == corpus[:300001]


def test_empty_and_one_byte(seg_env):
    empty, _ = sb.lzma_encode(b"", 6)
    assert empty == lzma.compress(b"", check=lzma.CHECK_CRC64)
    one, _ = sb.lzma_encode(b"x", 6)
    assert lzma.decompress(one) == b"x" and len(sb.parse_blocks(one)) == 1


def test_round_trip_through_the_plain_device_decode(seg_env, corpus):
    import torch
    import xz_amd
    got, _ = sb.lzma_encode(corpus, 6)
    enc = xz_amd.Encoder()
    t = torch.frombuffer(bytearray(got), dtype=torch.uint8).cuda()
    dec, nb = enc.decode(t, N + 16)
    assert nb == 1 and dec.cpu().numpy().tobytes() == corpus
    assert enc.debug_decode_units() == (5, 1, 2)          # five segments: five units of one Block
    enc.close()


def test_declined_at_init(seg_env):
    import ctypes as C
    import xz_amd
    Mt, Stream = sb._structs()
    L = xz_amd.lib()
    L.lzma_easy_encoder.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    s = Stream()
    assert L.lzma_easy_encoder(C.byref(s), 6, 10) == 8           # SHA-256: LZMA_OPTIONS_ERROR
    assert L.lzma_easy_encoder(C.byref(s), 10, 4) == 8           # no such preset
    assert s.internal is None


def test_interposer_routes_xz_T1_to_the_device(tmp_path, corpus):
    """The stock `xz -T1` (single-threaded lzma_stream_encoder) under LD_PRELOAD=libxz_amd_preload.so."""
    import xz_amd
    xz = shutil.which("xz")
    if not xz:
        pytest.skip("no xz binary")
    pre = os.path.join(os.path.dirname(xz_amd.LIB_PATH), "libxz_amd_preload.so")
    assert os.path.exists(pre), "libxz_amd_preload.so not built"
    data = corpus[: 1 << 20]
    src = tmp_path / "input.bin"
    src.write_bytes(data)
    env = dict(os.environ, LD_PRELOAD=pre, XZ_AMD_VERBOSE="1")
    p = subprocess.run(["timeout", "-k", "10", "120", xz, "-T1", "-1", "-c", str(src)], capture_output=True, env=env, timeout=150)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"-> GPU" in p.stderr and b"lzma_stream_encoder_mt" not in p.stderr, p.stderr.decode()[-2000:]
    d = subprocess.run([xz, "-dc"], input=p.stdout, capture_output=True, timeout=120)
    assert d.returncode == 0 and d.stdout == data
    assert len(sb.parse_blocks(p.stdout)) == 1
    env2 = dict(env, XZ_AMD_DISABLE="1")
    p2 = subprocess.run(["timeout", "-k", "10", "120", xz, "-T1", "-1", "-c", str(src)], capture_output=True, env=env2, timeout=150)
    assert p2.returncode == 0 and b"-> GPU" not in p2.stderr
