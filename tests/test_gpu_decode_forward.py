"""Forward decode on the device (Encoder.decode_forward: xzamd_file_decode_forward_device, k_dec_walk): an .xz file read from
its front without its Index -- against the backward reader (Encoder.decode_file) on intact files, against the real liblzma
(oracle/_ref: lzma_stream_buffer_decode for the codes of whole files, lzma_stream_decoder / lzma_code for what a truncated or
damaged input still delivers), and the reads and launches per file."""
import glob
import os

import pytest

import _forward as fw
import _oracle as o
import _xzfiles as x

pytestmark = pytest.mark.gpu

OPTIONS_ERROR, DATA_ERROR, BUF_ERROR, UNSUPPORTED_CHECK = 8, 9, 10, 3
END, TRUNCATED, DEFECT, OUT_FULL = 1, 2, 3, 4
BS = x.BS


@pytest.fixture(scope="module")
def enc():
    import xz_amd
    e = xz_amd.Encoder()
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref():
    """the tests whose inputs or verdicts come from the real liblzma"""
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    return fw.ref_lib()


def _cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _forward(enc, raw, out_cap, concatenated=True):
    """(code, bytes delivered, report) of decode_forward, whatever the code"""
    import xz_amd
    try:
        got, rp = enc.decode_forward(_cuda(raw), out_cap, concatenated=concatenated)
    except xz_amd.XzAmdError as e:
        assert e.code not in (0, BUF_ERROR) and e.report["stop"] == DEFECT
        return e.code, _bytes(e.partial), e.report
    return rp["code"], _bytes(got), rp


def _backward_code(enc, raw, out_cap):
    import xz_amd
    try:
        enc.decode_file(_cuda(raw), out_cap)
    except xz_amd.XzAmdError as e:
        return e.code
    return 0


# ---------------------------------------------------------------- 3. intact inputs: forward == backward
def _own(enc, data, preset, chain=0, **kw):
    import xz_amd
    opts = xz_amd.preset_options(preset)
    opts.bcj = chain
    xz, _ = enc.encode(_cuda(data), opts=opts, block_size=BS, **kw)
    return _bytes(xz)


def _same_as_backward(enc, raw, data):
    want, nb = enc.decode_file(_cuda(raw), len(data) + 16)
    assert _bytes(want) == data
    code, got, rp = _forward(enc, raw, len(data) + 16)
    assert code == 0 and o.first_diff(got, data) == -1 and len(got) == len(data)
    assert rp["stop"] == END and rp["blocks"] == rp["blocks_delivered"] == nb and rp["consumed"] == len(raw)
    return rp


@pytest.mark.parametrize("name", ["checks-p0", "checks-p1", "delta-p0", "delta-p1"])
def test_forward_equals_backward_on_built_files(enc, ref, name):
    fl = x.built_files()[name]
    rp = _same_as_backward(enc, fl.raw, fl.data)
    assert rp["streams"] == 3


@pytest.fixture(scope="module")
def ragged():
    return o.corpus_mixed(5 * BS + 777, 71)


@pytest.mark.parametrize("preset", [1, 6])
@pytest.mark.parametrize("chain", ["plain", "delta", "x86"])
def test_forward_equals_backward_on_own_streams(enc, ragged, preset, chain):
    """5 Blocks of 64 KiB and a ragged last one from the device encoder"""
    import xz_amd
    data = ragged if chain != "x86" else o.corpus_x86(5 * BS + 777, 72)
    raw = _own(enc, data, preset, {"plain": 0, "delta": xz_amd.filter_delta(4), "x86": 4}[chain])
    rp = _same_as_backward(enc, raw, data)
    assert rp["blocks"] == 6 and rp["streams"] == 1


def test_forward_equals_backward_on_a_single_block_stream(enc):
    """Encoder.encode(single=True), four segments: one Block whose header has no sizes -- the walk follows its chunk chain"""
    data = o.corpus_mixed(4 * BS, 73)
    raw = _own(enc, data, 1, single=True)
    assert raw[12 + 1] & 0xC0 == 0, "the single-Block Stream carries no sizes in its Block Header"
    rp = _same_as_backward(enc, raw, data)
    assert rp["blocks"] == 1


@pytest.mark.parametrize("chain", ["delta", "x86"])
def test_forward_equals_backward_without_sizes_and_with_filters(enc, ref, chain):
    """{delta, LZMA2} and {x86, LZMA2} with Block Headers without sizes (the single-Block encoder takes no filters: the
    reference's Streams, one Block of four chunks' worth and four Blocks, with the sizes taken out of their headers)"""
    data = o.corpus_x86(4 * BS, 74) if chain == "x86" else o.corpus_mixed(4 * BS, 75)
    for bs in (1 << 20, BS):
        raw = fw.strip_sizes(o.ref_encode_mt_chain(data, 1, 4 if chain == "x86" else 3, 4, block_size=bs))
        r, want = x.ref_concat_decode(raw, len(data) + 16)
        assert r == 0 and want == data
        rp = _same_as_backward(enc, raw, data)
        assert rp["blocks"] == (1 if bs > BS else 4)


def test_built_files_with_an_x86_stream(enc, ref):
    a, b, c = x.inputs()
    code_like = o.corpus_x86(len(c), 76)
    raw = o.ref_encode_mt(b, 1, block_size=BS) + o.ref_encode_mt_chain(code_like, 1, 4, block_size=BS) + b"\0" * 4 \
        + o.ref_encode_mt(a, 1, block_size=BS)
    rp = _same_as_backward(enc, raw, b + code_like + a)
    assert rp["streams"] == 3


# ---------------------------------------------------------------- 4. every fixture file against the reference
def test_every_fixture_against_the_reference(enc, ref):
    files = sorted(glob.glob(os.path.join(x.GOLD, "ref_files*", "*.xz")))
    assert len(files) >= 40
    good = 0
    for p in files:
        raw = open(p, "rb").read()
        r, want = x.ref_concat_decode(raw, 1 << 20)
        back = _backward_code(enc, raw, 1 << 20)
        code, got, rp = _forward(enc, raw, 1 << 20)
        if back == r:
            assert code == r, (p, code, r, rp)
            if r == 0:
                assert got == want, p
                good += os.path.basename(p).startswith("good-")
        else:
            # what decode_file itself declines although the reference reads it: the same answer from the front
            assert back in (OPTIONS_ERROR, UNSUPPORTED_CHECK) and code == back, (p, code, back, r)
    assert good >= 15


# ---------------------------------------------------------------- 5. truncation
@pytest.fixture(scope="module")
def four(ref):
    import xz_amd
    data = o.corpus_mixed(4 * BS, 77)
    raw = o.ref_encode_mt(data, 1, block_size=BS)
    _, blocks, _ = xz_amd.file_index(raw)
    assert len(blocks) == 4
    return raw, data, blocks


def _cuts(raw, blocks):
    ends = [b["header_offset"] + b["total_size"] for b in blocks]
    index_at = ends[-1]
    cuts = {5, 11, 12, blocks[0]["header_offset"] + 3, blocks[2]["header_offset"] + blocks[2]["total_size"] // 2, index_at + 2, len(raw) - 1}
    for e in ends:
        cuts |= {e - 1, e, e + 1}
    return sorted(cuts), ends


def test_truncated_input_delivers_the_whole_blocks(enc, ref, four):
    raw, data, blocks = four
    L = ref
    cuts, ends = _cuts(raw, blocks)
    assert len(cuts) >= 7 + 3 * 4 - 1
    for cut in cuts:
        whole = sum(1 for e in ends if e <= cut)
        code, got, rp = _forward(enc, raw[:cut], len(data) + 16)
        assert code == BUF_ERROR and rp["stop"] == TRUNCATED and rp["blocks_delivered"] == whole, (cut, code, rp)
        assert got == data[: whole * BS], cut
        r, ref, _, _ = fw.stream_decode(L, raw[:cut], len(data) + 16)
        assert r == BUF_ERROR and ref[: len(got)] == got and len(ref) >= len(got), (cut, r)


def test_truncated_single_block_stream_delivers_nothing_until_it_is_whole(enc):
    data = o.corpus_mixed(4 * BS, 78)
    raw = _own(enc, data, 1, single=True)
    index_size = x.index_size(raw)
    end = len(raw) - 12 - index_size                 # where the Block ends
    for cut in (5, 11, 12, 15, end // 3, end // 2, end - 1, end, end + 1, end + 2, len(raw) - 1):
        code, got, rp = _forward(enc, raw[:cut], len(data) + 16)
        assert code == BUF_ERROR and rp["stop"] == TRUNCATED, (cut, code, rp)
        assert rp["blocks_delivered"] == (cut >= end) and got == (data if cut >= end else b""), cut


# ---------------------------------------------------------------- 6. damage
def test_damage_delivers_the_blocks_in_front_of_it(enc, ref, four):
    raw, data, blocks = four
    L = ref
    h = [b["header_offset"] for b in blocks]
    index_at = h[3] + blocks[3]["total_size"]
    cases = {"payload of Block 2": (h[2] + blocks[2]["total_size"] // 2, 2),
             "stored Check of Block 1": (h[2] - 1, 1),
             "Index": (index_at + 3, 4)}
    for name, (at, whole) in cases.items():
        bad = bytearray(raw)
        bad[at] ^= 0x20
        code, got, rp = _forward(enc, bad, len(data) + 16)
        assert code == DATA_ERROR and rp["blocks_delivered"] == whole and got == data[: whole * BS], (name, code, rp)
        assert rp["stop_offset"] == (h[whole] if whole < 4 else index_at), name
        r, ref, _, _ = fw.stream_decode(L, bytes(bad), len(data) + 16)
        assert r == DATA_ERROR and ref[: len(got)] == got, name
        assert _backward_code(enc, bad, len(data) + 16) == DATA_ERROR, name


def test_an_output_that_is_too_small_delivers_the_blocks_that_fit(enc, ref, four):
    raw, data, _ = four
    code, got, rp = _forward(enc, raw, 2 * BS + 100)
    assert code == BUF_ERROR and rp["stop"] == OUT_FULL and rp["blocks_delivered"] == 2 and got == data[: 2 * BS]


def test_without_concatenated_the_read_ends_behind_the_first_stream(enc, ref, four):
    raw, data, _ = four
    code, got, rp = _forward(enc, raw + b"\0" * 4 + raw, 2 * len(data) + 16, concatenated=False)
    assert code == 0 and got == data and rp["consumed"] == len(raw) and rp["streams"] == 1
    code, got, rp = _forward(enc, raw + b"\0" * 4 + raw, 2 * len(data) + 16)
    assert code == 0 and got == data + data and rp["streams"] == 2


# ---------------------------------------------------------------- 7. reads and launches
def test_reads_and_launches_do_not_grow_with_the_blocks(enc, ref):
    import xz_amd
    bs = 16384
    d64 = o.corpus_mixed(64 * bs - 5, 79)
    one = o.ref_encode_mt(d64[:bs], 1, block_size=bs)
    many = o.ref_encode_mt(d64, 1, block_size=bs)
    counts = {}
    for name, raw, data, nblocks in (("1", one, d64[:bs], 1), ("64", many, d64, 64), ("2 streams", one + many, d64[:bs] + d64, 65),
                                     ("3 streams", one + many + b"\0" * 8 + one, d64[:bs] + d64 + d64[:bs], 66)):
        code, got, rp = _forward(enc, raw, len(data) + 16)
        assert code == 0 and got == data and rp["blocks_delivered"] == nblocks
        counts[name] = xz_amd.Encoder.debug_forward_counters()
        assert counts[name][2] == nblocks
    assert counts["1"][:2] == counts["64"][:2] and counts["1"][3] == counts["64"][3] == 1, counts
    assert counts["1"][0] > 0 and counts["1"][1] > 0
    # what a Stream adds: the same from the second to the third as from the first to the second, one walk each
    r1, r2, r3 = (counts[k][0] for k in ("64", "2 streams", "3 streams"))
    assert 0 < r2 - r1 == r3 - r2, counts
    l1, l2, l3 = (counts[k][1] for k in ("64", "2 streams", "3 streams"))
    assert 0 < l2 - l1 == l3 - l2, counts
    assert [counts[k][3] for k in ("64", "2 streams", "3 streams")] == [1, 2, 3], counts
