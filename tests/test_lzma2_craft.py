"""Crafted LZMA2 symbol streams (tests/_lzma2_craft.py) against their golden record and the CPU decoders.

The golden file tests/golden/lzma2_craft.json holds what the REAL liblzma said about every case (return code, size and
SHA-256 of its output).  Here, without a GPU:
  * the generator is deterministic: it writes the very Streams the golden record was made from;
  * with oracle/_ref built, the live reference agrees with the record on every case;
  * the project's own CPU decoder (oracle/lzma2_dec.c) gives the recorded verdict for every case and the recorded bytes
    for every accepted one -- a third implementation, and the oracle other tests trust.
tests/test_gpu_decode_craft.py feeds the same cases to the device decoder.
"""
import collections
import hashlib
import json
import os

import pytest

import _lzma2_craft as craft
import _oracle as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzma2_craft.json")
SLACK = 4096


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_case_list_is_the_recorded_one(golden):
    cases = craft.cases()
    assert sorted(c.name for c in cases) == sorted(golden)
    for c in cases:
        g = golden[c.name]
        assert hashlib.sha256(c.stream()).hexdigest() == g["stream_sha256"], c.name
        assert (g["section"], g["seed"], g["intent"], g["record_only"]) == (c.section, c.seed, c.intent, c.record_only), c.name


def test_sections_are_complete(golden):
    cases = craft.cases()
    per = collections.Counter(c.section for c in cases)
    geom = {c.name for c in cases if c.name.startswith("A-geom-")}
    assert len(geom) == 75 and per["G"] >= 200 and set(per) == set("ABCDEFG")
    pairs = [c for c in cases if c.name.startswith("B-pair-")]
    assert len(pairs) == 34
    assert sum(1 for c in cases if c.record_only) == 2
    # the reference agrees with the intent wherever the verdict is not merely recorded, and a third of all cases is accepted
    for c in cases:
        if not c.record_only:
            assert (golden[c.name]["ret"] == 1) == (c.intent == "accept"), c.name
    assert 3 * sum(1 for g in golden.values() if g["ret"] == 1) >= len(cases)
    # the two size extremes of a chunk are what they claim to be
    by = {c.name: c for c in cases}
    assert by["C-max-usize-chunk"].payload[:3] == b"\xFF\xFF\xFF"
    assert by["C-max-csize-chunk"].payload[3:5] == b"\xFF\xFF"


def test_accepted_cases_decode_to_the_intended_plaintext(golden):
    for c in craft.cases():
        g = golden[c.name]
        if g["ret"] == 1 and not c.record_only:
            assert (len(c.plain), hashlib.sha256(c.plain).hexdigest()) == (g["size"], g["sha256"]), c.name


def test_live_reference_agrees_with_the_golden_record(golden):
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    for c in craft.cases():
        g = golden[c.name]
        ret, out = o.ref_decode(c.stream(), c.usize + SLACK)
        assert ret == g["ret"], c.name
        if ret == 1:
            assert (len(out), hashlib.sha256(out).hexdigest()) == (g["size"], g["sha256"]), c.name


def test_cpu_decoder_gives_the_golden_verdict_and_bytes(golden):
    for c in craft.cases():
        g = golden[c.name]
        r, out, nb = o.orc_xz_decode(c.stream(), c.usize + SLACK)
        assert (r == 0) == (g["ret"] == 1), (c.name, r)
        if r == 0:
            assert nb == 1 and (len(out), hashlib.sha256(out).hexdigest()) == (g["size"], g["sha256"]), c.name
        if "block-usize" in c.name:
            continue                    # (the Block's declared size: nothing the raw decoder sees)
        r, out = o.orc_decode_raw(c.payload, c.dict_size, c.usize + SLACK)
        assert (r == 0) == (g["ret"] == 1), (c.name, r)
        if r == 0:
            assert (len(out), hashlib.sha256(out).hexdigest()) == (g["size"], g["sha256"]), c.name


def test_bare_chains_have_the_verdict_the_gpu_test_expects(golden):
    """a case as a bare chunk chain (no end marker): with the marker put back, the CPU decoder -- and the live reference
    where it is built -- accept exactly the chains the device test expects to be good"""
    for c in craft.cases():
        if "block-usize" in c.name:
            continue
        ok = golden[c.name]["ret"] == 1 if c.chain_intent == c.intent else c.chain_intent == "accept"
        r, out = o.orc_decode_raw(c.chain + b"\0", c.dict_size, c.usize + SLACK)
        assert (r == 0 and len(out) == c.usize) == ok, (c.name, r)
        if ok:
            assert out == c.plain, c.name
        if o.have_ref():
            r, out = o.ref_raw_decode(c.chain + b"\0", c.dict_size, c.usize + SLACK)
            assert (r == 1 and len(out) == c.usize) == ok, (c.name, r)
