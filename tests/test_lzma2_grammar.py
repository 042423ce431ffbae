"""The independent LZMA2 chunk walker (tests/_lzma2_grammar.py) against the reference, not against this project's encoder.

* The crafted cases of tests/_lzma2_craft.py with the golden record of what liblzma said about them
  (tests/golden/lzma2_craft.json): every accepted case passes the decoder rules (a); every rejected case whose step is
  "grammar" fails them; every rejected case whose step is "decode" passes them (its fault lies in the range-coded bits).
  The two "block-usize" cases are rejected for the Block Header's size field, which no LZMA2 decoder sees: they pass (a)
  and trip the sum rule of (b) -- the only rule that knows the Block's size.
* Streams of the reference's own encoder pass (a) and (b), incompressible and mixed data included.
"""
import json
import os

import numpy as np
import pytest

import _composite as cp
import _lzma2_craft as craft
import _lzma2_grammar as g
import _oracle as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzma2_craft.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_blocks_of_cuts_the_payload_out(golden):
    for c in craft.cases():
        blocks = g.blocks_of(c.stream())
        assert len(blocks) == 1 and blocks[0].payload == c.payload, c.name


def test_walker_agrees_with_the_reference_on_the_crafted_cases(golden):
    seen = {"accept": 0, "grammar": 0, "decode": 0}
    for c in craft.cases():
        accepted = golden[c.name]["ret"] == 1
        w = g.walk(c.payload, c.usize)
        if accepted:
            assert w.decoder_ok, (c.name, w)
            seen["accept"] += 1
        elif c.record_only:
            continue                        # (no step claimed: the verdict was whatever the reference said)
        elif c.step == "grammar":
            if "block-usize" in c.name:
                assert w.decoder_ok and w.convention_error is not None and "add up" in w.convention_error[1], (c.name, w)
            else:
                assert not w.decoder_ok, (c.name, w)
            seen["grammar"] += 1
        else:
            assert c.step == "decode" and w.decoder_ok, (c.name, w)
            seen["decode"] += 1
    print("cases", seen)
    assert seen["accept"] >= 300 and seen["grammar"] >= 15 and seen["decode"] >= 15


def test_accepted_crafted_cases_account_for_their_plaintext(golden):
    """the chunk sizes the walker reads add up to the recorded output size of every accepted case"""
    for c in craft.cases():
        if golden[c.name]["ret"] == 1:
            w = g.walk(c.payload)
            assert sum(k.usize for k in w.chunks) == golden[c.name]["size"], c.name


def test_hand_made_payloads():
    lit = bytes([0xE0, 0, 0, 0, 5, 0x5D]) + bytes(6)                                # one LZMA chunk: 1 byte from 6
    raw = lambda ctl, n: bytes([ctl, (n - 1) >> 8, (n - 1) & 0xFF]) + bytes(n)
    assert g.walk(lit + b"\0", 1).ok
    assert g.walk(raw(1, 70) + raw(2, 65536) + b"\0", 70 + 65536).ok
    assert g.walk(b"\0", 0).ok
    bad = {
        "first chunk 0x02": raw(2, 5) + b"\0",
        "first chunk 0xC0": bytes([0xC0]) + lit[1:] + b"\0",
        "control 0x03": raw(1, 5) + raw(3, 5) + b"\0",
        "control 0x7F": raw(1, 5) + raw(0x7F, 5) + b"\0",
        "0x80 in front of properties": raw(1, 5) + bytes([0x80, 0, 0, 0, 5]) + bytes(6) + b"\0",
        "0xA0 in front of properties": raw(1, 5) + bytes([0xA0, 0, 0, 0, 5]) + bytes(6) + b"\0",
        "properties byte 225": lit[:5] + bytes([225]) + bytes(6) + b"\0",
        "lc + lp = 5": lit[:5] + bytes([4 + 9 * 1]) + bytes(6) + b"\0",
        "no end marker": lit,
        "bytes behind the end marker": lit + b"\0\0",
        "chunk past the payload": lit[:-1],
        "header past the payload": lit + bytes([0x80, 0]),
    }
    for name, p in bad.items():
        assert not g.walk(p).decoder_ok, name
    # the reference decoder says the same of every one of them
    if o.have_ref():
        for name, p in bad.items():
            assert o.ref_raw_decode(p, 1 << 20, 1 << 17)[0] != 1, name
        assert o.ref_raw_decode(raw(1, 70) + raw(2, 65536) + b"\0", 1 << 20, 1 << 17)[0] == 1
    # the defect's shape, and shapes that are not it
    w = g.walk(bad["0xA0 in front of properties"])
    assert g.is_stored_prefix_defect(w) and g.verdict(w) == g.DEFECT
    assert g.verdict(g.walk(raw(1, 5) + bytes([0xBF, 0, 0, 0, 5]) + bytes(6) + b"\0")) == g.DEFECT          # low bits: size
    assert g.verdict(g.walk(bad["0x80 in front of properties"])) == g.INVALID
    assert g.verdict(g.walk(bytes([0xA0]) + lit[1:5] + bytes(6) + b"\0")) == g.INVALID                       # nothing stored in front
    assert g.verdict(g.walk(lit + raw(1, 5) + bytes([0xA0, 0, 0, 0, 5]) + bytes(6) + b"\0")) == g.INVALID    # not the first LZMA chunk
    # (b) alone: valid for a decoder, not what an encoder promises
    w = g.walk(lit + raw(2, 5) + bytes([0x80, 0, 0, 0, 5]) + bytes(6) + b"\0", 7)
    assert w.decoder_ok and not w.ok and w.convention_error[0] == 2
    assert g.verdict(w) == g.INVALID
    w = g.walk(lit + b"\0", 2)
    assert w.decoder_ok and not w.ok


def _kinds():
    rng = np.random.default_rng(3)
    return {
        "random": rng.integers(0, 256, 300000, dtype=np.uint8).tobytes(),
        "lorem": o.corpus_lorem(400000),
        "mixed": o.corpus_mixed(500000, 7),
        "random+text": cp.named("r320k+t"),
        "alternating": cp.named("alternate-3"),
        "tiny": b"a",
    }


@pytest.mark.parametrize("preset", [0, 1, 6, 9 | 0x80000000])
def test_streams_of_the_reference_encoder_pass_both_rule_sets(preset):
    if not o.have_ref():
        pytest.skip("oracle/_ref not built")
    for name, data in _kinds().items():
        for bs in (0, 100000):
            xz = o.ref_encode_mt(data, preset, block_size=bs)
            blocks = g.blocks_of(xz)
            assert sum(b.uncompressed_size for b in blocks) == len(data)
            if bs:
                assert len(blocks) == (len(data) + bs - 1) // bs
            for k, b in enumerate(blocks):
                w = g.walk(b.payload, b.uncompressed_size)
                assert w.ok, (name, preset, bs, k, w)
            if name == "random":
                assert all(c.kind == g.STORED for b in blocks for c in g.walk(b.payload).chunks)
