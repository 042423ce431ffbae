#!/usr/bin/env python3
"""Regenerates tests/golden/lzma2_craft.json (needs oracle/_ref, the real reference liblzma).

Every crafted case of tests/_lzma2_craft.py is framed as a one-Block Stream with Check none and decoded by the real
liblzma.  Recorded per case: the library's return code, size and SHA-256 of what it wrote, the SHA-256 of the Stream it
judged, and the verdict the case was built for; per multi-Block Stream of the forward-decode test the return code and
the bytes in front of the defect.  The file holds results only.

The reference must agree with the intent of every case (the two "distance = dictionary size" cases excepted: there
liblzma versions differ, so its verdict is simply recorded): a disagreement is a bug of the generator and stops this
script.  At least a third of the cases must be accepted ones.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _lzma2_craft as craft  # noqa: E402
import _oracle as o  # noqa: E402

LZMA_STREAM_END = 1
SLACK = 4096


def judge(case):
    """what the reference says about the case: (return code, bytes written)"""
    return o.ref_decode(case.stream(), case.usize + SLACK)


def record(case, ret, out):
    return {"section": case.section, "seed": case.seed, "intent": case.intent, "record_only": case.record_only,
            "stream_sha256": hashlib.sha256(case.stream()).hexdigest(), "ret": ret, "size": len(out),
            "sha256": hashlib.sha256(out).hexdigest()}


def main():
    assert o.have_ref(), "needs oracle/_ref (the real reference build)"
    cases = craft.cases()
    man = {"reference_version": o.ref().ref_version().decode(), "cases": {}}
    wrong = []
    for c in cases:
        ret, out = judge(c)
        accepted = ret == LZMA_STREAM_END
        if not c.record_only:
            if accepted != (c.intent == "accept") or (accepted and out != c.plain):
                wrong.append((c.name, c.intent, ret, len(out)))
        man["cases"][c.name] = record(c, ret, out)
    assert not wrong, "the reference disagrees with the intent (a generator bug): %r" % wrong
    man["forward"] = {}
    for name in craft.FORWARD_CASES:
        raw, front = craft.forward_stream(name)
        ret, out = o.ref_decode(raw, len(front) + 65536)
        assert ret != LZMA_STREAM_END and out[:len(front)] == front, name
        man["forward"][name] = {"stream_sha256": hashlib.sha256(raw).hexdigest(), "ret": ret, "front_size": len(front),
                                "front_sha256": hashlib.sha256(front).hexdigest()}
    naccept = sum(1 for r in man["cases"].values() if r["ret"] == LZMA_STREAM_END)
    assert 3 * naccept >= len(cases), (naccept, len(cases))
    with open(os.path.join(HERE, "lzma2_craft.json"), "w") as f:
        json.dump(man, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d cases (%d accepted) judged by liblzma %s" % (len(cases), naccept, man["reference_version"]))


if __name__ == "__main__":
    main()
