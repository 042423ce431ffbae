"""Seeded option/data fuzz of the HIP path against the oracle and the real reference decoder
(tools/gpu_fuzz.py): presets, span sizes, custom depths / nice_len / dictionary / lc-lp-pb, BCJ, checks."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [11, 12])
def test_fuzz_against_oracle(seed):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_fuzz.py"), str(seed), "40"],
                       capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"FUZZ seed {seed}: 40 / 40 ok" in p.stdout


@pytest.mark.parametrize("seed", [23, 24])
def test_fuzz_composite_against_oracle(seed):
    """gpu_fuzz.py --composite: the data of every case is a composite Block input (tests/_composite.py: draw), the options
    are drawn as in the plain mode.  A case is ok when the Stream equals the oracle's and every Block is either valid
    (chunk walker, reference decoder) or the stored-prefix defect, named by verify_blocks; at most 3 known-defect cases per
    seed.  The seeds were chosen with the oracle alone on the CPU (seeds 21..36 looked at, 24 cases each): seed 23 has
    one known-defect case (case 5: preset 6e, Blocks of 1 MiB, r300000+p1+t400000+z100000+l5), seed 24 has none, and no
    seed showed any other invalid Block."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_fuzz.py"), str(seed), "24", "--composite"],
                       capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    last = [ln for ln in p.stdout.splitlines() if ln.startswith(f"FUZZ composite seed {seed}: ")]
    assert len(last) == 1 and last[0].startswith(f"FUZZ composite seed {seed}: 24 / 24 ok, "), p.stdout[-4000:]
    known = int(last[0].split(" ok, ")[1].split(" known-defect")[0])
    print(last[0])
    assert known <= 3
