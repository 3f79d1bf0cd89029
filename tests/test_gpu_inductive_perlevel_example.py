"""examples/inductive_perlevel_synthetic.py runs end to end in a fresh process on a small corpus, under a time limit, and
prints level-1 and final accuracy for the in-graph test split and for the held-out documents (`FoldInLevels`).  The example
reports; no figure is asserted beyond being a share."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_prints_the_accuracies_of_both_levels(cuda):
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                          os.path.join(ROOT, "examples", "inductive_perlevel_synthetic.py"), "--docs", "600", "--epochs", "5"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0, out[-3000:]
    for who in ("in-graph test split:", "held-out documents: "):
        m = re.findall(rf"^{who}\s+level 1 accuracy ([\d.]+), final accuracy ([\d.]+)", out, flags=re.M)
        assert len(m) == 1, out[-3000:]
        assert all(0.0 <= float(v) <= 1.0 for v in m[0])
    assert re.search(r"^\s+60 new documents, \d+ known words", out, flags=re.M), out[-3000:]
