"""examples/inductive_synthetic.py runs end to end in a fresh process on a small corpus, under a time limit, and prints both
accuracies: transductive (held-out documents inside the graph) and fold-in (the same documents outside it).  The example
reports; neither figure is asserted beyond being a share."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_prints_both_accuracies(cuda):
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "inductive_synthetic.py"),
                          "--docs", "600", "--epochs", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0, out[-3000:]
    trans = re.findall(r"^transductive test accuracy: ([\d.]+)", out, flags=re.M)
    fold = re.findall(r"^fold-in accuracy:\s+([\d.]+)", out, flags=re.M)
    assert len(trans) == 1 and len(fold) == 1, out[-3000:]
    assert 0.0 <= float(trans[0]) <= 1.0 and 0.0 <= float(fold[0]) <= 1.0
    assert re.search(r"^\s+60 new documents, \d+ known words", out, flags=re.M), out[-3000:]
