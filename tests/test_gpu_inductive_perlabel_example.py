"""examples/inductive_perlabel_synthetic.py runs end to end in a fresh process on a small corpus, under a time limit, and
prints top-label accuracy, routed accuracy and macro-F1 for the held-out documents (`FoldInPerLabel`).  The example reports;
no figure is asserted beyond being a share."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_prints_the_scores_of_the_held_out_documents(cuda):
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                          os.path.join(ROOT, "examples", "inductive_perlabel_synthetic.py"), "--docs", "600", "--epochs", "5"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0, out[-3000:]
    m = re.findall(r"^held-out documents: top-label accuracy ([\d.]+), routed accuracy ([\d.]+), macro-F1 ([\d.]+)", out,
                   flags=re.M)
    assert len(m) == 1, out[-3000:]
    assert all(0.0 <= float(v) <= 1.0 for v in m[0])
    assert re.search(r"^routed by the true top label: accuracy ([\d.]+)", out, flags=re.M), out[-3000:]
    assert re.search(r"^\s+60 new documents, \d+ known words", out, flags=re.M), out[-3000:]
