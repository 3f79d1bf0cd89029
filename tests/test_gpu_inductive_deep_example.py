"""examples/inductive_deep_synthetic.py runs end to end in a fresh process on a small corpus, under a time limit, and prints
for the JumpingKnowledgeNetwork and for the three-layer GCN the fold-in accuracy and the agreement of `FoldInDeep` with the
model's own forward on the extended graph.  The logits agree at BASELINE's bar; the accuracy is reported, not asserted beyond
being a share."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_prints_accuracy_and_agreement_for_both_models(cuda):
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "inductive_deep_synthetic.py"),
                          "--docs", "600", "--epochs", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0, out[-3000:]
    assert re.search(r"60 new documents, \d+ known words", out), out[-3000:]
    for name in (r"JumpingKnowledgeNetwork\(n_gcn=2\)", r"GCN\(n_gcn=3\)"):
        acc = re.findall(rf"^{name}: fold-in accuracy ([\d.]+)", out, flags=re.M)
        agree = re.findall(rf"^{name}: agreement with the full forward on the extended graph ([\d.]+), largest relative "
                           r"difference of the\s+logits ([\d.e+-]+)", out, flags=re.M)
        assert len(acc) == 1 and len(agree) == 1, out[-3000:]
        assert 0.0 <= float(acc[0]) <= 1.0 and 0.0 <= float(agree[0][0]) <= 1.0
        assert float(agree[0][1]) <= 1e-5, out[-3000:]
