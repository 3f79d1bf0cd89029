"""examples/perlevel_mlp_synthetic.py (MLP_level.py's loop on a synthetic two-level corpus) runs end to end in a fresh
process, on a small corpus and under a time limit."""
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_end_to_end(cuda):
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "perlevel_mlp_synthetic.py"),
                          "--docs", "600", "--epochs", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("test accuracy:")]
    assert line, res.stdout[-3000:]
    acc, f1 = float(line[-1].split()[2]), float(line[-1].split()[-1])
    assert math.isfinite(acc) and math.isfinite(f1) and 0.0 <= acc <= 1.0 and 0.0 <= f1 <= 1.0
    # the level-2 model ran on the plans the level-1 model built
    assert "feature plans built for level 2: 0" in res.stdout, res.stdout[-3000:]
    assert "the base tensor is x_train itself: True" in res.stdout
