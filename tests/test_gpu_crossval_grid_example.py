"""examples/crossval_grid_synthetic.py (the whole grid of one graph of old/h_o_train.py's sweep: 2 dropout values x 2 learning
rates x KFold(3) as one network with a dropout rate per member) runs end to end in a fresh process at its small default
size and prints one F1 mean and standard deviation per (dropout, rate) cell."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_trains_the_grid_as_one_network(cuda):
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "crossval_grid_synthetic.py")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0, out[-3000:]
    rows = re.findall(r"^member (\d+): do ([\d.]+) lr ([\d.e-]+) split (\d), first loss\s+([-\d.naninf]+), final loss\s+"
                      r"([-\d.naninf]+)", out, flags=re.M)
    assert [int(r[0]) for r in rows] == list(range(12)), out[-3000:]
    assert [(float(r[1]), float(r[2]), int(r[3])) for r in rows] == \
        [(do, lr, f) for do in (0.5, 0.7) for lr in (0.01, 0.05) for f in range(3)]
    for k, _, _, _, first, last in rows:
        assert math.isfinite(float(first)) and math.isfinite(float(last)), (k, first, last)
    table = re.findall(r"^LR ([\d.e-]+) DO ([\d.]+) max_df 0.7 GCN: mean f1 ([\d.]+) std f1 ([\d.]+)", out, flags=re.M)
    assert [(float(do), float(lr)) for lr, do, _, _ in table] == [(do, lr) for do in (0.5, 0.7) for lr in (0.01, 0.05)]
    assert all(0.0 <= float(m) <= 1.0 and float(s) >= 0.0 for _, _, m, s in table), out[-1500:]
    assert "dropout [0.5, 0.7]" in out
