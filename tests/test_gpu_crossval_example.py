"""examples/crossval_synthetic.py (one cell of old/h_o_train.py's sweep: 4 learning rates x KFold(3) as one network) runs end
to end in a fresh process, on a small corpus and under a time limit, and every member's training loss falls."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_trains_every_member(cuda):
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "crossval_synthetic.py"),
                          "--docs", "600", "--epochs", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0, out[-3000:]
    rows = re.findall(r"^member (\d+): lr ([\d.e-]+) split (\d), first loss\s+([-\d.naninf]+), final loss\s+([-\d.naninf]+)", out,
                      flags=re.M)
    assert [int(r[0]) for r in rows] == list(range(12)), out[-3000:]
    assert sorted({float(r[1]) for r in rows}) == [0.001, 0.005, 0.01, 0.05] and {r[2] for r in rows} == {"0", "1", "2"}
    for k, _, _, first, last in rows:
        assert math.isfinite(float(first)) and float(last) < float(first), (k, first, last)
    per_epoch = re.findall(r"^\[\s*(\d+)\] lr [\d.e-]+ split \d: loss:\s+[-\d.]+, val_loss:\s+[-\d.]+, training accuracy:\s+[\d.]+, "
                           r"val_f1:\s+[\d.]+", out, flags=re.M)
    assert len(per_epoch) == 5 * 12, out[-3000:]                        # a line per epoch and member
    table = re.findall(r"^LR ([\d.e-]+) DO 0.5 max_df 0.7 GCN: mean f1 ([\d.]+) std f1 ([\d.]+)", out, flags=re.M)
    assert len(table) == 4 and all(0.0 <= float(m) <= 1.0 and float(s) >= 0.0 for _, m, s in table), out[-1500:]
