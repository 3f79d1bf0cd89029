"""examples/crossval_scoreboard_synthetic.py (the grid of crossval_grid_synthetic.py scored on the device, one
`Scoreboard.to_host()` for the whole run) runs end to end in a fresh process: one line per epoch and member, a result table
with values in [0, 1], and a final F1 per member equal to sklearn's on the predictions the run dumps."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _metrics_cases as MC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_scores_the_grid_on_the_device(cuda, tmp_path):
    dump = str(tmp_path / "run.npz")
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                          os.path.join(ROOT, "examples", "crossval_scoreboard_synthetic.py"), "--docs", "600", "--epochs", "5",
                          "--dump", dump], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    out = res.stdout
    assert res.returncode == 0, out[-3000:]
    num = r"\s*([-\d.naninf]+)"
    lines = re.findall(r"^\[(\d+)\] do ([\d.]+) lr ([\d.e-]+) split (\d): loss:" + num + ", val_loss:" + num
                       + ", training accuracy:" + num + ", val_f1:" + num, out, flags=re.M)
    grid = [(do, lr, f) for do in (0.5, 0.7) for lr in (0.01, 0.05) for f in range(3)]
    assert [(int(e), float(do), float(lr), int(f)) for e, do, lr, f, *_ in lines] == \
        [(e + 1,) + cell for e in range(5) for cell in grid], out[-3000:]
    for *_, loss, val_loss, acc, f1 in lines:
        assert np.isfinite(float(loss)) and np.isfinite(float(val_loss)) and 0.0 <= float(acc) <= 1.0 and 0.0 <= float(f1) <= 1.0
    table = re.findall(r"^LR ([\d.e-]+) DO ([\d.]+) max_df 0.7 GCN: mean f1 ([\d.]+) std f1 ([\d.]+)", out, flags=re.M)
    assert [(float(do), float(lr)) for lr, do, _, _ in table] == [(do, lr) for do in (0.5, 0.7) for lr in (0.01, 0.05)]
    assert all(0.0 <= float(m) <= 1.0 and 0.0 <= float(s) <= 1.0 for _, _, m, s in table), out[-1500:]
    z = np.load(dump)
    K = z["pred"].shape[1]
    assert K == 12
    for k in range(K):
        val = ((z["val_bits"] >> k) & 1).astype(bool)
        train = ((z["train_bits"] >> k) & 1).astype(bool)
        assert val.any() and MC.close(z["val_f1"][k], MC.sklearn_scores(z["y"][val], z["pred"][val, k])[1])
        assert MC.close(z["train_accuracy"][k], MC.sklearn_scores(z["y"][train], z["pred"][train, k])[0])
    cells = z["val_f1"].reshape(4, 3)
    for (_, _, m, s), c in zip(table, cells):
        assert abs(float(m) - c.mean()) <= 5.1e-4 and abs(float(s) - c.std()) <= 5.1e-4         # three printed decimals
