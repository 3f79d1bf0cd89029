"""CPU tests of the device-side scores (pytextgcn_amd/metrics.py, csrc/metrics.hip): the numpy restatement of the class
counts and scores in tests/_metrics_cases.py against sklearn's `f1_score(average="macro")` and `accuracy_score`, the
coverage of the case list the GPU tests run, the exported symbols and the argument errors the library returns before
anything is enqueued -- so on a host without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _metrics_cases as MC
from pytextgcn_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tgcn_class_counts_members", "tgcn_class_counts_groups", "tgcn_class_scores", "tgcn_class_counts_workspace_bytes"]


@pytest.mark.parametrize("key", [k for k, c in MC.CASES.items() if c["n"] <= 4 * MC.R and not c["oob_pred"]])
def test_numpy_restatement_equals_sklearn(key):
    """accuracy and macro-F1 from (tp, n_pred, n_true) within 1e-12 of sklearn on the selected rows, member by member (at
    most 256 members' classes are asked of sklearn per case: it takes milliseconds per call)."""
    ops = MC.operands(key)
    c = ops["case"]
    for s, counts in enumerate(ops["expected"]):
        got = MC.scores_np(counts)
        for k in list(range(c["K"]))[:6] + list(range(c["K"]))[-2:]:
            t, p = MC.selected_rows(ops, s, k)
            assert got[k, 2] == t.size
            if t.size == 0:
                assert np.isnan(got[k, 0]) and np.isnan(got[k, 1]) and got[k, 3] == 0 and not counts[k].any()
                continue
            acc, f1 = MC.sklearn_scores(t, p)
            assert MC.close(got[k, 0], acc) and MC.close(got[k, 1], f1), (key, s, k, got[k], acc, f1)
            assert got[k, 3] == np.union1d(t, p).size


def test_random_cases_against_sklearn():
    rng = np.random.default_rng(5)
    for C in (1, 2, 3, 8, 70, 219):
        for n in (1, 7, 400, 5000):
            t, p = rng.integers(0, C, n), rng.integers(0, C, n)
            got = MC.scores_np(MC.counts_groups(p, t, np.ones(n, dtype=bool), 1, C))
            acc, f1 = MC.sklearn_scores(t, p)
            assert MC.close(got[0, 0], acc) and MC.close(got[0, 1], f1), (C, n)


def test_hand_counted_case_with_predictions_outside_the_classes():
    h = MC.HAND
    counts = MC.counts_groups(h["pred"], h["target"], np.ones(5, dtype=bool), 1, 3)
    assert np.array_equal(counts, h["counts"])
    assert MC.close(MC.scores_np(counts), h["scores"])


def test_case_list_covers_what_the_kernels_branch_on():
    mem = [c for c in MC.MEMBER_CASES]
    R, CAP, LDS = MC.R, MC.CAP, MC.LDS
    assert {1, 2, 63, 64} <= {c["K"] for c in mem} and {1, 2, 3, 8, 219, 4096} <= {c["C"] for c in mem}
    assert {0, 1, 63, 64, 65, R - 1, R, R + 1, CAP * R + 1} <= {c["n"] for c in mem}
    assert any(c["n"] == CAP * R + 1 and c["K"] == 1 and c["C"] == 2 for c in mem)
    assert all(c["ldp"] > c["K"] for c in mem) and any(not c["two"] for c in mem) and any(c["oob_pred"] for c in mem)
    assert any((c["K"], c["C"]) == (64, 219) for c in mem)
    table = lambda c: (2 if c["two"] else 1) * c["K"] * 3 * c["C"] * 4
    for two in (True, False):                        # a (K, C) pair on each side of the LDS budget, as near as C allows
        sizes = [table(c) for c in mem if c["two"] == two and c["K"] == 64]
        assert LDS in sizes and any(LDS < s <= LDS + 2 * 64 * 12 for s in sizes)
    grp = MC.GROUP_CASES
    assert any(not c["group"] for c in grp) and any(c["widths"] == (1, 3, 8) and c["offset"] for c in grp)
    assert any(c["widths"] == (1, 3, 8) and not c["offset"] for c in grp) and any(not c["two"] for c in grp)
    for key in MC.CASES:                             # what a case promises is in its operands
        ops, c = MC.operands(key), MC.CASES[key]
        if c["form"] == "members" and c["n"] >= 63:
            a, b = ops["sets"][0], ops["sets"][-1]
            low = np.uint64((1 << c["K"]) - 1)
            if c["two"]:
                assert ((a & b & low) != 0).any() and (((a & low) != 0) & ((b & low) == 0)).any()
            none = ((a | b) & low) == 0
            assert none.any() and ((ops["target"][none] < 0) | (ops["target"][none] >= c["C"])).all()
            if c["K"] < 64:
                assert ((a >> np.uint64(c["K"])) != 0).all()
            if c["empty_member"]:
                assert not ops["expected"][0][ops["empty"]].any() and ops["expected"][0][0].any()
            if c["K"] == 64:                            # bit 63, the sign bit of the int64 the bits travel in, selects rows
                assert (a.view(np.int64) < 0).any() and ops["expected"][0][63].any()
            if 3 <= c["C"] <= 8 and c["n"] >= 200:      # a class in the predictions only, one in the targets only
                tp, n_pred, n_true = ops["expected"][0].sum(0)
                assert n_pred[-1] > 0 and n_true[-1] == 0 and n_true[-2] > 0 and n_pred[-2] == 0
        if c["form"] == "groups" and c["group"] and c["n"] > 63:
            assert (ops["group"] == -1).any()


def test_python_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "tgcn.h")).read()
    macro = lambda name: int(re.search(rf"#define TGCN_CLASS_COUNTS_{name} (\d+)", text).group(1))
    assert metrics.ROWS_PER_WORKGROUP == macro("ROWS_PER_WORKGROUP") and metrics.WORKGROUP_CAP == macro("WORKGROUP_CAP")
    assert metrics.LDS_BUDGET_BYTES == macro("LDS_BYTES") <= 64 * 1024
    assert metrics.PARTIAL_BUDGET_BYTES == macro("PARTIAL_BYTES") and metrics.MAX_CLASSES == macro("MAX_CLASSES") == 4096


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s) and re.fullmatch(r"tgcn_[a-z_]+", s)
    assert lib.tgcn_abi_version() == 7


def test_workspace_bytes():
    lib = _lib.load()
    ws = lib.tgcn_class_counts_workspace_bytes
    R, CAP = metrics.ROWS_PER_WORKGROUP, metrics.WORKGROUP_CAP
    per = lambda K, C: 2 * K * 3 * C * 4
    assert ws(0, 2, 3) == 0 and ws(1, 2, 3) == per(2, 3) and ws(R + 1, 2, 3) == 2 * per(2, 3)
    assert ws(CAP * R + 1, 1, 2) == CAP * per(1, 2) == ws((1 << 31) - 1, 1, 2)
    assert ws(10 ** 6, 64, 4096) == (metrics.PARTIAL_BUDGET_BYTES // per(64, 4096)) * per(64, 4096)
    for bad in [(-1, 2, 3), (1 << 31, 2, 3), (5, 0, 3), (5, 65, 3), (5, 2, 0), (5, 2, 4097)]:
        assert ws(*bad) == 0


def test_argument_errors_do_not_need_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()                       # host memory: an invalid call returns before it touches a pointer
    p = ctypes.addressof(buf)
    members = lambda pred=p, ldp=2, target=p, a=p, b=p, n=8, K=2, C=3, ca=p, cb=p, ws=p, wsb=1 << 20: \
        lib.tgcn_class_counts_members(pred, ldp, target, a, b, n, K, C, ca, cb, ws, wsb, None)
    groups = lambda pred=p, off=p, target=p, group=p, a=p, b=p, n=8, K=2, C=3, ca=p, cb=p, ws=p, wsb=1 << 20: \
        lib.tgcn_class_counts_groups(pred, off, target, group, a, b, n, K, C, ca, cb, ws, wsb, None)
    for call in (members, groups):
        for kw in (dict(K=0), dict(K=65), dict(C=0), dict(C=4097), dict(n=-1), dict(n=1 << 31), dict(pred=None),
                   dict(target=None), dict(a=None), dict(ca=None), dict(b=None), dict(cb=None)):
            assert call(**kw) == _lib.E_INVALID, kw
            assert lib.tgcn_last_error()
        assert call(ws=None) == _lib.E_WORKSPACE and call(wsb=16) == _lib.E_WORKSPACE
    assert members(ldp=1) == _lib.E_INVALID and b"ldp" in lib.tgcn_last_error()
    with pytest.raises(ValueError):
        _lib.check(members(K=65))
    scores = lambda counts=p, K=2, C=3, out=p: lib.tgcn_class_scores(counts, K, C, out, None)
    for kw in (dict(K=0), dict(K=65), dict(C=0), dict(C=4097), dict(counts=None), dict(out=None)):
        assert scores(**kw) == _lib.E_INVALID, kw


def test_python_wrappers_refuse_host_tensors_and_bad_shapes():
    import torch
    pred = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises((RuntimeError, TypeError, ValueError)):
        metrics.member_class_counts(pred, torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(ValueError):
        metrics.Scoreboard(0, 2, ["a"], device="cpu")
    with pytest.raises(ValueError):
        metrics.Scoreboard(2, 2, ["a", "a"], device="cpu")
    board = metrics.Scoreboard(2, 4, ["f1", "acc"], device="cpu")      # plain torch ops: the bookkeeping runs anywhere
    with pytest.raises(ValueError):
        board.record(f1=torch.zeros(4))
    for e in range(2):
        board.record(f1=torch.arange(4.0) + e, acc=torch.ones(4, dtype=torch.float32))
    with pytest.raises(IndexError):
        board.record(f1=torch.zeros(4), acc=torch.zeros(4))
    host = board.buffer.numpy()
    assert int(board.cursor) == 2 and np.array_equal(host[1, :, 0], [1, 2, 3, 4]) and np.array_equal(host[0, :, 1], [1, 1, 1, 1])
    mean, std = board.fold_summary("f1", 2, host=host)
    assert np.allclose(mean, [1.5, 3.5]) and np.allclose(std, [0.5, 0.5])
    with pytest.raises(ValueError):
        board.fold_summary("f1", 3, host=host)
