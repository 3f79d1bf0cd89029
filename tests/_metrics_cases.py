"""Shared by tests/test_metrics_host.py (CPU) and tests/test_gpu_metrics.py: the numpy restatement of the class counts and
scores of pytextgcn_amd/metrics.py (csrc/metrics.hip), the case list of both count kernels and the generator of a case's
operands.  A case is built once per session (`operands`) and never modified."""
import functools
import warnings

import numpy as np

from pytextgcn_amd import metrics as M

R, CAP, LDS = M.ROWS_PER_WORKGROUP, M.WORKGROUP_CAP, M.LDS_BUDGET_BYTES
TOL = 1e-12          # fewer than C + 10 float64 roundings of values in [0, 1], C <= 256 where sklearn is asked


# ---- numpy restatement ---------------------------------------------------------------------------------------------------
def _planes(t, p, C):
    """[3, C] (tp, n_pred, n_true) of selected targets t (all in [0, C)) and predictions p (any integer)."""
    ok = (p >= 0) & (p < C)
    return np.stack([np.bincount(t[ok & (p == t)], minlength=C), np.bincount(p[ok], minlength=C),
                     np.bincount(t, minlength=C)]).astype(np.int32)


def counts_members(pred, target, bits, K, C):
    """[K, 3, C]: `pred` [n, >= K] int, `bits` uint64 [n]; bits at or above K are ignored."""
    out = np.zeros((K, 3, C), dtype=np.int32)
    for k in range(K):
        sel = ((bits >> np.uint64(k)) & np.uint64(1)).astype(bool)
        out[k] = _planes(target[sel], pred[sel, k].astype(np.int64), C)
    return out


def counts_groups(pred, target, mask, K, C, group=None, pred_offset=None):
    out = np.zeros((K, 3, C), dtype=np.int32)
    group = np.zeros(len(pred), dtype=np.int64) if group is None else group.astype(np.int64)
    off = np.zeros(K, dtype=np.int64) if pred_offset is None else np.asarray(pred_offset, dtype=np.int64)
    for k in range(K):
        sel = mask.astype(bool) & (group == k)
        out[k] = _planes(target[sel], pred[sel] - off[k], C)
    return out


def scores_np(counts):
    """[K, 4] float64: accuracy, f1_macro, n_rows, n_labels."""
    K = counts.shape[0]
    out = np.zeros((K, 4))
    for k in range(K):
        tp, n_pred, n_true = counts[k].astype(np.int64)
        den = n_pred + n_true
        live = den > 0
        out[k, 0] = tp.sum() / n_true.sum() if n_true.sum() else np.nan
        out[k, 1] = np.mean(2.0 * tp[live] / den[live]) if live.any() else np.nan
        out[k, 2], out[k, 3] = n_true.sum(), live.sum()
    return out


def sklearn_scores(y_true, y_pred):
    """(accuracy_score, f1_score(average="macro")) of one member's selected rows."""
    from sklearn.metrics import accuracy_score, f1_score
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return accuracy_score(y_true, y_pred), f1_score(y_true, y_pred, average="macro")


def close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)))


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _m(name, n, K, C, **kw):
    case = dict(form="members", name=name, n=n, K=K, C=C, ldp=K + 3, two=True, oob_pred=False, empty_member=K >= 2)
    case.update(kw)
    return case


# the LDS table holds [sets][members][3][C] int32: with both sets 64 members of 32 classes fill the budget exactly, one
# class more tiles the members; with one set 64 classes do; above 2048 classes the two sets go to workgroups of their own
assert 2 * 64 * 3 * 32 * 4 == LDS and 64 * 3 * 64 * 4 == LDS and 2 * 3 * 2048 * 4 == LDS
MEMBER_CASES = (
    [_m(f"K{K}", 300, K, 8) for K in (1, 2, 63, 64)]
    + [_m(f"C{C}", 200, 2, C) for C in (1, 2, 3, 8, 219, 4096)]
    + [_m(f"n{n}", n, 2, 3) for n in (0, 1, 63, 64, 65, R - 1, R, R + 1)]
    + [_m("n_cap", CAP * R + 1, 1, 2, ldp=2),
       _m("lds_fits_two_sets", 2 * R + 7, 64, 32), _m("lds_tiles_members_two_sets", 2 * R + 7, 64, 33),
       _m("lds_fits_one_set", R + 9, 64, 64, two=False), _m("lds_tiles_members_one_set", R + 9, 64, 65, two=False),
       _m("lds_both_sets_C2048", 150, 2, 2048), _m("lds_sets_apart_C2049", 150, 2, 2049),
       _m("K64_C219", R + 5, 64, 219), _m("K64_C4096", 90, 64, 4096),
       _m("one_set", 3 * R + 1, 5, 8, two=False), _m("ldp_wide", 100, 3, 8, ldp=17),
       _m("oob_pred", 2 * R + 3, 4, 8, oob_pred=True), _m("oob_pred_C1", 70, 2, 1, oob_pred=True)])


def _g(name, n, widths, **kw):
    case = dict(form="groups", name=name, n=n, widths=tuple(widths), K=len(widths), C=max(widths), group=True, offset=True,
                two=True, oob_pred=False)
    case.update(kw)
    return case


GROUP_CASES = [
    _g("flat", 2 * R + 1, [8], group=False, offset=False), _g("flat_one_mask", R - 1, [219], group=False, offset=False, two=False),
    _g("widths_offset", 3 * R + 2, [1, 3, 8]), _g("widths_no_offset", 3 * R + 2, [1, 3, 8], offset=False),
    _g("one_mask", R + 1, [1, 3, 8], two=False), _g("oob_pred", 2 * R, [1, 3, 8], oob_pred=True),
    _g("n0", 0, [1, 3, 8]), _g("n1", 1, [1, 3, 8]), _g("tiles_members", R + 3, [4096, 5, 4000]),
    _g("K64", 2 * R + 5, list(range(1, 65)))]

CASES = {c["name"] + "/" + c["form"]: c for c in MEMBER_CASES + GROUP_CASES}
GARBAGE = np.array([-7, 1 << 40, -(1 << 62), 4096, 1 << 31], dtype=np.int64)     # targets of rows nobody selects


def _classes(rng, n, C):
    """Targets and predictions in [0, C): where C >= 3 class C - 1 occurs in the predictions only and class C - 2 in the
    targets only, so both enter the macro mean with 0."""
    if C >= 3:
        t = rng.integers(0, C - 1, n)
        p = np.where(rng.random(n) < 0.6, t, rng.integers(0, C, n))
        p = np.where(p == C - 2, C - 1, p)
        t = np.where(rng.random(n) < 0.1, C - 2, t)
        return t, p
    t = rng.integers(0, C, n)
    return t, np.where(rng.random(n) < 0.6, t, rng.integers(0, C, n))


@functools.lru_cache(maxsize=None)
def operands(key):
    """The host operands of a case (read-only numpy arrays) and its expected counts per set."""
    c = CASES[key]
    rng = np.random.default_rng(sum(map(ord, key)))
    n, K, C = c["n"], c["K"], c["C"]
    out = dict(case=c)
    if c["form"] == "members":
        target, _ = _classes(rng, n, C)
        pred = np.full((n, c["ldp"]), 0x5A5A5A5A, dtype=np.int32)              # pad columns: poison
        for k in range(K):
            pred[:, k] = _classes(rng, n, C)[1] if k else np.where(rng.random(n) < 0.7, target, _classes(rng, n, C)[1])
        if C >= 3:
            pred[:, :K] = np.where(pred[:, :K] == C - 2, C - 1, pred[:, :K])
        if c["oob_pred"]:
            bad = rng.random((n, K)) < 0.2
            pred[:, :K] = np.where(bad, rng.choice(np.array([-1, C, C + 5, -(1 << 31), (1 << 31) - 1]), (n, K)), pred[:, :K])
        # one member has no row in either set: the last but one, so that member 63 of 64 (the sign bit) keeps its rows
        empty = out["empty"] = (K - 2 if K >= 3 else K - 1) if c["empty_member"] else None
        live = K
        kind = rng.integers(0, 4, n)               # a row is in no set, in set a only, in set b only, or free to be in both
        sets = []
        for s in range(2):
            on = (rng.random((n, live)) < (0.5 if s == 0 else 0.3)) & ((kind == s + 1) | (kind == 3))[:, None]
            if n >= 4:                             # one row of each kind for certain
                on[0], on[1, 0], on[2, 0], on[3, 0] = False, s == 0, s == 1, True
            if empty is not None:
                on[:, empty] = False
            bits = np.zeros(n, dtype=np.uint64)
            for k in range(live):
                bits |= on[:, k].astype(np.uint64) << np.uint64(k)
            sets.append(bits)
        none = (sets[0] | sets[1]) == 0 if c["two"] else sets[0] == 0
        target = np.where(none, GARBAGE[rng.integers(0, len(GARBAGE), n)], target).astype(np.int64)
        if K < 64:                                                              # bits at or above K: set, and ignored
            junk = (rng.integers(0, 1 << 20, n).astype(np.uint64) | np.uint64(1)) << np.uint64(K)
            sets = [b | junk for b in sets]
        if not c["two"]:
            sets = sets[:1]
        out.update(pred=pred, target=target, sets=sets)
        clean = np.where(none, 0, target)
        out["expected"] = [counts_members(pred, clean, b, K, C) for b in sets]
    else:
        widths = np.array(c["widths"])
        starts = np.concatenate([[0], np.cumsum((widths + 3) & ~3)[:-1]])       # perlabel.segment_layout
        group = rng.integers(-1, K, n).astype(np.int32) if c["group"] else None
        g = np.zeros(n, dtype=np.int64) if group is None else group.astype(np.int64)
        target, local = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for k in range(K):
            rows = np.nonzero(g == k)[0]
            target[rows], local[rows] = _classes(rng, rows.size, int(widths[k]))
        if c["oob_pred"]:
            local = np.where(rng.random(n) < 0.2, rng.choice(np.array([-1, C, C + 9, -(1 << 40)]), n), local)
        pred = local + (starts[np.maximum(g, 0)] if c["offset"] else 0)
        pred = np.where(g < 0, -1, pred).astype(np.int64)                       # a route of -1 predicts -1
        sets = [rng.random(n) < 0.5, rng.random(n) < 0.3][:2 if c["two"] else 1]
        none = ~(sets[0] | sets[1] if c["two"] else sets[0]) | (g < 0)
        target = np.where(none, GARBAGE[rng.integers(0, len(GARBAGE), n)], target).astype(np.int64)
        out.update(pred=pred, target=target, sets=[m.astype(np.uint8) for m in sets], group=group,
                   offset=starts.astype(np.int32) if c["offset"] else None)
        clean = np.where(none, 0, target)
        out["expected"] = [counts_groups(pred, clean, m, K, C, group, out["offset"]) for m in sets]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def selected_rows(ops, s, k):
    """(targets, local predictions) of the rows set s selects for member k."""
    c = ops["case"]
    if c["form"] == "members":
        sel = ((ops["sets"][s] >> np.uint64(k)) & np.uint64(1)).astype(bool)
        return ops["target"][sel], ops["pred"][sel, k].astype(np.int64)
    g = np.zeros(c["n"], dtype=np.int64) if ops["group"] is None else ops["group"]
    sel = ops["sets"][s].astype(bool) & (g == k)
    return ops["target"][sel], ops["pred"][sel] - (0 if ops["offset"] is None else int(ops["offset"][k]))


# counted by hand: 5 rows of 3 classes, predictions -1 and 3 outside [0, 3)
HAND = dict(target=np.array([0, 1, 2, 1, 0]), pred=np.array([0, -1, 3, 1, 2]),
            counts=np.array([[[1, 1, 0], [1, 1, 1], [2, 2, 1]]], dtype=np.int32),
            scores=np.array([[2 / 5, (2 / 3 + 2 / 3 + 0.0) / 3, 5.0, 3.0]]))
