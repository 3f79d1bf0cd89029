"""Exact sweep of the SpMM kernels (csrc/spmm.hip) through the C ABI: every kernel leaf of launch_vec, every partition
path of plan.hip:build_items that feeds them, in every operand layout (tests/_spmm_cases.py; the table is kept complete on
the CPU by tests/test_spmm_cases.py).

Operators are host COO triplets of small integers built under their own partition knobs, operands small integers, so the
fp32 result of ANY correct kernel in any summation order is the int64 reference bit for bit: there is no tolerance in the
integer sweep.  The two inexact comparisons of the module are the float family's derived forward-error bound
(gamma_{d+2} * (sum |m||x| + |bias| + |y0|) per element of a row with d stored entries) and, for the fused optimizer, the
measure and bound that tests/test_gpu_train_kernels.py applies to tgcn_adam_step (imported, not restated) -- next to the
bit-for-bit comparison with tgcn_adam_step on the exact gradient that include/tgcn.h promises.

Every operand is a strided view into a pool of NaN (gap columns, guard rows), every result a view into a pool of a
sentinel no result can equal, the carry workspace exactly tgcn_spmm_workspace_bytes long, NaN-filled, with a guard behind
it.  After a call: status, exact finite result, every sentinel outside the views in place, the workspace guard in place,
rows without entries of the accumulate form untouched, and the plan's long-row / hot-row / segment / item counts equal to
the restated ones, so that a case cannot quietly miss the leaf it names."""
import numpy as np
import pytest
import torch

import _spmm_cases as sc
import _train_cases as tc
from _arena import _Arena
from pytextgcn_amd import _lib
from pytextgcn_amd.plan import GraphPlan
from test_gpu_train_kernels import TOL, adam_rel_err

pytestmark = pytest.mark.gpu

SENTINEL = 0.15625               # finite, exact in fp32 and not an integer: no result of the integer sweep can equal it
GUARD_FLOATS = 256
F32 = torch.float32


class _Pools:
    def __init__(self, dev):
        self.dev = dev
        self.nan = self.out = self.ws = None
        self.plans, self.count_errors = {}, {}

    def workspace(self, nbytes, shift=0):
        """[shift floats][nbytes of NaN][guard of SENTINEL]; returns (address of the NaN part, guard view)"""
        assert nbytes % 4 == 0
        n = nbytes // 4
        if self.ws is None or self.ws.numel() < shift + n + GUARD_FLOATS:
            self.ws = None
            self.ws = torch.empty(max(shift + n + GUARD_FLOATS, 1 << 18), dtype=F32, device=self.dev)
        assert self.ws.data_ptr() % 16 == 0
        self.ws[:shift + n].fill_(float("nan"))
        guard = self.ws[shift + n:shift + n + GUARD_FLOATS]
        guard.fill_(SENTINEL)
        return self.ws.data_ptr() + 4 * shift, guard

    def release(self):
        for plan in self.plans.values():
            plan.close()
        self.plans.clear()
        self.nan = self.out = self.ws = None
        sc._product.cache_clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def pools(cuda):
    p = _Pools(cuda)
    yield p
    p.release()


@pytest.fixture
def lib(cuda):
    return _lib.load()


def plan_of(pools, op, monkeypatch):
    """The plan of an operator, created once under the operator's knob set (read at plan creation) and kept for the
    module; its counts against the restated partition, for every direction the cases use."""
    if op not in pools.plans:
        for k in sc.KNOB_NAMES:
            monkeypatch.delenv(k, raising=False)
        for k, v in op.knobs:
            monkeypatch.setenv(k, v)
        n_rows, n_cols, row, col, val = sc.plan_coo(op)
        dev = pools.dev
        plan = GraphPlan.from_coo(torch.from_numpy(row).to(dev), torch.from_numpy(col).to(dev),
                                  torch.from_numpy(val.astype(np.float32)).to(dev), n_rows, n_cols,
                                  with_transpose=sc.needs_transpose(op))
        errs = []
        for t in ((0, 1) if sc.needs_transpose(op) else (0,)):
            f = sc.facts(op, t)
            want = {"long rows": (_lib.Q_LONG_ROWS, _lib.Q_LONG_ROWS_T, len(f.long_rows)),
                    "hot rows": (_lib.Q_HOT_ROWS, _lib.Q_HOT_ROWS_T, f.n_hot)}
            if f.exact_segments:
                want["segments"] = (_lib.Q_SEGMENTS, _lib.Q_SEGMENTS_T, f.segments)
                want["items"] = (_lib.Q_ITEMS, _lib.Q_ITEMS_T, f.n_items)
            for name, (q, q_t, n) in want.items():
                got = plan.query(q_t if t else q)
                if got != n:
                    errs.append(f"{name} of transpose={t}: plan {got}, restated {n}")
        pools.plans[op], pools.count_errors[op] = plan, errs
    assert not pools.count_errors[op], f"{sc.op_id(op)}: {pools.count_errors[op]}"
    return pools.plans[op]


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _exact(got, want, what, c):
    assert got.shape == want.shape, (what, sc.case_id(c))
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values (an operand gap or an unwritten carry slot reached it)"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, k = (int(v) for v in bad[0])
        rows = torch.unique(bad[:, 0])
        pytest.fail(f"{what} differs at {bad.shape[0]} of {got.numel()} elements in {rows.numel()} rows "
                    f"(first rows {rows[:6].tolist()}), first [{r}, {k}]: {float(got[r, k])} != {float(want[r, k])}")


def run_case(lib, pools, c, monkeypatch):
    """One call of the case's entry point on guarded, strided buffers and all the checks of the module docstring."""
    plan = plan_of(pools, c.op, monkeypatch)
    ref, L, F, dev = sc.reference(c), sc.layout(c), c.F, pools.dev
    n_out, n_in = sc.applied(c.op, c.t)[:2]
    adam, split = c.form == "adam", c.split
    h = plan._h

    ins = _Arena(pools, "nan", F32)
    ix = ins.take(n_in if split is None else split, F, L.ldx, L.off_x)
    ix2 = ins.take(n_in - split, F, L.ldx2, L.off_x2) if split is not None else None
    ib = ins.take(1, F, F, L.off_b) if c.bias else None
    ins.fill(float("nan"))
    x = _dev(ref["x"], dev)
    if split is None:
        ins.view(ix).copy_(x)
    else:
        ins.view(ix).copy_(x[:split])
        ins.view(ix2).copy_(x[split:])
    if c.bias:
        ins.view(ib).copy_(_dev(ref["bias"], dev)[None, :])

    outs = _Arena(pools, "out", F32)
    if adam:
        names = ("p", "m", "v") + (("vmax",) if c.adam.amsgrad else ())
        io = {n: outs.take(n_out, F, L.ldp, 0) for n in names}
    else:
        iy = outs.take(n_out, F, L.ldy, L.off_y)
    outs.fill(SENTINEL)
    if adam:
        first = {n: _dev(ref[n], dev) for n in names}
        for n in names:
            outs.view(io[n]).copy_(first[n])
    elif c.form == "acc":
        outs.view(iy).copy_(_dev(ref["y0"], dev))

    need = int(lib.tgcn_spmm_workspace_bytes(h, c.t, F))
    if sc.workspace_floats(c) is not None:
        assert need == 4 * sc.workspace_floats(c), (need, sc.workspace_floats(c))
    ws, guard = pools.workspace(need)
    X, X2 = ins.ptr(ix), (ins.ptr(ix2) if split is not None else None)
    B = ins.ptr(ib) if c.bias else None
    if c.form == "plain":
        st = lib.tgcn_spmm(h, c.t, X, L.ldx, F, B, outs.ptr(iy), L.ldy, ws, need, None)
    elif c.form == "split":
        st = lib.tgcn_spmm_split(h, c.t, X, L.ldx, X2, L.ldx2, split, F, B, outs.ptr(iy), L.ldy, ws, need, None)
    elif c.form == "relu":
        st = lib.tgcn_spmm_act(h, c.t, X, L.ldx, F, B, _lib.ACT_RELU, outs.ptr(iy), L.ldy, ws, need, None)
    elif c.form == "acc":
        st = lib.tgcn_spmm_acc(h, c.t, X, L.ldx, X2, L.ldx2 if split is not None else 0, split or 0, F, outs.ptr(iy), L.ldy,
                               ws, need, None)
    else:
        a = c.adam
        scal = None
        if a.dev:
            scal = torch.tensor([float(v) for v in tc.adam_scalars(1, sc.ADAM_LR, sc.ADAM_BETA1, sc.ADAM_BETA2)], dtype=F32,
                                device=dev)
        hyper = (sc.ADAM_LR, sc.ADAM_BETA1, sc.ADAM_BETA2, sc.ADAM_EPS, a.wd)
        ptrs = [outs.ptr(io[n]) for n in ("p", "m", "v")] + [outs.ptr(io["vmax"]) if a.amsgrad else None]
        tail = (*hyper, 1, scal.data_ptr() if a.dev else None, ws, need, None)
        if split is None:
            st = lib.tgcn_spmm_adam(h, c.t, X, L.ldx, F, *ptrs, L.ldp, *tail)
        else:
            st = lib.tgcn_spmm_adam_split(h, c.t, X, L.ldx, X2, L.ldx2, split, F, *ptrs, L.ldp, *tail)
    torch.cuda.synchronize()
    assert st == _lib.OK, (st, lib.tgcn_last_error().decode())

    if adam:
        # the gradient is exact, so parameter and state are the bits of tgcn_adam_step on the uploaded reference gradient
        # (include/tgcn.h: tgcn_spmm_adam == tgcn_spmm + tgcn_adam_step), and within the imported measure of float64 Adam
        g = _dev(ref["grad"], dev)
        sep = {n: first[n].clone() for n in names}
        assert lib.tgcn_adam_step(sep["p"].data_ptr(), g.data_ptr(), sep["m"].data_ptr(), sep["v"].data_ptr(),
                                  sep["vmax"].data_ptr() if a.amsgrad else None, n_out * F, *hyper, 1, None) == _lib.OK
        torch.cuda.synchronize()
        want64 = tc.adam_reference(tc.AdamCase(n_out * F, a.amsgrad, a.wd, sc.ADAM_BETA1),
                                   *(ref[n].ravel() for n in ("p", "m", "v", "vmax")), [ref["grad"].ravel()],
                                   lr=sc.ADAM_LR, beta2=sc.ADAM_BETA2, eps=sc.ADAM_EPS)
        for n, w64 in zip(("p", "m", "v", "vmax"), want64):
            if n not in names:
                continue
            got = outs.view(io[n]).contiguous()
            _exact(got, sep[n], f"Adam {n} against tgcn_adam_step on the exact gradient", c)
            e = adam_rel_err(n, got.cpu().ravel(), torch.from_numpy(w64))
            assert e < TOL, (n, e)
    else:
        got = outs.view(iy).contiguous()
        if c.op.values == "int":
            _exact(got, _dev(ref["want"], dev), "Y", c)
        else:
            assert bool(torch.isfinite(got).all()), "Y: non-finite values"
            err = (got.double().cpu() - torch.from_numpy(ref["want"])).abs()
            over = err > torch.from_numpy(ref["bound"])
            if bool(over.any()):
                r, k = (int(v) for v in over.nonzero()[0])
                pytest.fail(f"Y beyond the forward-error bound at {int(over.sum())} elements, first [{r}, {k}]: error "
                            f"{float(err[r, k]):.3e}, bound {float(ref['bound'][r, k]):.3e}")
        if c.form == "acc":
            idle = _dev(~ref["has"], dev)
            assert torch.equal(got[idle].view(torch.int32), _dev(ref["y0"], dev)[idle].view(torch.int32)), \
                "a row without entries was written by the accumulate form"
    assert outs.untouched(), "a store outside the result view (gap columns / rows before or behind)"
    assert bool((guard == SENTINEL).all()), "a store behind the carry workspace"


def run_group(lib, pools, cases, monkeypatch):
    """Every case of a group -- the cases of one operator (with its knob set) and one form are the pytest item -- each on
    its own buffers; a case that fails does not hide the ones behind it: the failure lists every failing case id."""
    failures = []
    for c in cases:
        try:
            run_case(lib, pools, c, monkeypatch)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(f"{sc.case_id(c)} {sorted(sc.leaf_of(c))}: {str(e)[:300]}")
    if failures:
        pytest.fail(f"{len(failures)} of {len(cases)} cases fail:\n" + "\n".join(failures), pytrace=False)


def _group_ids(groups):
    return [f"{sc.op_id(g[0].op)}-{g[0].form}" for g in groups]


_INT = sc.grouped(sc.int_cases())
_FLOAT = sc.grouped(sc.float_cases())


@pytest.mark.parametrize("cases", _INT, ids=_group_ids(_INT))
def test_spmm_exact(lib, pools, monkeypatch, cases):
    run_group(lib, pools, cases, monkeypatch)


@pytest.mark.parametrize("cases", _FLOAT, ids=_group_ids(_FLOAT))
def test_spmm_float_within_the_forward_error_bound(lib, pools, monkeypatch, cases):
    """rand - 0.3 values and randn operands against float64: every element of a row with d stored entries within
    gamma_{d+2} (sum |m||x| + |bias| + |y0|), gamma_k = k u / (1 - k u), u = 2^-24 -- the bound of any order of fp32 FMAs and
    adds over that row (d products, the bias, the initial row), the segment sums and the hot block's pre-summed duplicates
    included.  Derived, not measured."""
    run_group(lib, pools, cases, monkeypatch)


def test_bad_workspace_leading_dimensions_and_optimizer_operands_are_refused(lib, pools, monkeypatch):
    """A workspace one byte short or 4 bytes past 16, ldx < F, ldy < F, the optimizer form at F % 4 != 0 or with a
    misaligned parameter: each returns its status before any launch and leaves every result sentinel in place."""
    op = sc.make_op("segs")
    plan = plan_of(pools, op, monkeypatch)
    h, F, dev = plan._h, 8, pools.dev
    n_out, n_in = sc.applied(op, 0)[:2]
    x = torch.ones(n_in * (F + 4) + 4, device=dev)
    bias = torch.ones(F + 4, device=dev)
    outs = _Arena(pools, "out", F32)
    iy, ip, im, iv, ix = (outs.take(n_out, F, F + 4, 0) for _ in range(5))
    outs.fill(SENTINEL)
    Y, P, M, V, VM = (outs.ptr(i) for i in (iy, ip, im, iv, ix))
    need = int(lib.tgcn_spmm_workspace_bytes(h, 0, F))
    assert need > 0
    ws, guard = pools.workspace(need, shift=4)
    X, B, INV, WSP = x.data_ptr(), bias.data_ptr(), _lib.E_INVALID, _lib.E_WORKSPACE

    def calls(ldx, ldy, w, nbytes):
        return (lib.tgcn_spmm(h, 0, X, ldx, F, B, Y, ldy, w, nbytes, None),
                lib.tgcn_spmm_split(h, 0, X, ldx, X, F, 450, F, B, Y, ldy, w, nbytes, None),
                lib.tgcn_spmm_act(h, 0, X, ldx, F, B, _lib.ACT_RELU, Y, ldy, w, nbytes, None),
                lib.tgcn_spmm_acc(h, 0, X, ldx, None, 0, 0, F, Y, ldy, w, nbytes, None))

    def adam(F_, p, w, nbytes, ldp=F + 4):
        return lib.tgcn_spmm_adam(h, 0, X, F + 4, F_, p, M, V, VM, ldp, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, w, nbytes, None)

    assert calls(F, F + 4, ws, need - 1) == (WSP,) * 4 and adam(F, P, ws, need - 1) == WSP
    assert calls(F, F + 4, ws + 4, need) == (INV,) * 4 and adam(F, P, ws + 4, need) == INV
    assert calls(F, F + 4, None, need) == (WSP,) * 4
    assert calls(F - 1, F + 4, ws, need) == (INV,) * 4
    assert calls(F, F - 1, ws, need) == (INV,) * 4
    assert adam(6, P, ws, int(lib.tgcn_spmm_workspace_bytes(h, 0, 6)), ldp=8) == INV
    assert adam(F, P + 4, ws, need) == INV
    assert adam(F, P, ws, need, ldp=F - 4) == INV
    torch.cuda.synchronize()
    assert bool((outs.pool[:outs.used] == SENTINEL).all()), "a refused call wrote to a result"
    assert bool((guard == SENTINEL).all()) and bool(torch.isnan(pools.ws[:4 + need // 4]).all()), "a refused call wrote to the workspace"
