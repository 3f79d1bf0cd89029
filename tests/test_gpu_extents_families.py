"""The kernel families added since tests/test_gpu_extents.py -- the embedding front ends, the hierarchy product, the fused
MLP products, the block-diagonal products, the JK pieces, the grouped and member cross-entropy, the activation gradient,
the member class counts -- on operands whose row offsets pass 2^31 bytes, 2^32 bytes, 2^31 elements and 2^32 elements, and
`tgcn_adam_members` on tensors of more than 2^31 elements (its `IDX32 = false` leaves).

tests/_extent_cases.py holds the case table and the placement (checked on the CPU by tests/test_extent_cases.py).  One
float32 pool serves the module.  A case fills it with NaN and places ONE 2-D operand of the call in it as the strided
view `pool[MARGIN:].view(rows, ld)[:, :width]`; every other operand is compact.  The call runs twice on the same values:
  * compact: the results are held to the float64 restatement the family's own tests use, at their bound (1e-5 in the max
    norm, BASELINE.json; exact for the integer results);
  * placed: every result is bit for bit the compact run's (a row's arithmetic does not depend on its stride, and both runs
    are in the same alignment class: rows of 4 j floats from a 16-byte aligned base), and the pool holds exactly the view's
    elements and NaN: a read through a wrapped offset meets NaN, a write through one lands in a gap and is counted.
Everything goes through the C ABI (the `c_int64` signatures of `_lib.SIGNATURES`): most Python wrappers allocate their own
results, so they cannot place an output."""
import ctypes

import numpy as np
import pytest
import torch

import _blockdiag_ref as B
import _crossval_ref as CV
import _egcn_hier_ref as EH
import _egcn_ref as EG
import _extent_cases as X
import _jkn_ref as J
import _metrics_cases as MC
import _mlp_ref as M
import _perlabel_ref as PL
import _perlevel_ref as PV
from pytextgcn_amd import _lib, mlp
from pytextgcn_amd import plan as plan_mod
from pytextgcn_amd.functional import Segments
from pytextgcn_amd.perlabel import BlockDiagLayout

pytestmark = pytest.mark.gpu
TOL = 1e-5                          # BASELINE.json: max|a - b| / max|b|, the bound of every family's own tests
F32, I32, I64 = torch.float32, torch.int32, torch.int64
NAN = float("nan")
FILL = 7.0                          # what an "inout" result holds before the call (tests/_blockdiag_ref.py: FILL)
ROW0 = (1 << 32) + 5                # mask_row0 of the fused dropout products: the row key is the 64-bit row index
SEED = 0x5DEECE66D12345
R = X.R


def _r4(v):
    return (v + 3) & ~3


def _need(nbytes, cuda):
    free = torch.cuda.mem_get_info(cuda)[0]
    if free < nbytes + X.GiB:
        pytest.skip(f"needs {nbytes / 1e9:.1f} GB of free device memory, {free / 1e9:.1f} GB free")


@pytest.fixture(scope="module")
def pool(cuda):
    n = X.pool_elems()
    _need(4 * n, cuda)
    buf = torch.full((n,), NAN, device=cuda)
    yield buf
    del buf
    _BASE.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _compact(dev, a):
    """a host tensor [.., rows, width] on the device as rows of width rounded up to 4 floats"""
    buf = torch.empty(*a.shape[:-1], _r4(a.size(-1)), dtype=a.dtype, device=dev)
    v = buf[..., :a.size(-1)]
    v.copy_(a)
    assert v.data_ptr() % 16 == 0 and v.stride(-2) % 4 == 0
    return v


def _placed(pool, op, pl):
    """the operand's view of the pool (float32, or int32 for the index operands)"""
    base = (pool if op.dtype == "f32" else pool.view(I32))[X.MARGIN:]
    if op.kind == "planes":
        v = base.as_strided((pl.planes, pl.rows, pl.width), (pl.hstep, pl.ld, 1))
    else:
        v = base[:pl.rows * pl.ld].view(pl.rows, pl.ld)[:, :pl.width]
        assert v.stride() == (pl.ld, 1)
    assert v.data_ptr() % 16 == 0 and v.data_ptr() - pool.data_ptr() == 4 * X.MARGIN
    return v


def _nan(*shape):
    return torch.full(shape, NAN)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    return t.stride(-2)


def _err(got, want):
    """max|got - want| / max|want|; against an all-zero truth: max|got|, which must then be 0 to pass"""
    got, want = got.detach().cpu().double(), torch.as_tensor(want).detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.equal(torch.isfinite(got), torch.isfinite(want))
    fin = torch.isfinite(want)
    assert torch.equal(got[~fin].isnan(), want[~fin].isnan())
    got, want = got[fin], want[fin]
    if want.numel() == 0 or float(want.abs().max()) == 0.0:
        return float(got.abs().max()) if got.numel() else 0.0
    return float((got - want).abs().max() / want.abs().max())


def _hold(got, want):
    """every named result within TOL of the float64 truth, finite exactly where the truth is"""
    errs = {k: _err(got[k], w) for k, w in want.items()}
    assert all(e <= TOL for e in errs.values()), errs


def _ok(lib, st):
    assert st == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()


def _ws(dev, nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _seed(dev, p, k=None):
    if not p:
        return None
    return torch.tensor([SEED] if k is None else B.seeds_for(k), dtype=I64, device=dev)


def _keep(seed, rows, cols, p, row0=ROW0):
    return EG.keep_matrix(int(seed), rows, cols, p, row0) if p else None


class Call:
    """One entry point on fixed values: `ops` name -> host tensor of every placeable operand (an "out" operand is NaN),
    `run(t)` the call on device tensors `t` of the same names (any row stride) returning every result, `check(res)` the float64
    bar; `gap` name -> the id that fills the gaps of an index operand."""

    def __init__(self, ops, run, check, gap=None):
        self.ops, self.run, self.check, self.gap = ops, run, check, gap or {}


# ----------------------------------------------------------------------------------------------------------------------
# CrossVal: block-diagonal products, member CE, member class counts
# ----------------------------------------------------------------------------------------------------------------------
def _blockdiag(dev, p, grad):
    lib = _lib.load()
    h, widths, starts, n_cols = X.BD["h"], list(X.BD["widths"]), list(X.BD["starts"]), X.BD["n_cols"]
    assert (starts, n_cols) == B.layout(widths)
    K = len(widths)
    Xh, Wh, Gh = (torch.from_numpy(a) for a in B.operands(R, h, K, n_cols, "randn"))
    rates = [p] * K
    lay = BlockDiagLayout(starts, widths, h, n_cols, rates, dev)
    seeds = _seed(dev, p, K)
    seeds_py = None if seeds is None else seeds.tolist()
    stream = plan_mod._stream_ptr(dev)
    want = B.products(Xh, Wh, Gh, h, starts, widths, rates, seeds_py, ROW0)
    pad = torch.from_numpy(np.array([not any(s <= c < s + w for s, w in zip(starts, widths)) for c in range(n_cols)]))
    if not grad:
        def run(t):
            _ok(lib, lib.tgcn_blockdiag_xw(_ptr(t["X"]), _ld(t["X"]), _ptr(t["W"]), _ld(t["W"]), _ptr(t["C"]), _ld(t["C"]), R,
                                           lay.host.ctypes.data, lay.dev.data_ptr(), _ptr(seeds), ROW0, stream))
            return dict(C=t["C"])

        def check(res):
            _hold(res, dict(C=want[0]))
            assert not bool(res["C"].cpu()[:, pad].any())
        return Call(dict(X=Xh, W=Wh, C=_nan(R, n_cols)), run, check)

    def run(t):
        need = lib.tgcn_blockdiag_xw_grad_workspace_bytes(lay.host.ctypes.data, R)
        ws = _ws(dev, need)
        cs = torch.full((K * h,), NAN, device=dev)
        _ok(lib, lib.tgcn_blockdiag_xw_grad(_ptr(t["X"]), _ld(t["X"]), _ptr(t["W"]), _ld(t["W"]), _ptr(t["G"]), _ld(t["G"]),
                                            _ptr(t["dX"]), _ld(t["dX"]), cs.data_ptr(), _ptr(t["dW"]), _ld(t["dW"]), R,
                                            lay.host.ctypes.data, lay.dev.data_ptr(), _ptr(seeds), ROW0, ws.data_ptr(),
                                            ws.numel(), stream))
        return dict(dX=t["dX"], colsum=cs, dW=t["dW"])

    def check(res):
        _hold(res, dict(dX=want[1], colsum=want[2], dW=want[3]))
        assert bool((res["dX"].cpu()[torch.from_numpy(want[1] == 0)] == 0.0).all())      # the dropped elements: exactly zero
        assert not bool(res["dW"].cpu()[:, pad].any())
    return Call(dict(X=Xh, W=Wh, G=Gh, dX=_nan(R, K * h), dW=_nan(h, n_cols)), run, check)


def _member_ce(dev, p):
    lib = _lib.load()
    K, C, S = X.MCE["K"], X.MCE["C"], X.MCE["S"]
    c = CV.make_case(R, K, C, S)
    ref = CV.reference(R, K, C, S)
    counts = CV.counts_of(c["bits"], K)
    inv = torch.tensor([1.0 / v if v else 0.0 for v in counts], dtype=F32, device=dev)
    target, bits = c["target"].to(dev), c["bits"].to(dev)
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        loss, loss_k = torch.full((1,), -5.0, device=dev), torch.full((K,), -5.0, device=dev)
        dbias = torch.full((K * S,), NAN, device=dev)
        pred = torch.full((R, K), -7, dtype=I32, device=dev)
        need = lib.tgcn_member_ce_workspace_bytes(R, K, C)
        ws = _ws(dev, need)
        _ok(lib, lib.tgcn_member_ce(_ptr(t["logits"]), _ld(t["logits"]), R, K, C, S, target.data_ptr(), bits.data_ptr(),
                                    inv.data_ptr(), loss.data_ptr(), loss_k.data_ptr(), _ptr(t["dlogits"]), _ld(t["dlogits"]),
                                    dbias.data_ptr(), pred.data_ptr(), ws.data_ptr(), need, stream))
        return dict(loss=loss, loss_k=loss_k, dlogits=t["dlogits"], dbias=dbias, pred=pred)

    def check(res):
        loss, loss_k, d, db, pred = ref
        _hold(res, dict(loss=loss.reshape(1), loss_k=loss_k, dlogits=d, dbias=db))
        assert bool((res["dlogits"].cpu()[d == 0] == 0.0).all())            # other segments, unselected rows, pad columns
        assert torch.equal(res["pred"].cpu(), pred)
    return Call(dict(logits=c["logits"], dlogits=_nan(R, K * S)), run, check)


def _class_counts(dev, p):
    lib = _lib.load()
    K, C = X.CNT["K"], X.CNT["C"]
    gap = C - 1                                           # a class no real row predicts: the reference counts it as zero
    rng = np.random.default_rng(273)
    pred = rng.integers(0, gap, size=(R, K)).astype(np.int32)
    pred[::17, 1] = -1                                    # a route of -1: a miss
    target = rng.integers(0, C, size=R).astype(np.int64)
    sets = [rng.integers(0, 1 << K, size=R).astype(np.uint64) | (np.uint64(1) << np.uint64(40)) for _ in range(2)]
    want = [MC.counts_members(pred, target, s, K, C) for s in sets]
    assert all(not w[:, 1, gap].any() for w in want) and all(w[:, 1].any() for w in want)
    tgt = torch.from_numpy(target).to(dev)
    bits = [torch.from_numpy(s.view(np.int64)).to(dev) for s in sets]
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        outs = [torch.full((K, 3, C), -7, dtype=I32, device=dev) for _ in sets]
        need = lib.tgcn_class_counts_workspace_bytes(R, K, C)
        ws = _ws(dev, need)
        _ok(lib, lib.tgcn_class_counts_members(_ptr(t["pred"]), _ld(t["pred"]), tgt.data_ptr(), bits[0].data_ptr(),
                                               bits[1].data_ptr(), R, K, C, outs[0].data_ptr(), outs[1].data_ptr(),
                                               ws.data_ptr(), need, stream))
        return dict(counts_a=outs[0], counts_b=outs[1])

    def check(res):
        for name, w in zip(("counts_a", "counts_b"), want):
            assert np.array_equal(res[name].cpu().numpy(), w), name
    return Call(dict(pred=torch.from_numpy(pred)), run, check, gap=dict(pred=gap))


# ----------------------------------------------------------------------------------------------------------------------
# the embedding front ends: plain, on [I | H] features, member-batched
# ----------------------------------------------------------------------------------------------------------------------
def _embed(dev, p, dims, grad, hier, members):
    lib = _lib.load()
    Mm = dims.get("M", 1)
    D, n, N = dims["K"], dims["n"], R                    # D: the embedding rows of ONE member
    Fh, h0 = dims.get("Fh", 0), dims.get("h_row0", 0)
    g = _gen(1000 + 10 * Mm + n + Fh)
    E = torch.randn(Mm * D, N, generator=g) * 0.7
    Eh = torch.randn(Mm * D, max(Fh, 1), generator=g) * 0.7
    b = torch.randn(Mm * D, generator=g) * 0.2
    W = torch.randn(Mm * D, n, generator=g) * 0.3
    G = torch.randn(N, Mm * n, generator=g)
    Hd = torch.softmax(2.0 * torch.randn(N - h0, max(Fh, 1), generator=g), dim=1)
    seeds = _seed(dev, p, Mm if members else None)
    bd = b.to(dev)
    stream = plan_mod._stream_ptr(dev)
    rates = (ctypes.c_double * Mm)(*([p] * Mm))
    # float64, member by member
    want = dict(C=[], dE=[], dEh=[], db=[], dW=[])
    for m in range(Mm):
        rows = slice(m * D, (m + 1) * D)
        keep = _keep(seeds[m if members else 0], N, D, p) if p else None
        Gm = G[:, m * n:(m + 1) * n]
        if hier:
            c, dwt, db, dw = EH.truth(torch.cat([E[rows], Eh[rows]], 1), b[rows], Hd, h0, W[rows], Gm, keep, p)
            de, deh = dwt[:, :N], dwt[:, N:]
        else:
            c, de, db, dw = EG.fused_truth(E[rows], b[rows], W[rows], Gm, keep, p)
            deh = torch.zeros(D, 1, dtype=torch.float64)
        for k, v in zip(("C", "dE", "dEh", "db", "dW"), (c, de, deh, db, dw)):
            want[k].append(v)
    want = {k: torch.cat(v, 1 if k == "C" else 0) for k, v in want.items()}
    ops = dict(E=E, W=W)
    if hier:
        ops.update(Eh=Eh, Hd=Hd)

    def head(t):
        a = [_ptr(t["E"]), _ld(t["E"]), bd.data_ptr()]
        if hier:
            a += [_ptr(t["Eh"]), _ld(t["Eh"]), _ptr(t["Hd"]), _ld(t["Hd"]), h0, Fh]
        elif members:
            a += [None, 0, None, 0, 0, 0]
        return a + [_ptr(t["W"]), _ld(t["W"])]

    def tail():
        return [N, D, n] + ([Mm, rates, _ptr(seeds)] if members else [float(p), _ptr(seeds)]) + [ROW0]

    if not grad:
        fn = lib.tgcn_embed_xw_members if members else (lib.tgcn_embed_xw_h if hier else lib.tgcn_embed_xw)

        def run(t):
            _ok(lib, fn(*head(t), _ptr(t["C"]), _ld(t["C"]), *tail(), stream))
            return dict(C=t["C"])
        ops.update(C=_nan(N, Mm * n))
        return Call(ops, run, lambda res: _hold(res, dict(C=want["C"])))

    if members:
        fn, need = lib.tgcn_embed_xw_members_grad, lib.tgcn_embed_xw_members_grad_workspace_bytes(N, D, n, Fh, Mm)
    elif hier:
        fn, need = lib.tgcn_embed_xw_h_grad, lib.tgcn_embed_xw_h_grad_workspace_bytes(N, D, n, Fh)
    else:
        fn, need = lib.tgcn_embed_xw_grad, lib.tgcn_embed_xw_grad_workspace_bytes(N, D, n)

    def run(t):
        ws = _ws(dev, need)
        db = torch.full((Mm * D,), NAN, device=dev)
        mid = [_ptr(t["G"]), _ld(t["G"]), _ptr(t["dE"]), _ld(t["dE"]), db.data_ptr()]
        if hier:
            mid += [_ptr(t["dEh"]), _ld(t["dEh"])]
        elif members:
            mid += [None, 0]
        _ok(lib, fn(*head(t), *mid, _ptr(t["dW"]), _ld(t["dW"]), *tail(), ws.data_ptr(), ws.numel(), stream))
        return dict(dE=t["dE"], db=db, dW=t["dW"], **(dict(dEh=t["dEh"]) if hier else {}))

    def check(res):
        got = dict(db=res["db"], dW=res["dW"])
        if hier:                                          # dE and dEh are the two column ranges of ONE parameter's gradient
            got["dWeight"] = torch.cat([res["dE"].cpu(), res["dEh"].cpu()], 1)
            _hold(got, dict(db=want["db"], dW=want["dW"], dWeight=torch.cat([want["dE"], want["dEh"]], 1)))
        else:
            _hold(dict(got, dE=res["dE"]), dict(db=want["db"], dW=want["dW"], dE=want["dE"]))
    ops.update(G=G, dE=_nan(Mm * D, N), dW=_nan(Mm * D, n))
    if hier:
        ops.update(dEh=_nan(Mm * D, Fh))
    return Call(ops, run, check)


# ----------------------------------------------------------------------------------------------------------------------
# the hierarchy product
# ----------------------------------------------------------------------------------------------------------------------
def _hier(dev, p, grad):
    lib = _lib.load()
    N, Fh, h0, F = X.HIER["N"], X.HIER["Fh"], X.HIER["h_row0"], X.HIER["F"]
    stream = plan_mod._stream_ptr(dev)
    if not grad:
        W, G, Hd = PV.operands(N, F, Fh, h0, "dense", 11)
        want = PV.truth(W, G, Hd, h0)[0]

        def run(t):
            _ok(lib, lib.tgcn_hier_xw(_ptr(t["W"]), _ld(t["W"]), _lib.HIER_DENSE, None, _ptr(t["Hd"]), _ld(t["Hd"]), h0, Fh,
                                      _ptr(t["C"]), _ld(t["C"]), N, F, stream))
            return dict(C=t["C"])
        return Call(dict(W=W, Hd=Hd, C=_nan(N, F)), run, lambda res: _hold(res, dict(C=want)))
    W, G, cls = PV.operands(N, F, Fh, h0, "onehot", 12)
    want = PV.truth(W, G, cls, h0)[1]
    cd = cls.to(dev)
    need = lib.tgcn_hier_xw_grad_workspace_bytes(N, F, Fh, h0, _lib.HIER_ONEHOT)

    def run(t):
        ws = _ws(dev, need)
        _ok(lib, lib.tgcn_hier_xw_grad(_ptr(t["G"]), _ld(t["G"]), _lib.HIER_ONEHOT, cd.data_ptr(), h0, Fh, _ptr(t["dW"]),
                                       _ld(t["dW"]), N, F, ws.data_ptr(), ws.numel(), stream))
        return dict(dW=t["dW"])
    return Call(dict(G=G, dW=_nan(N + Fh, F)), run, lambda res: _hold(res, dict(dW=want)))


# ----------------------------------------------------------------------------------------------------------------------
# the fused MLP products: plain, with class rows, grouped
# ----------------------------------------------------------------------------------------------------------------------
def _mlp(dev, p, grad, with_cls):
    lib = _lib.load()
    d = X.MLPC if with_cls else X.MLP
    k, n, N = d["k"], d["n"], R
    g = _gen(77 + with_cls)
    Z = torch.randn(N, k, generator=g)
    b, W, c = torch.randn(k, generator=g) * 0.2, torch.randn(n, k, generator=g) * 0.2, torch.randn(n, generator=g) * 0.1
    G = torch.randn(N, n, generator=g)
    seed = _seed(dev, p)
    keep = _keep(SEED, N, k, p)
    bd, cdv = b.to(dev), c.to(dev)
    stream = plan_mod._stream_ptr(dev)
    ops, gap = dict(Z=Z, W=W), {}
    Zeff = Z.double()
    if with_cls:
        S, Fh = d["S"], d["Fh"]
        gap_id = Fh - 1                                   # a valid id that no real row uses; its row of T is NaN
        cls = torch.randint(0, gap_id, (N, S), generator=g).to(I32)
        cls[::13, 1] = -1                                 # an id outside [0, Fh) selects nothing
        T = torch.randn(Fh, k, generator=g) * 0.5
        T[gap_id] = NAN
        valid = cls >= 0
        for s in range(S):
            Zeff[valid[:, s]] += T.double()[cls[valid[:, s], s].long()]
        ops.update(cls=cls, T=T)
        gap = dict(cls=gap_id)
    wc, wz, wb, ww, _ = M.fused_truth(Zeff, b, W, c, G, keep, p)

    def term(t):
        return [_ptr(t["cls"]), _ld(t["cls"]), d["S"], _ptr(t["T"]), _ld(t["T"]), d["Fh"]] if with_cls else []

    if not grad:
        fn = lib.tgcn_mlp_act_linear_cls if with_cls else lib.tgcn_mlp_act_linear

        def run(t):
            _ok(lib, fn(_ptr(t["Z"]), _ld(t["Z"]), *term(t), bd.data_ptr(), _ptr(t["W"]), _ld(t["W"]), cdv.data_ptr(),
                        _ptr(t["C"]), _ld(t["C"]), N, k, n, float(p), _ptr(seed), ROW0, stream))
            return dict(C=t["C"])
        ops.update(C=_nan(N, n))
        return Call(ops, run, lambda res: _hold(res, dict(C=wc)), gap)
    want = dict(dZ=wz, db=wb, dW=ww)
    if with_cls:
        wt = torch.zeros(d["Fh"], k, dtype=torch.float64)
        for s in range(d["S"]):
            wt.index_add_(0, cls[valid[:, s], s].long(), wz[valid[:, s]])
        want["dT"] = wt
        fn, need = lib.tgcn_mlp_act_linear_cls_grad, lib.tgcn_mlp_act_linear_cls_grad_workspace_bytes(N, k, n, d["Fh"])
    else:
        fn, need = lib.tgcn_mlp_act_linear_grad, lib.tgcn_mlp_act_linear_grad_workspace_bytes(N, k, n)

    def run(t):
        ws = _ws(dev, need)
        db = torch.full((k,), NAN, device=dev)
        dt = [_ptr(t["dT"]), _ld(t["dT"])] if with_cls else []
        _ok(lib, fn(_ptr(t["Z"]), _ld(t["Z"]), *term(t), bd.data_ptr(), _ptr(t["W"]), _ld(t["W"]), _ptr(t["G"]), _ld(t["G"]),
                    _ptr(t["dZ"]), _ld(t["dZ"]), db.data_ptr(), *dt, _ptr(t["dW"]), _ld(t["dW"]), N, k, n, float(p), _ptr(seed),
                    ROW0, ws.data_ptr(), ws.numel(), stream))
        return dict(dZ=t["dZ"], db=db, dW=t["dW"], **(dict(dT=t["dT"]) if with_cls else {}))
    ops.update(G=G, dZ=_nan(N, k), dW=_nan(n, k))
    if with_cls:
        ops.update(dT=_nan(d["Fh"], k))
    return Call(ops, run, lambda res: _hold(res, want), gap)


def _mlp_grouped(dev, p, grad):
    lib = _lib.load()
    d = X.MLPG
    k, ns, rp, w_rows, c_cols, N = d["k"], list(d["n"]), list(d["row_ptr"]), d["w_rows"], d["c_cols"], R
    K = len(ns)
    w0 = [sum(ns[:g]) for g in range(K)]                 # stacked weights and result columns, back to back
    b_off = [g * k for g in range(K)]
    assert w0[-1] + ns[-1] == w_rows == c_cols and rp[-1] == N
    lay = mlp.GroupedLayout(rp, w0, ns, w0, b_off, N, k, w_rows, c_cols, K * k, dev)
    g = _gen(99)
    Z, b, W = torch.randn(N, k, generator=g), torch.randn(K * k, generator=g) * 0.2, torch.randn(w_rows, k, generator=g) * 0.3
    c, G = torch.randn(c_cols, generator=g) * 0.1, torch.randn(N, c_cols, generator=g)
    seed = _seed(dev, p)
    bd, cdv = b.to(dev), c.to(dev)
    stream = plan_mod._stream_ptr(dev)
    wC = torch.full((N, c_cols), FILL, dtype=torch.float64)
    wZ, wb, wW = torch.zeros(N, k, dtype=torch.float64), torch.zeros(K * k, dtype=torch.float64), torch.zeros(w_rows, k, dtype=torch.float64)
    wc = torch.zeros(c_cols, dtype=torch.float64)
    own = torch.zeros(N, c_cols, dtype=torch.bool)
    for q in range(K):
        rows, cols = slice(rp[q], rp[q + 1]), slice(w0[q], w0[q] + ns[q])
        keep = _keep(SEED, rp[q + 1] - rp[q], k, p, ROW0 + rp[q])
        t = M.fused_truth(Z[rows], b[b_off[q]:b_off[q] + k], W[cols], c[cols], G[rows, cols], keep, p)
        wC[rows, cols], wZ[rows], wb[b_off[q]:b_off[q] + k], wW[cols], wc[cols] = t
        own[rows, cols] = True
    if not grad:
        def run(t):
            _ok(lib, lib.tgcn_mlp_grouped_act_linear(_ptr(t["Z"]), _ld(t["Z"]), bd.data_ptr(), _ptr(t["W"]), _ld(t["W"]),
                                                     cdv.data_ptr(), _ptr(t["C"]), _ld(t["C"]), N, k, lay.host.ctypes.data,
                                                     lay.dev.data_ptr(), float(p), _ptr(seed), ROW0, stream))
            return dict(C=t["C"])

        def check(res):
            got = res["C"].cpu()
            assert bool((got[~own] == FILL).all())         # the other groups' columns keep what they held
            _hold(dict(C=got[own]), dict(C=wC[own]))
        return Call(dict(Z=Z, W=W, C=torch.full((N, c_cols), FILL)), run, check)
    need = lib.tgcn_mlp_grouped_act_linear_grad_workspace_bytes(lay.host.ctypes.data)

    def run(t):
        ws = _ws(dev, need)
        db, dc = torch.full((K * k,), NAN, device=dev), torch.full((c_cols,), NAN, device=dev)
        _ok(lib, lib.tgcn_mlp_grouped_act_linear_grad(
            _ptr(t["Z"]), _ld(t["Z"]), bd.data_ptr(), _ptr(t["W"]), _ld(t["W"]), _ptr(t["G"]), _ld(t["G"]), _ptr(t["dZ"]),
            _ld(t["dZ"]), db.data_ptr(), _ptr(t["dW"]), _ld(t["dW"]), dc.data_ptr(), N, k, lay.host.ctypes.data,
            lay.dev.data_ptr(), float(p), _ptr(seed), ROW0, ws.data_ptr(), ws.numel(), stream))
        return dict(dZ=t["dZ"], db=db, dW=t["dW"], dc=dc)
    return Call(dict(Z=Z, W=W, G=G, dZ=_nan(N, k), dW=_nan(w_rows, k)), run,
                lambda res: _hold(res, dict(dZ=wZ, db=wb, dW=wW, dc=wc)))


# ----------------------------------------------------------------------------------------------------------------------
# JumpingKnowledge: the fused forward and the pieces.  The pieces have no restatement of their own in tests/_jkn_ref.py
# (it states the whole step through nn.LSTM); theirs is the arithmetic include/tgcn.h documents, in float64.
# ----------------------------------------------------------------------------------------------------------------------
def _xs_args(t, L):
    xs = [t[f"xs{i}"] for i in range(L)]
    return (ctypes.c_void_p * L)(*[x.data_ptr() for x in xs]), (ctypes.c_int64 * L)(*[_ld(x) for x in xs])


def _jk_forward(dev, p):
    lib = _lib.load()
    L, C, H, N = X.JKF["L"], X.JKF["C"], X.JKF["H"], R
    assert H == L * C // 2 and lib.tgcn_jk_lstm_forward_supported(H)
    with torch.random.fork_rng(devices=[]):              # (nn.LSTM draws its parameters from the global generator)
        torch.manual_seed(C + L)
        state = {k: v.detach().clone() for k, v in J.JKRef(C, L).state_dict().items()}
    vs, _ = J.jk_values(N, C, L, 1000 + N + C + L)
    want_out, want_alpha = J.jk_truth(vs, state, with_alpha=True)
    lstm = [state["lstm." + k] for k in J.LSTM_KEYS]
    Wih, Whh = torch.cat([lstm[0], lstm[4]], 0), torch.cat([lstm[1], lstm[5]], 0)        # the two directions share ldwi / ldwh
    bias = [lstm[i].to(dev) for i in (2, 3, 6, 7)]
    aw, ab = state["att.weight"].flatten().to(dev), state["att.bias"].to(dev)
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        xs, lds = _xs_args(t, L)
        wi, wh = t["Wih"], t["Whh"]
        ptrs = (ctypes.c_void_p * 8)(wi.data_ptr(), wh.data_ptr(), bias[0].data_ptr(), bias[1].data_ptr(),
                                     wi[4 * H:].data_ptr(), wh[4 * H:].data_ptr(), bias[2].data_ptr(), bias[3].data_ptr())
        _ok(lib, lib.tgcn_jk_lstm_forward(xs, lds, L, N, C, H, ptrs, _ld(wi), _ld(wh), aw.data_ptr(), ab.data_ptr(),
                                          _ptr(t["out"]), _ld(t["out"]), _ptr(t["alpha"]), _ld(t["alpha"]), 0, stream))
        return dict(out=t["out"], alpha=t["alpha"])
    ops = {f"xs{i}": v for i, v in enumerate(vs)}
    ops.update(Wih=Wih, Whh=Whh, out=_nan(N, C), alpha=_nan(N, L))
    return Call(ops, run, lambda res: _hold(res, dict(out=want_out, alpha=want_alpha)))


def _jk_cell(dev, p):
    lib = _lib.load()
    H, N = X.JKC["H"], R
    g = _gen(25)
    px, ph, cp = torch.randn(N, 4 * H, generator=g), torch.randn(N, 4 * H, generator=g), torch.randn(N, H, generator=g)
    bi, bh = torch.randn(4 * H, generator=g) * 0.3, torch.randn(4 * H, generator=g) * 0.3
    z = (px.double() + ph.double() + (bi.double() + bh.double())).view(N, 4, H)
    gates = torch.stack([torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.tanh(z[:, 2]), torch.sigmoid(z[:, 3])], 1)
    c = gates[:, 1] * cp.double() + gates[:, 0] * gates[:, 2]
    h = gates[:, 3] * torch.tanh(c)
    bid, bhd = bi.to(dev), bh.to(dev)
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        _ok(lib, lib.tgcn_jk_cell(_ptr(t["pre_x"]), _ld(t["pre_x"]), _ptr(t["pre_h"]), _ld(t["pre_h"]), bid.data_ptr(),
                                  bhd.data_ptr(), _ptr(t["c_prev"]), _ld(t["c_prev"]), _ptr(t["gates"]), _ld(t["gates"]),
                                  _ptr(t["c"]), _ld(t["c"]), _ptr(t["h"]), _ld(t["h"]), N, H, stream))
        return dict(gates=t["gates"], c=t["c"], h=t["h"])
    return Call(dict(pre_x=px, pre_h=ph, c_prev=cp, gates=_nan(N, 4 * H), c=_nan(N, H), h=_nan(N, H)), run,
                lambda res: _hold(res, dict(gates=gates.reshape(N, 4 * H), c=c, h=h)))


def _jk_attention(dev, p):
    lib = _lib.load()
    L, C, H, N = X.JKA["L"], X.JKA["C"], X.JKA["H"], R
    Hp = _r4(H)                                           # h_bwd sits Hp floats behind h_fwd in the same rows
    vs, _ = J.jk_values(N, C, L, 31)
    g = _gen(32)
    hh = torch.randn(L, N, Hp + H, generator=g)
    aw, ab = torch.randn(2 * H, generator=g) * 0.5, torch.randn(1, generator=g)
    hf, hb = hh[:, :, :H].double(), hh[:, :, Hp:].double()
    score = (hf * aw[:H].double()).sum(2) + (hb * aw[H:].double()).sum(2) + ab.double()          # [L, N]
    alpha = torch.softmax(score.t(), dim=1)                                                      # [N, L]
    out = torch.relu(sum(alpha[:, i:i + 1] * vs[i].double() for i in range(L)))
    awd, abd = aw.to(dev), ab.to(dev)
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        xs, lds = _xs_args(t, L)
        h = t["h"]
        assert h.stride(2) == 1
        _ok(lib, lib.tgcn_jk_attention(xs, lds, L, N, C, H, h.data_ptr(), h.data_ptr() + 4 * Hp, h.stride(1), h.stride(0),
                                       awd.data_ptr(), abd.data_ptr(), _ptr(t["out"]), _ld(t["out"]), _ptr(t["alpha"]),
                                       _ld(t["alpha"]), 1, stream))
        return dict(out=t["out"], alpha=t["alpha"])
    ops = {f"xs{i}": v for i, v in enumerate(vs)}
    ops.update(h=hh, out=_nan(N, C), alpha=_nan(N, L))
    return Call(ops, run, lambda res: _hold(res, dict(out=out, alpha=alpha)))


def _jk_attention_grad(dev, p):
    lib = _lib.load()
    L, C, N = X.JKA["L"], X.JKA["C"], R
    vs, G = J.jk_values(N, C, L, 41)
    g = _gen(42)
    out = torch.randn(N, C, generator=g)
    alpha = torch.softmax(torch.randn(N, L, generator=g), dim=1)
    gg = G.double() * (out > 0)
    da = torch.stack([(gg * v.double()).sum(1) for v in vs], 1)
    dscore = alpha.double() * (da - (alpha.double() * da).sum(1, keepdim=True))
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        xs, lds = _xs_args(t, L)
        _ok(lib, lib.tgcn_jk_attention_grad(xs, lds, L, N, C, _ptr(t["G"]), _ld(t["G"]), _ptr(t["out"]), _ld(t["out"]),
                                            _ptr(t["alpha"]), _ld(t["alpha"]), _ptr(t["dscore"]), _ld(t["dscore"]), stream))
        return dict(dscore=t["dscore"])
    ops = {f"xs{i}": v for i, v in enumerate(vs)}
    ops.update(G=G, out=out, alpha=alpha, dscore=_nan(N, L))
    return Call(ops, run, lambda res: _hold(res, dict(dscore=dscore)))


def _jk_cell_grad(dev, p):
    lib = _lib.load()
    H, N = X.JKC["H"], R
    g = _gen(51)
    z = torch.randn(N, 4, H, generator=g)
    gates = torch.stack([torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.tanh(z[:, 2]), torch.sigmoid(z[:, 3])], 1)
    gates = gates.reshape(N, 4 * H).contiguous()
    c, cp, dh, dc = (torch.randn(N, H, generator=g) for _ in range(4))
    ds, aw = torch.randn(N, 1, generator=g), torch.randn(H, generator=g) * 0.5
    ig, fg, gg, og = (gates.double().view(N, 4, H)[:, i] for i in range(4))
    dhh = dh.double() + ds.double() * aw.double()
    tc_ = torch.tanh(c.double())
    dcn = dc.double() + dhh * og * (1 - tc_ * tc_)
    want = dict(dgates=torch.stack([dcn * gg * ig * (1 - ig), dcn * cp.double() * fg * (1 - fg), dcn * ig * (1 - gg * gg),
                                    dhh * tc_ * og * (1 - og)], 1).reshape(N, 4 * H), dc=dcn * fg)
    awd = aw.to(dev)
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        _ok(lib, lib.tgcn_jk_cell_grad(_ptr(t["gates"]), _ld(t["gates"]), _ptr(t["c"]), _ld(t["c"]), _ptr(t["c_prev"]),
                                       _ld(t["c_prev"]), _ptr(t["dh_rec"]), _ld(t["dh_rec"]), _ptr(t["dscore_t"]),
                                       _ld(t["dscore_t"]), awd.data_ptr(), _ptr(t["dc"]), _ld(t["dc"]), 0, _ptr(t["dgates"]),
                                       _ld(t["dgates"]), N, H, stream))
        return dict(dgates=t["dgates"], dc=t["dc"])
    return Call(dict(gates=gates, c=c, c_prev=cp, dh_rec=dh, dscore_t=ds, dc=dc, dgates=_nan(N, 4 * H)), run,
                lambda res: _hold(res, want))


def _jk_input_grad(dev, p):
    lib = _lib.load()
    C, N = X.JKA["C"], R
    g = _gen(61)
    T, G, out = (torch.randn(N, C, generator=g) for _ in range(3))
    al = torch.rand(N, 1, generator=g)
    want = al.double() * (G.double() * (out > 0)) + T.double()
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        _ok(lib, lib.tgcn_jk_input_grad(_ptr(t["dx"]), _ld(t["dx"]), _ptr(t["T"]), _ld(t["T"]), _ptr(t["G"]), _ld(t["G"]),
                                        _ptr(t["out"]), _ld(t["out"]), _ptr(t["alpha_t"]), _ld(t["alpha_t"]), N, C, stream))
        return dict(dx=t["dx"])
    return Call(dict(dx=_nan(N, C), T=T, G=G, out=out, alpha_t=al), run, lambda res: _hold(res, dict(dx=want)))


# ----------------------------------------------------------------------------------------------------------------------
# loss and activation
# ----------------------------------------------------------------------------------------------------------------------
def _grouped_ce(dev, p):
    lib = _lib.load()
    widths = list(X.GCE["widths"])
    c = PL.make_case(R, widths, True, seed=5, empty_group=R)
    n_cols, K = c["n_cols"], len(widths)
    assert n_cols == X.GCE["n_cols"]
    seg = Segments.of(c["starts"], widths, dev)
    counts = [int((c["mask"] & (c["group"] == k)).sum()) for k in range(K)]
    inv = torch.tensor([1.0 / v if v else 0.0 for v in counts], dtype=F32, device=dev)
    tg, mk, gr, rt, cm = (c[k].to(dev) for k in ("target", "mask", "group", "route", "class_map"))
    loss, loss_k, d, db = PL.grouped_ce(c["logits"], c["target"], c["mask"], c["group"], c["starts"], widths)
    want_pred = PL.routed_pred(c["logits"], c["route"], c["starts"], widths, c["class_map"])
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        ls, lk = torch.full((1,), -5.0, device=dev), torch.full((K,), -5.0, device=dev)
        dbias = torch.full((n_cols,), NAN, device=dev)
        pred = torch.full((R,), -7, dtype=I64, device=dev)
        ws = _ws(dev, lib.tgcn_grouped_ce_workspace_bytes(R, n_cols, K))
        _ok(lib, lib.tgcn_grouped_ce(_ptr(t["logits"]), _ld(t["logits"]), R, n_cols, K, seg.host_start, seg.host_width,
                                     seg.dev_start.data_ptr(), seg.dev_width.data_ptr(), gr.data_ptr(), rt.data_ptr(),
                                     tg.data_ptr(), mk.data_ptr(), inv.data_ptr(), cm.data_ptr(), ls.data_ptr(), lk.data_ptr(),
                                     _ptr(t["dlogits"]), _ld(t["dlogits"]), dbias.data_ptr(), pred.data_ptr(), ws.data_ptr(),
                                     ws.numel(), stream))
        return dict(loss=ls, loss_k=lk, dlogits=t["dlogits"], dbias=dbias, pred=pred)

    def check(res):
        _hold(res, dict(loss=loss.reshape(1), loss_k=loss_k, dlogits=d, dbias=db))
        assert bool((res["dlogits"].cpu()[d == 0] == 0.0).all())
        assert torch.equal(res["pred"].cpu(), want_pred)
    return Call(dict(logits=c["logits"], dlogits=_nan(R, n_cols)), run, check)


def _act_grad(dev, p):
    lib = _lib.load()
    F, N = X.ACT["F"], R
    g = _gen(71)
    A = torch.relu(torch.randn(N, F, generator=g))
    G = torch.randn(N, F, generator=g)
    want = G.double() * (A > 0)
    stream = plan_mod._stream_ptr(dev)

    def run(t):
        cs = torch.full((F,), NAN, device=dev)
        ws = _ws(dev, lib.tgcn_act_grad_workspace_bytes(N, F))
        _ok(lib, lib.tgcn_act_grad(_lib.ACT_RELU, _ptr(t["A"]), _ld(t["A"]), _ptr(t["G"]), _ld(t["G"]), N, F, cs.data_ptr(),
                                   ws.data_ptr(), ws.numel(), stream))
        return dict(G=t["G"], colsum=cs)

    def check(res):
        _hold(res, dict(G=want, colsum=want.sum(0)))
        assert torch.equal(res["G"].cpu(), want.float())                  # a gate: the kept entries are G's own bits
    return Call(dict(A=A, G=G), run, check)


BUILDERS = {
    "tgcn_blockdiag_xw": lambda d, p: _blockdiag(d, p, False),
    "tgcn_blockdiag_xw_grad": lambda d, p: _blockdiag(d, p, True),
    "tgcn_member_ce": _member_ce,
    "tgcn_class_counts_members": _class_counts,
    "tgcn_embed_xw": lambda d, p: _embed(d, p, X.EMB, False, False, False),
    "tgcn_embed_xw_grad": lambda d, p: _embed(d, p, X.EMB, True, False, False),
    "tgcn_embed_xw_h": lambda d, p: _embed(d, p, X.EMBH, False, True, False),
    "tgcn_embed_xw_h_grad": lambda d, p: _embed(d, p, X.EMBH, True, True, False),
    "tgcn_embed_xw_members": lambda d, p: _embed(d, p, X.EMBM, False, True, True),
    "tgcn_embed_xw_members_grad": lambda d, p: _embed(d, p, X.EMBM, True, True, True),
    "tgcn_hier_xw": lambda d, p: _hier(d, p, False),
    "tgcn_hier_xw_grad": lambda d, p: _hier(d, p, True),
    "tgcn_mlp_act_linear": lambda d, p: _mlp(d, p, False, False),
    "tgcn_mlp_act_linear_grad": lambda d, p: _mlp(d, p, True, False),
    "tgcn_mlp_act_linear_cls": lambda d, p: _mlp(d, p, False, True),
    "tgcn_mlp_act_linear_cls_grad": lambda d, p: _mlp(d, p, True, True),
    "tgcn_mlp_grouped_act_linear": lambda d, p: _mlp_grouped(d, p, False),
    "tgcn_mlp_grouped_act_linear_grad": lambda d, p: _mlp_grouped(d, p, True),
    "tgcn_jk_lstm_forward": _jk_forward,
    "tgcn_jk_cell": _jk_cell,
    "tgcn_jk_attention": _jk_attention,
    "tgcn_jk_attention_grad": _jk_attention_grad,
    "tgcn_jk_cell_grad": _jk_cell_grad,
    "tgcn_jk_input_grad": _jk_input_grad,
    "tgcn_grouped_ce": _grouped_ce,
    "tgcn_act_grad": _act_grad,
}
assert set(BUILDERS) == set(X.ENTRIES)

_BASE = {}                          # (entry, p) -> (Call, the results of its compact run): computed and checked once


def _bits(t):
    t = t.detach().contiguous()
    return t.view(I32) if t.dtype == F32 else t


def _base(dev, entry, p):
    key = (entry, p)
    if key not in _BASE:
        call = BUILDERS[entry](dev, p or 0.0)
        for op in X.ENTRIES[entry][1]:
            want = (op.planes, op.rows, op.width) if op.kind == "planes" else (op.rows, op.width)
            assert tuple(call.ops[op.name].shape) == want, (entry, op.name, tuple(call.ops[op.name].shape), want)
            assert call.ops[op.name].dtype == (F32 if op.dtype == "f32" else I32)
        assert set(call.ops) == {op.name for op in X.ENTRIES[entry][1]}, entry
        res = {k: v.detach().clone() for k, v in call.run({n: _compact(dev, a) for n, a in call.ops.items()}).items()}
        call.check(res)
        _BASE[key] = (call, res)
    return _BASE[key]


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_one_operand_past_2_to_the_32_elements(cuda, pool, case):
    call, base = _base(cuda, case.entry, case.p)                          # the compact run, held to float64
    op = X.operand(case.entry, case.operand)
    pl = X.placement_of(op)
    host = call.ops[op.name]
    if op.dtype == "f32":
        pool.fill_(NAN)
    else:
        pool.view(I32).fill_(call.gap[op.name])
    view = _placed(pool, op, pl)
    t = {n: _compact(cuda, a) for n, a in call.ops.items() if n != op.name}
    if op.io != "out":
        view.copy_(host)                                                  # (an "out" view stays NaN: the call writes all of it)
    t[op.name] = view
    res = call.run(t)
    for k, want in base.items():
        assert torch.equal(_bits(res[k]), _bits(want)), (X.case_id(case), k)
    # the pool holds the view's elements and nothing else: no write through a wrapped offset landed in a gap
    if op.dtype == "f32":
        expect = int((host == host).sum()) if op.io == "in" else host.numel()
        assert int(torch.count_nonzero(pool == pool)) == expect, X.case_id(case)
    else:
        assert int(torch.count_nonzero(pool.view(I32) != call.gap[op.name])) == host.numel(), X.case_id(case)
    if op.io == "in":
        assert torch.equal(_bits(view), _bits(host.to(cuda)))              # an input is left as it was


# ----------------------------------------------------------------------------------------------------------------------
# tgcn_adam_members past 2^31 and 2^32 elements: the `IDX32 = false` leaves of adam_members_impl (csrc/crossval.hip)
# ----------------------------------------------------------------------------------------------------------------------
BETA1, BETA2, EPS, WD = 0.9, 0.999, 1e-8, 0.01
# leaf -> (member width, K, n_rows): n_rows * n_cols lies just past 2^31 -- the threshold of adam_members_impl -- with room
# for the windows.  (128, 2) has n_cols % 4 == 0: the 16-byte leaf; (3, 3) the 4-byte one.
ADAM_SHAPES = {"16-byte": (128, 2, (1 << 23) + 8), "4-byte": (3, 3, -(-((1 << 31) + 2048) // 9))}
# The same two leaves just past 2^32 elements, beyond what a uint32 index holds: `ColumnBlockRates::col_of` takes a 32-bit
# remainder of the truncated index under IDX32, which is still the right column for every index below 2^32, so only an
# index past it tells the two remainders apart -- and only when n_cols does not divide 2^32: 36 and 9 columns.
ADAM_SHAPES_2_32 = {"16-byte": (12, 3, -(-((1 << 32) + 2048) // 36)), "4-byte": (3, 3, -(-((1 << 32) + 2048) // 9))}


def _adam_elements(shapes):
    return max(w * k * rows for w, k, rows in shapes.values())


@pytest.fixture(scope="module")
def adam_buffers(cuda):
    """p, g, m, v, vmax as `torch.empty` tensors shared by the cases: 5 x 17.2 GB with 96 GB free, 5 x 8.6 GB (the cases past
    2^31 only) with 48 GB free, nothing below that."""
    free, _ = torch.cuda.mem_get_info(cuda)
    n = _adam_elements(ADAM_SHAPES_2_32) if free >= 96 * 10 ** 9 else _adam_elements(ADAM_SHAPES) if free >= 48 * 10 ** 9 else 0
    bufs = [torch.empty(n, dtype=F32, device=cuda) for _ in range(5)]
    yield bufs
    del bufs
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _adam_members_windows(cuda, bufs, width, K, n_rows, edge, ams, form):
    if bufs[0].numel() < width * K * n_rows:
        pytest.skip(f"less than {5 * 4 * width * K * n_rows / 1e9 + 5:.0f} GB of device memory free")
    lib = _lib.load()
    n_cols = width * K
    n = n_rows * n_cols
    assert edge - 1 < n - 2048 <= edge + n_cols and edge > 2 ** 31 - 1       # INT32_MAX < n: never the 32-bit leaf
    assert edge % n_cols != 0 or edge == 1 << 31
    lrs = [0.1, 0.001, 0.03][:K]
    lr_host = (ctypes.c_double * K)(*lrs)
    stream = plan_mod._stream_ptr(cuda)
    big = [b[:n] for b in bufs]                                              # p, g, m, v, vmax
    windows = [(0, 1024), (edge - 512, edge + 512), (n - 1024, n)]
    gen = _gen(31)
    kept = []
    for a, b in windows:
        vals = [torch.randn(b - a, generator=gen).to(cuda) for _ in range(3)]
        v = (torch.rand(b - a, generator=gen) + 0.1).to(cuda)
        vals += [v, v * (0.5 + torch.rand(b - a, generator=gen).to(cuda))]
        for t, val in zip(big, vals):
            t[a:b] = val
        kept.append(vals)
    ptrs = [t.data_ptr() for t in big[:4]] + [big[4].data_ptr() if ams else None]
    if form == "host":
        st = lib.tgcn_adam_members(*ptrs, n_rows, n_cols, width, K, lr_host, BETA1, BETA2, EPS, WD, 1, stream)
    else:
        step_dev = torch.zeros((), dtype=I64, device=cuda)
        scalars = torch.full((K + 2,), FILL, dtype=F32, device=cuda)
        st = lib.tgcn_adam_members_capturable(*ptrs, n_rows, n_cols, width, K, lr_host, BETA1, BETA2, EPS, WD,
                                              step_dev.data_ptr(), scalars.data_ptr(), stream)
    assert st == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    if form == "capturable":
        assert int(step_dev) == 1 and float(scalars[K + 1]) == FILL
    compared = 0
    for (a, b), vals in zip(windows, kept):
        member = (torch.arange(a, b, device=cuda) % n_cols) // width
        for k in range(K):
            sel = member == k
            cnt = int(sel.sum())
            assert cnt > 0
            want = [t[sel].clone() for t in vals]
            assert lib.tgcn_adam_step(want[0].data_ptr(), want[1].data_ptr(), want[2].data_ptr(), want[3].data_ptr(),
                                      want[4].data_ptr() if ams else None, cnt, lrs[k], BETA1, BETA2, EPS, WD, 1,
                                      stream) == _lib.OK
            torch.cuda.synchronize()
            for i, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")):
                got = big[i][a:b][sel]
                assert torch.equal(got.view(I32), want[i].view(I32)), (width, K, ams, form, (a, b), k, name)
            assert not torch.equal(want[0], vals[0][sel])                      # the step moved the parameter
            compared += cnt
    assert compared == 3 * 1024


@pytest.mark.parametrize("form", ["host", "capturable"])
@pytest.mark.parametrize("ams", [False, True], ids=["adam", "amsgrad"])
@pytest.mark.parametrize("leaf", list(ADAM_SHAPES))
def test_adam_members_past_two_to_the_31_elements(cuda, adam_buffers, leaf, ams, form):
    """[n_rows, K width] tensors of just over 2^31 elements, where adam_members_impl leaves its 32-bit leaves.  The update is
    elementwise, so 1024-element windows at the start, across flat index 2^31 and at the end are initialised; inside each,
    every member's columns are compared bit for bit with `tgcn_adam_step` at that member's rate on a contiguous copy.  The
    rest of the `torch.empty` tensors (5 x 8.6 GB in use; skipped below 48 GB free) is whatever it was."""
    width, K, n_rows = ADAM_SHAPES[leaf]
    assert (width % 4 == 0 and (width * K) % 4 == 0) == (leaf == "16-byte")
    _adam_members_windows(cuda, adam_buffers, width, K, n_rows, 1 << 31, ams, form)


@pytest.mark.parametrize("form", ["host", "capturable"])
@pytest.mark.parametrize("ams", [False, True], ids=["adam", "amsgrad"])
@pytest.mark.parametrize("leaf", list(ADAM_SHAPES_2_32))
def test_adam_members_past_two_to_the_32_elements(cuda, adam_buffers, leaf, ams, form):
    """The same past 2^32 elements (5 x 17.2 GB), the window in the middle across flat index 2^32: the first size at which
    the 64-bit remainder of the `IDX32 = false` leaves differs from the 32-bit one."""
    width, K, n_rows = ADAM_SHAPES_2_32[leaf]
    assert (width % 4 == 0 and (width * K) % 4 == 0) == (leaf == "16-byte")
    _adam_members_windows(cuda, adam_buffers, width, K, n_rows, 1 << 32, ams, form)
