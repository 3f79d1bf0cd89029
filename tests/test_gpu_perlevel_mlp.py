"""GPU tests of the per-level MLP: the fused products with a per-row class term (libtgcn.so `tgcn_mlp_act_linear_cls*`,
pytextgcn_amd/csrc/mlp.hip) and `MLP` on `perlevel.AppendedFeatures`.

1.  EXACT: `act_linear_cls` on (Z, cls, T) gives the bits of `act_linear` on Z' = (Z + T[cls[:, 0]]) + T[cls[:, 1]], Z' formed
    by torch in fp32 in that order (an id outside [0, Fh) adds nothing): C, dZ, db and dW under torch.equal, without a mask
    and with one (p in {0.3, 0.7}, one seed, one mask_row0).  The class term changes WHERE the pre-activation comes from and
    nothing after it, so any difference is an error.
2.  dT against a float64 restatement at the project's bar, max|a - b| / max|b| <= 1e-5 (BASELINE.json; the TOL of
    test_gpu_mlp.py).  The same expression evaluated in fp32 on the CPU (operands() of test_gpu_mlp.py, T ~ U(+-0.1), ids
    uniform with a few invalid ones; p in {0, 0.5}) sits at 1.5e-7 .. 5.4e-7 from float64 over dT at (N, k, n, S, Fh) =
    (1025, 256, 128, 1, 6), (333, 515, 33, 2, 79) and (129, 63, 219, 1, 128) -- the worst is (1025, 256, 128, 1, 6) without a
    mask -- and at 1.4e-7 .. 8.8e-7 over C, dZ, db and dW (the worst: dW at (333, 515, 33, 2, 79)), so the bar leaves more
    than ten-fold room at the shapes used here and no operand is rescaled.
3.  The model `MLP(F + Fh, C, [256, 128])` on AppendedFeatures against tests/_mlp_ref.MLPRef in float64 on the densified
    [X | H], and against its own run on the sparse `torch.cat` form under the same seeds when dropout is on."""
import math

import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from pytextgcn_amd import conv, mlp
from pytextgcn_amd.perlevel import AppendedFeatures, append_classes, predicted_classes

import _mlp_ref as R
from _mlp_ref import MLPRef, rel_err
from test_gpu_mlp import operands

pytestmark = pytest.mark.gpu
TOL = 1e-5
SEED, ROW0 = (1 << 41) + 977, 12345


def class_operands(N, k, S, Fh, seed):
    """cls int64 [N, S] uniform over [0, Fh) with -1 and Fh (both select nothing) sprinkled in, T ~ U(+-0.1) [Fh, k]; CPU."""
    gen = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, Fh, (N, S), generator=gen)
    bad = torch.rand(N, S, generator=gen)
    cls[bad < 0.1] = -1
    cls[bad > 0.9] = Fh
    if N > 2:
        cls[0, 0], cls[N - 1, S - 1] = -1, Fh
    T = (torch.rand(Fh, k, generator=gen) * 2 - 1) * 0.1
    return cls, T


def plus_rows(Z, cls, T):
    """Z' = (Z + T[cls[:, 0]]) + T[cls[:, 1]] in Z's dtype, slot after slot; an id outside [0, Fh) leaves the row as it is."""
    out = Z.clone()
    for s in range(cls.size(1)):
        ids = cls[:, s].long()
        ok = (ids >= 0) & (ids < T.size(0))
        out[ok] = out[ok] + T[ids[ok]]
    return out


def _in_nan(rows, cols, values, dev, col0=0, more_cols=0):
    """`values` [rows, cols] as a slice of a buffer with two more rows that is NaN everywhere else."""
    buf = torch.full((rows + 2, col0 + cols + more_cols), float("nan"), device=dev)
    view = buf[:rows, col0:col0 + cols]
    view.copy_(values)
    return view


# (N, k, n, S, Fh, ldz - k, ldcls - S, ldt - k, operands among NaN).  Every N of {0, 1, 31, 33, 129, 1025, 4100}, k of {1, 33,
# 63, 256, 257, 515}, n of {1, 33, 128, 219, 300} and (S, Fh) of {(1, 1), (1, 6), (2, 79), (1, 128)} appears.  The forward
# serves ceil(ng / 32) tiles of a 256-column group on the next leaf NT of {1, 2, 4, 8}: n = 1 (NT 1), 33 (2), 128 (4), 219 (8),
# 300 (8, then 2), and the rounded-up n = 65, 96 (three tiles on NT 4, the fourth all padding), those two among NaN.  dZ
# reduces over n in groups of 128 on NT of {1, 2, 4}: one group (n <= 128), two (219: 4 tiles, then 3 on NT 4), three (300).
# dW: n = 300 runs k_mlp_grad_w<2> and <1>; (4100, 515, 3) is 33 chunks of 128 rows in 17 slices of 2.  ldz % 4 != 0 in
# most (33, 63, 257, 515, 259, ...).
CASES = [
    (0, 33, 33, 1, 6, 0, 0, 0, False), (1, 1, 1, 1, 1, 0, 0, 0, False), (31, 63, 33, 1, 6, 0, 2, 0, False),
    (33, 33, 65, 2, 79, 0, 0, 3, True), (129, 63, 96, 1, 128, 3, 1, 1, True), (129, 256, 128, 2, 79, 3, 1, 0, False),
    (1025, 257, 219, 1, 6, 2, 0, 5, False), (1025, 256, 300, 2, 79, 0, 0, 0, False), (33, 515, 300, 1, 1, 6, 3, 2, False),
    (4100, 515, 3, 1, 128, 2, 0, 0, False), (129, 33, 1, 2, 79, 0, 2, 7, False),
]


@pytest.mark.parametrize("N,k,n,S,Fh,ldz_extra,ldcls_extra,ldt_extra,among_nan", CASES)
def test_class_term_gives_the_bits_of_the_plain_product_on_the_summed_operand(cuda, N, k, n, S, Fh, ldz_extra, ldcls_extra,
                                                                              ldt_extra, among_nan):
    Zbuf, b, W, c, G = (t.to(cuda) for t in operands(N, k, n, 500 + N + k + n, ldz_extra))
    Z = Zbuf[:, :k]
    cls64, T = (t.to(cuda) for t in class_operands(N, k, S, Fh, 900 + N + k))
    clsbuf = torch.full((N, S + ldcls_extra), 1 << 20, dtype=torch.int32, device=cuda)     # the padding: ids that must not be read
    clsbuf[:, :S] = cls64.to(torch.int32)
    cls = clsbuf[:, :S]
    if among_nan:
        Z = _in_nan(N, k, Z, cuda, more_cols=ldz_extra)
        W = _in_nan(n, k, W, cuda, more_cols=3)
        G = _in_nan(N, n, G, cuda, col0=3, more_cols=4)
        T = _in_nan(Fh, k, T, cuda, more_cols=ldt_extra)
    else:
        Tbuf = torch.full((Fh, k + ldt_extra), 3.0, device=cuda)
        Tbuf[:, :k] = T
        T = Tbuf[:, :k]
    assert N <= 1 or (Z.stride(0) == k + ldz_extra and cls.stride(0) == S + ldcls_extra)
    assert Fh <= 1 or T.stride(0) == k + ldt_extra
    if N > 2:
        assert bool((cls == -1).any()) and bool((cls == Fh).any())
    Zp = plus_rows(Z, cls, T)
    assert N == 0 or not torch.equal(Zp, Z)
    seed = torch.tensor([SEED], dtype=torch.int64, device=cuda)
    for p in (0.0, 0.3, 0.7):
        kw = dict(p=p, seed=seed if p else None, mask_row0=ROW0 if p else 0)
        C = mlp.act_linear_cls_forward(Z, b, W, cls, T, c, **kw)
        dZ, db, dW, dT = mlp.act_linear_cls_backward(Z, b, W, cls, T, G, **kw)
        wC = mlp.act_linear_forward(Zp, b, W, c, **kw)
        wZ, wb, wW = mlp.act_linear_backward(Zp, b, W, G, **kw)
        torch.cuda.synchronize()
        assert C.shape == (N, n) and dZ.shape == (N, k) and db.shape == (k,) and dW.shape == (n, k) and dT.shape == (Fh, k)
        same = {"C": torch.equal(C, wC), "dZ": torch.equal(dZ, wZ), "db": torch.equal(db, wb), "dW": torch.equal(dW, wW)}
        assert all(same.values()), (p, same)
        assert all(bool(torch.isfinite(t).all()) for t in (C, dZ, db, dW, dT))
        if N == 0:
            assert float(db.abs().sum()) == 0.0 and float(dW.abs().sum()) == 0.0 and float(dT.abs().sum()) == 0.0
        # the pieces on their own are the same numbers
        only_w = mlp.act_linear_cls_backward(Z, b, W, cls, T, G, want_z=False, want_t=False, **kw)
        only_z = mlp.act_linear_cls_backward(Z, b, W, cls, T, G, want_w=False, want_t=False, **kw)
        assert only_w[0] is None and only_w[1] is None and only_w[3] is None and only_z[2] is None and only_z[3] is None
        assert torch.equal(only_w[2], dW) and torch.equal(only_z[0], dZ) and torch.equal(only_z[1], db)


def cls_truth(Z, b, W, c, G, cls, T, keep=None, p=0.0, dtype=torch.float64):
    """(C, dZ, db, dW, dT) by autograd through tests/_mlp_ref.act_linear on Z + the selected rows of T, in `dtype` on the CPU."""
    Z, b, W, c, T = (t.detach().cpu().to(dtype).requires_grad_() for t in (Z, b, W, c, T))
    cls = cls.cpu().long()
    Zp = Z
    for s in range(cls.size(1)):
        ok = ((cls[:, s] >= 0) & (cls[:, s] < T.size(0))).unsqueeze(1)
        Zp = Zp + torch.where(ok, T[cls[:, s].clamp(0, T.size(0) - 1)], torch.zeros((), dtype=dtype))
    C = R.act_linear(Zp, b, W, c, keep, p)
    dZ, db, dW, dT = torch.autograd.grad(C, (Z, b, W, T), G.detach().cpu().to(dtype))
    return C.detach(), dZ, db, dW, dT


DT_SHAPES = [(1025, 256, 128, 1, 6), (333, 515, 33, 2, 79), (129, 63, 219, 1, 128)]


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("N,k,n,S,Fh", DT_SHAPES)
def test_table_gradient_against_float64(cuda, N, k, n, S, Fh, p):
    Zc, bc, Wc, cc, Gc = operands(N, k, n, 77 + N)
    clsc, Tc = class_operands(N, k, S, Fh, 78 + N)
    clsc[clsc == 3] = 2                                           # row 3 of T: selected by nobody
    Z, b, W, c, G, T = (t.to(cuda) for t in (Zc, bc, Wc, cc, Gc, Tc))
    cls = clsc.to(cuda).to(torch.int32)
    value = -(N * 1_000_003 + k)
    seed = torch.tensor([value], dtype=torch.int64, device=cuda) if p else None
    keep = R.keep_matrix(value, N, k, p) if p else None
    Zg, bg, Wg, cg, Tg = (t.clone().requires_grad_() for t in (Z, b, W, c, T))
    C = mlp.act_linear_cls(Zg, bg, Wg, cg, cls, Tg, p, seed)
    C.backward(G)
    tC, tZ, tb, tW, tT = cls_truth(Zc, bc, Wc, cc, Gc, clsc, Tc, keep, p)
    errs = {"C": rel_err(C, tC), "dZ": rel_err(Zg.grad, tZ), "db": rel_err(bg.grad, tb), "dW": rel_err(Wg.grad, tW),
            "dc": rel_err(cg.grad, Gc.double().sum(0)), "dT": rel_err(Tg.grad, tT)}
    print(f"mlp class term p={p} N={N} k={k} n={n} S={S} Fh={Fh}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    dT = Tg.grad
    if Fh > 3:
        assert float(dT[3].abs().sum()) == 0.0 and float(dT[2].abs().sum()) > 0.0      # a row that no id selects: exact zeros
    again = mlp.act_linear_cls_backward(Z, b, W, cls, T, G, p, seed)
    assert torch.equal(again[3], dT) and torch.equal(again[0], Zg.grad)                # the same bits every run
    if S == 1:                                                    # every row selects exactly one row of T: dT sums to db
        full = clsc.clamp(0, Fh - 1).to(cuda).to(torch.int32)
        _, db1, _, dT1 = mlp.act_linear_cls_backward(Z, b, W, full, T, G, p, seed, want_w=False)
        assert rel_err(dT1.sum(0), db1.double()) <= TOL


def test_python_layer_refuses_what_the_kernels_do_not_take(cuda):
    Z, b, W, c, _ = (t.to(cuda) for t in operands(9, 6, 4, 1))
    cls = torch.zeros(9, 1, dtype=torch.int32, device=cuda)
    T = torch.zeros(5, 6, device=cuda)
    with pytest.raises(TypeError, match="int32"):
        mlp.act_linear_cls(Z, b, W, c, cls.long(), T)
    with pytest.raises(ValueError, match="do not fit"):
        mlp.act_linear_cls(Z, b, W, c, cls[:8], T)
    with pytest.raises(ValueError, match="do not fit"):
        mlp.act_linear_cls(Z, b, W, c, torch.zeros(9, 3, dtype=torch.int32, device=cuda), T)
    with pytest.raises(ValueError, match="do not fit"):
        mlp.act_linear_cls(Z, b, W, c, cls, torch.zeros(129, 6, device=cuda))
    with pytest.raises(ValueError, match="outside"):
        mlp.act_linear_cls(Z, b, W, c, cls, T, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp.act_linear_cls(Z, b, W, c, cls.cpu(), T)


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
N_DOCS, VOCAB, N_CLASSES, HIDDEN = 129, 300, 7, [256, 128]
BLOCKS = [(6,), (9, 70)]
_TRUTH = {}


def _case(blocks):
    """X (sparse COO, CPU), the class ids of every block (with an id of -1), labels, the float64 reference on the densified
    [X | H] with its eval logits and its p = 0 training step: computed once per case."""
    if blocks not in _TRUTH:
        gen = torch.Generator().manual_seed(31 + len(blocks))
        rows = torch.arange(N_DOCS).repeat_interleave(12)
        cols = torch.randint(0, VOCAB, (N_DOCS * 12,), generator=gen)
        vals = torch.rand(N_DOCS * 12, generator=gen) * 0.4 + 0.05
        x = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (N_DOCS, VOCAB)).coalesce()
        ids = [torch.randint(0, nb, (N_DOCS,), generator=gen) for nb in blocks]
        ids[0][5] = -1
        y = torch.randint(0, N_CLASSES, (N_DOCS,), generator=gen)
        onehots = [torch.zeros(N_DOCS, nb).scatter_(1, i.clamp(min=0).unsqueeze(1), (i >= 0).float().unsqueeze(1))
                   for i, nb in zip(ids, blocks)]
        xd = torch.cat([x.to_dense()] + onehots, dim=1).double()
        torch.manual_seed(len(blocks))
        ref = MLPRef(xd.size(1), N_CLASSES, HIDDEN, dropout=0.0).double()
        with torch.no_grad():
            logits_eval = ref.eval()(xd)
        loss = nn.CrossEntropyLoss()(ref.train()(xd), y)
        ref.zero_grad(set_to_none=True)
        loss.backward()
        grads = {name: q.grad.detach().clone() for name, q in ref.named_parameters()}
        _TRUTH[blocks] = (x, ids, y, xd, ref, logits_eval, loss.detach(), grads)
    return _TRUTH[blocks]


def _appended(x, ids, blocks, dev):
    a = x.to(dev)
    base = a
    for i, nb in zip(ids, blocks):
        a = append_classes(a, i.to(dev), nb)
    assert isinstance(a, AppendedFeatures) and a.base is base and a.blocks == blocks
    return a


def _mine(ref, dev, dropout):
    model = pkg.MLP(ref.layers[0].in_features, ref.layers[-1].out_features, HIDDEN, dropout=dropout)
    model.load_state_dict({name: v.float() for name, v in ref.state_dict().items()}, strict=True)
    return model.to(dev).float()


def _step(model, x, y):
    logits = model(x)
    loss = nn.CrossEntropyLoss()(logits, y)
    model.zero_grad(set_to_none=True)
    loss.backward()
    return logits.detach(), loss.detach(), {name: q.grad.detach().clone() for name, q in model.named_parameters()}


@pytest.mark.parametrize("blocks", BLOCKS)
def test_model_on_appended_features_matches_the_reference_in_float64(cuda, blocks):
    x, ids, y, xd, ref, want_eval, want_loss, want_grads = _case(blocks)
    a, yd = _appended(x, ids, blocks, cuda), y.to(cuda)
    assert torch.equal(a.to_sparse().to_dense().cpu().double(), xd)
    mine = _mine(ref, cuda, 0.0)
    assert mine.eval().takes_class_term(a) and mine.train().takes_class_term(a)
    with torch.no_grad():
        got_eval = mine.eval()(a)
    _, loss, grads = _step(mine.train(), a, yd)
    errs = {"eval logits": rel_err(got_eval, want_eval), "loss": abs(loss.item() - want_loss.item()) / want_loss.item()}
    errs.update({name: rel_err(grads[name], want_grads[name]) for name in want_grads})
    print(f"MLP on appended features, blocks {blocks}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert set(grads) == set(want_grads)
    assert grads["layers.0.weight"].shape == mine.layers[0].weight.shape          # ONE gradient of the weight's shape
    assert all(v <= TOL for v in errs.values()), errs
    # off the fused path the same features are composed on to_sparse(): the same model within the bar
    was = pkg.enable_fused_mlp(False)
    try:
        assert not mine.takes_class_term(a)
        _, loss2, grads2 = _step(mine.train(), a, yd)
    finally:
        pkg.enable_fused_mlp(was)
    assert abs(loss2.item() - want_loss.item()) / want_loss.item() <= TOL
    assert all(rel_err(grads2[name], want_grads[name]) <= TOL for name in want_grads)


@pytest.mark.parametrize("blocks", BLOCKS)
def test_fused_dropout_step_matches_the_sparse_composition_under_the_same_seeds(cuda, blocks):
    """p = 0.5 under enable_fused_dropout: the masks are a hash of (seed, row, column) and the seeds come from torch's
    generator, so the step on AppendedFeatures and the step on the sparse torch.cat form draw the same masks."""
    x, ids, y, _, ref, *_ = _case(blocks)
    a, yd = _appended(x, ids, blocks, cuda), y.to(cuda)
    mine = _mine(ref, cuda, 0.5).train()
    pkg.enable_fused_dropout(True)
    try:
        assert mine.takes_class_term(a) and mine.takes_fused_path(a.to_sparse())
        torch.manual_seed(99)
        logits, loss, grads = _step(mine, a, yd)
        torch.manual_seed(99)
        want_logits, want_loss, want_grads = _step(mine, a.to_sparse(), yd)
        torch.manual_seed(99)
        assert torch.equal(_step(mine, a, yd)[0], logits)        # the same seeds: the same bits
    finally:
        pkg.enable_fused_dropout(False)
    errs = {"logits": rel_err(logits, want_logits), "loss": abs(loss.item() - want_loss.item()) / want_loss.item()}
    errs.update({name: rel_err(grads[name], want_grads[name]) for name in want_grads})
    print(f"MLP on appended features, fused dropout step, blocks {blocks}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert bool((logits != 0).any()) and all(v <= TOL for v in errs.values()), errs


def test_level_two_reuses_the_plan_of_level_one_and_what_does_not_fit_is_composed(cuda):
    x, ids, y, *_ = _case((9, 70))
    xdev = x.to(cuda)
    level1 = pkg.MLP(VOCAB, 9, HIDDEN).to(cuda).float().eval()
    with torch.no_grad():
        level1(xdev)                                             # builds X's plan
        plans = len(conv._FEATURE_PLANS)
        pred = predicted_classes(level1.train(), xdev)
        assert level1.training and pred.shape == (N_DOCS,) and pred.is_cuda and pred.dtype == torch.int64
        assert torch.equal(pred, level1.eval()(xdev).argmax(1))
        a = append_classes(xdev, pred, 9)
        level2 = pkg.MLP(VOCAB + 9, 70, HIDDEN).to(cuda).float().eval()
        out = level2(a)
        a3 = append_classes(a, ids[1].to(cuda), 70)
        level3 = pkg.MLP(VOCAB + 79, N_CLASSES, HIDDEN).to(cuda).float().eval()
        out3 = level3(a3)
        assert len(conv._FEATURE_PLANS) == plans                 # nothing new: X's plan served all three
        assert rel_err(out, level2(a.to_sparse())) <= TOL and rel_err(out3, level3(a3.to_sparse())) <= TOL
        # three blocks, or more than 128 appended columns: composed on to_sparse()
        a4 = append_classes(a3, pred, 9)
        wide = append_classes(xdev, pred, 129)
        m4 = pkg.MLP(VOCAB + 88, 3, [32]).to(cuda).float().eval()
        mw = pkg.MLP(VOCAB + 129, 3, [32]).to(cuda).float().eval()
        assert not m4.takes_class_term(a4) and not mw.takes_class_term(wide)
        assert torch.equal(m4(a4), m4(a4.to_sparse())) and torch.equal(mw(wide), mw(wide.to_sparse()))


def test_eval_forward_replays_from_a_graph_with_the_eager_bits(cuda):
    x, ids, _, _, ref, *_ = _case((9, 70))
    a = _appended(x, ids, (9, 70), cuda)
    mine = _mine(ref, cuda, 0.5).eval()
    assert mine.takes_class_term(a)
    with torch.no_grad():
        eager = mine(a).clone()                                  # (builds the feature plan and the stream's workspaces)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            mine(a)                                              # the side stream's own workspaces
            with torch.cuda.graph(graph, stream=side):
                out = mine(a)
        torch.cuda.current_stream().wait_stream(side)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
