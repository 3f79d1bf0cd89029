"""GPU tests of the grouped MLP products (libtgcn.so `tgcn_mlp_grouped_*`, pytextgcn_amd/csrc/mlp_grouped.hip) and of
`PerLabelMLP`, the K per-label MLPs of MLP_label.py as one network.

The kernels are held to float64 at the project's bar, max|a - b| / max|b| <= 1e-5 (BASELINE.json): the truth of a grouped
call is tests/_mlp_ref.fused_truth per row segment, side by side (tests/_perlabel_mlp_ref.Case.truth).  The operands are
those of tests/test_gpu_mlp.py (Z ~ U(+-1), b ~ U(+-0.1), W glorot, G ~ N(0, 1)), whose fp32 evaluation sits below 9e-7
from float64 at every shape there; the reductions here are no longer (k <= 515, n <= 257, at most 4100 rows per group).
Group g's slices of C and dZ are held to the per-member kernels bit for bit (torch.equal): the sums of an element run over
k and m in the same order whatever the row tiling."""
import math
import os
import subprocess
import sys

import pytest
import torch

import pytextgcn_amd as pkg
from pytextgcn_amd import mlp
from pytextgcn_amd.perlabel import GroupedRows, PerLabelMLP, column_class_map

import _mlp_ref as R
import _perlabel_mlp_ref as P
from _mlp_ref import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEVEN = [0, 1, 32, 64, 97, 161, 256, 256]
# name -> (row_ptr, N, k, n per group, col0 per group).  col0 all zero: hidden style (W stacked by rows, one result block);
# otherwise class style (W rows and result columns at col0, segments at multiples of 4 columns).
CASES = {
    "a_hidden": ([0, 33, 33, 162], 162, 33, [5, 5, 5], [0, 0, 0]),              # an empty group in the middle
    "a_class": ([0, 33, 33, 162], 162, 33, [1, 3, 10], [0, 4, 8]),
    "b": ([0, 127, 128], 128, 100, [129, 129], [0, 0]),                         # a group of one row; dZ in two pieces
    "c": ([0, 257], 257, 256, [257], [0]),                                      # K = 1: two forward launches, three dZ pieces
    "d": (SEVEN, 261, 32, [32] * 7, [0] * 7),                                   # seven groups, five rows without one
    "e": ([0, 129, 258], 258, 63, [33, 65], [0, 36]),                           # the leaf of the wider group serves both
    "f": ([0, 4100, 4230], 4230, 515, [3, 3], [0, 0]),                          # dW: two chunks per slice, a ragged last one
}
_BUILT = {}


def case(name):
    if name not in _BUILT:
        rp, N, k, n, col0 = CASES[name]
        _BUILT[name] = P.Case(rp, N, k, n, col0, seed=sorted(CASES).index(name))
    return _BUILT[name]


def layout_of(cs, dev):
    return mlp.GroupedLayout(cs.row_ptr, cs.w_row0, cs.n, cs.col0, cs.b_off, cs.N, cs.k, cs.w_rows, cs.c_cols, cs.K * cs.k, dev)


def _in_nan(rows, cols, values, dev, col0=0, more_cols=0):
    """`values` [rows, cols] as a slice of a buffer with two more rows that is NaN everywhere else."""
    buf = torch.full((rows + 2, col0 + cols + more_cols), float("nan"), device=dev)
    view = buf[:rows, col0:col0 + cols]
    view.copy_(values)
    return view


def _seed_tensor(value, dev):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _errs(got, want):
    return {name: rel_err(g, w) for name, g, w in zip(("C", "dZ", "db", "dW", "dc"), got, want)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_against_float64_among_nan(cuda, name):
    """A.  Every operand sits in a NaN-filled buffer, and whatever the call must not read is NaN as well: the rows of Z and
    G at or past row_ptr[K], the columns of G outside a row's own segment, the rows of W that belong to no group.  C and G
    are column slices of wider buffers, ldz % 4 != 0.  Whatever the call must not write holds a sentinel afterwards."""
    cs = case(name)
    N, k, routed = cs.N, cs.k, cs.row_ptr[-1]
    tC, tZ, tb, tW, tc, own = cs.truth()
    extra = 1 if (k + 1) % 4 else 2
    Z = _in_nan(N, k, cs.Z, cuda, more_cols=extra)
    assert Z.stride(0) % 4 != 0
    Z[routed:] = float("nan")
    Wv = cs.W.clone()
    w_own = torch.zeros(cs.w_rows, dtype=torch.bool)
    for _, _, _, wr, _, _ in cs.members():
        w_own[wr] = True
    Wv[~w_own] = float("nan")
    W = _in_nan(cs.w_rows, k, Wv, cuda, more_cols=3)
    Gv = cs.G.clone()
    Gv[~own] = float("nan")
    G = _in_nan(N, cs.c_cols, Gv, cuda, col0=3, more_cols=4)
    b, c = cs.b.to(cuda), cs.c.to(cuda)
    lay = layout_of(cs, cuda)
    wide = torch.full((N, cs.c_cols + 9), 7.0, device=cuda)
    C = mlp.grouped_act_linear_forward(Z, b, W, c, lay, out=wide[:, 5:5 + cs.c_cols])
    bufs = (torch.full((N, k), 7.0, device=cuda), torch.full((cs.K * k,), 7.0, device=cuda),
            torch.full((cs.w_rows, k), 7.0, device=cuda), torch.full((cs.c_cols,), 7.0, device=cuda))
    class_style = any(cs.col0)                               # dc is the gradient of c: defined where the segments are disjoint
    dZ, db, dW, dc = mlp.grouped_act_linear_backward(Z, b, W, G, lay, want_c=class_style, out=bufs)
    torch.cuda.synchronize()
    # nothing outside the rows' own segments, nothing at or past row_ptr[K]
    assert bool((wide[:, :5] == 7.0).all()) and bool((wide[:, 5 + cs.c_cols:] == 7.0).all())
    assert bool((C.cpu()[~own] == 7.0).all()) and bool((dZ[routed:] == 7.0).all())
    assert bool((dW.cpu()[~w_own] == 7.0).all())
    c_own = torch.zeros(cs.c_cols, dtype=torch.bool)
    for g, r0, r1, wr, br, cr in cs.members():
        c_own[cr] = True
        if r0 == r1:                                         # an empty group: exact zeros
            assert float(db[br].abs().sum()) == 0.0 and float(dW[wr].abs().sum()) == 0.0
            assert not class_style or float(dc[cr].abs().sum()) == 0.0
    if class_style:
        assert bool((dc.cpu()[~c_own] == 7.0).all())        # the pad columns between the segments
    else:
        dc, tc = torch.zeros(1), torch.zeros(1, dtype=torch.float64)
    got = (torch.where(own, C.cpu(), torch.zeros(())), dZ[:routed], db, dW.cpu()[w_own], dc.cpu()[c_own[:dc.numel()]])
    assert all(bool(torch.isfinite(t).all()) for t in got)
    errs = _errs(got, (tC, tZ[:routed], tb, tW[w_own], tc[c_own[:tc.numel()]]))
    print(f"grouped mlp kernels, case {name}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("name", ["a_hidden", "a_class", "b", "c", "d", "e"])
def test_bits_of_a_group_are_the_per_member_kernels(cuda, name, p):
    """B.  By construction, no tolerance for C and dZ: k_gmlp_fwd / k_gmlp_grad_z accumulate an element over k / over m
    (pieces of 128 included) as k_mlp_fwd / k_mlp_grad_z do, and the mask row of grouped row i is mask_row0 + i.  db and dW
    are summed over other row slices than the per-member call's, hence the tolerance there."""
    cs = case(name)
    Z, b, W, c, G = (t.to(cuda) for t in (cs.Z, cs.b, cs.W, cs.c, cs.G))
    seed = _seed_tensor(0x5EED5 + len(name), cuda) if p else None
    lay = layout_of(cs, cuda)
    C = mlp.grouped_act_linear_forward(Z, b, W, c, lay, p, seed, mask_row0=11)
    dZ, db, dW, _ = mlp.grouped_act_linear_backward(Z, b, W, G, lay, p, seed, mask_row0=11)
    checked = 0
    for g, r0, r1, wr, br, cr in cs.members():
        if r0 == r1:
            continue
        Cg = mlp.act_linear_forward(Z[r0:r1], b[br], W[wr], c[cr], p, seed, mask_row0=11 + r0)
        dZg, dbg, dWg = mlp.act_linear_backward(Z[r0:r1], b[br], W[wr], G[r0:r1, cr], p, seed, mask_row0=11 + r0)
        assert torch.equal(C[r0:r1, cr], Cg), (name, g, "C")
        assert torch.equal(dZ[r0:r1], dZg), (name, g, "dZ")
        assert rel_err(db[br], dbg) <= TOL and rel_err(dW[wr], dWg) <= TOL, (name, g)
        checked += 1
    assert checked == sum(1 for _, r0, r1, *_ in cs.members() if r1 > r0) >= 1


def test_mask_is_the_documented_hash(cuda):
    """C.  p = 0.5 on case (a) with mask rows offset by 2**32 + 5: C, dZ, db and dW against float64 under the keep matrix of
    tests/_dropout_hash.py; then, as tests/test_gpu_mlp.py::test_mask_is_the_documented_hash_bit_for_bit has it, W_g = I and
    |Z + b| >= 0.1 so that C IS the activation: its zero pattern is the keep matrix and every kept entry is within 1e-6."""
    p, value, row0 = 0.5, (1 << 40) + 12345, 2 ** 32 + 5
    seed = _seed_tensor(value, cuda)
    for name in ("a_hidden", "a_class"):
        cs = case(name)
        Z, b, W, c, G = (t.to(cuda) for t in (cs.Z, cs.b, cs.W, cs.c, cs.G))
        lay = layout_of(cs, cuda)
        C = mlp.grouped_act_linear_forward(Z, b, W, c, lay, p, seed, mask_row0=row0)
        dZ, db, dW, _ = mlp.grouped_act_linear_backward(Z, b, W, G, lay, p, seed, mask_row0=row0)
        tC, tZ, tb, tW, _, own = cs.truth(seed=value, p=p, mask_row0=row0)
        errs = _errs((C, dZ, db, dW), (tC, tZ, tb, tW))
        print(f"grouped mlp kernels under the mask, case {name}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
        assert all(v <= TOL for v in errs.values()), errs
    rp, N, k = [0, 33, 33, 162], 162, 33
    cs = P.Case(rp, N, k, [k] * 3, [0] * 3, seed=77)
    gen = torch.Generator().manual_seed(5)
    sign = torch.where(torch.rand(N, k, generator=gen) < 0.5, -1.0, 1.0)
    Z = (sign * (0.2 + 0.8 * torch.rand(N, k, generator=gen))).to(cuda)          # |Z| >= 0.2, |b| <= 0.1
    b = cs.b.to(cuda)
    W = torch.eye(k).repeat(3, 1).to(cuda)
    G = (0.5 + torch.rand(N, k, generator=gen)).to(cuda)
    lay = layout_of(cs, cuda)
    C = mlp.grouped_act_linear_forward(Z, b, W, None, lay, p, seed, mask_row0=row0)
    dZ = mlp.grouped_act_linear_backward(Z, b, W, G, lay, p, seed, want_w=False, mask_row0=row0)[0]
    keep = R.keep_matrix(value, N, k, p, row0=row0)
    assert 0.4 < keep.float().mean() < 0.6
    assert torch.equal((C != 0).cpu(), keep) and torch.equal((dZ != 0).cpu(), keep)
    bias = torch.cat([cs.b[g * k:(g + 1) * k].expand(rp[g + 1] - rp[g], k) for g in range(3)]).double()
    want = torch.selu(Z.double().cpu() + bias) / (1 - p)
    assert float(((C.double().cpu() - want).abs() / want.abs())[keep].max()) <= 1e-6


@pytest.mark.parametrize("name", ["f", "d"])
def test_two_runs_give_the_same_bits(cuda, name):
    """D.  Fixed summation orders, no atomics; and a part of the results on its own is the same numbers."""
    cs = case(name)
    Z, b, W, c, G = (t.to(cuda) for t in (cs.Z, cs.b, cs.W, cs.c, cs.G))
    seed = _seed_tensor(-77, cuda)
    lay = layout_of(cs, cuda)
    for p in (0.0, 0.5):
        runs = [(mlp.grouped_act_linear_forward(Z, b, W, c, lay, p, seed),)
                + mlp.grouped_act_linear_backward(Z, b, W, G, lay, p, seed)[:3] for _ in range(2)]
        assert all(torch.equal(x, y) for x, y in zip(*runs))
        only_w = mlp.grouped_act_linear_backward(Z, b, W, G, lay, p, seed, want_z=False)
        only_z = mlp.grouped_act_linear_backward(Z, b, W, G, lay, p, seed, want_w=False)
        assert only_w[0] is None and only_w[1] is None and only_z[2] is None
        assert torch.equal(only_w[2], runs[0][3]) and torch.equal(only_z[0], runs[0][1]) and torch.equal(only_z[1], runs[0][2])


# ---------------------------------------------------------------------------------------------------------------------
# The model.  K = 3 members on F = 40 features, hidden [33, 17], class counts [2, 5, 3]; 70 documents: 33 of group 0, none of
# group 1, 30 of group 2 and 7 without a group, in shuffled order; 6 non-zeros per row.
# ---------------------------------------------------------------------------------------------------------------------
K_, F_, HID, COUNTS, N_ = 3, 40, [33, 17], [2, 5, 3], 70
CLASS_MAP = [[3, 8], [0, 1, 4, 6, 9], [2, 5, 7]]
_MODEL = {}


def _data(data_seed=0):
    """(group [N], sparse x [N, F], local target [N], rows) on the CPU, built once per seed."""
    if data_seed not in _MODEL:
        gen = torch.Generator().manual_seed(100 + data_seed)
        group = torch.cat([torch.zeros(33), torch.full((30,), 2.0), torch.full((7,), -1.0)]).long()
        group = group[torch.randperm(N_, generator=gen)]
        cols = torch.stack([torch.randperm(F_, generator=gen)[:6] for _ in range(N_)])
        idx = torch.stack([torch.arange(N_).repeat_interleave(6), cols.reshape(-1)])
        x = torch.sparse_coo_tensor(idx, torch.rand(N_ * 6, generator=gen) + 0.5, (N_, F_)).coalesce()
        counts = torch.tensor(COUNTS)
        target = (torch.rand(N_, generator=gen) * counts[group.clamp(min=0)]).long().clamp(min=0)
        target = torch.where(group >= 0, target, torch.full_like(target, -1))
        _MODEL[data_seed] = (group, x, target)
    return _MODEL[data_seed]


def _on_gpu(dev, data_seed=0, model_seed=3, dropout=0.5):
    group, x, target = _data(data_seed)
    rows = GroupedRows(group, K_).to(dev)
    torch.manual_seed(model_seed)
    model = PerLabelMLP(F_, COUNTS, HID, dropout=dropout).to(dev)
    xg = rows.features(x.to(dev))
    return model, rows, xg, rows.take(target.to(dev))


def _truth_inputs(model, rows, data_seed=0):
    group, x, target = _data(data_seed)
    order = rows.order.cpu()
    params = [(layer.weight.detach().cpu().double().requires_grad_(), layer.bias.detach().cpu().double().requires_grad_())
              for layer in model.layers]
    return params, x.to_dense().double()[order], target[order]


def _truth(model, rows, params, xs, keeps=None, p=0.0):
    return P.network_truth(params, COUNTS, model.seg_start, HID, xs, rows.row_ptr, keeps, p)


def test_eval_logits_against_float64_on_both_paths(cuda):
    """E."""
    model, rows, xg, _ = _on_gpu(cuda)
    model.eval()
    assert rows.row_ptr == [0, 33, 33, 63] and rows.n_routed == 63 and model.n_cols == 16
    params, xs, _ = _truth_inputs(model, rows)
    want = _truth(model, rows, params, xs).detach()
    with torch.no_grad():
        fused = model(xg, rows)
        was = pkg.enable_fused_mlp(False)
        try:
            assert not model.takes_fused_path()
            composed = model(xg, rows)
        finally:
            pkg.enable_fused_mlp(was)
    assert fused.shape == composed.shape == (N_, 16)
    print(f"PerLabelMLP eval logits: fused {rel_err(fused, want):.2e}, composed {rel_err(composed, want):.2e}")
    assert rel_err(fused, want) <= TOL and rel_err(composed, want) <= TOL
    own = want != 0
    assert float(fused.cpu()[~own].abs().sum()) == 0.0 and float(composed.cpu()[~own].abs().sum()) == 0.0
    # K ordinary MLPs, each on its own rows, through from_members
    torch.manual_seed(21)
    members = [pkg.MLP(F_, c, HID).to(cuda).eval() for c in COUNTS]
    net = PerLabelMLP.from_members(members).eval()
    _, x, _ = _data()
    xo = x.to_dense()[rows.order.cpu()].to(cuda)
    with torch.no_grad():
        z = net(xg, rows)
        for g, m in enumerate(members):
            r0, r1 = rows.row_ptr[g], rows.row_ptr[g + 1]
            if r1 > r0:
                s, c = net.seg_start[g], COUNTS[g]
                assert rel_err(z[r0:r1, s:s + c], m(xo[r0:r1].to_sparse())) <= TOL, g


DATA_SEED_F = 0      # chosen so that the float64 top-two logit gap of every routed row exceeds 1e-4 (asserted in the test)


def test_training_step_loss_and_predictions_against_float64(cuda, monkeypatch):
    """F.  One training step at p = 0.5 under enable_fused_dropout(): the loss is sum_k CE_mean and every parameter gradient
    is float64 autograd's under the hash masks; predictions are the host routing of MLP_label.py:157-162."""
    data_seed = DATA_SEED_F
    model, rows, xg, target = _on_gpu(cuda, data_seed)
    params, xs, tgt = _truth_inputs(model, rows, data_seed)
    seeds = []
    real = mlp.new_seed

    def recording(dev):
        seeds.append(real(dev))
        return seeds[-1]

    monkeypatch.setattr(mlp, "new_seed", recording)
    pkg.enable_fused_dropout(True)
    try:
        model.train()
        assert model.takes_fused_path()
        loss, loss_k = model.loss(xg, rows, target)
        loss.backward()
    finally:
        pkg.enable_fused_dropout(False)
    assert len(seeds) == len(HID)
    keeps = [R.keep_matrix(int(s.item()), N_, h, 0.5) for s, h in zip(seeds, HID)]
    z64 = _truth(model, rows, params, xs, keeps, 0.5)
    want = P.grouped_ce(z64, tgt, rows.row_ptr, model.seg_start, COUNTS)
    want.backward()
    assert abs(loss.item() - want.item()) <= TOL * abs(want.item())
    lk = loss_k.cpu()
    assert math.isnan(lk[1].item()) and abs(lk[0].item() + lk[2].item() - want.item()) <= TOL * abs(want.item())
    for i, (layer, (W, b)) in enumerate(zip(model.layers, params)):
        ew, eb = rel_err(layer.weight.grad, W.grad), rel_err(layer.bias.grad, b.grad)
        print(f"PerLabelMLP layer {i}: dW {ew:.2e}, db {eb:.2e}")
        assert ew <= TOL and eb <= TOL, i
    # predictions, eval mode
    model.eval()
    z64 = _truth(model, rows, params, xs).detach()
    want_pred = torch.full((N_,), -1, dtype=torch.int64)
    for g in range(K_):
        r0, r1 = rows.row_ptr[g], rows.row_ptr[g + 1]
        if r1 == r0:
            continue
        seg = z64[r0:r1, model.seg_start[g]:model.seg_start[g] + COUNTS[g]]
        top = seg.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-4                 # the arg-max is not a matter of rounding
        want_pred[r0:r1] = torch.tensor(CLASS_MAP[g])[seg.argmax(1)]       # le.inverse_transform(pred)
    pred = model.predict(xg, rows, class_map=column_class_map(CLASS_MAP, cuda))
    group = _data(data_seed)[0]
    restored = rows.restore(pred).cpu()
    assert torch.equal(restored, rows.restore(want_pred.to(cuda)).cpu())
    assert bool((restored[group < 0] == -1).all()) and bool((restored[group >= 0] >= 0).all())


def _descent_cpu(data_seed=0, steps=30):
    """The float64 restatement with p = 0 under torch's Adam: (first, last) summed loss."""
    group, x, target = _data(data_seed)
    rows = GroupedRows(group, K_)
    torch.manual_seed(3)
    model = PerLabelMLP(F_, COUNTS, HID, dropout=0.0)
    params, xs, tgt = _truth_inputs(model, rows, data_seed)
    opt = torch.optim.Adam([t for pair in params for t in pair], lr=0.05)
    losses = []
    for _ in range(steps + 1):
        loss = P.grouped_ce(_truth(model, rows, params, xs), tgt, rows.row_ptr, model.seg_start, COUNTS)
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    return losses[0], losses[-1]


def test_thirty_adam_steps_lower_the_loss_on_both_paths(cuda):
    """G.  The condition is the data's: the float64 restatement satisfies it first."""
    first, last = _descent_cpu()
    assert last < first
    for fused in (True, False):
        model, rows, xg, target = _on_gpu(cuda)
        opt = pkg.optim.Adam(model.parameters(), lr=0.05)
        was = pkg.enable_fused_mlp(fused)
        pkg.enable_fused_dropout(True)
        try:
            model.train()
            assert model.takes_fused_path() is fused
            losses = []
            for _ in range(31):
                loss, _ = model.loss(xg, rows, target)
                losses.append(loss)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
        finally:
            pkg.enable_fused_mlp(was)
            pkg.enable_fused_dropout(False)
        print(f"PerLabelMLP, fused={fused}: loss {losses[0].item():.4f} -> {losses[-1].item():.4f}")
        assert losses[-1].item() < losses[0].item()
        pad = [i for i in range(model.n_cols) if not any(s <= i < s + c for s, c in zip(model.seg_start, COUNTS))]
        assert float(model.layers[-1].weight.detach()[pad].abs().sum()) == 0.0            # pad rows stay zero


def test_forward_and_train_step_under_graph_capture(cuda):
    """H."""
    model, rows, xg, target = _on_gpu(cuda)
    model.eval()
    with torch.no_grad():
        eager = model(xg, rows).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        model(xg, rows)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static = model(xg, rows)
    static.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    # a whole training step, the GraphedTrainStep pattern
    opt = pkg.optim.Adam(model.parameters(), lr=0.05, capturable=True)
    pkg.enable_fused_dropout(True)
    try:
        model.train()

        def step():
            loss, _ = model.loss(xg, rows, target)
            loss.backward()
            opt.step()
            return loss

        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                opt.zero_grad(set_to_none=True)
                step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(graph):
            loss = step()
        before = [p.detach().clone() for p in model.parameters()]
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
    finally:
        pkg.enable_fused_dropout(False)
    assert math.isfinite(loss.item())
    assert all(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_the_python_layer_refuses_what_it_cannot_run(cuda):
    """I."""
    model, rows, xg, target = _on_gpu(cuda)
    model.eval()
    group, x, _ = _data()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(GroupedRows(group, K_).features(x), rows)
    with pytest.raises(TypeError, match="float32"):
        model(xg.double(), rows)
    with pytest.raises(ValueError, match="groups"):
        model(xg, GroupedRows(group.clamp(max=1), 2).to(cuda))
    with pytest.raises(ValueError, match="do not fit"):
        model(x.to(cuda), rows)                                          # F columns, not K F
    cs = case("a_hidden")
    lay = layout_of(cs, cuda)
    Z, b, W = cs.Z.to(cuda), cs.b.to(cuda), cs.W.to(cuda)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp.grouped_act_linear(cs.Z, b, W, None, lay)
    with pytest.raises(TypeError, match="float32"):
        mlp.grouped_act_linear(Z.double(), b, W, None, lay)
    with pytest.raises(ValueError, match="do not fit the layout"):
        mlp.grouped_act_linear(Z[:, :-1], b, W, None, lay)
    with pytest.raises(ValueError, match="uploaded"):
        mlp.grouped_act_linear(Z, b, W, None, mlp.GroupedLayout(cs.row_ptr, cs.w_row0, cs.n, cs.col0, cs.b_off, cs.N, cs.k,
                                                                 cs.w_rows, cs.c_cols, cs.K * cs.k))
    with pytest.raises(ValueError, match="outside"):
        mlp.grouped_act_linear(Z, b, W, None, lay, p=1.0)


def test_example_runs_end_to_end(cuda):
    """J.  examples/perlabel_mlp_synthetic.py in a fresh process."""
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "perlabel_mlp_synthetic.py"),
                          "--docs", "600", "--epochs", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("test accuracy:")]
    assert line, res.stdout[-3000:]
    acc, f1 = float(line[-1].split()[2]), float(line[-1].split()[-1])
    assert math.isfinite(acc) and math.isfinite(f1) and 0.0 <= acc <= 1.0 and 0.0 <= f1 <= 1.0
