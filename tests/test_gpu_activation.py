"""The ReLU between the GCN layers (`GCN(..., apply_activation=True)`): `tgcn_spmm_act` / `tgcn_act_grad` at kernel level
(exact: same sums, same order, one select), the network against the unfused composition on the device and against
float64 built from the oracle's operator, and the switches of the package it has to live with.  Config c2 and smaller."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from oracle import gcn_oracle as O
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, conv as conv_, models as models_, plan as plan_mod, synth
from pytextgcn_amd.functional import masked_cross_entropy
from pytextgcn_amd.plan import GraphPlan, relu_grad_

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-5                                # BASELINE.json: relative, max-norm


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


class _C2:
    """BASELINE.json configs[1]: 100 k nodes, 2 M edges, hidden 200, 64 classes (the seed of the existing c2 tests)."""
    N, E, F, C = 100_000, 2_000_000, 200, 64

    def __init__(self, cuda):
        self.g = synth.word_doc_graph(self.N, self.E, seed=44, n_classes=self.C)
        self.gd = pkg.Data(**{k: getattr(self.g, k) for k in self.g.keys}).to(cuda)
        self.plan = plan_mod.plan_for(self.gd.edge_index, self.gd.edge_attr, self.N)

    def model(self, cuda, seed=17, **kw):
        torch.manual_seed(seed)
        m = pkg.GCN(self.N, self.C, n_hidden_gcn=self.F, dropout=0.0, **kw)
        with torch.no_grad():
            m.layers[0].bias.normal_(0, 0.1)
            m.layers[1].bias.normal_(0, 0.1)
        return m.to(cuda).float()


@pytest.fixture(scope="module")
def c2(cuda):
    return _C2(cuda)


def _spmm_act(plan, x, bias, act, transpose=False, out=None):
    """`tgcn_spmm_act` called directly (strides taken from the tensors)."""
    lib = _lib.load()
    n_out = plan.n_rows_t if transpose else plan.n_rows
    F = x.size(1)
    if out is None:
        out = torch.empty(n_out, F, device=x.device)
    ws = plan._workspace(int(transpose), F, x.device)
    _lib.check(lib.tgcn_spmm_act(plan._h, int(transpose), x.data_ptr(), x.stride(0), F,
                                 bias.data_ptr() if bias is not None else None, act, out.data_ptr(), out.stride(0),
                                 ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                 plan_mod._stream_ptr(x.device)))
    return out


# ------------------------------------------------------------------------------------------------
# kernel level: exact
# ------------------------------------------------------------------------------------------------
def test_spmm_act_relu_known_answer(cuda):
    z = np.load(os.path.join(GOLD, "known_answer.npz"))
    plan = GraphPlan(torch.from_numpy(z["edge_index"]).to(cuda), torch.from_numpy(z["edge_weight"]).to(cuda), 3)
    W, b = torch.from_numpy(z["W"]).to(cuda), torch.from_numpy(z["b"]).to(cuda)
    for w_, b_ in ((W, b), (-W, -b), (W, None)):
        plain = plan.spmm(w_, b_)
        assert torch.equal(plan.spmm(w_, b_, activation=_lib.ACT_RELU), torch.relu(plain))
        assert torch.equal(_spmm_act(plan, w_, b_, _lib.ACT_NONE), plain)
    assert rel_err(plan.spmm(W, b, activation=_lib.ACT_RELU), torch.relu(torch.from_numpy(z["out"]))) < TOL


@pytest.mark.parametrize("F", [200, 64, 203, 128])       # full-wave float4, sub-group 16 / 32 lanes, scalar lanes (VEC 1)
def test_spmm_act_relu_is_relu_of_spmm_bit_for_bit_on_c2(cuda, c2, F):
    """Gather and sub-group kernels, long rows (completed, and activated, by k_spmm_fix), a padded stride, the transposed
    block, bias present and NULL; act = NONE gives tgcn_spmm's bits."""
    plan = c2.plan
    assert plan.stats()["long_rows"] > 0
    gen = torch.Generator(device=cuda).manual_seed(F)
    x = torch.randn(c2.N, F, device=cuda, generator=gen)
    bias = torch.randn(F, device=cuda, generator=gen)
    for transpose in (False, True):
        for b in (bias, None):
            plain = plan.spmm(x, b, transpose=transpose)
            got = plan.spmm(x, b, transpose=transpose, activation=_lib.ACT_RELU)
            assert torch.equal(got, torch.relu(plain)), (F, transpose, b is None)
            assert bool((got == 0).any()) and bool((got > 0).any())
            assert torch.equal(_spmm_act(plan, x, b, _lib.ACT_NONE, transpose), plain)
    # padded strides on both sides (the float4 path needs strides of 4 k floats; 12 keeps it, 203 has none)
    wide = torch.randn(c2.N, F + 12, device=cuda, generator=gen)
    xs = wide[:, 4:4 + F]
    out = torch.full((c2.N, F + 12), 7.0, device=cuda)
    plan.spmm(xs, bias, out=out[:, 8:8 + F], activation=_lib.ACT_RELU)
    assert torch.equal(out[:, 8:8 + F], torch.relu(plan.spmm(xs.contiguous(), bias)))
    assert bool((out[:, :8] == 7).all()) and bool((out[:, 8 + F:] == 7).all())


@pytest.mark.parametrize("F", [200, 64, 7])
def test_spmm_act_relu_on_the_dense_hot_block(cuda, F):
    """The 32 hot rows are finished by k_spmm_fix from the partial sums of k_spmm_hot: that is where they are activated
    (the float4 kernels; the scalar kernel walks the complete partition)."""
    n = 5000
    gen = torch.Generator().manual_seed(n)
    srcs, dsts = [], []
    for h in range(40):                                   # hubs connected to a large random share of the others
        others = torch.nonzero(torch.rand(n, generator=gen) < 0.9 / (1 + h * 0.35)).flatten()
        others = others[others != h]
        srcs += [others, torch.full_like(others, h)]
        dsts += [torch.full_like(others, h), others]
    bg = torch.randint(0, n, (2, 4 * n), generator=gen)
    ei = torch.stack([torch.cat(srcs + [bg[0]]), torch.cat(dsts + [bg[1]])])
    w = torch.rand(ei.shape[1], generator=gen) + 0.05
    plan = GraphPlan(ei.to(cuda), w.to(cuda), n)
    assert plan.stats()["hot_rows"] == 32
    x, b = torch.randn(n, F, generator=gen).to(cuda), torch.randn(F, generator=gen).to(cuda)
    for transpose in (False, True):
        plain = plan.spmm(x, b, transpose=transpose)
        got = plan.spmm(x, b, transpose=transpose, activation=_lib.ACT_RELU)
        assert torch.equal(got, torch.relu(plain))
        assert bool((got[:40] == 0).any()) and bool((got[:40] > 0).any())          # hub rows on both sides of the gate
    plan.close()


def test_spmm_act_passes_nan_like_torch_relu_and_refuses_what_it_cannot_do(cuda):
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]], device=cuda)
    plan = GraphPlan(ei, None, 4)
    x = torch.tensor([[float("nan"), -1.0, 2.0, -0.0]] * 4, device=cuda)
    got, want = plan.spmm(x, activation=_lib.ACT_RELU), torch.relu(plan.spmm(x))
    assert bool(torch.isnan(got[:, 0]).all()) and torch.equal(got[:, 1:], want[:, 1:]) and bool((got[:, 1] == 0).all())
    lib = _lib.load()
    y = torch.empty(4, 4, device=cuda)
    assert lib.tgcn_spmm_act(plan._h, 0, x.data_ptr(), 4, 4, None, 2, y.data_ptr(), 4, None, 0, None) == _lib.E_INVALID
    assert b"act" in lib.tgcn_last_error()
    with pytest.raises(ValueError):
        plan.spmm(x, out=y, accumulate=True, activation=_lib.ACT_RELU)
    with pytest.raises(ValueError):
        plan.spmm(x[:2], x2=x[2:], activation=_lib.ACT_RELU)


@pytest.mark.parametrize("n,F", [(100_003, 200), (70_001, 64), (30_011, 203), (9, 64), (4097, 128), (50_000, 260)])
def test_act_grad_gates_in_place_and_leaves_the_column_sums(cuda, n, F):
    """G <- A > 0 ? G : 0 bit for bit, rows with A == 0 and A == -0.0 gated off; the column sums of the GATED matrix at the
    bound test_colsum (tests/test_gpu_parity.py) holds tgcn_colsum to; two runs give the same bits."""
    gen = torch.Generator(device=cuda).manual_seed(n + F)
    a = torch.relu(torch.randn(n, F, device=cuda, generator=gen))
    a[::7, ::3] = 0.0
    a[1::7, 1::3] = -0.0
    g0 = torch.randn(n, F, device=cuda, generator=gen) + 0.25
    want = torch.where(a > 0, g0, torch.zeros_like(g0))
    runs = []
    for _ in range(2):
        g = g0.clone()
        sums = relu_grad_(a, g, want_colsum=True)
        assert torch.equal(g, want)
        runs.append(sums.clone())
    assert torch.equal(runs[0], runs[1])
    ref = want.double().sum(0)
    assert ((runs[0].double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item() < 1e-5, (n, F)
    g = g0.clone()
    assert relu_grad_(a, g) is None and torch.equal(g, want)                        # gate only
    # padded strides (scalar lanes unless both strides are multiples of 4) and the identity
    wide_a, wide_g = torch.zeros(n, F + 5, device=cuda), torch.full((n, F + 5), 3.0, device=cuda)
    wide_a[:, 1:1 + F], wide_g[:, 2:2 + F] = a, g0
    sums = relu_grad_(wide_a[:, 1:1 + F], wide_g[:, 2:2 + F], want_colsum=True)
    assert torch.equal(wide_g[:, 2:2 + F], want) and bool((wide_g[:, :2] == 3).all()) and bool((wide_g[:, 2 + F:] == 3).all())
    assert ((sums.double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item() < 1e-5
    lib = _lib.load()
    g = g0.clone()
    out = torch.empty(F, device=cuda)
    ws = torch.empty(lib.tgcn_act_grad_workspace_bytes(n, F), dtype=torch.uint8, device=cuda)
    args = (a.data_ptr(), F, g.data_ptr(), F, n, F, out.data_ptr())
    assert lib.tgcn_act_grad(_lib.ACT_NONE, *args, ws.data_ptr(), ws.numel(), None) == _lib.OK
    assert torch.equal(g, g0) and torch.equal(out, plan_mod.colsum(g0))
    assert lib.tgcn_act_grad(_lib.ACT_RELU, *args, ws.data_ptr(), 8, None) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(g, g0)                                                       # refused before anything ran


# ------------------------------------------------------------------------------------------------
# network level
# ------------------------------------------------------------------------------------------------
def _unfused_forward(model, gd):
    """The composition a user had to write before: torch.relu on the first layer's output, torch autograd."""
    l1, l2 = model.layers
    h = torch.relu(l1(gd.x, gd.edge_index, gd.edge_attr))
    return l2(h, gd.edge_index, gd.edge_attr), h


def test_network_equals_the_unfused_composition_on_the_device(cuda, c2):
    """Same pre-activation bits, therefore the same gate: logits bit for bit, gradients at 1e-5 (column-sum order of the
    bias gradient may differ).  And the non-linearity is really there."""
    fused, plain = c2.model(cuda, apply_activation=True), c2.model(cuda)
    gd = c2.gd
    crit = nn.CrossEntropyLoss()
    lo_f = fused(gd)
    lo_u, h = _unfused_forward(plain, gd)
    assert torch.equal(lo_f, lo_u)
    assert bool((h == 0).any()), "no hidden element is clamped: the test does not see the activation"
    lo_lin = plain(gd)
    assert not torch.equal(lo_f, lo_lin)
    assert torch.equal(lo_lin, c2.model(cuda, apply_activation=False)(gd))       # the switch off: the network as it was
    crit(lo_f[gd.train_mask], gd.y[gd.train_mask]).backward()
    crit(lo_u[gd.train_mask], gd.y[gd.train_mask]).backward()
    for (k, pf), pu in zip(fused.named_parameters(), plain.parameters()):
        e = rel_err(pf.grad, pu.grad)
        print(f"fused vs unfused composition, {k}: {e:.3e}")
        assert e < TOL, (k, e)


def _float64_network(g, N, state, gate=None):
    """relu(M W1 + b1) -> M (. W2) + b2 in float64 on the host, M the oracle's normalised operator
    (oracle.gcn_oracle.normalized_coo: the fp32 weights of the reference, summed in float64 here).  `gate`: a 0/1 matrix
    that takes the place of float64's own `h > 0` (the device's gate), so that the gradients are those of the same
    piecewise-linear function."""
    tgt, src, w = O.normalized_coo(g.edge_index, g.edge_attr, N)
    M = torch.sparse_coo_tensor(torch.stack([tgt, src]), w.double(), (N, N)).coalesce()
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in state.items()}
    pre = torch.sparse.mm(M, p["layers.0.weight"]) + p["layers.0.bias"]
    h = torch.relu(pre) if gate is None else pre * gate
    z = torch.sparse.mm(M, h @ p["layers.1.weight"]) + p["layers.1.bias"]
    return z, pre, p


def test_network_against_float64_on_c2(cuda, c2):
    """Forward at the 1e-5 bar of the linear network (ReLU is 1-Lipschitz).  Gradients: float64's backward takes the
    DEVICE's gate, so that every element is compared; separately, wherever the device's gate and float64's own gate
    disagree the float64 pre-activation is within 1e-5 of zero on the scale of max |h64| (checked on the host with the
    fp32 CSR restatement of the oracle in place of the device for this seed before the test was committed: 0 elements
    disagree there)."""
    model = c2.model(cuda, apply_activation=True)
    gd, g = c2.gd, c2.g
    lo = model(gd)
    with torch.no_grad():
        a_gpu = model.layers[0](gd.x, gd.edge_index, gd.edge_attr, activation=model.activation)
    z64, pre64, _ = _float64_network(g, c2.N, model.state_dict())
    e = rel_err(lo, z64)
    print(f"logits vs float64: {e:.3e}")
    assert e < TOL
    gate = (a_gpu > 0).cpu()
    differ = gate != (pre64.detach() > 0)
    print(f"gate: {int(differ.sum())} of {differ.numel()} elements differ between the device and float64")
    if bool(differ.any()):
        assert float(pre64.detach()[differ].abs().max()) <= 1e-5 * float(pre64.detach().abs().max())
    masked_cross_entropy(lo, gd.y, gd.train_mask).backward()
    z64g, _, p64 = _float64_network(g, c2.N, model.state_dict(), gate=gate.double())
    nn.CrossEntropyLoss()(z64g[g.train_mask], g.y[g.train_mask]).backward()
    for k, pm in model.named_parameters():
        e = rel_err(pm.grad, p64[k].grad)
        print(f"gradient vs float64 (device gate), {k}: {e:.3e}")
        assert e < TOL, (k, e)


def _small(cuda, hidden=32, **kw):
    N, C = 1200, 5
    g = synth.word_doc_graph(N, 16000, seed=6, n_classes=C)
    torch.manual_seed(3)
    m = pkg.GCN(N, C, n_hidden_gcn=hidden, dropout=0.0, **kw)
    with torch.no_grad():
        m.layers[0].bias.normal_(0, 0.1)
    return g, pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(cuda), m.to(cuda).float()


def test_ten_training_steps_track_the_float64_loop(cuda):
    """flat_amazon.py:89,99-109 with the activation on, dropout off: the loss curve against a float64 loop at the bars of
    test_training_steps_track_the_oracle (1e-4 on the loss, 1e-3 on the eval logits)."""
    g, gd, mine = _small(cuda, apply_activation=True)
    N = g.x.shape[0]
    tgt, src, w = O.normalized_coo(g.edge_index, g.edge_attr, N)
    M = torch.sparse_coo_tensor(torch.stack([tgt, src]), w.double(), (N, N)).coalesce()
    p64 = [v.detach().cpu().double().requires_grad_() for v in mine.parameters()]         # W1, b1, W2, b2

    def fwd64():
        return torch.sparse.mm(M, torch.relu(torch.sparse.mm(M, p64[0]) + p64[1]) @ p64[2]) + p64[3]
    o_r = torch.optim.Adam(p64, lr=0.05, amsgrad=True)
    o_m = torch.optim.Adam(mine.parameters(), lr=0.05, amsgrad=True)
    crit = nn.CrossEntropyLoss()
    for step in range(10):
        l_r = crit(fwd64()[g.train_mask], g.y[g.train_mask])
        o_r.zero_grad(set_to_none=True)
        l_r.backward()
        o_r.step()
        with torch.no_grad():
            z_r = fwd64()
        l_m, z_m = O.train_step(mine, gd, o_m)
        e_l, e_z = abs(l_m.item() - l_r.item()) / abs(l_r.item()), rel_err(z_m, z_r)
        print(f"step {step}: loss {l_m.item():.6f} vs {l_r.item():.6f} ({e_l:.2e}), eval logits {e_z:.2e}")
        assert e_l < 1e-4, step
        assert e_z < 1e-3, step


def test_flat_loop_with_the_activation_tracks_the_plain_loop(cuda):
    """FlatLoop (fused CE, fused Adam, W1's update inside the backward SpMM, activation reuse, fused dropout at p = 0)
    with the activation on against the plain loop (torch CE, torch Adam, no switch) on the same network: the same bars."""
    from pytextgcn_amd.train import FlatLoop
    g, gd, a = _small(cuda, hidden=200, apply_activation=True)
    _, _, b = _small(cuda, hidden=200, apply_activation=True)
    o_b = torch.optim.Adam(b.parameters(), lr=0.05, amsgrad=True)
    crit = nn.CrossEntropyLoss()
    with FlatLoop(a, gd, lr=0.05) as loop:
        for step in range(10):
            loss, val_loss, _, _ = loop.epoch()
            l_b, z_b = O.train_step(b, gd, o_b)
            v_b = crit(z_b[gd.val_mask], gd.y[gd.val_mask]).item()
            print(f"step {step}: loss {loss:.6f} vs {l_b.item():.6f}, val {val_loss:.6f} vs {v_b:.6f}")
            assert abs(loss - l_b.item()) < 1e-4 * abs(l_b.item()), step
            assert abs(val_loss - v_b) < 1e-4 * abs(v_b), step
    a.eval()
    with torch.no_grad():
        assert rel_err(a(gd), z_b) < 1e-3
    assert not models_._FUSED_DROPOUT and not conv_._REUSE


# ------------------------------------------------------------------------------------------------
# the switches of the package
# ------------------------------------------------------------------------------------------------
def test_linear_collapse_is_not_taken(cuda):
    _, gd, m = _small(cuda, apply_activation=True)
    m.eval()
    with torch.no_grad():
        want = m(gd)
        pkg.enable_linear_collapse(True)
        try:
            assert torch.equal(m(gd), want)
        finally:
            pkg.enable_linear_collapse(False)


def test_activation_reuse_keeps_the_post_relu_value(cuda):
    """The kept layer-1 value is the post-ReLU one; handing it out is bit for bit recomputing it, forward and backward,
    and an entry made without the activation is not handed to a call with it."""
    _, gd, m = _small(cuda, hidden=200, apply_activation=True)
    _, _, ref = _small(cuda, hidden=200, apply_activation=True)
    crit = nn.CrossEntropyLoss()
    want = ref(gd)
    crit(want[gd.train_mask], gd.y[gd.train_mask]).backward()
    pkg.enable_activation_reuse(True)
    try:
        m.eval()
        with torch.no_grad():
            assert torch.equal(m(gd), want)
        l1 = m.layers[0]
        key, kept = l1._reuse_cache[0], l1._reuse_cache[1]
        assert float(kept.min()) == 0.0 and bool((kept == 0).any())
        assert key == conv_._reuse_key(plan_mod.plan_for(gd.edge_index, gd.edge_attr, gd.x.size(0)), l1.weight, l1.bias)
        m.train()
        got = m(gd)                                              # served from the entry, with autograd
        assert l1._reuse_cache[1] is kept and torch.equal(got, want)
        crit(got[gd.train_mask], gd.y[gd.train_mask]).backward()
        for pm, pr in zip(m.parameters(), ref.parameters()):
            assert torch.equal(pm.grad, pr.grad)
        with torch.no_grad():                                    # the same layer without the activation: not the kept value
            lin = l1(gd.x, gd.edge_index, gd.edge_attr)
            assert bool((lin < 0).any()) and torch.equal(torch.relu(lin), kept)
    finally:
        pkg.enable_activation_reuse(False)


@pytest.mark.parametrize("fused_dropout", [False, True])
def test_bias_gradient_of_layer_one_is_the_gated_one(cuda, fused_dropout):
    """The input-gradient GEMM of layer 2 leaves the column sums of dH1 as a note for `plan.colsum`; under the gate those
    are the sums of the wrong matrix.  b1.grad against float64 (p = 0, so the fused-dropout products are deterministic)."""
    g, gd, m = _small(cuda, hidden=200, apply_activation=True)
    m.dropout = 0.0
    m.train()
    pkg.enable_fused_dropout(fused_dropout)
    try:
        lo = m(gd)
        with torch.no_grad():
            a_gpu = m.layers[0](gd.x, gd.edge_index, gd.edge_attr, activation=m.activation)
        masked_cross_entropy(lo, gd.y, gd.train_mask).backward()
    finally:
        pkg.enable_fused_dropout(False)
    z64, _, p64 = _float64_network(g, g.x.shape[0], m.state_dict(), gate=(a_gpu > 0).cpu().double())
    nn.CrossEntropyLoss()(z64[g.train_mask], g.y[g.train_mask]).backward()
    e = rel_err(m.layers[0].bias.grad, p64["layers.0.bias"].grad)
    print(f"b1.grad vs float64: {e:.3e}")
    assert e < TOL


def test_a_gradient_that_is_not_ours_is_gated_as_a_copy(cuda):
    """`h.backward(G)` with the caller's own G: the gate must not edit it; the gradient a kernel of this package produced
    is gated in place (its column-sum note dropped)."""
    _, gd, m = _small(cuda, hidden=64)
    l1 = m.layers[0]
    h = l1(gd.x, gd.edge_index, gd.edge_attr, activation=nn.ReLU())
    G = torch.randn_like(h)
    keep = G.clone()
    h.backward(G)
    assert torch.equal(G, keep)
    want_b = torch.where(h > 0, G, torch.zeros_like(G)).double().sum(0)
    assert ((l1.bias.grad.double() - want_b).abs() / want_b.abs().clamp_min(1.0)).max().item() < 1e-5
    gw, gb = l1.weight.grad, l1.bias.grad
    l1.weight.grad = l1.bias.grad = None
    ref = torch.relu(l1(gd.x, gd.edge_index, gd.edge_attr))      # the unfused composition, torch's own gate
    ref.backward(G)
    assert torch.equal(h, ref) and torch.equal(gw, l1.weight.grad) and rel_err(gb, l1.bias.grad) < TOL


def test_rows_and_other_activation_modules(cuda):
    """`GCN.forward(g, rows=mask)` with the activation on (it never touches the last layer); a module that is not exactly
    nn.ReLU is called on the layer's output."""
    _, gd, m = _small(cuda, hidden=200, apply_activation=True)
    m.eval()
    with torch.no_grad():
        full = m(gd)
        part = m(gd, rows=gd.train_mask)
        assert rel_err(part[gd.train_mask], full[gd.train_mask]) < TOL
    _, _, t = _small(cuda, hidden=200, activation=nn.Tanh, apply_activation=True)
    t.train()
    l1, l2 = t.layers
    want = l2(torch.tanh(l1(gd.x, gd.edge_index, gd.edge_attr)), gd.edge_index, gd.edge_attr)
    got = t(gd)
    assert torch.equal(got, want)
    got.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in t.parameters())


def test_graph_capture_of_a_flat_loop_step_with_the_activation(cuda):
    """One FlatLoop-style optimisation step (fused CE, capturable fused Adam with W1's update in the backward SpMM, fused
    dropout at p = 0, needed rows only) captured into a HIP graph with the activation on: replays equal eager steps."""
    from pytextgcn_amd.train import GraphedTrainStep
    _, gd, a = _small(cuda, hidden=200, apply_activation=True)
    _, _, b = _small(cuda, hidden=200, apply_activation=True)
    pkg.enable_fused_dropout(True)
    try:
        opts = []
        for m in (a, b):
            o = pkg.optim.Adam(m.parameters(), lr=0.05, amsgrad=True, capturable=True)
            o.fuse_into_backward(m.layers[0].weight)
            opts.append(o)
        step = GraphedTrainStep(a, gd, opts[0], gd.train_mask, warmup=2, needed_rows_only=True)
        losses = [step().item() for _ in range(3)]
        b.train()
        eager = []
        for _ in range(5):
            loss = masked_cross_entropy(b(gd, rows=gd.train_mask), gd.y, gd.train_mask)
            opts[1].zero_grad(set_to_none=True)
            loss.backward()
            opts[1].step()
            eager.append(loss.item())
        torch.cuda.synchronize()
        assert losses == eager[2:]
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.equal(pa, pb)
    finally:
        pkg.enable_fused_dropout(False)
