"""GPU tests of JumpingKnowledgeNetwork and of its aggregation step (libtgcn.so `tgcn_jk_*`, pytextgcn_amd/csrc/jk.hip).

The kernels are held to the float64 restatement of tests/_jkn_ref.py (torch.stack, nn.LSTM, nn.Linear, softmax, weighted
sum) at the project's bar, max|a - b| / max|b| <= 1e-5 (BASELINE.json).  torch's own float32 LSTM stays at <= 1.4e-7 on the
output and <= 1.1e-6 on every gradient against float64 on these shapes, so the bar leaves a decade of margin.  The gradient of
`att.bias` is exact zeros by construction (the softmax is shift invariant); wherever the float32 restatement's rounding noise
would be the denominator it is compared in absolute terms against the scale of the `att.weight` gradient.

The leaf tests run every instantiation k_jk_fwd<1 .. 8> of the fused forward, both workgroup shapes, L up to 8 and, on the
composed path, H = 257 (`_jkn_ref.LEAF_SHAPES`), with the inputs surrounded by NaN, and hold `alpha` -- which the kernel
writes and the whole backward is built on -- to float64 on both paths.  On those shapes plus (257, 2), at N in {33, 65, 129},
torch's float32 LSTM on the CPU is within 1.8e-7 (out), 2.0e-7 (alpha) and 2.6e-6 (gradients; the worst at L = 8, N = 65)
of float64, so the bar leaves four-fold room over a faithful float32 evaluation.  The kernels on an MI355X: out <= 2.3e-7
(the composed path at C = 24, L = 8; the fused kernel 1.8e-7), alpha <= 1.8e-7, every gradient <= 1.0e-6 (the biases at
C = 11, L = 6, N = 1), and the rows of alpha sum to 1 within 1.25 ulp.  tests/test_jkn_host.py shows on the same parameters
and inputs that a defect of one hidden unit or one input column moves out and alpha by at least 1e-4."""
import os
import threading

import numpy as np
import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from pytextgcn_amd import jk, synth
from pytextgcn_amd.plan import alloc_padded

import _jkn_ref as R
from _jkn_ref import JKNRef, rel_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-5


def _inputs(N, C, L, dev, seed, scale=1.0, poison=False):
    """L separate [N, C] tensors of N(0, 1) values: one from `alloc_padded`, one a column slice of a wider tensor (its
    leading dimension is not its width), one 4 bytes off every 16-byte boundary; then the same again.  `poison`: each is the
    first N rows of a buffer with three more, and whatever surrounds the values -- those rows, the other columns of the wide
    tensor -- is NaN, so that a read outside an input shows in the result (the padding columns of `alloc_padded` stay
    zero: that is its contract)."""
    vs, G = R.jk_values(N, C, L, seed, scale)
    nan = float("nan")
    xs = []
    for t, v in enumerate(vs):
        if t % 3 == 0:
            if poison:
                buf = alloc_padded(N + 3, C, dev)
                buf[N:] = nan
                x = buf[:N]
            else:
                x = alloc_padded(N, C, dev)
        elif t % 3 == 1:
            x = torch.full((N + 3, C + 7), nan, device=dev)[:N, 3:3 + C] if poison else torch.zeros(N, C + 7, device=dev)[:, 3:3 + C]
            assert N <= 1 or x.stride(0) == C + 7
        else:
            x = (torch.full(((N + 3) * C + 1,), nan, device=dev)[1:1 + N * C] if poison
                 else torch.empty(N * C + 1, device=dev)[1:]).view(N, C)
            assert N == 0 or x.data_ptr() % 16 == 4
        x.copy_(v.to(dev))
        xs.append(x.requires_grad_())
    return xs, G.to(dev)


def _module(C, L, dev, seed=0, chunk_rows=jk.DEFAULT_CHUNK_ROWS):
    torch.manual_seed(seed)
    return jk.JumpingKnowledge("lstm", channels=C, num_layers=L, chunk_rows=chunk_rows).to(dev).float()


def _run(agg, xs, G, relu=False):
    """out and every gradient of one forward + backward, in the layout of `_jkn_ref.jk_truth`."""
    for x in xs:
        x.grad = None
    agg.zero_grad(set_to_none=True)
    out = agg.aggregate(xs, relu=relu)
    out.backward(G)
    torch.cuda.synchronize()
    return out.detach(), {"x": [x.grad.clone() for x in xs], "lstm": [getattr(agg.lstm, k).grad.clone() for k in R.LSTM_KEYS],
                          "att.weight": agg.att.weight.grad.clone(), "att.bias": agg.att.bias.grad.clone()}


def _errors(got, want):
    (go, gg), (wo, wg) = got, want
    errs = {"out": rel_err(go, wo), "att.weight": rel_err(gg["att.weight"], wg["att.weight"])}
    errs.update({f"dx{t}": rel_err(a, b) for t, (a, b) in enumerate(zip(gg["x"], wg["x"]))})
    errs.update({k: rel_err(a, b) for k, a, b in zip(R.LSTM_KEYS, gg["lstm"], wg["lstm"])})
    return errs


def _flat(res):
    out, g = res
    return [out] + g["x"] + g["lstm"] + [g["att.weight"], g["att.bias"]]


SHAPES = [(8, 1), (5, 3), (64, 2), (33, 4), (200, 2)]


@pytest.mark.parametrize("C,L", SHAPES)
@pytest.mark.parametrize("N", [1, 31, 33, 257])
def test_kernels_against_float64(cuda, N, C, L):
    agg = _module(C, L, cuda, seed=C + L)
    assert agg.takes_fused_path()
    xs, G = _inputs(N, C, L, cuda, 1000 + N + C + L)
    got = _run(agg, xs, G)
    want = R.jk_truth(xs, agg.state_dict(), G)
    errs = _errors(got, want)
    print(f"jk kernels N={N} C={C} L={L} H={agg.lstm.hidden_size}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert got[0].shape == (N, C)
    assert all(v <= TOL for v in errs.values()), errs
    assert float(got[1]["att.bias"].abs().max()) == 0.0                  # exactly zero, not rounding noise


ULP = 2.0 ** -23                   # of a float32 in [1, 2)


def _check_alpha(agg, xs, want_out, want_alpha, relu=False, paths=(True, False)):
    """`jk.lstm_forward` itself, on the fused kernel and on the composed pieces (in chunks of 96 rows where there are more):
    `out` and `alpha` -- which the whole backward is built on -- against float64, the rows of alpha summing to 1 within 4
    ulps (alpha_t = e_t / fl(sum e): L - 1 roundings in the sum and one per quotient, half an ulp each, L <= 8).  Returns the
    worst (out, alpha) error."""
    N, L = xs[0].size(0), len(xs)
    params = [p.detach() for p in agg._lstm_parameters()]
    worst = [0.0, 0.0]
    for fused in paths:
        out, alpha = jk.lstm_forward([x.detach() for x in xs], params, agg.att.weight.detach().reshape(-1),
                                     agg.att.bias.detach(), relu, fused, 96 if N > 96 else jk.DEFAULT_CHUNK_ROWS)
        torch.cuda.synchronize()
        assert out.shape == want_out.shape and alpha.shape == (N, L)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(alpha).all()), fused
        e_out, e_alpha = rel_err(out, want_out), rel_err(alpha, want_alpha)
        off_one = float((alpha.double().sum(1) - 1).abs().max())
        print(f"jk lstm_forward N={N} C={xs[0].size(1)} L={L} relu={relu} fused={fused}: out {e_out:.2e}, alpha {e_alpha:.2e}, "
              f"|sum alpha - 1| {off_one / ULP:.2f} ulp")
        assert e_out <= TOL and e_alpha <= TOL, (fused, e_out, e_alpha)
        assert off_one <= 4 * ULP, (fused, off_one)
        worst = [max(worst[0], e_out), max(worst[1], e_alpha)]
    return worst


def _finite(res):
    return all(bool(torch.isfinite(t).all()) for t in _flat(res))


@pytest.mark.parametrize("C,L", SHAPES)
@pytest.mark.parametrize("N", [1, 31, 33, 257])
def test_alpha_against_float64_on_both_paths(cuda, N, C, L):
    agg = _module(C, L, cuda, seed=C + L)
    xs, _ = _inputs(N, C, L, cuda, 1000 + N + C + L)
    _check_alpha(agg, xs, *R.jk_truth(xs, agg.state_dict(), with_alpha=True))


# Every leaf of the fused forward's dispatch (the table and its reasons: `_jkn_ref.LEAF_SHAPES`), each at one node, at a
# partly filled wave and at one node past a full workgroup: 128 nodes on 4 waves, 64 on 2.
LEAF_CASES = [(N, C, L, waves) for C, L, waves in R.LEAF_SHAPES for N in ((1, 33, 129) if waves == 4 else (1, 33, 65))]


@pytest.mark.parametrize("N,C,L,waves", LEAF_CASES)
def test_every_leaf_of_the_fused_forward_against_float64(cuda, N, C, L, waves):
    """out, alpha and every gradient at each k_jk_fwd<NHB> and workgroup shape, the inputs surrounded by NaN."""
    H = (L * C) // 2
    module_seed, input_seed = R.leaf_seeds(N, C, L)
    agg = _module(C, L, cuda, seed=module_seed, chunk_rows=96)
    assert agg.lstm.hidden_size == H and agg.takes_fused_path()
    # the library answers whether the kernel takes H, not on how many waves: `_jkn_ref.fwd_waves` restates the launcher's
    # arithmetic (139 is the last width on 4 waves, 140 the first on 2) and has to agree with the answer it does give
    assert R.fwd_waves(H) == waves and jk.fused_forward_takes(H)
    xs, G = _inputs(N, C, L, cuda, input_seed, poison=True)
    got = _run(agg, xs, G)
    *want, want_alpha = R.jk_truth(xs, agg.state_dict(), G, with_alpha=True)
    errs = _errors(got, want)
    print(f"jk leaf N={N} C={C} L={L} H={H} NHB={(H + 31) // 32} waves={waves}: "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f", worst gradient {max(v for k, v in errs.items() if k != 'out'):.2e}")
    assert got[0].shape == (N, C) and _finite(got)
    assert all(v <= TOL for v in errs.values()), errs
    assert float(got[1]["att.bias"].abs().max()) == 0.0
    _check_alpha(agg, xs, want[0], want_alpha)


@pytest.mark.parametrize("N,C,L", [(65, 64, 8), (129, 97, 2)])
def test_relu_epilogue_on_the_new_leaves(cuda, N, C, L):
    module_seed, input_seed = R.leaf_seeds(N, C, L)
    agg = _module(C, L, cuda, seed=module_seed, chunk_rows=96)
    assert agg.takes_fused_path()
    xs, G = _inputs(N, C, L, cuda, input_seed, poison=True)
    got = _run(agg, xs, G, relu=True)
    *want, want_alpha = R.jk_truth(xs, agg.state_dict(), G, relu=True, with_alpha=True)
    errs = _errors(got, want)
    print(f"jk leaf relu N={N} C={C} L={L}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert _finite(got) and all(v <= TOL for v in errs.values()), errs
    assert float(got[0].min()) >= 0.0 and bool((got[0] == 0).any())
    _check_alpha(agg, xs, want[0], want_alpha, relu=True)


@pytest.mark.parametrize("N", [33, 129])
def test_a_width_beyond_the_fused_kernel_takes_the_composed_path(cuda, N):
    """H = 257: nine blocks of hidden units.  The switch stays on; the module goes to the composed pieces on its own."""
    C, L = 257, 2
    module_seed, input_seed = R.leaf_seeds(N, C, L)
    agg = _module(C, L, cuda, seed=module_seed, chunk_rows=96)
    assert agg.lstm.hidden_size == 257 and R.fwd_waves(257) == 0
    assert not jk.fused_forward_takes(257) and not agg.takes_fused_path()
    xs, G = _inputs(N, C, L, cuda, input_seed, poison=True)
    got = _run(agg, xs, G)
    *want, want_alpha = R.jk_truth(xs, agg.state_dict(), G, with_alpha=True)
    errs = _errors(got, want)
    print(f"jk composed N={N} C={C} L={L} H=257: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert _finite(got) and all(v <= TOL for v in errs.values()), errs
    assert float(got[1]["att.bias"].abs().max()) == 0.0
    _check_alpha(agg, xs, want[0], want_alpha, paths=(False,))


def test_inputs_scaled_by_four_against_float64(cuda):
    """Saturated gates and a peaked softmax."""
    N, C, L = 257, 33, 4
    agg = _module(C, L, cuda, seed=2)
    xs, G = _inputs(N, C, L, cuda, 5, scale=4.0)
    errs = _errors(_run(agg, xs, G), R.jk_truth(xs, agg.state_dict(), G))
    print("jk kernels, inputs x 4: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs


def test_no_rows_return_an_empty_result_without_a_launch(cuda):
    agg = _module(8, 2, cuda)
    for fused in (True, False):
        was = jk.enable_fused_jk(fused)
        try:
            xs, G = _inputs(0, 8, 2, cuda, 1)
            out, g = _run(agg, xs, G)
        finally:
            jk.enable_fused_jk(was)
        assert out.shape == (0, 8) and all(x.shape == (0, 8) for x in g["x"])
        assert all(float(t.abs().sum()) == 0.0 for t in g["lstm"] + [g["att.weight"], g["att.bias"]])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N,C,L", [(257, 64, 2), (33, 5, 3), (257, 200, 2), (31, 8, 1)])
def test_fused_and_composed_forward_agree(cuda, N, C, L, relu):
    agg = _module(C, L, cuda, seed=3, chunk_rows=96)
    xs, G = _inputs(N, C, L, cuda, 7 + N)
    want = R.jk_truth(xs, agg.state_dict(), G, relu=relu)
    res = {}
    for fused in (True, False):
        was = jk.enable_fused_jk(fused)
        try:
            assert agg.takes_fused_path() is fused
            res[fused] = _run(agg, xs, G, relu=relu)
        finally:
            jk.enable_fused_jk(was)
        errs = _errors(res[fused], want)
        print(f"jk N={N} C={C} L={L} relu={relu} fused={fused}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert all(v <= TOL for v in errs.values()), (fused, errs)
    a, b = res[True][0], res[False][0]
    assert rel_err(a, b) <= TOL and rel_err(b, a) <= TOL
    if relu:
        assert float(a.min()) >= 0.0 and float(b.min()) >= 0.0 and bool((a == 0).any())


def test_chunked_backward_matches_one_chunk_and_is_reproducible(cuda):
    N, C, L = 257, 64, 2
    xs, G = _inputs(N, C, L, cuda, 11)
    want = None
    for chunk_rows in (96, None):                           # 96 does not divide 257
        agg = _module(C, L, cuda, seed=4, chunk_rows=chunk_rows)
        want = want or R.jk_truth(xs, agg.state_dict(), G, relu=True)
        for fused in (True, False):
            was = jk.enable_fused_jk(fused)
            try:
                first, second = _run(agg, xs, G, relu=True), _run(agg, xs, G, relu=True)
            finally:
                jk.enable_fused_jk(was)
            errs = _errors(first, want)
            print(f"jk chunk_rows={chunk_rows} fused={fused}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            assert all(v <= TOL for v in errs.values()), (chunk_rows, errs)
            assert all(torch.equal(a, b) for a, b in zip(_flat(first), _flat(second)))      # bit for bit, run to run


def test_workspace_is_bounded_by_chunk_rows_not_by_n(cuda):
    """A condition, not a measurement: the peak memory of a forward + backward may grow from N = 4 r to N = 16 r by the
    N-proportional tensors the caller sees (the L inputs, their gradients, G, out, alpha) plus 1 MiB, and by nothing of
    size N x H."""
    r, C, L = 4096, 64, 2
    agg = _module(C, L, cuda, chunk_rows=r)
    peak = {}
    for N in (r, 4 * r, 16 * r):                            # the first round warms the allocator and the kernels
        xs = [torch.randn(N, C, device=cuda).requires_grad_() for _ in range(L)]
        G = torch.randn(N, C, device=cuda)
        agg.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = agg(xs)
        out.backward(G)
        torch.cuda.synchronize()
        peak[N] = torch.cuda.max_memory_allocated()
        assert all(x.grad.shape == (N, C) for x in xs)
        del xs, G, out
    growth = peak[16 * r] - peak[4 * r]
    allowed = 12 * r * 4 * (L * C + L * C + C + C + L) + (1 << 20)
    print(f"jk peak memory: N=4r {peak[4 * r] / 2**20:.1f} MiB, N=16r {peak[16 * r] / 2**20:.1f} MiB, growth "
          f"{growth / 2**20:.1f} MiB, allowed {allowed / 2**20:.1f} MiB")
    assert growth <= allowed, (peak, allowed)


# ------------------------------------------------------------------------------------------------
# the model against the restatement
# ------------------------------------------------------------------------------------------------
def _identity(n):
    ar = torch.arange(n)
    return torch.sparse_coo_tensor(torch.stack([ar, ar]), torch.ones(n), (n, n)).coalesce()


def _tiny():
    z = np.load(os.path.join(GOLD, "tiny_textgcn.npz"))
    N = int(z["y"].shape[0])
    return pkg.Data(x=_identity(N), edge_index=torch.from_numpy(z["edge_index"]), edge_attr=torch.from_numpy(z["edge_attr"]),
                    y=torch.from_numpy(z["y"]), train_mask=torch.from_numpy(z["train_mask"])), 3


def _to(g, dev):
    return pkg.Data(**{k: getattr(g, k) for k in ("x", "edge_index", "edge_attr", "y", "train_mask")}).to(dev)


def _step(model, g):
    logits = model(g)
    loss = nn.CrossEntropyLoss()(logits[g.train_mask], g.y[g.train_mask])
    model.zero_grad(set_to_none=True)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _compare(tag, got, want):
    (gl, gloss, gg), (wl, wloss, wg) = got, want
    assert set(gg) == set(wg)
    errs = {"logits": rel_err(gl, wl), "loss": abs(gloss.item() - wloss.item()) / abs(wloss.item())}
    errs.update({k: rel_err(gg[k], wg[k]) for k in wg if k != "jk.att.bias"})
    # exact zeros here, float32 rounding noise in the restatement: absolute, at the scale of the neighbouring gradient
    scale = wg["jk.att.weight"].abs().max().item()
    errs["jk.att.bias"] = (gg["jk.att.bias"].cpu() - wg["jk.att.bias"]).abs().max().item() / max(scale, 1e-30)
    print(f"JKN parity {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert float(gg["jk.att.bias"].abs().max()) == 0.0
    assert all(v <= TOL for v in errs.values()), (tag, errs)


def _pair(N, n_classes, dev, n_gcn=2, h=16, dropout=0.0, activation=nn.ReLU, seed=0):
    torch.manual_seed(seed)
    ref = JKNRef(N, n_classes, n_gcn=n_gcn, n_hidden_gcn=h, activation=activation, dropout=dropout)
    mine = pkg.JumpingKnowledgeNetwork(N, n_classes, n_gcn=n_gcn, n_hidden_gcn=h, activation=activation, dropout=dropout)
    mine.load_state_dict(ref.state_dict(), strict=True)
    return ref, mine.to(dev).float()


@pytest.mark.parametrize("n_gcn", [2, 3])
def test_model_matches_the_restatement(cuda, n_gcn):
    g, n_classes = _tiny()
    gd = _to(g, cuda)
    ref, mine = _pair(g.x.size(0), n_classes, cuda, n_gcn=n_gcn, seed=n_gcn)
    want_train = _step(ref.train(), g)                       # training mode, dropout = 0
    with torch.no_grad():
        want_eval = ref.eval()(g)
    for fused in (True, False):
        was = jk.enable_fused_jk(fused)
        try:
            got = _step(mine.train(), gd)
            with torch.no_grad():
                got_eval = mine.eval()(gd)
        finally:
            jk.enable_fused_jk(was)
        _compare(f"tiny_textgcn n_gcn={n_gcn} fused={fused}", got, want_train)
        assert rel_err(got_eval, want_eval) <= TOL
        assert torch.equal(got_eval, got[0])                 # eval equals train at p = 0


def test_a_non_relu_activation_takes_the_module_path_and_matches(cuda):
    g, n_classes = _tiny()
    ref, mine = _pair(g.x.size(0), n_classes, cuda, activation=nn.ELU, seed=5)
    assert isinstance(mine.activation, nn.ELU)
    _compare("tiny_textgcn ELU", _step(mine.train(), _to(g, cuda)), _step(ref.train(), g))


def test_dropout_draws_from_torchs_stream(cuda):
    g, n_classes = _tiny()
    gd = _to(g, cuda)
    _, mine = _pair(g.x.size(0), n_classes, cuda, dropout=0.5, seed=6)
    mine.train()
    outs = []
    for seed in (1, 1, 2):
        torch.manual_seed(seed)
        outs.append(mine(gd).detach())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    with torch.no_grad():
        assert torch.equal(mine.eval()(gd), mine.eval()(gd))
    pkg.enable_fused_dropout(True)                           # does not apply to this model: still torch's stream
    try:
        torch.manual_seed(1)
        assert torch.equal(mine.train()(gd).detach(), outs[0])
    finally:
        pkg.enable_fused_dropout(False)


def test_twenty_adam_steps_follow_the_restatement(cuda):
    """Bar: 1e-4 relative on the loss at every step -- one decade over the per-step 1e-5, for the error compounding through
    the optimiser (the bar and the reasoning of the EGCN test of the same name)."""
    N, n_classes = 2000, 6
    g = synth.word_doc_graph(N, 30000, seed=44, n_classes=n_classes)
    ref, mine = _pair(N, n_classes, cuda, h=32)
    ref.train(), mine.train()
    gd = _to(g, cuda)
    opts = [torch.optim.Adam(m.parameters(), lr=0.02) for m in (ref, mine)]
    crit = nn.CrossEntropyLoss()
    worst, curve = 0.0, []
    for step in range(20):
        losses = []
        for m, gg, opt in ((ref, g, opts[0]), (mine, gd, opts[1])):
            loss = crit(m(gg)[gg.train_mask], gg.y[gg.train_mask])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        curve.append(losses)
        worst = max(worst, abs(losses[1] - losses[0]) / abs(losses[0]))
    print(f"JKN 20 Adam steps: loss {curve[0][1]:.6f} -> {curve[-1][1]:.6f} (restatement {curve[0][0]:.6f} -> "
          f"{curve[-1][0]:.6f}), worst relative difference {worst:.2e}")
    assert curve[-1][0] < curve[0][0]                        # it does train
    assert worst <= 1e-4, curve


def test_two_host_threads_do_not_disturb_each_other_and_a_side_stream_works(cuda):
    N, C, L = 1025, 64, 2
    agg = _module(C, L, cuda, seed=8)
    cases = [_inputs(N, C, L, cuda, s) for s in (21, 22)]
    alone = [_run(agg, xs, G) for xs, G in cases]
    assert not torch.equal(alone[0][0], alone[1][0])
    got, errors = [None, None], []

    def work(i):
        try:
            xs = [x.detach() for x in cases[i][0]]
            with torch.no_grad():
                for _ in range(20):
                    got[i] = agg(xs)
            torch.cuda.synchronize()
        except Exception as e:                               # noqa: BLE001 -- reported by the assertion below
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert torch.equal(got[0], alone[0][0]) and torch.equal(got[1], alone[1][0])      # no hidden state between the calls
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = _run(agg, *cases[0])
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(_flat(res), _flat(alone[0])))
    errs = _errors(res, R.jk_truth(cases[0][0], agg.state_dict(), cases[0][1]))
    assert all(v <= TOL for v in errs.values()), errs
