"""GPU tests of EGCN and of its fused front end (libtgcn.so `tgcn_embed_xw*`, pytextgcn_amd/csrc/embed.hip).

The kernels are held to a float64 restatement (tests/_egcn_ref.py) at the project's bar, max|a - b| / max|b| <= 1e-5
(BASELINE.json): an fp32 evaluation of the same expressions on the CPU sits at 2.5e-7 .. 6.5e-7 from float64 at
(N, K, n) = (3000, 2000, 100), (4097, 515, 200), (2000, 2000, 64) with E, b ~ U(+-1/sqrt(N)) and W glorot, so the bar leaves
more than ten-fold room.  On ROUNDED_CASES (the tile counts that are rounded up to a leaf, operands surrounded by NaN) the
kernels on an MI355X stay within C 4.2e-7, dE 4.8e-7, db 3.9e-7, dW 4.3e-7, and a column's bits do not depend on the leaf
that serves it (torch.equal, no tolerance).  The dropout mask is held to tests/_dropout_hash.py bit for bit.  The model is
held to the reference's EGCN restated from torch's Linear / selu / dropout and the CPU oracle's GCNConv."""
import math
import os
import threading

import numpy as np
import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from pytextgcn_amd import embed, synth

import _egcn_ref as R
from _egcn_ref import EGCNRef, rel_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-5


def _operands(N, K, n, seed, dev, lde_extra=0):
    gen = torch.Generator().manual_seed(seed)
    a = 1.0 / math.sqrt(max(N, 1))
    Ebuf = (torch.rand(K, N + lde_extra, generator=gen) * 2 - 1) * a
    b = (torch.rand(K, generator=gen) * 2 - 1) * a
    g = math.sqrt(6.0 / (K + n))
    W = (torch.rand(K, n, generator=gen) * 2 - 1) * g
    G = torch.randn(N, n, generator=gen)
    Ebuf = Ebuf.to(dev)
    return Ebuf[:, :N], b.to(dev), W.to(dev), G.to(dev)


# every N of {0, 1, 31, 33, 1025, 4097}, K of {1, 2, 63, 515, 2000} and n of {1, 3, 64, 100, 200, 219} appears; N not a
# multiple of 4 nearly everywhere; (lde - N, strided C and G) vary; n = 300 crosses the 256-column group of one launch
CASES = [
    (0, 5, 3, 0, False), (1, 1, 1, 0, False), (31, 2, 3, 0, False), (33, 63, 64, 0, False), (1025, 515, 100, 0, False),
    (4097, 2000, 200, 0, False), (4097, 63, 219, 0, True), (1025, 2000, 1, 3, False), (33, 515, 219, 5, True),
    (1025, 63, 100, 7, True), (4097, 1, 64, 0, False), (31, 2000, 200, 1, False), (1025, 2, 300, 0, True),
    (4097, 515, 3, 2, False), (128, 32, 32, 0, False), (129, 33, 33, 0, False),
]


@pytest.mark.parametrize("N,K,n,lde_extra,strided", CASES)
def test_kernels_against_float64_without_dropout(cuda, N, K, n, lde_extra, strided):
    E, b, W, G = _operands(N, K, n, 1000 + N + K + n, cuda, lde_extra)
    assert E.stride(0) == N + lde_extra or N <= 1
    out = None
    if strided:                                              # a result (and a gradient) with rows wider than n
        wide = torch.full((N, n + 9), 7.0, device=cuda)
        out = wide[:, 4:4 + n]
        Gw = torch.zeros(N, n + 6, device=cuda)
        Gw[:, 2:2 + n] = G
        G = Gw[:, 2:2 + n]
    C = embed.embed_xw_forward(E, b, W, out=out)
    dE, db, dW = embed.embed_xw_backward(E, b, W, G)
    torch.cuda.synchronize()
    assert C.shape == (N, n) and dE.shape == (K, N) and db.shape == (K,) and dW.shape == (K, n)
    if strided:
        assert bool((wide[:, :4] == 7.0).all()) and bool((wide[:, 4 + n:] == 7.0).all())   # nothing outside the n columns
    if N == 0:
        assert float(db.abs().sum()) == 0.0 and float(dW.abs().sum()) == 0.0
        return
    tC, tE, tb, tW = R.fused_truth(E, b, W, G)
    errs = {"C": rel_err(C, tC), "dE": rel_err(dE, tE), "db": rel_err(db, tb), "dW": rel_err(dW, tW)}
    print(f"embed kernels N={N} K={K} n={n}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    # the weight gradient on its own, and the input / bias gradients on their own, are the same numbers
    only_w = embed.embed_xw_backward(E, b, W, G, want_e=False)
    only_e = embed.embed_xw_backward(E, b, W, G, want_w=False)
    assert only_w[0] is None and only_e[2] is None
    assert torch.equal(only_w[2], dW) and torch.equal(only_e[0], dE) and torch.equal(only_e[1], db)


# The forward and dE serve a group of nt = ceil(ng / 32) column tiles on the next leaf of NT in {1, 2, 4, 7, 8}; CASES runs
# every leaf at its own tile count only.  Here the leaves that are rounded up to: nt = 3 on NT = 4 (n = 65, 96: the fourth
# tile is all padding), nt = 5 and 6 on NT = 7 (n = 129, 160, 192), seven full tiles (224), the k_embed_grad_w<1 | 2>
# boundary (128 | 129), a full group followed by a group of one column (256 | 257) and three groups (513).  K in {33, 63}
# and N in {33, 129} are enough for that: one and two chunks of k, one and two tiles of rows, a tail in each.  Same layout
# as CASES; about a third with lde > N and column slices for C and G.
ROUNDED_CASES = [
    (33, 33, 65, 0, False), (129, 63, 96, 3, True), (129, 63, 65, 0, False), (129, 33, 129, 0, False), (33, 63, 160, 1, True),
    (129, 63, 192, 0, False), (33, 33, 128, 5, False), (129, 33, 224, 0, False), (33, 63, 256, 0, False),
    (129, 63, 257, 2, True), (33, 33, 513, 0, False), (129, 63, 513, 7, True),
]


def _in_nan(rows, cols, values, dev, row0=0, col0=0, more_rows=2, more_cols=0):
    """`values` [rows, cols] as a slice of a buffer that is NaN everywhere else: a read outside the operand shows."""
    buf = torch.full((row0 + rows + more_rows, col0 + cols + more_cols), float("nan"), device=dev)
    view = buf[row0:row0 + rows, col0:col0 + cols]
    view.copy_(values)
    return view


@pytest.mark.parametrize("N,K,n,lde_extra,strided", ROUNDED_CASES)
def test_rounded_up_leaves_against_float64_among_nan(cuda, N, K, n, lde_extra, strided):
    """The checks of `test_kernels_against_float64_without_dropout` with every operand surrounded by NaN: Ebuf's columns past
    N and two rows past K, W's rows past K and columns past n, G's surroundings.  No result may hold one."""
    E, b, W, G = _operands(N, K, n, 1000 + N + K + n, cuda, lde_extra)
    E = _in_nan(K, N, E, cuda, more_cols=lde_extra)
    W = _in_nan(K, n, W, cuda, more_cols=3)
    assert E.stride(0) == N + lde_extra and W.stride(0) == n + 3
    out = None
    if strided:
        wide = torch.full((N, n + 9), 7.0, device=cuda)
        out = wide[:, 4:4 + n]
        G = _in_nan(N, n, G, cuda, col0=2, more_cols=4)
    else:
        G = _in_nan(N, n, G, cuda)
    C = embed.embed_xw_forward(E, b, W, out=out)
    dE, db, dW = embed.embed_xw_backward(E, b, W, G)
    torch.cuda.synchronize()
    assert C.shape == (N, n) and dE.shape == (K, N) and db.shape == (K,) and dW.shape == (K, n)
    if strided:
        assert bool((wide[:, :4] == 7.0).all()) and bool((wide[:, 4 + n:] == 7.0).all())   # nothing outside the n columns
    assert all(bool(torch.isfinite(t).all()) for t in (C, dE, db, dW))
    tC, tE, tb, tW = R.fused_truth(E, b, W, G)
    errs = {"C": rel_err(C, tC), "dE": rel_err(dE, tE), "db": rel_err(db, tb), "dW": rel_err(dW, tW)}
    print(f"embed kernels, rounded-up leaves, N={N} K={K} n={n}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    only_w = embed.embed_xw_backward(E, b, W, G, want_e=False)
    only_e = embed.embed_xw_backward(E, b, W, G, want_w=False)
    assert torch.equal(only_w[2], dW) and torch.equal(only_e[0], dE) and torch.equal(only_e[1], db)


_FULL_GROUP = {}


def _full_group(dev):
    """Operands with n = 256 columns -- eight full tiles on NT = 8, dW on k_embed_grad_w<2> -- and their C and dW, once."""
    if not _FULL_GROUP:
        E, b, W, G = _operands(129, 63, 256, 4242, dev)
        _FULL_GROUP["v"] = (E, b, W, G, embed.embed_xw_forward(E, b, W), embed.embed_xw_backward(E, b, W, G, want_e=False)[2])
    return _FULL_GROUP["v"]


@pytest.mark.parametrize("n1", [65, 96, 129, 192])
def test_bits_of_a_column_do_not_depend_on_the_leaf_that_serves_it(cuda, n1):
    """By construction, no tolerance.  An element of C is accumulated over k in the same order whichever NT serves its tile
    (`acc[t]` of k_embed_fwd depends on its own column only), so the forward on W[:, :n1] -- NT = 4 or 7 with padding tiles
    -- gives the first n1 columns of the forward on all 256.  The row slices of dW are set by N and K alone (`grad_w_split`)
    and k_embed_reduce_w adds them in slice order under either TW (two slices here), so the same holds for dW with
    G[:, :n1].  A difference means a leaf sums in another order or reads its padding."""
    E, b, W, G, C, dW = _full_group(cuda)
    W1, G1 = W[:, :n1], G[:, :n1]
    assert W1.stride(0) == 256 and G1.stride(0) == 256
    assert torch.equal(embed.embed_xw_forward(E, b, W1), C[:, :n1])
    assert torch.equal(embed.embed_xw_backward(E, b, W1, G1, want_e=False)[2], dW[:, :n1])


def _seed_tensor(value, dev):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def test_mask_is_the_documented_hash_bit_for_bit(cuda):
    N, K, p = 300, 64, 0.5
    gen = torch.Generator().manual_seed(5)
    sign = torch.where(torch.rand(K, N, generator=gen) < 0.5, -1.0, 1.0)
    E = (sign * (0.2 + 0.8 * torch.rand(K, N, generator=gen))).to(cuda)          # |E| >= 0.2
    b = ((torch.rand(K, generator=gen) * 2 - 1) * 0.1).to(cuda)                   # |b| <= 0.1: E + b != 0 everywhere
    W = torch.eye(K, device=cuda)
    G = (0.5 + torch.rand(N, K, generator=gen)).to(cuda)                          # non-zero
    for value in (0x1234567890ABCDE, -77, 1 << 40):
        seed = _seed_tensor(value, cuda)
        keep = R.keep_matrix(value, N, K, p)
        C = embed.embed_xw_forward(E, b, W, p, seed)
        assert torch.equal((C != 0).cpu(), keep)
        want = torch.selu(E.t().double().cpu() + b.double().cpu()) / (1 - p)
        got = C.double().cpu()
        assert float(((got - want).abs() / want.abs())[keep].max()) <= 1e-6
        assert torch.equal(embed.embed_xw_forward(E, b, W, p, seed), C)          # the same seed: the same bits
        dE, db, dW = embed.embed_xw_backward(E, b, W, G, p, seed)
        assert torch.equal((dE != 0).cpu(), keep.t())                            # the backward takes the same decisions
        tC, tE, tb, tW = R.fused_truth(E, b, W, G, keep, p)
        assert max(rel_err(C, tC), rel_err(dE, tE), rel_err(db, tb), rel_err(dW, tW)) <= TOL
    other = embed.embed_xw_forward(E, b, W, p, _seed_tensor(12345, cuda))
    assert not torch.equal(other != 0, C != 0)
    # p = 0 and a missing seed both mean "no mask"
    plain = embed.embed_xw_forward(E, b, W)
    assert torch.equal(embed.embed_xw_forward(E, b, W, 0.0, seed), plain)
    assert torch.equal(embed.embed_xw_forward(E, b, W, 0.5, None), plain) and bool((plain != 0).all())


@pytest.mark.parametrize("p", [0.3, 0.7])
@pytest.mark.parametrize("N,K,n", [(1025, 515, 100), (333, 2000, 64), (4097, 63, 219)])
def test_training_gradients_with_the_mask_against_float64(cuda, p, N, K, n):
    E, b, W, G = _operands(N, K, n, 77 + N, cuda)
    E, b, W = (t.clone().requires_grad_() for t in (E, b, W))
    value = -(N * 1_000_003 + K)
    seed = _seed_tensor(value, cuda)
    C = embed.embed_xw(E, b, W, p, seed)
    C.backward(G)
    tC, tE, tb, tW = R.fused_truth(E, b, W, G, R.keep_matrix(value, N, K, p), p)
    errs = {"C": rel_err(C, tC), "dE": rel_err(E.grad, tE), "db": rel_err(b.grad, tb), "dW": rel_err(W.grad, tW)}
    print(f"embed kernels with mask p={p} N={N} K={K} n={n}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------
# the model against the restatement
# ------------------------------------------------------------------------------------------------
def _identity(n):
    ar = torch.arange(n)
    return torch.sparse_coo_tensor(torch.stack([ar, ar]), torch.ones(n), (n, n)).coalesce()


def _labels(n, n_classes, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_classes, (n,), generator=gen), torch.rand(n, generator=gen) < 0.6


def _graph(name):
    if name == "tiny_textgcn":
        z = np.load(os.path.join(GOLD, "tiny_textgcn.npz"))
        N = int(z["y"].shape[0])
        return pkg.Data(x=_identity(N), edge_index=torch.from_numpy(z["edge_index"]), edge_attr=torch.from_numpy(z["edge_attr"]),
                        y=torch.from_numpy(z["y"]), train_mask=torch.from_numpy(z["train_mask"])), 3
    if name == "random53":
        z = np.load(os.path.join(GOLD, "random53.npz"))
        N = int(z["n"])
        y, mask = _labels(N, 5, 53)
        return pkg.Data(x=_identity(N), edge_index=torch.from_numpy(z["edge_index"]),
                        edge_attr=torch.from_numpy(z["edge_weight"]), y=y, train_mask=mask), 5
    docs, y = synth.synthetic_corpus(2000, 1500, n_classes=6, seed=44)
    perm = np.random.default_rng(0).permutation(len(docs))
    t2g = pkg.Text2GraphTransformer(n_jobs=8, min_df=5, window_size=5, rm_stopwords=False, verbose=0, max_df=0.7)
    g = t2g.fit_transform(docs, y, test_idx=perm[:200], val_idx=perm[200:400])
    return g, 6


def _to(g, dev, x=None):
    d = {k: getattr(g, k) for k in ("edge_index", "edge_attr", "y", "train_mask")}
    return pkg.Data(x=g.x if x is None else x, **d).to(dev)


def _step(model, g):
    logits = model(g)
    loss = nn.CrossEntropyLoss()(logits[g.train_mask], g.y[g.train_mask])
    model.zero_grad(set_to_none=True)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _compare(tag, got, want):
    (gl, gloss, gg), (wl, wloss, wg) = got, want
    errs = {"logits": rel_err(gl, wl), "loss": abs(gloss.item() - wloss.item()) / abs(wloss.item())}
    errs.update({k: rel_err(gg[k], wg[k]) for k in wg})
    print(f"EGCN parity {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert set(gg) == set(wg)
    assert all(v <= TOL for v in errs.values()), (tag, errs)


@pytest.mark.parametrize("n_gcn", [2, 3])
@pytest.mark.parametrize("name", ["tiny_textgcn", "random53", "corpus2000"])
def test_model_matches_the_restatement(cuda, name, n_gcn):
    g, n_classes = _graph(name)
    N = g.x.size(0)
    torch.manual_seed(n_gcn)
    ref = EGCNRef(N, n_classes, embedding_dim=48, n_gcn=n_gcn, n_hidden_gcn=20, dropout=0.0)
    mine = pkg.EGCN(N, n_classes, embedding_dim=48, n_gcn=n_gcn, n_hidden_gcn=20, dropout=0.0)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(cuda).float()
    gd = _to(g, cuda)
    want_train = _step(ref.train(), g)                       # training mode, dropout = 0
    with torch.no_grad():
        want_eval = ref.eval()(g)
    for fused in (True, False):
        was = pkg.enable_fused_embedding(fused)
        try:
            assert mine.train().takes_fused_path(gd.x) is fused
            got = _step(mine, gd)
            with torch.no_grad():
                got_eval = mine.eval()(gd)
        finally:
            pkg.enable_fused_embedding(was)
        _compare(f"{name} n_gcn={n_gcn} fused={fused}", got, want_train)
        assert rel_err(got_eval, want_eval) <= TOL
        if fused:
            fused_out = got
    _compare(f"{name} n_gcn={n_gcn} unfused against fused", got, fused_out)


def test_other_feature_formats_take_the_composition_and_match(cuda):
    """[I | H] (hierarchy_feats), dense identity and a general sparse matrix: the unfused path, same bar."""
    g, n_classes = _graph("random53")
    N = g.x.size(0)
    gen = torch.Generator().manual_seed(9)
    Fh = 7
    hi = torch.stack([torch.randint(0, N, (90,), generator=gen), torch.randint(0, Fh, (90,), generator=gen)])
    H = torch.sparse_coo_tensor(hi, torch.rand(90, generator=gen), (N, Fh)).coalesce()
    ar = torch.arange(N)
    IH = torch.sparse_coo_tensor(torch.cat([torch.stack([ar, ar]), torch.stack([H.indices()[0], H.indices()[1] + N])], 1),
                                 torch.cat([torch.ones(N), H.values()]), (N, N + Fh)).coalesce()
    gi = torch.stack([torch.randint(0, N, (200,), generator=gen), torch.randint(0, N, (200,), generator=gen)])
    general = torch.sparse_coo_tensor(gi, torch.randn(200, generator=gen), (N, N)).coalesce()
    for tag, x in (("[I|H]", IH), ("dense identity", torch.eye(N)), ("general sparse", general)):
        torch.manual_seed(1)
        ref = EGCNRef(x.size(1), n_classes, embedding_dim=40, n_hidden_gcn=12, dropout=0.0)
        mine = pkg.EGCN(x.size(1), n_classes, embedding_dim=40, n_hidden_gcn=12, dropout=0.0)
        mine.load_state_dict(ref.state_dict())
        mine = mine.to(cuda).float().train()
        gd = _to(g, cuda, x)
        assert not mine.takes_fused_path(gd.x)
        _compare(tag, _step(mine, gd), _step(ref.train(), _to(g, "cpu", x)))


def test_twenty_adam_steps_follow_the_restatement(cuda):
    """Bar: 1e-4 relative on the loss at every step -- one decade over the per-step 1e-5, for the error compounding through
    the optimiser."""
    N, n_classes = 2000, 6
    g = synth.word_doc_graph(N, 30000, seed=44, n_classes=n_classes)
    torch.manual_seed(0)
    ref = EGCNRef(N, n_classes, embedding_dim=64, n_hidden_gcn=32, dropout=0.0).train()
    mine = pkg.EGCN(N, n_classes, embedding_dim=64, n_hidden_gcn=32, dropout=0.0)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(cuda).float().train()
    gd = _to(g, cuda)
    assert mine.takes_fused_path(gd.x)
    opts = [torch.optim.Adam(m.parameters(), lr=0.02) for m in (ref, mine)]
    crit = nn.CrossEntropyLoss()
    worst = 0.0
    curve = []
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
    print(f"EGCN 20 Adam steps: loss {curve[0][1]:.6f} -> {curve[-1][1]:.6f} (restatement {curve[0][0]:.6f} -> "
          f"{curve[-1][0]:.6f}), worst relative difference {worst:.2e}")
    assert curve[-1][0] < curve[0][0]                        # it does train
    assert worst <= 1e-4, curve


def test_fused_path_holds_one_n_by_k_matrix_and_the_composition_more_than_two_and_a_half(cuda):
    """A condition, not a measurement: extra peak memory of one training forward + backward, in units of N K 4 bytes.  The
    fused path has to hold dE (one N x K matrix, the parameter's gradient) and nothing else of that size; the composition
    holds dE plus at least the pre-activation and the dropped activation.  Every other tensor of the step is at most
    N x h = 5 % of N x K."""
    N, K, h, n_classes = 20000, 2000, 100, 6
    g = _to(synth.word_doc_graph(N, 200000, seed=44, n_classes=n_classes), cuda)
    torch.manual_seed(0)
    model = pkg.EGCN(N, n_classes, embedding_dim=K, n_hidden_gcn=h, dropout=0.5).to(cuda).float().train()
    unit = N * K * 4
    pkg.enable_fused_dropout(True)
    extra = {}
    try:
        for fused in (True, False):
            was = pkg.enable_fused_embedding(fused)
            try:
                assert model.takes_fused_path(g.x) is fused
                for measured in (False, True):               # the first round builds the plan and warms the caches
                    model.zero_grad(set_to_none=True)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    loss = nn.CrossEntropyLoss()(model(g)[g.train_mask], g.y[g.train_mask])
                    loss.backward()
                    torch.cuda.synchronize()
                    extra[fused] = (torch.cuda.max_memory_allocated() - base) / unit
                    del loss
            finally:
                pkg.enable_fused_embedding(was)
    finally:
        pkg.enable_fused_dropout(False)
    print(f"EGCN extra peak memory of a training step in units of N K 4 B: fused {extra[True]:.3f}, "
          f"composition {extra[False]:.3f}")
    assert extra[True] < 1.5, extra
    assert extra[False] > 2.5, extra


def test_two_host_threads_each_get_their_own_mask_and_a_side_stream_works(cuda):
    N, K, n, p = 1025, 515, 100, 0.5
    E, b, W, _ = _operands(N, K, n, 3, cuda)
    seeds = [_seed_tensor(v, cuda) for v in (11, 22)]
    alone = [embed.embed_xw_forward(E, b, W, p, s) for s in seeds]
    torch.cuda.synchronize()
    assert not torch.equal(alone[0], alone[1])
    got = [None, None]
    errors = []

    def work(i):
        try:
            for _ in range(20):
                got[i] = embed.embed_xw_forward(E, b, W, p, seeds[i])
            torch.cuda.synchronize()
        except Exception as e:                               # noqa: BLE001 -- reported by the assertion below
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert torch.equal(got[0], alone[0]) and torch.equal(got[1], alone[1])     # no hidden state between the calls
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        C = embed.embed_xw_forward(E, b, W, p, seeds[0])
        dE, db, dW = embed.embed_xw_backward(E, b, W, torch.ones(N, n, device=cuda), p, seeds[0])
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    ref = embed.embed_xw_backward(E, b, W, torch.ones(N, n, device=cuda), p, seeds[0])
    torch.cuda.synchronize()
    assert torch.equal(C, alone[0]) and all(torch.equal(x, y) for x, y in zip((dE, db, dW), ref))
