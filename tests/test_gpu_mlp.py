"""GPU tests of MLP and of its fused products (libtgcn.so `tgcn_mlp_act_linear*`, pytextgcn_amd/csrc/mlp.hip).

The kernels are held to a float64 restatement (tests/_mlp_ref.py) at the project's bar, max|a - b| / max|b| <= 1e-5
(BASELINE.json).  An fp32 evaluation of the same expressions on the CPU (Z ~ U(+-1), b ~ U(+-0.1), W glorot,
G ~ N(0, 1); p in {0, 0.3, 0.7}) sits at 1.0e-7 .. 8.9e-7 from float64 over C, dZ, db, dW and dc at (N, k, n) = (1025, 256,
128), (333, 515, 33), (129, 63, 219), (1025, 257, 219), (33, 515, 300), (1025, 515, 3), (1025, 1, 32), (31, 256, 300),
(1, 257, 33), (1025, 128, 129), (4100, 515, 3) and (8300, 256, 33) -- the worst is dW at (333, 515, 33) -- so the bar leaves more than ten-fold room at every
shape used here and no operand is rescaled.  On ROUNDED_CASES (the forward's tile counts that are rounded up to a leaf,
operands surrounded by NaN) the kernels on an MI355X stay within C 4.0e-7, dZ 3.2e-7, db 3.2e-7, dW 4.3e-7, and a column's
bits do not depend on the leaf that serves it (torch.equal, no tolerance).
The dropout mask is held to tests/_dropout_hash.py bit for bit.  The model is held to the reference's MLP restated from
torch's Linear / SELU / Dropout (tests/_mlp_ref.MLPRef) in float64."""
import math

import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from pytextgcn_amd import dense, mlp

import _mlp_ref as R
from _mlp_ref import MLPRef, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5


def operands(N, k, n, seed, ldz_extra=0):
    """Z ~ U(+-1), b ~ U(+-0.1), W glorot, c ~ U(+-0.1), G ~ N(0, 1) on the CPU; Z is the leading part of a buffer whose rows
    are ldz_extra floats longer."""
    gen = torch.Generator().manual_seed(seed)
    Zbuf = torch.rand(N, k + ldz_extra, generator=gen) * 2 - 1
    b = (torch.rand(k, generator=gen) * 2 - 1) * 0.1
    W = (torch.rand(n, k, generator=gen) * 2 - 1) * math.sqrt(6.0 / (k + n))
    c = (torch.rand(n, generator=gen) * 2 - 1) * 0.1
    G = torch.randn(N, n, generator=gen)
    return Zbuf, b, W, c, G


def _on(dev, N, k, n, seed, ldz_extra=0):
    Zbuf, b, W, c, G = (t.to(dev) for t in operands(N, k, n, seed, ldz_extra))
    return Zbuf[:, :k], b, W, c, G


# (N, k, n, ldz - k, C and G column slices of wider buffers, output bias given).  Every N of {0, 1, 31, 33, 129, 1025}, k of
# {1, 2, 63, 128, 256, 257, 515} and n of {1, 3, 32, 33, 128, 219, 300} appears; ldz % 4 != 0 in most (259, 521, 63, 3, ...).
# The forward and dW run n in groups of 256 (n = 300 crosses it), dZ reduces over n in groups of 128 (n = 129, 219, 300
# cross it, n = 128 fills it); every kernel walks k in chunks of 32 and rows in tiles of 128 (N = 129, 1025 cross it).
# dW cuts the rows into at most min(256, 512 / ceil(k / 32)) slices of whole 128-row chunks; only with more chunks than that
# does a workgroup walk SEVERAL chunks (re-staging its tile, summing over them).  The last two cases do: N = 4100, k = 515
# is 33 chunks in 17 slices of 2 (the last slice has one chunk, of 4 rows), N = 8300, k = 256 is 65 chunks in 33 slices of
# 2 (the last slice one chunk of 108 rows).
CASES = [
    (0, 5, 3, 0, False, True), (1, 1, 1, 0, False, False), (31, 2, 3, 1, False, True), (33, 63, 32, 0, False, False),
    (129, 128, 33, 3, True, True), (1025, 256, 128, 0, False, True), (1025, 257, 219, 2, True, False),
    (33, 515, 300, 6, True, True), (129, 63, 128, 0, False, False), (1025, 1, 32, 0, False, True),
    (31, 256, 300, 1, False, False), (1025, 515, 3, 2, False, True), (129, 2, 219, 0, True, False),
    (33, 128, 1, 0, False, True), (1, 257, 33, 0, False, False), (129, 32, 32, 0, False, True),
    (1025, 128, 129, 0, False, False), (4100, 515, 3, 2, False, True), (8300, 256, 33, 0, True, False),
]
GRAD_SHAPES = [(1025, 256, 128), (333, 515, 33), (129, 63, 219)]
MULTI_CHUNK_SHAPES = [(4100, 515, 3), (8300, 256, 33)]      # dW with two chunks per slice and a ragged last slice


@pytest.mark.parametrize("N,k,n,ldz_extra,strided,with_c", CASES)
def test_kernels_against_float64_without_dropout(cuda, N, k, n, ldz_extra, strided, with_c):
    Z, b, W, c, G = _on(cuda, N, k, n, 1000 + N + k + n, ldz_extra)
    assert Z.stride(0) == k + ldz_extra or N <= 1
    c = c if with_c else None
    out = None
    if strided:                                              # a result and a gradient that are column slices
        wide = torch.full((N, n + 9), 7.0, device=cuda)
        out = wide[:, 5:5 + n]
        Gw = torch.zeros(N, n + 7, device=cuda)
        Gw[:, 3:3 + n] = G
        G = Gw[:, 3:3 + n]
    C = mlp.act_linear_forward(Z, b, W, c, out=out)
    dZ, db, dW = mlp.act_linear_backward(Z, b, W, G)
    torch.cuda.synchronize()
    assert C.shape == (N, n) and dZ.shape == (N, k) and db.shape == (k,) and dW.shape == (n, k)
    if strided:
        assert bool((wide[:, :5] == 7.0).all()) and bool((wide[:, 5 + n:] == 7.0).all())   # nothing outside the n columns
    if N == 0:
        assert float(db.abs().sum()) == 0.0 and float(dW.abs().sum()) == 0.0
        return
    tC, tZ, tb, tW, _ = R.fused_truth(Z, b, W, c, G)
    errs = {"C": rel_err(C, tC), "dZ": rel_err(dZ, tZ), "db": rel_err(db, tb), "dW": rel_err(dW, tW)}
    print(f"mlp kernels N={N} k={k} n={n}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    # the weight gradient on its own, and the input / bias gradients on their own, are the same numbers
    only_w = mlp.act_linear_backward(Z, b, W, G, want_z=False)
    only_z = mlp.act_linear_backward(Z, b, W, G, want_w=False)
    assert only_w[0] is None and only_w[1] is None and only_z[2] is None
    assert torch.equal(only_w[2], dW) and torch.equal(only_z[0], dZ) and torch.equal(only_z[1], db)


# The forward serves a group of nt = ceil(ng / 32) tiles of result columns on the next leaf of NT in {1, 2, 4, 8}.  CASES
# runs every leaf, and nt = 3 only in dZ (the second 128-wide group of n = 219).  Here the forward's rounding nt = 3 on
# NT = 4 (n = 65, 96: the fourth tile is all padding), and a full group followed by a group of one column (256 | 257).
# k in {33, 63} and N in {33, 129}: one and two chunks of k, one and two tiles of rows, a tail in each.  Layout of CASES.
ROUNDED_CASES = [
    (33, 33, 65, 0, False, True), (129, 63, 96, 3, True, False), (129, 63, 65, 0, False, False), (33, 33, 96, 1, False, True),
    (129, 33, 256, 0, False, True), (33, 63, 257, 2, True, True), (129, 63, 257, 0, False, False),
]


def _in_nan(rows, cols, values, dev, col0=0, more_cols=0):
    """`values` [rows, cols] as a slice of a buffer with two more rows that is NaN everywhere else."""
    buf = torch.full((rows + 2, col0 + cols + more_cols), float("nan"), device=dev)
    view = buf[:rows, col0:col0 + cols]
    view.copy_(values)
    return view


@pytest.mark.parametrize("N,k,n,ldz_extra,strided,with_c", ROUNDED_CASES)
def test_rounded_up_leaves_against_float64_among_nan(cuda, N, k, n, ldz_extra, strided, with_c):
    """The checks of `test_kernels_against_float64_without_dropout` with every operand surrounded by NaN: Zbuf's columns past
    k and two rows past N, W's rows past n and columns past k, G's surroundings.  No result may hold one."""
    Z, b, W, c, G = _on(cuda, N, k, n, 1000 + N + k + n, ldz_extra)
    Z = _in_nan(N, k, Z, cuda, more_cols=ldz_extra)
    W = _in_nan(n, k, W, cuda, more_cols=3)
    assert (Z.stride(0) == k + ldz_extra or N <= 1) and W.stride(0) == k + 3
    c = c if with_c else None
    out = None
    if strided:
        wide = torch.full((N, n + 9), 7.0, device=cuda)
        out = wide[:, 5:5 + n]
        G = _in_nan(N, n, G, cuda, col0=3, more_cols=4)
    else:
        G = _in_nan(N, n, G, cuda)
    C = mlp.act_linear_forward(Z, b, W, c, out=out)
    dZ, db, dW = mlp.act_linear_backward(Z, b, W, G)
    torch.cuda.synchronize()
    assert C.shape == (N, n) and dZ.shape == (N, k) and db.shape == (k,) and dW.shape == (n, k)
    if strided:
        assert bool((wide[:, :5] == 7.0).all()) and bool((wide[:, 5 + n:] == 7.0).all())   # nothing outside the n columns
    assert all(bool(torch.isfinite(t).all()) for t in (C, dZ, db, dW))
    tC, tZ, tb, tW, _ = R.fused_truth(Z, b, W, c, G)
    errs = {"C": rel_err(C, tC), "dZ": rel_err(dZ, tZ), "db": rel_err(db, tb), "dW": rel_err(dW, tW)}
    print(f"mlp kernels, rounded-up leaves, N={N} k={k} n={n}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    only_w = mlp.act_linear_backward(Z, b, W, G, want_z=False)
    only_z = mlp.act_linear_backward(Z, b, W, G, want_w=False)
    assert torch.equal(only_w[2], dW) and torch.equal(only_z[0], dZ) and torch.equal(only_z[1], db)


_FULL_GROUP = {}


def _full_group(dev):
    """Operands with n = 256 -- eight full tiles on NT = 8, dW on k_mlp_grad_w<2> -- and their C and dW, computed once."""
    if not _FULL_GROUP:
        Z, b, W, c, G = _on(dev, 129, 63, 256, 4242)
        _FULL_GROUP["v"] = (Z, b, W, c, G, mlp.act_linear_forward(Z, b, W, c), mlp.act_linear_backward(Z, b, W, G, want_z=False)[2])
    return _FULL_GROUP["v"]


@pytest.mark.parametrize("n1", [65, 96, 129, 192])
def test_bits_of_a_column_do_not_depend_on_the_leaf_that_serves_it(cuda, n1):
    """By construction, no tolerance.  An element of C is accumulated over k in the same order whichever NT serves its tile
    (`acc[t]` of k_mlp_fwd depends on its own column only, and the output bias is added to the finished sum), so the forward
    on W[:n1], c[:n1] -- NT = 4 with a padding tile, or NT = 8 with up to three -- gives the first n1 columns of the forward
    on all 256.  The row slices of dW are set by N and k alone (`grad_w_split`) and k_mlp_reduce_w adds them in slice order
    under either TW (two slices here), so the rows dW[:n1] are those of the run with G[:, :n1].  A difference means a leaf
    sums in another order or reads its padding."""
    Z, b, W, c, G, C, dW = _full_group(cuda)
    G1 = G[:, :n1]
    assert G1.stride(0) == 256
    assert torch.equal(mlp.act_linear_forward(Z, b, W[:n1], c[:n1]), C[:, :n1])
    assert torch.equal(mlp.act_linear_backward(Z, b, W[:n1], G1, want_z=False)[2], dW[:n1])


def _seed_tensor(value, dev):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def test_mask_is_the_documented_hash_bit_for_bit(cuda):
    N, k, p = 300, 64, 0.5
    gen = torch.Generator().manual_seed(5)
    sign = torch.where(torch.rand(N, k, generator=gen) < 0.5, -1.0, 1.0)
    Z = (sign * (0.2 + 0.8 * torch.rand(N, k, generator=gen))).to(cuda)          # |Z| >= 0.2
    b = ((torch.rand(k, generator=gen) * 2 - 1) * 0.1).to(cuda)                   # |b| <= 0.1: |Z + b| >= 0.1 everywhere
    W = torch.eye(k, device=cuda)
    G = (0.5 + torch.rand(N, k, generator=gen)).to(cuda)                          # non-zero
    patterns = []
    for value in (0x1234567890ABCDE, -77, (1 << 40) + 12345):
        seed = _seed_tensor(value, cuda)
        keep = R.keep_matrix(value, N, k, p)
        C = mlp.act_linear_forward(Z, b, W, None, p, seed)
        assert torch.equal((C != 0).cpu(), keep)
        want = torch.selu(Z.double().cpu() + b.double().cpu()) / (1 - p)
        assert float(((C.double().cpu() - want).abs() / want.abs())[keep].max()) <= 1e-6
        assert torch.equal(mlp.act_linear_forward(Z, b, W, None, p, seed), C)    # the same seed: the same bits
        dZ, db, dW = mlp.act_linear_backward(Z, b, W, G, p, seed)
        assert torch.equal((dZ != 0).cpu(), keep)                                # the backward takes the same decisions
        again = mlp.act_linear_backward(Z, b, W, G, p, seed)
        assert all(torch.equal(x, y) for x, y in zip((dZ, db, dW), again))
        tC, tZ, tb, tW, _ = R.fused_truth(Z, b, W, None, G, keep, p)
        assert max(rel_err(C, tC), rel_err(dZ, tZ), rel_err(db, tb), rel_err(dW, tW)) <= TOL
        # a mask row offset shifts the rows of the mask: row i takes the decision of mask row i + 1000
        shifted = R.keep_matrix(value, N, k, p, row0=1000)
        Cs = mlp.act_linear_forward(Z, b, W, None, p, seed, mask_row0=1000)
        assert torch.equal((Cs != 0).cpu(), shifted) and not torch.equal(shifted, keep)
        dZs, _, dWs = mlp.act_linear_backward(Z, b, W, G, p, seed, mask_row0=1000)
        assert torch.equal((dZs != 0).cpu(), shifted)
        assert rel_err(dWs, R.fused_truth(Z, b, W, None, G, shifted, p)[3]) <= TOL
        Ct = mlp.act_linear_forward(Z[7:], b, W, None, p, seed, mask_row0=7)     # rows 7.. on their own, same decisions
        assert torch.equal(Ct, C[7:])
        patterns.append(keep)
    assert not torch.equal(patterns[0], patterns[1]) and not torch.equal(patterns[1], patterns[2])
    other = mlp.act_linear_forward(Z, b, W, None, p, _seed_tensor(12345, cuda))
    assert not torch.equal(other != 0, C != 0)
    # p = 0 with a seed and p > 0 without one both mean "no mask"
    plain = mlp.act_linear_forward(Z, b, W)
    assert torch.equal(mlp.act_linear_forward(Z, b, W, None, 0.0, seed), plain)
    assert torch.equal(mlp.act_linear_forward(Z, b, W, None, 0.5, None), plain) and bool((plain != 0).all())
    unmasked = mlp.act_linear_backward(Z, b, W, G)
    for other in (mlp.act_linear_backward(Z, b, W, G, 0.0, seed), mlp.act_linear_backward(Z, b, W, G, 0.5, None)):
        assert all(torch.equal(x, y) for x, y in zip(other, unmasked))


@pytest.mark.parametrize("p", [0.3, 0.7])
@pytest.mark.parametrize("N,k,n", GRAD_SHAPES)
def test_training_gradients_with_the_mask_against_float64(cuda, p, N, k, n):
    Z, b, W, c, G = _on(cuda, N, k, n, 77 + N)
    Z, b, W, c = (t.clone().requires_grad_() for t in (Z, b, W, c))
    value = -(N * 1_000_003 + k)
    C = mlp.act_linear(Z, b, W, c, p, _seed_tensor(value, cuda))
    C.backward(G)
    tC, tZ, tb, tW, tc = R.fused_truth(Z, b, W, c, G, R.keep_matrix(value, N, k, p), p)
    errs = {"C": rel_err(C, tC), "dZ": rel_err(Z.grad, tZ), "db": rel_err(b.grad, tb), "dW": rel_err(W.grad, tW),
            "dc": rel_err(c.grad, tc)}
    print(f"mlp kernels with mask p={p} N={N} k={k} n={n}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("N,k,n", MULTI_CHUNK_SHAPES)
def test_masked_gradients_over_several_row_chunks_per_slice(cuda, N, k, n):
    """dW's workgroups walk two 128-row chunks each here (see CASES): the tile of a = s keep selu(Z + b) and its row keys are
    staged again for the second chunk and both chunks add into one partial sum.  Against float64 under the hash's keep
    matrix, with a mask row offset; the weight gradient alone gives the bits of the full call."""
    p, value, row0 = 0.5, (1 << 41) + N, 12345
    Z, b, W, _, G = _on(cuda, N, k, n, 313 + N, 1)
    seed = _seed_tensor(value, cuda)
    dZ, db, dW = mlp.act_linear_backward(Z, b, W, G, p, seed, mask_row0=row0)
    keep = R.keep_matrix(value, N, k, p, row0=row0)
    _, tZ, tb, tW, _ = R.fused_truth(Z, b, W, None, G, keep, p)
    errs = {"dZ": rel_err(dZ, tZ), "db": rel_err(db, tb), "dW": rel_err(dW, tW)}
    print(f"mlp kernels, several chunks per slice, p={p} N={N} k={k} n={n}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert not bool((dZ.cpu() != 0)[~keep].any())                       # a dropped element passes no gradient
    assert all(v <= TOL for v in errs.values()), errs
    only_w = mlp.act_linear_backward(Z, b, W, G, p, seed, mask_row0=row0, want_z=False)
    assert only_w[0] is None and only_w[1] is None and torch.equal(only_w[2], dW)
    assert torch.equal(mlp.act_linear_backward(Z, b, W, G, p, seed, mask_row0=row0)[2], dW)     # the same bits again


def test_python_layer_refuses_what_the_kernels_do_not_take(cuda):
    Z, b, W, c, _ = _on(cuda, 9, 6, 4, 1)
    with pytest.raises(TypeError, match="float32"):
        mlp.act_linear(Z.double(), b, W)
    with pytest.raises(ValueError, match="do not fit"):
        mlp.act_linear(Z, b[:5], W)
    with pytest.raises(ValueError, match="do not fit"):
        mlp.act_linear(Z, b, W, c[:3])
    with pytest.raises(ValueError, match="outside"):
        mlp.act_linear(Z, b, W, c, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp.act_linear(Z, b.cpu(), W)


# ------------------------------------------------------------------------------------------------
# the model against the restatement
# ------------------------------------------------------------------------------------------------
N_DOCS, VOCAB, EXTRA, N_CLASSES = 700, 1500, 12, 7


def _features(kind):
    """The TF-IDF-like sparse COO matrix of csr_to_torch with a second sparse block appended the way append_feats does it
    (torch.cat of two sparse tensors along dim 1: one-hot labels of the level above), or a dense matrix."""
    gen = torch.Generator().manual_seed(21)
    if kind == "dense":
        return torch.randn(N_DOCS, 90, generator=gen) * 0.3
    rows = torch.arange(N_DOCS).repeat_interleave(20)
    cols = torch.randint(0, VOCAB, (N_DOCS * 20,), generator=gen)
    vals = torch.rand(N_DOCS * 20, generator=gen) * 0.4 + 0.05
    tfidf = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (N_DOCS, VOCAB))
    top = torch.randint(0, EXTRA, (N_DOCS,), generator=gen)
    onehot = torch.sparse_coo_tensor(torch.stack([torch.arange(N_DOCS), top]), torch.ones(N_DOCS), (N_DOCS, EXTRA))
    return torch.cat([tfidf, onehot], dim=1)


_TRUTH = {}


def _case(kind, hidden):
    """Features, labels, the float64 reference model and its eval logits / p = 0 training step: computed once per case."""
    key = (kind, tuple(hidden))
    if key not in _TRUTH:
        x = _features(kind)
        y = torch.randint(0, N_CLASSES, (N_DOCS,), generator=torch.Generator().manual_seed(4))
        torch.manual_seed(len(hidden))
        ref = MLPRef(x.size(1), N_CLASSES, hidden, dropout=0.0).double()
        xd = x.double()
        with torch.no_grad():
            logits_eval = ref.eval()(xd)
        logits = ref.train()(xd)
        loss = nn.CrossEntropyLoss()(logits, y)
        ref.zero_grad(set_to_none=True)
        loss.backward()
        grads = {name: q.grad.detach().clone() for name, q in ref.named_parameters()}
        _TRUTH[key] = (x, y, ref, logits_eval, loss.detach(), grads)
    return _TRUTH[key]


def _mine(ref, dev, dropout):
    model = pkg.MLP(ref.layers[0].in_features, ref.layers[-1].out_features, [layer.out_features for layer in ref.layers[:-1]],
                    dropout=dropout)
    model.load_state_dict({name: v.float() for name, v in ref.state_dict().items()}, strict=True)
    return model.to(dev).float()


def _step(model, x, y):
    logits = model(x)
    loss = nn.CrossEntropyLoss()(logits, y)
    model.zero_grad(set_to_none=True)
    loss.backward()
    return logits.detach(), loss.detach(), {name: q.grad.detach().clone() for name, q in model.named_parameters()}


@pytest.mark.parametrize("hidden", [[256, 128], [64], [96, 64, 48]])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_model_matches_the_reference_in_float64(cuda, kind, hidden):
    x, y, ref, want_eval, want_loss, want_grads = _case(kind, hidden)
    xd, yd = x.to(cuda), y.to(cuda)
    mine = _mine(ref, cuda, 0.0)
    for fused in (True, False):
        was = pkg.enable_fused_mlp(fused)
        try:
            assert mine.eval().takes_fused_path(xd) is fused and mine.train().takes_fused_path(xd) is fused
            with torch.no_grad():
                got_eval = mine.eval()(xd)
            _, loss, grads = _step(mine.train(), xd, yd)           # training mode, dropout = 0
        finally:
            pkg.enable_fused_mlp(was)
        errs = {"eval logits": rel_err(got_eval, want_eval), "loss": abs(loss.item() - want_loss.item()) / want_loss.item()}
        errs.update({name: rel_err(grads[name], want_grads[name]) for name in want_grads})
        print(f"MLP parity {kind} hidden={hidden} fused={fused}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
        assert set(grads) == set(want_grads)
        assert all(v <= TOL for v in errs.values()), (fused, errs)
    # a model in eval mode with a dropout rate: the fused path, the same logits
    with torch.no_grad():
        assert torch.equal(_mine(ref, cuda, 0.5).eval()(xd), mine.eval()(xd))


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_fused_training_step_with_dropout_follows_the_hash(cuda, kind):
    """p = 0.5 under enable_fused_dropout: the step's gradients against the float64 restatement driven by the keep
    matrices of the seeds the step drew (torch's generator, re-seeded, hands out the same ones)."""
    hidden, p = [256, 128], 0.5
    x, y, ref, *_ = _case(kind, hidden)
    xd, yd = x.to(cuda), y.to(cuda)
    mine = _mine(ref, cuda, p).train()
    pkg.enable_fused_dropout(True)
    try:
        assert mine.takes_fused_path(xd)
        torch.manual_seed(99)
        seeds = [int(dense.new_seed(cuda).item()) for _ in hidden]
        torch.manual_seed(99)
        logits, loss, grads = _step(mine, xd, yd)
        torch.manual_seed(99)
        assert torch.equal(_step(mine, xd, yd)[0], logits)      # the same seeds: the same bits
    finally:
        pkg.enable_fused_dropout(False)
    params = [(layer.weight.detach().clone().requires_grad_(), layer.bias.detach().clone().requires_grad_())
              for layer in ref.layers]
    keeps = [R.keep_matrix(s, N_DOCS, h, p) for s, h in zip(seeds, hidden)]
    dense_x = (x.to_dense() if x.is_sparse else x).double()
    want = R.mlp_truth(params, dense_x, keeps, p)
    want_loss = nn.CrossEntropyLoss()(want, y)
    want_loss.backward()
    errs = {"logits": rel_err(logits, want), "loss": abs(loss.item() - want_loss.item()) / want_loss.item()}
    for i, (W, b) in enumerate(params):
        errs[f"layers.{i}.weight"] = rel_err(grads[f"layers.{i}.weight"], W.grad)
        errs[f"layers.{i}.bias"] = rel_err(grads[f"layers.{i}.bias"], b.grad)
    print(f"MLP fused dropout step {kind}: " + ", ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs


def test_without_fused_dropout_training_draws_from_torchs_generator(cuda):
    x, y, ref, *_ = _case("sparse", [64])
    xd, yd = x.to(cuda), y.to(cuda)
    mine = _mine(ref, cuda, 0.5).train()
    assert not mine.takes_fused_path(xd)
    losses = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        losses.append(_step(mine, xd, yd)[1].item())
    assert losses[0] == losses[1] and losses[0] != losses[2]
    # rate 1 trains through the composition whatever the switches say: everything is dropped, the logits are the last bias
    pkg.enable_fused_dropout(True)
    try:
        one = _mine(ref, cuda, 1.0).train()
        assert not one.takes_fused_path(xd)
        assert torch.equal(one(xd), one.layers[-1].bias.expand(N_DOCS, -1))
    finally:
        pkg.enable_fused_dropout(False)


def test_thirty_adam_steps_reduce_the_loss_on_both_paths(cuda):
    gen = torch.Generator().manual_seed(0)
    N, F, n_classes = 300, 24, 3
    y = torch.randint(0, n_classes, (N,), generator=gen)
    centres = torch.randn(n_classes, F, generator=gen) * 2.0
    x = (centres[y] + 0.3 * torch.randn(N, F, generator=gen)).to(cuda)            # separable clusters
    y = y.to(cuda)
    pkg.enable_fused_dropout(True)
    try:
        for fused in (True, False):
            torch.manual_seed(1)
            model = pkg.MLP(F, n_classes, [32, 16], dropout=0.2).to(cuda).float().train()
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
            was = pkg.enable_fused_mlp(fused)
            try:
                assert model.takes_fused_path(x) is fused
                curve = []
                for _ in range(30):
                    loss = nn.CrossEntropyLoss()(model(x), y)
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    opt.step()
                    curve.append(loss.item())
            finally:
                pkg.enable_fused_mlp(was)
            print(f"MLP 30 Adam steps fused={fused}: loss {curve[0]:.4f} -> {curve[-1]:.4f}")
            assert curve[-1] < 0.5 * curve[0], curve
    finally:
        pkg.enable_fused_dropout(False)


def test_fused_eval_forward_replays_from_a_graph_with_the_eager_bits(cuda):
    x, _, ref, *_ = _case("sparse", [256, 128])
    xd = x.to(cuda)
    mine = _mine(ref, cuda, 0.5).eval()
    assert mine.takes_fused_path(xd)
    with torch.no_grad():
        eager = mine(xd).clone()                             # (builds the feature plan and the stream's workspaces)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            mine(xd)                                         # the side stream's own workspaces
            with torch.cuda.graph(graph, stream=side):
                out = mine(xd)
        torch.cuda.current_stream().wait_stream(side)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
