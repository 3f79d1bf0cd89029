"""GPU tests of EGCN's fused front end on [I_N | H] features (libtgcn.so `tgcn_embed_xw_h*`, pytextgcn_amd/csrc/embed.hip)
and of the switch `enable_fused_hierarchy_embedding` that routes the model to it.

The kernels are held to the float64 restatement of tests/_egcn_hier_ref.py at the project's bar, max|a - b| / max|b| <=
1e-5 (BASELINE.json; the bar of tests/test_gpu_egcn.py).  An fp32 evaluation of the same expressions on the CPU stays
within 8.5e-7 of float64 on every shape of CASES and MASK_CASES below, with and without a mask (worst per output: C 6.1e-7,
dE 8.5e-7 at (333, 515, 300, 6), db 4.0e-7, dEh 6.2e-7, dW 5.8e-7), so the bar leaves more than ten-fold room.  On
ROUNDED_CASES (the tile counts that are rounded up to a leaf, operands surrounded by NaN) the kernels on an MI355X stay
within C 3.7e-7, dE 7.9e-7, db 3.8e-7, dEh 4.6e-7, dW 5.1e-7, and a column's bits do not depend on the leaf that serves it
(torch.equal, no tolerance).  The mask is held to tests/_dropout_hash.py bit for bit, the model
to the reference's EGCN restated from torch's Linear / selu / dropout and the CPU oracle's GCNConv (tests/_egcn_ref.py)."""
import ctypes
import math

import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, embed, synth
from pytextgcn_amd.plan import _stream_ptr

import _egcn_hier_ref as R
from _egcn_hier_ref import rel_err
from _egcn_ref import EGCNRef
from test_gpu_egcn import _compare, _graph, _in_nan, _seed_tensor, _step, _to

pytestmark = pytest.mark.gpu
TOL = 1e-5
CAP = 128            # tgcn_embed_xw_h_max_features(), asserted below


def h_rows(rows, Fh, kind, gen):
    """[rows, Fh] with entries in [0, 1]: one-hot rows (training, perlevel_amazon.py:110) or softmax rows (test time, :156)."""
    if kind == "onehot":
        H = torch.zeros(rows, Fh)
        H[torch.arange(rows), torch.randint(0, Fh, (rows,), generator=gen)] = 1.0
        return H
    return torch.softmax(2.0 * torch.randn(rows, Fh, generator=gen), dim=1)


def operands(N, K, n, Fh, h_row0, kind, seed):
    """Scaled as `_operands` of tests/test_gpu_egcn.py: the Linear's weight [K, N + Fh] and bias ~ U(+-1/sqrt(N)), W glorot,
    G standard normal (CPU tensors)."""
    gen = torch.Generator().manual_seed(seed)
    a = 1.0 / math.sqrt(max(N, 1))
    weight = (torch.rand(K, N + Fh, generator=gen) * 2 - 1) * a
    b = (torch.rand(K, generator=gen) * 2 - 1) * a
    W = (torch.rand(K, n, generator=gen) * 2 - 1) * math.sqrt(6.0 / (K + n))
    G = torch.randn(N, n, generator=gen)
    return weight, b, W, G, h_rows(N - h_row0, Fh, kind, gen)


# (N, K, n, Fh, h_row0, rows of H, strided).  Every N of {0, 31, 333, 1025}, K of {1, 63, 515}, n of {1, 64, 100, 219, 300}
# (each leaf NT in {1, 2, 4, 7, 8} of the column dispatch at its own tile count -- 1, 2, 4, 7 and, in the first group of
# 300, 8 tiles; 300 crosses the 256-column group), Fh of {1, 6, 33, 70, 128} plus 16 | 17, the two sides of the
# registers / reload split of the H operand, and h_row0 of {0, 77 (inside a tile), 128, N} appears; N + Fh is odd nearly
# everywhere (rows of the weight that are not 16-byte aligned).  The tile counts that are ROUNDED UP to a leaf are
# ROUNDED_CASES' below.
CASES = [
    (0, 63, 1, 6, 0, "onehot", False), (31, 1, 1, 1, 0, "onehot", False), (31, 63, 64, 6, 31, "softmax", False),
    (333, 63, 64, 6, 77, "onehot", False), (333, 515, 100, 33, 128, "softmax", False),
    (333, 63, 219, 70, 0, "softmax", False), (333, 515, 300, 6, 77, "onehot", True),
    (1025, 515, 100, 6, 128, "onehot", False), (1025, 63, 64, CAP, 77, "softmax", False),
    (1025, 1, 219, 33, 0, "onehot", False), (1025, 515, 1, 70, 1025, "softmax", False),
    (1025, 63, 300, CAP, 128, "onehot", False), (333, 1, 100, 1, 77, "softmax", False),
    (1025, 515, 64, 16, 700, "softmax", False), (333, 63, 100, 17, 0, "softmax", False),
]
MASK_CASES = [(333, 515, 100, 6, 77, "onehot"), (1025, 63, 219, 33, 128, "softmax"), (1025, 515, 64, 70, 0, "softmax")]
# The roundings of the column dispatch (forward and dE; the list and its reasons are those of ROUNDED_CASES in
# tests/test_gpu_egcn.py): nt = 3 tiles on NT = 4 (n = 65, 96), nt = 5 and 6 on NT = 7 (129, 160, 192), seven full tiles
# (224), the k_embed_h_grad_w<1 | 2> boundary (128 | 129), a full group and a group of one column (256 | 257), three
# groups (513).  K in {33, 63}, N in {33, 129}, Fh in {6, 17} (either side of the registers / reload split), h_row0 in
# {0, 77}.
ROUNDED_CASES = [
    (33, 33, 65, 6, 0, "onehot", False), (129, 63, 96, 17, 77, "softmax", True), (129, 63, 65, 17, 0, "onehot", False),
    (129, 33, 129, 6, 77, "onehot", False), (33, 63, 160, 17, 0, "softmax", True), (129, 63, 192, 6, 0, "softmax", False),
    (33, 33, 128, 17, 0, "onehot", False), (129, 33, 224, 6, 77, "softmax", False), (33, 63, 256, 6, 0, "onehot", False),
    (129, 63, 257, 17, 77, "onehot", True), (33, 33, 513, 6, 0, "softmax", False), (129, 63, 513, 17, 77, "softmax", True),
]


def _errors(got, want, N):
    (C, dWt, db, dW), (tC, tWt, tb, tW) = got, want
    return {"C": rel_err(C, tC), "dE": rel_err(dWt[:, :N], tWt[:, :N]), "db": rel_err(db, tb),
            "dEh": rel_err(dWt[:, N:], tWt[:, N:]), "dW": rel_err(dW, tW)}


@pytest.mark.parametrize("N,K,n,Fh,h_row0,kind,strided", CASES)
def test_kernels_against_float64_without_dropout(cuda, N, K, n, Fh, h_row0, kind, strided):
    assert embed.max_hierarchy_features() == CAP
    weight, b, W, G, Hd = operands(N, K, n, Fh, h_row0, kind, 2000 + N + K + n + Fh)
    wd, bd, Wd, Gd, Hdd = (t.to(cuda) for t in (weight, b, W, G, Hd))
    out = None
    if strided:                                              # H, the result and its gradient with rows wider than they need
        wide = torch.full((N, n + 9), 7.0, device=cuda)
        out = wide[:, 4:4 + n]
        Gw = torch.zeros(N, n + 6, device=cuda)
        Gw[:, 2:2 + n] = Gd
        Gd = Gw[:, 2:2 + n]
        Hw = torch.full((N - h_row0, Fh + 5), 3.0, device=cuda)
        Hw[:, 1:1 + Fh] = Hdd
        Hdd = Hw[:, 1:1 + Fh]
    C = embed.embed_xw_forward(wd, bd, Wd, out=out, h=Hdd, h_row0=h_row0)
    dWt, db, dW = embed.embed_xw_backward(wd, bd, Wd, Gd, h=Hdd, h_row0=h_row0)
    torch.cuda.synchronize()
    assert C.shape == (N, n) and dWt.shape == (K, N + Fh) and db.shape == (K,) and dW.shape == (K, n)
    if strided:
        assert bool((wide[:, :4] == 7.0).all()) and bool((wide[:, 4 + n:] == 7.0).all())   # nothing outside the n columns
    if N == 0:
        assert float(db.abs().sum()) == 0.0 and float(dW.abs().sum()) == 0.0 and float(dWt.abs().sum()) == 0.0
        return
    errs = _errors((C, dWt, db, dW), R.truth(weight, b, Hd, h_row0, W, G), N)
    print(f"embed_h kernels N={N} K={K} n={n} Fh={Fh} h_row0={h_row0} {kind}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    if h_row0 == N:
        assert float(dWt[:, N:].abs().sum()) == 0.0          # nobody has an H row: exact zeros
        errs.pop("dEh")
    assert all(v <= TOL for v in errs.values()), errs
    # the weight gradient on its own, and the other three on their own, are the same numbers
    only_w = embed.embed_xw_backward(wd, bd, Wd, Gd, want_e=False, h=Hdd, h_row0=h_row0)
    only_e = embed.embed_xw_backward(wd, bd, Wd, Gd, want_w=False, h=Hdd, h_row0=h_row0)
    assert only_w[0] is None and only_e[2] is None
    assert torch.equal(only_w[2], dW) and torch.equal(only_e[0], dWt) and torch.equal(only_e[1], db)


@pytest.mark.parametrize("N,K,n,Fh,h_row0,kind,strided", ROUNDED_CASES)
def test_rounded_up_leaves_against_float64_among_nan(cuda, N, K, n, Fh, h_row0, kind, strided):
    """The checks of `test_kernels_against_float64_without_dropout` with the operands surrounded by NaN: two rows past the
    weight's K, past W's K, past G's N and past H's rows, W's columns past n; `strided` also gives the weight rows longer
    than N + Fh and makes H, G and the result column slices of wider buffers.  No result may hold a NaN."""
    weight, b, W, G, Hd = operands(N, K, n, Fh, h_row0, kind, 2000 + N + K + n + Fh)
    wd = _in_nan(K, N + Fh, weight, cuda, more_cols=3 if strided else 0)
    Wd = _in_nan(K, n, W, cuda, more_cols=3)
    bd = b.to(cuda)
    out = None
    if strided:
        wide = torch.full((N, n + 9), 7.0, device=cuda)
        out = wide[:, 4:4 + n]
        Gd = _in_nan(N, n, G, cuda, col0=2, more_cols=4)
        Hdd = _in_nan(N - h_row0, Fh, Hd, cuda, col0=1, more_cols=4)
        assert wd.stride(0) == N + Fh + 3 and Hdd.stride(0) == Fh + 5
    else:
        Gd, Hdd = _in_nan(N, n, G, cuda), _in_nan(N - h_row0, Fh, Hd, cuda)
    C = embed.embed_xw_forward(wd, bd, Wd, out=out, h=Hdd, h_row0=h_row0)
    dWt, db, dW = embed.embed_xw_backward(wd, bd, Wd, Gd, h=Hdd, h_row0=h_row0)
    torch.cuda.synchronize()
    assert C.shape == (N, n) and dWt.shape == (K, N + Fh) and db.shape == (K,) and dW.shape == (K, n)
    if strided:
        assert bool((wide[:, :4] == 7.0).all()) and bool((wide[:, 4 + n:] == 7.0).all())   # nothing outside the n columns
    assert all(bool(torch.isfinite(t).all()) for t in (C, dWt, db, dW))
    errs = _errors((C, dWt, db, dW), R.truth(weight, b, Hd, h_row0, W, G), N)
    print(f"embed_h kernels, rounded-up leaves, N={N} K={K} n={n} Fh={Fh} h_row0={h_row0} {kind}: "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    only_w = embed.embed_xw_backward(wd, bd, Wd, Gd, want_e=False, h=Hdd, h_row0=h_row0)
    only_e = embed.embed_xw_backward(wd, bd, Wd, Gd, want_w=False, h=Hdd, h_row0=h_row0)
    assert torch.equal(only_w[2], dW) and torch.equal(only_e[0], dWt) and torch.equal(only_e[1], db)


_FULL_GROUP = {}


def _full_group(dev):
    """Operands with n = 256 columns -- eight full tiles on NT = 8, dW on k_embed_h_grad_w<2> -- and their C and dW, once."""
    if not _FULL_GROUP:
        N, K, Fh, h_row0 = 129, 63, 17, 77
        t = tuple(x.to(dev) for x in operands(N, K, 256, Fh, h_row0, "softmax", 4242))
        weight, b, W, G, Hd = t
        _FULL_GROUP["v"] = t + (h_row0, embed.embed_xw_forward(weight, b, W, h=Hd, h_row0=h_row0),
                                embed.embed_xw_backward(weight, b, W, G, want_e=False, h=Hd, h_row0=h_row0)[2])
    return _FULL_GROUP["v"]


@pytest.mark.parametrize("n1", [65, 96, 129, 192])
def test_bits_of_a_column_do_not_depend_on_the_leaf_that_serves_it(cuda, n1):
    """By construction, no tolerance (the test of the same name in tests/test_gpu_egcn.py has the reasoning; `acc[t]` of
    k_embed_h_fwd depends on its own column only, the H term enters the activation before any tile is touched, and
    k_embed_h_grad_w's slices are those of `grad_w_split`): C on W[:, :n1] is C[:, :n1] on all 256 columns, dW with
    G[:, :n1] is dW[:, :n1]."""
    weight, b, W, G, Hd, h_row0, C, dW = _full_group(cuda)
    W1, G1 = W[:, :n1], G[:, :n1]
    assert W1.stride(0) == 256 and G1.stride(0) == 256
    assert torch.equal(embed.embed_xw_forward(weight, b, W1, h=Hd, h_row0=h_row0), C[:, :n1])
    assert torch.equal(embed.embed_xw_backward(weight, b, W1, G1, want_e=False, h=Hd, h_row0=h_row0)[2], dW[:, :n1])


@pytest.mark.parametrize("p", [0.3, 0.7])
@pytest.mark.parametrize("N,K,n,Fh,h_row0,kind", MASK_CASES)
def test_training_gradients_with_the_mask_against_float64(cuda, p, N, K, n, Fh, h_row0, kind):
    weight, b, W, G, Hd = operands(N, K, n, Fh, h_row0, kind, 77 + N + Fh)
    wd, bd, Wd = (t.to(cuda).requires_grad_() for t in (weight, b, W))
    value = -(N * 1_000_003 + K)
    C = embed.embed_xw(wd, bd, Wd, p, _seed_tensor(value, cuda), h=Hd.to(cuda), h_row0=h_row0)
    C.backward(G.to(cuda))
    want = R.truth(weight, b, Hd, h_row0, W, G, R.keep_matrix(value, N, K, p), p)
    errs = _errors((C, wd.grad, bd.grad, Wd.grad), want, N)
    print(f"embed_h kernels with mask p={p} N={N} K={K} n={n} Fh={Fh}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs


def _away_from_zero(N, K, Fh, h_row0, dev):
    """Operands whose pre-activation keeps |z| >= 0.05 (|E| >= 0.2, |b| <= 0.1, |t| <= 0.05), W = I and G > 0: an element of
    C or of dE is zero exactly where the mask drops it."""
    gen = torch.Generator().manual_seed(5)
    sign = torch.where(torch.rand(K, N, generator=gen) < 0.5, -1.0, 1.0)
    E = sign * (0.2 + 0.8 * torch.rand(K, N, generator=gen))
    Eh = (torch.rand(K, Fh, generator=gen) * 2 - 1) * 0.05
    weight = torch.cat([E, Eh], 1).contiguous()
    b = (torch.rand(K, generator=gen) * 2 - 1) * 0.1
    Hd = h_rows(N - h_row0, Fh, "softmax", gen)              # rows sum to 1: |t| <= max|Eh|
    G = 0.5 + torch.rand(N, K, generator=gen)
    return tuple(t.to(dev) for t in (weight, b, torch.eye(K), G, Hd))


def _raw_forward(weight, b, W, Hd, h_row0, p, seed, mask_row0):
    lib = _lib.load()
    K, n = W.shape
    Fh = Hd.size(1)
    N = weight.size(1) - Fh
    C = torch.empty(N, n, device=weight.device)
    _lib.check(lib.tgcn_embed_xw_h(weight.data_ptr(), N + Fh, b.data_ptr(), weight.data_ptr() + 4 * N, N + Fh, Hd.data_ptr(), Fh,
                                   h_row0, Fh, W.data_ptr(), n, C.data_ptr(), n, N, K, n, p, seed.data_ptr(), mask_row0,
                                   _stream_ptr(weight.device)))
    return C


def test_mask_is_the_documented_hash_bit_for_bit(cuda):
    N, K, Fh, h_row0, p = 300, 64, 6, 77, 0.5
    weight, b, W, G, Hd = _away_from_zero(N, K, Fh, h_row0, cuda)
    for value in (0x1234567890ABCDE, -77):
        seed = _seed_tensor(value, cuda)
        keep = R.keep_matrix(value, N, K, p)
        C = embed.embed_xw_forward(weight, b, W, p, seed, h=Hd, h_row0=h_row0)
        assert torch.equal((C != 0).cpu(), keep)
        assert torch.equal(embed.embed_xw_forward(weight, b, W, p, seed, h=Hd, h_row0=h_row0), C)
        dWt, db, dW = embed.embed_xw_backward(weight, b, W, G, p, seed, h=Hd, h_row0=h_row0)
        assert torch.equal((dWt[:, :N] != 0).cpu(), keep.t())                    # the backward takes the same decisions
        errs = _errors((C, dWt, db, dW), R.truth(weight, b, Hd, h_row0, W, G, keep, p), N)
        assert all(v <= TOL for v in errs.values()), errs
    # the mask row offset: node i is mask row i + mask_row0, also past 2^32
    row0 = 2**32 + 5
    C = _raw_forward(weight, b, W, Hd, h_row0, p, seed, row0)
    assert torch.equal((C != 0).cpu(), R.keep_matrix(value, N, K, p, row0))
    assert not torch.equal((C != 0).cpu(), keep)
    assert torch.equal(_raw_forward(weight, b, W, Hd, h_row0, p, seed, 0) != 0, keep.to(cuda))


@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("N,K,n,Fh", [(333, 63, 100, 6), (1025, 515, 300, 33)])
def test_without_an_h_term_the_bits_are_those_of_the_identity_kernels(cuda, p, N, K, n, Fh):
    """h_row0 == N (nobody has an H row) and an all-zero Hd (t = +0, and x + 0 is x): C, dE, db and dW are bit for bit what
    tgcn_embed_xw / tgcn_embed_xw_grad give on the first N columns of the same buffer (lde = N + Fh), and dEh is zero."""
    weight, b, W, G, _ = operands(N, K, n, Fh, N, "onehot", 5 + N)
    wd, bd, Wd, Gd = (t.to(cuda) for t in (weight, b, W, G))
    seed = _seed_tensor(991, cuda) if p else None
    E = wd[:, :N]
    assert E.stride(0) == N + Fh
    C0 = embed.embed_xw_forward(E, bd, Wd, p, seed)
    dE0, db0, dW0 = embed.embed_xw_backward(E, bd, Wd, Gd, p, seed)
    for h_row0 in (N, 77):
        Hd = torch.zeros(N - h_row0, Fh, device=cuda)
        C = embed.embed_xw_forward(wd, bd, Wd, p, seed, h=Hd, h_row0=h_row0)
        dWt, db, dW = embed.embed_xw_backward(wd, bd, Wd, Gd, p, seed, h=Hd, h_row0=h_row0)
        assert torch.equal(C, C0) and torch.equal(dWt[:, :N], dE0) and torch.equal(db, db0) and torch.equal(dW, dW0)
        assert float(dWt[:, N:].abs().sum()) == 0.0


def test_two_runs_of_the_backward_give_the_same_bits_and_a_side_stream_works(cuda):
    N, K, n, Fh, h_row0, p = 1025, 515, 100, 33, 128, 0.5
    weight, b, W, G, Hd = (t.to(cuda) for t in operands(N, K, n, Fh, h_row0, "softmax", 3))
    seed = _seed_tensor(11, cuda)
    C = embed.embed_xw_forward(weight, b, W, p, seed, h=Hd, h_row0=h_row0)
    first = embed.embed_xw_backward(weight, b, W, G, p, seed, h=Hd, h_row0=h_row0)
    again = embed.embed_xw_backward(weight, b, W, G, p, seed, h=Hd, h_row0=h_row0)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Cs = embed.embed_xw_forward(weight, b, W, p, seed, h=Hd, h_row0=h_row0)
        on_side = embed.embed_xw_backward(weight, b, W, G, p, seed, h=Hd, h_row0=h_row0)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(Cs, C) and all(torch.equal(x, y) for x, y in zip(first, on_side))


# ------------------------------------------------------------------------------------------------
# the model against the restatement
# ------------------------------------------------------------------------------------------------
def with_hierarchy(N, Fh, kind, seed, extra=None):
    """Sparse [I_N | H]: H on the last third of the rows (the documents) only.  `extra`: one more (row, column, value)."""
    gen = torch.Generator().manual_seed(seed)
    docs = torch.arange(N - N // 3, N)
    H = torch.zeros(N, Fh)
    H[docs] = h_rows(docs.numel(), Fh, kind, gen)
    hi = H.nonzero().t()
    ar = torch.arange(N)
    idx = torch.cat([torch.stack([ar, ar]), torch.stack([hi[0], hi[1] + N])], 1)
    val = torch.cat([torch.ones(N), H[hi[0], hi[1]]])
    if extra is not None:
        idx = torch.cat([idx, torch.tensor([[extra[0]], [extra[1]]])], 1)
        val = torch.cat([val, torch.tensor([extra[2]])])
    return torch.sparse_coo_tensor(idx, val, (N, N + Fh)).coalesce()


def _pair(x, n_classes, n_gcn, cuda, K=48, hdim=20):
    torch.manual_seed(n_gcn)
    ref = EGCNRef(x.size(1), n_classes, embedding_dim=K, n_gcn=n_gcn, n_hidden_gcn=hdim, dropout=0.0)
    mine = pkg.EGCN(x.size(1), n_classes, embedding_dim=K, n_gcn=n_gcn, n_hidden_gcn=hdim, dropout=0.0)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(cuda).float()


@pytest.mark.parametrize("n_gcn", [2, 3])
@pytest.mark.parametrize("kind", ["onehot", "softmax"])
@pytest.mark.parametrize("name", ["tiny_textgcn", "random53"])
def test_model_matches_the_restatement(cuda, name, kind, n_gcn):
    g, n_classes = _graph(name)
    N, Fh = g.x.size(0), 5
    x = with_hierarchy(N, Fh, kind, 17)
    ref, mine = _pair(x, n_classes, n_gcn, cuda)
    gc, gd = _to(g, "cpu", x), _to(g, cuda, x)
    want_train = _step(ref.train(), gc)
    with torch.no_grad():
        want_eval = ref.eval()(gc)
    assert pkg.models._FUSED_HIERARCHY is False                # off by default
    for fused in (True, False):
        was = pkg.enable_fused_hierarchy_embedding(fused)
        try:
            assert was is False
            assert mine.train().takes_fused_path(gd.x) is fused
            got = _step(mine, gd)
            with torch.no_grad():
                got_eval = mine.eval()(gd)
        finally:
            assert pkg.enable_fused_hierarchy_embedding(was) is fused
        assert got[2]["layers.0.weight"].shape == (48, N + Fh)
        _compare(f"[I|H] {name} {kind} n_gcn={n_gcn} fused={fused}", got, want_train)
        assert rel_err(got_eval, want_eval) <= TOL


def test_what_the_kernels_do_not_take_goes_to_the_composition(cuda):
    g, n_classes = _graph("random53")
    N = g.x.size(0)
    was = pkg.enable_fused_hierarchy_embedding(True)
    try:
        too_wide = with_hierarchy(N, CAP + 1, "onehot", 3)
        in_identity = with_hierarchy(N, 5, "onehot", 3, extra=(N - 1, 0, 0.5))
        dense = with_hierarchy(N, 5, "onehot", 3).to_dense()
        for tag, x in (("Fh above the cap", too_wide), ("entry in the identity part", in_identity), ("dense", dense)):
            ref, mine = _pair(x, n_classes, 2, cuda, K=40, hdim=12)
            gd = _to(g, cuda, x)
            assert not mine.train().takes_fused_path(gd.x), tag
            _compare(tag, _step(mine, gd), _step(ref.train(), _to(g, "cpu", x)))
        ok = _to(g, cuda, with_hierarchy(N, CAP, "onehot", 3))
        assert _pair(ok.x, n_classes, 2, cuda)[1].takes_fused_path(ok.x)
        assert pkg.enable_fused_embedding(False) is True     # the master switch still switches every fused front end off
        try:
            assert not _pair(ok.x, n_classes, 2, cuda)[1].takes_fused_path(ok.x)
        finally:
            pkg.enable_fused_embedding(True)
    finally:
        pkg.enable_fused_hierarchy_embedding(was)


def test_fused_path_holds_one_n_by_k_matrix_and_the_composition_more_than_two_and_a_half(cuda):
    """A condition, not a measurement (the protocol and the bounds of the test of the same name in tests/test_gpu_egcn.py):
    extra peak memory of one training forward + backward in units of N K 4 bytes.  With the switch on the step holds the
    weight's gradient -- one matrix [K, N + Fh] -- and nothing else of that size; the composition holds it plus at least the
    pre-activation and the dropped activation."""
    N, K, h, Fh, n_classes = 20000, 2000, 100, 6, 6
    g0 = synth.word_doc_graph(N, 200000, seed=44, n_classes=n_classes)
    g = _to(g0, cuda, with_hierarchy(N, Fh, "onehot", 1))
    torch.manual_seed(0)
    model = pkg.EGCN(N + Fh, n_classes, embedding_dim=K, n_hidden_gcn=h, dropout=0.5).to(cuda).float().train()
    unit = N * K * 4
    pkg.enable_fused_dropout(True)
    extra = {}
    try:
        for fused in (True, False):
            was = pkg.enable_fused_hierarchy_embedding(fused)
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
                pkg.enable_fused_hierarchy_embedding(was)
    finally:
        pkg.enable_fused_dropout(False)
    print(f"EGCN [I|H] extra peak memory of a training step in units of N K 4 B: fused {extra[True]:.3f}, "
          f"composition {extra[False]:.3f}")
    assert extra[True] < 1.5, extra
    assert extra[False] > 2.5, extra


def test_eval_forward_replays_from_a_graph_with_the_eager_bits(cuda):
    g, n_classes = _graph("random53")
    x = with_hierarchy(g.x.size(0), 5, "softmax", 17)
    _, mine = _pair(x, n_classes, 2, cuda)
    mine.eval()
    gd = _to(g, cuda, x)
    was = pkg.enable_fused_hierarchy_embedding(True)
    try:
        assert mine.takes_fused_path(gd.x)
        with torch.no_grad():
            eager = mine(gd).clone()                         # (builds the plan, the dense rows of H and the workspaces)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                mine(gd)                                     # the side stream's own workspaces
                with torch.cuda.graph(graph, stream=side):
                    out = mine(gd)
            torch.cuda.current_stream().wait_stream(side)
            for _ in range(2):
                out.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager)
    finally:
        pkg.enable_fused_hierarchy_embedding(was)
