"""Host tests of the MLP drop-in (pytextgcn_amd.models.MLP) and of the argument checks of its two entry points
(`tgcn_mlp_act_linear*`, pytextgcn_amd/csrc/mlp.hip).  No GPU: nothing is enqueued here."""
import ctypes

import pytest
import torch

import _mlp_ref as R
from _mlp_ref import MLPRef


def test_mlp_is_importable_from_the_reference_path():
    from pytextgcn_amd.lib.models import EGCN, GCN, MLP, JumpingKnowledgeNetwork
    import pytextgcn_amd as pkg
    assert MLP is pkg.MLP is pkg.models.MLP
    assert all(isinstance(m, type) for m in (GCN, EGCN, JumpingKnowledgeNetwork))


@pytest.mark.parametrize("hidden", [[256, 128], [40], [24, 16, 8]])
def test_state_dict_is_the_references_and_loads_strictly_both_ways(hidden):
    from pytextgcn_amd.lib.models import MLP
    torch.manual_seed(3)
    ref = MLPRef(37, 5, hidden, dropout=0.3)
    mine = MLP(37, 5, hidden, dropout=0.3)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == want
    assert sorted(want) == sorted(f"layers.{i}.{s}" for i in range(len(hidden) + 1) for s in ("weight", "bias"))
    assert want["layers.0.weight"] == (hidden[0], 37) and want[f"layers.{len(hidden)}.weight"] == (5, hidden[-1])
    mine.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in mine.state_dict().items())
    again = MLPRef(37, 5, hidden)
    again.load_state_dict(mine.state_dict(), strict=True)
    # the reference's attributes
    assert isinstance(mine.dropout, torch.nn.Dropout) and mine.dropout.p == 0.3
    assert isinstance(mine.act, torch.nn.SELU) and isinstance(mine.layers, torch.nn.ModuleList)
    assert all(isinstance(layer, torch.nn.Linear) for layer in mine.layers)
    assert MLP(37, 5, hidden).dropout.p == 0.5


def test_default_init_is_torchs_linear_init():
    from pytextgcn_amd.lib.models import MLP
    torch.manual_seed(11)
    ref = MLPRef(19, 4, [12, 6])
    torch.manual_seed(11)
    mine = MLP(19, 4, [12, 6])
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in mine.state_dict().items())


def test_empty_hidden_asserts():
    from pytextgcn_amd.lib.models import MLP
    with pytest.raises(AssertionError):
        MLP(10, 3, [])


def test_cpu_tensors_are_refused_not_computed():
    import pytextgcn_amd as pkg
    from pytextgcn_amd import mlp
    model = pkg.MLP(10, 3, [8]).eval()
    idx = torch.tensor([[0, 1, 2], [1, 5, 9]])
    sparse = torch.sparse_coo_tensor(idx, torch.ones(3), (3, 10))
    for fused in (True, False):
        was = pkg.enable_fused_mlp(fused)
        try:
            for x in (torch.zeros(3, 10), sparse):
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    model(x)
        finally:
            assert pkg.enable_fused_mlp(was) is fused
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp.act_linear(torch.zeros(3, 8), torch.zeros(8), torch.zeros(4, 8))


def test_which_path_runs():
    import pytextgcn_amd as pkg
    x = torch.zeros(2, 10)
    try:
        for p, training, fused_dropout, want in ((0.5, False, False, True), (0.0, True, False, True),
                                                 (0.5, True, False, False), (0.5, True, True, True),
                                                 (1.0, True, True, False), (1.0, False, False, True)):
            pkg.enable_fused_dropout(fused_dropout)
            model = pkg.MLP(10, 3, [8], dropout=p).train(training)
            assert model.takes_fused_path(x) is want, (p, training, fused_dropout)
            was = pkg.enable_fused_mlp(False)
            assert model.takes_fused_path(x) is False
            pkg.enable_fused_mlp(was)
    finally:
        pkg.enable_fused_dropout(False)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from pytextgcn_amd import _lib
    lib = _lib.load()
    host = ctypes.create_string_buffer(4096)        # an address that is never read: every call returns before it enqueues
    a = ctypes.addressof(host)
    N, k, n = 8, 4, 3

    def fwd(Z=a, b=a, W=a, C=a, p=0.5, ldz=k):
        return lib.tgcn_mlp_act_linear(Z, ldz, b, W, k, None, C, n, N, k, n, p, None, 0, None)

    for kw, word in (({"Z": None}, b"Z is NULL"), ({"b": None}, b"b is NULL"), ({"W": None}, b"W is NULL"),
                     ({"C": None}, b"C is NULL"), ({"p": 1.0}, b"[0, 1)"), ({"p": -0.1}, b"[0, 1)"), ({"ldz": k - 1}, b"ldz")):
        assert fwd(**kw) == _lib.E_INVALID, kw
        assert word in lib.tgcn_last_error(), (kw, lib.tgcn_last_error())
    with pytest.raises(ValueError):
        _lib.check(fwd(p=1.0))
    assert lib.tgcn_mlp_act_linear(a, k, a, a, k, None, a, n, N, 0, n, 0.0, None, 0, None) == _lib.E_INVALID     # k = 0
    assert lib.tgcn_mlp_act_linear(a, k, a, a, k, None, a, n, N, k, n, 0.5, None, -1, None) == _lib.E_INVALID    # mask_row0 < 0
    assert b"mask_row0" in lib.tgcn_last_error()

    need = lib.tgcn_mlp_act_linear_grad_workspace_bytes(N, k, n)
    assert need > 0 and lib.tgcn_mlp_act_linear_grad_workspace_bytes(-1, k, n) == 0
    # partial sums only: the workspace does not grow like N x k (here N grows 64-fold, the workspace less than 4-fold)
    assert lib.tgcn_mlp_act_linear_grad_workspace_bytes(1 << 22, 256, 128) < 4 * lib.tgcn_mlp_act_linear_grad_workspace_bytes(1 << 16, 256, 128)

    def grad(Z=a, b=a, W=a, G=a, dZ=a, db=a, dW=a, p=0.5, ws=a, ws_bytes=need, row0=0):
        return lib.tgcn_mlp_act_linear_grad(Z, k, b, W, k, G, n, dZ, k, db, dW, k, N, k, n, p, None, row0, ws, ws_bytes, None)

    for kw, word in (({"Z": None}, b"Z is NULL"), ({"b": None}, b"b is NULL"), ({"W": None}, b"W is NULL"),
                     ({"G": None}, b"G is NULL"), ({"p": 1.0}, b"[0, 1)"), ({"ws_bytes": need - 1}, b"workspace"),
                     ({"ws": None}, b"workspace"), ({"ws_bytes": 0}, b"workspace"), ({"db": None}, b"both or neither"),
                     ({"dZ": None}, b"both or neither"), ({"dZ": None, "db": None, "dW": None}, b"nothing to compute"),
                     ({"row0": -1}, b"mask_row0")):
        assert grad(**kw) == _lib.E_INVALID, kw
        assert word in lib.tgcn_last_error(), (kw, lib.tgcn_last_error())


@pytest.mark.parametrize("hidden", [[16, 8], [12], [10, 9, 7]])
def test_the_float64_restatement_is_the_reference_model(hidden):
    """tests/_mlp_ref.mlp_truth (bias deferred into the next product, as the kernels have it) against MLPRef (Linear,
    SELU, Dropout in the reference's order), both in double precision: logits and every parameter gradient."""
    torch.manual_seed(5)
    ref = MLPRef(23, 4, hidden, dropout=0.5).double().eval()
    x = torch.randn(30, 23, dtype=torch.float64)
    params = [(layer.weight.detach().clone().requires_grad_(), layer.bias.detach().clone().requires_grad_())
              for layer in ref.layers]
    got = R.mlp_truth(params, x)
    want = ref(x)
    assert R.rel_err(got, want) <= 1e-13
    G = torch.randn_like(want)
    want.backward(G)
    got.backward(G)
    for (W, b), layer in zip(params, ref.layers):
        assert R.rel_err(W.grad, layer.weight.grad) <= 1e-12 and R.rel_err(b.grad, layer.bias.grad) <= 1e-12
    # and a sparse input goes the same way
    xs = (x * (torch.rand_like(x) < 0.2)).to_sparse()
    assert R.rel_err(R.mlp_truth(params, xs.to_dense()), ref(xs)) <= 1e-13
