"""`pytextgcn_amd.EGCN` and the C entry points of its fused front end (`tgcn_embed_xw*`), as far as a host without a GPU
can see them: the public surface against the reference's (textgcn/lib/models.py:28-52), the order of layers and dropout,
pickling, state_dict exchange, the argument checks.  The arithmetic is tested on the GPU (tests/test_gpu_egcn.py)."""
import inspect
import io
import pickle

import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, conv, models

from _egcn_ref import EGCNRef


def test_constructor_signature_and_defaults_are_the_references():
    params = list(inspect.signature(pkg.EGCN.__init__).parameters.values())[1:]
    got = tuple((p.name, p.default) for p in params)
    E = inspect.Parameter.empty
    assert got == (("in_channels", E), ("out_channels", E), ("embedding_dim", 2000), ("n_gcn", 2), ("n_hidden_gcn", 64),
                   ("activation", nn.ReLU), ("dropout", 0.5))
    m = pkg.EGCN(10, 3)
    assert isinstance(m.activation, nn.ReLU) and m.dropout == 0.5
    m = pkg.EGCN(10, 3, 16, 3, 8, nn.Tanh, 0.25)             # positional, as flat_amazon.py:79 could
    assert isinstance(m.activation, nn.Tanh) and m.dropout == 0.25 and len(m.layers) == 4


def test_exports_follow_the_reference_import_path():
    import pytextgcn_amd.lib.models as lm
    from pytextgcn_amd.lib.models import GCN, EGCN      # perlevel_amazon.py:14, minus JumpingKnowledgeNetwork
    assert EGCN is pkg.EGCN and GCN is pkg.GCN and lm.EGCN is models.EGCN
    assert "EGCN" in pkg.__all__ and "EGCN" in lm.__all__


@pytest.mark.parametrize("n_gcn", [2, 3])
def test_layers_and_state_dict_keys(n_gcn):
    m = pkg.EGCN(10, 3, embedding_dim=16, n_gcn=n_gcn, n_hidden_gcn=8)
    assert isinstance(m.layers, nn.ModuleList) and isinstance(m.layers[0], nn.Linear)
    assert all(isinstance(layer, pkg.GCNConv) for layer in m.layers[1:]) and len(m.layers) == n_gcn + 1
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {"layers.0.weight": (16, 10), "layers.0.bias": (16,), "layers.1.weight": (16, 8), "layers.1.bias": (8,)}
    for i in range(2, n_gcn):
        want.update({f"layers.{i}.weight": (8, 8), f"layers.{i}.bias": (8,)})
    want.update({f"layers.{n_gcn}.weight": (8, 3), f"layers.{n_gcn}.bias": (3,)})
    assert shapes == want
    assert shapes == {k: tuple(v.shape) for k, v in EGCNRef(10, 3, 16, n_gcn, 8).state_dict().items()}


def test_embedding_init_is_torchs_linear_init():
    torch.manual_seed(3)
    a = pkg.EGCN(40, 3, embedding_dim=16, n_hidden_gcn=8).layers[0]
    torch.manual_seed(3)
    b = nn.Linear(40, 16)
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)


def test_state_dict_exchange_with_the_restatement():
    torch.manual_seed(0)
    ref, mine = EGCNRef(10, 3, 16, 3, 8), pkg.EGCN(10, 3, 16, 3, 8)
    mine.load_state_dict(ref.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), mine.state_dict().values()))
    ref.load_state_dict(mine.state_dict())


def test_whole_module_pickle_round_trip():
    m = pkg.EGCN(10, 3, embedding_dim=16, n_hidden_gcn=8, dropout=0.3)
    m.layers[1]._reuse_cache = ("a key", object())          # a cache entry must stay behind, as for GCN
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert isinstance(back, pkg.EGCN) and back.dropout == 0.3 and isinstance(back.layers[0], nn.Linear)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), back.state_dict().values()))
    assert not hasattr(back.layers[1], "_reuse_cache")
    blob = pickle.dumps(m)
    assert b"ctypes" not in blob and b"CDLL" not in blob


def _events(model, monkeypatch, x):
    """Run EGCN.forward with every layer and the dropout replaced by recorders (no GPU): the order of the calls."""
    seen = []

    def fake_embed(self, x):
        seen.append("embedding")
        return torch.zeros(4, self.out_features)

    def fake_conv(self, x, edge_index, edge_weight=None, **kw):
        seen.append("conv")
        return torch.zeros(4, self.out_channels)

    def fake_dropout(x, p=0.5, training=True, inplace=False):
        seen.append(("dropout", p, training))
        return x

    def fake_selu(x):
        seen.append("selu")
        return x
    monkeypatch.setattr(models.EmbeddingLinear, "forward", fake_embed)
    monkeypatch.setattr(conv.GCNConv, "forward", fake_conv)
    monkeypatch.setattr(torch.nn.functional, "dropout", fake_dropout)
    monkeypatch.setattr(torch, "selu", fake_selu)
    model(pkg.Data(x=x, edge_index=torch.zeros(2, 0, dtype=torch.long), edge_attr=None))
    return seen


@pytest.mark.parametrize("n_gcn", [2, 3])
def test_dropout_follows_the_embedding_and_every_layer_including_the_last(monkeypatch, n_gcn):
    m = pkg.EGCN(10, 3, embedding_dim=16, n_gcn=n_gcn, n_hidden_gcn=8, dropout=0.4).train()
    d = ("dropout", 0.4, True)
    assert _events(m, monkeypatch, torch.zeros(4, 10)) == ["embedding", "selu", d] + ["conv", d] * n_gcn
    m.eval()
    assert _events(m, monkeypatch, torch.zeros(4, 10)) == ["embedding", "selu"] + ["conv"] * n_gcn      # no dropout at all


def _identity(n):
    ar = torch.arange(n)
    return torch.sparse_coo_tensor(torch.stack([ar, ar]), torch.ones(n), (n, n))


def test_which_features_take_the_fused_path():
    m = pkg.EGCN(10, 3, embedding_dim=16, n_hidden_gcn=8, dropout=0.5)
    eye = _identity(10)
    other = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.ones(2), (10, 10))
    m.eval()
    assert m.takes_fused_path(eye) and not m.takes_fused_path(other) and not m.takes_fused_path(torch.eye(10))
    m.train()
    assert not m.takes_fused_path(eye)                      # torch's random stream unless asked otherwise
    pkg.enable_fused_dropout(True)
    try:
        assert m.takes_fused_path(eye)
        assert pkg.enable_fused_embedding(False) is True    # the switch for A/B runs; returns the previous setting
        assert not m.takes_fused_path(eye)
        m.eval()
        assert not m.takes_fused_path(eye)
    finally:
        pkg.enable_fused_embedding(True)
        pkg.enable_fused_dropout(False)
    m.train()
    m.dropout = 0.0
    assert m.takes_fused_path(eye)                          # nothing random: the default in training as well


@pytest.mark.parametrize("fused", [True, False])
def test_cpu_features_raise_the_no_cpu_fallback_error(fused):
    m = pkg.EGCN(10, 3, embedding_dim=16, n_hidden_gcn=8).eval()
    ei = torch.tensor([[0, 1], [1, 0]])
    was = pkg.enable_fused_embedding(fused)
    try:
        for x in (_identity(10), torch.eye(10)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                m(pkg.Data(x=x, edge_index=ei, edge_attr=None))
    finally:
        pkg.enable_fused_embedding(was)


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.tgcn_abi_version() == 7       # the addition is purely additive
    P = 0x1000                                                          # a non-NULL pointer nobody dereferences

    def fwd(E=P, lde=8, b=P, W=P, ldw=4, C=P, ldc=4, N=8, K=6, n=4, p=0.0, seed=None, row0=0):
        return lib.tgcn_embed_xw(E, lde, b, W, ldw, C, ldc, N, K, n, p, seed, row0, None)

    def bwd(E=P, lde=8, b=P, W=P, ldw=4, G=P, ldg=4, dE=P, ldde=8, db=P, dW=P, lddw=4, N=8, K=6, n=4, p=0.0, seed=None,
            row0=0, ws=P, ws_bytes=1 << 30):
        return lib.tgcn_embed_xw_grad(E, lde, b, W, ldw, G, ldg, dE, ldde, db, dW, lddw, N, K, n, p, seed, row0, ws,
                                      ws_bytes, None)

    def refused(status, *words):
        msg = lib.tgcn_last_error()
        assert status == _lib.E_INVALID, (status, msg)
        assert all(w in msg for w in words), msg
    for call, name in ((fwd, b"tgcn_embed_xw"), (bwd, b"tgcn_embed_xw_grad")):
        for arg in ("E", "b", "W"):
            refused(call(**{arg: None}), name, arg.encode() + b" is NULL")
        refused(call(K=0), name, b"K")
        refused(call(K=-3), name, b"K")
        refused(call(n=0), name, b"n >= 1")
        refused(call(N=-1), name, b"N >= 0")
        for p in (-0.1, 1.0, 1.5, float("nan")):
            refused(call(p=p, seed=P), name, b"p must be in [0, 1)")
        refused(call(lde=7), name, b"lde")
        refused(call(ldw=3), name, b"ldw")
        refused(call(row0=-1), name, b"mask_row0")
    refused(fwd(C=None), b"C is NULL")
    refused(fwd(ldc=3), b"ldc")
    refused(bwd(G=None), b"G is NULL")
    refused(bwd(ldg=3), b"ldg")
    refused(bwd(ldde=7), b"ldde")
    refused(bwd(lddw=3), b"lddw")
    refused(bwd(db=None), b"dE and db")
    refused(bwd(dE=None, db=None, dW=None), b"nothing to compute")
    with pytest.raises(ValueError):
        _lib.check(fwd(K=0))
    need = lib.tgcn_embed_xw_grad_workspace_bytes(20000, 2000, 100)
    assert 0 < need < 20000 * 2000 * 4 // 8                  # partial sums of dW: far from an N x K matrix
    assert lib.tgcn_embed_xw_grad_workspace_bytes(0, 5, 3) > 0
    assert lib.tgcn_embed_xw_grad_workspace_bytes(100, 0, 3) == 0
    assert fwd(N=0, E=None, C=None) == _lib.OK               # an empty product: nothing is enqueued


def test_embed_module_rejects_cpu_tensors_and_bad_rates():
    from pytextgcn_amd import embed
    E, b, W = torch.zeros(6, 8), torch.zeros(6), torch.zeros(6, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        embed.embed_xw(E, b, W)
