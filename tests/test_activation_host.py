"""`GCN(..., apply_activation=True)` and the two C entry points behind it, as far as a host without a GPU can see them:
construction, pickling, which layers are handed the activation, the argument checks of `tgcn_spmm_act` /
`tgcn_act_grad`.  The arithmetic is tested on the GPU (tests/test_gpu_activation.py)."""
import inspect
import io
import pickle

import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, conv, models


def test_apply_activation_is_the_last_keyword_and_off_by_default():
    params = list(inspect.signature(pkg.GCN.__init__).parameters.values())
    assert [p.name for p in params[1:]] == ["in_channels", "out_channels", "n_gcn", "n_hidden_gcn", "activation", "dropout",
                                            "apply_activation"]
    assert params[-1].default is False
    m = pkg.GCN(10, 3)                                   # the reference's positional signature is untouched
    assert m.apply_activation is False and isinstance(m.activation, nn.ReLU)
    m = pkg.GCN(10, 3, 2, 8, nn.ReLU, 0.5, True)
    assert m.apply_activation is True
    assert sorted(m.state_dict()) == sorted(pkg.GCN(10, 3, n_hidden_gcn=8).state_dict())      # no new keys


def test_module_round_trips_through_pickle_and_an_old_pickle_is_the_linear_network():
    m = pkg.GCN(10, 3, n_hidden_gcn=8, apply_activation=True)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert back.apply_activation is True
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), back.state_dict().values()))
    old = pickle.loads(pickle.dumps(m))
    del old.__dict__["apply_activation"]                 # a module pickled before the switch existed
    old = pickle.loads(pickle.dumps(old))
    assert "apply_activation" not in old.__dict__
    assert _activations_handed_to_layers(old) == [None, None]


def _activations_handed_to_layers(model, monkeypatch=None, **fwd):
    """Run GCN.forward with GCNConv.forward replaced by a recorder (no GPU): which layer got which `activation=`."""
    seen = []

    def fake(self, x, edge_index, edge_weight=None, input_dropout=0.0, rows=None, activation=None):
        seen.append(activation)
        return torch.zeros(4, self.out_channels)
    real, conv.GCNConv.forward = conv.GCNConv.forward, fake
    try:
        g = pkg.Data(x=torch.zeros(4, model.layers[0].in_channels), edge_index=torch.zeros(2, 0, dtype=torch.long),
                     edge_attr=None)
        model(g, **fwd)
    finally:
        conv.GCNConv.forward = real
    return seen


def test_activation_goes_between_the_layers_and_never_after_the_last():
    m = pkg.GCN(10, 3, n_gcn=3, n_hidden_gcn=8, apply_activation=True)
    seen = _activations_handed_to_layers(m)
    assert seen[0] is m.activation and seen[1] is m.activation and seen[2] is None
    assert _activations_handed_to_layers(pkg.GCN(10, 3, n_gcn=3, n_hidden_gcn=8)) == [None, None, None]
    t = pkg.GCN(10, 3, n_hidden_gcn=8, activation=nn.Tanh, apply_activation=True)
    assert _activations_handed_to_layers(t) == [t.activation, None]
    assert conv._is_fused_activation(m.activation) and not conv._is_fused_activation(t.activation)

    class MyReLU(nn.ReLU):                               # "exactly nn.ReLU": a subclass may compute anything
        pass
    assert not conv._is_fused_activation(MyReLU()) and not conv._is_fused_activation(None)


def test_linear_collapse_is_not_taken_when_the_activation_is_applied(monkeypatch):
    def boom(self, g, rows=None):
        raise AssertionError("the collapsed forward rests on the linear network")
    monkeypatch.setattr(models.GCN, "_collapsed_forward", boom)
    models.enable_linear_collapse(True)
    try:
        m = pkg.GCN(10, 3, n_hidden_gcn=8, apply_activation=True).eval()
        with torch.no_grad():
            assert _activations_handed_to_layers(m) == [m.activation, None]
            with pytest.raises(AssertionError):          # the linear network still takes it
                _activations_handed_to_layers(pkg.GCN(10, 3, n_hidden_gcn=8).eval())
    finally:
        models.enable_linear_collapse(False)


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.tgcn_abi_version() == 7
    assert (_lib.ACT_NONE, _lib.ACT_RELU) == (0, 1)
    # tgcn_spmm's checks (shared): a NULL plan is refused before anything is enqueued
    assert lib.tgcn_spmm_act(None, 0, None, 8, 8, None, _lib.ACT_RELU, None, 8, None, 0, None) == _lib.E_INVALID
    assert b"NULL" in lib.tgcn_last_error()
    assert lib.tgcn_spmm_act(None, 0, None, 8, 8, None, 7, None, 8, None, 0, None) == _lib.E_INVALID
    assert b"act" in lib.tgcn_last_error() and b"7" in lib.tgcn_last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.E_INVALID)
    assert lib.tgcn_act_grad_workspace_bytes(1000, 200) > 0
    assert lib.tgcn_act_grad_workspace_bytes(1000, 200) == lib.tgcn_colsum_workspace_bytes(1000, 200)
    assert lib.tgcn_act_grad(5, None, 8, None, 8, 0, 8, None, None, 0, None) == _lib.E_INVALID
    assert b"act" in lib.tgcn_last_error()
    assert lib.tgcn_act_grad(_lib.ACT_RELU, None, 8, None, 8, 4, 8, None, None, 0, None) == _lib.E_INVALID    # NULL A / G
    assert lib.tgcn_act_grad(_lib.ACT_RELU, None, 8, None, 8, 4, 0, None, None, 0, None) == _lib.E_INVALID    # F = 0
