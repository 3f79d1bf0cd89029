"""`pytextgcn_amd.JumpingKnowledgeNetwork`, `pytextgcn_amd.jk.JumpingKnowledge` and the `tgcn_jk_*` entry points as far
as a host without a GPU can see them: the public surface against the reference's (textgcn/lib/models.py:55-81), state_dict
exchange, pickling, the argument checks.  The arithmetic is tested on the GPU (tests/test_gpu_jkn.py); here, in float64 on
the CPU, only that the inputs of its leaf tests let the bar see a defect of one hidden unit."""
import ctypes
import inspect
import io
import pickle

import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, jk

import _jkn_ref as R
from _jkn_ref import JKNRef, JKRef


def test_exports_follow_the_reference_import_path():
    import pytextgcn_amd.lib.models as lm
    from pytextgcn_amd.lib.models import JumpingKnowledgeNetwork, GCN, EGCN      # perlevel_amazon.py:14, verbatim
    assert JumpingKnowledgeNetwork is pkg.JumpingKnowledgeNetwork is pkg.models.JumpingKnowledgeNetwork
    assert GCN is pkg.GCN and EGCN is pkg.EGCN
    assert "JumpingKnowledgeNetwork" in pkg.__all__ and "JumpingKnowledgeNetwork" in lm.__all__
    assert pkg.JumpingKnowledge is jk.JumpingKnowledge


def test_constructor_signature_and_defaults_are_the_references():
    params = list(inspect.signature(pkg.JumpingKnowledgeNetwork.__init__).parameters.values())[1:]
    E = inspect.Parameter.empty
    assert tuple((p.name, p.default) for p in params) == (
        ("in_channels", E), ("out_channels", E), ("n_gcn", 2), ("n_hidden_gcn", 64), ("activation", nn.ReLU),
        ("dropout", 0.5))
    m = pkg.JumpingKnowledgeNetwork(10, 3)
    assert isinstance(m.activation, nn.ReLU) and m.dropout == 0.5 and len(m.layers) == 2
    assert m.jk.mode == "lstm" and m.jk.lstm.input_size == 64 and m.jk.lstm.hidden_size == 64
    assert m.jk.lstm.bidirectional and m.jk.lstm.batch_first and m.jk.att.in_features == 128
    m = pkg.JumpingKnowledgeNetwork(10, 3, 3, 8, nn.Tanh, 0.25)             # positional
    assert isinstance(m.activation, nn.Tanh) and m.dropout == 0.25 and len(m.layers) == 3
    assert all(isinstance(layer, pkg.GCNConv) for layer in m.layers) and isinstance(m.lin, nn.Linear)
    # PyG's surface of the aggregation module
    sig = list(inspect.signature(jk.JumpingKnowledge.__init__).parameters.values())[1:4]
    assert tuple((p.name, p.default) for p in sig) == (("mode", E), ("channels", None), ("num_layers", None))
    assert repr(jk.JumpingKnowledge("cat")) == "JumpingKnowledge(cat)"


@pytest.mark.parametrize("n_gcn", [2, 3])
def test_state_dict_keys_and_shapes_equal_the_restatements(n_gcn):
    mine = pkg.JumpingKnowledgeNetwork(10, 3, n_gcn=n_gcn, n_hidden_gcn=5)      # odd L C at n_gcn = 3: H = 7
    ref = JKNRef(10, 3, n_gcn=n_gcn, n_hidden_gcn=5)
    got = sorted((k, tuple(v.shape)) for k, v in mine.state_dict().items())
    want = sorted((k, tuple(v.shape)) for k, v in ref.state_dict().items())
    assert got == want
    H = (n_gcn * 5) // 2
    shapes = dict(got)
    assert shapes["jk.lstm.weight_ih_l0"] == (4 * H, 5) and shapes["jk.lstm.weight_hh_l0_reverse"] == (4 * H, H)
    assert shapes["jk.lstm.bias_ih_l0"] == (4 * H,) and shapes["jk.att.weight"] == (1, 2 * H) and shapes["jk.att.bias"] == (1,)
    assert shapes["lin.weight"] == (3, 5) and shapes[f"layers.{n_gcn - 1}.weight"] == (5, 5)


def test_a_state_dict_of_the_restatement_loads_strictly():
    torch.manual_seed(0)
    ref, mine = JKNRef(10, 3, 3, 8), pkg.JumpingKnowledgeNetwork(10, 3, 3, 8)
    mine.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(ref.state_dict()[k], v) for k, v in mine.state_dict().items())
    ref.load_state_dict(mine.state_dict(), strict=True)
    agg = jk.JumpingKnowledge("lstm", channels=8, num_layers=3)
    agg.load_state_dict(JKRef(8, 3).state_dict(), strict=True)


def test_whole_module_pickle_round_trip():
    m = pkg.JumpingKnowledgeNetwork(10, 3, n_hidden_gcn=8, dropout=0.3)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert isinstance(back, pkg.JumpingKnowledgeNetwork) and back.dropout == 0.3 and back.jk.chunk_rows == m.jk.chunk_rows
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), back.state_dict().values()))
    blob = pickle.dumps(m)
    assert b"ctypes" not in blob and b"CDLL" not in blob


def test_cpu_input_raises_the_no_cpu_fallback_error():
    m = pkg.JumpingKnowledgeNetwork(10, 3, n_hidden_gcn=8).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(pkg.Data(x=torch.eye(10), edge_index=torch.tensor([[0, 1], [1, 0]]), edge_attr=None))
    agg = jk.JumpingKnowledge("lstm", channels=8, num_layers=2)
    for fused in (True, False):
        was = jk.enable_fused_jk(fused)
        try:
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                agg([torch.zeros(4, 8), torch.zeros(4, 8)])
        finally:
            assert jk.enable_fused_jk(was) is fused              # the switch returns the previous setting
    with pytest.raises(TypeError, match="float32"):
        agg.double()([torch.zeros(4, 8, dtype=torch.float64)] * 2)


def test_more_than_eight_layers_raise():
    assert jk.MAX_LAYERS == 8
    with pytest.raises(ValueError, match="at most 8"):
        jk.JumpingKnowledge("lstm", channels=4, num_layers=9)
    with pytest.raises(ValueError, match="at most 8"):
        pkg.JumpingKnowledgeNetwork(10, 3, n_gcn=9, n_hidden_gcn=4)
    jk.JumpingKnowledge("lstm", channels=4, num_layers=8)
    agg = jk.JumpingKnowledge("lstm", channels=4, num_layers=2)
    with pytest.raises(ValueError, match="TGCN_JK_MAX_LAYERS"):
        agg([torch.zeros(2, 4)] * 9)
    with pytest.raises(ValueError):
        jk.JumpingKnowledge("lstm", channels=4, num_layers=2, chunk_rows=0)


def test_cat_and_max_are_the_torch_expressions():
    gen = torch.Generator().manual_seed(1)
    xs = [torch.randn(6, 3, generator=gen) for _ in range(3)]
    assert torch.equal(jk.JumpingKnowledge("cat")(xs), torch.cat(xs, dim=-1))
    assert torch.equal(jk.JumpingKnowledge("max")(xs), torch.stack(xs, dim=-1).max(dim=-1)[0])
    assert not list(jk.JumpingKnowledge("max").parameters())


def _defects(C, H):
    """Three one-unit defects of a fused LSTM kernel, simulated in the parameters: (A) the last hidden unit of the reverse
    direction never reaches the score, (B) the last input column is dropped from the forward direction's input product,
    (C) the last recurrent column is dropped in the reverse direction."""
    return {"A": ("att.weight", (0, 2 * H - 1)), "B": ("lstm.weight_ih_l0", (slice(None), C - 1)),
            "C": ("lstm.weight_hh_l0_reverse", (slice(None), H - 1))}


@pytest.mark.parametrize("C,L,waves", R.LEAF_SHAPES)
def test_the_bar_sees_a_one_unit_defect_on_the_leaf_tests_inputs(C, L, waves):
    """With default initialisation alpha stays within about +-0.05 of 1 / L, so `out` might hide an error of the LSTM.  It
    does not on the inputs of tests/test_gpu_jkn.py's leaf tests: in float64, at N = 33, each defect of `_defects` moves
    `out` and `alpha` by at least 10 x the bar of 1e-5.  A condition on the chosen parameters and inputs (`leaf_seeds`),
    not a tolerance on the kernel: a seed that misses it is changed, the factor is not."""
    N, H, TOL = 33, (L * C) // 2, 1e-5
    assert R.fwd_waves(H) == waves and (H + 31) // 32 <= 8
    module_seed, input_seed = R.leaf_seeds(N, C, L)
    torch.manual_seed(module_seed)
    state = jk.JumpingKnowledge("lstm", channels=C, num_layers=L).state_dict()
    xs, _ = R.jk_values(N, C, L, input_seed)
    out, alpha = R.jk_truth(xs, state, with_alpha=True)
    assert float((alpha.sum(1) - 1).abs().max()) <= 1e-12
    moved = {}
    for tag, (key, where) in _defects(C, H).items():
        broken = {k: v.clone() for k, v in state.items()}
        assert float(broken[key][where].abs().min()) > 0.0
        broken[key][where] = 0.0
        o, a = R.jk_truth(xs, broken, with_alpha=True)
        moved[tag] = (R.rel_err(o, out), R.rel_err(a, alpha))
    print(f"jk defects C={C} L={L} H={H}: " + ", ".join(f"({k}) out {o:.1e} alpha {a:.1e}" for k, (o, a) in moved.items()))
    assert all(o >= 10 * TOL and a >= 10 * TOL for o, a in moved.values()), moved


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.tgcn_abi_version() == 7       # the addition is purely additive
    P = 0x1000                                                          # a non-NULL pointer nobody dereferences

    def arrays(L):
        return (ctypes.c_void_p * max(L, 1))(*[P] * max(L, 1)), (ctypes.c_int64 * max(L, 1))(*[8] * max(L, 1))

    def fwd(L=2, N=4, C=8, H=8, ldwi=8, ldwh=8, aw=P, out=P, ldo=8, alpha=P, lda=2, ld0=None):
        xs, lds = arrays(L)
        if ld0 is not None:
            lds[0] = ld0
        lstm = (ctypes.c_void_p * 8)(*[P] * 8)
        return lib.tgcn_jk_lstm_forward(xs, lds, L, N, C, H, lstm, ldwi, ldwh, aw, P, out, ldo, alpha, lda, 0, None)

    def refused(status, *words):
        msg = lib.tgcn_last_error()
        assert status == _lib.E_INVALID, (status, msg)
        assert all(w in msg for w in words), msg
    refused(fwd(L=9), b"tgcn_jk_lstm_forward", b"TGCN_JK_MAX_LAYERS")
    refused(fwd(L=0), b"TGCN_JK_MAX_LAYERS")
    refused(fwd(N=-1), b"row count")
    refused(fwd(C=0), b"widths")
    refused(fwd(H=257, ldwh=300), b"hidden width 257")
    refused(fwd(ld0=7), b"ldxs[t]")
    refused(fwd(ldwi=7), b"ldwi")
    refused(fwd(ldwh=7), b"ldwh")
    refused(fwd(ldo=7), b"ldo")
    refused(fwd(lda=1), b"lda")
    refused(fwd(aw=None), b"att_w is NULL")
    refused(fwd(out=None), b"out is NULL")
    assert fwd(N=0, out=None, alpha=None) == _lib.OK                    # empty: nothing is enqueued
    assert lib.tgcn_jk_lstm_forward_supported(7) == 1 and lib.tgcn_jk_lstm_forward_supported(200) == 1
    assert lib.tgcn_jk_lstm_forward_supported(256) == 1 and lib.tgcn_jk_lstm_forward_supported(257) == 0
    xs, lds = arrays(9)
    refused(lib.tgcn_jk_attention(xs, lds, 9, 4, 8, 8, P, P, 8, 32, P, P, P, 8, P, 9, 0, None), b"tgcn_jk_attention")
    refused(lib.tgcn_jk_attention_grad(xs, lds, 9, 4, 8, P, 8, None, 0, P, 9, P, 9, None), b"tgcn_jk_attention_grad")
    refused(lib.tgcn_jk_cell(P, 31, None, 0, P, P, None, 0, P, 32, P, 8, P, 8, 4, 8, None), b"ldpx")
    refused(lib.tgcn_jk_cell_grad(P, 32, P, 8, None, 0, None, 0, P, 2, P, P, 8, 1, P, 31, 4, 8, None), b"lddg")
    refused(lib.tgcn_jk_input_grad(P, 7, P, 8, P, 8, None, 0, P, 2, 4, 8, None), b"lddx")
    assert lib.tgcn_jk_cell(None, 32, None, 0, None, None, None, 0, None, 32, None, 8, None, 8, 0, 8, None) == _lib.OK
    with pytest.raises(ValueError):
        _lib.check(fwd(L=9))
