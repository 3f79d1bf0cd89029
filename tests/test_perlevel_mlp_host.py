"""Host tests of the per-level MLP: `perlevel.AppendedFeatures` / `append_classes` against a restatement of the reference's
`append_feats` (mlp_helper.py:141-151), the argument checks of `tgcn_mlp_act_linear_cls*` (pytextgcn_amd/csrc/mlp.hip) and
the parameters of an `MLP` that is used on such features.  No GPU: nothing is enqueued here."""
import ctypes

import pytest
import torch

from _mlp_ref import MLPRef

N, F = 23, 17


def _tfidf(seed=0):
    gen = torch.Generator().manual_seed(seed)
    dense = torch.rand(N, F, generator=gen) * (torch.rand(N, F, generator=gen) < 0.3)
    return dense.to_sparse()


def _one_hot(ids, n_classes):
    """OneHotEncoder's dense rows; an id outside [0, n_classes) gives a row of zeros."""
    out = torch.zeros(len(ids), n_classes)
    ok = (ids >= 0) & (ids < n_classes)
    out[torch.arange(len(ids))[ok], ids[ok]] = 1.0
    return out


def append_feats(feats, top_labels):
    """mlp_helper.py:141-151 restated: the non-zeros of the dense `top_labels` as a sparse block, concatenated to `feats`."""
    indices = torch.nonzero(top_labels).t()
    values = top_labels[indices[0], indices[1]]
    mat = torch.sparse_coo_tensor(indices, values, top_labels.shape)
    return torch.cat([feats, mat], dim=1)


def _same_sparse(a, b):
    a, b = a.coalesce(), b.coalesce()
    return a.shape == b.shape and torch.equal(a.indices(), b.indices()) and torch.equal(a.values(), b.values())


def test_to_sparse_is_append_feats_also_chained_and_with_unknown_ids():
    from pytextgcn_amd.perlevel import AppendedFeatures, append_classes
    x = _tfidf()
    gen = torch.Generator().manual_seed(1)
    y1 = torch.randint(0, 6, (N,), generator=gen)
    y1[3], y1[7] = -1, 6                                     # unknown to the encoder: a row of zeros
    y2 = torch.randint(0, 9, (N,), generator=gen)
    y2[0] = -1
    a1 = append_classes(x, y1, 6)
    assert isinstance(a1, AppendedFeatures) and a1.base is x and a1.blocks == (6,) and a1.ids.dtype == torch.int32
    assert a1.ids[3, 0] == -1 and a1.ids[7, 0] == -1
    want1 = append_feats(x, _one_hot(y1, 6))
    assert _same_sparse(a1.to_sparse(), want1) and a1.to_sparse().is_coalesced()
    assert a1.to_sparse() is a1.to_sparse()                  # built once and kept
    a2 = append_classes(a1, y2.numpy(), 9)                   # chains like the script's call; ids as a numpy array
    assert a2.base is x and a2.blocks == (6, 9) and tuple(a2.ids.shape) == (N, 2)
    assert torch.equal(a2.ids[:, 0], a1.ids[:, 0])
    valid = y2 >= 0
    assert torch.equal(a2.ids[valid, 1].long(), y2[valid] + 6) and a2.ids[0, 1] == -1   # offsets into the stacked columns
    assert _same_sparse(a2.to_sparse(), append_feats(want1, _one_hot(y2, 9)))
    assert torch.equal(a2.to_sparse().to_dense(), torch.cat([x.to_dense(), _one_hot(y1, 6), _one_hot(y2, 9)], dim=1))


def test_shape_and_to():
    from pytextgcn_amd.perlevel import append_classes
    x = _tfidf()
    a = append_classes(append_classes(x, torch.zeros(N, dtype=torch.long), 6), torch.ones(N, dtype=torch.long), 9)
    assert a.shape == (N, F + 15) and a.size() == (N, F + 15) and a.size(0) == N and a.size(1) == F + 15 and a.dim() == 2
    assert a.is_sparse is False and a.is_cuda is False and a.device == x.device and a.dtype == torch.float32
    assert a.n_base == F and a.n_appended == 15
    assert a.to("cpu") is a and a.to(torch.device("cpu")) is a and a.float() is a
    with pytest.raises(ValueError, match="rows"):
        append_classes(x, torch.zeros(N + 1, dtype=torch.long), 3)
    with pytest.raises(ValueError, match="integers"):
        append_classes(x, torch.zeros(N), 3)
    with pytest.raises(TypeError, match="sparse"):
        append_classes(x.to_dense(), torch.zeros(N, dtype=torch.long), 3)


def test_cpu_features_are_refused_not_computed():
    import pytextgcn_amd as pkg
    from pytextgcn_amd import mlp
    from pytextgcn_amd.perlevel import append_classes
    a = append_classes(_tfidf(), torch.zeros(N, dtype=torch.long), 6)
    model = pkg.MLP(F + 6, 3, [8]).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp.act_linear_cls(torch.zeros(3, 8), torch.zeros(8), torch.zeros(4, 8), None, torch.zeros(3, 1, dtype=torch.int32),
                           torch.zeros(6, 8))


@pytest.mark.parametrize("blocks", [(6,), (9, 70)])
def test_state_dict_is_the_references(blocks):
    """Using an MLP on appended features asks nothing of its parameters: they are those of MLP(F + Fh, C, hidden)."""
    from pytextgcn_amd.lib.models import MLP
    Fh = sum(blocks)
    torch.manual_seed(2)
    ref = MLPRef(F + Fh, 5, [256, 128], dropout=0.7)
    mine = MLP(F + Fh, 5, [256, 128], dropout=0.7)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == want
    assert want["layers.0.weight"] == (256, F + Fh)
    mine.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in mine.state_dict().items())


def test_entry_points_refuse_bad_arguments_without_a_device():
    from pytextgcn_amd import _lib
    lib = _lib.load()
    host = ctypes.create_string_buffer(4096)        # an address that is never read: every call returns before it enqueues
    a = ctypes.addressof(host)
    N_, k, n, Fh = 8, 4, 3, 6

    def fwd(Z=a, cls=a, ldcls=2, S=2, T=a, ldt=k, Fh=Fh, b=a, W=a, C=a, p=0.5, ldz=k, N=N_):
        return lib.tgcn_mlp_act_linear_cls(Z, ldz, cls, ldcls, S, T, ldt, Fh, b, W, k, None, C, n, N, k, n, p, None, 0, None)

    bad = (({"S": 0}, b"S must be 1 or 2"), ({"S": 3}, b"S must be 1 or 2"), ({"Fh": 0}, b"Fh must be in [1, 128]"),
           ({"Fh": 129}, b"Fh must be in [1, 128]"), ({"ldcls": 1}, b"ldcls"), ({"ldt": k - 1}, b"ldt"),
           ({"cls": None}, b"cls is NULL"), ({"T": None}, b"T is NULL"))
    for kw, word in bad + (({"Z": None}, b"Z is NULL"), ({"b": None}, b"b is NULL"), ({"W": None}, b"W is NULL"),
                           ({"C": None}, b"C is NULL"), ({"p": 1.0}, b"[0, 1)"), ({"ldz": k - 1}, b"ldz")):
        assert fwd(**kw) == _lib.E_INVALID, kw
        assert word in lib.tgcn_last_error(), (kw, lib.tgcn_last_error())
    assert fwd(N=0, cls=None, T=None, Z=None, C=None) == _lib.OK          # an empty problem's pointers may be NULL
    assert fwd(N=0, S=3) == _lib.E_INVALID                                # ... its sizes are still checked
    with pytest.raises(ValueError):
        _lib.check(fwd(S=3))

    need = lib.tgcn_mlp_act_linear_cls_grad_workspace_bytes(N_, k, n, Fh)
    assert need > lib.tgcn_mlp_act_linear_grad_workspace_bytes(N_, k, n) > 0
    assert lib.tgcn_mlp_act_linear_cls_grad_workspace_bytes(N_, k, n, 0) == 0
    assert lib.tgcn_mlp_act_linear_cls_grad_workspace_bytes(N_, k, n, 129) == 0
    # partial sums only: the workspace does not grow like N x k
    assert (lib.tgcn_mlp_act_linear_cls_grad_workspace_bytes(1 << 22, 256, 128, 79)
            < 4 * lib.tgcn_mlp_act_linear_cls_grad_workspace_bytes(1 << 16, 256, 128, 79))

    def grad(Z=a, cls=a, ldcls=2, S=2, T=a, ldt=k, Fh=Fh, b=a, W=a, G=a, dZ=a, db=a, dT=a, lddt=k, dW=a, p=0.5, ws=a,
             ws_bytes=need):
        return lib.tgcn_mlp_act_linear_cls_grad(Z, k, cls, ldcls, S, T, ldt, Fh, b, W, k, G, n, dZ, k, db, dT, lddt, dW, k,
                                                N_, k, n, p, None, 0, ws, ws_bytes, None)

    for kw, word in bad + (({"dZ": None, "db": None}, b"dT is requested without dZ"), ({"lddt": k - 1}, b"lddt"),
                           ({"G": None}, b"G is NULL"), ({"ws_bytes": need - 1}, b"workspace"), ({"ws": None}, b"workspace"),
                           ({"db": None}, b"both or neither"),
                           ({"dZ": None, "db": None, "dT": None, "dW": None}, b"nothing to compute")):
        assert grad(**kw) == _lib.E_INVALID, kw
        assert word in lib.tgcn_last_error(), (kw, lib.tgcn_last_error())
