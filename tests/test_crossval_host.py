"""CPU tests of the cross-validation sweep cell (pytextgcn_amd/crossval.py, csrc/crossval.hip): the row bits, the float64
reference of tests/_crossval_ref.py against torch's own `CrossEntropyLoss('mean')` member by member, the bridge to K
ordinary `GCN`s, and every argument error of `tgcn_member_ce` / `tgcn_adam_members`, which the library returns before
anything is enqueued -- so on a host without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _crossval_ref as R
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits, member_bits


def _kfold(n, k):
    """the (train, validation) index pairs `KFold(k).split(range(n))` yields (contiguous folds, the first n % k one longer)"""
    sizes = np.full(k, n // k)
    sizes[:n % k] += 1
    idx, at, out = np.arange(n), 0, []
    for s in sizes:
        out.append((np.concatenate([idx[:at], idx[at + s:]]), idx[at:at + s]))
        at += s
    return out


@pytest.mark.parametrize("pairs", [True, False])
def test_fold_bits_every_document_in_one_validation_fold_and_k_minus_one_training_folds(pairs):
    n_vocab, n_docs, k, L = 11, 23, 3, 2
    rows = n_vocab + np.arange(n_docs)
    folds = _kfold(n_docs, k)
    train, val = fold_bits(rows, folds if pairs else [f[1] for f in folds], n_vocab + n_docs, n_repeats=L)
    assert train.dtype == val.dtype == torch.int64 and train.shape == val.shape == (n_vocab + n_docs,)
    assert bool((train[:n_vocab] == 0).all()) and bool((val[:n_vocab] == 0).all())          # word rows
    pop = lambda b: sum(((b >> j) & 1) for j in range(64))
    assert bool((pop(val[n_vocab:]) == L).all()) and bool((pop(train[n_vocab:]) == L * (k - 1)).all())
    assert bool((train & val == 0).all()) and bool(((train | val)[n_vocab:] == (1 << (k * L)) - 1).all())
    for rep in range(L):
        for f, (tr, va) in enumerate(folds):
            m = rep * k + f
            assert torch.equal(torch.nonzero(R.selected(val, m)).flatten(), torch.from_numpy(rows[va]))
            assert torch.equal(torch.nonzero(R.selected(train, m)).flatten(), torch.from_numpy(rows[tr]))
    with pytest.raises(ValueError):
        fold_bits(rows, [f[1] for f in folds], n_vocab + n_docs, n_repeats=22)                # 66 members


def test_member_bits_including_bit_63():
    gen = torch.Generator().manual_seed(1)
    masks = [torch.rand(50, generator=gen) < 0.4 for _ in range(64)]
    bits = member_bits(masks)
    assert bits.dtype == torch.int64
    for k, m in enumerate(masks):
        assert torch.equal(R.selected(bits, k), m)
    assert torch.equal(member_bits(masks[:1]), masks[0].long())
    with pytest.raises(ValueError):
        member_bits(masks + masks[:1])
    with pytest.raises(ValueError):
        member_bits([masks[0].long()])


@pytest.mark.parametrize("n,K,C,S", [(63, 3, 5, 8), (257, 12, 17, 20), (65, 1, 1, 1), (40, 64, 2, 4)])
def test_reference_is_k_separate_cross_entropy_losses(n, K, C, S):
    c = R.make_case(n, K, C, S)
    loss, loss_k, d, db, pred = R.reference(n, K, C, S)
    want_k, want_d = R.separate_ce(c["logits"], c["target"], c["bits"], K, C, S)
    empty = torch.isnan(want_k)
    assert torch.equal(torch.isnan(loss_k), empty)
    if K >= 2:
        assert bool(empty[c["empty"]])
    assert R.rel_err(loss_k[~empty], want_k[~empty]) <= 1e-12
    assert abs(float(loss) - float(want_k[~empty].sum())) <= 1e-12 * max(1.0, abs(float(loss)))
    assert R.rel_err(d, want_d) <= 1e-12 and R.rel_err(db, want_d.sum(0)) <= 1e-12
    pad = torch.ones(K * S, dtype=torch.bool)
    for k in range(K):
        pad[k * S:k * S + C] = False
    assert bool((d[:, pad] == 0).all())
    assert pred.shape == (n, K) and pred.dtype == torch.int32 and bool(((pred >= 0) & (pred < C)).all())
    if K >= 2:
        assert R.counts_of(c["bits"], K)[c["empty"]] == 0
    free = torch.nonzero(c["bits"] == 0).flatten()
    if n >= 63:                                                         # the all -inf row: arg-max 0
        assert bool(torch.isneginf(c["logits"][free[0], :C]).all()) and int(pred[free[0], 0]) == 0


def test_from_members_and_export_members_round_trip_bit_exact():
    torch.manual_seed(5)
    members = [pkg.GCN(30, 5, n_hidden_gcn=8, dropout=0.25) for _ in range(6)]
    with torch.no_grad():
        for m in members:
            for layer in m.layers:
                layer.bias.uniform_(-0.5, 0.5)
    net = CrossValGCN.from_members(members)
    assert isinstance(net, pkg.PerLabelGCN) and net.n_members == 6 and net.seg_stride == 8 and net.n_cols == 48
    assert net.layers[0].weight.shape == (30, 48) and net.dropout == 0.25
    pad = torch.ones(48, dtype=torch.bool)
    for k in range(6):
        pad[k * 8:k * 8 + 5] = False
    assert bool((net.layers[1].weight[:, pad] == 0).all()) and bool((net.layers[1].bias[pad] == 0).all())
    out = net.export_members()
    assert len(out) == 6
    for a, b in zip(members, out):
        assert type(b) is pkg.GCN
        for (na, ta), (nb, tb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert na == nb and torch.equal(ta, tb) and ta.data_ptr() != tb.data_ptr()       # copies
    again = CrossValGCN.from_members(out)
    for ta, tb in zip(net.state_dict().values(), again.state_dict().values()):
        assert torch.equal(ta, tb)
    with pytest.raises(ValueError):
        CrossValGCN.from_members(members + [pkg.GCN(30, 4, n_hidden_gcn=8)])
    from pytextgcn_amd.lib.models import CrossValGCN as exported
    assert exported is CrossValGCN


def test_member_adam_refuses_the_update_fused_into_the_backward():
    net = CrossValGCN(30, 5, 6, n_hidden_gcn=8)
    opt = MemberAdam(net, [0.1, 0.05, 0.01, 0.001, 0.1, 0.05])
    with pytest.raises(NotImplementedError, match="tgcn_spmm_adam"):
        opt.fuse_into_backward(net.layers[0].weight)
    assert MemberAdam(net, 0.01).defaults["lr"] == (0.01,) * 6
    with pytest.raises(ValueError):
        MemberAdam(net, [0.1, 0.05])
    with pytest.raises(TypeError):
        MemberAdam(pkg.GCN(30, 5), 0.1)


def test_member_ce_argument_errors_do_not_need_a_gpu():
    lib = _lib.load()
    p = 4096                                    # any non-NULL address: nothing is read before the arguments are refused

    def call(K=3, C=5, S=8, ld=24, ldd=24, dl=p, db=p, ws=p, ws_bytes=1 << 30, n=10):
        return lib.tgcn_member_ce(p, ld, n, K, C, S, p, p, p, p, p, dl, ldd, db, None, ws, ws_bytes, None)

    for kw, word in ((dict(K=0), b"n_members"), (dict(K=65), b"n_members"), (dict(C=0), b"n_classes"),
                     (dict(S=4), b"seg_stride"), (dict(ld=23), b"ld="), (dict(ldd=23), b"ldd="),
                     (dict(dl=None, db=p), b"dbias")):
        assert call(**kw) == _lib.E_INVALID, kw
        assert word in lib.tgcn_last_error(), (kw, lib.tgcn_last_error())
    with pytest.raises(ValueError):
        _lib.check(call(K=0))
    need = lib.tgcn_member_ce_workspace_bytes(10, 3, 5)
    assert need == 4 * R.mce_cap(3) * 3 * (5 + 1)
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE and b"workspace" in lib.tgcn_last_error()
    assert call(ws=None) == _lib.E_WORKSPACE
    assert call(n=-1) == _lib.E_INVALID
    assert lib.tgcn_member_ce_workspace_bytes(10, 0, 5) == 0 and lib.tgcn_member_ce_workspace_bytes(10, 65, 5) == 0


def test_adam_members_argument_errors_do_not_need_a_gpu():
    lib = _lib.load()
    p = 4096
    lr = (ctypes.c_double * 64)(*([0.01] * 64))

    def host(n_rows=7, n_cols=24, width=8, K=3, lrs=lr):
        return lib.tgcn_adam_members(p, p, p, p, None, n_rows, n_cols, width, K, lrs, 0.9, 0.999, 1e-8, 0.0, 1, None)

    def capt(n_rows=7, n_cols=24, width=8, K=3, lrs=lr, step=p, scal=p):
        return lib.tgcn_adam_members_capturable(p, p, p, p, None, n_rows, n_cols, width, K, lrs, 0.9, 0.999, 1e-8, 0.0, step,
                                                scal, None)

    for f in (host, capt):
        for kw in (dict(n_cols=25), dict(K=0, n_cols=0), dict(K=65, n_cols=65 * 8), dict(lrs=None), dict(n_rows=-1),
                   dict(n_cols=-24, width=-8)):
            assert f(**kw) == _lib.E_INVALID, (f.__name__, kw)
            assert b"tgcn_adam_members" in lib.tgcn_last_error()
    assert capt(step=None) == _lib.E_INVALID and capt(scal=None) == _lib.E_INVALID
    # sizes of zero are no-ops of the host form (nothing is enqueued, NULL buffers are fine)
    assert lib.tgcn_adam_members(None, None, None, None, None, 0, 24, 8, 3, lr, 0.9, 0.999, 1e-8, 0.0, 1, None) == _lib.OK
    assert lib.tgcn_adam_members(None, None, None, None, None, 7, 0, 0, 3, lr, 0.9, 0.999, 1e-8, 0.0, 1, None) == _lib.OK
