"""Host-side tests of the per-label strategy (pytextgcn_amd/perlabel.py): the float64 restatement the GPU tests hold the
kernel to (tests/_perlabel_ref.py) against the K separate `CrossEntropyLoss('mean')` calls of perlabel_amazon.py:130-137,
`relabel` against sklearn's LabelEncoder (:104-109), and the surface of `PerLabelGCN`.  No GPU."""
import pickle

import numpy as np
import pytest
import torch

import _perlabel_ref as R


@pytest.mark.parametrize("widths", [[1], [3, 4], [64, 65, 1, 7], [257, 2]])
@pytest.mark.parametrize("aligned", [True, False])
def test_restatement_equals_k_separate_cross_entropies(widths, aligned):
    c = R.make_case(257, widths, aligned, seed=11 + len(widths))
    loss, loss_k, d, db = R.grouped_ce(c["logits"], c["target"], c["mask"], c["group"], c["starts"], c["widths"])
    want_k, want_d = R.separate_ce(c["logits"], c["target"], c["mask"], c["group"], c["starts"], c["widths"])
    empty = torch.isnan(want_k)
    assert torch.equal(torch.isnan(loss_k), empty)
    if len(widths) >= 2:
        assert bool(empty[-1]) and not bool(empty[0])       # the case holds an empty group and a non-empty one
    assert torch.allclose(loss_k[~empty], want_k[~empty], rtol=1e-12, atol=1e-13)
    assert abs(float(loss) - float(want_k[~empty].sum())) <= 1e-12 * max(1.0, abs(float(loss)))
    assert torch.allclose(d, want_d, rtol=1e-11, atol=1e-14)
    assert torch.allclose(db, want_d.sum(0), rtol=1e-11, atol=1e-14)
    # zero outside each row's segment, on unselected rows, on rows of group -1 and in pad columns
    inside = torch.zeros_like(d, dtype=torch.bool)
    for k, (s, w) in enumerate(zip(c["starts"], c["widths"])):
        inside[(c["mask"] & (c["group"] == k)).nonzero().flatten(), s:s + w] = True
    assert bool((d[~inside] == 0).all()) and bool((want_d[~inside] == 0).all())
    assert float(d[inside].abs().max()) > 0 or widths == [1]      # (a one-class segment: loss 0, gradient 0)
    if widths == [1]:
        assert float(loss) == 0.0 and float(d.abs().max()) == 0.0


def test_routed_prediction_takes_the_first_maximum_of_the_route_segment():
    c = R.make_case(65, [3, 4], True, seed=5)
    pred = R.routed_pred(c["logits"], c["route"], c["starts"], c["widths"])
    assert bool((pred[c["route"] < 0] == -1).all())
    assert int(pred[0]) in (-1, c["starts"][max(int(c["route"][0]), 0)])          # the all-zero row: the first class
    for r in range(65):
        q = int(c["route"][r])
        if q >= 0:
            s, w = c["starts"][q], c["widths"][q]
            assert s <= int(pred[r]) < s + w
            assert float(c["logits"][r, int(pred[r])]) == float(c["logits"][r, s:s + w].max())
            assert not bool((c["logits"][r, s:int(pred[r])] == c["logits"][r, int(pred[r])]).any())
    mapped = R.routed_pred(c["logits"], c["route"], c["starts"], c["widths"], c["class_map"])
    assert torch.equal(mapped[pred >= 0], c["class_map"][pred[pred >= 0]]) and bool((mapped[pred < 0] == -1).all())


def test_relabel_is_the_per_group_label_encoder():
    from sklearn.preprocessing import LabelEncoder
    from pytextgcn_amd.perlabel import column_class_map, relabel, segment_layout
    rng = np.random.RandomState(3)
    n_vocab, n_docs, K = 40, 300, 4
    top_docs = rng.randint(0, K, n_docs)
    y_docs = top_docs * 20 + rng.choice([0, 3, 4, 9, 17], n_docs) * (top_docs != 2)     # group 2: a single class
    y = np.concatenate([np.zeros(n_vocab, dtype=np.int64), y_docs])
    top = np.concatenate([np.zeros(n_vocab, dtype=np.int64), top_docs])
    select = np.arange(n_vocab + n_docs) >= n_vocab
    group, target, counts, cmap = relabel(torch.from_numpy(y), top, torch.from_numpy(select))
    assert group.dtype == torch.int32 and target.dtype == torch.int64
    assert bool((group[:n_vocab] == -1).all()) and bool((target[:n_vocab] == -1).all())      # `g.y[:] = -1` elsewhere
    assert torch.equal(group[n_vocab:].long(), torch.from_numpy(top_docs).long())
    for k in range(K):                                       # perlabel_amazon.py:104-109, classifier by classifier
        idx = np.nonzero(top_docs == k)[0] + n_vocab
        le = LabelEncoder()
        assert np.array_equal(target[idx].numpy(), le.fit_transform(y[idx]))
        assert cmap[k] == le.classes_.tolist() and counts[k] == len(le.classes_)
    assert counts[2] == 1
    starts, n_cols = segment_layout(counts)
    assert all(s % 4 == 0 for s in starts) and n_cols % 4 == 0
    cm = column_class_map(cmap)
    assert cm.shape == (n_cols,) and int((cm >= 0).sum()) == sum(counts)
    for k in range(K):
        assert cm[starts[k]:starts[k] + counts[k]].tolist() == cmap[k]
    # mapping a local prediction back is `mapping[str(i)][pred[j]]` of eval_perlabel.py:77
    docs = torch.arange(n_vocab, n_vocab + n_docs)
    cols = torch.tensor(starts)[group[docs].long()] + target[docs]
    assert torch.equal(cm[cols], torch.from_numpy(y_docs).long())
    with pytest.raises(ValueError):
        relabel(y, np.where(top == 1, 3, top), select)       # a top-level label without a document


def test_perlabel_gcn_surface_and_state_dict():
    from pytextgcn_amd import PerLabelGCN as top_level
    from pytextgcn_amd.lib.models import PerLabelGCN
    from pytextgcn_amd.conv import GCNConv
    assert top_level is PerLabelGCN
    net = PerLabelGCN(50, [2, 5, 1], n_hidden_gcn=8, dropout=0.3)
    assert list(net.state_dict()) == ["layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias"]
    assert isinstance(net.layers[0], GCNConv) and net.layers[0].weight.shape == (50, 24)
    assert net.layers[1].weight.shape == (8, 16) and net.layers[1].bias.shape == (16,)
    assert net.n_groups == 3 and tuple(net.seg_start) == (0, 4, 12) and tuple(net.seg_width) == (2, 5, 1) and net.n_cols == 16
    assert net.dropout == 0.3 and PerLabelGCN(50, [3]).n_hidden == 64 and PerLabelGCN(50, [3]).dropout == 0.5
    w2 = net.layers[1].weight.detach()
    pad = torch.ones(16, dtype=torch.bool)
    for s, c in zip(net.seg_start, net.seg_width):
        pad[s:s + c] = False
        assert float(w2[:, s:s + c].abs().max()) <= (6.0 / (8 + c)) ** 0.5 and float(w2[:, s:s + c].abs().min()) > 0
    assert float(w2[:, pad].abs().max()) == 0.0 and float(net.layers[1].bias.detach().abs().max()) == 0.0
    assert float(net.layers[0].weight.abs().max()) <= (6.0 / (50 + 8)) ** 0.5       # glorot of GCNConv(50, 8), not (50, 24)
    with pytest.raises(ValueError):
        PerLabelGCN(50, [])
    with pytest.raises(ValueError):
        PerLabelGCN(50, [3, 0])
    with pytest.raises(RuntimeError):                        # no CPU fallback
        net(type("G", (), dict(x=torch.eye(50).to_sparse(), edge_index=torch.zeros(2, 0, dtype=torch.long), edge_attr=None))())


@pytest.mark.parametrize("counts", [[2, 5, 1], [4, 8], [7]])
def test_members_round_trip_is_bit_exact_and_pickles(counts):
    from pytextgcn_amd.models import GCN
    from pytextgcn_amd.perlabel import PerLabelGCN
    torch.manual_seed(7)
    members = [GCN(30, c, n_hidden_gcn=8, dropout=0.25) for c in counts]
    for m in members:
        with torch.no_grad():
            for layer in m.layers:
                layer.bias.uniform_(-1, 1)
    net = PerLabelGCN.from_members(members)
    assert net.class_counts == tuple(counts) and net.n_hidden == 8 and net.in_channels == 30 and net.dropout == 0.25
    back = net.export_members()
    assert len(back) == len(members)
    for a, b in zip(members, back):
        assert isinstance(b, GCN) and list(a.state_dict()) == list(b.state_dict())
        for key, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[key]), key
    # pad columns carry zero weight and bias
    pad = torch.ones(net.n_cols, dtype=torch.bool)
    for s, c in zip(net.seg_start, net.seg_width):
        pad[s:s + c] = False
    assert float(net.layers[1].weight[:, pad].abs().sum()) == 0.0 and float(net.layers[1].bias[pad].abs().sum()) == 0.0
    # members are copies, not views
    with torch.no_grad():
        net.layers[0].weight.add_(1.0)
    assert torch.equal(back[0].layers[0].weight, members[0].layers[0].weight)
    # th.save / th.load of the whole module (perlabel_amazon.py:154), and of a member
    clone = pickle.loads(pickle.dumps(net))
    assert clone.class_counts == net.class_counts
    for key, v in net.state_dict().items():
        assert torch.equal(v, clone.state_dict()[key])
    again = PerLabelGCN.from_members(pickle.loads(pickle.dumps(back)))
    assert torch.equal(again.layers[1].weight, PerLabelGCN.from_members(members).layers[1].weight)
    with pytest.raises(ValueError):
        PerLabelGCN.from_members(members + [GCN(30, 3, n_hidden_gcn=16)])


def test_grouped_ce_rejects_invalid_segments_without_a_gpu():
    """Argument errors are found on the host before anything is enqueued (as tests/test_abi.py checks for the plan calls)."""
    import ctypes
    from pytextgcn_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                  # non-NULL stand-ins: nothing is dereferenced on this path

    def call(starts, widths, n_cols, ld):
        K = len(starts)
        hs, hw = (ctypes.c_int32 * K)(*starts), (ctypes.c_int32 * K)(*widths)
        return lib.tgcn_grouped_ce(one, ld, 8, n_cols, K, hs, hw, one, one, one, None, one, one, one, None, one, None, None, ld,
                                   None, None, None, 0, None)
    assert call([0, 4], [3, 4], 8, 8) == _lib.E_WORKSPACE                        # valid segments: the next check refuses
    for starts, widths, n_cols, ld in [([0, 2], [3, 4], 8, 8),                   # overlapping
                                       ([4, 0], [3, 4], 8, 8),                   # decreasing
                                       ([0, 4], [3, 5], 8, 8),                   # past n_cols
                                       ([0, 4], [3, 0], 8, 8),                   # an empty segment
                                       ([0, 4], [3, 4], 8, 7)]:                  # ld < n_cols
        assert call(starts, widths, n_cols, ld) == _lib.E_INVALID, (starts, widths, n_cols, ld)
        assert b"tgcn_grouped_ce" in lib.tgcn_last_error()
    assert lib.tgcn_grouped_ce_workspace_bytes(1000, 64, 6) > 0 and lib.tgcn_grouped_ce_workspace_bytes(-1, 64, 6) == 0
