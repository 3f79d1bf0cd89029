"""GPU tests of the device-side scores (csrc/metrics.hip, pytextgcn_amd/metrics.py).  The count kernels run through the C
ABI on poisoned, padded buffers: counts equal numpy's exactly (tests/_metrics_cases.py), scores lie within 1e-12 of
sklearn's on the same predictions.  Then the network level: `score()` of the three K-member networks and
`FlatLoop.epoch_scored` against host scoring of the predictions the existing methods return, and `Scoreboard.record` +
`score()` under HIP-graph replay against the eager run, bit for bit."""
import os

import numpy as np
import pytest
import torch

import _metrics_cases as MC
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, conv, metrics, synth
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits
from pytextgcn_amd.perlabel import GroupedRows, PerLabelGCN, PerLabelMLP, relabel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON, PAD = 0x5A5A5A5A, 64


def _padded(shape, dtype, dev, fill=POISON):
    """(view of `shape`, whole buffer): PAD poisoned elements on either side of the view."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    return whole[PAD:PAD + n].view(*shape), whole


def _pads_intact(whole, fill=POISON):
    return bool((whole[:PAD] == fill).all()) and bool((whole[-PAD:] == fill).all())


def raw_counts(dev, key):
    """One call of the case's count kernel through the C ABI: ([counts per set] as numpy, buffers to check)."""
    lib = _lib.load()
    ops = MC.operands(key)
    c = ops["case"]
    n, K, C = c["n"], c["K"], c["C"]
    dev_of = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)            # (a copy: the case is read-only)
    target = dev_of(ops["target"])
    sets = [dev_of(s.view(np.int64) if s.dtype == np.uint64 else s) for s in ops["sets"]]
    outs = [_padded((K, 3, C), torch.int32, dev) for _ in sets]
    need = lib.tgcn_class_counts_workspace_bytes(n, K, C)
    ws, ws_whole = _padded((max(need, 1),), torch.uint8, dev, fill=0xA5)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    second = (ptr(sets[1]) if n else 1) if len(sets) == 2 else None            # (n = 0: any non-NULL pointer says "two sets")
    if c["form"] == "members":
        pred = dev_of(ops["pred"])
        st = lib.tgcn_class_counts_members(ptr(pred), c["ldp"], ptr(target), ptr(sets[0]), second, n, K, C,
                                           outs[0][0].data_ptr(), outs[1][0].data_ptr() if len(sets) == 2 else None,
                                           ws.data_ptr(), need, stream)
    else:
        pred, group, off = dev_of(ops["pred"]), dev_of(ops["group"]), dev_of(ops["offset"])
        st = lib.tgcn_class_counts_groups(ptr(pred), ptr(off), ptr(target), ptr(group), ptr(sets[0]), second, n, K, C,
                                          outs[0][0].data_ptr(), outs[1][0].data_ptr() if len(sets) == 2 else None,
                                          ws.data_ptr(), need, stream)
    assert st == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    assert all(_pads_intact(whole) for _, whole in outs) and _pads_intact(ws_whole, 0xA5), key
    return [o.cpu().numpy() for o, _ in outs], [o for o, _ in outs]


def raw_scores(dev, counts_dev):
    lib = _lib.load()
    K, _, C = counts_dev.shape
    out, whole = _padded((K, 4), torch.float64, dev, fill=-7.0)
    assert lib.tgcn_class_scores(counts_dev.data_ptr(), K, C, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == _lib.OK
    torch.cuda.synchronize()
    assert _pads_intact(whole, -7.0)
    return out.cpu().numpy()


@pytest.mark.parametrize("key", list(MC.CASES))
def test_counts_equal_numpy_exactly_and_scores_equal_sklearn(cuda, key):
    ops = MC.operands(key)
    c = ops["case"]
    got, got_dev = raw_counts(cuda, key)
    again, _ = raw_counts(cuda, key)
    for s, want in enumerate(ops["expected"]):
        assert np.array_equal(got[s], want), (key, s, np.argwhere(got[s] != want)[:5])
        assert np.array_equal(got[s], again[s])                                 # two calls: identical bits
        sc = raw_scores(cuda, got_dev[s])
        assert MC.close(sc, MC.scores_np(want)), (key, s)
        members = sorted(set(list(range(c["K"]))[:3] + list(range(c["K"]))[-2:]))
        for k in members:
            t, p = MC.selected_rows(ops, s, k)
            assert sc[k, 2] == t.size
            if t.size == 0:                     # a member with no row: NaN scores, zero counts
                assert np.isnan(sc[k, 0]) and np.isnan(sc[k, 1]) and sc[k, 3] == 0 and not got[s][k].any()
            elif not c["oob_pred"] and c["C"] <= 256:
                acc, f1 = MC.sklearn_scores(t, p)
                assert MC.close(sc[k, 0], acc) and MC.close(sc[k, 1], f1), (key, s, k, sc[k], acc, f1)


def test_hand_counted_predictions_outside_the_classes(cuda):
    h = MC.HAND
    pred, target = torch.from_numpy(h["pred"]).to(cuda), torch.from_numpy(h["target"]).to(cuda)
    counts = metrics.grouped_class_counts(pred, target, torch.ones(5, dtype=torch.bool, device=cuda), 3)
    assert np.array_equal(counts.cpu().numpy(), h["counts"])
    sc = metrics.scores(counts)
    assert MC.close(torch.stack(list(sc), 1).cpu().numpy(), h["scores"])
    # the members form on the same rows, as member 1 of 2 (member 0 selects nothing)
    pred2 = torch.stack([torch.zeros_like(pred), pred], 1).to(torch.int32)
    bits = torch.full((5,), 2, dtype=torch.int64, device=cuda)
    counts2 = metrics.member_class_counts(pred2, target, bits, 3)
    assert np.array_equal(counts2[1:].cpu().numpy(), h["counts"]) and not bool(counts2[0].any())


def test_python_layer_checks_the_targets_of_selected_rows_before_the_launch(cuda):
    pred = torch.zeros(6, 2, dtype=torch.int32, device=cuda)
    target = torch.tensor([0, 1, 2, 7, 1, -3], device=cuda)
    ok = torch.tensor([1, 3, 2, 0, 1, 0], device=cuda)                          # rows 3 and 5 (bad targets): selected by nobody
    assert metrics.member_class_counts(pred, target, ok, 3).shape == (2, 3, 3)
    with pytest.raises(IndexError):
        metrics.member_class_counts(pred, target, ok, 3, also=torch.tensor([0, 0, 0, 2, 0, 0], device=cuda))
    high = torch.tensor([1, 3, 2, 4, 1, 8], device=cuda)                        # bits at or above K select nothing
    assert metrics.member_class_counts(pred, target, high, 3).shape == (2, 3, 3)
    mask = torch.tensor([1, 1, 1, 0, 1, 0], dtype=torch.bool, device=cuda)
    flat = pred[:, 0].long()
    a, b = metrics.grouped_class_counts(flat, target, mask, 3, also=mask.clone())
    assert torch.equal(a, b) and int(a[0, 2].sum()) == 4
    with pytest.raises(IndexError):
        metrics.grouped_class_counts(flat, target, ~mask, 3)
    with pytest.raises(ValueError):
        metrics.grouped_class_counts(flat, target, mask, 3, n_groups=2)


# ----------------------------------------------------------------------------------------------------------------------
# the networks
# ----------------------------------------------------------------------------------------------------------------------
def _host_scores(y, pred, sel):
    """(accuracy, macro-F1) of the rows `sel` on the host (NaN, NaN without a row)."""
    if not sel.any():
        return np.nan, np.nan
    return MC.sklearn_scores(y[sel], pred[sel])


def _check_scores(got: metrics.Scores, y, preds, sels):
    acc, f1, n_rows = (t.cpu().numpy() for t in (got.accuracy, got.f1_macro, got.n_rows))
    for k, (pred, sel) in enumerate(zip(preds, sels)):
        want = _host_scores(y, pred, sel)
        assert n_rows[k] == sel.sum() and MC.close(acc[k], want[0]) and MC.close(f1[k], want[1]), (k, acc[k], f1[k], want)


def _tiny(cuda):
    z = np.load(os.path.join(GOLD, "tiny_textgcn.npz"))
    N = int(z["y"].shape[0])
    ar = torch.arange(N)
    g = pkg.Data(x=torch.sparse_coo_tensor(torch.stack([ar, ar]), torch.ones(N), (N, N)),
                 edge_index=torch.from_numpy(z["edge_index"]), edge_attr=torch.from_numpy(z["edge_attr"]),
                 y=torch.from_numpy(z["y"]), train_mask=torch.from_numpy(z["train_mask"])).to(cuda)
    return g, N, z["y"].astype(np.int64)


def _crossval_on_tiny(cuda, K=4, C=3, graph="tiny_textgcn"):
    """K members of 3 classes on the 8 nodes of tests/golden/tiny_textgcn.npz (every node carries a label: all are rows
    of the two folds), or on the documents of a 400-node synthetic graph."""
    if graph == "tiny_textgcn":
        g, N, y = _tiny(cuda)
        docs = np.nonzero((y >= 0) & (y < C))[0]
    else:
        N = 400
        gh = synth.word_doc_graph(N, 3000, seed=7, n_classes=C)
        g, y, docs = pkg.Data(**{k: getattr(gh, k) for k in gh.keys}).to(cuda), gh.y.numpy().astype(np.int64), np.arange(gh.n_vocab, N)
    folds = [docs[f::2] for f in range(2)]
    doc_index = [np.nonzero(np.isin(docs, f))[0] for f in folds]
    train_bits, val_bits = fold_bits(docs, doc_index, N, n_repeats=K // 2)
    torch.manual_seed(5)
    net = CrossValGCN(N, C, K, n_hidden_gcn=8, dropout=0.5).to(cuda).float()
    target = torch.from_numpy(y).to(cuda)
    return g, y, net, target, train_bits.to(cuda), val_bits.to(cuda)


@pytest.mark.parametrize("graph", ["tiny_textgcn", "synth400"])
def test_crossval_score_equals_host_scoring_of_evaluate(cuda, graph):
    g, y, net, target, train_bits, val_bits = _crossval_on_tiny(cuda, graph=graph)
    K = net.n_members
    opt = MemberAdam(net, [0.05] * K)
    for _ in range(3):                                                          # off the initial weights
        loss, _ = net.train().loss(g, target, train_bits)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    want_loss, pred = net.evaluate(g, target, val_bits)
    val_loss, train_s, val_s = net.score(g, target, train_bits, val_bits)
    assert net.training and torch.equal(val_loss.view(torch.int32), want_loss.view(torch.int32))
    pred = pred.cpu().numpy()
    sel = lambda bits: [((bits.cpu().numpy() >> k) & 1).astype(bool) for k in range(K)]
    _check_scores(train_s, y, [pred[:, k] for k in range(K)], sel(train_bits))
    _check_scores(val_s, y, [pred[:, k] for k in range(K)], sel(val_bits))
    assert all(t.dtype == torch.float64 and t.is_cuda and t.shape == (K,) for t in train_s + val_s)


def test_perlabel_gcn_score_equals_host_scoring_of_its_predictions(cuda):
    N, counts = 400, [2, 5, 1]
    top_of = torch.tensor([0, 0, 1, 1, 1, 1, 1, 2])
    g = synth.word_doc_graph(N, 3000, seed=7, n_classes=8)
    group, target, got_counts, _ = relabel(g.y, top_of[g.y], torch.arange(N) >= g.n_vocab)
    assert got_counts == counts
    torch.manual_seed(3)
    net = PerLabelGCN(N, counts, n_hidden_gcn=8, dropout=0.5).to(cuda).float()
    gd = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(cuda)
    group_d, target_d = group.to(cuda), target.to(cuda)
    val_loss, train_s, val_s = net.score(gd, target_d, group_d, gd.train_mask, gd.val_mask)
    net.eval()
    with torch.no_grad():
        _, want_loss, pred = net.loss(gd, target_d, gd.val_mask, group_d, return_pred=True)
    assert torch.equal(val_loss.view(torch.int32), want_loss.view(torch.int32))
    pred, grp, tgt = pred.cpu().numpy(), group.numpy(), target.numpy()
    for s, mask in ((train_s, g.train_mask.numpy()), (val_s, g.val_mask.numpy())):
        _check_scores(s, tgt, [pred - net.seg_start[k] for k in range(3)], [mask & (grp == k) for k in range(3)])


def test_perlabel_mlp_score_equals_host_scoring_of_its_predictions(cuda):
    K, F, hid, counts, n = 3, 40, [33, 17], [2, 5, 3], 70
    gen = torch.Generator().manual_seed(100)
    group = torch.cat([torch.zeros(33), torch.full((30,), 2.0), torch.full((7,), -1.0)]).long()[torch.randperm(n, generator=gen)]
    cols = torch.stack([torch.randperm(F, generator=gen)[:6] for _ in range(n)])
    idx = torch.stack([torch.arange(n).repeat_interleave(6), cols.reshape(-1)])
    x = torch.sparse_coo_tensor(idx, torch.rand(n * 6, generator=gen) + 0.5, (n, F)).coalesce()
    target = (torch.rand(n, generator=gen) * torch.tensor(counts)[group.clamp(min=0)]).long().clamp(min=0)
    target = torch.where(group >= 0, target, torch.full_like(target, -1))
    rows = GroupedRows(group, K).to(cuda)
    torch.manual_seed(3)
    model = PerLabelMLP(F, counts, hid, dropout=0.5).to(cuda).eval()
    xg, tgt = rows.features(x.to(cuda)), rows.take(target.to(cuda))
    mask = (torch.rand(n, generator=gen) < 0.7).to(cuda) & rows.routed
    for m in (None, mask):
        loss_k, s = model.score(xg, rows, tgt, m)
        with torch.no_grad():
            _, want_loss, pred = model.loss(xg, rows, tgt, m, return_pred=True)
        assert torch.equal(loss_k.view(torch.int32), want_loss.view(torch.int32))
        sel = (rows.routed if m is None else m).cpu().numpy()
        grp = rows.group_sorted.cpu().numpy()
        pred = pred.cpu().numpy()
        _check_scores(s, tgt.cpu().numpy(), [pred - model.seg_start[k] for k in range(K)], [sel & (grp == k) for k in range(K)])
        assert np.isnan(s.f1_macro.cpu().numpy()[1]) and s.n_rows.cpu().numpy()[1] == 0          # group 1 has no document


def test_flat_loop_epoch_scored_is_epoch_plus_sklearn(cuda):
    from pytextgcn_amd.train import FlatLoop
    N, C = 1500, 7
    g = synth.word_doc_graph(N, 20000, seed=29, n_classes=C, device=cuda)
    y = g.y.cpu().numpy()
    y_val, y_train = y[g.val_mask.cpu().numpy()], y[g.train_mask.cpu().numpy()]
    runs = []
    for scored in (False, True):
        torch.manual_seed(13)
        model = pkg.GCN(N, C, n_hidden_gcn=32, dropout=0.5).to(cuda)
        torch.manual_seed(77)
        with FlatLoop(model, g, lr=0.05) as loop:
            if scored:
                runs.append([loop.epoch_scored() for _ in range(3)])
            else:
                out = []
                for _ in range(3):
                    loss, val_loss, pred_val, pred_train = loop.epoch()
                    out.append((loss, val_loss, MC.sklearn_scores(y_train, pred_train)[0], MC.sklearn_scores(y_val, pred_val)[1]))
                runs.append(out)
    for want, got in zip(*runs):
        assert got[0] == want[0] and got[1] == want[1]                          # the losses: bit for bit
        assert MC.close(got[2], want[2]) and MC.close(got[3], want[3]), (got, want)


def test_scoreboard_and_score_under_graph_replay_equal_the_eager_run(cuda):
    """Three epochs of `score()` + `Scoreboard.record`, once eagerly and once as three replays of one captured epoch
    (the weights move between the epochs in both runs): the boards are equal bit for bit."""
    g, y, net, target, train_bits, val_bits = _crossval_on_tiny(cuda)
    K, E = net.n_members, 3
    cols = ["val_loss", "train_accuracy", "val_f1", "val_rows"]
    was = conv._REUSE
    conv.enable_activation_reuse(False)
    try:
        start = {k: v.clone() for k, v in net.state_dict().items()}

        def epoch(board):
            val_loss, tr, va = net.score(g, target, train_bits, val_bits)
            board.record(val_loss=val_loss, train_accuracy=tr.accuracy, val_f1=va.f1_macro, val_rows=va.n_rows)
            with torch.no_grad():
                net.layers[1].weight.mul_(1.25)                                # the next epoch scores other weights

        eager = metrics.Scoreboard(E, K, cols, device=cuda)
        for _ in range(E):
            epoch(eager)
        want = eager.to_host()
        net.load_state_dict(start)
        board = metrics.Scoreboard(E, K, cols, device=cuda)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            epoch(metrics.Scoreboard(1, K, cols, device=cuda))                  # warm-up: the checks that synchronise
        torch.cuda.current_stream().wait_stream(side)
        net.load_state_dict(start)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            epoch(board)
        for _ in range(E):
            graph.replay()
        got = board.to_host()
    finally:
        conv.enable_activation_reuse(was)
    assert got.shape == want.shape == (E, K, len(cols)) and not np.isnan(want[:, :, 2]).any()
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert not np.array_equal(want[0], want[-1])
    mean, std = board.fold_summary("val_f1", 2, host=got)
    assert mean.shape == std.shape == (K // 2,) and np.allclose(mean, got[-1, :, 2].reshape(-1, 2).mean(1))
