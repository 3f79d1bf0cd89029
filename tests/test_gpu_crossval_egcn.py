"""GPU tests of `crossval.CrossValEGCN`: the EGCN members of a sweep cell as one network, its member-batched front end
(`embed.embed_xw_members`), the dropout on the logits and `MemberAdam` on its row and column blocks.

The graph is tests/test_gpu_crossval.py's: 400 nodes of `synth.word_doc_graph`, M = 6 members (2 rates x 3 folds), D = 70
(no multiple of the k tile of 32), h in {8, 40}, C = 5; the features are the sparse identity or a one-hot
`hier.HierarchyFeatures` with Fh = 3 on the document rows.  The truth is tests/_egcn_ref.py's `EGCNRef` in float64, one
model per member, under `torch.optim.Adam(lr=LRS[m])`, held at the project's bar max|a - b| / max|b| <= 1e-5
(BASELINE.json) with the bounds of test_gpu_crossval.py's training-step test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _crossval_ref as R
import _metrics_cases as MC
import pytextgcn_amd as pkg
from _egcn_ref import EGCNRef
from pytextgcn_amd import embed, hier, models, synth
from pytextgcn_amd.crossval import CrossValEGCN, MemberAdam, fold_bits, member_logits_dropout

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, N_CLASSES, N_FOLDS, EMBED = 400, 5, 3, 70
RATES = (0.05, 0.01)
LRS = [lr for lr in RATES for _ in range(N_FOLDS)]                   # member l * 3 + f: rate l, fold f
ADAM_EPS = 0.1


def _build(cuda, h, feats):
    """6 `EGCN`s with random biases, the one network built from them, and per member the float64 reference's logits,
    loss, gradients and parameters after one `torch.optim.Adam(lr=LRS[k], eps=ADAM_EPS)` step (computed once)."""
    N, C, K, D = N_NODES, N_CLASSES, len(LRS), EMBED
    g = synth.word_doc_graph(N, 3000, seed=7, n_classes=C)
    doc_rows = np.arange(g.n_vocab, N)
    order = np.random.default_rng(11).permutation(doc_rows.size)
    folds = [np.sort(order[f::N_FOLDS]) for f in range(N_FOLDS)]
    train_bits, val_bits = fold_bits(doc_rows, folds, N, n_repeats=len(RATES))
    target = g.y.clone().long()
    if feats == "hier":
        x = hier.HierarchyFeatures(N, g.n_vocab, classes=(g.y[g.n_vocab:].long() * 7 + 1) % 3, n_classes=3)
        x64 = x.to_sparse().double()
    else:
        x, x64 = g.x, g.x.double()
    n_in = x.size(1)
    torch.manual_seed(3 + h)
    members = [pkg.EGCN(n_in, C, embedding_dim=D, n_hidden_gcn=h, dropout=0.0) for _ in range(K)]
    with torch.no_grad():
        for mem in members:
            for layer in mem.layers[1:]:
                layer.bias.uniform_(-0.5, 0.5)
    g64 = pkg.Data(x=x64, edge_index=g.edge_index, edge_attr=g.edge_attr.double())
    crit = torch.nn.CrossEntropyLoss(reduction="mean")
    truth = []
    for k, mem in enumerate(members):
        ref = EGCNRef(n_in, C, embedding_dim=D, n_hidden_gcn=h, dropout=0.0)
        ref.load_state_dict(mem.state_dict())
        ref = ref.double().train()
        z = ref(g64)
        sel = R.selected(train_bits, k)
        lk = crit(z[sel], target[sel])
        lk.backward()
        before = {n_: p.detach().clone() for n_, p in ref.named_parameters()}
        grads = {n_: p.grad.clone() for n_, p in ref.named_parameters()}
        torch.optim.Adam(ref.parameters(), lr=LRS[k], eps=ADAM_EPS).step()
        truth.append(dict(logits=z.detach(), loss=lk.item(), grads=grads, before=before,
                          after={n_: p.detach().clone() for n_, p in ref.named_parameters()}))
    net = CrossValEGCN.from_members(members).to(cuda).float()
    gd = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(cuda)
    gd.x = x.to(cuda)
    return dict(g=g, gd=gd, target=target.to(cuda), train_bits=train_bits.to(cuda), val_bits=val_bits.to(cuda),
                bits_host=(train_bits, val_bits), members=members, truth=truth, net=net, h=h, N=N, K=K, C=C, D=D, feats=feats)


@pytest.fixture(scope="module", params=[(8, "identity"), (40, "identity"), (8, "hier"), (40, "hier")],
                ids=["h8-identity", "h40-identity", "h8-hierarchy", "h40-hierarchy"])
def small(request, cuda):
    return _build(cuda, *request.param)


def _member_slices(net, k):
    D, h, S, C = net.embedding_dim, net.n_hidden, net.seg_stride, net.out_channels
    emb, first, second = net.layers
    rows = slice(k * D, (k + 1) * D)
    return {"layers.0.weight": (emb.weight, (rows,)),
            "layers.0.bias": (emb.bias, (rows,)),
            "layers.1.weight": (first.weight, (rows,)),
            "layers.1.bias": (first.bias, (slice(k * h, (k + 1) * h),)),
            "layers.2.weight": (second.weight, (slice(None), slice(k * S, k * S + C))),
            "layers.2.bias": (second.bias, (slice(k * S, k * S + C),))}


def test_eval_logits_of_every_member_against_the_reference_the_exported_egcn_and_the_composed_path(cuda, small):
    net, gd, C, S, K = small["net"].eval(), small["gd"], small["C"], small["net"].seg_stride, small["K"]
    assert net.layers[0].weight.shape == (K * small["D"], gd.x.size(1)) and S == 8
    assert net.layers[1].weight.shape == (K * small["D"], small["h"]) and net.layers[1].bias.shape == (K * small["h"],)
    with torch.no_grad():
        assert net.takes_fused_path(gd.x)
        z = net(gd)
        assert z.shape == (small["N"], K * S)
        exported = net.export_members()
        for k in range(K):
            assert R.rel_err(z[:, k * S:k * S + C], small["truth"][k]["logits"]) <= TOL
            assert exported[k].eval().takes_fused_path(gd.x)
            assert R.rel_err(z[:, k * S:k * S + C], exported[k](gd).double()) <= TOL
        was = pkg.enable_fused_embedding(False)
        try:
            assert not net.takes_fused_path(gd.x)
            composed = net(gd)
        finally:
            pkg.enable_fused_embedding(was)
        for k in range(K):
            assert R.rel_err(composed[:, k * S:k * S + C], z[:, k * S:k * S + C].double()) <= TOL
        val_k, pred = net.evaluate(gd, small["target"], small["val_bits"])
        assert not net.training and pred.shape == (small["N"], K)
        want = R.member_ce(z, small["target"], small["val_bits"], K, C, S)
        assert R.rel_err(val_k, want[1]) <= TOL and torch.equal(pred.cpu(), want[4])


def test_one_training_step_at_rate_zero_against_m_reference_models(cuda, small):
    net, gd, K = small["net"].train(), small["gd"], small["K"]
    start = {n_: p.detach().clone() for n_, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    assert net.takes_fused_path(gd.x)
    loss, loss_k = net.loss(gd, small["target"], small["train_bits"])
    loss.backward()
    torch.cuda.synchronize()
    truth = small["truth"]
    total = sum(t["loss"] for t in truth)
    assert abs(loss.item() - total) <= TOL * total
    for k in range(K):
        want = truth[k]
        assert abs(float(loss_k[k]) - want["loss"]) <= TOL * want["loss"], (k, float(loss_k[k]), want["loss"])
        for name, (p, idx) in _member_slices(net, k).items():
            e = R.rel_err(p.grad[idx], want["grads"][name])
            print(f"h={small['h']} {small['feats']} member {k} {name} gradient: {e:.2e}")
            assert e <= TOL, (k, name, e)
    pad = torch.ones(net.n_cols, dtype=torch.bool)
    for k in range(K):
        pad[k * net.seg_stride:k * net.seg_stride + net.out_channels] = False
    second = net.layers[2]
    assert bool((second.weight.grad.cpu()[:, pad] == 0.0).all()) and bool((second.bias.grad.cpu()[pad] == 0.0).all())
    # one step of MemberAdam(eps = 0.1): see test_gpu_crossval.py for why the comparison runs at that eps
    opt = MemberAdam(net, LRS, eps=ADAM_EPS)
    opt.step()
    torch.cuda.synchronize()
    try:
        for k in range(K):
            want = truth[k]
            for name, (p, idx) in _member_slices(net, k).items():
                got = p.detach()[idx].cpu().double()
                assert R.rel_err(got, want["after"][name]) <= TOL, (k, name)
                upd, wupd = got - want["before"][name], want["after"][name] - want["before"][name]
                bound = TOL * float(wupd.abs().max()) + 2.0 ** -23 * float(want["after"][name].abs().max())
                assert float((upd - wupd).abs().max()) <= bound, (k, name, float((upd - wupd).abs().max()), bound)
        assert bool((second.weight.detach().cpu()[:, pad] == 0.0).all()) and bool((second.bias.detach().cpu()[pad] == 0.0).all())
    finally:
        with torch.no_grad():                                                     # (the fixture is shared)
            for n_, p in net.named_parameters():
                p.copy_(start[n_])
        net.zero_grad(set_to_none=True)


def test_fused_front_end_is_embed_xw_per_member_bit_for_bit(cuda, small):
    net, gd, K, D, h, N = small["net"], small["gd"], small["K"], small["D"], small["h"], small["N"]
    rates = [(0.0, 0.3, 0.7)[k % 3] for k in range(K)]
    emb, first = net.layers[0], net.layers[1]
    hd, h_row0 = models.fused_embedding_operand(gd.x)
    gen = torch.Generator().manual_seed(23)
    G = torch.randn(N, K * h, generator=gen).to(cuda)
    seeds = torch.tensor([0x1234567890ABCDE, -77, (1 << 40) + 12345, 5, -(1 << 62), 99][:K], dtype=torch.int64, device=cuda)
    E, b, W = (t.detach().clone().requires_grad_() for t in (emb.weight, emb.bias, first.weight))
    out = embed.embed_xw_members(E, b, W, K, rates, seeds, h=hd, h_row0=h_row0)
    out.backward(G)
    for k in range(K):
        rows = slice(k * D, (k + 1) * D)
        Ek, bk, Wk = (t.detach()[rows].clone().requires_grad_() for t in (emb.weight, emb.bias, first.weight))
        ok = embed.embed_xw(Ek, bk, Wk, rates[k], seeds[k:k + 1] if rates[k] > 0 else None, h=hd, h_row0=h_row0)
        ok.backward(G[:, k * h:(k + 1) * h])
        assert torch.equal(out[:, k * h:(k + 1) * h], ok), k
        assert torch.equal(E.grad[rows], Ek.grad) and torch.equal(b.grad[rows], bk.grad) and torch.equal(W.grad[rows], Wk.grad), k
    was, kept = models._FUSED_DROPOUT, net.dropout
    try:
        pkg.enable_fused_dropout()
        net.dropout = tuple(rates)
        assert net.train().takes_fused_path(gd.x)
        z1, z2 = net(gd), net(gd)
        assert bool(torch.isfinite(z1).all()) and not torch.equal(z1, z2)         # fresh seeds per member and forward
        pkg.enable_fused_dropout(False)
        assert not net.takes_fused_path(gd.x)                                     # torch's stream: the composed front end
        assert bool(torch.isfinite(net(gd)).all())
    finally:
        pkg.enable_fused_dropout(was)
        net.dropout = kept
        net.eval()
    assert models._FUSED_DROPOUT == was


def test_logits_dropout_one_draw_for_all_members(cuda):
    M, C, S, N = 6, 5, 8, 20000
    rates = [0.0, 0.3, 0.7, 0.5, 0.0, 0.9]
    torch.manual_seed(1)
    z = torch.randn(N, M * S, device=cuda) + 3.0
    z.view(N, M, S)[:, :, C:] = 0.0                                               # the pad columns of real logits
    out = member_logits_dropout(z, rates, C, S)
    z3, o3 = z.view(N, M, S).double().cpu(), out.view(N, M, S).double().cpu()
    assert bool((o3[:, :, C:] == 0.0).all())
    for m, p in enumerate(rates):
        zm, om = z3[:, m, :C], o3[:, m, :C]
        kept = om != 0.0
        scaled = (zm.float() * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)).double()      # z * scale in float32
        assert torch.equal(om[kept], scaled[kept])                                # every entry is 0 or z / (1 - p_m)
        n, share = zm.numel(), kept.double().mean().item()
        sd = (p * (1.0 - p) / n) ** 0.5
        assert abs(share - (1.0 - p)) <= 5.0 * sd, (m, p, share)
        if p == 0.0:
            assert torch.equal(out.view(N, M, S)[:, m], z.view(N, M, S)[:, m])    # untouched, bit for bit
    assert not torch.equal(member_logits_dropout(z, rates, C, S), out)            # torch's stream moves on


def test_score_equals_host_scoring_of_evaluate(cuda, small):
    net, gd, K = small["net"], small["gd"], small["K"]
    y = small["g"].y.numpy().astype(np.int64)
    val_k, pred = net.evaluate(gd, small["target"], small["val_bits"])
    val_k2, tr, va = net.score(gd, small["target"], small["train_bits"], small["val_bits"])
    assert torch.equal(val_k, val_k2)
    pred = pred.cpu().numpy()
    for got, bits in ((tr, small["bits_host"][0]), (va, small["bits_host"][1])):
        acc, f1, n_rows = (t.cpu().numpy() for t in (got.accuracy, got.f1_macro, got.n_rows))
        for k in range(K):
            sel = R.selected(bits, k).numpy()
            want = MC.sklearn_scores(y[sel], pred[sel, k])
            assert n_rows[k] == sel.sum() and MC.close(acc[k], want[0]) and MC.close(f1[k], want[1]), (k, acc[k], f1[k], want)


def test_the_example_runs(cuda):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "crossval_egcn_synthetic.py"), "--docs", "300",
                          "--epochs", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "front end of 12 members as one product: True" in out.stdout and "EGCN: mean f1" in out.stdout
