"""GPU tests of the per-level strategy: the kernels `tgcn_hier_xw*` (pytextgcn_amd/csrc/hier.hip), `HierarchyFeatures` as
`g.x` of GCN, EGCN and JumpingKnowledgeNetwork, graph capture, and the three steps of perlevel_amazon.py on one graph.

The kernels are held to the float64 restatement of tests/_perlevel_ref.py at the project's bar, max|a - b| / max|b| <= 1e-5
(BASELINE.json; the bar of tests/test_gpu_egcn_hier.py).  A sequential fp32 evaluation of the same expressions on the CPU
stays within 1.4e-6 of float64 on every shape of CASES (worst: dWh of the dense form at (1025, 64, 128, 77); one-hot dWh at
most 9.7e-7, C at most 2.9e-7), so the bar leaves seven-fold room.  That figure -- the error of the same expressions in
float32 on the CPU, not of the kernels -- is 1.3e-7 for dWh and 3.3e-8 for C at the two shapes with 7001 document rows, whose
grouped sum runs slices of 65 rows (the kernels on an MI355X: dWh 2.9e-7, C 3.3e-8).  The exact tests hold by construction
and carry no tolerance.  The models are held to the CPU oracle (oracle/gcn_oracle.py) on the dense [I | H] matrix at the
same bar."""
import numpy as np
import pytest
import torch
from torch import nn

import pytextgcn_amd as pkg
from oracle import gcn_oracle as O
from pytextgcn_amd import _lib, conv, hier, perlevel, synth
from pytextgcn_amd.functional import masked_cross_entropy
from pytextgcn_amd.hier import HierarchyFeatures
from pytextgcn_amd.plan import plan_for

import _perlevel_ref as R
from _perlevel_ref import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
CAP = 128            # tgcn_hier_max_features(), asserted below

# (N, F, Fh, h_row0, form): F odd, not a multiple of 4 and past 256; Fh at 1 and at the cap; h_row0 inside a tile, at 0, at N
CASES = [
    (0, 64, 6, 0, "onehot"), (31, 1, 1, 0, "onehot"), (31, 64, 6, 31, "dense"), (333, 100, 6, 77, "onehot"),
    (333, 200, 33, 128, "dense"), (333, 300, CAP, 0, "onehot"), (1025, 200, 6, 700, "onehot"), (1025, 64, CAP, 77, "dense"),
    (1025, 219, 9, 0, "onehot"), (1025, 1, 70, 1025, "dense"), (1025, 300, 17, 128, "dense"), (1025, 100, 1, 0, "onehot"),
    # The grouped sum of the one-hot dWh cuts the document rows into slices of max(64, ceil(n_doc / most)) rows with most =
    # min(1024, max(16, 2^22 / (Fh round_up4(F)))): every case above has at most 1025 document rows and gets the minimum
    # of 64.  These two have n_doc = 7001 at Fh = 128, round_up4(F) = 300: most = 109, ceil(7001 / 109) = 65 rows per slice
    # -- not a multiple of 4, the unroll of the row loop -- in 108 slices, the last of 46 rows (asserted below through the
    # workspace size, 108 x 128 x 300 x 4 bytes for both).  F = 300 sums in float4 lanes, F = 299 in dword lanes.
    (7078, 300, CAP, 77, "onehot"), (7078, 299, CAP, 77, "onehot"),
]


def _class_sum_split(n_doc, F, Fh):
    """(slices, rows per slice) of the one-hot dWh: `class_sum_split` of hier.hip restated."""
    most = min(1024, max(16, (1 << 22) // (Fh * ((F + 3) & ~3))))
    rows = max(64, -(-n_doc // most))
    return -(-n_doc // rows), rows


def _feats(N, h_row0, held, Fh, dev):
    if held.dtype.is_floating_point:
        return HierarchyFeatures(N, h_row0, dense=held.to(dev))
    return HierarchyFeatures(N, h_row0, classes=held.to(dev), n_classes=Fh)


@pytest.mark.parametrize("N,F,Fh,h_row0,form", CASES)
def test_kernels_against_float64(cuda, N, F, Fh, h_row0, form):
    assert hier.max_features() == CAP
    W, G, held = R.operands(N, F, Fh, h_row0, form, 3000 + N + F + Fh)
    feats = _feats(N, h_row0, held, Fh, cuda)
    if form == "onehot" and N > h_row0:                      # the slices of the grouped sum, seen through its workspace
        slices, rows = _class_sum_split(N - h_row0, F, Fh)
        assert _lib.load().tgcn_hier_xw_grad_workspace_bytes(N, F, Fh, h_row0, _lib.HIER_ONEHOT) == slices * Fh * ((F + 3) & ~3) * 4
        if N == 7078:
            assert (slices, rows, N - h_row0 - 107 * rows) == (108, 65, 46) and slices * Fh * ((F + 3) & ~3) * 4 == 108 * 128 * 300 * 4
        else:
            assert rows == 64
    C = hier.xw_forward(feats, W.to(cuda))
    dW = hier.xw_backward(feats, G.to(cuda))
    torch.cuda.synchronize()
    assert C.shape == (N, F) and dW.shape == (N + Fh, F)
    tC, tdW = R.truth(W, G, held, h_row0)
    if N == 0 or h_row0 == N:
        assert float(dW[N:].abs().sum()) == 0.0              # nobody has a row: exact zeros
        if N == 0:
            return
    errs = {"C": rel_err(C, tC), "dWh": rel_err(dW[N:], tdW[N:]) if h_row0 < N else 0.0}
    print(f"hier kernels N={N} F={F} Fh={Fh} h_row0={h_row0} {form}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.equal(dW[:N].cpu(), G)                      # the first N rows ARE the incoming gradient
    assert torch.equal(C[:h_row0].cpu(), W[:h_row0])         # the rows below h_row0 are W's rows
    assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("F,lead", [(100, 2), (64, 4)])       # dword lanes (rows not 16-byte aligned) and float4 lanes
@pytest.mark.parametrize("form", ["onehot", "dense"])
def test_column_slices_of_wider_buffers_and_nothing_outside_them(cuda, form, F, lead):
    N, Fh, h_row0 = 333, 6, 77
    W, G, held = R.operands(N, F, Fh, h_row0, form, 7)
    wide = torch.full((N, F + 12), 7.0, device=cuda)
    out = wide[:, lead:lead + F]
    Gw = torch.full((N, F + 8), 5.0, device=cuda)
    Gw[:, lead:lead + F] = G.to(cuda)
    dWw = torch.full((N + Fh, F + 8), 9.0, device=cuda)
    if form == "dense":
        Hw = torch.full((N - h_row0, Fh + 5), 3.0, device=cuda)
        Hw[:, 1:1 + Fh] = held.to(cuda)
        feats = HierarchyFeatures(N, h_row0, dense=Hw[:, 1:1 + Fh])
        assert feats.dense.data_ptr() == Hw.data_ptr() + 4             # the slice itself, not a copy
    else:
        feats = _feats(N, h_row0, held, Fh, cuda)
    C = hier.xw_forward(feats, W.to(cuda), out=out)
    dW = hier.xw_backward(feats, Gw[:, lead:lead + F], out=dWw[:, lead:lead + F])
    torch.cuda.synchronize()
    assert C.data_ptr() == out.data_ptr() and dW.data_ptr() == dWw[:, lead:].data_ptr()
    for buf, fill in ((wide, 7.0), (dWw, 9.0), (Gw, 5.0)):
        assert bool((buf[:, :lead] == fill).all()) and bool((buf[:, lead + F:] == fill).all())
    if form == "dense":
        assert bool((Hw[:, :1] == 3.0).all()) and bool((Hw[:, 1 + Fh:] == 3.0).all())
    tC, tdW = R.truth(W, G, held, h_row0)
    assert rel_err(C, tC) <= TOL and rel_err(dW[N:], tdW[N:]) <= TOL and torch.equal(dW[:N].cpu(), G)
    # the same bits as on contiguous operands, whichever lanes ran (the dense form's dWh is tgcn_gemm_tn's, not held to that)
    assert torch.equal(C, hier.xw_forward(feats, W.to(cuda)))
    if form == "onehot":
        assert torch.equal(dW, hier.xw_backward(feats, G.to(cuda)))


@pytest.mark.parametrize("N,F,Fh,h_row0", [(333, 100, 6, 77), (1025, 219, 9, 0), (333, 300, CAP, 0), (1025, 64, 33, 700)])
def test_exact_properties(cuda, N, F, Fh, h_row0):
    W, G, cls = R.operands(N, F, Fh, h_row0, "onehot", 11 + N)
    Wd, Gd = W.to(cuda), G.to(cuda)
    onehot = _feats(N, h_row0, cls, Fh, cuda)
    C = hier.xw_forward(onehot, Wd)
    # ONEHOT == DENSE on the one-hot rows, and == w[:N] + Wh[cls] in torch, bit for bit
    assert torch.equal(C, hier.xw_forward(HierarchyFeatures(N, h_row0, dense=R.one_hot(cls, Fh).to(cuda)), Wd))
    want = Wd[:N].clone()
    want[h_row0:] += Wd[N:][cls.long().to(cuda)]
    assert torch.equal(C, want)
    # an empty class has an exactly zero row; two runs give equal bits
    spare = cls.clone()
    spare[spare == Fh - 1] = 0 if Fh > 1 else -1
    f2 = _feats(N, h_row0, spare, Fh, cuda)
    dW = hier.xw_backward(f2, Gd)
    assert torch.equal(dW[:N], Gd) and float(dW[N + Fh - 1].abs().sum()) == 0.0
    assert torch.equal(dW, hier.xw_backward(f2, Gd))
    if Fh > 1:
        assert float(dW[N].abs().sum()) > 0.0
    # ids that select nothing (-1, Fh): the rows behave as rows without a term, in both directions
    holes = cls.clone()
    holes[::3] = -1
    holes[1::5] = Fh
    kept = (holes >= 0) & (holes < Fh)
    f3 = _feats(N, h_row0, holes, Fh, cuda)
    C3, dW3 = hier.xw_forward(f3, Wd), hier.xw_backward(f3, Gd)
    torch.cuda.synchronize()
    rows = torch.arange(h_row0, N)
    assert torch.equal(C3[rows[~kept]].cpu(), W[rows[~kept]])
    assert torch.equal(C3[rows[kept]], C[rows[kept]])
    tC, tdW = R.truth(W, G, holes, h_row0)
    assert rel_err(C3, tC) <= TOL and rel_err(dW3[N:], tdW[N:]) <= TOL and torch.equal(dW3[:N], Gd)


# ------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------
N_NODES, FH, N_CLASSES = 400, 6, 5


class _Small:
    """A word-document graph of a few hundred nodes with both forms of the hierarchy features, built once."""

    def __init__(self, cuda):
        g = synth.word_doc_graph(N_NODES, 4000, seed=5, n_classes=N_CLASSES)
        self.g, self.h_row0 = g, g.n_vocab
        gen = torch.Generator().manual_seed(9)
        rows = N_NODES - g.n_vocab
        self.held = {"onehot": torch.randint(0, FH, (rows,), generator=gen).to(torch.int32),
                     "dense": torch.softmax(2.0 * torch.randn(rows, FH, generator=gen), dim=1)}
        base = {k: getattr(g, k) for k in ("edge_index", "edge_attr", "y", "train_mask", "val_mask", "test_mask", "n_vocab")}
        self.sparse = {k: R.sparse_features(N_NODES, g.n_vocab, v, FH) for k, v in self.held.items()}
        self.cpu = {k: pkg.Data(x=v.to_dense(), **base) for k, v in self.sparse.items()}          # the oracle's input
        dev = pkg.Data(x=g.x, **base).to(cuda)
        self.on_sparse = {k: perlevel.with_hierarchy(dev, v.to(cuda)) for k, v in self.sparse.items()}
        self.on_feats = {k: perlevel.with_hierarchy(dev, _feats(N_NODES, g.n_vocab, v, FH, cuda)) for k, v in self.held.items()}


@pytest.fixture(scope="module")
def small(cuda):
    return _Small(cuda)


def _pair(cuda, cls=pkg.GCN, hidden=20, **kw):
    torch.manual_seed(4)
    ref = O.GCNOracle(N_NODES + FH, N_CLASSES, n_hidden_gcn=hidden, dropout=0.0)
    with torch.no_grad():
        ref.layers[0].bias.normal_(0, 0.1)
    mine = cls(N_NODES + FH, N_CLASSES, n_hidden_gcn=hidden, dropout=0.0, **kw)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(cuda).float()


def _step(model, g):
    logits = model(g)
    loss = nn.CrossEntropyLoss()(logits[g.train_mask], g.y[g.train_mask])
    model.zero_grad(set_to_none=True)
    loss.backward()
    return logits.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("form", ["onehot", "dense"])
def test_gcn_logits_and_gradients_against_the_oracle(cuda, small, form):
    ref, mine = _pair(cuda)
    with torch.no_grad():
        want = ref.eval()(small.cpu[form])
        on_feats = mine.eval()(small.on_feats[form])
        on_sparse = mine(small.on_sparse[form])
    if form == "onehot":
        assert torch.equal(on_feats, on_sparse)               # each row of H @ Wh has exactly one term: the same bits
    errs = {"features": rel_err(on_feats, want), "sparse": rel_err(on_sparse, want)}
    want_logits, want_grads = _step(ref.train(), small.cpu[form])
    for tag, g in (("features", small.on_feats[form]), ("sparse", small.on_sparse[form])):
        logits, grads = _step(mine.train(), g)
        assert set(grads) == set(want_grads) and grads["layers.0.weight"].shape == (N_NODES + FH, 20)
        errs[tag + " train logits"] = rel_err(logits, want_logits)
        errs.update({f"{tag} d {k}": rel_err(grads[k], want_grads[k]) for k in want_grads})
    print(f"GCN on [I|H] {form}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs


def test_collapsed_eval_forward_takes_the_features(cuda, small):
    ref, mine = _pair(cuda)
    with torch.no_grad():
        want = ref.eval()(small.cpu["dense"])
        pkg.enable_linear_collapse(True)
        try:
            got = mine.eval()(small.on_feats["dense"])
        finally:
            pkg.enable_linear_collapse(False)
    assert rel_err(got, want) <= TOL


def test_apply_activation_goes_through_unchanged(cuda, small):
    _, mine = _pair(cuda, apply_activation=True)
    with torch.no_grad():
        assert torch.equal(mine.eval()(small.on_feats["onehot"]), mine(small.on_sparse["onehot"]))
    (la, ga), (lb, gb) = _step(mine.train(), small.on_feats["dense"]), _step(mine, small.on_sparse["dense"])
    assert rel_err(la, lb) <= TOL and set(ga) == set(gb) and all(rel_err(ga[k], gb[k]) <= TOL for k in gb)
    _, plain = _pair(cuda)
    with torch.no_grad():
        assert not torch.equal(plain.eval()(small.on_feats["onehot"]), mine.eval()(small.on_feats["onehot"]))   # the ReLU is there


@pytest.mark.parametrize("form", ["onehot", "dense"])
def test_egcn_takes_the_fused_product_with_the_bits_of_the_switch(cuda, small, form):
    torch.manual_seed(2)
    m = pkg.EGCN(N_NODES + FH, N_CLASSES, embedding_dim=48, n_hidden_gcn=20, dropout=0.0).to(cuda).float().eval()
    assert m.takes_fused_path(small.on_feats[form].x) and not m.takes_fused_path(small.on_sparse[form].x)
    was = pkg.enable_fused_hierarchy_embedding(True)
    try:
        assert m.takes_fused_path(small.on_sparse[form].x)
        with torch.no_grad():
            assert torch.equal(m(small.on_feats[form]), m(small.on_sparse[form]))
    finally:
        pkg.enable_fused_hierarchy_embedding(was)
    # the composition (the master switch off) goes through `to_sparse()` and agrees at the bar
    with torch.no_grad():
        fused = m(small.on_feats[form])
        pkg.enable_fused_embedding(False)
        try:
            assert not m.takes_fused_path(small.on_feats[form].x)
            assert rel_err(m(small.on_feats[form]), fused) <= TOL
        finally:
            pkg.enable_fused_embedding(True)


def test_jumping_knowledge_network_runs_on_the_features(cuda, small):
    torch.manual_seed(6)
    m = pkg.JumpingKnowledgeNetwork(N_NODES + FH, N_CLASSES, n_hidden_gcn=16, dropout=0.0).to(cuda).float()
    (la, ga), (lb, gb) = _step(m.train(), small.on_feats["onehot"]), _step(m, small.on_sparse["onehot"])
    assert rel_err(la, lb) <= TOL and set(ga) == set(gb) and all(rel_err(ga[k], gb[k]) <= TOL for k in gb)
    with torch.no_grad():
        assert rel_err(m.eval()(small.on_feats["dense"]), m(small.on_sparse["dense"])) <= TOL


def test_graph_capture_of_a_training_step_on_the_features(cuda, small):
    """`GraphedTrainStep` (fused CE, capturable fused Adam) captures and replays a step on `HierarchyFeatures`: three
    replays equal the eager steps of a twin model at dropout 0, bit for bit."""
    from pytextgcn_amd.train import GraphedTrainStep
    gd = small.on_feats["onehot"]
    (_, a), (_, b) = _pair(cuda, hidden=32), _pair(cuda, hidden=32)
    opts = [pkg.optim.Adam(m.parameters(), lr=0.05, amsgrad=True, capturable=True) for m in (a, b)]
    step = GraphedTrainStep(a, gd, opts[0], gd.train_mask, warmup=2)
    losses = [step().item() for _ in range(3)]
    b.train()
    eager = []
    for _ in range(5):
        loss = masked_cross_entropy(b(gd), gd.y, gd.train_mask)
        opts[1].zero_grad(set_to_none=True)
        loss.backward()
        opts[1].step()
        eager.append(loss.item())
    torch.cuda.synchronize()
    assert losses == eager[2:]
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)


# ------------------------------------------------------------------------------------------------
# perlevel_amazon.py's three steps on one graph
# ------------------------------------------------------------------------------------------------
def test_per_level_end_to_end(cuda):
    """300 documents, 2 x 3 classes (top = class // 3), dropout 0 so that the run is the same arithmetic everywhere: level 1
    on the top labels, level 2 on the one-hot of the true top labels, prediction on the level-1 softmax -- on ONE graph.
    With the top label among its features the level-2 model fits the training documents sooner than the flat model on
    the same seed after the same epochs.  That is a property of the early epochs (with one-hot node features both
    networks memorise 240 training documents within ~20 epochs at this size), so seed and epoch count were chosen in the
    CPU oracle's arithmetic first (GCNOracle, torch's CE and Adam(amsgrad), lr 0.02): seed 46 after 8 epochs gives training
    accuracies of 0.433 (flat) and 0.658 (level 2), a margin of 54 of the 240 documents; level 1 reaches 1.000."""
    from pytextgcn_amd.train import FlatLoop
    seed, epochs, k = 46, 8, 3
    docs, y = synth.synthetic_corpus(300, 400, n_classes=2 * k, seed=seed)
    y = np.asarray(y)
    perm = np.random.default_rng(seed).permutation(len(docs))
    t2g = pkg.Text2GraphTransformer(n_jobs=1, min_df=2, window_size=5, rm_stopwords=False, verbose=0, max_df=0.7)
    g = t2g.fit_transform(docs, y // k, test_idx=perm[:30], val_idx=perm[30:60]).to(cuda)
    N = g.num_nodes
    y_nodes = torch.zeros(N, dtype=torch.long)
    y_nodes[g.n_vocab:] = torch.from_numpy(y)
    y_nodes = y_nodes.to(cuda)

    def train(graph, n_out):
        torch.manual_seed(seed)
        model = pkg.GCN(graph.x.size(1), n_out, n_hidden_gcn=32, dropout=0.0).to(cuda).float()
        with FlatLoop(model, graph, lr=0.02) as loop:
            for _ in range(epochs):
                pred_train = loop.epoch()[3]
        want = graph.y[graph.train_mask].cpu().numpy()
        return model, float((pred_train == want).mean())

    level1, acc1 = train(g, 2)                                                     # perlevel_amazon.py:71-104
    plan = plan_for(g.edge_index, g.edge_attr, N)
    g2 = perlevel.with_hierarchy(g, perlevel.one_hot_hierarchy(g, y // k, n_classes=2), y=y_nodes)     # :112,122
    assert plan_for(g2.edge_index, g2.edge_attr, N) is plan and level1.layers[0].plan(g2.x, g2.edge_index, g2.edge_attr) is plan
    level2, acc2 = train(g2, 2 * k)                                                # :124-150
    flat, acc_flat = train(perlevel.with_hierarchy(g, g.x, y=y_nodes), 2 * k)      # the flat model of flat_amazon.py
    feats = perlevel.predicted_hierarchy(level1, g)                                # :110
    assert feats.is_cuda and feats.dense.shape == (N - g.n_vocab, 2) and feats.h_row0 == g.n_vocab and not level1.training
    assert float((feats.dense.sum(1) - 1).abs().max()) <= 1e-6
    g3 = perlevel.with_hierarchy(g2, feats)                                        # :156
    assert plan_for(g3.edge_index, g3.edge_attr, N) is plan and g3.y is g2.y
    level2.eval()
    with torch.no_grad():
        pred = level2(g3)[g3.test_mask].argmax(1)
    acc_test = float((pred == g3.y[g3.test_mask]).float().mean())
    print(f"per level: level-1 train acc {acc1:.3f}, level-2 train acc {acc2:.3f}, flat train acc {acc_flat:.3f}, "
          f"level-2 test acc on predicted features {acc_test:.3f}")
    assert pred.numel() == 30 and acc1 > 0.5
    assert acc2 > acc_flat, (acc2, acc_flat)
