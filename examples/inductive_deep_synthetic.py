#!/usr/bin/env python3
"""Classify documents that were never part of the graph with the DEEPER networks of the reference's model surface
(textgcn/lib/models.py): a `JumpingKnowledgeNetwork` and a `GCN(n_gcn=3)`, through `pytextgcn_amd.inductive.FoldInDeep`.
On a synthetic corpus because the Amazon / DBpedia CSVs are not in the reference tree (.MISSING_LARGE_BLOBS:1-3).

    python examples/inductive_deep_synthetic.py [--docs 1200] [--epochs 30] [--composed]

The graph is built WITHOUT the held-out documents; both models are trained on it with the package's masked cross-entropy;
then `FoldInDeep(model, g).predict_text(t2g, held_out)` weights the new documents with the fitted vocabulary and idf
(`Text2GraphTransformer.transform`) and carries them through all layers in one kernel launch (the JKN's LSTM aggregation
and `lin` follow on the B rows).  Printed per model: the fold-in accuracy, and the agreement with what a user would do
without it -- `model(extended_graph(g, tfidf))`, a new plan and a full forward over all N + B nodes: the share of equal
predictions and the largest relative difference of the logits.  The script reports; it asserts nothing.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import FoldInDeep, Text2GraphTransformer, enable_fused_foldin, extended_graph, synth  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402
from pytextgcn_amd.models import GCN, JumpingKnowledgeNetwork  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=1200)
p.add_argument("--epochs", type=int, default=30)
p.add_argument("--composed", action="store_true", help="enable_fused_foldin(False): the composition instead of the fused kernel")
args = p.parse_args()

seed, lr, min_df, dropout, window_size, n_hidden, n_classes = 44, 0.02, 3, 0.5, 20, 64, 6
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 2000, n_classes=n_classes, seed=seed)
y = np.asarray(y)
perm = np.random.permutation(len(docs))
n_hold = len(docs) // 10
held, inside = perm[:n_hold], perm[n_hold:]
device = th.device("cuda")
if args.composed:
    enable_fused_foldin(False)

t2g = Text2GraphTransformer(n_jobs=8, min_df=min_df, window_size=window_size, rm_stopwords=False)
g = t2g.fit_transform([docs[i] for i in inside], y[inside].tolist(), val_idx=np.arange(n_hold)).to(device)
new_docs = [docs[i] for i in held]
tfidf = t2g.transform(new_docs)
N = g.x.shape[0]
print(f"graph {g}; {len(new_docs)} new documents, {tfidf.nnz} known words, "
      f"{int((np.diff(tfidf.indptr) == 0).sum())} without any")

models = {
    "JumpingKnowledgeNetwork(n_gcn=2)": JumpingKnowledgeNetwork(N, n_classes, n_gcn=2, n_hidden_gcn=n_hidden, dropout=dropout),
    "GCN(n_gcn=3)": GCN(N, n_classes, n_gcn=3, n_hidden_gcn=n_hidden, dropout=dropout),
}
for name, model in models.items():
    model = model.to(device).float()
    opt = th.optim.Adam(model.parameters(), lr=lr)
    for epoch in range(args.epochs):
        model.train()
        loss = masked_cross_entropy(model(g), g.y, g.train_mask)
        opt.zero_grad()
        loss.backward()
        opt.step()
    model.eval()
    fold = FoldInDeep(model, g)
    th.cuda.synchronize()
    t0 = time.time()
    pred = fold.predict_text(t2g, new_docs)
    th.cuda.synchronize()
    dt = time.time() - t0
    z = fold.logits(tfidf)
    with th.no_grad():
        full = model(extended_graph(g, tfidf))[N:]
    same = float((pred == full.argmax(dim=1)).float().mean())
    rel = float((z - full).abs().max() / full.abs().max())
    acc = float((pred.cpu().numpy() == y[held]).mean())
    print(f"{name}: {args.epochs} epochs, loss {float(loss):.3f}; transform + predict {dt * 1e3:.1f} ms "
          f"({'composed' if args.composed else 'fused'})")
    print(f"{name}: fold-in accuracy {acc:.3f}")
    print(f"{name}: agreement with the full forward on the extended graph {same:.3f}, largest relative difference of the "
          f"logits {rel:.1e}")
