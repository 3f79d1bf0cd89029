#!/usr/bin/env python3
"""examples/perlevel_synthetic.py with a tenth of the corpus held OUT of the graph: both levels are trained on the graph of
the other documents (perlevel_amazon.py:71-150), then `FoldInLevels(...).predict_text` labels the held-out documents on
both levels in one kernel launch -- level 2 sees the softmax of their own level-1 logits, as the script's test pass does for
graph nodes (:110,156-165).  The reference cannot do this: its test documents must be nodes of the graph.

    python examples/inductive_perlevel_synthetic.py [--docs 5000] [--epochs 50] [--composed]

The script reports the accuracies on the held-out documents next to those of the in-graph test split; it asserts neither.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.metrics import accuracy_score

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import GCN, FoldInLevels, Text2GraphTransformer, enable_fused_foldin, synth  # noqa: E402
from pytextgcn_amd.perlevel import one_hot_hierarchy, predicted_hierarchy, with_hierarchy  # noqa: E402
from pytextgcn_amd.train import FlatLoop  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=5000)
p.add_argument("--epochs", type=int, default=50)
p.add_argument("--top", type=int, default=4, help="top-level labels")
p.add_argument("--children", type=int, default=3, help="classes under each top-level label (k)")
p.add_argument("--composed", action="store_true", help="enable_fused_foldin(False): the composition instead of the fused kernel")
args = p.parse_args()

seed, lr, dropout, n_hidden = 44, 0.05, 0.7, 100
k, n_top = args.children, args.top
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=n_top * k, seed=seed)
y = np.asarray(y)
perm = np.random.permutation(len(docs))
n_hold = len(docs) // 10
held, inside = perm[:n_hold], perm[n_hold:]                            # the held-out tenth never enters the graph
docs_in, y_in = [docs[i] for i in inside], y[inside]
test_idx, val_idx = np.arange(n_hold), np.arange(n_hold, 2 * n_hold)   # the in-graph test split, of the same size
device = th.device("cuda")
if args.composed:
    enable_fused_foldin(False)

t2g = Text2GraphTransformer(n_jobs=8, min_df=5, window_size=20, rm_stopwords=False, max_df=0.7)
g = t2g.fit_transform(docs_in, y_in // k, test_idx=test_idx, val_idx=val_idx).to(device)
print(f"graph: {g}")


def train(model, graph, name):
    with FlatLoop(model, graph, lr=lr) as loop:
        for epoch in range(args.epochs):
            loss, val_loss, _, _ = loop.epoch()
    print(f"{name}: {args.epochs} epochs, loss {float(loss):.3f}, val_loss {float(val_loss):.3f}")
    return model.eval()


level1 = train(GCN(g.x.shape[1], n_top, n_hidden_gcn=n_hidden, dropout=dropout).to(device).float(), g, "level 1")
y_nodes = th.zeros(g.num_nodes, dtype=th.long)
y_nodes[g.n_vocab:] = th.from_numpy(y_in)
g2 = with_hierarchy(g, one_hot_hierarchy(g, y_in // k, n_classes=n_top), y=y_nodes.to(device))
level2 = train(GCN(g2.x.shape[1], n_top * k, n_hidden_gcn=n_hidden, dropout=dropout).to(device).float(), g2, "level 2")

# in-graph test split: H = softmax(level-1 logits) of every document (:110,156-165)
g3 = with_hierarchy(g2, predicted_hierarchy(level1, g))
with th.no_grad():
    top_in = level1(g)[g.test_mask].argmax(1).cpu().numpy()
    fin_in = level2(g3)[g3.test_mask].argmax(1).cpu().numpy()
y_test = g3.y[g3.test_mask].cpu().numpy()

# held-out documents: the old documents keep the H the graph is served with (the predicted one), the new ones get their own
fold = FoldInLevels([level1, level2], [g, g3])
new_docs = [docs[i] for i in held]
th.cuda.synchronize()
t0 = time.time()
pred = fold.predict_text(t2g, new_docs).cpu().numpy()
dt = time.time() - t0
tfidf = t2g.transform(new_docs)
print(f"  {len(new_docs)} new documents, {tfidf.nnz} known words, {int((np.diff(tfidf.indptr) == 0).sum())} without any; "
      f"transform + predict {dt * 1e3:.1f} ms ({'composed' if args.composed else 'fused'})")
print(f"in-graph test split: level 1 accuracy {accuracy_score(y_test // k, top_in):.3f}, final accuracy "
      f"{accuracy_score(y_test, fin_in):.3f}")
print(f"held-out documents:  level 1 accuracy {accuracy_score(y[held] // k, pred[:, 0]):.3f}, final accuracy "
      f"{accuracy_score(y[held], pred[:, 1]):.3f}")
