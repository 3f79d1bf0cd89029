#!/usr/bin/env python3
"""perlevel_amazon.py re-played on pytextgcn_amd with the graph built ONCE: a level-1 GCN on the top labels (:71-104), a
level-2 GCN on the features [I | H] with H the one-hot of the documents' true top label (:112,122-150), and the test pass
with H swapped for the softmax of the level-1 logits (:110,156-165) -- the swap happens on the device
(pytextgcn_amd.perlevel).  A synthetic corpus with a two-level label (top = class // k) stands in for the Amazon CSVs
(.MISSING_LARGE_BLOBS:1-3).  Line references: perlevel_amazon.py.

    python examples/perlevel_synthetic.py [--docs 5000] [--epochs 50]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.metrics import accuracy_score, f1_score

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import GCN, Text2GraphTransformer, synth  # noqa: E402
from pytextgcn_amd.perlevel import one_hot_hierarchy, predicted_hierarchy, with_hierarchy  # noqa: E402
from pytextgcn_amd.train import FlatLoop  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=5000)
p.add_argument("--epochs", type=int, default=50)
p.add_argument("--top", type=int, default=4, help="top-level labels")
p.add_argument("--children", type=int, default=3, help="classes under each top-level label (k)")
args = p.parse_args()

seed, lr, dropout, n_hidden = 44, 0.05, 0.7, 100                       # :22-40 (lr of the flat script: 30 epochs suffice)
k, n_top = args.children, args.top
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=n_top * k, seed=seed)
y = np.asarray(y)
y_top = y // k                                                         # :44-46,68-69
perm = np.random.permutation(len(docs))
test_idx, val_idx = perm[:len(docs) // 10], perm[len(docs) // 10:len(docs) // 5]
device = th.device("cuda")

t0 = time.time()
t2g = Text2GraphTransformer(n_jobs=8, min_df=5, window_size=20, rm_stopwords=False, verbose=1, max_df=0.7)
g = t2g.fit_transform(docs, y_top, test_idx=test_idx, val_idx=val_idx).to(device)     # :71 -- the ONE graph of all three steps
print(f"graph: {g}  ({time.time() - t0:.2f} s)")


def train(model, graph, name):
    """The loop of :89-104 / :134-150 as `FlatLoop` runs it (fused loss, fused Adam, dropout fused into the layer-2 products)."""
    th.cuda.synchronize()
    t0 = time.time()
    with FlatLoop(model, graph, lr=lr) as loop:
        y_train = graph.y[graph.train_mask].cpu().numpy()
        y_val = graph.y[graph.val_mask].cpu().numpy()
        for epoch in range(args.epochs):
            loss, val_loss, pred_val, pred_train = loop.epoch()
            if epoch % 10 == 0 or epoch == args.epochs - 1:
                print(f"{name} [{epoch + 1:3d}] loss: {loss: .3f}, val_loss: {val_loss: .3f}, training accuracy: "
                      f"{accuracy_score(y_train, pred_train):.3f}, val_f1: {f1_score(y_val, pred_val, average='macro'):.3f}")
    th.cuda.synchronize()
    print(f"{name}: {args.epochs} epochs in {time.time() - t0:.2f} s")


# ---- level 1: the top labels on one-hot node features (:71-104) ----------------------------------------------------------
level1 = GCN(g.x.shape[1], n_top, n_hidden_gcn=n_hidden, dropout=dropout).to(device).float()
train(level1, g, "level 1")

# ---- level 2: all classes on [I | one-hot of the TRUE top label] (:112,122-150): same edges, same cached operator ---------
y_nodes = th.zeros(g.num_nodes, dtype=th.long)
y_nodes[g.n_vocab:] = th.from_numpy(y)
g2 = with_hierarchy(g, one_hot_hierarchy(g, y_top, n_classes=n_top), y=y_nodes.to(device))
level2 = GCN(g2.x.shape[1], n_top * k, n_hidden_gcn=n_hidden, dropout=dropout).to(device).float()
train(level2, g2, "level 2")

# ---- test: H = softmax(level-1 logits), computed and swapped in on the device (:110,156-165) ----------------------------
g3 = with_hierarchy(g2, predicted_hierarchy(level1, g))
level2.eval()
with th.no_grad():
    logits = level2(g3)
test = g3.test_mask
y_true = g3.y[test].cpu().numpy()
pred = logits[test].argmax(1).cpu().numpy()
top_pred = g3.x.dense[(test[g.n_vocab:]).nonzero().flatten()].argmax(1).cpu().numpy()
print(f"level 1 test accuracy: {accuracy_score(y_true // k, top_pred):.3f}")
print(f"Test Accuracy: {accuracy_score(y_true, pred):.3f}  F1-Macro: {f1_score(y_true, pred, average='macro'):.3f}")
