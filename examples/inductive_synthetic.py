#!/usr/bin/env python3
"""Classify documents that were never part of the graph (pytextgcn_amd.inductive.FoldIn), next to the reference's way of
testing, where the test documents are nodes of the training graph (flat_amazon.py:57-71: `fit_transform(X, y, test_idx=...)`
sees train and test documents together; there is no `transform`).  On a synthetic corpus because the Amazon / DBpedia CSVs
are not in the reference tree (.MISSING_LARGE_BLOBS:1-3).

    python examples/inductive_synthetic.py [--docs 3000] [--epochs 40] [--relu] [--composed]

Two runs on the same split, both trained with `train.FlatLoop`:
  transductive   the held-out documents are in the graph (masked out of the loss), as the reference has them;
  fold-in        the graph is built WITHOUT them; afterwards `FoldIn(gcn, g).predict_text(t2g, held_out)` weights them with
                 the fitted vocabulary and idf (`Text2GraphTransformer.transform`) and runs one kernel launch.
The script reports both accuracies; it asserts neither.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.metrics import accuracy_score

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import FoldIn, Text2GraphTransformer, enable_fused_foldin, synth  # noqa: E402
from pytextgcn_amd.models import GCN  # noqa: E402
from pytextgcn_amd.train import FlatLoop  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=3000)
p.add_argument("--epochs", type=int, default=40)
p.add_argument("--relu", action="store_true", help="GCN(apply_activation=True)")
p.add_argument("--composed", action="store_true", help="enable_fused_foldin(False): the composition instead of the fused kernel")
args = p.parse_args()

seed, lr, min_df, dropout, window_size, n_hidden, n_classes = 44, 0.05, 5, 0.5, 20, 100, 6
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=n_classes, seed=seed)
y = np.asarray(y)
perm = np.random.permutation(len(docs))
n_hold = len(docs) // 10
held, val, rest = perm[:n_hold], perm[n_hold:2 * n_hold], perm[2 * n_hold:]
device = th.device("cuda")
if args.composed:
    enable_fused_foldin(False)


def train(corpus, labels, test_idx, val_idx):
    t2g = Text2GraphTransformer(n_jobs=8, min_df=min_df, window_size=window_size, rm_stopwords=False)
    g = t2g.fit_transform(corpus, labels, test_idx=test_idx, val_idx=val_idx).to(device)
    gcn = GCN(g.x.shape[1], n_classes, n_hidden_gcn=n_hidden, dropout=dropout, apply_activation=args.relu).to(device).float()
    with FlatLoop(gcn, g, lr=lr) as loop:
        for epoch in range(args.epochs):
            loss, val_loss, _, _ = loop.epoch()
    print(f"  graph {g}\n  {args.epochs} epochs: loss {float(loss):.3f}, val_loss {float(val_loss):.3f}")
    return t2g, g, gcn.eval()


print("transductive: the held-out documents are nodes of the graph")
_, g, gcn = train(docs, y.tolist(), held, val)
with th.no_grad():
    pred = gcn(g)[g.test_mask].argmax(dim=1).cpu().numpy()
acc_trans = accuracy_score(g.y[g.test_mask].cpu().numpy(), pred)

print("fold-in: the graph is built without them")
inside = np.concatenate([val, rest])                       # positions [0, n_hold) of this corpus are the validation documents
t2g, g, gcn = train([docs[i] for i in inside], y[inside].tolist(), None, np.arange(n_hold))
fold = FoldIn(gcn, g)
new_docs = [docs[i] for i in held]
th.cuda.synchronize()
t0 = time.time()
pred = fold.predict_text(t2g, new_docs).cpu().numpy()
dt = time.time() - t0
acc_fold = accuracy_score(y[held], pred)
tfidf = t2g.transform(new_docs)
print(f"  {len(new_docs)} new documents, {tfidf.nnz} known words, {int((np.diff(tfidf.indptr) == 0).sum())} without any; "
      f"transform + predict {dt * 1e3:.1f} ms ({'composed' if args.composed else 'fused'})")
print(f"transductive test accuracy: {acc_trans:.3f}  (held-out documents inside the graph)")
print(f"fold-in accuracy:           {acc_fold:.3f}  (the same documents outside the graph)")
