#!/usr/bin/env python3
"""perlabel_amazon.py + eval_perlabel.py re-played on pytextgcn_amd, with the K per-label classifiers as ONE network
(pytextgcn_amd.perlabel.PerLabelGCN): the loop of perlabel_amazon.py:134-151 is written once for all top-level labels, then
every test document is routed to the member of its top label and its local arg-max mapped back to the global class
(eval_perlabel.py:71-82).  A synthetic corpus with a two-level label stands in for the Amazon CSVs
(.MISSING_LARGE_BLOBS:1-3).  Line references: perlabel_amazon.py unless eval_perlabel.py is named.

    python examples/perlabel_synthetic.py [--docs 5000] [--epochs 50]

The top label that routes a test document is its TRUE one here (eval_perlabel.py:58,73 takes the level-1 model's prediction:
train `examples/flat_synthetic.py` on `y_top` for that); routing by a prediction only changes the `route` tensor.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.metrics import accuracy_score, f1_score

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import Text2GraphTransformer, optim, synth  # noqa: E402
from pytextgcn_amd.perlabel import PerLabelGCN, column_class_map, relabel  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=5000)
p.add_argument("--epochs", type=int, default=50)
args = p.parse_args()

seed, lr, dropout, n_hidden = 44, 0.05, 0.7, 100                       # :22-40 (lr of the flat script: 30 epochs suffice)
TOP_OF = np.array([0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 3, 3])                # Cat2 class -> Cat1 label: 3, 5, 2 and 2 children
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=len(TOP_OF), seed=seed)
y = np.asarray(y)
y_top = TOP_OF[y]                                                      # :44-46,68-69
perm = np.random.permutation(len(docs))
test_idx, val_idx = perm[:len(docs) // 10], perm[len(docs) // 10:len(docs) // 5]

t0 = time.time()
t2g = Text2GraphTransformer(n_jobs=8, min_df=5, window_size=20, rm_stopwords=False, verbose=1, max_df=0.7)
g = t2g.fit_transform(docs, y, test_idx=test_idx, val_idx=val_idx)     # :95 -- ONE graph for all classifiers
print(f"graph: {g}  ({time.time() - t0:.2f} s)")

# :99-110 for every classifier at once: the documents of label k are relabelled 0..C_k-1, everything else is -1
is_doc = th.arange(len(g.y)) >= g.n_vocab
top_nodes = th.zeros(len(g.y), dtype=th.long)
top_nodes[g.n_vocab:] = th.from_numpy(y_top)
group, target, class_counts, mapping = relabel(g.y, top_nodes, is_doc)
print(f"{len(class_counts)} classifiers with {class_counts} classes")

gcn = PerLabelGCN(g.x.shape[1], class_counts, n_hidden_gcn=n_hidden, dropout=dropout)      # :113, K models in one
device = th.device("cuda")
gcn = gcn.to(device).float()
g = g.to(device)
group, target = group.to(device), target.to(device)
class_map = column_class_map(mapping, device)
optimizer = optim.Adam(gcn.parameters(), lr=lr)                        # :124 (the package's fused Adam)

# `logical_and(g.train_mask, mask)` of :130-132 needs no mask per classifier: the loss reads row r in the segment of group[r]
y_local = target.cpu()
first_loss = None
th.cuda.synchronize()
t0 = time.time()
for epoch in range(args.epochs):                                       # :134-151
    gcn.train()
    loss, loss_k = gcn.loss(g, target, g.train_mask, group)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    gcn.eval()
    with th.no_grad():
        val_loss, val_loss_k, pred = gcn.loss(g, target, g.val_mask, group, return_pred=True)
    train_loss_k = loss_k.cpu().numpy()
    first_loss = train_loss_k if first_loss is None else first_loss
    if epoch % 10 == 0 or epoch == args.epochs - 1:
        # per classifier, in its own local classes, as :145-148 computes them one model at a time
        local = (pred - th.tensor(gcn.seg_start, device=device)[group.clamp(min=0).long()]).cpu()
        parts = []
        for k in range(len(class_counts)):
            tr, va = (g.train_mask & (group == k)).cpu(), (g.val_mask & (group == k)).cpu()
            parts.append(f"{k}: acc {accuracy_score(y_local[tr], local[tr]):.3f} val_f1 "
                         f"{f1_score(y_local[va], local[va], average='macro'):.3f}")
        print(f"[{epoch + 1:3d}] loss: {loss.item(): .3f}, val_loss: {val_loss.item(): .3f} | " + " | ".join(parts))
th.cuda.synchronize()
print(f"{args.epochs} epochs in {time.time() - t0:.2f} s")
for k, c in enumerate(class_counts):
    print(f"group {k}: {c} classes, first loss {first_loss[k]: .4f}, final loss {train_loss_k[k]: .4f}")

# eval_perlabel.py:65-82: route every test document to the member of its top label, map the arg-max back to the global class
predictions = gcn.predict(g, route=group, class_map=class_map).cpu().numpy()
test = g.test_mask.cpu().numpy()
y_true = g.y.cpu().numpy()
assert (predictions[test] >= 0).all()
acc = accuracy_score(y_true[test], predictions[test])
f1 = f1_score(y_true[test], predictions[test], average="macro")
print(f"test accuracy: {acc:.3f}  test f1-macro: {f1:.3f}")

# :154 / eval_perlabel.py:16-19: the K ordinary GCN modules, ready for th.save(member, f"lvl2-cat{k}")
members = gcn.export_members()
print("members: " + ", ".join(repr(m.layers[1]) for m in members))
