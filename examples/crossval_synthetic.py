#!/usr/bin/env python3
"""One cell of old/h_o_train.py's sweep -- one `max_df`, one dropout value, every learning rate x every fold of `KFold(3)` --
re-played on pytextgcn_amd with its 12 two-layer GCNs trained as ONE network (pytextgcn_amd.crossval.CrossValGCN): the loop
of h_o_train.py:79-125 is written once for all learning rates and folds.  A synthetic corpus stands in for the Amazon CSVs
(.MISSING_LARGE_BLOBS:1-3).  Line references: old/h_o_train.py.

    python examples/crossval_synthetic.py [--docs 5000] [--epochs 50]

The members differ in their initial weights, their rows (the fold) and their learning rate; the dropout value and `max_df`
stay the sweep's outer loops (:66-78): run this once per pair.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.metrics import accuracy_score, f1_score
from sklearn.model_selection import KFold

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import Text2GraphTransformer, synth  # noqa: E402
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=5000)
p.add_argument("--epochs", type=int, default=50)
p.add_argument("--dropout", type=float, default=0.5)
p.add_argument("--max-df", type=float, default=0.7)
args = p.parse_args()

seed, k_split, n_hidden = 44, 3, 100                                   # :19-37
lrs = [0.001, 0.005, 0.01, 0.05]                                       # :26
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=8, seed=seed)
y = np.asarray(y)
test_idx = np.random.choice(len(docs), int(0.1 * len(docs)), replace=False)                # :51

t0 = time.time()
t2g = Text2GraphTransformer(n_jobs=8, min_df=5, verbose=1, max_df=args.max_df)             # :67
g = t2g.fit_transform(docs, y, test_idx=test_idx)                      # :69 -- ONE graph for the whole cell
print(f"graph: {g}  ({time.time() - t0:.2f} s)")

# :72-88 for every member at once: the sweep splits ALL documents (train and test mask alike) into k folds; member
# l * k + f trains on the complement of fold f at learning rate lrs[l] and validates on the fold
doc_rows = th.nonzero(th.logical_or(g.train_mask, g.test_mask)).flatten().numpy()
folds = list(KFold(n_splits=k_split, shuffle=True, random_state=seed).split(doc_rows))
train_bits, val_bits = fold_bits(doc_rows, folds, len(g.y), n_repeats=len(lrs))
K = k_split * len(lrs)
member_lrs = [lr for lr in lrs for _ in range(k_split)]
n_classes = len(np.unique(y))

gcn = CrossValGCN(g.x.shape[1], n_classes, K, n_hidden_gcn=n_hidden, dropout=args.dropout)  # :90, K models in one
device = th.device("cuda")
gcn = gcn.to(device).float()
g = g.to(device)
train_bits, val_bits = train_bits.to(device), val_bits.to(device)
target = g.y.long()
optimizer = MemberAdam(gcn, member_lrs)                                # :98, one rate per member

y_host = g.y.cpu().numpy()
sel = lambda bits, k: ((bits >> k) & 1).bool().cpu().numpy()
train_rows = [sel(train_bits, k) for k in range(K)]
val_rows = [sel(val_bits, k) for k in range(K)]
first_loss, scores = None, np.zeros(K)
length = len(str(args.epochs))
th.cuda.synchronize()
t0 = time.time()
for epoch in range(args.epochs):                                       # :106-124
    gcn.train()
    loss, loss_k = gcn.loss(g, target, train_bits)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    val_loss_k, pred = gcn.evaluate(g, target, val_bits)
    train_loss_k, val_loss_k, pred = loss_k.cpu().numpy(), val_loss_k.cpu().numpy(), pred.cpu().numpy()
    first_loss = train_loss_k if first_loss is None else first_loss
    for k in range(K):                                                 # :116-122, on the host as in the reference
        scores[k] = f1_score(y_host[val_rows[k]], pred[val_rows[k], k], average="macro")
        acc_train = accuracy_score(y_host[train_rows[k]], pred[train_rows[k], k])
        print(f"[{epoch + 1:{length}}] lr {member_lrs[k]:g} split {k % k_split}: loss: {train_loss_k[k]: .3f}, "
              f"val_loss: {val_loss_k[k]: .3f}, training accuracy: {acc_train: .3f}, val_f1: {scores[k]: .3f}")
th.cuda.synchronize()
print(f"{args.epochs} epochs of {K} members in {time.time() - t0:.2f} s")
for k in range(K):
    print(f"member {k}: lr {member_lrs[k]:g} split {k % k_split}, first loss {first_loss[k]: .4f}, final loss "
          f"{train_loss_k[k]: .4f}")

# :125-131: one row of the result table per learning rate
for l, lr in enumerate(lrs):
    s = scores[l * k_split:(l + 1) * k_split]
    print(f"LR {lr:g} DO {args.dropout:g} max_df {args.max_df:g} GCN: mean f1 {s.mean():.3f} std f1 {s.std():.3f}")

# the K ordinary GCN modules, ready for th.save
members = gcn.export_members()
print(f"members: {len(members)} x {members[0].layers[1]!r}")
