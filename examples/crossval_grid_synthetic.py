#!/usr/bin/env python3
"""The whole grid of ONE graph of old/h_o_train.py's sweep -- one `max_df`, every dropout value x every learning rate x
every fold of `KFold(3)` -- re-played on pytextgcn_amd as ONE network (pytextgcn_amd.crossval.CrossValGCN with a dropout rate
per member): the loops of h_o_train.py:77-125 over `dos`, `lrs` and the folds are one training.  A synthetic corpus stands
in for the Amazon CSVs (.MISSING_LARGE_BLOBS:1-3).  Line references: old/h_o_train.py.

    python examples/crossval_grid_synthetic.py [--docs 600] [--epochs 5]

Member `(d * len(lrs) + l) * k + f` has dropout `dos[d]`, learning rate `lrs[l]` and validates on fold f
(`crossval.grid_members`, `fold_bits(..., n_repeats=len(dos) * len(lrs))`).  Only `max_df` stays an outer loop: it changes
the graph.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.metrics import f1_score
from sklearn.model_selection import KFold

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import Text2GraphTransformer, perlabel, synth  # noqa: E402
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits, grid_members  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=600)
p.add_argument("--epochs", type=int, default=5)
p.add_argument("--hidden", type=int, default=32)
p.add_argument("--max-df", type=float, default=0.7)
p.add_argument("--k-launch", action="store_true", help="keep the layer-2 products on the K-launch path")
args = p.parse_args()

seed, k_split = 44, 3                                                  # :19-37
dos, lrs = [0.5, 0.7], [0.01, 0.05]                                    # two values of each axis of :25-26
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=8, seed=seed)
y = np.asarray(y)
test_idx = np.random.choice(len(docs), int(0.1 * len(docs)), replace=False)                # :51

t0 = time.time()
t2g = Text2GraphTransformer(n_jobs=8, min_df=5, verbose=1, max_df=args.max_df)             # :67
g = t2g.fit_transform(docs, y, test_idx=test_idx)                      # :69 -- ONE graph for the whole grid
print(f"graph: {g}  ({time.time() - t0:.2f} s)")

doc_rows = th.nonzero(th.logical_or(g.train_mask, g.test_mask)).flatten().numpy()
folds = list(KFold(n_splits=k_split, shuffle=True, random_state=seed).split(doc_rows))
member_lrs, member_dos = grid_members(lrs, dos, k_split)
K = len(member_lrs)
train_bits, val_bits = fold_bits(doc_rows, folds, len(g.y), n_repeats=len(dos) * len(lrs))
n_classes = len(np.unique(y))

pkg.enable_fused_dropout()                                             # each member's mask from its own seed, in the product
perlabel.enable_fused_block_diag(not args.k_launch)                    # ... and one launch per product for all K members
gcn = CrossValGCN(g.x.shape[1], n_classes, K, n_hidden_gcn=args.hidden, dropout=member_dos)   # :90, K models in one
device = th.device("cuda")
gcn = gcn.to(device).float()
g = g.to(device)
train_bits, val_bits = train_bits.to(device), val_bits.to(device)
target = g.y.long()
optimizer = MemberAdam(gcn, member_lrs)                                # :98, one rate per member

y_host = g.y.cpu().numpy()
val_rows = [((val_bits >> k) & 1).bool().cpu().numpy() for k in range(K)]
first_loss, scores = None, np.zeros(K)
th.cuda.synchronize()
t0 = time.time()
for epoch in range(args.epochs):                                       # :106-124
    gcn.train()
    loss, loss_k = gcn.loss(g, target, train_bits)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    train_loss_k = loss_k.cpu().numpy()
    first_loss = train_loss_k if first_loss is None else first_loss
val_loss_k, pred = gcn.evaluate(g, target, val_bits)
pred = pred.cpu().numpy()
for k in range(K):                                                     # :116-122, on the host as in the reference
    scores[k] = f1_score(y_host[val_rows[k]], pred[val_rows[k], k], average="macro")
th.cuda.synchronize()
print(f"{args.epochs} epochs of {K} members in {time.time() - t0:.2f} s")
for k in range(K):
    print(f"member {k}: do {member_dos[k]:g} lr {member_lrs[k]:g} split {k % k_split}, first loss {first_loss[k]: .4f}, "
          f"final loss {train_loss_k[k]: .4f}")

# :125-131: one row of the result table per (dropout, learning rate) cell
for d, do in enumerate(dos):
    for l, lr in enumerate(lrs):
        at = (d * len(lrs) + l) * k_split
        s = scores[at:at + k_split]
        print(f"LR {lr:g} DO {do:g} max_df {args.max_df:g} GCN: mean f1 {s.mean():.3f} std f1 {s.std():.3f}")

members = gcn.export_members()
print(f"members: {len(members)} x {members[0].layers[1]!r}, dropout {sorted({m.dropout for m in members})}")
