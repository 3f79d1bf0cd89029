#!/usr/bin/env python3
"""The EGCN half of one cell of old/h_o_hierarchical.py's sweep -- `models = [GCN, EGCN]` (:33,80) on `[I | H]` hierarchy
features, every dropout value x every learning rate x every fold of `KFold(3)` -- re-played on pytextgcn_amd as ONE
network (pytextgcn_amd.crossval.CrossValEGCN): the front ends of all members are one product with a seed and a rate per
member, and nothing crosses to the host inside an epoch (`score`, `metrics.Scoreboard`).  A synthetic corpus stands in for
the Amazon CSVs (.MISSING_LARGE_BLOBS:1-3).  Line references: old/h_o_hierarchical.py.

    python examples/crossval_egcn_synthetic.py [--docs 600] [--epochs 5]

Member `(d * len(lrs) + l) * k + f` has dropout `dos[d]`, learning rate `lrs[l]` and validates on fold f
(`crossval.grid_members`, `fold_bits(..., n_repeats=len(dos) * len(lrs))`).  H is the one-hot of the documents' top-level
label, held as class ids (`hier.HierarchyFeatures`).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.model_selection import KFold

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import Text2GraphTransformer, perlabel, synth  # noqa: E402
from pytextgcn_amd.crossval import CrossValEGCN, MemberAdam, fold_bits, grid_members  # noqa: E402
from pytextgcn_amd.metrics import Scoreboard  # noqa: E402
from pytextgcn_amd.perlevel import one_hot_hierarchy, with_hierarchy  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=600)
p.add_argument("--epochs", type=int, default=5)
p.add_argument("--hidden", type=int, default=32)
p.add_argument("--embedding-dim", type=int, default=200)
p.add_argument("--max-df", type=float, default=0.7)
args = p.parse_args()

seed, k_split, per_top = 44, 3, 2
dos, lrs = [0.5, 0.7], [0.01, 0.05]                                    # two values of each axis of the sweep
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=8, seed=seed)
y = np.asarray(y)
y_top = y // per_top                                                   # the level above: 4 top-level labels
test_idx = np.random.choice(len(docs), int(0.1 * len(docs)), replace=False)

t0 = time.time()
t2g = Text2GraphTransformer(n_jobs=8, min_df=5, verbose=1, max_df=args.max_df)
g = t2g.fit_transform(docs, y, test_idx=test_idx)                      # ONE graph for the whole grid
print(f"graph: {g}  ({time.time() - t0:.2f} s)")

doc_rows = th.nonzero(th.logical_or(g.train_mask, g.test_mask)).flatten().numpy()
folds = list(KFold(n_splits=k_split, shuffle=True, random_state=seed).split(doc_rows))
member_lrs, member_dos = grid_members(lrs, dos, k_split)
K = len(member_lrs)
train_bits, val_bits = fold_bits(doc_rows, folds, len(g.y), n_repeats=len(dos) * len(lrs))
n_classes = len(np.unique(y))

device = th.device("cuda")
g = g.to(device)
g = with_hierarchy(g, one_hot_hierarchy(g, y_top, n_classes=int(y_top.max()) + 1))         # x = [I | H], the same operator
pkg.enable_fused_dropout()                                             # each member's masks from its own seeds, in the products
perlabel.enable_fused_block_diag()
egcn = CrossValEGCN(g.x.shape[1], n_classes, K, embedding_dim=args.embedding_dim, n_hidden_gcn=args.hidden,
                    dropout=member_dos).to(device).float()             # :80, K models in one
egcn.train()
print(f"front end of {K} members as one product: {egcn.takes_fused_path(g.x)}")
train_bits, val_bits = train_bits.to(device), val_bits.to(device)
target = g.y.long()
optimizer = MemberAdam(egcn, member_lrs)                               # one rate per member

board = Scoreboard(args.epochs, K, ["loss", "val_loss", "train_accuracy", "val_f1"], device=device)
th.cuda.synchronize()
t0 = time.time()
for epoch in range(args.epochs):                                       # nothing crosses to the host
    egcn.train()
    loss, loss_k = egcn.loss(g, target, train_bits)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    val_loss_k, train_scores, val_scores = egcn.score(g, target, train_bits, val_bits)
    board.record(loss=loss_k, val_loss=val_loss_k, train_accuracy=train_scores.accuracy, val_f1=val_scores.f1_macro)
run = board.to_host()                                                  # the one synchronisation: [epochs, K, 4]
print(f"{args.epochs} epochs of {K} members in {time.time() - t0:.2f} s")

for k in range(K):
    print(f"member {k}: do {member_dos[k]:g} lr {member_lrs[k]:g} split {k % k_split}, first loss {run[0, k, 0]: .4f}, "
          f"final loss {run[-1, k, 0]: .4f}, val_f1 {run[-1, k, 3]: .3f}")

mean, std = board.fold_summary("val_f1", k_split, host=run)            # one row of the result table per cell
for d, do in enumerate(dos):
    for l, lr in enumerate(lrs):
        cell = d * len(lrs) + l
        print(f"LR {lr:g} DO {do:g} max_df {args.max_df:g} EGCN: mean f1 {mean[cell]:.3f} std f1 {std[cell]:.3f}")

members = egcn.export_members()
print(f"members: {len(members)} x EGCN({members[0].layers[0]!r}), dropout {sorted({m.dropout for m in members})}")
