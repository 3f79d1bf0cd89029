#!/usr/bin/env python3
"""examples/crossval_grid_synthetic.py's grid -- one `max_df`, every dropout value x every learning rate x every fold of
`KFold(3)` of old/h_o_train.py's sweep as ONE network -- with the scores of every epoch taken on the DEVICE: the reference
copies the predictions to the host every epoch and calls `f1_score` / `accuracy_score` once per member (:116-122); here
`CrossValGCN.score` leaves the training accuracy and the validation macro-F1 of all members in a
`pytextgcn_amd.metrics.Scoreboard`, and ONE `Scoreboard.to_host()` after the last epoch brings the whole run back.  The
per-epoch lines and the result table are the reference's.  Line references: old/h_o_train.py.

    python examples/crossval_scoreboard_synthetic.py [--docs 600] [--epochs 5] [--dump run.npz]

`--dump` writes the final predictions, labels, validation rows and the final F1 per member (what the test compares with
sklearn's).
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
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits, grid_members  # noqa: E402
from pytextgcn_amd.metrics import Scoreboard  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=600)
p.add_argument("--epochs", type=int, default=5)
p.add_argument("--hidden", type=int, default=32)
p.add_argument("--max-df", type=float, default=0.7)
p.add_argument("--dump", default=None, help="write the final predictions and scores to this .npz")
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

pkg.enable_fused_dropout()
perlabel.enable_fused_block_diag()
gcn = CrossValGCN(g.x.shape[1], n_classes, K, n_hidden_gcn=args.hidden, dropout=member_dos)   # :90, K models in one
device = th.device("cuda")
gcn = gcn.to(device).float()
g = g.to(device)
train_bits, val_bits = train_bits.to(device), val_bits.to(device)
target = g.y.long()
optimizer = MemberAdam(gcn, member_lrs)                                # :98, one rate per member

board = Scoreboard(args.epochs, K, ["loss", "val_loss", "train_accuracy", "val_f1"], device=device)
th.cuda.synchronize()
t0 = time.time()
for epoch in range(args.epochs):                                       # :106-124, nothing crosses to the host
    gcn.train()
    loss, loss_k = gcn.loss(g, target, train_bits)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    val_loss_k, train_scores, val_scores = gcn.score(g, target, train_bits, val_bits)
    board.record(loss=loss_k, val_loss=val_loss_k, train_accuracy=train_scores.accuracy, val_f1=val_scores.f1_macro)
run = board.to_host()                                                  # the one synchronisation: [epochs, K, 4]
print(f"{args.epochs} epochs of {K} members in {time.time() - t0:.2f} s")

length = len(str(args.epochs))
for epoch in range(args.epochs):                                       # :116-122, the reference's lines
    for k in range(K):
        l, vl, acc, f1 = run[epoch, k]
        print(f"[{epoch + 1:{length}}] do {member_dos[k]:g} lr {member_lrs[k]:g} split {k % k_split}: loss: {l: .3f}, "
              f"val_loss: {vl: .3f}, training accuracy: {acc: .3f}, val_f1: {f1: .3f}")
for k in range(K):
    print(f"member {k}: do {member_dos[k]:g} lr {member_lrs[k]:g} split {k % k_split}, first loss {run[0, k, 0]: .4f}, "
          f"final loss {run[-1, k, 0]: .4f}")

# :125-131: one row of the result table per (dropout, learning rate) cell
mean, std = board.fold_summary("val_f1", k_split, host=run)
for d, do in enumerate(dos):
    for l, lr in enumerate(lrs):
        cell = d * len(lrs) + l
        print(f"LR {lr:g} DO {do:g} max_df {args.max_df:g} GCN: mean f1 {mean[cell]:.3f} std f1 {std[cell]:.3f}")

if args.dump:
    _, pred = gcn.evaluate(g, target, val_bits)                        # the weights the last epoch scored
    np.savez(args.dump, pred=pred.cpu().numpy(), y=g.y.cpu().numpy(), val_bits=val_bits.cpu().numpy(),
             val_f1=run[-1, :, 3], train_accuracy=run[-1, :, 2], train_bits=train_bits.cpu().numpy())
