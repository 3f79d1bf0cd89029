#!/usr/bin/env python3
"""MLP_label.py re-played on pytextgcn_amd: the top-level `MLP` (:44-96), then the K second-level classifiers as ONE network
(pytextgcn_amd.perlabel.PerLabelMLP) -- the loop of :104-150 written once for all top-level labels -- then every test
document routed to the member of its PREDICTED top label and its local arg-max mapped back to the global class (:157-162).
A synthetic corpus with a two-level label stands in for the Amazon CSVs (.MISSING_LARGE_BLOBS:1-3); the features are the
TF-IDF bag of words of mlp_helper.py.  Line references: MLP_label.py.

    python examples/perlabel_mlp_synthetic.py [--docs 5000] [--epochs 30]

The members train in lock step for `--epochs` epochs: the per-member early stopping of :138-144 is not rebuilt.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.feature_extraction.text import TfidfVectorizer
from sklearn.metrics import accuracy_score, f1_score

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import MLP, enable_fused_dropout, optim, synth  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402
from pytextgcn_amd.perlabel import GroupedRows, PerLabelMLP, column_class_map, relabel  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=5000)
p.add_argument("--epochs", type=int, default=30)
args = p.parse_args()

seed, lr, dropout, hidden = 44, 0.05, 0.7, [256, 128]                   # :11-19, :44
TOP_OF = np.array([0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 3, 3])                # Cat2 class -> Cat1 label: 3, 5, 2 and 2 children
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=len(TOP_OF), seed=seed)
y = np.asarray(y)
y_top = TOP_OF[y]
perm = np.random.permutation(len(docs))
n_test, n_val = len(docs) // 10, len(docs) // 10
test_idx, val_idx, train_idx = perm[:n_test], perm[n_test:n_test + n_val], perm[n_test + n_val:]

device = th.device("cuda")
enable_fused_dropout()                                                  # the masks come from the library's random stream


def to_torch(m):
    """mlp_helper.csr_to_torch: a scipy matrix as a sparse COO float tensor."""
    m = m.tocoo()
    return th.sparse_coo_tensor(np.stack([m.row, m.col]), m.data.astype(np.float32), m.shape).coalesce()


tfidf = TfidfVectorizer(min_df=2).fit([docs[i] for i in train_idx])
x_train, x_val, x_test = (to_torch(tfidf.transform([docs[i] for i in idx])).to(device) for idx in (train_idx, val_idx, test_idx))
print(f"x_train shape: {tuple(x_train.shape)}, x_val shape: {tuple(x_val.shape)}, x_test shape: {tuple(x_test.shape)}")

# ---- the first category (= flat), :44-96 -------------------------------------------------------------------------
model1 = MLP(x_train.shape[1], len(np.unique(y_top)), hidden, dropout=dropout).to(device).float()
optimizer = optim.Adam(model1.parameters(), lr=lr)
yt = th.from_numpy(y_top[train_idx]).to(device)
every = th.ones(len(train_idx), dtype=th.bool, device=device)
t0 = time.time()
for epoch in range(args.epochs):
    model1.train()
    loss = masked_cross_entropy(model1(x_train), yt, every)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
model1.eval()
with th.no_grad():
    top_val = model1(x_val).argmax(1).cpu().numpy()
    y_pred = model1(x_test).argmax(1).cpu().numpy()                    # :84-86, the labels that route the test documents
print(f"level 1: {args.epochs} epochs in {time.time() - t0:.2f} s, loss {loss.item():.3f}, "
      f"val accuracy {accuracy_score(y_top[val_idx], top_val):.3f}, test accuracy {accuracy_score(y_top[test_idx], y_pred):.3f}")

# ---- the second category, every top-level label at once, :100-150 ------------------------------------------------
# select_relabel_documents for every label: the documents of label k are relabelled 0..C_k-1 (one LabelEncoder per label)
sel = np.zeros(len(docs), dtype=bool)
sel[train_idx] = True
_, target_all, class_counts, mapping = relabel(y, y_top, sel)           # classes as the TRAINING documents of a label have them
K = len(class_counts)
print(f"{K} classifiers with {class_counts} classes")


def local_target(idx):
    """The LOCAL class of documents `idx` under their TRUE top label; -1 where the class was never seen in training."""
    out = np.full(len(idx), -1, dtype=np.int64)
    for i, d in enumerate(idx):
        classes = mapping[y_top[d]]
        if y[d] in classes:
            out[i] = classes.index(y[d])
    return th.from_numpy(out)


rows_train = GroupedRows(y_top[train_idx], K).to(device)                # the rows in grouped order, once per split
rows_val = GroupedRows(y_top[val_idx], K).to(device)
xg_train, xg_val = rows_train.features(x_train), rows_val.features(x_val)
t_train = rows_train.take(local_target(train_idx).to(device))
t_val = rows_val.take(local_target(val_idx).to(device))
val_mask = t_val >= 0

model2 = PerLabelMLP(x_train.shape[1], class_counts, hidden, dropout=dropout).to(device).float()     # :116, K models in one
optimizer = optim.Adam(model2.parameters(), lr=lr)
first_loss = None
th.cuda.synchronize()
t0 = time.time()
for epoch in range(args.epochs):                                        # :125-137
    model2.train()
    loss, loss_k = model2.loss(xg_train, rows_train, t_train)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    model2.eval()
    with th.no_grad():
        val_loss, _, pred_val = model2.loss(xg_val, rows_val, t_val, val_mask, return_pred=True)
    train_loss_k = loss_k.cpu().numpy()
    first_loss = train_loss_k if first_loss is None else first_loss
    if epoch % 10 == 0 or epoch == args.epochs - 1:
        local = (pred_val - th.tensor(model2.seg_start, device=device)[rows_val.group_sorted.clamp(min=0).long()])
        ok = val_mask.cpu().numpy()
        f1 = f1_score(t_val.cpu().numpy()[ok], local.cpu().numpy()[ok], average="macro")
        print(f"[{epoch + 1:3d}] loss: {loss.item(): .3f}, val_loss: {val_loss.item(): .3f}, val_f1 (local classes): {f1: .3f}")
th.cuda.synchronize()
print(f"level 2: {args.epochs} epochs in {time.time() - t0:.2f} s")
for k, c in enumerate(class_counts):
    print(f"group {k}: {c} classes, first loss {first_loss[k]: .4f}, final loss {train_loss_k[k]: .4f}")

# ---- prediction, :152-162: `mask = y_pred == label` for every label at once ----------------------------------------
rows_test = GroupedRows(y_pred, K).to(device)                           # routed by the PREDICTED top label
pred = model2.predict(rows_test.features(x_test), rows_test, class_map=column_class_map(mapping, device))
predictions = rows_test.restore(pred).cpu().numpy()                     # back in the order of the test documents
assert (predictions >= 0).all()
acc = accuracy_score(y[test_idx], predictions)
f1 = f1_score(y[test_idx], predictions, average="macro")
print(f"test accuracy: {acc:.3f}  test f1-macro: {f1:.3f}")

# the K ordinary MLP modules, as MLP_label.py trains them one by one
members = model2.export_members()
print("members: " + ", ".join(f"MLP(.., {m.layers[-1].out_features})" for m in members))
