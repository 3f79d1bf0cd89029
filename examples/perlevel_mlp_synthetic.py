#!/usr/bin/env python3
"""MLP_level.py re-played on pytextgcn_amd: the top-level `MLP` on the TF-IDF features (:48-103), then the second-level `MLP`
on the features with the one-hot top label appended (:105-178) -- the TRUE label for train and val (:120-121), the level-1
model's prediction for test (:85,122).  The script builds a new sparse tensor per split and per level on the host
(`append_feats`, OneHotEncoder, `.cpu()`); here the three feature tensors are uploaded once and the appended blocks are
class ids on the device (`pytextgcn_amd.perlevel.append_classes`), so the level-2 model runs on the plans that level 1
built.  A synthetic corpus with a two-level label stands in for the Amazon CSVs (.MISSING_LARGE_BLOBS:1-3).  Line
references: MLP_level.py.

    python examples/perlevel_mlp_synthetic.py [--docs 5000] [--epochs 30]
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
from pytextgcn_amd import MLP, conv, enable_fused_dropout, optim, synth  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402
from pytextgcn_amd.perlevel import append_classes, predicted_classes  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=5000)
p.add_argument("--epochs", type=int, default=30)
args = p.parse_args()

seed, lr, dropout, hidden = 42, 0.05, 0.7, [256, 128]                   # :18-21, :48
TOP_OF = np.array([0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 3, 3])                # Cat2 class -> Cat1 label
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=len(TOP_OF), seed=seed)
y = np.asarray(y)
levels = [TOP_OF[y], y]                                                 # y_train[0], y_train[1] of the script
n_classes = [int(lv.max()) + 1 for lv in levels]
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
# the one upload: everything below happens on the device
x_train, x_val, x_test = (to_torch(tfidf.transform([docs[i] for i in idx])).to(device) for idx in (train_idx, val_idx, test_idx))
print(f"x_train shape: {tuple(x_train.shape)}, x_val shape: {tuple(x_val.shape)}, x_test shape: {tuple(x_test.shape)}")


def labels(level, idx):
    return th.from_numpy(levels[level][idx]).to(device)


def train(model, x, yt, xv, yv, name):
    optimizer = optim.Adam(model.parameters(), lr=lr)                   # :63, :135
    every = th.ones(yt.numel(), dtype=th.bool, device=device)
    th.cuda.synchronize()
    t0 = time.time()
    for epoch in range(args.epochs):                                    # :69-76, :138-145
        model.train()
        loss = masked_cross_entropy(model(x), yt, every)
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        if epoch % 10 == 0 or epoch == args.epochs - 1:
            pred_val = predicted_classes(model, xv).cpu().numpy()
            f1 = f1_score(yv.cpu().numpy(), pred_val, average="macro")
            print(f"[{epoch + 1:3d}] loss: {loss.item(): .3f}, val_f1: {f1: .3f}")
    th.cuda.synchronize()
    print(f"{name}: {args.epochs} epochs in {time.time() - t0:.2f} s")


# ---- the first level, :48-103 ------------------------------------------------------------------------------------
model1 = MLP(x_train.shape[1], n_classes[0], hidden, dropout=dropout).to(device).float()
train(model1, x_train, labels(0, train_idx), x_val, labels(0, val_idx), "level 1")
y_pred = predicted_classes(model1, x_test)                              # :85, stays on the device
print(f"level 1 test accuracy: {accuracy_score(levels[0][test_idx], y_pred.cpu().numpy()):.3f}")
plans = len(conv._FEATURE_PLANS)

# ---- the second level, :105-178 ----------------------------------------------------------------------------------
x2_train = append_classes(x_train, labels(0, train_idx), n_classes[0])  # :120, the true labels
x2_val = append_classes(x_val, labels(0, val_idx), n_classes[0])        # :121
x2_test = append_classes(x_test, y_pred, n_classes[0])                  # :122, the predictions of the level above
print(f"x2_train shape: {tuple(x2_train.shape)} (the base tensor is x_train itself: {x2_train.base is x_train})")
model2 = MLP(x2_train.shape[1], n_classes[1], hidden, dropout=dropout).to(device).float()       # :124
train(model2, x2_train, labels(1, train_idx), x2_val, labels(1, val_idx), "level 2")
print(f"feature plans built for level 2: {len(conv._FEATURE_PLANS) - plans}")

pred_test = predicted_classes(model2, x2_test).cpu().numpy()            # :171
acc = accuracy_score(levels[1][test_idx], pred_test)
f1 = f1_score(levels[1][test_idx], pred_test, average="macro")
print(f"test accuracy: {acc:.3f}  test f1-macro: {f1:.3f}")
