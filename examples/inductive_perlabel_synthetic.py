#!/usr/bin/env python3
"""examples/perlabel_synthetic.py with a tenth of the corpus held OUT of the graph: the top-level GCN and the K per-label
classifiers (ONE `PerLabelGCN`) are trained on the graph of the other documents (perlabel_amazon.py:90-155), then
`FoldInPerLabel(...).predict_text` labels the held-out documents in one kernel launch -- the top model's arg-max routes a
document to that label's own classifier and the local arg-max is mapped back to the global class, as eval_perlabel.py:57-78
does for graph nodes.  The reference cannot do this: its test documents must be nodes of the graph.

    python examples/inductive_perlabel_synthetic.py [--docs 5000] [--epochs 50] [--composed]

The script reports the scores on the held-out documents; it asserts none.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch as th
from sklearn.metrics import accuracy_score, f1_score

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import GCN, FoldInPerLabel, Text2GraphTransformer, enable_fused_foldin, optim, synth  # noqa: E402
from pytextgcn_amd.perlabel import PerLabelGCN, relabel  # noqa: E402
from pytextgcn_amd.train import FlatLoop  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=5000)
p.add_argument("--epochs", type=int, default=50)
p.add_argument("--composed", action="store_true", help="enable_fused_foldin(False): the composition instead of the fused kernel")
args = p.parse_args()

seed, lr, dropout, n_hidden = 44, 0.05, 0.7, 100
TOP_OF = np.array([0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 3, 3])                # class -> top label: 3, 5, 2 and 2 children
np.random.seed(seed)
th.manual_seed(seed)
docs, y = synth.synthetic_corpus(args.docs, 3000, n_classes=len(TOP_OF), seed=seed)
y = np.asarray(y)
perm = np.random.permutation(len(docs))
n_hold = len(docs) // 10
held, inside = perm[:n_hold], perm[n_hold:]                            # the held-out tenth never enters the graph
docs_in, y_in = [docs[i] for i in inside], y[inside]
test_idx, val_idx = np.arange(n_hold), np.arange(n_hold, 2 * n_hold)
device = th.device("cuda")
if args.composed:
    enable_fused_foldin(False)

t2g = Text2GraphTransformer(n_jobs=8, min_df=5, window_size=20, rm_stopwords=False, max_df=0.7)
g_top = t2g.fit_transform(docs_in, TOP_OF[y_in], test_idx=test_idx, val_idx=val_idx).to(device)   # labelled with the top label
print(f"graph: {g_top}")

# the top model (eval_perlabel.py:57-58 loads it)
top = GCN(g_top.x.shape[1], int(TOP_OF.max()) + 1, n_hidden_gcn=n_hidden, dropout=dropout).to(device).float()
with FlatLoop(top, g_top, lr=lr) as loop:
    for epoch in range(args.epochs):
        loss, val_loss, _, _ = loop.epoch()
print(f"top model: {args.epochs} epochs, loss {float(loss):.3f}, val_loss {float(val_loss):.3f}")
top.eval()

# the K per-label classifiers on the same graph, as one network (perlabel_amazon.py:99-151)
N, V = g_top.num_nodes, int(g_top.n_vocab)
y_nodes, top_nodes = th.zeros(N, dtype=th.long), th.zeros(N, dtype=th.long)
y_nodes[V:], top_nodes[V:] = th.from_numpy(y_in), th.from_numpy(TOP_OF[y_in])
group, target, class_counts, mapping = relabel(y_nodes, top_nodes, th.arange(N) >= V)
group, target = group.to(device), target.to(device)
net = PerLabelGCN(g_top.x.shape[1], class_counts, n_hidden_gcn=n_hidden, dropout=dropout).to(device).float()
optimizer = optim.Adam(net.parameters(), lr=lr)
for epoch in range(args.epochs):
    net.train()
    loss, _ = net.loss(g_top, target, g_top.train_mask, group)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
print(f"{len(class_counts)} classifiers with {class_counts} classes: {args.epochs} epochs, loss {float(loss):.3f}")
net.eval()

# held-out documents: top label and class from ONE launch
fold = FoldInPerLabel(top, net, g_top, mapping)
new_docs = [docs[i] for i in held]
tfidf = t2g.transform(new_docs)
th.cuda.synchronize()
t0 = time.time()
both = fold.predict_levels(tfidf).cpu().numpy()
dt = time.time() - t0
print(f"  {len(new_docs)} new documents, {tfidf.nnz} known words, {int((np.diff(tfidf.indptr) == 0).sum())} without any; "
      f"predict {dt * 1e3:.1f} ms ({'composed' if args.composed else 'fused'})")
assert np.array_equal(fold.predict_text(t2g, new_docs).cpu().numpy(), both[:, 1])
by_truth = fold.predict(tfidf, route=th.from_numpy(TOP_OF[y[held]])).cpu().numpy()        # eval_perlabel.py:73 with a known label
print(f"held-out documents: top-label accuracy {accuracy_score(TOP_OF[y[held]], both[:, 0]):.3f}, routed accuracy "
      f"{accuracy_score(y[held], both[:, 1]):.3f}, macro-F1 {f1_score(y[held], both[:, 1], average='macro'):.3f}")
print(f"routed by the true top label: accuracy {accuracy_score(y[held], by_truth):.3f}")
