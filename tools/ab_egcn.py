#!/usr/bin/env python3
"""Interleaved timing of EGCN's fused front end against the composition it replaces, on one graph in one run: the train
step (forward, loss, backward; dropout 0.5, fused dropout on so that both draw their masks) and the eval forward, with
HIP events, a warm-up round and the median of the repetitions (several rounds, variants alternating, so that clock and
temperature drift hits both alike).  The composition is built from the package's other kernels (`dense.xw`,
`features_times`) plus torch's SELU and dropout: `enable_fused_embedding(False)`.  Also reports the peak memory of a train
step for both (`torch.cuda.max_memory_allocated`) and the forward product's achieved TFLOP/s.

    python tools/ab_egcn.py [--config c2] [--embedding-dim 2000] [--hidden 100] [--dropout 0.5] [--rounds 6] [--hierarchy FH]

`--hierarchy FH`: the features are [I_N | H] with one-hot rows of H (FH classes) on the document rows -- the second level
of a per-level run -- and the A/B is `enable_fused_hierarchy_embedding(True)` (`tgcn_embed_xw_h*`) against the composition.
"""
import argparse
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import conv, embed, synth  # noqa: E402

CONFIGS = {"c1": (5_000, 60_000, 6), "c2": (100_000, 2_000_000, 64)}      # nodes, edges, classes (BASELINE.json)

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=sorted(CONFIGS), default="c2")
ap.add_argument("--embedding-dim", type=int, default=2000)
ap.add_argument("--hidden", type=int, default=100)
ap.add_argument("--dropout", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--hierarchy", type=int, default=0, metavar="FH",
                help="[I | H] features: FH one-hot hierarchy columns on the document rows (0: identity features)")
args = ap.parse_args()

dev = torch.device("cuda:0")
N, n_edges, n_classes = CONFIGS[args.config]
K, h, p = args.embedding_dim, args.hidden, args.dropout
g0 = synth.word_doc_graph(N, n_edges, seed=44, n_classes=n_classes)
FH = args.hierarchy
HD, H_ROW0 = None, 0
if FH:
    V = max(2, int(N * 0.1))                              # synth.word_doc_graph: the words come first, then the documents
    docs = torch.arange(V, N)
    cls = torch.randint(0, FH, (N - V,), generator=torch.Generator().manual_seed(7))
    ar = torch.arange(N)
    g0.x = torch.sparse_coo_tensor(torch.cat([torch.stack([ar, ar]), torch.stack([docs, N + cls])], 1), torch.ones(2 * N - V),
                                   (N, N + FH)).coalesce()
g = pkg.Data(**{k: getattr(g0, k) for k in g0.keys}).to(dev)
torch.manual_seed(0)
model = pkg.EGCN(N + FH, n_classes, embedding_dim=K, n_hidden_gcn=h, dropout=p).to(dev).float()
crit = nn.CrossEntropyLoss()
pkg.enable_fused_dropout(True)
if FH:
    HD, H_ROW0 = conv.dense_hierarchy_block(conv.split_identity_block(g.x))
# the switch of the A/B: with [I | H] features the hierarchy switch (the master switch stays on), else the master switch
switch = pkg.enable_fused_hierarchy_embedding if FH else pkg.enable_fused_embedding


def train_step():
    model.train()
    model.zero_grad(set_to_none=True)
    crit(model(g)[g.train_mask], g.y[g.train_mask]).backward()


def eval_forward():
    model.eval()
    with torch.no_grad():
        model(g)


def product_forward():
    with torch.no_grad():
        embed.embed_xw_forward(model.layers[0].weight, model.layers[0].bias, model.layers[1].weight, h=HD, h_row0=H_ROW0)


def product_forward_dropout():
    with torch.no_grad():
        embed.embed_xw_forward(model.layers[0].weight, model.layers[0].bias, model.layers[1].weight, p, SEED, h=HD,
                               h_row0=H_ROW0)


SEED = torch.tensor([20240607], dtype=torch.int64, device=dev)
cases = [("train step", train_step, True), ("train step", train_step, False), ("eval forward", eval_forward, True),
         ("eval forward", eval_forward, False), ("forward product", product_forward, True),
         ("forward product + dropout", product_forward_dropout, True)]
times = {(name, fused): [] for name, _, fused in cases}
for rnd in range(args.rounds + 1):                       # round 0 = warm-up (plan build, allocator)
    for name, fn, fused in cases:
        was = switch(fused)
        try:
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record()
            for i in range(args.reps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
        finally:
            switch(was)
        if rnd:
            times[(name, fused)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]

peak = {}
for fused in (True, False):
    was = switch(fused)
    try:
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        train_step()
        torch.cuda.synchronize()
        peak[fused] = (torch.cuda.max_memory_allocated(), torch.cuda.max_memory_allocated() - base)
    finally:
        switch(was)

print(f"ab_egcn: {torch.cuda.get_device_name(0)}; config {args.config}: N={N} edges={n_edges} classes={n_classes}; "
      f"embedding_dim={K} hidden={h} dropout={p}; "
      + (f"[I | H] features, Fh={FH} one-hot on the {N - H_ROW0} document rows (h_row0={H_ROW0}); " if FH else "")
      + f"{args.rounds} rounds x {args.reps} repetitions, interleaved")


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return med, ts[0], ts[-1], (ts[-1] - ts[0]) / med


med = {}
for (name, fused), ts in times.items():
    m, lo, hi, spread = stats(ts)
    med[(name, fused)] = m
    print(f"  {name:26s} {'fused      ' if fused else 'composition'}  median {m:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   "
          f"spread (max - min) / median {100 * spread:5.1f} %")
for name in ("train step", "eval forward"):
    f, c = med[(name, True)], med[(name, False)]
    print(f"  {name}: fused / composition = {f / c:.3f}  ({c / f:.2f} x)")
flop = 2.0 * N * K * h
for name in ("forward product", "forward product + dropout"):
    print(f"  {name}: {flop / med[(name, True)] / 1e9:.1f} TFLOP/s (2 N K h = {flop / 1e9:.1f} GFLOP)")
unit = N * K * 4
for fused in (True, False):
    print(f"  peak memory of a train step, {'fused      ' if fused else 'composition'}: max_memory_allocated "
          f"{peak[fused][0] / 2**20:9.1f} MiB, above the resting level {peak[fused][1] / 2**20:9.1f} MiB "
          f"= {peak[fused][1] / unit:.2f} x N K 4 B")
