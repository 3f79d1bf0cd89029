#!/usr/bin/env python3
"""Interleaved timing of MLP's fused products against the composition they replace, in one process at the shape of the
reference's MLP_flat.py: hidden = [256, 128], dropout 0.5, a synthetic sparse TF-IDF-like matrix (about 40 000 documents x
50 000 terms, about 60 non-zeros per row) and 30 classes.  The train step (forward, loss, backward; fused dropout on, so
that the fused path is the one taken in training: it draws its masks from the library's hash, while the composition
draws torch's masks through its nn.Dropout) and the eval forward are timed with HIP events after a warm-up round;
several rounds with the variants alternating, so that clock and temperature drift hits both alike; reported are the
median and the spread (max - min) / median of the repetitions.  The composition is built from the package's other
kernels (`EmbeddingLinear` on `features_times` / `dense.xw`) plus torch's SELU and dropout: `enable_fused_mlp(False)`.
Also reports the peak extra memory of a train step for both in units of N x 256 x 4 B (`torch.cuda.max_memory_allocated`).

    timeout 600 python tools/ab_mlp.py [--docs 40000] [--vocab 50000] [--nnz-per-row 60] [--classes 30] [--rounds 6]
"""
import argparse
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytextgcn_amd as pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=40_000)
ap.add_argument("--vocab", type=int, default=50_000)
ap.add_argument("--nnz-per-row", type=int, default=60)
ap.add_argument("--classes", type=int, default=30)
ap.add_argument("--hidden", type=int, nargs="+", default=[256, 128])
ap.add_argument("--dropout", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda:0")
N, V, p = args.docs, args.vocab, args.dropout
gen = torch.Generator().manual_seed(44)
rows = torch.arange(N).repeat_interleave(args.nnz_per_row)
cols = (torch.rand(N * args.nnz_per_row, generator=gen) ** 2 * V).long().clamp_(max=V - 1)   # frequent terms are frequent
vals = torch.rand(N * args.nnz_per_row, generator=gen) * 0.3 + 0.02
x = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (N, V)).coalesce().to(dev)
y = torch.randint(0, args.classes, (N,), generator=gen).to(dev)
torch.manual_seed(0)
model = pkg.MLP(V, args.classes, args.hidden, dropout=p).to(dev).float()
crit = nn.CrossEntropyLoss()
pkg.enable_fused_dropout(True)


def train_step():
    model.train()
    model.zero_grad(set_to_none=True)
    crit(model(x), y).backward()


def eval_forward():
    model.eval()
    with torch.no_grad():
        model(x)


cases = [("train step", train_step, True), ("train step", train_step, False), ("eval forward", eval_forward, True),
         ("eval forward", eval_forward, False)]
times = {(name, fused): [] for name, _, fused in cases}
for rnd in range(args.rounds + 1):                       # round 0 = warm-up (plan build, allocator)
    for name, fn, fused in cases:
        was = pkg.enable_fused_mlp(fused)
        try:
            assert model.train().takes_fused_path(x) is fused
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record()
            for i in range(args.reps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
        finally:
            pkg.enable_fused_mlp(was)
        if rnd:
            times[(name, fused)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]

peak = {}
for fused in (True, False):
    was = pkg.enable_fused_mlp(fused)
    try:
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        train_step()
        torch.cuda.synchronize()
        peak[fused] = (torch.cuda.max_memory_allocated(), torch.cuda.max_memory_allocated() - base)
    finally:
        pkg.enable_fused_mlp(was)

print(f"ab_mlp: {torch.cuda.get_device_name(0)}; N={N} vocab={V} nnz={x._nnz()} classes={args.classes} hidden={args.hidden} "
      f"dropout={p}; 1 warm-up round, then {args.rounds} rounds x {args.reps} timed repetitions, variants interleaved")


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return med, ts[0], ts[-1], (ts[-1] - ts[0]) / med


med = {}
for (name, fused), ts in times.items():
    m, lo, hi, spread = stats(ts)
    med[(name, fused)] = m
    print(f"  {name:14s} {'fused      ' if fused else 'composition'}  median {m:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   "
          f"spread (max - min) / median {100 * spread:5.1f} %")
for name in ("train step", "eval forward"):
    f, c = med[(name, True)], med[(name, False)]
    print(f"  {name}: fused / composition = {f / c:.3f}  ({c / f:.2f} x)")
unit = N * 256 * 4
for fused in (True, False):
    print(f"  peak memory of a train step, {'fused      ' if fused else 'composition'}: max_memory_allocated "
          f"{peak[fused][0] / 2**20:9.1f} MiB, above the resting level {peak[fused][1] / 2**20:9.1f} MiB "
          f"= {peak[fused][1] / unit:.2f} x N 256 4 B")
print(f"  peak extra memory: fused / composition = {peak[True][1] / peak[False][1]:.3f}")
