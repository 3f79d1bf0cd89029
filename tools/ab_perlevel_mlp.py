#!/usr/bin/env python3
"""Interleaved timing of MLP_level.py's level-2 (and DBpedia's level-3) `MLP` on `perlevel.AppendedFeatures` against the
same model on the sparse `torch.cat` composition (what `append_feats` builds, mlp_helper.py:141-151), in one process and on
one build.  Two arms per block set:

    appended   MLP on AppendedFeatures: X @ W1[:, :F].t() on X's own plan (the one the level-1 model built), the class
               columns as a per-row bias inside the first fused product (`mlp.act_linear_cls`)
    sparse     MLP on torch.cat([X, H], dim=1): a new sparse tensor with its own plan and transposed plan

Both use the package's fused loss and fused Adam, and enable_fused_dropout() is on.  Shape: MLP_flat.py's -- N documents x F
TF-IDF features with `nnz` non-zeros per row, hidden [256, 128], dropout 0.5 -- with blocks (6) and (9, 70).  Reported per
block set: the set-up time from the class ids until the first train step has finished (plans included; the level-1 model
has run on X before, as in the script), then, timed with HIP events after a warm-up round, the train step (forward, loss,
backward, optimizer step) and the eval forward over several rounds with the arms alternating, so that clock and temperature
drift hits both alike: the median and the spread max - min of the repetitions, and the peak memory a step allocates on top
of what is resident.  Before timing, the eval logits of the two arms are compared (faster and different is not faster).

    timeout 900 python tools/ab_perlevel_mlp.py [--docs 40000] [--features 50000] [--log profiles/r14_ab_perlevel_mlp.log]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402
from pytextgcn_amd.perlevel import append_classes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN = [256, 128]

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=40_000)
ap.add_argument("--features", type=int, default=50_000)
ap.add_argument("--nnz", type=int, default=60)
ap.add_argument("--classes", type=int, default=64)
ap.add_argument("--dropout", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r14_ab_perlevel_mlp.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
N, F = args.docs, args.features
log = open(args.log, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


say(f"ab_perlevel_mlp: {torch.cuda.get_device_name(0)}; N={N} F={F} nnz/row={args.nnz} hidden={HIDDEN} classes={args.classes} "
    f"dropout={args.dropout}; 1 warm-up round, then {args.rounds} rounds x {args.reps} timed repetitions, arms interleaved")
gen = torch.Generator().manual_seed(44)
pkg.enable_fused_dropout(True)
cols = torch.randint(0, F, (N, args.nnz), generator=gen)
idx = torch.stack([torch.arange(N).repeat_interleave(args.nnz), cols.reshape(-1)])
x = torch.sparse_coo_tensor(idx, torch.rand(N * args.nnz, generator=gen) + 0.1, (N, F)).coalesce().to(dev)
target = torch.randint(0, args.classes, (N,), generator=gen).to(dev)
every = torch.ones(N, dtype=torch.bool, device=dev)
level1 = pkg.MLP(F, 6, HIDDEN, dropout=args.dropout).to(dev).float().eval()
with torch.no_grad():
    level1(x)                                                # the level-1 model has run: X's plan exists
torch.cuda.synchronize()


def append_feats(ids_per_block, blocks):
    """mlp_helper.append_feats on the device, block after block: torch.cat of the features and the sparse one-hot block."""
    feats = x
    for ids, nb in zip(ids_per_block, blocks):
        rows = torch.arange(N, device=dev)
        mat = torch.sparse_coo_tensor(torch.stack([rows, ids]), torch.ones(N, device=dev), (N, nb))
        feats = torch.cat([feats, mat], dim=1)
    return feats.coalesce()


def appended(ids_per_block, blocks):
    a = x
    for ids, nb in zip(ids_per_block, blocks):
        a = append_classes(a, ids, nb)
    return a


class Arm:
    """One model on one form of the features; `first_step_s`: from the class ids to the end of the first train step."""

    def __init__(self, build, ids_per_block, blocks, state):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.x = build(ids_per_block, blocks)
        self.model = pkg.MLP(F + sum(blocks), args.classes, HIDDEN, dropout=args.dropout).to(dev).float()
        if state is not None:
            self.model.load_state_dict(state)
        self.opt = pkg.optim.Adam(self.model.parameters(), lr=0.05)
        self.train()
        torch.cuda.synchronize()
        self.first_step_s = time.perf_counter() - t0

    def train(self):
        self.model.train()
        loss = masked_cross_entropy(self.model(self.x), target, every)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()

    def eval(self):
        self.model.eval()
        with torch.no_grad():
            return self.model(self.x)


for blocks in ((6,), (9, 70)):
    say()
    say(f"blocks {blocks}: MLP({F} + {sum(blocks)}, {args.classes}, {HIDDEN})")
    ids_per_block = [torch.randint(0, nb, (N,), generator=gen).to(dev) for nb in blocks]
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in pkg.MLP(F + sum(blocks), args.classes, HIDDEN).state_dict().items()}
    plans = len(pkg.conv._FEATURE_PLANS)
    arms = {}
    for name, build in (("appended", appended), ("sparse", append_feats)):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        arms[name] = Arm(build, ids_per_block, blocks, state)
        torch.cuda.synchronize()
        say(f"  set-up until the first train step has finished, {name:8s}: {arms[name].first_step_s * 1e3:9.1f} ms; resident "
            f"afterwards {(torch.cuda.memory_allocated() - base) / 2 ** 20:8.1f} MiB; feature plans built "
            f"{len(pkg.conv._FEATURE_PLANS) - plans}")
        plans = len(pkg.conv._FEATURE_PLANS)
    # the same function: both arms from one state, one more eval forward each
    arms["sparse"].model.load_state_dict(arms["appended"].model.state_dict())
    za, zs = arms["appended"].eval(), arms["sparse"].eval()
    say(f"  eval logits, appended against sparse, max|a - b| / max|b|: {float((za - zs).abs().max() / zs.abs().max()):.2e}")
    cases = [(what, name, getattr(arms[name], fn)) for what, fn in (("train step", "train"), ("eval forward", "eval"))
             for name in ("appended", "sparse")]
    times = {(what, name): [] for what, name, _ in cases}
    peak = {}
    for rnd in range(args.rounds + 1):                       # round 0 = warm-up
        for what, name, fn in cases:
            fn()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record()
            for i in range(args.reps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            if rnd:
                times[(what, name)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
                peak[(what, name)] = max(peak.get((what, name), 0), torch.cuda.max_memory_allocated() - base)
    med, spread = {}, {}
    for (what, name), ts in times.items():
        m_, lo, hi = stats(ts)
        med[(what, name)], spread[(what, name)] = m_, hi - lo
        say(f"  {what:13s} {name:9s}  median {m_:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   spread (max - min) {hi - lo:7.3f} ms   "
            f"peak extra memory {peak[(what, name)] / 2 ** 20:8.1f} MiB")
    for what in ("train step", "eval forward"):
        a, b = med[(what, "appended")], med[(what, "sparse")]
        margin = spread[(what, "appended")] + spread[(what, "sparse")]
        verdict = "faster" if a < b - margin else ("slower" if a > b + margin else "no difference beyond the spreads")
        say(f"  {what}: appended / sparse = {a / b:.3f}  ({b / a:.2f} x); the medians differ by {abs(a - b):.3f} ms, the spreads "
            f"add up to {margin:.3f} ms: {verdict}")
    del arms
log.close()
