#!/usr/bin/env python3
"""Interleaved timing of MLP_label.py's second level as ONE grouped network (`PerLabelMLP`) against K sequential `MLP`s
(what MLP_label.py:104-162 runs, one model after the other), in one process and on one build.  Three arms:

    fused       PerLabelMLP on `mlp.grouped_act_linear` (one product per layer whatever K is)
    composed    the same network after enable_fused_mlp(False): a Python loop over the groups on row slices
    sequential  K `MLP`s, each on the documents of its label (the package's fused products, as `MLP` runs them)

All arms use the package's fused loss and fused Adam, and enable_fused_dropout() is on.  Shape: MLP_label.py's -- N
documents x F TF-IDF features with `nnz` non-zeros per row, hidden [256, 128], K = 6 labels with class counts
[10, 11, 11, 10, 11, 11], dropout 0.5; the test split is a tenth of N, routed by a random "predicted" label.  Timed with HIP
events after a warm-up round: the train step (forward, loss, backward, optimizer step, all K members), the eval forward and
the routed test prediction (global classes for every test document); several rounds with the arms alternating, so that
clock and temperature drift hits all alike; reported are the median and the spread max - min of the repetitions, and the
peak memory a train step allocates on top of what is resident.  Before timing, the grouped network is built from the K
members and its eval logits are compared with theirs (faster and different is not faster).

    timeout 900 python tools/ab_perlabel_mlp.py [--docs 40000] [--features 50000] [--log profiles/r13_ab_perlabel_mlp.log]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402
from pytextgcn_amd.perlabel import GroupedRows, PerLabelMLP, column_class_map  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [10, 11, 11, 10, 11, 11]
HIDDEN = [256, 128]

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=40_000)
ap.add_argument("--features", type=int, default=50_000)
ap.add_argument("--nnz", type=int, default=60)
ap.add_argument("--dropout", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r13_ab_perlabel_mlp.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
K, N, F = len(COUNTS), args.docs, args.features
log = open(args.log, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def features(n, gen):
    cols = torch.randint(0, F, (n, args.nnz), generator=gen)
    idx = torch.stack([torch.arange(n).repeat_interleave(args.nnz), cols.reshape(-1)])
    return torch.sparse_coo_tensor(idx, torch.rand(n * args.nnz, generator=gen) + 0.1, (n, F)).coalesce()


def rows_of(x, sel):
    """The rows `sel` (sorted indices) of a sparse COO matrix, as a sparse COO matrix (mlp_helper.csr_to_torch(csr[mask]))."""
    new = torch.full((x.size(0),), -1, dtype=torch.int64, device=x.device)
    new[sel] = torch.arange(sel.numel(), device=x.device)
    idx, val = x.indices(), x.values()
    keep = new[idx[0]] >= 0
    return torch.sparse_coo_tensor(torch.stack([new[idx[0]][keep], idx[1][keep]]), val[keep], (sel.numel(), F)).coalesce()


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


say(f"ab_perlabel_mlp: {torch.cuda.get_device_name(0)}; N={N} F={F} nnz/row={args.nnz} hidden={HIDDEN} K={K} class counts "
    f"{COUNTS} dropout={args.dropout}; 1 warm-up round, then {args.rounds} rounds x {args.reps} timed repetitions, arms interleaved")
gen = torch.Generator().manual_seed(44)
pkg.enable_fused_dropout(True)
x, x_test = features(N, gen).to(dev), features(N // 10, gen).to(dev)
group = torch.randint(0, K, (N,), generator=gen)
route = torch.randint(0, K, (N // 10,), generator=gen)                   # the "predicted" top label of a test document
target = (torch.rand(N, generator=gen) * torch.tensor(COUNTS)[group]).long()
class_map = [list(range(sum(COUNTS[:k]), sum(COUNTS[:k + 1]))) for k in range(K)]

torch.manual_seed(0)
members = [pkg.MLP(F, c, HIDDEN, dropout=args.dropout).to(dev).float() for c in COUNTS]
net = PerLabelMLP.from_members(members)
rows, rows_test = GroupedRows(group, K).to(dev), GroupedRows(route, K).to(dev)
xg, xg_test = rows.features(x), rows_test.features(x_test)
tg = rows.take(target.to(dev))
cmap = column_class_map(class_map, dev)
sel = [torch.nonzero(group == k).squeeze(1).to(dev) for k in range(K)]
sel_test = [torch.nonzero(route == k).squeeze(1).to(dev) for k in range(K)]
x_k = [rows_of(x, s) for s in sel]
x_test_k = [rows_of(x_test, s) for s in sel_test]
t_k = [target.to(dev)[s] for s in sel]
every = [torch.ones(s.numel(), dtype=torch.bool, device=dev) for s in sel]
maps = [torch.tensor(m, device=dev) for m in class_map]
opt_net = pkg.optim.Adam(net.parameters(), lr=0.05)
opt_members = [pkg.optim.Adam(m.parameters(), lr=0.05) for m in members]

with torch.no_grad():                                        # the same function, before anything is timed
    z = net.eval()(xg, rows)
    pkg.enable_fused_mlp(False)
    zc = net(xg, rows)
    pkg.enable_fused_mlp(True)
    worst = worst_c = 0.0
    for k, (m, s, c) in enumerate(zip(members, net.seg_start, net.seg_width)):
        zk = m.eval()(x_k[k])
        r0, r1 = rows.row_ptr[k], rows.row_ptr[k + 1]
        worst = max(worst, float((z[r0:r1, s:s + c] - zk).abs().max() / zk.abs().max()))
        worst_c = max(worst_c, float((zc[r0:r1, s:s + c] - zk).abs().max() / zk.abs().max()))
say(f"eval logits against the members, max|a - b| / max|b|: fused {worst:.2e}, composed {worst_c:.2e}")


def train_grouped():
    net.train()
    loss, _ = net.loss(xg, rows, tg)
    opt_net.zero_grad(set_to_none=True)
    loss.backward()
    opt_net.step()


def train_sequential():
    for m, opt, xk, tk, ek in zip(members, opt_members, x_k, t_k, every):
        m.train()
        loss = masked_cross_entropy(m(xk), tk, ek)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()


def eval_grouped():
    net.eval()
    with torch.no_grad():
        net(xg, rows)


def eval_sequential():
    with torch.no_grad():
        for m, xk in zip(members, x_k):
            m.eval()(xk)


def predict_grouped():
    net.eval()
    return rows_test.restore(net.predict(xg_test, rows_test, class_map=cmap))


def predict_sequential():
    out = torch.full((N // 10,), -1, dtype=torch.int64, device=dev)
    with torch.no_grad():
        for m, xk, s, mp in zip(members, x_test_k, sel_test, maps):
            out[s] = mp[m.eval()(xk).argmax(1)]               # MLP_label.py:157-162
    return out


def composed(fn):
    def run():
        was = pkg.enable_fused_mlp(False)
        try:
            return fn()
        finally:
            pkg.enable_fused_mlp(was)
    return run


same = bool(torch.equal(predict_grouped(), predict_sequential()))
say(f"routed test predictions, grouped == sequential: {same}")
cases = [("train step", "fused", train_grouped), ("train step", "composed", composed(train_grouped)),
         ("train step", "sequential", train_sequential),
         ("eval forward", "fused", eval_grouped), ("eval forward", "composed", composed(eval_grouped)),
         ("eval forward", "sequential", eval_sequential),
         ("test prediction", "fused", predict_grouped), ("test prediction", "composed", composed(predict_grouped)),
         ("test prediction", "sequential", predict_sequential)]
times = {(name, arm): [] for name, arm, _ in cases}
peak = {}
for rnd in range(args.rounds + 1):                          # round 0 = warm-up (feature plans, layouts, allocator)
    for name, arm, fn in cases:
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
            times[(name, arm)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
            peak[(name, arm)] = max(peak.get((name, arm), 0), torch.cuda.max_memory_allocated() - base)
med, spread = {}, {}
for (name, arm), ts in times.items():
    m_, lo, hi = stats(ts)
    med[(name, arm)], spread[(name, arm)] = m_, hi - lo
    say(f"  {name:16s} {arm:10s}  median {m_:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   spread (max - min) {hi - lo:7.3f} ms   "
        f"peak extra memory {peak[(name, arm)] / 2 ** 20:8.1f} MiB")
for name in ("train step", "eval forward", "test prediction"):
    b = med[(name, "sequential")]
    for arm in ("fused", "composed"):
        a = med[(name, arm)]
        margin = spread[(name, arm)] + spread[(name, "sequential")]
        verdict = "faster" if a < b - margin else ("slower" if a > b + margin else "no difference beyond the spreads")
        say(f"  {name}: {arm} / sequential = {a / b:.3f}  ({b / a:.2f} x); the medians differ by {abs(a - b):.3f} ms, the "
            f"spreads add up to {margin:.3f} ms: {verdict}")
log.close()
