#!/usr/bin/env python3
"""Interleaved timing of the EGCN half of one cell of old/h_o_hierarchical.py's sweep (4 dropout values x KFold(3) = 12
two-layer EGCNs on one graph) in three forms, in one process:

    (a) one network   `CrossValEGCN`: the front ends of all members as ONE product (`tgcn_embed_xw_members`), one SpMM at
                      width M h, `member_masked_cross_entropy`, `MemberAdam` (`tgcn_adam_member_rows` on the stacked tensors)
    (b) composed      the same network with its front end composed from M single-member calls (`tgcn_embed_xw`, `_grad`) on
                      the members' rows -- everything else as (a): the difference is the member-batched kernel alone
    (c) sequential    12 `EGCN`s one after the other, each on the fused `masked_cross_entropy` and the fused `optim.Adam` --
                      what the sweep runs, on this package

Settings: M = 12, D = 2000, hidden width 100, 8 classes, dropout 0.5 under `enable_fused_dropout()` in every form.  Shapes:
config c2 of bench.py (100 000 nodes / 2 M edges) and a `synth` word-document graph of real-corpus size (60 000 nodes / 6 M
edges).  The train step (forward, loss, backward, optimizer step, all 12 members) and the eval forward with validation
losses and predictions (all 12) are timed with HIP events after a warm-up round; several rounds with the forms alternating,
so that clock and temperature drift hits all alike.  Reported: the median and the spread (max - min) of the repetitions, and
the peak memory a call allocates on top of what is live before it.  Verdict by the project's rule: a form is faster or
slower than another only if the medians differ by more than the SUM of the two spreads.  Before timing, the eval logits of
the network are compared with its members'.  The three forms hold their own parameters and Adam states: about 115 GB at c2.

    timeout 1200 python tools/ab_crossval_egcn.py [--shapes c2 corpus] [--rounds 5] [--reps 5] [--log profiles/r18_ab_crossval_egcn.log]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import _lib, embed, synth  # noqa: E402
from pytextgcn_amd.crossval import CrossValEGCN, MemberAdam, fold_bits  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402
from pytextgcn_amd.plan import _stream_ptr  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}
N_RATES, N_FOLDS, N_CLASSES = 4, 3, 8
LRS = [0.001, 0.005, 0.01, 0.05]

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--hidden", type=int, default=100)
ap.add_argument("--embedding-dim", type=int, default=2000)
ap.add_argument("--dropout", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r18_ab_crossval_egcn.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
M, h, D, C = N_RATES * N_FOLDS, args.hidden, args.embedding_dim, N_CLASSES
member_lrs = [lr for lr in LRS for _ in range(N_FOLDS)]
log = open(args.log, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def verdict(a, b):
    """(median, spread) of two forms -> what may be said about a against b"""
    if abs(a[0] - b[0]) <= a[1] + b[1]:
        return "no difference (the medians differ by less than the sum of the spreads)"
    return f"{'faster' if a[0] < b[0] else 'slower'} ({b[0] / a[0]:.2f} x)"


class _PerMemberXW(torch.autograd.Function):
    """The member product as M single-member calls (`tgcn_embed_xw`, `tgcn_embed_xw_grad`) that write into the members'
    blocks of ONE result and ONE gradient per parameter: what `embed.embed_xw_members` replaces, with nothing else added
    (no concatenation, no zero-filled gradient of a slice)."""

    @staticmethod
    def forward(ctx, E, b, W, n_members, rates, seeds):
        ctx.n_members, ctx.rates = n_members, rates
        ctx.save_for_backward(E, b, W, *([seeds] if seeds is not None else []))
        Dm, N, n = E.size(0) // n_members, E.size(1), W.size(1)
        out = torch.empty(N, n_members * n, dtype=torch.float32, device=E.device)
        for m in range(n_members):
            rows = slice(m * Dm, (m + 1) * Dm)
            seed = seeds[m:m + 1] if seeds is not None and rates[m] > 0 else None
            embed.embed_xw_forward(E.detach()[rows], b.detach()[rows], W.detach()[rows], rates[m], seed,
                                   out=out[:, m * n:(m + 1) * n])
        return out

    @staticmethod
    def backward(ctx, G):
        E, b, W = ctx.saved_tensors[:3]
        seeds = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        lib, K = _lib.load(), ctx.n_members
        Dm, N, n = E.size(0) // K, E.size(1), W.size(1)
        G = G if G.stride(1) == 1 else G.contiguous()
        dE, db, dW = torch.empty_like(E), torch.empty_like(b), torch.empty_like(W)
        ws = torch.empty(max(lib.tgcn_embed_xw_grad_workspace_bytes(N, Dm, n), 16), dtype=torch.uint8, device=E.device)
        stream = _stream_ptr(E.device)
        for m in range(K):
            r0 = m * Dm
            seed = seeds.data_ptr() + 8 * m if seeds is not None and ctx.rates[m] > 0 else None
            _lib.check(lib.tgcn_embed_xw_grad(E.data_ptr() + 4 * r0 * N, N, b.data_ptr() + 4 * r0, W.data_ptr() + 4 * r0 * n, n,
                                              G.data_ptr() + 4 * m * n, G.stride(0), dE.data_ptr() + 4 * r0 * N, N,
                                              db.data_ptr() + 4 * r0, dW.data_ptr() + 4 * r0 * n, n, N, Dm, n, ctx.rates[m],
                                              seed, 0, ws.data_ptr(), ws.numel(), stream))
        return dE, db, dW, None, None, None


class ComposedFrontEnd(CrossValEGCN):
    """form (b): M single-member calls on the members' rows in the place of the one member product"""

    def _front_end(self, x):
        emb, first = self.layers[0], self.layers[1]
        assert self.takes_fused_path(x) and x.size(0) == x.size(1)
        K = self.n_groups
        rates = self._rates() if self.training else (0.0,) * K
        seeds = torch.empty(K, dtype=torch.int64, device=emb.weight.device).random_() if max(rates) > 0 else None
        return _PerMemberXW.apply(emb.weight, emb.bias, first.weight, K, rates, seeds)


pkg.enable_fused_dropout()
say(f"ab_crossval_egcn: {torch.cuda.get_device_name(0)}; M={M} ({N_RATES} rates x {N_FOLDS} folds) D={D} hidden={h} "
    f"classes={C} dropout={args.dropout} (fused); 1 warm-up round, then {args.rounds} rounds x {args.reps} timed repetitions, "
    "forms interleaved")
for shape in args.shapes:
    N, E = SHAPES[shape]
    g = synth.word_doc_graph(N, E, seed=44, n_classes=C)
    doc_rows = np.arange(g.n_vocab, N)
    order = np.random.default_rng(44).permutation(doc_rows.size)
    train_bits, val_bits = fold_bits(doc_rows, [np.sort(order[f::N_FOLDS]) for f in range(N_FOLDS)], N, n_repeats=N_RATES)
    g = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(dev)
    train_bits, val_bits, target = train_bits.to(dev), val_bits.to(dev), g.y.long()
    train_masks = [((train_bits >> k) & 1).bool() for k in range(M)]
    val_masks = [((val_bits >> k) & 1).bool() for k in range(M)]
    torch.manual_seed(0)
    with torch.device(dev):                                 # 12 x [2000, N] weights: initialised where they live
        members = [pkg.EGCN(N, C, embedding_dim=D, n_hidden_gcn=h, dropout=args.dropout).float() for _ in range(M)]
    net = CrossValEGCN.from_members(members)
    net2 = ComposedFrontEnd.from_members(members)
    S = net.seg_stride
    opt_net, opt_net2 = MemberAdam(net, member_lrs), MemberAdam(net2, member_lrs)
    opt_members = [pkg.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(members, member_lrs)]

    with torch.no_grad():                                   # the same function, before anything is timed
        z, z2 = net.eval()(g), net2.eval()(g)
        worst = 0.0
        for k, m in enumerate(members):
            zk = m.eval()(g)
            worst = max(worst, float((z[:, k * S:k * S + C] - zk).abs().max() / zk.abs().max()))
        same = torch.equal(z, z2)
        del z, z2, zk
    say(f"{shape}: N={N} edges={E}; eval logits, the network against its members: max|a - b| / max|b| = {worst:.2e}; "
        f"(a) and (b) bit-equal: {same}")

    def train_of(n_, opt):
        def step():
            n_.train()
            loss, _ = n_.loss(g, target, train_bits)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return step

    def train_sequential():
        for m, opt, mask in zip(members, opt_members, train_masks):
            m.train()
            loss = masked_cross_entropy(m(g), target, mask)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

    def eval_sequential():
        with torch.no_grad():
            return [masked_cross_entropy(m.eval()(g), target, mask, return_pred=True) for m, mask in zip(members, val_masks)]

    cases = [("train step", "one network", train_of(net, opt_net)), ("train step", "composed", train_of(net2, opt_net2)),
             ("train step", "sequential", train_sequential),
             ("eval + pred", "one network", lambda: net.evaluate(g, target, val_bits)),
             ("eval + pred", "composed", lambda: net2.evaluate(g, target, val_bits)),
             ("eval + pred", "sequential", eval_sequential)]
    times = {(name, form): [] for name, form, _ in cases}
    peak = {}
    for rnd in range(args.rounds + 1):                      # round 0 = warm-up (plans, Adam states, allocator)
        for name, form, fn in cases:
            fn()
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record()
            for i in range(args.reps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            if rnd:
                times[(name, form)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
                peak[(name, form)] = max(peak.get((name, form), 0), torch.cuda.max_memory_allocated() - before)
    res = {}
    for (name, form), ts in times.items():
        ts = sorted(ts)
        res[(name, form)] = (ts[len(ts) // 2], ts[-1] - ts[0])
        say(f"  {name:12s} {form:12s} median {res[(name, form)][0]:9.3f} ms   min {ts[0]:9.3f}   max {ts[-1]:9.3f}   spread "
            f"(max - min) {ts[-1] - ts[0]:8.3f} ms   peak extra memory {peak[(name, form)] / 2 ** 20:9.1f} MiB")
    for name in ("train step", "eval + pred"):
        for other in ("composed", "sequential"):
            say(f"  {shape} {name}: one network against {other}: {verdict(res[(name, 'one network')], res[(name, other)])}")
    del net, net2, members, opt_net, opt_net2, opt_members, g, cases
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
log.close()
