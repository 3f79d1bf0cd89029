#!/usr/bin/env python3
"""Interleaved timing of one EPOCH of a sweep cell -- train step + evaluation + scores of all K members -- with the scores
taken in two ways, in one process:

    (a) host     as the examples do (examples/crossval_synthetic.py:77-84, the reference's old/h_o_train.py:116-122):
                 `CrossValGCN.evaluate`, the predictions [N, K] and both loss vectors copied to the host every epoch, then
                 `f1_score(average="macro")` on the validation rows and `accuracy_score` on the training rows, once per member
    (b) device   `CrossValGCN.score` + `metrics.Scoreboard.record`: nothing crosses to the host during the epochs; ONE
                 `Scoreboard.to_host()` after the last epoch of a block (its time is part of the block)

Settings: K = 12 (dropout 0.5) and K = 24 (dropouts 0.5, 0.7) x rates [0.001, 0.005, 0.01, 0.05] x 3 folds, hidden width 100,
8 classes, fused dropout and the one-launch layer-2 products on.  Shapes: config c2 of bench.py (100 000 nodes / 2 M edges)
and a `synth` word-document graph of real-corpus size (60 000 nodes / 6 M edges).  An epoch has host work in form (a), so
the clock is the host's: a block of `--reps` epochs between two synchronisations, divided by the number of epochs; one
warm-up round, then `--rounds` rounds with the two forms alternating.  Reported: the median and the spread (max - min) of
the rounds.  Verdict by the project's rule: faster or slower only if the medians differ by more than the SUM of the two
spreads.  Before timing, the scores of the two forms are compared.

    timeout 900 python tools/ab_scoreboard.py [--shapes c2 corpus] [--rounds 7] [--reps 5] [--log profiles/r17_ab_scoreboard.log]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch
from sklearn.metrics import accuracy_score, f1_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import perlabel, synth  # noqa: E402
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits, grid_members  # noqa: E402
from pytextgcn_amd.metrics import Scoreboard  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}
GRIDS = {12: [0.5], 24: [0.5, 0.7]}
LRS, N_FOLDS, N_CLASSES = [0.001, 0.005, 0.01, 0.05], 3, 8
COLUMNS = ["loss", "val_loss", "train_accuracy", "val_f1"]

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--members", nargs="+", type=int, default=[12, 24], choices=sorted(GRIDS))
ap.add_argument("--hidden", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r17_ab_scoreboard.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
h, C = args.hidden, N_CLASSES
log = open(args.log, "w")
warnings.filterwarnings("ignore")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def verdict(a, b):
    """(median, spread) of two forms -> what may be said about a against b"""
    if abs(a[0] - b[0]) <= a[1] + b[1]:
        return "no difference (the medians differ by less than the sum of the spreads)"
    return f"{'faster' if a[0] < b[0] else 'slower'} ({b[0] / a[0]:.2f} x)"


pkg.enable_fused_dropout()
perlabel.enable_fused_block_diag()
say(f"ab_scoreboard: {torch.cuda.get_device_name(0)}; hidden={h} classes={C} fused dropout and one-launch layer-2 products on; "
    f"one epoch = train step + evaluation + scores of all members; host clock over blocks of {args.reps} epochs; 1 warm-up "
    f"round, then {args.rounds} rounds, forms interleaved")
for shape in args.shapes:
    N, E = SHAPES[shape]
    gh = synth.word_doc_graph(N, E, seed=44, n_classes=C)
    doc_rows = np.arange(gh.n_vocab, N)
    order = np.random.default_rng(44).permutation(doc_rows.size)
    folds = [np.sort(order[f::N_FOLDS]) for f in range(N_FOLDS)]
    g = pkg.Data(**{k: getattr(gh, k) for k in gh.keys}).to(dev)
    target = g.y.long()
    y_host = gh.y.numpy()
    for K in args.members:
        dos = GRIDS[K]
        member_lrs, member_dos = grid_members(LRS, dos, N_FOLDS)
        bits = fold_bits(doc_rows, folds, N, n_repeats=len(dos) * len(LRS))
        train_rows, val_rows = ([((b.numpy() >> k) & 1).astype(bool) for k in range(K)] for b in bits)
        train_bits, val_bits = (b.to(dev) for b in bits)
        torch.manual_seed(0)
        members = [pkg.GCN(N, C, n_hidden_gcn=h, dropout=p).to(dev).float() for p in member_dos]
        nets = {form: CrossValGCN.from_members(members) for form in ("host", "device")}
        opts = {form: MemberAdam(n_, member_lrs) for form, n_ in nets.items()}
        del members

        def train_step(form):
            net, opt = nets[form], opts[form]
            net.train()
            loss, loss_k = net.loss(g, target, train_bits)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss_k

        def host_scores(net):
            val_loss_k, pred = net.evaluate(g, target, val_bits)
            pred, val_loss = pred.cpu().numpy(), val_loss_k.cpu().numpy()
            acc, f1 = np.zeros(K), np.zeros(K)
            for k in range(K):
                f1[k] = f1_score(y_host[val_rows[k]], pred[val_rows[k], k], average="macro")
                acc[k] = accuracy_score(y_host[train_rows[k]], pred[train_rows[k], k])
            return val_loss, acc, f1

        def block_host():
            rows = []
            for _ in range(args.reps):
                loss_k = train_step("host")
                val_loss, acc, f1 = host_scores(nets["host"])
                rows.append(np.stack([loss_k.cpu().numpy(), val_loss, acc, f1], 1))
            return np.stack(rows)

        def block_device():
            board = Scoreboard(args.reps, K, COLUMNS, device=dev)
            net = nets["device"]
            for _ in range(args.reps):
                loss_k = train_step("device")
                val_loss_k, tr, va = net.score(g, target, train_bits, val_bits)
                board.record(loss=loss_k, val_loss=val_loss_k, train_accuracy=tr.accuracy, val_f1=va.f1_macro)
            return board.to_host()

        # the same scores, before anything is timed: the device scores of net "device" against host scoring of ITS predictions
        _, tr, va = nets["device"].score(g, target, train_bits, val_bits)
        _, acc, f1 = host_scores(nets["device"])
        err = max(float(np.abs(tr.accuracy.cpu().numpy() - acc).max()), float(np.abs(va.f1_macro.cpu().numpy() - f1).max()))
        say(f"{shape} K={K}: N={N} edges={E}; device scores against sklearn on the same predictions: max abs difference {err:.1e}")

        forms = {"(a) host": block_host, "(b) device": block_device}
        times = {form: [] for form in forms}
        for rnd in range(args.rounds + 1):                  # round 0 = warm-up (plans, layouts, restricted operators, allocator)
            for form, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rnd:
                    times[form].append((time.perf_counter() - t0) * 1e3 / args.reps)
        res = {}
        for form, ts in times.items():
            ts = sorted(ts)
            res[form] = (ts[len(ts) // 2], ts[-1] - ts[0])
            say(f"  epoch K={K:2d} {form:11s} median {res[form][0]:9.3f} ms   min {ts[0]:9.3f}   max {ts[-1]:9.3f}   spread "
                f"(max - min) {ts[-1] - ts[0]:8.3f} ms")
        say(f"  {shape} K={K} epoch: (b) device against (a) host: {verdict(res['(b) device'], res['(a) host'])}")
        del nets, opts
    del g
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
log.close()
