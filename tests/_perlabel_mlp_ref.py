"""Restatements for the tests of the grouped MLP products (pytextgcn_amd/csrc/mlp_grouped.hip) and of `PerLabelMLP`: the
layout tables in Python, the float64 truth of a grouped call (tests/_mlp_ref.fused_truth per segment, side by side) and
the K-member network in any dtype.  Test infrastructure; nothing under pytextgcn_amd/ imports this."""
import math

import torch

import _mlp_ref as R

CHUNK = 128          # rows of a forward / dZ tile and of a chunk of the dW reduction
W_TARGET = 512       # workgroups of a dW launch, about (csrc/fused_act.h: grad_w_split)


def tables(row_ptr, k):
    """(tiles [(group, row0, count)], slices [(group, row0, row_end)], chunks per slice) as DESIGN.md 4.2g states them."""
    K = len(row_ptr) - 1
    tiles = [(g, r, min(CHUNK, row_ptr[g + 1] - r)) for g in range(K) for r in range(row_ptr[g], row_ptr[g + 1], CHUNK)]
    chunks = max(1, len(tiles))
    want = min(256, max(1, W_TARGET // ((k + 31) // 32)))
    cps = (chunks + want - 1) // want
    slices = [(g, r, min(r + cps * CHUNK, row_ptr[g + 1])) for g in range(K)
              for r in range(row_ptr[g], row_ptr[g + 1], cps * CHUNK)]
    return tiles, slices, cps


class Case:
    """One grouped call: operands on the CPU in float32 (Z ~ U(+-1), b ~ U(+-0.1), W glorot of the member, c ~ U(+-0.1),
    G ~ N(0, 1)), the description of the groups, and the float64 truth."""

    def __init__(self, row_ptr, N, k, n, col0, w_row0=None, seed=0):
        K = len(row_ptr) - 1
        self.row_ptr, self.N, self.k, self.K = list(row_ptr), N, k, K
        self.n, self.col0 = list(n), list(col0)
        if w_row0 is None:                                   # hidden style: stacked by rows; class style: at col0
            w_row0 = [sum(self.n[:g]) for g in range(K)] if all(c == 0 for c in col0) else list(col0)
        self.w_row0 = list(w_row0)
        self.b_off = [g * k for g in range(K)]
        self.w_rows = max(w + m for w, m in zip(self.w_row0, self.n))
        self.c_cols = max(c + m for c, m in zip(self.col0, self.n))
        gen = torch.Generator().manual_seed(1234 + seed)
        self.Z = torch.rand(N, k, generator=gen) * 2 - 1
        self.b = (torch.rand(K * k, generator=gen) * 2 - 1) * 0.1
        self.W = torch.zeros(self.w_rows, k)
        for g in range(K):
            a = math.sqrt(6.0 / (k + self.n[g]))
            self.W[self.w_row0[g]:self.w_row0[g] + self.n[g]] = (torch.rand(self.n[g], k, generator=gen) * 2 - 1) * a
        self.c = (torch.rand(self.c_cols, generator=gen) * 2 - 1) * 0.1
        self.G = torch.randn(N, self.c_cols, generator=gen)

    def members(self):
        """(g, r0, r1, W rows slice, b slice, C columns slice) of every group."""
        for g in range(self.K):
            yield (g, self.row_ptr[g], self.row_ptr[g + 1], slice(self.w_row0[g], self.w_row0[g] + self.n[g]),
                   slice(self.b_off[g], self.b_off[g] + self.k), slice(self.col0[g], self.col0[g] + self.n[g]))

    def truth(self, with_c=True, seed=None, p=0.0, mask_row0=0):
        """float64 (C, dZ, db, dW, dc, own): `fused_truth` per segment; C and dZ are zero and `own` (bool [N, c_cols]) False
        wherever the call writes nothing."""
        C = torch.zeros(self.N, self.c_cols, dtype=torch.float64)
        own = torch.zeros(self.N, self.c_cols, dtype=torch.bool)
        dZ = torch.zeros(self.N, self.k, dtype=torch.float64)
        db = torch.zeros(self.K * self.k, dtype=torch.float64)
        dW = torch.zeros(self.w_rows, self.k, dtype=torch.float64)
        dc = torch.zeros(self.c_cols, dtype=torch.float64)
        for g, r0, r1, wr, br, cr in self.members():
            if r0 == r1:
                continue
            keep = None if seed is None else R.keep_matrix(seed, r1 - r0, self.k, p, row0=mask_row0 + r0)
            out = R.fused_truth(self.Z[r0:r1], self.b[br], self.W[wr], self.c[cr] if with_c else None, self.G[r0:r1, cr],
                                keep, p)
            C[r0:r1, cr], dZ[r0:r1], db[br], dW[wr] = out[0], out[1], out[2], out[3]
            dc[cr] = self.G[r0:r1, cr].double().sum(0)
            own[r0:r1, cr] = True
        return C, dZ, db, dW, dc, own


def network_truth(model_params, class_counts, seg_start, hidden, xs, row_ptr, keeps=None, p=0.0):
    """Zcat [N, n_cols] of the K-member network from `_mlp_ref.mlp_truth` per member on its own rows.  `model_params`:
    [(weight, bias)] of PerLabelMLP's stacked layers as leaf tensors of one dtype; `xs` the dense [N, F] features in
    grouped order; keeps[i]: the [N, hidden[i]] keep matrix after layer i (None: no dropout)."""
    K, F, L = len(class_counts), xs.size(1), len(hidden)
    n_cols = model_params[-1][0].size(0)
    out = torch.zeros(xs.size(0), n_cols, dtype=xs.dtype)
    pieces = []
    for g in range(K):
        r0, r1 = row_ptr[g], row_ptr[g + 1]
        if r0 == r1:
            continue
        params = []
        for i, (W, b) in enumerate(model_params):
            if i == 0:
                params.append((W[:, g * F:(g + 1) * F], b[g * hidden[0]:(g + 1) * hidden[0]]))
            elif i < L:
                params.append((W[g * hidden[i]:(g + 1) * hidden[i]], b[g * hidden[i]:(g + 1) * hidden[i]]))
            else:
                s, c = seg_start[g], class_counts[g]
                params.append((W[s:s + c], b[s:s + c]))
        z = R.mlp_truth(params, xs[r0:r1], None if keeps is None else [kp[r0:r1] for kp in keeps], p)
        pieces.append((r0, r1, seg_start[g], class_counts[g], z))
    for r0, r1, s, c, z in pieces:
        out = out + torch.nn.functional.pad(z, (s, n_cols - s - c, r0, xs.size(0) - r1))
    return out


def grouped_ce(z, target, row_ptr, seg_start, class_counts):
    """sum_k CrossEntropyLoss('mean')(z[rows of k, segment k], target[rows of k]) over the non-empty groups."""
    total = 0.0
    for g in range(len(class_counts)):
        r0, r1 = row_ptr[g], row_ptr[g + 1]
        if r1 > r0:
            s, c = seg_start[g], class_counts[g]
            total = total + torch.nn.functional.cross_entropy(z[r0:r1, s:s + c], target[r0:r1])
    return total
