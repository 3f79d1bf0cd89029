"""The per-label strategy of the reference (perlabel_amazon.py, eval_perlabel.py) as ONE network.

perlabel_amazon.py:90-155 builds the same graph once per top-level label k and trains one two-layer `GCN` on it per
label: the masks are restricted to that label's documents (:130-132), their classes relabelled to 0..C_k-1 (:104-109), the
model saved as `lvl2-cat{k}` next to a JSON `mapping` (:154-160).  eval_perlabel.py:71-78 routes every test document to the
model of its (predicted) top label and maps the local argmax back through `mapping`.

The K classifiers share the operator M, the features and the optimiser settings; their parameters are disjoint, the loss
is a sum of K terms and Adam is element-wise.  So the K trainings are, in exact arithmetic, one training of

    H1cat = M [W1_1 | ... | W1_K] + [b1_1 | ... | b1_K]                         one SpMM at width K h
    Zcat  = M (dropout(H1cat) blockdiag(W2_1 ... W2_K)) + [b2_1 | ... | b2_K]   one SpMM at width sum C_k
    loss  = sum_k CE_mean(Zcat[rows of group k, segment k], local labels)       functional.grouped_masked_cross_entropy

`PerLabelGCN` is that network, `relabel` the per-group LabelEncoder, `from_members` / `export_members` the bridge to the K
ordinary `GCN` modules the reference's scripts save and load.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor, nn

from . import dense, functional, models
from .conv import GCNConv, propagate
from .plan import _require_cuda, note_colsum


def relabel(y_nodes, top_nodes, select):
    """The per-group LabelEncoder of perlabel_amazon.py:104-109, for all groups at once (host).

    `y_nodes` [N]: the global class of every node, `top_nodes` [N]: its top-level label in 0..K-1 (the script's `y_top`
    after its own LabelEncoder, :68), `select` [N] bool: the nodes that carry labels (the documents).  Returns

        group        int32 [N]   `top_nodes` on the selected nodes, -1 elsewhere
        target       int64 [N]   the class re-numbered inside its group in ascending order, -1 elsewhere (`g.y[:] = -1`)
        class_counts [K]         distinct classes per group
        class_map    K lists     per group the sorted distinct global labels: what `mapping[k]` holds (:107)

    Every one of the K = max(top) + 1 groups must hold a selected node (the script would construct a model with no class)."""
    y = np.asarray(torch.as_tensor(y_nodes).cpu()).astype(np.int64).ravel()
    top = np.asarray(torch.as_tensor(top_nodes).cpu()).astype(np.int64).ravel()
    sel = np.asarray(torch.as_tensor(select).cpu()).astype(bool).ravel()
    if not (y.shape == top.shape == sel.shape):
        raise ValueError("y_nodes, top_nodes and select must have one entry per node")
    if not sel.any() or top[sel].min() < 0:
        raise ValueError("relabel: no selected node, or a negative top-level label on one")
    K = int(top[sel].max()) + 1
    group = np.where(sel, top, -1).astype(np.int32)
    target = np.full(y.shape, -1, dtype=np.int64)
    class_counts, class_map = [], []
    for k in range(K):
        rows = np.nonzero(group == k)[0]
        if rows.size == 0:
            raise ValueError(f"relabel: top-level label {k} has no selected node")
        classes, local = np.unique(y[rows], return_inverse=True)
        target[rows] = local
        class_counts.append(int(classes.size))
        class_map.append(classes.tolist())
    return torch.from_numpy(group), torch.from_numpy(target), class_counts, class_map


def segment_layout(class_counts: Sequence[int]):
    """(starts, n_cols) of the concatenated class axis: segment k begins at a multiple of 4 columns (16-byte rows for every
    slice product), so `sum round_up(C_k, 4)` columns in all; the pad columns behind a segment belong to nobody."""
    starts, at = [], 0
    for c in class_counts:
        if int(c) < 1:
            raise ValueError("every group needs at least one class")
        starts.append(at)
        at += (int(c) + 3) & ~3
    return starts, at


def column_class_map(class_map: Sequence[Sequence[int]], device=None) -> Tensor:
    """`relabel`'s per-group lists as the kernel takes them: int64 [n_cols], column -> global class, -1 in pad columns."""
    starts, n_cols = segment_layout([len(m) for m in class_map])
    out = torch.full((n_cols,), -1, dtype=torch.int64)
    for s, m in zip(starts, class_map):
        out[s:s + len(m)] = torch.as_tensor(list(m), dtype=torch.int64)
    return out if device is None else out.to(device)


class _BlockDiagXW(torch.autograd.Function):
    """Hcat [N, K h] times blockdiag(W_1 .. W_K), the W_k [h, C_k] stored side by side as column segments of `w`
    [h, n_cols]: K launches of the package's tall-skinny products on column slices, writing into ONE result buffer, ONE
    dHcat and ONE dW (no torch.cat, no zero tensor at the hidden width).  With `seeds` (int64 [K]) product k is
    `dense.xw_dropout(Hcat[:, slice k], W_k, p, seeds[k])`: the same kernels, the same hash, the same bits."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, starts, widths, p: float, seeds: Optional[Tensor]):
        K, h = len(starts), w.size(0)
        N = x.size(0)
        xd, wd = x.detach(), w.detach()
        out = torch.zeros(N, w.size(1), dtype=torch.float32, device=x.device)       # class width; pad columns stay zero
        want_mask = seeds is not None and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        masks = []
        for k, (s, c) in enumerate(zip(starts, widths)):
            a, b, o = xd[:, k * h:(k + 1) * h], wd[:, s:s + c], out[:, s:s + c]
            if seeds is None:
                dense.gemm_nn(a, b, out=o)
            elif want_mask:
                masks.append(dense.gemm_nn(a, b, p, seeds[k:k + 1], record_mask=True, out=o)[1])
            else:
                dense.gemm_nn(a, b, p, seeds[k:k + 1], out=o)
        ctx.starts, ctx.widths, ctx.p = starts, widths, p
        ctx.has_seeds, ctx.n_masks = seeds is not None, len(masks)
        ctx.mask_none = [m is None for m in masks]
        ctx.save_for_backward(x, w, *([seeds] if seeds is not None else []), *[m for m in masks if m is not None])
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, w = ctx.saved_tensors[:2]
        rest = list(ctx.saved_tensors[2:])
        seeds = rest.pop(0) if ctx.has_seeds else None
        masks = [None if none else rest.pop(0) for none in ctx.mask_none] if ctx.n_masks else [None] * len(ctx.starts)
        h, p = w.size(0), ctx.p
        if g.stride(1) != 1:
            g = g.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x, memory_format=torch.contiguous_format)
            sums = torch.empty(x.size(1), dtype=torch.float32, device=x.device)
        if ctx.needs_input_grad[1]:
            dw = torch.zeros_like(w, memory_format=torch.contiguous_format)           # (pad columns: exactly zero)
        for k, (s, c) in enumerate(zip(ctx.starts, ctx.widths)):
            a, b, gk = x[:, k * h:(k + 1) * h], w[:, s:s + c], g[:, s:s + c]
            seed = None if seeds is None else seeds[k:k + 1]
            if dx is not None:                 # g_k W_k^T (masked and scaled under dropout) and its column sums
                dense.gemm_nt(gk, b, p, seed, note_colsums=True, mask=masks[k], out=dx[:, k * h:(k + 1) * h],
                              sums_out=sums[k * h:(k + 1) * h])
            if dw is not None:                 # dropout(H_k)^T g_k
                dense.gemm_tn(a, gk, p, seed, masks[k], out=dw[:, s:s + c])
        if dx is not None:
            note_colsum(dx, sums)              # the bias gradient of layer 1, ready for its propagate step
        return dx, dw, None, None, None, None


def block_diag_xw(x: Tensor, w: Tensor, starts, widths, p: float = 0.0, seeds: Optional[Tensor] = None) -> Tensor:
    """`x [N, K h] @ blockdiag(w[:, seg_1] .. w[:, seg_K])` -> [N, n_cols] (see `_BlockDiagXW`); `seeds` (int64 [K] on the
    device) with 0 < p < 1 fuses dropout(x, p) into product k under seed k."""
    _require_cuda(x, "x")
    K, h = len(starts), w.size(0)
    if x.dim() != 2 or w.dim() != 2 or x.size(1) != K * h or x.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError(f"block_diag_xw: x {tuple(x.shape)} does not fit {K} blocks of {h} rows")
    if any(s % 4 or s + c > w.size(1) for s, c in zip(starts, widths)):
        raise ValueError("block_diag_xw: segments start at multiples of 4 columns inside w")
    if seeds is not None:
        if not 0.0 < p < 1.0:
            raise ValueError("block_diag_xw: seeds go with 0 < p < 1")
        if seeds.dtype != torch.int64 or seeds.shape != (K,) or seeds.device != x.device:
            raise TypeError("block_diag_xw: seeds must be an int64 [K] tensor on the operand's device")
    return _BlockDiagXW.apply(x, w, tuple(starts), tuple(widths), float(p), seeds)


class BlockDiagonalConv(nn.Module):
    """Layer 2 of `PerLabelGCN`: K `GCNConv(h, C_k)` side by side.  `weight` [h, n_cols] holds W2_k in the columns of
    segment k (nothing off the diagonal is stored), `bias` [n_cols] likewise; pad columns are zero and stay zero (their
    gradient is exactly zero)."""

    def __init__(self, n_hidden: int, class_counts: Sequence[int]):
        super().__init__()
        self.n_hidden = int(n_hidden)
        self.class_counts = tuple(int(c) for c in class_counts)
        starts, n_cols = segment_layout(self.class_counts)
        self.seg_start, self.n_cols = tuple(starts), n_cols
        self.weight = nn.Parameter(torch.zeros(self.n_hidden, n_cols))
        self.bias = nn.Parameter(torch.zeros(n_cols))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        with torch.no_grad():
            self.weight.zero_()
            self.bias.zero_()
            for s, c in zip(self.seg_start, self.class_counts):          # glorot of a GCNConv(h, C_k), group by group
                a = math.sqrt(6.0 / (self.n_hidden + c))
                self.weight[:, s:s + c].uniform_(-a, a)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.n_hidden}, {list(self.class_counts)})"


class PerLabelGCN(nn.Module):
    """The K two-layer `GCN(in_channels, C_k, n_hidden_gcn=h, dropout=...)` of perlabel_amazon.py:113 as one network
    (module docstring).  `n_gcn` other than 2, an activation and `ShardedGCN` are out of scope.

    `layers[0]` is ONE `GCNConv(in_channels, K h)` -- member k owns columns [k h, (k + 1) h) -- so activation reuse, the
    optimizer fused into the backward SpMM and every feature format apply as they do to `GCN`.  `layers[1]` is a
    `BlockDiagonalConv`: member k owns the column segment `[seg_start[k], seg_start[k] + class_counts[k])`; segments start
    at multiples of 4 columns and the pad columns between them carry zero weight and bias, which the loss never reads.

    Dropout follows the package's rule: torch's `F.dropout` on H1cat from torch's stream by default; after
    `enable_fused_dropout()` and with 0 < p < 1 each member's product is `dense.xw_dropout` under its own seed.

    `from_members` / `export_members` copy parameters from / to K ordinary `GCN` modules -- the objects
    perlabel_amazon.py:154 saves with `th.save(gcn, "lvl2-cat{k}")` and eval_perlabel.py:16-19 loads; a checkpoint of the
    reference loads into a `GCN` and from there into this class.  Members are COPIES, not views: training this network
    does not change a member that was exported earlier, and the round trip is bit-exact."""

    def __init__(self, in_channels, class_counts, n_hidden_gcn=64, dropout=0.5):
        super().__init__()
        self.class_counts = tuple(int(c) for c in class_counts)
        if not self.class_counts:
            raise ValueError("PerLabelGCN needs at least one group")
        self.in_channels, self.n_hidden, self.dropout = int(in_channels), int(n_hidden_gcn), dropout
        K, h = len(self.class_counts), self.n_hidden
        first = GCNConv(self.in_channels, K * h, add_self_loops=True)
        with torch.no_grad():                  # glorot of a GCNConv(in, h): the same bound for every member
            a = math.sqrt(6.0 / (self.in_channels + h))
            first.weight.uniform_(-a, a)
        self.layers = nn.ModuleList([first, BlockDiagonalConv(h, self.class_counts)])

    @property
    def n_groups(self) -> int:
        return len(self.class_counts)

    @property
    def seg_start(self):
        return self.layers[1].seg_start

    @property
    def seg_width(self):
        return self.class_counts

    @property
    def n_cols(self) -> int:
        return self.layers[1].n_cols

    def forward(self, g, rows=None):
        """Zcat [N, n_cols]: the logits of member k in the columns of segment k.  `rows` (a bool mask the caller keeps):
        the rows that will be read; the last propagate step runs on the operator restricted to them, as in `GCN`."""
        first, second = self.layers
        x = first(g.x, g.edge_index, g.edge_attr)
        p = float(self.dropout) if self.training else 0.0
        if models._FUSED_DROPOUT and 0.0 < p < 1.0:
            seeds = torch.empty(self.n_groups, dtype=torch.int64, device=x.device).random_()
            xw = block_diag_xw(x, second.weight, self.seg_start, self.seg_width, p, seeds)
        else:
            x = nn.functional.dropout(x, p=self.dropout, training=self.training)
            xw = block_diag_xw(x, second.weight, self.seg_start, self.seg_width)
        plan = first.plan(g.x, g.edge_index, g.edge_attr)
        if rows is not None:
            plan = plan.on_rows(rows) or plan
        return propagate(plan, xw, second.bias)

    def loss(self, g, target, mask, group, counts=None, return_pred=False, route=None, class_map=None, rows=None):
        """`grouped_masked_cross_entropy` of `self(g, rows)`: `(loss, loss_k[, pred])`."""
        return functional.grouped_masked_cross_entropy(self(g, rows), target, mask, group, self.seg_start, self.seg_width,
                                                       counts, return_pred, route, class_map)

    @torch.no_grad()
    def predict(self, g, route, class_map=None, rows=None):
        """eval_perlabel.py:71-78 for every node at once: int64 [N], the argmax of the member `route[r]` selects (int32; -1
        = none -> -1), as a column of Zcat or, through `class_map` (`column_class_map`), as the global class."""
        z = self(g, rows)
        n = z.size(0)
        nothing = torch.zeros(n, dtype=torch.bool, device=z.device)
        return functional.grouped_masked_cross_entropy(
            z, torch.zeros(n, dtype=torch.int64, device=z.device), nothing, route, self.seg_start, self.seg_width,
            counts=[0] * self.n_groups, return_pred=True, route=route, class_map=class_map)[2]

    @classmethod
    def from_members(cls, members: Sequence[nn.Module], dropout: Optional[float] = None) -> "PerLabelGCN":
        """One network from K two-layer `GCN`s (or modules with the same `layers.{0,1}.{weight,bias}`, such as the
        reference's checkpoints loaded into `GCN`) of equal input and hidden width.  Parameters are copied."""
        members = list(members)
        if not members:
            raise ValueError("from_members: no member")
        w1 = [m.layers[0].weight for m in members]
        if any(len(m.layers) != 2 for m in members) or any(w.shape != w1[0].shape for w in w1) or \
                any(m.layers[1].weight.size(0) != w1[0].size(1) for m in members):
            raise ValueError("from_members: members must be two-layer GCNs of equal input and hidden width")
        if any(layer.bias is None for m in members for layer in m.layers):
            raise ValueError("from_members: members must carry biases")
        h = w1[0].size(1)
        net = cls(w1[0].size(0), [m.layers[1].weight.size(1) for m in members], n_hidden_gcn=h,
                  dropout=members[0].dropout if dropout is None else dropout)
        net = net.to(w1[0].device)
        first, second = net.layers
        with torch.no_grad():
            second.weight.zero_()
            second.bias.zero_()
            for k, (m, s, c) in enumerate(zip(members, net.seg_start, net.seg_width)):
                first.weight[:, k * h:(k + 1) * h].copy_(m.layers[0].weight)
                first.bias[k * h:(k + 1) * h].copy_(m.layers[0].bias)
                second.weight[:, s:s + c].copy_(m.layers[1].weight)
                second.bias[s:s + c].copy_(m.layers[1].bias)
        return net

    @torch.no_grad()
    def export_members(self) -> List[nn.Module]:
        """K `GCN(in_channels, C_k, n_hidden_gcn=h, dropout=...)` holding COPIES of the members' parameters, in this
        network's training mode: what perlabel_amazon.py:154 saves one by one."""
        first, second = self.layers
        h, out = self.n_hidden, []
        for k, (s, c) in enumerate(zip(self.seg_start, self.seg_width)):
            m = models.GCN(self.in_channels, c, n_hidden_gcn=h, dropout=self.dropout).to(first.weight.device)
            m.layers[0].weight.copy_(first.weight[:, k * h:(k + 1) * h])
            m.layers[0].bias.copy_(first.bias[k * h:(k + 1) * h])
            m.layers[1].weight.copy_(second.weight[:, s:s + c])
            m.layers[1].bias.copy_(second.bias[s:s + c])
            out.append(m.train(self.training))
        return out
