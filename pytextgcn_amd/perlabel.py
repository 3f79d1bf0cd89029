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
import weakref
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor, nn

from . import _lib, dense, functional, mlp, models
from .conv import GCNConv, features_times, propagate
from .plan import _require_cuda, _stream_ptr, note_colsum


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
    def forward(ctx, x: Tensor, w: Tensor, starts, widths, p, seeds: Optional[Tensor]):
        K, h = len(starts), w.size(0)
        rates = p if isinstance(p, tuple) else (p,) * K       # a rate per member; a member at rate 0 runs the plain product
        N = x.size(0)
        xd, wd = x.detach(), w.detach()
        out = torch.zeros(N, w.size(1), dtype=torch.float32, device=x.device)       # class width; pad columns stay zero
        want_mask = seeds is not None and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        masks = []
        for k, (s, c) in enumerate(zip(starts, widths)):
            a, b, o = xd[:, k * h:(k + 1) * h], wd[:, s:s + c], out[:, s:s + c]
            if seeds is None or rates[k] == 0.0:
                dense.gemm_nn(a, b, out=o)
                masks.append(None)
            elif want_mask:
                masks.append(dense.gemm_nn(a, b, rates[k], seeds[k:k + 1], record_mask=True, out=o)[1])
            else:
                dense.gemm_nn(a, b, rates[k], seeds[k:k + 1], out=o)
                masks.append(None)
        ctx.starts, ctx.widths, ctx.rates = starts, widths, rates
        ctx.has_seeds = seeds is not None
        ctx.mask_none = [m is None for m in masks]
        ctx.save_for_backward(x, w, *([seeds] if seeds is not None else []), *[m for m in masks if m is not None])
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, w = ctx.saved_tensors[:2]
        rest = list(ctx.saved_tensors[2:])
        seeds = rest.pop(0) if ctx.has_seeds else None
        masks = [None if none else rest.pop(0) for none in ctx.mask_none]
        h, rates = w.size(0), ctx.rates
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
            p = rates[k]
            seed = None if seeds is None or p == 0.0 else seeds[k:k + 1]
            if dx is not None:                 # g_k W_k^T (masked and scaled under dropout) and its column sums
                dense.gemm_nt(gk, b, p, seed, note_colsums=True, mask=masks[k], out=dx[:, k * h:(k + 1) * h],
                              sums_out=sums[k * h:(k + 1) * h])
            if dw is not None:                 # dropout(H_k)^T g_k
                dense.gemm_tn(a, gk, p, seed, masks[k], out=dw[:, s:s + c])
        if dx is not None:
            note_colsum(dx, sums)              # the bias gradient of layer 1, ready for its propagate step
        return dx, dw, None, None, None, None


_FUSED_BLOCK_DIAG = False


def enable_fused_block_diag(on: bool = True) -> bool:
    """Route `block_diag_xw` through the one-launch products of all K members (`tgcn_blockdiag_xw`, `_grad`) instead of K
    launches per product; returns the previous setting.  Off by default: the mask decisions are the same, but the sums run
    in another order than `dense.xw_dropout`'s, so the bits are not those of the K separate members."""
    global _FUSED_BLOCK_DIAG
    was, _FUSED_BLOCK_DIAG = _FUSED_BLOCK_DIAG, bool(on)
    return was


class BlockDiagLayout:
    """The member table of the one-launch products: segment k is columns [starts[k], starts[k] + widths[k]) of the
    [h, n_cols] weight, `rates[k]` its dropout rate.  Built and validated on the HOST by `tgcn_blockdiag_layout` (a
    ValueError names what does not fit; no GPU is touched); `host` is the blob as a uint8 array, `dev` its copy on `device`
    (None: host only), uploaded once."""

    HEADER = ("magic", "bytes", "K", "h", "n_cols", "n_max", "own_max", "any_drop")
    MEMBER = np.dtype([("col0", "<i4"), ("n", "<i4"), ("own0", "<i4"), ("own1", "<i4"), ("thresh", "<u4"), ("scale", "<f4"),
                       ("drop", "<i4"), ("pad", "<i4")])

    def __init__(self, starts: Sequence[int], widths: Sequence[int], h: int, n_cols: int, rates=None, device=None):
        lib = _lib.load()
        K = len(starts)
        col0 = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
        n = np.ascontiguousarray(np.asarray(widths, dtype=np.int32))
        p = None if rates is None else np.ascontiguousarray(np.asarray(rates, dtype=np.float64))
        if n.shape != (K,) or (p is not None and p.shape != (K,)):
            raise ValueError(f"BlockDiagLayout: widths and rates need one entry per member (K = {K})")
        size = lib.tgcn_blockdiag_layout_bytes(K)
        self.host = np.zeros(max(size, 8), dtype=np.uint8)
        _lib.check(lib.tgcn_blockdiag_layout(K, int(h), int(n_cols), col0.ctypes.data, n.ctypes.data,
                                             None if p is None else p.ctypes.data, self.host.ctypes.data, size))
        self.header = dict(zip(self.HEADER, np.frombuffer(self.host, dtype="<i8", count=len(self.HEADER)).tolist()))
        self.K, self.h, self.n_cols = K, int(h), int(n_cols)
        self.dev = None if device is None else torch.from_numpy(self.host).to(device)

    def members(self):
        """The member table of the blob as a numpy record array (a view of `host`)."""
        return np.frombuffer(self.host, dtype=self.MEMBER, count=self.K, offset=8 * len(self.HEADER))


_BD_LAYOUTS: dict = {}            # id(weight) -> (weak reference to the weight, {description: BlockDiagLayout})


def _bd_layout(w: Tensor, starts, widths, rates) -> BlockDiagLayout:
    """The layout of the product with the weight `w`, kept for as long as `w` lives -- for a network, its layer-2
    parameter: built in the first, eager step, found by a captured one, and NEVER evicted while the network exists (a
    captured graph holds the raw pointer of the device blob; freeing the blob under it would hand a replay a foreign
    member table).  An entry goes when its weight is collected."""
    key = id(w)
    hit = _BD_LAYOUTS.get(key)
    if hit is None or hit[0]() is not w:
        hit = _BD_LAYOUTS[key] = (weakref.ref(w, lambda _, k=key: _BD_LAYOUTS.pop(k, None)), {})
    what = (starts, widths, w.size(0), w.size(1), rates, w.device)
    layout = hit[1].get(what)
    if layout is None:
        layout = hit[1][what] = BlockDiagLayout(starts, widths, w.size(0), w.size(1), rates, w.device)
    return layout


def _ld(t: Tensor) -> int:
    return max(t.stride(0), t.size(1))


def _rows_cols(t: Tensor) -> Tensor:
    return t if (t.stride(1) == 1 and (t.size(0) <= 1 or t.stride(0) >= t.size(1))) else t.contiguous()


def block_diag_forward(x: Tensor, w: Tensor, layout: BlockDiagLayout, seeds: Optional[Tensor] = None, mask_row0: int = 0,
                       out: Optional[Tensor] = None) -> Tensor:
    """C [N, n_cols] of `tgcn_blockdiag_xw`: one launch per 256 columns of the widest segment for all K members; pad
    columns are written as zeros.  `seeds` None: no member drops anything.  No autograd."""
    lib = _lib.load()
    x, w = _rows_cols(x), _rows_cols(w)
    N = x.size(0)
    c = torch.empty(N, layout.n_cols, dtype=torch.float32, device=x.device) if out is None else out
    _lib.check(lib.tgcn_blockdiag_xw(x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), c.data_ptr(), _ld(c), N,
                                     layout.host.ctypes.data, layout.dev.data_ptr(),
                                     None if seeds is None else seeds.data_ptr(), int(mask_row0), _stream_ptr(x.device)))
    return c


def block_diag_backward(x: Tensor, w: Tensor, g: Tensor, layout: BlockDiagLayout, seeds: Optional[Tensor] = None,
                        want_x: bool = True, want_w: bool = True, mask_row0: int = 0):
    """(dX, colsum, dW) of `tgcn_blockdiag_xw_grad` for G = dC; what is not wanted comes back as None."""
    if not (want_x or want_w):
        return None, None, None
    lib = _lib.load()
    x, w, g = _rows_cols(x), _rows_cols(w), _rows_cols(g)
    N, dev = x.size(0), x.device
    dx = torch.empty(N, x.size(1), dtype=torch.float32, device=dev) if want_x else None
    sums = torch.empty(x.size(1), dtype=torch.float32, device=dev) if want_x else None
    dw = torch.empty(w.size(0), w.size(1), dtype=torch.float32, device=dev) if want_w else None
    need = lib.tgcn_blockdiag_xw_grad_workspace_bytes(layout.host.ctypes.data, N)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _lib.check(lib.tgcn_blockdiag_xw_grad(
        x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), g.data_ptr(), _ld(g), dx.data_ptr() if want_x else None,
        _ld(dx) if want_x else x.size(1), sums.data_ptr() if want_x else None, dw.data_ptr() if want_w else None,
        _ld(dw) if want_w else w.size(1), N, layout.host.ctypes.data, layout.dev.data_ptr(),
        None if seeds is None else seeds.data_ptr(), int(mask_row0), ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
    return dx, sums, dw


class _FusedBlockDiagXW(torch.autograd.Function):
    """`_BlockDiagXW` on the one-launch products: ONE kernel per product for all K members (a launch more per 256 / 128
    columns of the widest segment), a rate and a seed per member, the mask regenerated from the seeds in all three."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, layout: BlockDiagLayout, seeds: Optional[Tensor]):
        ctx.layout = layout
        ctx.save_for_backward(x, w, *([seeds] if seeds is not None else []))
        return block_diag_forward(x.detach(), w.detach(), layout, seeds)

    @staticmethod
    def backward(ctx, g: Tensor):
        x, w = ctx.saved_tensors[:2]
        seeds = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        dx, sums, dw = block_diag_backward(x, w, g, ctx.layout, seeds, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if dx is not None:
            note_colsum(dx, sums)              # the bias gradient of layer 1, ready for its propagate step
        return dx, dw, None, None


def member_rates(dropout, K: int, what: str = "dropout"):
    """`dropout` as the networks keep it: a float as it is, K rates as a tuple of K floats, each in [0, 1)."""
    if isinstance(dropout, (int, float)):
        return dropout
    rates = tuple(float(v) for v in dropout)
    if len(rates) != K:
        raise ValueError(f"{what}: {len(rates)} rates for {K} members")
    if not all(0.0 <= v < 1.0 for v in rates):
        raise ValueError(f"{what}: every member's rate must be in [0, 1), got {list(rates)}")
    return rates


def block_diag_xw(x: Tensor, w: Tensor, starts, widths, p=0.0, seeds: Optional[Tensor] = None) -> Tensor:
    """`x [N, K h] @ blockdiag(w[:, seg_1] .. w[:, seg_K])` -> [N, n_cols] (see `_BlockDiagXW`); `seeds` (int64 [K] on the
    device) with 0 < p < 1 fuses dropout(x, p) into product k under seed k.  `p` may also be K rates in [0, 1), at least
    one of them > 0: member k drops at `p[k]` (a member at rate 0 runs the plain product).  After
    `enable_fused_block_diag()` the three products are one launch each for all K members (`_FusedBlockDiagXW`)."""
    _require_cuda(x, "x")
    K, h = len(starts), w.size(0)
    if x.dim() != 2 or w.dim() != 2 or x.size(1) != K * h or x.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError(f"block_diag_xw: x {tuple(x.shape)} does not fit {K} blocks of {h} rows")
    if any(s % 4 or s + c > w.size(1) for s, c in zip(starts, widths)):
        raise ValueError("block_diag_xw: segments start at multiples of 4 columns inside w")
    p = float(p) if isinstance(p, (int, float)) else member_rates(p, K, "block_diag_xw")
    if seeds is not None:
        if isinstance(p, tuple):
            if not max(p) > 0.0:
                raise ValueError("block_diag_xw: seeds go with at least one rate > 0")
        elif not 0.0 < p < 1.0:
            raise ValueError("block_diag_xw: seeds go with 0 < p < 1")
        if seeds.dtype != torch.int64 or seeds.shape != (K,) or seeds.device != x.device:
            raise TypeError("block_diag_xw: seeds must be an int64 [K] tensor on the operand's device")
    if _FUSED_BLOCK_DIAG:
        rates = None if seeds is None else (p if isinstance(p, tuple) else (p,) * K)
        if w.device != x.device:
            raise RuntimeError(f"block_diag_xw: x lives on {x.device}, w on {w.device}")
        layout = _bd_layout(w, tuple(starts), tuple(widths), rates)
        return _FusedBlockDiagXW.apply(x, w, layout, seeds)
    return _BlockDiagXW.apply(x, w, tuple(starts), tuple(widths), p, seeds)


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


class MemberDropoutXW:
    """The dropout of the propagated [N, K h] activation and its product with the block-diagonal layer-2 weight, for the
    networks of K members (`PerLabelGCN`, `crossval.CrossValGCN`, `crossval.CrossValEGCN`).  It reads these and nothing else
    of the network: `dropout` (a float, or a tuple of K rates), `n_groups`, `n_hidden`, `seg_start`, `seg_width` and
    `training`."""

    def _dropout_xw(self, x: Tensor, weight: Tensor) -> Tensor:
        """dropout(H1cat) blockdiag(W2) under the class's dropout rules (`crossval.CrossValEGCN` runs it as well)."""
        if isinstance(self.dropout, tuple):
            return self._xw_member_rates(x, weight)
        if models._FUSED_DROPOUT and self.training and 0.0 < float(self.dropout) < 1.0:
            seeds = torch.empty(self.n_groups, dtype=torch.int64, device=x.device).random_()
            return block_diag_xw(x, weight, self.seg_start, self.seg_width, float(self.dropout), seeds)
        x = nn.functional.dropout(x, p=self.dropout, training=self.training)
        return block_diag_xw(x, weight, self.seg_start, self.seg_width)

    def _xw_member_rates(self, x: Tensor, weight: Tensor) -> Tensor:
        """dropout(H1cat) blockdiag(W2) with a rate per member (`self.dropout` is a tuple)."""
        rates, h = self.dropout, self.n_hidden
        if not self.training or max(rates) == 0.0:
            return block_diag_xw(x, weight, self.seg_start, self.seg_width)
        if models._FUSED_DROPOUT:
            seeds = torch.empty(self.n_groups, dtype=torch.int64, device=x.device).random_()
            return block_diag_xw(x, weight, self.seg_start, self.seg_width, rates, seeds)
        # torch's stream: F.dropout per column block with its rate (K small launches and one concatenation)
        x = torch.cat([nn.functional.dropout(x[:, k * h:(k + 1) * h], p=p, training=True) for k, p in enumerate(rates)], 1)
        return block_diag_xw(x, weight, self.seg_start, self.seg_width)

    def member_dropout(self, k: int) -> float:
        """The dropout rate of member k."""
        return self.dropout[k] if isinstance(self.dropout, tuple) else self.dropout

    @staticmethod
    def _rates_of(members, dropout):
        """`from_members`' rule: `dropout` when it is given; else the members' rates -- a float when they are all equal,
        the K rates when they differ."""
        if dropout is not None:
            return dropout
        rates = [m.dropout for m in members]
        return rates[0] if all(r == rates[0] for r in rates) else rates


class PerLabelGCN(MemberDropoutXW, nn.Module):
    """The K two-layer `GCN(in_channels, C_k, n_hidden_gcn=h, dropout=...)` of perlabel_amazon.py:113 as one network
    (module docstring).  `n_gcn` other than 2, an activation and `ShardedGCN` are out of scope.  `dropout` is one rate for
    all members (a float) or K rates in [0, 1), one per member.

    `layers[0]` is ONE `GCNConv(in_channels, K h)` -- member k owns columns [k h, (k + 1) h) -- so activation reuse, the
    optimizer fused into the backward SpMM and every feature format apply as they do to `GCN`.  `layers[1]` is a
    `BlockDiagonalConv`: member k owns the column segment `[seg_start[k], seg_start[k] + class_counts[k])`; segments start
    at multiples of 4 columns and the pad columns between them carry zero weight and bias, which the loss never reads.

    Dropout follows the package's rule: torch's `F.dropout` on H1cat from torch's stream by default; after
    `enable_fused_dropout()` and with 0 < p < 1 each member's product is `dense.xw_dropout` under its own seed.  With a rate
    per member the fused form hands the K rates to `block_diag_xw` (a fresh seed per member, a member at rate 0 keeps
    everything); on torch's stream the dropout is `F.dropout` per column block with its rate, which costs K small launches
    and a concatenation per step.  `enable_fused_block_diag()` runs the three layer-2 products as one launch each for all
    K members.  Eval mode drops nothing in any form.

    `from_members` / `export_members` copy parameters from / to K ordinary `GCN` modules -- the objects
    perlabel_amazon.py:154 saves with `th.save(gcn, "lvl2-cat{k}")` and eval_perlabel.py:16-19 loads; a checkpoint of the
    reference loads into a `GCN` and from there into this class.  Members are COPIES, not views: training this network
    does not change a member that was exported earlier, and the round trip is bit-exact."""

    def __init__(self, in_channels, class_counts, n_hidden_gcn=64, dropout=0.5):
        super().__init__()
        self.class_counts = tuple(int(c) for c in class_counts)
        if not self.class_counts:
            raise ValueError("PerLabelGCN needs at least one group")
        K = len(self.class_counts)
        self.in_channels, self.n_hidden = int(in_channels), int(n_hidden_gcn)
        self.dropout = member_rates(dropout, K, type(self).__name__)       # a float, or a tuple of K rates
        h = self.n_hidden
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
        xw = self._dropout_xw(x, second.weight)
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

    @torch.no_grad()
    def score(self, g, target, group, train_mask, val_mask, counts=None, rows=None):
        """The eval forward (no dropout, whatever mode the network is in; the mode is put back) scored on the device:
        `(val_loss_k [K], train_scores, val_scores)` -- the members' validation losses on `val_mask & (group == k)` and two
        `metrics.Scores(accuracy, f1_macro, n_rows, n_labels)` of float64 [K] device tensors, member k's on the rows of its
        group that `train_mask` / `val_mask` select (perlabel_amazon.py:139-150 takes them per label on the host).  One
        forward, one `tgcn_grouped_ce` with predictions, one count launch for both masks, two score launches; no host
        round trip (`counts`: the validation rows per group, as in `loss`)."""
        from . import metrics
        was = self.training
        self.eval()
        try:
            z = self(g, rows)
            seg = functional.Segments.of(self.seg_start, self.seg_width, z.device)
            _, val_loss_k, pred = functional.grouped_masked_cross_entropy(z, target, val_mask, group, seg, None, counts, True)
        finally:
            self.train(was)
        c_train, c_val = metrics.grouped_class_counts(pred, target, train_mask, max(self.class_counts), group, self.n_groups,
                                                      seg.dev_start, also=val_mask)
        return val_loss_k, metrics.scores(c_train), metrics.scores(c_val)

    @classmethod
    def from_members(cls, members: Sequence[nn.Module], dropout=None) -> "PerLabelGCN":
        """One network from K two-layer `GCN`s (or modules with the same `layers.{0,1}.{weight,bias}`, such as the
        reference's checkpoints loaded into `GCN`) of equal input and hidden width.  Parameters are copied.  `dropout`
        (a float or K floats) overrides the members' rates; without it the network keeps one float when the members'
        rates are all equal and the K rates when they differ."""
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
                  dropout=cls._rates_of(members, dropout))
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
        """K `GCN(in_channels, C_k, n_hidden_gcn=h, dropout=...)` holding COPIES of the members' parameters, member k with
        its own rate, in this network's training mode: what perlabel_amazon.py:154 saves one by one."""
        first, second = self.layers
        h, out = self.n_hidden, []
        for k, (s, c) in enumerate(zip(self.seg_start, self.seg_width)):
            m = models.GCN(self.in_channels, c, n_hidden_gcn=h, dropout=self.member_dropout(k)).to(first.weight.device)
            m.layers[0].weight.copy_(first.weight[:, k * h:(k + 1) * h])
            m.layers[0].bias.copy_(first.bias[k * h:(k + 1) * h])
            m.layers[1].weight.copy_(second.weight[:, s:s + c])
            m.layers[1].bias.copy_(second.bias[s:s + c])
            out.append(m.train(self.training))
        return out


# ---------------------------------------------------------------------------------------------------------------------
# The per-label strategy of the bag-of-words baseline (MLP_label.py): one `MLP(in, C_k, [256, 128])` per top-level label,
# trained on that label's documents.  A document belongs to exactly ONE member, so the K members are one MLP whose weight
# depends on the row's group: the rows are put in grouped order once per split (`GroupedRows`), layer 1 is the existing
# SpMM on features whose column ids are shifted by group * F, and every later layer is `mlp.grouped_act_linear`.
# ---------------------------------------------------------------------------------------------------------------------
class GroupedRows:
    """The rows of one split (train, val or routed test) in grouped order, built once on the host.

    `group` [N]: the member of every row, -1 = none (an unrouted document).  `order` (int64 [N]) is the stable sort by
    group with the -1 rows last, `row_ptr` (K + 1 ints) the segment boundaries, `n_routed = row_ptr[K]`; `group_sorted`
    (int32 [N]) is `group[order]`, the tensor `grouped_masked_cross_entropy` takes, `routed` (bool [N]) its rows with a group.  `to(device)` moves the index tensors;
    the per-layer layout blobs of `mlp.GroupedLayout` are cached here per device."""

    def __init__(self, group, n_groups: int):
        g = np.asarray(torch.as_tensor(group).cpu()).astype(np.int64).ravel()
        K = int(n_groups)
        if K < 1:
            raise ValueError("GroupedRows: n_groups must be >= 1")
        if g.size and (g.min() < -1 or g.max() >= K):
            raise ValueError(f"GroupedRows: groups must lie in [-1, {K}) (found {int(g.min())} .. {int(g.max())})")
        key = np.where(g < 0, K, g)
        order = np.argsort(key, kind="stable")
        counts = np.bincount(key, minlength=K + 1)[:K]
        self.n_groups, self.n_rows = K, int(g.size)
        self.row_ptr = [0] + np.cumsum(counts).tolist()
        self.n_routed = int(self.row_ptr[K])
        self.order = torch.from_numpy(order)
        self.group_sorted = torch.from_numpy(g[order].astype(np.int32))
        self.routed = self.group_sorted >= 0               # (one object: the loss counts a mask's rows once per object)
        self._group = torch.from_numpy(g)
        pos = np.empty_like(order)
        pos[order] = np.arange(order.size)
        self._pos = torch.from_numpy(pos)                  # row of the caller's order -> row in grouped order
        self._layouts: dict = {}

    def to(self, device) -> "GroupedRows":
        for name in ("order", "group_sorted", "routed", "_group", "_pos"):
            setattr(self, name, getattr(self, name).to(device))
        return self

    def _on(self, t: Tensor, name: str) -> Tensor:
        idx = getattr(self, name)
        if idx.device != t.device:
            raise RuntimeError(f"GroupedRows lives on {idx.device}, the tensor on {t.device}: call rows.to(device) once")
        return idx

    def take(self, t: Tensor) -> Tensor:
        """A per-row tensor [N, ...] in grouped order."""
        if t.size(0) != self.n_rows:
            raise ValueError(f"GroupedRows.take: {t.size(0)} rows, the split has {self.n_rows}")
        return t.index_select(0, self._on(t, "order"))

    def restore(self, t: Tensor, fill=-1) -> Tensor:
        """A per-row tensor in grouped order back in the caller's order; rows without a group hold `fill`."""
        if t.size(0) != self.n_rows:
            raise ValueError(f"GroupedRows.restore: {t.size(0)} rows, the split has {self.n_rows}")
        out = torch.full_like(t, fill)
        routed = self._on(t, "order")[:self.n_routed]
        out.index_copy_(0, routed, t[:self.n_routed])
        return out

    def features(self, x: Tensor) -> Tensor:
        """Sparse COO / CSR features [N, F] -> coalesced sparse COO [N, K F] in grouped order: the entry (i, j) of a row of
        group g sits at (position of i, g F + j), so `x' @ stack_k(W1_k)` is every row times its own member's W1.  Rows
        without a group are empty."""
        if x.layout not in (torch.sparse_coo, torch.sparse_csr) or x.dim() != 2:
            raise TypeError("GroupedRows.features takes a sparse COO or CSR [N, F] matrix")
        if x.size(0) != self.n_rows:
            raise ValueError(f"GroupedRows.features: {x.size(0)} rows, the split has {self.n_rows}")
        xc = (x.to_sparse_coo() if x.layout == torch.sparse_csr else x).coalesce()
        idx, val = xc.indices(), xc.values()
        g = self._on(val, "_group")[idx[0]]
        keep = g >= 0
        rows = self._on(val, "_pos")[idx[0]][keep]
        cols = (idx[1] + g * x.size(1))[keep]
        return torch.sparse_coo_tensor(torch.stack([rows, cols]), val[keep],
                                       (self.n_rows, self.n_groups * x.size(1))).coalesce()

    def layout(self, w_row0, n, col0, b_off, k: int, w_rows: int, c_cols: int, b_len: int, device) -> mlp.GroupedLayout:
        """The cached `mlp.GroupedLayout` of one layer on `device`."""
        key = (tuple(w_row0), tuple(n), tuple(col0), tuple(b_off), k, w_rows, c_cols, b_len, torch.device(device))
        hit = self._layouts.get(key)
        if hit is None:
            hit = self._layouts[key] = mlp.GroupedLayout(self.row_ptr, w_row0, n, col0, b_off, self.n_rows, k, w_rows,
                                                         c_cols, b_len, device)
        return hit


class PerLabelMLP(nn.Module):
    """The K `MLP(in_channels, C_k, hidden, dropout)` of MLP_label.py as one network (equal `in_channels` and `hidden`).

    `layers[0]` is an `EmbeddingLinear(K F, h_1)` whose bias is [K h_1]: member k owns the input columns [k F, (k + 1) F)
    and the bias slice [k h_1, (k + 1) h_1).  `layers[i]`, 0 < i < L, is an `EmbeddingLinear(h_i, K h_{i+1})`: member k owns
    the weight rows and bias entries [k h_{i+1}, (k + 1) h_{i+1}).  The last layer is an `EmbeddingLinear(h_L, n_cols)`:
    member k owns rows [seg_start[k], seg_start[k] + C_k) (`segment_layout`; the pad rows are zero, stay zero and are never
    read).  Every member's slice is initialised with torch's `nn.Linear` default bounds for the MEMBER's fan-in.

    `forward(xg, rows)` takes `xg = rows.features(x)` and returns Zcat [N, n_cols] in grouped order: the logits of a row in
    its member's segment, zero elsewhere -- what `functional.grouped_masked_cross_entropy` takes with `rows.group_sorted`.

    The fused path (`mlp.grouped_act_linear`, one product per layer whatever K is) follows `MLP.takes_fused_path`: eval
    mode, rate 0, or training with 0 < rate < 1 while `enable_fused_dropout()` is on.  Everything else, and everything
    after `enable_fused_mlp(False)`, is composed group by group from `torch.selu`, `self.dropout` and `dense.xw`.

    Not built: per-member early stopping (the members train in lock step), `hidden` differing between members, more than
    128 groups, the grouped network on the appended features of MLP_level.py (`perlevel.AppendedFeatures` is `MLP`'s
    input, not this class's), several GPUs."""

    def __init__(self, in_channels, class_counts, hidden, dropout=0.5):
        super().__init__()
        self.class_counts = tuple(int(c) for c in class_counts)
        self.hidden = tuple(int(h) for h in hidden)
        if not self.class_counts or not self.hidden:
            raise ValueError("PerLabelMLP needs at least one group and one hidden layer")
        if len(self.class_counts) > 128:
            raise ValueError("PerLabelMLP: at most 128 groups")
        self.in_channels = int(in_channels)
        self.dropout = nn.Dropout(p=dropout)
        self.act = nn.SELU()
        K, F = len(self.class_counts), self.in_channels
        starts, n_cols = segment_layout(self.class_counts)
        self.seg_start, self.n_cols = tuple(starts), n_cols
        first = models.EmbeddingLinear(K * F, self.hidden[0])
        first.bias = nn.Parameter(torch.zeros(K * self.hidden[0]))
        ls = [first]
        ls += [models.EmbeddingLinear(h1, K * h2) for h1, h2 in zip(self.hidden, self.hidden[1:])]
        ls += [models.EmbeddingLinear(self.hidden[-1], n_cols)]
        self.layers = nn.ModuleList(ls)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        """torch's `nn.Linear.reset_parameters` per member: weight and bias uniform in +-1 / sqrt(fan_in of the member)."""
        sizes = (self.in_channels,) + self.hidden
        with torch.no_grad():
            for layer, fan_in in zip(self.layers, sizes):
                a = 1.0 / math.sqrt(fan_in)
                layer.weight.uniform_(-a, a)
                layer.bias.uniform_(-a, a)
            last = self.layers[-1]
            own = torch.zeros(self.n_cols, dtype=torch.bool)
            for s, c in zip(self.seg_start, self.class_counts):
                own[s:s + c] = True
            last.weight[~own] = 0.0
            last.bias[~own] = 0.0

    @property
    def n_groups(self) -> int:
        return len(self.class_counts)

    @property
    def seg_width(self):
        return self.class_counts

    def takes_fused_path(self, x=None) -> bool:
        p = float(self.dropout.p)
        if not models._FUSED_MLP:
            return False
        return not (self.training and p != 0.0 and not (models._FUSED_DROPOUT and 0.0 < p < 1.0))

    def _member(self, i: int, g: int):
        """(first row, rows, first output column) of member g in layer i >= 1."""
        if i == len(self.layers) - 1:
            return self.seg_start[g], self.class_counts[g], self.seg_start[g]
        n = self.hidden[i]
        return g * n, n, 0

    def _check(self, xg, rows) -> None:
        _require_cuda(xg, "xg")
        if not isinstance(rows, GroupedRows) or rows.n_groups != self.n_groups:
            raise ValueError(f"PerLabelMLP: `rows` must be a GroupedRows of {self.n_groups} groups"
                             + (f" (it has {rows.n_groups})" if isinstance(rows, GroupedRows) else ""))
        if xg.dim() != 2 or xg.size(1) != self.n_groups * self.in_channels or xg.size(0) != rows.n_rows:
            raise ValueError(f"PerLabelMLP: features {tuple(xg.shape)} do not fit {rows.n_rows} rows of {self.n_groups} x "
                             f"{self.in_channels} columns (pass rows.features(x))")
        if xg.dtype != torch.float32:
            raise TypeError(f"PerLabelMLP takes float32 features, got {xg.dtype}")

    def forward(self, xg, rows: GroupedRows) -> Tensor:
        self._check(xg, rows)
        K, first, L = self.n_groups, self.layers[0], len(self.layers) - 1
        z = features_times(xg, first.weight.t(), first.in_features)        # no bias: the next product adds it
        if self.takes_fused_path():
            p = float(self.dropout.p) if self.training else 0.0
            for i in range(1, L + 1):
                prev, layer = self.layers[i - 1], self.layers[i]
                k = self.hidden[i - 1]
                w_row0, n, col0 = zip(*[self._member(i, g) for g in range(K)])
                lay = rows.layout(w_row0, n, col0, [g * k for g in range(K)], k, layer.weight.size(0),
                                  self.hidden[i] if i < L else self.n_cols, K * k, z.device)
                z = mlp.grouped_act_linear(z, prev.bias, layer.weight, layer.bias if i == L else None, lay, p)
            return z
        out = torch.zeros(rows.n_rows, self.n_cols, dtype=torch.float32, device=z.device)
        for g in range(K):
            r0, r1 = rows.row_ptr[g], rows.row_ptr[g + 1]
            if r0 == r1:
                continue
            a = z[r0:r1]
            for i in range(1, L + 1):
                k = self.hidden[i - 1]
                w0, n, _ = self._member(i, g)
                a = self.dropout(torch.selu(a + self.layers[i - 1].bias[g * k:(g + 1) * k]))
                a = dense.xw(a, self.layers[i].weight[w0:w0 + n].t())
            s, c = self.seg_start[g], self.class_counts[g]
            out[r0:r1, s:s + c] = a + self.layers[L].bias[s:s + c]
        return out

    def loss(self, xg, rows: GroupedRows, target, mask=None, return_pred=False, class_map=None):
        """`grouped_masked_cross_entropy` of `self(xg, rows)` -- the sum over the members of CrossEntropyLoss('mean') on
        their own rows: `(loss, loss_k[, pred])`.  `target` (int64 [N], grouped order: `rows.take`) holds the LOCAL class
        (`relabel`), `mask` (bool [N], grouped order; default: every routed row) the rows that count."""
        z = self(xg, rows)
        group = rows._on(z, "group_sorted")
        if mask is None:
            mask = rows.routed
        return functional.grouped_masked_cross_entropy(z, target, mask, group, self.seg_start, self.seg_width, None,
                                                       return_pred, None, class_map)

    @torch.no_grad()
    def score(self, xg, rows: GroupedRows, target, mask=None):
        """One split scored on the device (MLP_label.py takes accuracy and F1 per label on the host): `(loss_k [K],
        scores)` of `self(xg, rows)` in the network's current mode -- call `eval()` first for a validation or test split --
        with `scores` a `metrics.Scores(accuracy, f1_macro, n_rows, n_labels)` of float64 [K] device tensors, member k's on
        the rows of its group that `mask` selects (bool [N], grouped order; default: every routed row).  `target` as in
        `loss`.  No host round trip."""
        from . import metrics
        z = self(xg, rows)
        group = rows._on(z, "group_sorted")
        if mask is None:
            mask = rows.routed
        seg = functional.Segments.of(self.seg_start, self.seg_width, z.device)
        _, loss_k, pred = functional.grouped_masked_cross_entropy(z, target, mask, group, seg, None, None, True)
        counts = metrics.grouped_class_counts(pred, target, mask, max(self.class_counts), group, self.n_groups, seg.dev_start)
        return loss_k, metrics.scores(counts)

    @torch.no_grad()
    def predict(self, xg, rows: GroupedRows, class_map=None) -> Tensor:
        """MLP_label.py:157-162 for every routed row at once: int64 [N] in GROUPED order (apply `rows.restore`), the arg-max
        of the row's member as a column of Zcat or, through `class_map` (`column_class_map`), as the global class; -1 on
        rows without a group."""
        z = self(xg, rows)
        n = z.size(0)
        group = rows._on(z, "group_sorted")
        nothing = torch.zeros(n, dtype=torch.bool, device=z.device)
        return functional.grouped_masked_cross_entropy(
            z, torch.zeros(n, dtype=torch.int64, device=z.device), nothing, group, self.seg_start, self.seg_width,
            counts=[0] * self.n_groups, return_pred=True, route=group, class_map=class_map)[2]

    @classmethod
    def from_members(cls, members: Sequence[nn.Module], dropout: Optional[float] = None) -> "PerLabelMLP":
        """One network from K `MLP`s (or modules with the same `layers.{i}.{weight,bias}`, such as the reference's
        checkpoints loaded into `MLP`) of equal input and hidden widths.  Parameters are copied."""
        members = list(members)
        if not members:
            raise ValueError("from_members: no member")
        shapes = [[tuple(layer.weight.shape) for layer in m.layers] for m in members]
        if any(len(s) != len(shapes[0]) or len(s) < 2 or s[:-1] != shapes[0][:-1] or s[-1][1] != shapes[0][-1][1]
               for s in shapes):
            raise ValueError("from_members: members must be MLPs of equal input width and equal hidden widths")
        if any(layer.bias is None for m in members for layer in m.layers):
            raise ValueError("from_members: members must carry biases")
        hidden = [s[0] for s in shapes[0][:-1]]
        rate = dropout if dropout is not None else (members[0].dropout.p if isinstance(members[0].dropout, nn.Dropout)
                                                    else members[0].dropout)
        net = cls(shapes[0][0][1], [s[-1][0] for s in shapes], hidden, dropout=rate).to(members[0].layers[0].weight.device)
        F, L = net.in_channels, len(net.layers) - 1
        with torch.no_grad():
            net.layers[L].weight.zero_()
            net.layers[L].bias.zero_()
            for g, m in enumerate(members):
                h1 = hidden[0]
                net.layers[0].weight[:, g * F:(g + 1) * F].copy_(m.layers[0].weight)
                net.layers[0].bias[g * h1:(g + 1) * h1].copy_(m.layers[0].bias)
                for i in range(1, L + 1):
                    w0, n, _ = net._member(i, g)
                    net.layers[i].weight[w0:w0 + n].copy_(m.layers[i].weight)
                    net.layers[i].bias[w0:w0 + n].copy_(m.layers[i].bias)
        return net

    @torch.no_grad()
    def export_members(self) -> List[nn.Module]:
        """K `MLP(in_channels, C_k, hidden, dropout)` holding COPIES of the members' parameters, in this network's training
        mode: what MLP_label.py trains one by one."""
        F, L, out = self.in_channels, len(self.layers) - 1, []
        for g, c in enumerate(self.class_counts):
            m = models.MLP(F, c, list(self.hidden), dropout=self.dropout.p).to(self.layers[0].weight.device)
            h1 = self.hidden[0]
            m.layers[0].weight.copy_(self.layers[0].weight[:, g * F:(g + 1) * F])
            m.layers[0].bias.copy_(self.layers[0].bias[g * h1:(g + 1) * h1])
            for i in range(1, L + 1):
                w0, n, _ = self._member(i, g)
                m.layers[i].weight.copy_(self.layers[i].weight[w0:w0 + n])
                m.layers[i].bias.copy_(self.layers[i].bias[w0:w0 + n])
            out.append(m.train(self.training))
        return out
