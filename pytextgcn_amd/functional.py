"""Fused training-step operators around the GCN (the caller of the path, flat_amazon.py:82,99-106).

`masked_cross_entropy(logits, target, mask)` equals
`CrossEntropyLoss(reduction='mean')(logits[mask], target[mask])` -- what the reference computes at
flat_amazon.py:101-102 (train) and :110 (validation) -- but runs as ONE HIP kernel over the full
[N, C] logits (libtgcn.so `tgcn_masked_ce`) that also produces the gradient, instead of boolean-mask
indexing + log_softmax + nll_loss and their backward kernels.
"""
from __future__ import annotations

import ctypes

import torch
from torch import Tensor

from . import _lib
from .plan import _require_cuda, _stream_ptr, alloc_padded, note_colsum, note_zero_rows, padded_base

_COUNT_CACHE: dict = {}


def _mask_count(mask: Tensor) -> int:
    """Rows selected by a (static) mask; one device sync per distinct mask OBJECT and version.  Keyed
    by id() and validated through a weak reference: a data pointer is no identity (the allocator hands
    the storage of a dead temporary to the next one)."""
    import weakref
    key = id(mask)
    hit = _COUNT_CACHE.get(key)
    if hit is not None and hit[0]() is mask and hit[1] == mask._version:
        return hit[2]
    count = int(mask.sum().item())
    try:
        ref = weakref.ref(mask, lambda _, k=key: _COUNT_CACHE.pop(k, None))
    except TypeError:
        return count
    _COUNT_CACHE[key] = (ref, mask._version, count)
    return count


_TARGET_OK: dict = {}


def _check_targets(target: Tensor, mask: Tensor, C: int) -> None:
    """Class indices of the selected rows must lie in [0, C): torch raises for anything else (its
    `ignore_index` is not implemented here), and the kernel would otherwise index outside the row.
    Labels and masks are static across epochs (text2graph.py:180-191), so the check -- one device sync
    -- runs once per (target, mask) object pair and version."""
    import weakref
    key = (id(target), id(mask), C)
    hit = _TARGET_OK.get(key)
    if hit is not None and hit[0]() is target and hit[1]() is mask and hit[2] == (target._version, mask._version):
        return
    bad = ((target < 0) | (target >= C)) & mask
    if bool(bad.any().item()):
        t = int(target[bad][0].item())
        raise IndexError(f"Target {t} is out of bounds for {C} classes (on a row selected by the mask)")
    try:
        _TARGET_OK[key] = (weakref.ref(target, lambda _, k=key: _TARGET_OK.pop(k, None)),
                           weakref.ref(mask, lambda _, k=key: _TARGET_OK.pop(k, None)),
                           (target._version, mask._version))
    except TypeError:
        pass


def _launch(logits: Tensor, target: Tensor, mask: Tensor, want_grad: bool, count=None, want_pred: bool = False):
    lib = _lib.load()
    _require_cuda(logits, "logits")
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError("logits must be a 2-D float32 tensor")
    n, C = logits.shape
    if target.shape != (n,) or mask.shape != (n,):
        raise ValueError("target and mask must have one entry per logits row")
    if mask.dtype != torch.bool:
        raise TypeError("mask must be a bool tensor")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    if torch.cuda.is_current_stream_capturing():
        pass                                   # no sync inside a HIP-graph capture: checked on the eager warm-up step
    else:
        _check_targets(target, mask, C)
    target = target.long().contiguous()
    mask = mask.contiguous()
    if count is None:
        count = _mask_count(mask)
    inv = 1.0 / count if count else float("nan")          # torch: mean over an empty selection = nan
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    pred = torch.empty(n, dtype=torch.int64, device=logits.device) if want_pred else None
    if want_grad:
        # loss, gradient and the column sums of the gradient (the last layer's bias gradient) in one pass
        # rows of 4 j floats (zero pad columns) when C is not a multiple of 4: the backward propagate step then takes the
        # gradient as it is instead of padding a copy; its column sums are kept at the padded width for the same reason
        dlogits = alloc_padded(n, C, logits.device)
        C4 = (C + 3) & ~3
        dbias = torch.zeros(C4, dtype=torch.float32, device=logits.device)[:C] if C4 != C else \
            torch.empty(C, dtype=torch.float32, device=logits.device)
        ws_bytes = lib.tgcn_masked_ce_grad_workspace_bytes(n, C)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=logits.device)
        _lib.check(lib.tgcn_masked_ce_grad(
            logits.data_ptr(), logits.stride(0), n, C, target.data_ptr(), mask.data_ptr(),
            ctypes.c_float(inv), loss.data_ptr(), dlogits.data_ptr(), dlogits.stride(0), dbias.data_ptr(),
            pred.data_ptr() if pred is not None else None,
            ws.data_ptr(), ws_bytes, _stream_ptr(logits.device)))
        return loss, (dlogits, dbias), pred
    ws_bytes = lib.tgcn_masked_ce_workspace_bytes()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=logits.device)
    _lib.check(lib.tgcn_masked_ce_pred(
        logits.data_ptr(), logits.stride(0), n, C, target.data_ptr(), mask.data_ptr(),
        ctypes.c_float(inv), loss.data_ptr(), None, C,
        pred.data_ptr() if pred is not None else None,
        ws.data_ptr(), ws_bytes, _stream_ptr(logits.device)))
    return loss, None, pred


def _scale_by_device_scalar(x: Tensor, scale: Tensor) -> None:
    """x *= scale for a one-element float32 device tensor `scale`; a no-op on the device when it is exactly 1."""
    _lib.check(_lib.load().tgcn_scale_by_device_scalar(x.data_ptr(), x.numel(), scale.data_ptr(),
                                                       _stream_ptr(x.device)))
    torch.autograd.graph.increment_version(x)


class _MaskedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor, mask: Tensor, count, want_pred: bool):
        loss, grads, pred = _launch(logits.detach(), target, mask, ctx.needs_input_grad[0], count, want_pred)
        ctx.save_for_backward(*(grads if grads is not None else ()))
        ctx.mask, ctx.mask_version = mask, mask._version      # (the zero-row note below is only true for THIS version)
        if not want_pred:
            return loss
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, grad_out: Tensor, *_):
        dlogits, dbias = ctx.saved_tensors
        # dlogits is ours: scale it in place (no second N x C pass) -- which makes this node single-use:
        # a second backward through it (retain_graph=True) would compound the scale, so it is refused
        if getattr(ctx, "_tgcn_used", False):
            raise RuntimeError("masked_cross_entropy: backward was already run through this loss (its gradient "
                               "buffer is scaled in place); recompute the loss instead of retain_graph=True")
        ctx._tgcn_used = True
        base = padded_base(dlogits, (dlogits.size(1) + 3) & ~3)       # the zero-padded buffer behind an odd class width
        if grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.numel() == 1:
            # `loss.backward()` seeds this node with 1: the kernel reads the scalar and leaves at once.  (The kernel
            # walks a flat buffer: the padded one where there is one -- its pad columns are and stay zero.)
            _scale_by_device_scalar(base if base is not None else dlogits, grad_out)
            _scale_by_device_scalar(dbias, grad_out)
        else:
            dlogits.mul_(grad_out)
            dbias.mul_(grad_out)
        # the layer that produced the logits finds its bias gradient ready (plan.colsum) -- under the padded buffer too
        if base is not None:                  # (view and buffer share one address: one note, under the padded form)
            note_colsum(base, torch.as_strided(dbias, (base.size(1),), (1,)))     # dbias was cut from zeros(C4)
        else:
            note_colsum(dlogits, dbias)
        # every row the mask does not select is exactly zero (the kernel wrote 0.f there; scaling keeps it): the propagate
        # step that takes this gradient may skip those operand rows (plan.known_nonzero_rows)
        # -- unless the caller edited the mask in place since the forward pass: the gradient's zero pattern is the OLD
        # mask's, so no note is left and the consumer gathers every row
        if ctx.mask._version == ctx.mask_version:
            note_zero_rows(base if base is not None else dlogits, ctx.mask)
        return dlogits, None, None, None, None


def masked_cross_entropy(logits: Tensor, target: Tensor, mask: Tensor, count=None, return_pred: bool = False):
    """`count` overrides the divisor (default: rows selected by `mask`); the sharded path passes the
    GLOBAL count so that per-rank losses and gradients add up to the single-device ones.
    `return_pred=True` returns `(loss, pred)` with `pred = logits.argmax(1)` for EVERY row, taken in the
    same pass: `pred[mask]` is what the reference computes on the host at flat_amazon.py:111-114."""
    if logits.requires_grad and torch.is_grad_enabled():
        return _MaskedCE.apply(logits, target, mask, count, return_pred)
    loss, _, pred = _launch(logits, target, mask, False, count, return_pred)
    return (loss, pred) if return_pred else loss


# ---------------------------------------------------------------------------------------------------------------------
# Grouped masked cross-entropy: the K losses of the per-label strategy (perlabel_amazon.py:90-155) in one pass
# ---------------------------------------------------------------------------------------------------------------------
_SEGMENTS: dict = {}


class Segments:
    """Column segments of K concatenated classifiers: host lists (validation, Python-side arithmetic) and the int32 device
    copies the kernel reads.  `Segments.of(starts, widths, device)` caches one object per distinct layout and device."""

    def __init__(self, starts, widths, device):
        self.starts, self.widths = tuple(int(s) for s in starts), tuple(int(w) for w in widths)
        if len(self.starts) != len(self.widths) or not self.starts:
            raise ValueError("seg_start and seg_width must hold one entry per group (at least one group)")
        self.K = len(self.starts)
        self.host_start = (ctypes.c_int32 * self.K)(*self.starts)
        self.host_width = (ctypes.c_int32 * self.K)(*self.widths)
        self.dev_start = torch.tensor(self.starts, dtype=torch.int32, device=device)
        self.dev_width = torch.tensor(self.widths, dtype=torch.int32, device=device)

    @staticmethod
    def of(starts, widths, device) -> "Segments":
        if isinstance(starts, Segments):
            return starts
        as_list = lambda v: v.tolist() if isinstance(v, Tensor) else list(v)       # (a device tensor: one copy, then cached)
        key = (tuple(as_list(starts)), tuple(as_list(widths)), str(device))
        hit = _SEGMENTS.get(key)
        if hit is None:
            if len(_SEGMENTS) >= 64:
                _SEGMENTS.clear()
            hit = _SEGMENTS[key] = Segments(key[0], key[1], device)
        return hit


_GROUP_STATS: dict = {}


def _group_stats(mask: Tensor, group: Tensor, target: Tensor, seg: Segments):
    """(selected rows per group [K] on the host, `keep` = mask & (group >= 0) on the device) for static masks and groups:
    one device sync per distinct (mask, group, target) objects and versions, as `_mask_count` / `_check_targets` do.  The
    same visit checks that the groups lie in [-1, K) and the targets of the selected rows in [0, width of their group)."""
    import weakref
    key = (id(mask), id(group), id(target), seg.starts, seg.widths)
    versions = (mask._version, group._version, target._version)
    hit = _GROUP_STATS.get(key)
    if hit is not None and hit[0]() is mask and hit[1]() is group and hit[2]() is target and hit[3] == versions:
        return hit[4], hit[5]
    K = seg.K
    if bool(((group < -1) | (group >= K)).any().item()):
        raise IndexError(f"group holds an index outside [-1, {K})")
    keep = mask & (group >= 0)
    gk = group[keep].long()
    width = seg.dev_width.long()[gk]
    tk = target[keep]
    bad = (tk < 0) | (tk >= width)
    if bool(bad.any().item()):
        i = int(torch.nonzero(bad)[0].item())
        raise IndexError(f"Target {int(tk[i].item())} is out of bounds for the {int(width[i].item())} classes of group "
                         f"{int(gk[i].item())} (on a row selected by the mask)")
    counts = torch.bincount(gk, minlength=K).tolist()
    try:
        drop = lambda _, k=key: _GROUP_STATS.pop(k, None)
        _GROUP_STATS[key] = (weakref.ref(mask, drop), weakref.ref(group, drop), weakref.ref(target, drop), versions, counts, keep)
    except TypeError:
        pass
    return counts, keep


_INV_COUNTS: dict = {}


def _inv_counts(counts, device) -> Tensor:
    key = (tuple(int(c) for c in counts), str(device))
    hit = _INV_COUNTS.get(key)
    if hit is None:
        if len(_INV_COUNTS) >= 64:
            _INV_COUNTS.clear()
        hit = _INV_COUNTS[key] = torch.tensor([1.0 / c if c else 0.0 for c in key[0]], dtype=torch.float32, device=device)
    return hit


def _launch_grouped(logits: Tensor, target: Tensor, mask: Tensor, group: Tensor, seg: Segments, counts, want_grad: bool,
                    want_pred: bool, route, class_map):
    lib = _lib.load()
    _require_cuda(logits, "logits")
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError("logits must be a 2-D float32 tensor")
    n, C = logits.shape
    if target.shape != (n,) or mask.shape != (n,) or group.shape != (n,) or (route is not None and route.shape != (n,)):
        raise ValueError("target, mask, group and route must have one entry per logits row")
    if mask.dtype != torch.bool or group.dtype != torch.int32 or (route is not None and route.dtype != torch.int32):
        raise TypeError("mask must be a bool tensor, group and route int32 tensors")
    if target.dtype != torch.int64:
        raise TypeError("target must be an int64 tensor")
    if class_map is not None and (class_map.dtype != torch.int64 or class_map.shape != (C,)):
        raise TypeError("class_map must be an int64 tensor with one entry per logits column")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    keep = None
    if counts is None or (want_grad and not torch.cuda.is_current_stream_capturing()):
        # (no sync inside a HIP-graph capture: pass `counts`; the check ran on the eager warm-up step.  A forward-only call
        # that brings its counts is not checked on the host: the kernel never reads outside a row, a class index outside
        # the segment makes the group's loss NaN)
        own, keep = _group_stats(mask, group, target, seg)
        counts = own if counts is None else counts
    if len(counts) != seg.K:
        raise ValueError("counts must hold one entry per group")
    inv = _inv_counts(counts, logits.device)
    target, mask, group = target.contiguous(), mask.contiguous(), group.contiguous()
    route = None if route is None else route.contiguous()
    class_map = None if class_map is None else class_map.contiguous()
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    loss_k = torch.empty(seg.K, dtype=torch.float32, device=dev)
    pred = torch.empty(n, dtype=torch.int64, device=dev) if want_pred else None
    dlogits = dbias = None
    if want_grad:
        dlogits = alloc_padded(n, C, dev)
        C4 = (C + 3) & ~3
        dbias = torch.zeros(C4, dtype=torch.float32, device=dev)[:C] if C4 != C else \
            torch.empty(C, dtype=torch.float32, device=dev)
    ws_bytes = lib.tgcn_grouped_ce_workspace_bytes(n, C, seg.K)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.tgcn_grouped_ce(
        logits.data_ptr(), logits.stride(0), n, C, seg.K, seg.host_start, seg.host_width, seg.dev_start.data_ptr(),
        seg.dev_width.data_ptr(), group.data_ptr(), ptr(route), target.data_ptr(), mask.data_ptr(), inv.data_ptr(),
        ptr(class_map), loss.data_ptr(), loss_k.data_ptr(), ptr(dlogits), dlogits.stride(0) if want_grad else C,
        ptr(dbias), ptr(pred), ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
    return loss, loss_k, (dlogits, dbias) if want_grad else None, pred, keep


class _GroupedCE(torch.autograd.Function):
    """Built like `_MaskedCE`: the gradient buffer is scaled in place by the incoming device scalar (single use), and the
    backward leaves the column sums and the zero rows of the gradient for the propagate step that consumes it."""

    @staticmethod
    def forward(ctx, logits, target, mask, group, seg, counts, want_pred, route, class_map):
        loss, loss_k, grads, pred, keep = _launch_grouped(logits.detach(), target, mask, group, seg, counts,
                                                          ctx.needs_input_grad[0], want_pred, route, class_map)
        ctx.save_for_backward(*(grads if grads is not None else ()))
        ctx.keep = keep
        ctx.versions = (mask, mask._version, group, group._version)
        if not want_pred:
            ctx.mark_non_differentiable(loss_k)
            return loss, loss_k
        ctx.mark_non_differentiable(loss_k, pred)        # (one call: a second one would replace the first)
        return loss, loss_k, pred

    @staticmethod
    def backward(ctx, grad_out: Tensor, *_):
        # (asked before the saved tensors are: torch would refuse them with a message about an in-place edit)
        if getattr(ctx, "_tgcn_used", False):
            raise RuntimeError("grouped_masked_cross_entropy: backward was already run through this loss (its gradient "
                               "buffer is scaled in place); recompute the loss instead of retain_graph=True")
        ctx._tgcn_used = True
        dlogits, dbias = ctx.saved_tensors
        base = padded_base(dlogits, (dlogits.size(1) + 3) & ~3)
        if grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.numel() == 1:
            _scale_by_device_scalar(base if base is not None else dlogits, grad_out)
            _scale_by_device_scalar(dbias, grad_out)
        else:
            dlogits.mul_(grad_out)
            dbias.mul_(grad_out)
        if base is not None:
            note_colsum(base, torch.as_strided(dbias, (base.size(1),), (1,)))
        else:
            note_colsum(dlogits, dbias)
        # rows outside mask & (group >= 0) are exactly zero -- true for the mask and groups of the forward pass only
        mask, mv, group, gv = ctx.versions
        if ctx.keep is not None and mask._version == mv and group._version == gv:
            note_zero_rows(base if base is not None else dlogits, ctx.keep)
        return (dlogits,) + (None,) * 8


def grouped_masked_cross_entropy(logits: Tensor, target: Tensor, mask: Tensor, group: Tensor, seg_start, seg_width,
                                 counts=None, return_pred: bool = False, route: Tensor = None, class_map: Tensor = None):
    """The K losses of the per-label strategy (perlabel_amazon.py:130-137, one `CrossEntropyLoss('mean')` per top-level
    label) on the concatenated logits of the K classifiers, as ONE HIP kernel (libtgcn.so `tgcn_grouped_ce`).

    Row r is trained on the column segment `[seg_start[k], seg_start[k] + seg_width[k])` of its group `k = group[r]` (int32;
    -1 = none) with the LOCAL class `target[r]` (int64, read where `mask[r]` and `group[r] >= 0`).  Returns `(loss, loss_k)`:
    `loss_k[k] = CrossEntropyLoss('mean')(logits[sel_k][:, seg_k], target[sel_k])` with `sel_k = mask & (group == k)` (NaN
    for an empty selection, as torch's mean over nothing) and `loss` = the sum of the others -- the objective whose
    gradient is the K separate trainings' gradients side by side.  `loss` carries the gradient; `loss_k` is for reporting.

    `seg_start` / `seg_width`: sequences of ints (or a `Segments`): increasing, non-overlapping, width >= 1; gaps allowed.
    `counts`: the selected rows per group when the caller knows them (default: counted once per mask / group object).
    `return_pred=True` adds `pred` (int64 [N]): `seg_start[q] + argmax(logits[r, seg_q])` with `q = route[r]` (default: the
    group; eval_perlabel.py:73 routes by the top-level classifier's label), mapped through `class_map` (int64 [n_cols],
    column -> global class: the `mapping` of perlabel_amazon.py:107) when given, -1 where `q` is -1."""
    seg = Segments.of(seg_start, seg_width, logits.device)
    if logits.requires_grad and torch.is_grad_enabled():
        return _GroupedCE.apply(logits, target, mask, group, seg, counts, return_pred, route, class_map)
    loss, loss_k, _, pred, _ = _launch_grouped(logits, target, mask, group, seg, counts, False, return_pred, route, class_map)
    return (loss, loss_k, pred) if return_pred else (loss, loss_k)


# ---------------------------------------------------------------------------------------------------------------------
# Member masked cross-entropy: the K losses of one sweep cell (old/h_o_train.py: learning rates x KFold) in one pass
# ---------------------------------------------------------------------------------------------------------------------
_MEMBER_STATS: dict = {}


def _member_stats(bits: Tensor, target: Tensor, K: int, C: int, cached_only: bool = False):
    """(selected rows per member [K] on the host, `keep` = `bits != 0` on the device) for static bits and targets:
    one device sync per distinct (bits, target) objects and versions, as `_group_stats` does.  The same visit checks that
    the targets of the selected rows lie in [0, C).  `cached_only` (inside a HIP-graph capture): None instead of a visit."""
    import weakref
    key = (id(bits), id(target), K, C)
    versions = (bits._version, target._version)
    hit = _MEMBER_STATS.get(key)
    if hit is not None and hit[0]() is bits and hit[1]() is target and hit[2] == versions:
        return hit[3], hit[4]
    if cached_only:
        return None
    shifts = torch.arange(K, dtype=torch.int64, device=bits.device)
    member = ((bits.unsqueeze(1) >> shifts) & 1).bool()                  # [N, K]
    keep = bits != 0
    tk = target[member.any(1)]
    bad = (tk < 0) | (tk >= C)
    if bool(bad.any().item()):
        raise IndexError(f"Target {int(tk[bad][0].item())} is out of bounds for {C} classes (on a row selected by a member)")
    counts = member.sum(0).tolist()
    try:
        drop = lambda _, k=key: _MEMBER_STATS.pop(k, None)
        _MEMBER_STATS[key] = (weakref.ref(bits, drop), weakref.ref(target, drop), versions, counts, keep)
    except TypeError:
        pass
    return counts, keep


def _launch_member(logits: Tensor, target: Tensor, bits: Tensor, K: int, C: int, S: int, counts, want_grad: bool,
                   want_pred: bool):
    lib = _lib.load()
    _require_cuda(logits, "logits")
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError("logits must be a 2-D float32 tensor")
    n, n_cols = logits.shape
    if not 1 <= K <= 64 or C < 1 or S < C or n_cols != K * S:
        raise ValueError(f"member_masked_cross_entropy: logits of {n_cols} columns do not hold {K} members (1..64) of {C} "
                         f"classes at a stride of {S} columns (n_members * seg_stride columns, seg_stride >= n_classes)")
    if target.shape != (n,) or bits.shape != (n,):
        raise ValueError("target and bits must have one entry per logits row")
    if target.dtype != torch.int64 or bits.dtype != torch.int64:
        raise TypeError("target and bits must be int64 tensors (bit k of bits[r]: row r is selected for member k)")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    keep = None
    if counts is None or want_grad:
        # no sync inside a HIP-graph capture: there the counts, the range check and the zero-row mask are those of the
        # eager warm-up step with the same `bits` and `target` objects (or the caller's `counts`)
        stats = _member_stats(bits, target, K, C, cached_only=torch.cuda.is_current_stream_capturing())
        if stats is not None:
            keep = stats[1]
            counts = stats[0] if counts is None else counts
        elif counts is None:
            raise RuntimeError("member_masked_cross_entropy inside a HIP-graph capture: run one eager step with the same "
                               "`bits` and `target` tensors first, or pass `counts`")
    if len(counts) != K:
        raise ValueError("counts must hold one entry per member")
    inv = _inv_counts(counts, logits.device)
    target, bits = target.contiguous(), bits.contiguous()
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    loss_k = torch.empty(K, dtype=torch.float32, device=dev)
    pred = torch.empty(n, K, dtype=torch.int32, device=dev) if want_pred else None
    dlogits = dbias = None
    if want_grad:
        dlogits = alloc_padded(n, n_cols, dev)
        C4 = (n_cols + 3) & ~3
        dbias = torch.zeros(C4, dtype=torch.float32, device=dev)[:n_cols] if C4 != n_cols else \
            torch.empty(n_cols, dtype=torch.float32, device=dev)
    ws_bytes = lib.tgcn_member_ce_workspace_bytes(n, K, C)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.tgcn_member_ce(
        logits.data_ptr(), logits.stride(0), n, K, C, S, target.data_ptr(), bits.data_ptr(), inv.data_ptr(),
        loss.data_ptr(), loss_k.data_ptr(), ptr(dlogits), dlogits.stride(0) if want_grad else n_cols, ptr(dbias), ptr(pred),
        ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
    return loss, loss_k, (dlogits, dbias) if want_grad else None, pred, keep


class _MemberCE(torch.autograd.Function):
    """Built like `_GroupedCE`: the gradient buffer is scaled in place by the incoming device scalar (single use), and the
    backward leaves the column sums and the zero rows of the gradient for the propagate step that consumes it."""

    @staticmethod
    def forward(ctx, logits, target, bits, K, C, S, counts, want_pred):
        loss, loss_k, grads, pred, keep = _launch_member(logits.detach(), target, bits, K, C, S, counts,
                                                         ctx.needs_input_grad[0], want_pred)
        ctx.save_for_backward(*(grads if grads is not None else ()))
        ctx.keep = keep
        ctx.versions = (bits, bits._version)
        if not want_pred:
            ctx.mark_non_differentiable(loss_k)
            return loss, loss_k
        ctx.mark_non_differentiable(loss_k, pred)
        return loss, loss_k, pred

    @staticmethod
    def backward(ctx, grad_out: Tensor, *_):
        if getattr(ctx, "_tgcn_used", False):
            raise RuntimeError("member_masked_cross_entropy: backward was already run through this loss (its gradient "
                               "buffer is scaled in place); recompute the loss instead of retain_graph=True")
        ctx._tgcn_used = True
        dlogits, dbias = ctx.saved_tensors
        base = padded_base(dlogits, (dlogits.size(1) + 3) & ~3)
        if grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.numel() == 1:
            _scale_by_device_scalar(base if base is not None else dlogits, grad_out)
            _scale_by_device_scalar(dbias, grad_out)
        else:
            dlogits.mul_(grad_out)
            dbias.mul_(grad_out)
        if base is not None:
            note_colsum(base, torch.as_strided(dbias, (base.size(1),), (1,)))
        else:
            note_colsum(dlogits, dbias)
        # rows with bits == 0 are exactly zero -- true for the bits of the forward pass only
        bits, bv = ctx.versions
        if ctx.keep is not None and bits._version == bv:
            note_zero_rows(base if base is not None else dlogits, ctx.keep)
        return (dlogits,) + (None,) * 7


def member_masked_cross_entropy(logits: Tensor, target: Tensor, bits: Tensor, n_members: int, n_classes: int,
                                seg_stride: int, counts=None, return_pred: bool = False):
    """The K losses of one cell of the reference's sweeps (old/h_o_train.py: every learning rate x every fold of KFold trains
    its own two-layer GCN on the same graph) on the concatenated logits of the K members, as ONE HIP kernel (libtgcn.so
    `tgcn_member_ce`).

    Member k owns the columns `[k * seg_stride, k * seg_stride + n_classes)` of `logits` [N, n_members * seg_stride] and
    selects row r where bit k of `bits[r]` (int64, `crossval.member_bits` / `fold_bits`) is set; `target` (int64 [N]) is
    shared by the members and read where `bits[r] != 0`.  Returns `(loss, loss_k)`: `loss_k[k] =
    CrossEntropyLoss('mean')(logits[sel_k][:, seg_k], target[sel_k])` (NaN for a member without a selected row) and `loss` =
    the sum of the others -- the objective whose gradient is the K separate trainings' gradients side by side.  `loss`
    carries the gradient; `loss_k` is for reporting.

    `counts`: the selected rows per member when the caller knows them (default: counted once per bits / target object, with
    the range check of the targets; never inside a HIP-graph capture).  `return_pred=True` adds `pred` (int32 [N, K]): the
    local arg-max of every member on EVERY row, first index on ties."""
    K, C, S = int(n_members), int(n_classes), int(seg_stride)
    if logits.requires_grad and torch.is_grad_enabled():
        return _MemberCE.apply(logits, target, bits, K, C, S, counts, return_pred)
    loss, loss_k, _, pred, _ = _launch_member(logits, target, bits, K, C, S, counts, False, return_pred)
    return (loss, loss_k, pred) if return_pred else (loss, loss_k)
