"""Device-side scores of the K-member networks: macro-F1 and accuracy per member without a host round trip.

The reference scores every member on the host (old/h_o_train.py:116-122: `f1_score(average="macro")` on the validation
rows, `accuracy_score` on the training rows, once per member and epoch).  Both need three numbers per class -- `tp[c]`,
`n_pred[c]`, `n_true[c]` -- so the product here is `counts`, int32 [K, 3, C] with the planes in that order:

    member_class_counts    the members of a sweep cell: `pred` int32 [N, K] and a bit per member and row (libtgcn.so
                           `tgcn_class_counts_members`; `CrossValGCN.score`)
    grouped_class_counts   the per-label form: `pred` int64 [N], one member per row (`tgcn_class_counts_groups`;
                           `PerLabelGCN.score`, `PerLabelMLP.score`, and without groups the flat network,
                           `FlatLoop.epoch_scored`)
    scores                 counts -> `Scores(accuracy, f1_macro, n_rows, n_labels)`, float64 [K] each on the device
                           (`tgcn_class_scores`)
    Scoreboard             a device buffer [epochs, members, columns] that `record` fills without a synchronisation;
                           `to_host()` is the one synchronisation of a whole run

macro-F1 is sklearn's: the mean of `2 tp / (n_pred + n_true)` over the classes that occur in the predictions or in the
targets of the selected rows, NaN when there is none; accuracy is `sum tp / sum n_true`, NaN for a member without a row.
A prediction outside [0, C) (the -1 of a route of -1) is a miss: it counts in `n_true` only.
"""
from __future__ import annotations

import weakref
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .plan import _require_cuda, _stream_ptr

# how tgcn_class_counts_* tile their work (include/tgcn.h: TGCN_CLASS_COUNTS_*); the tests place their shapes with these
ROWS_PER_WORKGROUP = 256             # rows of one tile
WORKGROUP_CAP = 1024                 # workgroups that walk the row tiles, at most
LDS_BUDGET_BYTES = 48 * 1024         # the LDS table of one workgroup, at most
PARTIAL_BUDGET_BYTES = 64 << 20      # the workgroups' partial tables together, at most (or one workgroup's)
MAX_CLASSES = 4096
MAX_MEMBERS = 64

Scores = namedtuple("Scores", ["accuracy", "f1_macro", "n_rows", "n_labels"])

_CHECKED: dict = {}


def _check_once(tensors: Sequence[Tensor], extra, bad_target) -> None:
    """Run `bad_target()` (-> None or an offending class index; one device sync) once per set of tensor OBJECTS and
    versions, as `functional._member_stats` / `_group_stats` do: labels, bits, masks and groups are static across epochs.
    Never inside a HIP-graph capture (the eager warm-up step with the same tensors has checked)."""
    if torch.cuda.is_current_stream_capturing():
        return
    key = tuple(id(t) for t in tensors) + tuple(extra)
    versions = tuple(t._version for t in tensors)
    hit = _CHECKED.get(key)
    if hit is not None and all(r() is t for r, t in zip(hit[0], tensors)) and hit[1] == versions:
        return
    bad = bad_target()
    if bad is not None:
        raise IndexError(f"Target {bad} is out of bounds for {extra[-1]} classes (on a row selected for scoring)")
    try:
        drop = lambda _, k=key: _CHECKED.pop(k, None)
        _CHECKED[key] = (tuple(weakref.ref(t, drop) for t in tensors), versions)
    except TypeError:
        pass


def _first_bad(target: Tensor, selected: Tensor, C: int):
    bad = ((target < 0) | (target >= C)) & selected
    return int(target[bad][0].item()) if bool(bad.any().item()) else None


def _sizes(K: int, C: int, who: str) -> None:
    if not 1 <= K <= MAX_MEMBERS or not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"{who}: {K} members (1..{MAX_MEMBERS}) of {C} classes (1..{MAX_CLASSES})")


def _workspace(lib, n: int, K: int, C: int, device) -> Tensor:
    return torch.empty(max(lib.tgcn_class_counts_workspace_bytes(n, K, C), 16), dtype=torch.uint8, device=device)


def member_class_counts(pred: Tensor, target: Tensor, bits: Tensor, n_classes: int, also: Optional[Tensor] = None):
    """`counts` int32 [K, 3, C] (planes tp, n_pred, n_true) of the K members of a sweep cell: row r counts for member k
    where bit k of `bits[r]` (int64, `crossval.member_bits` / `fold_bits`) is set, with the prediction `pred[r, k]` (int32
    [N, K], `member_masked_cross_entropy(..., return_pred=True)`) and the shared class `target[r]` (int64).  `also`: a
    second row set (the validation rows next to the training rows), counted in the same pass -- the call then returns the
    pair `(counts, counts_also)`.  A selected row's target must lie in [0, n_classes): IndexError before the launch
    (checked once per tensor objects).  One launch pair, no synchronisation."""
    lib = _lib.load()
    _require_cuda(pred, "pred")
    if pred.dim() != 2 or pred.dtype != torch.int32:
        raise TypeError("pred must be an int32 [N, K] tensor")
    n, K = pred.shape
    C = int(n_classes)
    _sizes(K, C, "member_class_counts")
    sets = [bits] + ([also] if also is not None else [])
    if target.shape != (n,) or target.dtype != torch.int64 or any(b.shape != (n,) or b.dtype != torch.int64 for b in sets):
        raise TypeError("target, bits and also must be int64 tensors with one entry per row of pred")
    if pred.stride(1) != 1 or (n > 1 and pred.stride(0) < K):
        pred = pred.contiguous()
    low = -1 if K == 64 else (1 << K) - 1

    def bad_target():
        union = sets[0] if len(sets) == 1 else sets[0] | sets[1]
        return _first_bad(target, (union & low) != 0, C)
    _check_once([target] + sets, (K, C), bad_target)
    target = target.contiguous()
    sets = [b.contiguous() for b in sets]
    dev = pred.device
    out = [torch.empty(K, 3, C, dtype=torch.int32, device=dev) for _ in sets]
    ws = _workspace(lib, n, K, C, dev)
    _lib.check(lib.tgcn_class_counts_members(
        pred.data_ptr(), max(pred.stride(0), K) if n > 1 else K, target.data_ptr(), sets[0].data_ptr(),
        sets[1].data_ptr() if len(sets) == 2 else None, n, K, C, out[0].data_ptr(),
        out[1].data_ptr() if len(sets) == 2 else None, ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
    return (out[0], out[1]) if also is not None else out[0]


def grouped_class_counts(pred: Tensor, target: Tensor, mask: Tensor, n_classes: int, group: Optional[Tensor] = None,
                         n_groups: int = 1, pred_offset: Optional[Tensor] = None, also: Optional[Tensor] = None):
    """`counts` int32 [K, 3, C] of the per-label form: row r belongs to member `group[r]` (int32; -1 = none; without
    `group` every row belongs to member 0, the flat network), its predicted class is `pred[r] - pred_offset[group[r]]`
    (`pred` int64 [N] and the `seg_start` of `grouped_masked_cross_entropy`'s prediction as an int32 [K] device tensor;
    without it `pred` holds classes), its class `target[r]` the LOCAL one.  `mask` (bool [N]) selects the rows; `also` is a
    second mask counted in the same pass (the call then returns a pair).  `n_classes` is the widest member's; the planes of
    a narrower member are zero beyond its width.  A selected row's target must lie in [0, n_classes): IndexError before the
    launch (checked once per tensor objects)."""
    lib = _lib.load()
    _require_cuda(pred, "pred")
    if pred.dim() != 1 or pred.dtype != torch.int64:
        raise TypeError("pred must be an int64 [N] tensor")
    n, K, C = pred.numel(), int(n_groups), int(n_classes)
    _sizes(K, C, "grouped_class_counts")
    sets = [mask] + ([also] if also is not None else [])
    if target.shape != (n,) or target.dtype != torch.int64:
        raise TypeError("target must be an int64 tensor with one entry per row")
    if any(m.shape != (n,) or m.dtype not in (torch.bool, torch.uint8) for m in sets):
        raise TypeError("mask and also must be bool tensors with one entry per row")
    if group is not None and (group.shape != (n,) or group.dtype != torch.int32):
        raise TypeError("group must be an int32 tensor with one entry per row")
    if group is None and K != 1:
        raise ValueError("grouped_class_counts: without `group` every row belongs to member 0 (n_groups = 1)")
    if pred_offset is not None and (pred_offset.shape != (K,) or pred_offset.dtype != torch.int32
                                    or pred_offset.device != pred.device):
        raise TypeError("pred_offset must be an int32 [n_groups] tensor on pred's device")

    def bad_target():
        sel = sets[0].bool() if len(sets) == 1 else sets[0].bool() | sets[1].bool()
        if group is not None:
            sel = sel & (group >= 0) & (group < K)
        return _first_bad(target, sel, C)
    _check_once([target] + sets + ([group] if group is not None else []), (K, C), bad_target)
    pred, target = pred.contiguous(), target.contiguous()
    sets = [m.contiguous() for m in sets]
    group = None if group is None else group.contiguous()
    pred_offset = None if pred_offset is None else pred_offset.contiguous()
    dev = pred.device
    out = [torch.empty(K, 3, C, dtype=torch.int32, device=dev) for _ in sets]
    ws = _workspace(lib, n, K, C, dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.tgcn_class_counts_groups(
        pred.data_ptr(), ptr(pred_offset), target.data_ptr(), ptr(group), sets[0].data_ptr(),
        sets[1].data_ptr() if len(sets) == 2 else None, n, K, C, out[0].data_ptr(),
        out[1].data_ptr() if len(sets) == 2 else None, ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
    return (out[0], out[1]) if also is not None else out[0]


def scores(counts: Tensor) -> Scores:
    """`Scores(accuracy, f1_macro, n_rows, n_labels)` of `counts` [K, 3, C]: four float64 [K] device tensors (columns of
    one [K, 4] buffer).  One launch, no synchronisation."""
    lib = _lib.load()
    _require_cuda(counts, "counts")
    if counts.dim() != 3 or counts.size(1) != 3 or counts.dtype != torch.int32:
        raise TypeError("counts must be an int32 [K, 3, C] tensor")
    K, _, C = counts.shape
    _sizes(K, C, "scores")
    counts = counts.contiguous()
    out = torch.empty(K, 4, dtype=torch.float64, device=counts.device)
    _lib.check(lib.tgcn_class_scores(counts.data_ptr(), K, C, out.data_ptr(), _stream_ptr(counts.device)))
    return Scores(out[:, 0], out[:, 1], out[:, 2], out[:, 3])


class Scoreboard:
    """The scores of a whole run on the device: a float64 buffer [n_epochs, n_members, len(columns)] (NaN until written)
    and a device-side cursor.  `record(col=tensor [K], ...)` writes one epoch with plain torch ops -- no synchronisation,
    legal inside a HIP-graph capture, where every replay fills the next epoch -- and `to_host()` is the one synchronisation
    of the run.  Epochs recorded beyond `n_epochs` overwrite the last one (the cursor saturates; eager calls raise)."""

    def __init__(self, n_epochs: int, n_members: int, columns: Sequence[str], device="cuda"):
        self.columns = tuple(columns)
        if int(n_epochs) < 1 or int(n_members) < 1 or not self.columns or len(set(self.columns)) != len(self.columns):
            raise ValueError("Scoreboard needs at least one epoch, one member and distinct column names")
        self.n_epochs, self.n_members = int(n_epochs), int(n_members)
        self.buffer = torch.full((self.n_epochs, self.n_members, len(self.columns)), float("nan"), dtype=torch.float64,
                                 device=device)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=device)
        self._eager = 0

    def record(self, **cols: Tensor) -> None:
        """One epoch: a tensor [n_members] (any real dtype, on the board's device) per column, all columns at once."""
        if set(cols) != set(self.columns):
            raise ValueError(f"Scoreboard.record takes exactly the columns {list(self.columns)}")
        if not (self.buffer.is_cuda and torch.cuda.is_current_stream_capturing()):
            if self._eager >= self.n_epochs:
                raise IndexError(f"Scoreboard: more than {self.n_epochs} epochs recorded")
            self._eager += 1
        row = torch.stack([cols[c].detach().to(torch.float64).reshape(self.n_members) for c in self.columns], dim=1)
        self.buffer.index_copy_(0, self.cursor.clamp(max=self.n_epochs - 1), row.unsqueeze(0))
        self.cursor.add_(1)

    def to_host(self) -> np.ndarray:
        """The recorded epochs as a numpy array [epochs recorded, n_members, len(columns)]: ONE synchronisation."""
        buf = torch.empty(self.buffer.shape, dtype=torch.float64).pin_memory()
        cur = torch.empty(1, dtype=torch.int64).pin_memory()
        buf.copy_(self.buffer, non_blocking=True)
        cur.copy_(self.cursor, non_blocking=True)
        torch.cuda.current_stream(self.buffer.device).synchronize()
        return buf.numpy()[:min(int(cur[0]), self.n_epochs)].copy()

    def fold_summary(self, column: str, n_folds: int, epoch: int = -1, host: Optional[np.ndarray] = None):
        """`(mean, std)`, two arrays [n_members / n_folds]: `column` of one recorded epoch (default: the last) over each
        block of `n_folds` consecutive members -- the reference's result table (old/h_o_train.py:125-131).  `host`: what
        `to_host()` returned (default: it is called, one synchronisation)."""
        k = int(n_folds)
        if k < 1 or self.n_members % k:
            raise ValueError(f"fold_summary: {self.n_members} members are no whole number of blocks of {n_folds} folds")
        host = self.to_host() if host is None else host
        s = host[epoch, :, self.columns.index(column)].reshape(self.n_members // k, k)
        return s.mean(1), s.std(1)
