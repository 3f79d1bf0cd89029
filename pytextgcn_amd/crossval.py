"""One cell of the reference's hyper-parameter sweeps (old/h_o_train.py, h_o_train_dbpedia.py, h_o_hierarchical.py,
h_o_lables.py) as ONE network.

Every sweep builds one graph per `max_df` and then, for every dropout value, trains `len(lrs) x k_split` two-layer `GCN`s
on it (h_o_train.py: 4 learning rates x `KFold(3)`, 500 epochs each).  The members of such a cell differ in their initial
weights, their training rows (the fold) and their learning rate; they share the graph, the operator, the features, the
labels and the class count.  So the K trainings are, in exact arithmetic, one training of `PerLabelGCN` with
`class_counts = [C] * K` whose

    loss   = sum_k CE_mean(Zcat[rows bit k selects, segment k], labels)      functional.member_masked_cross_entropy
    update = Adam with lr[k] on member k's column blocks                     MemberAdam (libtgcn.so `tgcn_adam_members`)

A document is a training row of k - 1 folds and a validation row of the remaining one, so the rows of a member are a BIT of
an int64 per node (`member_bits`, `fold_bits`) instead of the one group per row the per-label strategy has.  The dropout
rate is one more axis of the members: `CrossValGCN(dropout=[...])` takes a rate per member, so the whole grid of one graph
-- `len(dropouts) x len(lrs) x k_split` members, `grid_members` lays them out -- trains as one network.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor, nn
from torch.optim import Optimizer

from . import _lib, functional
from .perlabel import PerLabelGCN
from .plan import _stream_ptr

MAX_MEMBERS = 64                      # one bit of an int64 per member


def _bit(k: int) -> int:
    """bit k of a 64-bit word as the int64 that holds it (bit 63 is the sign)"""
    return (1 << k) - (1 << 64) if k == 63 else 1 << k


def member_bits(masks: Sequence[Tensor]) -> Tensor:
    """int64 [N] from K bool masks [N] (K <= 64): bit k of entry r is set where `masks[k][r]` is -- the `bits` of
    `functional.member_masked_cross_entropy`.  On the masks' device."""
    masks = list(masks)
    if not 1 <= len(masks) <= MAX_MEMBERS:
        raise ValueError(f"member_bits takes 1..{MAX_MEMBERS} masks, got {len(masks)}")
    first = torch.as_tensor(masks[0])
    out = torch.zeros(first.shape, dtype=torch.int64, device=first.device)
    for k, m in enumerate(masks):
        m = torch.as_tensor(m)
        if m.dtype != torch.bool or m.shape != first.shape or m.dim() != 1:
            raise ValueError("member_bits: every mask must be a bool tensor with one entry per node")
        out |= torch.where(m, _bit(k), 0).to(torch.int64)
    return out


def fold_bits(doc_rows, folds, n_nodes: int, n_repeats: int = 1):
    """`(train_bits, val_bits)`, two int64 [n_nodes] tensors, from the folds of a cross-validation over the documents.

    `doc_rows` [D]: the node row of every document (h_o_train.py splits `np.arange(len(docs))` and shifts by the vocabulary
    size).  `folds`: one entry per fold, indices INTO `doc_rows` -- either the validation indices alone or the `(train,
    validation)` pair `sklearn.model_selection.KFold.split` yields (this package does not import sklearn).  The validation
    rows of member f are fold f, its training rows the fold's complement among the documents (the pair's first array when
    one is given).  Word rows stay 0.  `n_repeats` = L lays the k folds out L times, member `l * k + f` (one block of folds
    per learning rate)."""
    rows = np.asarray(torch.as_tensor(doc_rows).cpu()).astype(np.int64).ravel()
    folds = list(folds)
    k, L = len(folds), int(n_repeats)
    if k < 1 or L < 1 or k * L > MAX_MEMBERS:
        raise ValueError(f"fold_bits: {k} folds x {L} repeats must give 1..{MAX_MEMBERS} members")
    if rows.size and (rows.min() < 0 or rows.max() >= n_nodes):
        raise ValueError("fold_bits: doc_rows must lie in [0, n_nodes)")
    train = np.zeros(int(n_nodes), dtype=np.uint64)
    val = np.zeros(int(n_nodes), dtype=np.uint64)
    for f, fold in enumerate(folds):
        pair = isinstance(fold, (tuple, list)) and len(fold) == 2 and all(np.ndim(a) == 1 for a in fold)
        va = np.asarray(fold[1] if pair else fold).astype(np.int64).ravel()
        if pair:
            tr = np.asarray(fold[0]).astype(np.int64).ravel()
        else:
            keep = np.ones(rows.size, dtype=bool)
            keep[va] = False
            tr = np.nonzero(keep)[0]
        for rep in range(L):
            bit = np.uint64(1) << np.uint64(rep * k + f)
            train[rows[tr]] |= bit
            val[rows[va]] |= bit
    return torch.from_numpy(train.view(np.int64)), torch.from_numpy(val.view(np.int64))


def grid_members(lrs: Sequence[float], dropouts: Sequence[float], n_folds: int):
    """`(member_lrs, member_dropouts)` of the whole grid of one graph: two lists of `len(dropouts) * len(lrs) * n_folds`
    entries.  Member `(d * len(lrs) + l) * n_folds + f` belongs to dropout d, rate l and fold f -- the order in which
    `fold_bits(..., n_repeats=len(dropouts) * len(lrs))` lays the folds out."""
    lrs, dropouts, k = [float(v) for v in lrs], [float(v) for v in dropouts], int(n_folds)
    if not lrs or not dropouts or k < 1:
        raise ValueError("grid_members: need at least one learning rate, one dropout value and one fold")
    if len(dropouts) * len(lrs) * k > MAX_MEMBERS:
        raise ValueError(f"grid_members: {len(dropouts)} dropout values x {len(lrs)} rates x {k} folds are more than "
                         f"{MAX_MEMBERS} members")
    member_lrs = [lr for _ in dropouts for lr in lrs for _ in range(k)]
    member_dropouts = [p for p in dropouts for _ in lrs for _ in range(k)]
    return member_lrs, member_dropouts


class CrossValGCN(PerLabelGCN):
    """K two-layer `GCN(in_channels, out_channels, n_hidden_gcn=h, dropout=...)` of one sweep cell as one network: a
    `PerLabelGCN` with `class_counts = [out_channels] * n_members` (its layers, `forward(g, rows=None)`, fused dropout under
    `enable_fused_dropout` and activation reuse are inherited unchanged).  Member k owns the columns [k h, (k + 1) h) of
    layer 1 and the segment [k S, k S + C) of layer 2, S = `seg_stride` = C rounded up to 4.

    `loss` / `evaluate` take the members' rows as bits (`member_bits`, `fold_bits`); `MemberAdam` gives every member its own
    learning rate; `dropout` is a float or one rate per member (`PerLabelGCN`).  Out of scope: `n_gcn != 2`, an activation,
    `ShardedGCN`."""

    def __init__(self, in_channels, out_channels, n_members, n_hidden_gcn=64, dropout=0.5):
        K = int(n_members)
        if not 1 <= K <= MAX_MEMBERS:
            raise ValueError(f"CrossValGCN takes 1..{MAX_MEMBERS} members, got {n_members}")
        super().__init__(in_channels, [int(out_channels)] * K, n_hidden_gcn=n_hidden_gcn, dropout=dropout)
        self.out_channels = int(out_channels)

    @property
    def n_members(self) -> int:
        return self.n_groups

    @property
    def seg_stride(self) -> int:
        return (self.out_channels + 3) & ~3

    def loss(self, g, target, bits, counts=None, return_pred=False, rows=None):
        """`member_masked_cross_entropy` of `self(g, rows)`: `(loss, loss_k[, pred])` -- `loss` the sum of the members'
        `CrossEntropyLoss('mean')` on the rows their bit of `bits` selects (it carries the gradient), `loss_k` [K] the
        member losses."""
        return functional.member_masked_cross_entropy(self(g, rows), target, bits, self.n_members, self.out_channels,
                                                      self.seg_stride, counts, return_pred)

    @torch.no_grad()
    def evaluate(self, g, target, val_bits, counts=None, rows=None):
        """The eval forward (no dropout, whatever mode the network is in; the mode is put back): `(val_loss_k [K], pred
        [N, K])` -- every member's validation loss on the rows its bit of `val_bits` selects and its local arg-max on every
        row, from which the reference takes its F1 on the host."""
        was = self.training
        self.eval()
        try:
            _, loss_k, pred = functional.member_masked_cross_entropy(self(g, rows), target, val_bits, self.n_members,
                                                                     self.out_channels, self.seg_stride, counts, True)
        finally:
            self.train(was)
        return loss_k, pred

    @torch.no_grad()
    def score(self, g, target, train_bits, val_bits, counts=None, rows=None):
        """`evaluate` with the scores taken on the device: `(val_loss_k [K], train_scores, val_scores)`, two
        `metrics.Scores(accuracy, f1_macro, n_rows, n_labels)` of float64 [K] device tensors -- every member's scores on the
        rows its bit of `train_bits` / `val_bits` selects (old/h_o_train.py:116-122 reads the training accuracy and the
        validation macro-F1).  One eval forward, one `tgcn_member_ce` with predictions, one count launch for both row sets
        and two score launches; no host round trip (`counts`: the validation rows per member, as in `evaluate`)."""
        from . import metrics
        val_loss_k, pred = self.evaluate(g, target, val_bits, counts, rows)
        c_train, c_val = metrics.member_class_counts(pred, target, train_bits, self.out_channels, also=val_bits)
        return val_loss_k, metrics.scores(c_train), metrics.scores(c_val)

    @classmethod
    def from_members(cls, members: Sequence[nn.Module], dropout=None) -> "CrossValGCN":
        """One network from K two-layer `GCN`s of equal input, hidden and class width.  Parameters are copied.  `dropout`
        (a float or K floats) overrides the members' rates; without it the network keeps one float when the members'
        rates are all equal and the K rates when they differ."""
        members = list(members)
        if not members:
            raise ValueError("from_members: no member")
        if any(len(m.layers) != 2 for m in members):
            raise ValueError("from_members: members must be two-layer GCNs")
        w1, w2 = members[0].layers[0].weight, members[0].layers[1].weight
        if any(m.layers[0].weight.shape != w1.shape or m.layers[1].weight.shape != w2.shape for m in members) \
                or w2.size(0) != w1.size(1):
            raise ValueError("from_members: members must be two-layer GCNs of equal input, hidden and class width")
        if any(layer.bias is None for m in members for layer in m.layers):
            raise ValueError("from_members: members must carry biases")
        h, C = w1.size(1), w2.size(1)
        net = cls(w1.size(0), C, len(members), n_hidden_gcn=h, dropout=cls._rates_of(members, dropout)).to(w1.device)
        first, second = net.layers
        with torch.no_grad():
            second.weight.zero_()
            second.bias.zero_()
            for k, (m, s) in enumerate(zip(members, net.seg_start)):
                first.weight[:, k * h:(k + 1) * h].copy_(m.layers[0].weight)
                first.bias[k * h:(k + 1) * h].copy_(m.layers[0].bias)
                second.weight[:, s:s + C].copy_(m.layers[1].weight)
                second.bias[s:s + C].copy_(m.layers[1].bias)
        return net


class MemberAdam(Optimizer):
    """`optim.Adam` for a `CrossValGCN` with one learning rate per member: `lrs` is a float or K floats (h_o_train.py sweeps
    `lr in [0.1, 0.05, 0.01, 0.001]`).  The members are column blocks of the network's four tensors -- width h in layer 1's
    weight and bias, the segment stride in layer 2's -- and one `tgcn_adam_members` pass per tensor gives every block its
    rate; block k after a step is bit for bit what `optim.Adam(lr=lrs[k])` gives member k alone.  The state is that of
    `optim.Adam` (`step`, `exp_avg`, `exp_avg_sq`[, `max_exp_avg_sq`]; with `capturable=True` the step count lives on the
    device and `scalars` holds K + 1 floats)."""

    def __init__(self, net: CrossValGCN, lrs, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 capturable=False):
        if not isinstance(net, CrossValGCN):
            raise TypeError("MemberAdam updates a CrossValGCN")
        K = net.n_members
        lrs = [float(lrs)] * K if isinstance(lrs, (int, float)) else [float(v) for v in lrs]
        if len(lrs) != K:
            raise ValueError(f"MemberAdam: {len(lrs)} learning rates for {K} members")
        if min(lrs) < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        first, second = net.layers
        self.n_members = K
        self._width = {id(first.weight): net.n_hidden, id(first.bias): net.n_hidden,
                       id(second.weight): net.seg_stride, id(second.bias): net.seg_stride}
        super().__init__(net.parameters(), dict(lr=tuple(lrs), betas=betas, eps=eps, weight_decay=weight_decay,
                                                amsgrad=amsgrad, capturable=capturable))

    def fuse_into_backward(self, param) -> None:
        raise NotImplementedError(
            "MemberAdam.fuse_into_backward: the update fused into the backward SpMM (tgcn_spmm_adam) takes ONE learning "
            "rate for the whole tensor; the members of a CrossValGCN have one each.  Call step() after backward instead.")

    def _state_of(self, p, group):
        st = self.state[p]
        cap = group.get("capturable", False)
        if not st:
            st["step"] = torch.zeros((), dtype=torch.int64, device=p.device) if cap else 0
            if cap:
                st["scalars"] = torch.zeros(self.n_members + 1, dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if group["amsgrad"]:
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st, cap

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        K = self.n_members
        for group in self.param_groups:
            b1, b2 = group["betas"]
            lrs = group["lr"]
            lrs = [float(lrs)] * K if isinstance(lrs, (int, float)) else [float(v) for v in lrs]
            if len(lrs) != K:
                raise ValueError(f"MemberAdam: {len(lrs)} learning rates for {K} members")
            lr_host = (ctypes.c_double * K)(*lrs)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("pytextgcn_amd.crossval.MemberAdam handles contiguous float32 GPU parameters only "
                                       "(there is no CPU fallback)")
                if p.grad.is_sparse:
                    raise RuntimeError("MemberAdam does not support sparse gradients")
                width = self._width.get(id(p))
                if width is None:
                    raise RuntimeError("MemberAdam: a parameter that is not one of the network's four tensors")
                st, cap = self._state_of(p, group)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                vmax = st.get("max_exp_avg_sq")
                n_cols = p.size(-1)
                n_rows = p.numel() // n_cols if n_cols else 0
                head = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                        vmax.data_ptr() if vmax is not None else None, n_rows, n_cols, width, K, lr_host, b1, b2,
                        group["eps"], group["weight_decay"])
                if cap:
                    _lib.check(lib.tgcn_adam_members_capturable(*head, st["step"].data_ptr(), st["scalars"].data_ptr(),
                                                                _stream_ptr(p.device)))
                else:
                    st["step"] += 1
                    _lib.check(lib.tgcn_adam_members(*head, st["step"], _stream_ptr(p.device)))
                torch.autograd.graph.increment_version(p)
        return loss

