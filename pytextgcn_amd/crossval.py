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

The sweeps over `models = [GCN, EGCN]` (old/h_o_hierarchical.py:33,80, h_o_lables.py:28,95) have an EGCN half: `CrossValEGCN`
is the M two-layer `EGCN`s of such a cell as one network -- the front ends of all members as ONE product
(`embed.embed_xw_members`), everything behind it as in `CrossValGCN`, and `MemberAdam` on row blocks where the members are
stacked by rows (libtgcn.so `tgcn_adam_member_rows`).
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor, nn
from torch.optim import Optimizer

from . import _lib, embed, functional, models
from .conv import GCNConv, features_times, glorot_, propagate
from .models import EmbeddingLinear
from .perlabel import BlockDiagonalConv, MemberDropoutXW, PerLabelGCN, member_rates
from .plan import _require_cuda, _stream_ptr

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


class _SweepCell:
    """What the networks of a sweep cell share: K members whose logits are the segments [k S, k S + C) of one matrix
    (`n_groups`, `out_channels` and `forward(g, rows)` are the network's)."""

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


class CrossValGCN(_SweepCell, PerLabelGCN):
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

    def member_blocks(self):
        """How `MemberAdam` finds the members in the parameters: `(row_blocks, column_blocks)`, two dicts id(parameter) ->
        size.  All four tensors of this network hold their members as column blocks."""
        first, second = self.layers
        return {}, {id(first.weight): self.n_hidden, id(first.bias): self.n_hidden,
                    id(second.weight): self.seg_stride, id(second.bias): self.seg_stride}

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


class StackedGCNConv(GCNConv):
    """`layers[1]` of `CrossValEGCN`: the M first `GCNConv(D, h)` of the members.  `weight` [M D, h] holds W_m in the ROWS
    [m D, (m + 1) D) -- the operand layout of `embed.embed_xw_members` -- and `bias` [M h] b_m in the entries
    [m h, (m + 1) h), the columns member m owns in the propagated [N, M h] activation.  `plan` is `GCNConv`'s: the
    network runs both propagate steps on it."""

    def __init__(self, n_members: int, embedding_dim: int, n_hidden: int):
        self.n_members, self.embedding_dim, self.n_hidden = int(n_members), int(embedding_dim), int(n_hidden)
        super().__init__(self.n_members * self.embedding_dim, self.n_hidden, add_self_loops=True)
        self.bias = nn.Parameter(torch.zeros(self.n_members * self.n_hidden))

    def reset_parameters(self) -> None:
        D = self.embedding_dim
        with torch.no_grad():
            for m in range(self.n_members):                # glorot of a GCNConv(D, h), member by member
                glorot_(self.weight[m * D:(m + 1) * D])
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, *args, **kwargs):
        raise RuntimeError("StackedGCNConv holds the members' parameters; CrossValEGCN.forward runs the products")

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.n_members} x ({self.embedding_dim}, {self.n_hidden}))"


def logits_dropout_columns(rates: Sequence[float], n_classes: int, seg_stride: int, device):
    """(keep, scale): float32 [K * seg_stride] on `device` -- 1 - p_k and 1 / (1 - p_k) in member k's class columns, 0 in
    its pad columns: the per-column vectors of `member_logits_dropout`."""
    keep = torch.zeros(len(rates), seg_stride, dtype=torch.float64)
    keep[:, :n_classes] = 1.0 - torch.tensor([float(p) for p in rates], dtype=torch.float64)[:, None]
    scale = torch.where(keep > 0, 1.0 / keep.clamp_min(1e-300), torch.zeros_like(keep))
    return (keep.flatten().to(device=device, dtype=torch.float32), scale.flatten().to(device=device, dtype=torch.float32))


def member_logits_dropout(z: Tensor, rates: Sequence[float], n_classes: int, seg_stride: int, columns=None) -> Tensor:
    """Training-mode inverted dropout on the members' logits `z` [N, K * seg_stride] (the reference's EGCN drops its
    logits too, textgcn/lib/models.py:46-50): member k's `n_classes` columns are dropped at `rates[k]` and the kept ones
    scaled by 1 / (1 - rates[k]).  ONE mask draw over the whole matrix from torch's random stream against a per-column
    rate vector -- four elementwise ops whatever K is.  A member at rate 0 comes back untouched; pad columns come back 0.
    `columns`: what `logits_dropout_columns` returned for these arguments (a network keeps its pair; None builds one)."""
    K = len(rates)
    if z.dim() != 2 or z.size(1) != K * seg_stride or seg_stride < n_classes:
        raise ValueError(f"member_logits_dropout: z {tuple(z.shape)} is not {K} segments of stride {seg_stride}")
    keep, scale = columns if columns is not None else logits_dropout_columns(rates, n_classes, seg_stride, z.device)
    mask = torch.rand_like(z) < keep                       # rand is in [0, 1): a column with keep = 1 keeps every entry
    return z * mask * scale


class CrossValEGCN(_SweepCell, MemberDropoutXW, nn.Module):
    """M two-layer `EGCN(in_channels, out_channels, embedding_dim=D, n_hidden_gcn=h, dropout=...)` of one sweep cell as one
    network: the EGCN half of `models = [GCN, EGCN]` in old/h_o_hierarchical.py:33,80 and old/h_o_lables.py:28,95.

    `layers[0]` is ONE `EmbeddingLinear(in_channels, M D)` -- member m owns the rows [m D, (m + 1) D) of its weight and
    bias, initialised as `nn.Linear(in_channels, D)` initialises them.  `layers[1]` is a `StackedGCNConv`: the members'
    first GCNConv weights [M D, h] stacked by rows, their biases [M h].  `layers[2]` is a `BlockDiagonalConv(h, [C] * M)`,
    as in `CrossValGCN`: member m owns the segment [m S, m S + C), S = `seg_stride`.

    `forward(g, rows=None)` follows `EGCN`'s rules.  On the sparse identity, on `[I | H]` under
    `enable_fused_hierarchy_embedding()` and on a `hier.HierarchyFeatures` within the cap -- in eval mode, at rate 0, or
    under `enable_fused_dropout()` -- the front ends of all members are ONE product (`embed.embed_xw_members`, a seed and
    a rate per member); otherwise each member's is composed from the embedding Linear, SELU and `F.dropout`.  Then one
    propagate step at width M h, the per-member dropout and layer-2 product of `PerLabelGCN` (`MemberDropoutXW`), one
    propagate step (restricted to `rows`), and in training mode the reference's dropout on the logits
    (`member_logits_dropout`).

    `loss`, `evaluate` and `score` are `CrossValGCN`'s; `MemberAdam` gives every member its own learning rate.  `dropout`
    is one rate or M rates (`grid_members`).  Out of scope: `n_gcn != 2` and `ShardedGCN`.

    Memory: the embedding weight, its gradient and Adam's two states are 4 * M * D * in_channels * 4 bytes -- 38 GB for
    M = 12 members of D = 2000 on 100 000 nodes."""

    def __init__(self, in_channels, out_channels, n_members, embedding_dim=2000, n_hidden_gcn=64, dropout=0.5, n_gcn=2, *,
                 _init_embedding: bool = True):
        """`_init_embedding=False` (what `from_members` passes) leaves the embedding Linear's parameters uninitialised: they
        are about to be overwritten, and at M D x in_channels floats their initialisation is the cost of construction."""
        super().__init__()
        M = int(n_members)
        if not 1 <= M <= MAX_MEMBERS:
            raise ValueError(f"CrossValEGCN takes 1..{MAX_MEMBERS} members, got {n_members}")
        if int(n_gcn) != 2:
            raise ValueError(f"CrossValEGCN holds two-layer EGCNs (n_gcn=2), got n_gcn={n_gcn}")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.embedding_dim, self.n_hidden = int(embedding_dim), int(n_hidden_gcn)
        self.class_counts = (self.out_channels,) * M
        self.dropout = member_rates(dropout, M, type(self).__name__)       # a float, or a tuple of M rates
        D = self.embedding_dim
        # the [M D, in] weight is initialised ONCE (nn.Linear's own constructor would do it first, for the wrong fan-out)
        emb = nn.utils.skip_init(EmbeddingLinear, self.in_channels, M * D, device=torch.get_default_device())
        if _init_embedding:
            with torch.no_grad():                          # nn.Linear(in_channels, D).reset_parameters, member by member
                bound = 1.0 / math.sqrt(self.in_channels) if self.in_channels > 0 else 0.0
                for m in range(M):
                    nn.init.kaiming_uniform_(emb.weight[m * D:(m + 1) * D], a=math.sqrt(5))
                    emb.bias[m * D:(m + 1) * D].uniform_(-bound, bound)
        self._logits_columns = None                        # (rates, device, keep, scale) of the dropout on the logits
        self.layers = nn.ModuleList([emb, StackedGCNConv(M, D, self.n_hidden),
                                     BlockDiagonalConv(self.n_hidden, self.class_counts)])

    @property
    def n_groups(self) -> int:
        return len(self.class_counts)

    @property
    def seg_start(self):
        return self.layers[2].seg_start

    @property
    def seg_width(self):
        return self.class_counts

    @property
    def n_cols(self) -> int:
        return self.layers[2].n_cols

    def _rates(self):
        return self.dropout if isinstance(self.dropout, tuple) else (float(self.dropout),) * self.n_groups

    def _drop_logits(self, z: Tensor) -> Tensor:
        """`member_logits_dropout` with the per-column vectors built once per rates and device and kept by the network."""
        rates, kept = self._rates(), self._logits_columns
        if kept is None or kept[0] != rates or kept[1] != z.device:
            columns = logits_dropout_columns(rates, self.out_channels, self.seg_stride, z.device)
            kept = self._logits_columns = (rates, z.device) + columns
        return member_logits_dropout(z, rates, self.out_channels, self.seg_stride, kept[2:])

    def takes_fused_path(self, x) -> bool:
        """Whether `forward` on the features `x` runs the fused member product: `EGCN.takes_fused_path`'s rules, with
        "rate 0" meaning every member's."""
        rates = self._rates()
        if not models.fused_embedding_admits(x, self.layers[0].in_features):
            return False
        if self.training and max(rates) != 0.0 and not (models._FUSED_DROPOUT and all(0.0 <= p < 1.0 for p in rates)):
            return False
        return models.fused_embedding_features(x)

    def member_blocks(self):
        """How `MemberAdam` finds the members in the parameters: `(row_blocks, column_blocks)`, two dicts id(parameter) ->
        size -- the elements of one member's contiguous row block, or the columns of one member's column block."""
        emb, first, second = self.layers
        D, S = self.embedding_dim, self.seg_stride
        return ({id(emb.weight): D * self.in_channels, id(emb.bias): D, id(first.weight): D * self.n_hidden},
                {id(first.bias): self.n_hidden, id(second.weight): S, id(second.bias): S})

    def _front_end(self, x) -> Tensor:
        """[N, M h]: member m's `dropout(selu(Linear_m(x))) @ W_m` in the columns [m h, (m + 1) h)."""
        emb, first = self.layers[0], self.layers[1]
        M, D, rates = self.n_groups, self.embedding_dim, self._rates()
        if self.takes_fused_path(x):
            _require_cuda(x, "g.x")
            hd, h_row0 = models.fused_embedding_operand(x)
            return embed.embed_xw_members(emb.weight, emb.bias, first.weight, M, rates if self.training else 0.0, h=hd,
                                          h_row0=h_row0)
        parts = []
        for m in range(M):
            rows = slice(m * D, (m + 1) * D)
            y = features_times(x, emb.weight[rows].t(), emb.in_features) + emb.bias[rows]
            y = nn.functional.dropout(torch.selu(y), p=rates[m], training=self.training)
            parts.append(features_times(y, first.weight[rows], D))
        return torch.cat(parts, 1)

    def forward(self, g, rows=None):
        """Zcat [N, n_cols]: the logits of member m in the columns of segment m.  `rows`: as in `PerLabelGCN.forward`."""
        from .sharded import ShardedGraph
        if isinstance(g, ShardedGraph):
            raise ValueError("CrossValEGCN runs on one device: a ShardedGraph (the graph of ShardedGCN) is out of scope")
        first, second = self.layers[1], self.layers[2]
        plan = first.plan(g.x, g.edge_index, g.edge_attr)
        x = propagate(plan, self._front_end(g.x), first.bias)
        xw = self._dropout_xw(x, second.weight)
        if rows is not None:
            plan = plan.on_rows(rows) or plan
        z = propagate(plan, xw, second.bias)
        if self.training and max(self._rates()) > 0.0:     # also after the last layer, as the reference's EGCN does
            z = self._drop_logits(z)
        return z

    @classmethod
    def from_members(cls, members: Sequence[nn.Module], dropout=None) -> "CrossValEGCN":
        """One network from M two-layer `EGCN`s of equal input, embedding, hidden and class width.  Parameters are
        copied.  `dropout` (a float or M floats) overrides the members' rates, as in `CrossValGCN.from_members`."""
        members = list(members)
        if not members:
            raise ValueError("from_members: no member")
        if any(len(m.layers) != 3 for m in members):
            raise ValueError("from_members: members must be two-layer EGCNs (n_gcn=2)")
        e, w1, w2 = (members[0].layers[i].weight for i in range(3))
        if any(m.layers[i].weight.shape != w.shape for m in members for i, w in enumerate((e, w1, w2))) \
                or w1.size(0) != e.size(0) or w2.size(0) != w1.size(1):
            raise ValueError("from_members: members must be two-layer EGCNs of equal input, embedding, hidden and class "
                             "width")
        if any(layer.bias is None for m in members for layer in m.layers):
            raise ValueError("from_members: members must carry biases")
        D, h, C = e.size(0), w1.size(1), w2.size(1)
        with torch.device(e.device):               # M D x in floats: created where they will live
            net = cls(e.size(1), C, len(members), embedding_dim=D, n_hidden_gcn=h,
                      dropout=cls._rates_of(members, dropout), _init_embedding=False)
        emb, first, second = net.layers
        with torch.no_grad():
            second.weight.zero_()
            second.bias.zero_()
            for k, (m, s) in enumerate(zip(members, net.seg_start)):
                emb.weight[k * D:(k + 1) * D].copy_(m.layers[0].weight)
                emb.bias[k * D:(k + 1) * D].copy_(m.layers[0].bias)
                first.weight[k * D:(k + 1) * D].copy_(m.layers[1].weight)
                first.bias[k * h:(k + 1) * h].copy_(m.layers[1].bias)
                second.weight[:, s:s + C].copy_(m.layers[2].weight)
                second.bias[s:s + C].copy_(m.layers[2].bias)
        return net

    @torch.no_grad()
    def export_members(self) -> List[nn.Module]:
        """M `EGCN(in_channels, out_channels, embedding_dim=D, n_hidden_gcn=h, dropout=...)` holding COPIES of the members'
        parameters, member k with its own rate, in this network's training mode."""
        emb, first, second = self.layers
        D, h, C, out = self.embedding_dim, self.n_hidden, self.out_channels, []
        for k, s in enumerate(self.seg_start):
            with torch.device(emb.weight.device):
                m = models.EGCN(self.in_channels, C, embedding_dim=D, n_hidden_gcn=h, dropout=self.member_dropout(k))
            m.layers[0].weight.copy_(emb.weight[k * D:(k + 1) * D])
            m.layers[0].bias.copy_(emb.bias[k * D:(k + 1) * D])
            m.layers[1].weight.copy_(first.weight[k * D:(k + 1) * D])
            m.layers[1].bias.copy_(first.bias[k * h:(k + 1) * h])
            m.layers[2].weight.copy_(second.weight[:, s:s + C])
            m.layers[2].bias.copy_(second.bias[s:s + C])
            out.append(m.train(self.training))
        return out


class MemberAdam(Optimizer):
    """`optim.Adam` for a `CrossValGCN` or `CrossValEGCN` with one learning rate per member: `lrs` is a float or K floats
    (h_o_train.py sweeps `lr in [0.1, 0.05, 0.01, 0.001]`).  The members are column blocks of the network's four tensors --
    width h in layer 1's weight and bias, the segment stride in layer 2's -- and one `tgcn_adam_members` pass per tensor
    gives every block its rate; block k after a step is bit for bit what `optim.Adam(lr=lrs[k])` gives member k alone.
    The state is that of `optim.Adam` (`step`, `exp_avg`, `exp_avg_sq`[, `max_exp_avg_sq`]; with `capturable=True` the step
    count lives on the device and `scalars` holds K + 1 floats).  A `CrossValEGCN` also holds members as contiguous ROW
    blocks (its stacked embedding weight and bias and its first GCNConv weight, `member_blocks`): those take
    `tgcn_adam_member_rows`, whose indices are 64-bit -- the embedding weight of a sweep cell passes 2^31 elements."""

    def __init__(self, net, lrs, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 capturable=False):
        if not isinstance(net, (CrossValGCN, CrossValEGCN)):
            raise TypeError("MemberAdam updates a CrossValGCN")
        K = net.n_members
        lrs = [float(lrs)] * K if isinstance(lrs, (int, float)) else [float(v) for v in lrs]
        if len(lrs) != K:
            raise ValueError(f"MemberAdam: {len(lrs)} learning rates for {K} members")
        if min(lrs) < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        self.n_members = K
        # the members in the parameters, as the network lays them out: contiguous row blocks (elements per member; a
        # CrossValEGCN's stacked tensors) and column blocks (columns per member)
        self._block, self._width = net.member_blocks()
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
                block, width = self._block.get(id(p)), self._width.get(id(p))
                if block is None and width is None:
                    raise RuntimeError("MemberAdam: a parameter that is not one of the network's four tensors")
                st, cap = self._state_of(p, group)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                vmax = st.get("max_exp_avg_sq")
                buffers = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                           vmax.data_ptr() if vmax is not None else None)
                if block is not None:              # row blocks: a flat tensor of K * block elements, 64-bit indices
                    head = (*buffers, p.numel(), block, K, lr_host, b1, b2, group["eps"], group["weight_decay"])
                    host, capturable = lib.tgcn_adam_member_rows, lib.tgcn_adam_member_rows_capturable
                else:
                    n_cols = p.size(-1)
                    n_rows = p.numel() // n_cols if n_cols else 0
                    head = (*buffers, n_rows, n_cols, width, K, lr_host, b1, b2, group["eps"], group["weight_decay"])
                    host, capturable = lib.tgcn_adam_members, lib.tgcn_adam_members_capturable
                if cap:
                    _lib.check(capturable(*head, st["step"].data_ptr(), st["scalars"].data_ptr(), _stream_ptr(p.device)))
                else:
                    st["step"] += 1
                    _lib.check(host(*head, st["step"], _stream_ptr(p.device)))
                torch.autograd.graph.increment_version(p)
        return loss

