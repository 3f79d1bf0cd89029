"""GCN, EGCN, JumpingKnowledgeNetwork and MLP: drop-ins for `textgcn.lib.models.GCN` (textgcn/lib/models.py:6-25), `.EGCN`
(:28-52), `.JumpingKnowledgeNetwork` (:55-81) and `.MLP` (:83-102; the last two: their docstrings below).  For GCN and EGCN:

Same constructor signature and defaults, same `layers` ModuleList (state_dict keys
`layers.{i}.weight` (in, out) / `layers.{i}.bias`), same forward: dropout between layers, none
after the last, and by default NO activation -- the reference's activation call is commented out
(models.py:22) although `self.activation` is constructed (models.py:9); both facts are kept.

`apply_activation=True` (an extension, last keyword) restores that line: `x = layer(x); x = activation(x);
x = dropout(x)` between the layers, nothing after the last -- the two-layer GCN with a ReLU of Kipf & Welling and of
the TextGCN paper.  `nn.ReLU` runs in the epilogue of the first layer's SpMM kernel (pytextgcn_amd/conv.py); any other
module is called on the layer's output.  `pytextgcn_amd.sharded.ShardedGCN` has no such switch: its narrow exchange rests
on the network being linear.
"""
from __future__ import annotations

import torch
from torch import nn

from . import dense, embed, hier, mlp
from .conv import (GCNConv, _feature_plan, _pad_cols, dense_hierarchy_block, features_times, is_sparse_identity, propagate,
                   split_identity_block)
from .jk import JumpingKnowledge
from .perlevel import AppendedFeatures
from .plan import _require_cuda

# Opt-in: the reference network has no non-linearity (models.py:22 is commented out) and dropout is the
# identity in eval mode, so without autograd the L-layer forward
#     x_i = M (x_{i-1} W_i) + b_i
# equals   z_0 = X (W_1 W_2 ... W_L);  z_i = M z_{i-1} + b_i (W_{i+1} ... W_L)
# -- L propagations at the width of the OUTPUT (C classes) instead of one at every hidden width, and no
# N x h intermediate.  Same value up to fp32 rounding (different association), hence off by default
# and excluded from the bitwise tests; parity against the oracle is checked at the 1e-5 bar.
_COLLAPSE = False


def enable_linear_collapse(on: bool = True) -> None:
    global _COLLAPSE
    _COLLAPSE = bool(on)


# Opt-in: the dropout between the layers (models.py:23) fused into the next layer's x @ W and its
# autograd (libtgcn.so tgcn_gemm_*_dropout): neither the dropped activation nor its mask is stored, the
# three GEMMs regenerate the mask from an 8-byte seed.  Same distribution as torch's dropout, but the
# random stream is the library's own (seeded from torch's generator), hence off by default.
_FUSED_DROPOUT = False


def enable_fused_dropout(on: bool = True) -> None:
    global _FUSED_DROPOUT
    _FUSED_DROPOUT = bool(on)


class GCN(nn.Module):
    def __init__(self, in_channels, out_channels, n_gcn=2, n_hidden_gcn=64, activation=nn.ReLU,
                 dropout=0.5, apply_activation=False):
        super().__init__()
        self.activation = activation()
        self.apply_activation = bool(apply_activation)
        self.dropout = dropout
        self.layers = nn.ModuleList([GCNConv(in_channels, n_hidden_gcn, add_self_loops=True)])
        for _ in range(n_gcn - 2):
            self.layers.append(GCNConv(n_hidden_gcn, n_hidden_gcn, add_self_loops=True))
        self.layers.append(GCNConv(n_hidden_gcn, out_channels, add_self_loops=True))

    def _collapsed_forward(self, g, rows=None):
        layers = list(self.layers)
        tail = [None] * len(layers)            # tail[i] = W_{i+1} ... W_L (None = identity)
        for i in range(len(layers) - 2, -1, -1):
            w_next = layers[i + 1].weight
            tail[i] = w_next if tail[i + 1] is None else dense.xw(w_next, tail[i + 1])
        z = layers[0].features_times(g.x, dense.xw(layers[0].weight, tail[0]))
        for i, layer in enumerate(layers):
            b = layer.bias
            if b is not None and tail[i] is not None:
                b = dense.xw(b.unsqueeze(0), tail[i]).squeeze(0)      # a 1-row product: still no vendor GEMM
            plan = layer.plan(g.x, g.edge_index, g.edge_attr)
            if rows is not None and i == len(layers) - 1:
                plan = plan.on_rows(rows) or plan
            z = propagate(plan, z, b)
        return z

    def forward(self, g, rows=None):
        """`rows` (an extension of the reference's signature; a bool mask over the nodes that the caller keeps): the rows of
        the logits that will be READ -- `g.train_mask` in the training step (flat_amazon.py:101 indexes the output with it),
        the validation and training rows in evaluation (:109-114).  The LAST layer's propagate step then runs on the
        operator restricted to them; every other row of the result holds the last layer's bias.  In a TextGCN graph the
        word rows, which nobody reads, hold two thirds of the operator's entries."""
        # (modules pickled before `apply_activation` existed do not carry it: they are the linear network)
        act = self.activation if getattr(self, "apply_activation", False) else None
        if (_COLLAPSE and act is None and len(self.layers) > 1 and not torch.is_grad_enabled()
                and (not self.training or self.dropout == 0)):
            return self._collapsed_forward(g, rows)      # the identity it uses needs the LINEAR network
        x = g.x
        pending = 0.0                          # dropout still owed to x (fused into the next layer)
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            kw = {"rows": rows} if (rows is not None and i == last) else {}
            if act is not None and i < last:
                kw["activation"] = act
            x = layer(x, g.edge_index, g.edge_attr, input_dropout=pending, **kw) if pending > 0.0 \
                else layer(x, g.edge_index, g.edge_attr, **kw)
            pending = 0.0
            if i < len(self.layers) - 1:
                if _FUSED_DROPOUT and self.training and 0.0 < self.dropout < 1.0 and not x.is_sparse:
                    pending = float(self.dropout)
                else:
                    x = nn.functional.dropout(x, p=self.dropout, training=self.training)
        return x


# On by default: EGCN's front end on exact-identity features -- Linear, SELU, dropout and the first layer's x @ W -- as ONE
# product that never stores the N x embedding_dim activation (pytextgcn_amd/embed.py).  Off: the same arithmetic composed
# from the package's other kernels and torch's SELU / dropout, for A/B runs and tests.
_FUSED_EMBEDDING = True


def enable_fused_embedding(on: bool = True) -> bool:
    """Returns the previous setting."""
    global _FUSED_EMBEDDING
    was, _FUSED_EMBEDDING = _FUSED_EMBEDDING, bool(on)
    return was


# Opt-in: the same fused front end on [I_N | H] features (the hierarchy features of the per-level scripts,
# text2graph.py:226-246): the H term of the Linear joins the pre-activation in registers (`tgcn_embed_xw_h*`).  Off by
# default: those features then take the composition, as they always did.  `enable_fused_embedding(False)` switches
# every fused front end off, this one included.
_FUSED_HIERARCHY = False


def enable_fused_hierarchy_embedding(on: bool = True) -> bool:
    """Returns the previous setting."""
    global _FUSED_HIERARCHY
    was, _FUSED_HIERARCHY = _FUSED_HIERARCHY, bool(on)
    return was


def fused_embedding_admits(x, in_features: int) -> bool:
    """The first of the two feature tests of `EGCN.takes_fused_path` (`crossval.CrossValEGCN` shares both): the fused
    front end is on and `x` is a sparse matrix or a `hier.HierarchyFeatures` of the layer's width."""
    held = isinstance(x, hier.HierarchyFeatures)           # [I | H] as class ids or dense rows: the type selects the product
    return bool(_FUSED_EMBEDDING and (x.is_sparse or held) and x.size(1) == in_features)


def fused_embedding_features(x) -> bool:
    """The second: `x` is the sparse identity, `[I | H]` under `enable_fused_hierarchy_embedding()`, or a
    `hier.HierarchyFeatures` within the cap."""
    if isinstance(x, hier.HierarchyFeatures):
        return x.n_features <= embed.max_hierarchy_features()
    if is_sparse_identity(x):
        return True
    if not _FUSED_HIERARCHY:
        return False
    h = split_identity_block(x)
    return h is not None and h.size(1) <= embed.max_hierarchy_features()


def fused_embedding_operand(x):
    """`(Hd, h_row0)` of features that pass the two tests: what `embed.embed_xw` takes as `h`, `h_row0`."""
    if isinstance(x, hier.HierarchyFeatures):
        return x.dense_block(), x.h_row0
    return (None, 0) if x.size(0) == x.size(1) else dense_hierarchy_block(split_identity_block(x))


class EmbeddingLinear(nn.Linear):
    """`layers[0]` of EGCN: torch's `nn.Linear` (same parameters, same init, same state_dict keys) whose forward runs on
    this package's kernels for every feature format of text2graph.py:226-246 -- `features_times` on `weight.t()`, plus
    bias; no torch.sparse.mm, no vendor GEMM, no CPU fallback."""

    def forward(self, x):
        _require_cuda(x, "x")
        y = features_times(x, self.weight.t(), self.in_features)
        return y if self.bias is None else y + self.bias


class EGCN(nn.Module):
    """Drop-in for `textgcn.lib.models.EGCN` (textgcn/lib/models.py:28-52): an embedding `Linear(in_channels,
    embedding_dim)`, SELU, dropout, then GCNConv layers (embedding_dim -> h, (h -> h) x (n_gcn - 2), h -> out).

    Same constructor signature and defaults, same `layers` ModuleList (`layers.0.weight` is the Linear's
    (embedding_dim, in_channels), the GCNConv keys keep PyG's (in, out) layout).  As in the reference `self.activation` is
    constructed and never applied (models.py:32,49), and the dropout ALSO FOLLOWS THE LAST LAYER: the reference's guard
    `i < len(self.layers) - 1` is evaluated while enumerating `self.layers[1:]` (models.py:46-50), so it always holds and in
    training mode the logits themselves are dropped.  Both facts are kept.  Eval mode has no dropout anywhere.

    Exact-identity features take the fused product of `pytextgcn_amd.embed` -- by default in eval mode and whenever
    `dropout` is 0; in training with 0 < dropout < 1 only while `enable_fused_dropout()` is on, because the mask is then
    drawn from the library's random stream, not torch's (the rule `GCN` follows).  Everything else, and everything after
    `enable_fused_embedding(False)`, is composed from `EmbeddingLinear`, torch's SELU and dropout, and `GCNConv`.

    After `enable_fused_hierarchy_embedding()` sparse `[I_N | H]` features (H at most `embed.max_hierarchy_features()`
    columns wide) take the fused product under the same mode and dropout rules.  A `hier.HierarchyFeatures` of that width
    takes it without that switch; a wider one is composed on its `to_sparse()`."""

    def __init__(self, in_channels, out_channels, embedding_dim=2000, n_gcn=2, n_hidden_gcn=64, activation=nn.ReLU,
                 dropout=0.5):
        super().__init__()
        self.activation = activation()
        self.dropout = dropout
        self.layers = nn.ModuleList([EmbeddingLinear(in_channels, embedding_dim),
                                     GCNConv(embedding_dim, n_hidden_gcn, add_self_loops=True)])
        for _ in range(n_gcn - 2):
            self.layers.append(GCNConv(n_hidden_gcn, n_hidden_gcn, add_self_loops=True))
        self.layers.append(GCNConv(n_hidden_gcn, out_channels, add_self_loops=True))

    def _dropout(self, x):
        return nn.functional.dropout(x, p=self.dropout, training=True) if self.training else x

    def takes_fused_path(self, x) -> bool:
        """Whether `forward` on the features `x` runs the fused embedding product (see the class docstring)."""
        p = float(self.dropout)
        if not fused_embedding_admits(x, self.layers[0].in_features):
            return False
        if self.training and p != 0.0 and not (_FUSED_DROPOUT and 0.0 < p < 1.0):
            return False
        return fused_embedding_features(x)

    def forward(self, g):
        x = g.x
        emb, first = self.layers[0], self.layers[1]
        if self.takes_fused_path(x):
            _require_cuda(x, "g.x")
            plan = first.plan(x, g.edge_index, g.edge_attr)
            hd, h_row0 = fused_embedding_operand(x)
            xw = embed.embed_xw(emb.weight, emb.bias, first.weight, float(self.dropout) if self.training else 0.0,
                                h=hd, h_row0=h_row0)
            x = propagate(plan, xw, first.bias)
        else:
            x = emb(x)
            x = torch.selu(x)
            x = self._dropout(x)
            x = first(x, g.edge_index, g.edge_attr)
        x = self._dropout(x)
        for layer in self.layers[2:]:
            x = layer(x, g.edge_index, g.edge_attr)
            x = self._dropout(x)                 # also after the last layer, as the reference does
        return x


# On by default: the hidden layers of MLP -- bias, SELU, dropout and the next Linear -- as ONE product per layer that never
# stores the activated matrix (pytextgcn_amd/mlp.py).  Off: the same arithmetic composed from `EmbeddingLinear`, torch's
# SELU and dropout, for A/B runs and tests.
_FUSED_MLP = True


def enable_fused_mlp(on: bool = True) -> bool:
    """Returns the previous setting."""
    global _FUSED_MLP
    was, _FUSED_MLP = _FUSED_MLP, bool(on)
    return was


class _AppendedFirstLayer(torch.autograd.Function):
    """The first Linear of an MLP on `[X | H]` features, split at column `n_base` of its weight W1 [h, F + Fh]:
    `Z = X @ W1[:, :F].t()` on X's plan and `T = W1[:, F:].t()` [Fh, h], the table of `mlp.act_linear_cls`.  The backward
    writes X^T @ dZ and dT into the two row ranges of ONE [F + Fh, h] buffer and returns its transpose: one gradient of
    the weight's shape, no zero-filled halves."""

    @staticmethod
    def forward(ctx, plan, W1, n_base: int):
        if W1.dtype != torch.float32:
            raise TypeError("sparse features times weight: float32 weights only (MLP_level.py casts the model with .float())")
        ctx.plan, ctx.n_base = plan, n_base
        h = W1.size(0)
        h4 = (h + 3) & ~3
        w = W1.detach()
        z = plan.spmm(_pad_cols(w[:, :n_base].t(), h4).contiguous())
        return (z if h4 == h else z[:, :h]), w[:, n_base:].t().contiguous()

    @staticmethod
    def backward(ctx, dz, dt):
        h, n_base = dz.size(1), ctx.n_base
        h4 = (h + 3) & ~3
        dwt = torch.empty(n_base + dt.size(0), h4, dtype=torch.float32, device=dz.device)
        ctx.plan.spmm(_pad_cols(dz, h4).contiguous(), transpose=True, out=dwt[:n_base])
        dwt[n_base:, :h] = dt
        return None, dwt[:, :h].t(), None


class MLP(nn.Module):
    """Drop-in for `textgcn.lib.models.MLP` (textgcn/lib/models.py:83-102), the TF-IDF bag-of-words baseline of
    MLP_flat.py / MLP_level.py / MLP_label.py: `Linear(in_channels, hidden[0])`, `Linear(hidden[i], hidden[i + 1])` ...,
    `Linear(hidden[-1], out_channels)`, with SELU and dropout after every layer but the last.

    Same constructor signature, default and assertion (`hidden` is not empty), same attributes: `dropout` is an
    `nn.Dropout`, `act` an `nn.SELU`, `layers` a ModuleList of Linear modules (`layers.{i}.weight` (out, in),
    `layers.{i}.bias`, torch's default init: a checkpoint of the reference loads with strict=True).  `forward(x)` takes
    what the reference's scripts pass: the sparse COO [N, in_channels] TF-IDF matrix of `csr_to_torch` / `append_feats`,
    or a dense tensor.  The layers are `EmbeddingLinear`s, so every product runs on this package's kernels.

    The fused path: `Z1 = x @ layers[0].weight.t()` on the existing SpMM (or dense) kernel with NO bias added, then one
    `mlp.act_linear` per remaining layer, which applies the previous layer's bias, SELU and dropout on the way into its own
    product.  Per hidden layer one N x width matrix is written once and read once, and it is the only thing of that size
    kept for the backward.  It runs in eval mode and whenever the dropout rate is 0; in training with 0 < rate < 1 only
    while `enable_fused_dropout()` is on, because the mask is then drawn from the library's random stream, not torch's
    (the rule `GCN` and `EGCN` follow).  Everything else (rate 1 in training included), and everything after
    `enable_fused_mlp(False)`, is composed from `EmbeddingLinear`, `torch.selu` and `self.dropout`.

    The per-level strategy (MLP_level.py): `forward` also takes a `perlevel.AppendedFeatures`, the matrix `[X | H_1 | H_2]`
    of `append_feats` held as the sparse X plus class ids.  On the fused path `Z1 = X @ layers[0].weight[:, :F].t()` runs
    on X's own cached plan -- the one a level-1 model on X built -- and the class columns enter the first `mlp.act_linear_cls`
    as a per-row bias, rows of `layers[0].weight[:, F:].t()`; the weight's gradient is one tensor of its shape.  The
    parameters are those of `MLP(F + Fh, ...)`.  Off the fused path, with more than two blocks or more than
    `mlp.max_class_rows()` appended columns, `forward` runs on `x.to_sparse()`."""

    def __init__(self, in_channels, out_channels, hidden, dropout=0.5):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        assert hidden
        ls = [EmbeddingLinear(in_channels, hidden[0])]
        ls += [EmbeddingLinear(h1, h2) for h1, h2 in zip(hidden, hidden[1:])]
        ls += [EmbeddingLinear(hidden[-1], out_channels)]
        self.layers = nn.ModuleList(ls)
        self.act = nn.SELU()

    def takes_fused_path(self, x) -> bool:
        """Whether `forward` runs the fused products (see the class docstring).  The answer depends on the mode, the rate
        and the switches only, never on `x`: the argument is there because GCN and EGCN have it."""
        p = float(self.dropout.p)
        if not _FUSED_MLP or any(layer.bias is None for layer in self.layers):
            return False
        return not (self.training and p != 0.0 and not (_FUSED_DROPOUT and 0.0 < p < 1.0))

    def takes_class_term(self, x) -> bool:
        """Whether `forward` on the `perlevel.AppendedFeatures` `x` runs the class columns as a per-row bias of the first
        fused product: on the fused path, with at most `mlp.MAX_CLASS_SLOTS` blocks of at most `mlp.max_class_rows()`
        columns together.  Otherwise `forward` runs on `x.to_sparse()`."""
        return (isinstance(x, AppendedFeatures) and self.takes_fused_path(x) and len(x.blocks) <= mlp.MAX_CLASS_SLOTS
                and x.n_appended <= mlp.max_class_rows() and x.size(1) == self.layers[0].in_features)

    def forward(self, x):
        _require_cuda(x, "x")
        if isinstance(x, AppendedFeatures):
            if self.takes_class_term(x):
                p = float(self.dropout.p) if self.training else 0.0
                first, second, last = self.layers[0], self.layers[1], len(self.layers) - 1
                # [X | H] @ W1.t() = X @ W1[:, :F].t() + W1[:, F:].t()[class]: the first on X's own plan, the second in the product
                z, t = _AppendedFirstLayer.apply(_feature_plan(x.base), first.weight, x.n_base)
                z = mlp.act_linear_cls(z, first.bias, second.weight, second.bias if last == 1 else None, x.ids, t, p)
                for i in range(2, len(self.layers)):
                    prev, layer = self.layers[i - 1], self.layers[i]
                    z = mlp.act_linear(z, prev.bias, layer.weight, layer.bias if i == last else None, p)
                return z
            x = x.to_sparse()
        if not self.takes_fused_path(x):
            last = len(self.layers) - 1
            for i, layer in enumerate(self.layers):
                x = layer(x)
                if i < last:
                    x = torch.selu(x)
                    x = self.dropout(x)
            return x
        p = float(self.dropout.p) if self.training else 0.0
        first = self.layers[0]
        z = features_times(x, first.weight.t(), first.in_features)
        last = len(self.layers) - 1
        for i in range(1, len(self.layers)):
            prev, layer = self.layers[i - 1], self.layers[i]
            z = mlp.act_linear(z, prev.bias, layer.weight, layer.bias if i == last else None, p)
        return z


class JumpingKnowledgeNetwork(nn.Module):
    """Drop-in for `textgcn.lib.models.JumpingKnowledgeNetwork` (textgcn/lib/models.py:55-81): `n_gcn` GCNConv layers
    (in -> h, (h -> h) x (n_gcn - 2), h -> h), `jk = JumpingKnowledge("lstm", channels=h, num_layers=n_gcn)` over their
    outputs, then `lin = Linear(h, out)`.

    Same constructor signature and defaults, same state_dict keys (`layers.{i}.*`, `jk.lstm.*`, `jk.att.*`, `lin.*`: a
    checkpoint of the reference loads with strict=True), same forward: EVERY layer is followed by dropout and the dropped
    tensor is what the aggregation sees; then `jk`, the activation -- which, unlike in `GCN` and `EGCN`, IS applied here
    (models.py:76) -- dropout, and `lin`.  `nn.ReLU` runs in the epilogue of the aggregation kernel
    (pytextgcn_amd/jk.py); any other module is called on its result.  `lin` runs on this package's kernels
    (`EmbeddingLinear`): no vendor GEMM, no CPU fallback.

    Dropout is torch's `F.dropout` throughout, drawing from torch's random stream: `enable_fused_dropout` does not apply
    to this model.  At most 8 layers (`jk.MAX_LAYERS`)."""

    def __init__(self, in_channels, out_channels, n_gcn=2, n_hidden_gcn=64, activation=nn.ReLU, dropout=0.5):
        super().__init__()
        self.activation = activation()
        self.dropout = dropout
        self.layers = nn.ModuleList([GCNConv(in_channels, n_hidden_gcn, add_self_loops=True)])
        for _ in range(n_gcn - 2):
            self.layers.append(GCNConv(n_hidden_gcn, n_hidden_gcn, add_self_loops=True))
        self.layers.append(GCNConv(n_hidden_gcn, n_hidden_gcn, add_self_loops=True))
        self.jk = JumpingKnowledge(mode="lstm", channels=n_hidden_gcn, num_layers=n_gcn)
        self.lin = EmbeddingLinear(n_hidden_gcn, out_channels)

    def forward(self, g):
        x = g.x
        acts = []
        for layer in self.layers:
            x = layer(x, g.edge_index, g.edge_attr)
            x = nn.functional.dropout(x, p=self.dropout, training=self.training)
            acts += [x]
        relu = type(self.activation) is nn.ReLU
        x = self.jk.aggregate(acts, relu=relu)
        if not relu:
            x = self.activation(x)
        x = nn.functional.dropout(x, p=self.dropout, training=self.training)
        return self.lin(x)
