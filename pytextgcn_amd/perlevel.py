"""What perlevel_amazon.py / perlevel_dbpedia.py do between their two levels, with the graph built ONCE.

The scripts train a level-1 `GCN` on the top labels, then a level-2 `GCN` on the features [I_N | H] with H the one-hot of
the documents' top label (perlevel_amazon.py:112,122), and test it with H swapped for the softmax of the level-1 logits
(:110,156).  They call `Text2GraphTransformer.fit_transform` three times (:71,:122,:156) although only `x` changes, and
the test-time H travels device -> host -> `np.zeros([N, Fh])` -> sparse COO -> device.  Here:

    g  = t2g.fit_transform(docs, y_top, test_idx=..., val_idx=...).to(device)       # the one graph
    ... train the level-1 model on g ...
    g2 = with_hierarchy(g, one_hot_hierarchy(g, y_top), y=y_nodes)                  # :112,122 -- same edges, same plan
    ... train the level-2 model on g2 ...
    g3 = with_hierarchy(g2, predicted_hierarchy(level1, g))                         # :110,156 -- never leaves the device

The scripts use the same `max_df` (and `min_df`, `window_size`) for both levels, so both levels see one vocabulary and one
set of edges and ONE graph serves them.  Levels built with different vocabularies are different graphs: build two, and
give each its own features (`h_row0` is then each graph's own `n_vocab`)."""
from __future__ import annotations

import torch

from .data import Data
from .hier import HierarchyFeatures


def _n_vocab(g) -> int:
    n_vocab = getattr(g, "n_vocab", None)
    if n_vocab is None:
        raise ValueError("the graph carries no `n_vocab` (the first document row); Text2GraphTransformer sets it")
    return int(n_vocab)


def _edge_device(g):
    return g.edge_index.device


def one_hot_hierarchy(g, y_top, n_classes=None) -> HierarchyFeatures:
    """[I_N | H] with H the one-hot of the documents' top labels (perlevel_amazon.py:112): `y_top` has one integer entry
    per document (the rows g.n_vocab .. N - 1).  `n_classes` None: the largest label + 1.  Lives on the graph's device."""
    h_row0, n = _n_vocab(g), int(g.num_nodes)
    y_top = torch.as_tensor(y_top)
    if y_top.dim() != 1 or y_top.numel() != n - h_row0:
        raise ValueError(f"one_hot_hierarchy: y_top has {tuple(y_top.shape)} entries, the graph has {n - h_row0} documents")
    return HierarchyFeatures(n, h_row0, classes=y_top, n_classes=n_classes).to(_edge_device(g))


def predicted_hierarchy(model, g) -> HierarchyFeatures:
    """[I_N | H] with H = softmax(model(g)[g.n_vocab:], dim=1) (perlevel_amazon.py:110): the level-1 model's class
    probabilities of every document, computed in eval mode without autograd.  The rows stay on the device; the model's
    training flag is restored."""
    h_row0 = _n_vocab(g)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            probs = torch.softmax(model(g)[h_row0:].float(), dim=1).contiguous()
    finally:
        model.train(was_training)
    return HierarchyFeatures(int(g.num_nodes), h_row0, dense=probs)


# ---------------------------------------------------------------------------------------------------------------------
# The same strategy for the bag-of-words baseline: MLP_level.py trains every level after the first on
# `append_feats(x, one_hot(labels of the level above))` (mlp_helper.py:141-151; MLP_level.py:112-122), rebuilding the sparse
# tensor on the host per split and per level.  Here x stays ONE tensor on the device and the appended blocks are ids:
#
#     x_train = csr_to_torch(...).to(device)                                     # the one upload
#     ... train level1 = MLP(F, C1, [256, 128]) on x_train ...
#     x2_train = append_classes(x_train, y_train[0], C1)                         # :120 -- ids, no new sparse tensor
#     x2_test = append_classes(x_test, predicted_classes(level1, x_test), C1)    # :85,122 -- never leaves the device
#     ... train level2 = MLP(F + C1, C2, [256, 128]) on x2_train ...
#     x3_train = append_classes(x2_train, y_train[1], C2)                        # DBpedia's third level: [X | H1 | H2]
# ---------------------------------------------------------------------------------------------------------------------
class AppendedFeatures:
    """The matrix `[X | H_1 | ... | H_S]` of `append_feats`: `base` is the sparse COO tensor X [N, F] -- the SAME object at
    every level, so the SpMM plan cached for it serves them all -- and `ids` int32 [N, S] holds, per appended one-hot block,
    the row's column in the STACKED blocks (block s starts at `sum(blocks[:s])`; -1: the row has no entry in that block).
    `blocks` are the blocks' widths.  `MLP.forward` takes it in place of the sparse tensor; `to_sparse()` is that tensor.
    Built by `append_classes`."""

    is_sparse = False                 # not a torch sparse tensor: `MLP` and `conv.features_times` ask the type

    def __init__(self, base: torch.Tensor, ids: torch.Tensor, blocks):
        blocks = tuple(int(b) for b in blocks)
        if not isinstance(base, torch.Tensor) or not base.is_sparse or base.dim() != 2:
            raise TypeError("AppendedFeatures: `base` must be a 2-D sparse COO tensor (csr_to_torch's)")
        if ids.dim() != 2 or ids.size(0) != base.size(0) or ids.size(1) != len(blocks) or not blocks or min(blocks) < 1:
            raise ValueError(f"AppendedFeatures: ids {tuple(ids.shape)} must be [N = {base.size(0)}, one column per block] "
                             f"and every block at least one column wide (blocks {blocks})")
        if ids.dtype != torch.int32 or ids.device != base.device:
            raise TypeError("AppendedFeatures: `ids` must be an int32 tensor on the base's device")
        lo = torch.tensor((0,) + blocks[:-1], device=ids.device).cumsum(0)
        hi = torch.tensor(blocks, device=ids.device).cumsum(0)
        ids = torch.where((ids >= lo) & (ids < hi), ids, torch.full_like(ids, -1))     # outside its block: nothing
        self.base, self.ids, self.blocks = base, ids.contiguous(), blocks
        self.n_base = int(base.size(1))
        self.n_appended = sum(blocks)
        self._sparse = None

    @property
    def shape(self):
        return torch.Size((self.base.size(0), self.n_base + self.n_appended))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self) -> int:
        return 2

    @property
    def is_cuda(self) -> bool:
        return self.base.is_cuda

    @property
    def device(self):
        return self.base.device

    @property
    def dtype(self):
        return self.base.dtype

    def to(self, device) -> "AppendedFeatures":
        """The features on `device`; `self` when they live there already (the base stays the same object)."""
        device = torch.device(device)
        if device.type == self.device.type and (device.index is None or device.index == self.device.index):
            return self
        return AppendedFeatures(self.base.to(device), self.ids.to(device), self.blocks)

    def float(self) -> "AppendedFeatures":
        return self if self.base.dtype == torch.float32 else AppendedFeatures(self.base.float(), self.ids, self.blocks)

    def to_sparse(self) -> torch.Tensor:
        """The coalesced sparse COO [N, F + sum(blocks)] tensor `append_feats` returns, built once and kept."""
        if self._sparse is None:
            base = self.base.coalesce()
            rows = torch.arange(self.ids.size(0), device=self.device).unsqueeze(1).expand_as(self.ids)
            ids = self.ids.long()
            held = ids >= 0
            idx = torch.stack([rows[held], ids[held] + self.n_base])
            val = torch.ones(idx.size(1), dtype=base.dtype, device=self.device)
            self._sparse = torch.sparse_coo_tensor(torch.cat([base.indices(), idx], dim=1), torch.cat([base.values(), val]),
                                                   tuple(self.shape)).coalesce()
        return self._sparse


def append_classes(x, ids, n_classes: int) -> AppendedFeatures:
    """`append_feats(x, one_hot(ids, n_classes))` (MLP_level.py:112-122) without building a tensor: `x` is the sparse COO
    feature matrix or an `AppendedFeatures` (the call chains, as the script's does), `ids` one integer class per row -- an
    id outside [0, n_classes) gives a row of zeros, what OneHotEncoder(handle_unknown="ignore") would."""
    ids = torch.as_tensor(ids)
    if ids.dim() != 1 or ids.size(0) != x.size(0):
        raise ValueError(f"append_classes: ids has {tuple(ids.shape)} entries, the features have {x.size(0)} rows")
    if torch.is_floating_point(ids) or int(n_classes) < 1:
        raise ValueError("append_classes: `ids` must be integers and n_classes at least 1")
    base, old, blocks = (x.base, x.ids, x.blocks) if isinstance(x, AppendedFeatures) else (x, None, ())
    ids = ids.to(base.device).long()
    col = torch.where((ids >= 0) & (ids < int(n_classes)), ids + sum(blocks), torch.full_like(ids, -1)).to(torch.int32)
    col = col.unsqueeze(1)
    return AppendedFeatures(base, col if old is None else torch.cat([old, col], dim=1), blocks + (int(n_classes),))


def predicted_classes(model, x) -> torch.Tensor:
    """The arg-max of `model(x)` per row (MLP_level.py:85,171) in eval mode without autograd: int64 [N] on the features'
    device.  The model's training flag is restored."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            return model(x).argmax(dim=1)
    finally:
        model.train(was_training)


def with_hierarchy(g, feats, y=None) -> Data:
    """A shallow copy of `g` whose `x` is `feats` (and whose `y` is `y`, when given): `edge_index`, `edge_attr`, the masks
    and every other attribute are the SAME objects, so the normalised operator cached for `g` (`plan_for`) serves the copy
    too -- nothing about the graph is rebuilt."""
    if feats.size(0) != g.num_nodes:
        raise ValueError(f"with_hierarchy: the features have {feats.size(0)} rows, the graph {g.num_nodes} nodes")
    out = Data()
    out.__dict__.update(g.__dict__)
    out.x = feats
    if y is not None:
        out.y = y
    return out
