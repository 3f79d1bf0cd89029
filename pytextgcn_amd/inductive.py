"""Fold-in: the logits of documents that are NOT nodes of the training graph, from a trained two-layer network.

The reference cannot do this: its `Text2GraphTransformer` has `fit_transform` only and test documents must be nodes of the
training graph (flat_amazon.py:57-71).  The arithmetic is exact, not an approximation: PyG's `gcn_norm`
sums the degree at the TARGET of an edge, so a new document d added with edges word -> d only (weighted by its TF-IDF row,
plus PyG's self loop) changes no word's or old document's degree, normalised weight or activation, and d's row of the
two-layer forward is a closed form over tables frozen from the trained model (`tgcn_foldin_two_layer`, include/tgcn.h):

    u = act( sum_j a_j T1[w_j] + a_dd s1 + b1 ),     z = sum_j a_j P[w_j] + a_dd (u W2) + b2

  * `extended_graph(g, tfidf)` is that definition as a graph: what the reference arithmetic is run on in the tests;
  * `FoldIn(model, g)` freezes dis, T1, s1, P, W2 and the biases with one eval forward and serves batches through one
    kernel launch: no plan, no sort, no synchronisation, shape-static (legal under HIP-graph capture);
  * `enable_fused_foldin(False)` composes the same definition from the package's other kernels (a plan per batch, two SpMMs,
    a dense product), for A/B runs and as a second implementation in the tests;
  * `FoldInLevels(models, graphs)` does the same for the per-level strategy (perlevel_amazon.py, perlevel_dbpedia.py; DESIGN.md
    4.2n): level l >= 2 sees [I | H] with H the link -- softmax or one-hot -- of the level above.  A new document has no
    identity column, so its row of the first layer's operand is H_d W1[N:], a C_{l-1} x h product that the ONE kernel
    (`tgcn_foldin_levels`) resolves in LDS after ONE pass over the document's words for all levels;
  * `FoldInPerLabel(top_model, net, g, class_map)` does it for the per-label strategy (perlabel_amazon.py, eval_perlabel.py;
    DESIGN.md 4.2o): the top network's arg-max routes a document to that label's own network, and ONE kernel
    (`tgcn_foldin_routed`) gathers the top network's rows and then the rows of that ONE member -- never the K h-wide row;
  * `FoldInDeep(model, g)` does it for the deeper models of the reference's surface (textgcn/lib/models.py):
    `GCN` and `EGCN` with n_gcn up to 4 and the `JumpingKnowledgeNetwork`.  The argument holds at any depth -- no old node's
    activation changes in any layer -- so d's row of layer l is a closed form over the frozen word table
    T^l = (H^{l-1} W_l)[:V] and d's own previous row, and ONE kernel (`tgcn_foldin_layers`) carries a document through all L
    layers in one pass over its words.  The JKN's LSTM aggregation, activation and `lin` are row-wise: they run on d's own L
    rows.  (The three classes above are two-layer code and keep refusing these models in their own words.)
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from . import _lib, dense, embed, hier
from .conv import is_sparse_identity, propagate, split_identity_block
from .data import Data
from .plan import GraphPlan, _require_cuda, _stream_ptr, gcn_norm_factors

# On by default: one launch of the fused kernel per batch.  Off: the composition (see the module docstring).
_FUSED_FOLDIN = True


def enable_fused_foldin(on: bool = True) -> bool:
    """Returns the previous setting."""
    global _FUSED_FOLDIN
    was, _FUSED_FOLDIN = _FUSED_FOLDIN, bool(on)
    return was


def _host_csr(tfidf, n_vocab: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(rowptr int64, col int32, val float32) of a scipy sparse matrix [B, n_vocab], checked on the host."""
    from scipy import sparse as sp
    if not sp.issparse(tfidf):
        raise TypeError(f"expected a scipy sparse matrix [n_docs, {n_vocab}] (Text2GraphTransformer.transform) or device "
                        f"tensors (rowptr int64, col int32, val float32), got {type(tfidf).__name__}")
    m = tfidf.tocsr()
    if m.shape[1] != n_vocab:
        raise ValueError(f"the TF-IDF matrix has {m.shape[1]} columns, the training graph has {n_vocab} words")
    if m.nnz and (int(m.indices.min()) < 0 or int(m.indices.max()) >= n_vocab):
        raise IndexError(f"column ids must lie in [0, {n_vocab})")
    return (np.ascontiguousarray(m.indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float32))


def extended_graph(g, tfidf, hierarchy=None) -> Data:
    """The training graph `g` plus one node per row of `tfidf` (scipy sparse [B, g.n_vocab]), each with the edges word -> new
    document of its row, appended after g's edges in CSR order; no edge leaves a new node and PyG adds its self loop.  `x`
    keeps its columns and gains B rows (the sparse identity becomes [N + B, N]) -- empty ones, or, for [I | H] features
    (`HierarchyFeatures` or sparse), with the float32 [B, Fh] block `hierarchy` in the H columns: a new document has no
    identity column.  Masks and `y` are extended with False / 0.  On g's device, host or GPU.  Running the reference arithmetic on it leaves every old row as it was and
    gives the new documents' logits: the definition `FoldIn` evaluates in closed form."""
    n_vocab = int(g.n_vocab)
    rowptr, col, val = _host_csr(tfidf, n_vocab)
    B = rowptr.shape[0] - 1
    N = g.x.size(0)
    dev = g.edge_index.device
    doc = np.repeat(np.arange(B, dtype=np.int64), np.diff(rowptr)) + N
    new_index = torch.from_numpy(np.stack([col.astype(np.int64), doc])).to(dev)
    edge_index = torch.cat([g.edge_index.long(), new_index], dim=1)
    edge_attr = g.edge_attr
    if edge_attr is None:
        edge_attr = torch.ones(g.edge_index.size(1), dtype=torch.float32, device=dev)
    edge_attr = torch.cat([edge_attr.reshape(-1).float(), torch.from_numpy(val).to(dev)])
    x = g.x
    if isinstance(x, hier.HierarchyFeatures):
        x = x.to_sparse()
    if hierarchy is not None:
        Fh = x.size(1) - N
        if not x.is_sparse or Fh < 1:
            raise ValueError("extended_graph: `hierarchy` needs [I | H] features (HierarchyFeatures or sparse [N, N + Fh])")
        hierarchy = torch.as_tensor(hierarchy)
        if tuple(hierarchy.shape) != (B, Fh) or hierarchy.dtype != torch.float32:
            raise ValueError(f"extended_graph: `hierarchy` must be float32 [{B}, {Fh}], got {hierarchy.dtype} "
                             f"{tuple(hierarchy.shape)}")
    if x.is_sparse:
        xc = x if x.is_coalesced() else x.coalesce()
        idx, v = xc.indices(), xc.values()
        if hierarchy is not None:
            hd = hierarchy.to(dev)
            nz = torch.nonzero(hd)
            idx = torch.cat([idx, torch.stack([nz[:, 0] + N, nz[:, 1] + N])], 1)
            v = torch.cat([v, hd[nz[:, 0], nz[:, 1]].to(v.dtype)])
        x = torch.sparse_coo_tensor(idx, v, (N + B, x.size(1))).coalesce()
    else:
        x = torch.cat([x, x.new_zeros(B, x.size(1))])
    out = Data(x=x, edge_index=edge_index, edge_attr=edge_attr, n_vocab=n_vocab)
    if g.y is not None:
        out.y = torch.cat([g.y, g.y.new_zeros(B)])
    for name in ("train_mask", "val_mask", "test_mask"):
        m = getattr(g, name, None)
        if m is not None:
            setattr(out, name, torch.cat([m, m.new_zeros(B)]))
    return out


def _r4(v: int) -> int:
    return (v + 3) & ~3


def _bias_of(layer, n: int, dev) -> Tensor:
    return torch.zeros(n, dtype=torch.float32, device=dev) if layer.bias is None else layer.bias.detach().float().clone()


def _check_two_layer(who: str, convs, activation, at: str = "", layers_note: str = "") -> Tuple[int, int]:
    """What both fold-in kernels ask of a network: two GCNConv layers with self loops and normalisation, ReLU or nothing
    (`activation`: the module between the layers, None where there is none).  `at` names the level in the error texts.
    Returns the widths (h, C), which `_check_widths` holds against the kernels'."""
    if len(convs) != 2:
        raise NotImplementedError(f"{who}:{at} n_gcn != 2 (the model has {len(convs)} GCNConv layers){layers_note}")
    for c in convs:
        if not (c.add_self_loops and c.normalize) or c.improved:
            raise NotImplementedError(f"{who}: GCNConv(add_self_loops=True, normalize=True, improved=False) only")
    if activation is not None and type(activation) is not nn.ReLU:
        raise NotImplementedError(f"{who}:{at} other activations than nn.ReLU are not supported "
                                  f"({type(activation).__name__})")
    return convs[0].out_channels, convs[1].out_channels


def _check_widths(who: str, h: int, C: int, at: str = "") -> None:
    lib = _lib.load()
    if h > lib.tgcn_foldin_max_hidden() or C > lib.tgcn_foldin_max_classes():
        raise NotImplementedError(f"{who}:{at} hidden width {h} / {C} classes exceed the kernel's "
                                  f"{lib.tgcn_foldin_max_hidden()} / {lib.tgcn_foldin_max_classes()}")


def _check_identity_features(who: str, x) -> None:
    """`FoldIn` and `FoldInPerLabel` take the sparse identity features of a graph on the GPU and nothing else."""
    if isinstance(x, hier.HierarchyFeatures):
        raise NotImplementedError(f"{who}: [I | H] hierarchy features (HierarchyFeatures) are not supported")
    if not x.is_sparse:
        raise NotImplementedError(f"{who}: dense features are not supported (sparse identity features only)")
    if not is_sparse_identity(x):
        if split_identity_block(x) is not None:
            raise NotImplementedError(f"{who}: [I | H] hierarchy features are not supported")
        raise NotImplementedError(f"{who}: non-identity features are not supported (sparse identity features only)")
    _require_cuda(x, "g.x")


def _doc_scalars(rowptr: Tensor, col: Tensor, val: Tensor, dis: Tensor, V: int, degree_sum: str):
    """What both `_composed` methods begin with: a_dd [B, 1] and the plan of the [B, V] matrix of a_j (None for a batch
    without entries).  deg_d comes from `tgcn_gcn_norm` on the bipartite word -> document edges (the plan's own sums, in
    edge = CSR order, the loop last).  Builds a plan per batch, which sorts and synchronises."""
    B, dev = rowptr.numel() - 1, rowptr.device
    row = torch.repeat_interleave(torch.arange(B, device=dev), rowptr[1:] - rowptr[:-1])
    c = col.long()
    dis_d = gcn_norm_factors(torch.stack([c, row + V]), val, V + B, 1, degree_sum)[0][V:]
    dw = dis[c]
    a = (dw * val) * dis_d[row] if degree_sum == "reference" else val * (dw * dis_d[row])
    a_dd = ((dis_d * 1.0) * dis_d).unsqueeze(1)
    return a_dd, (GraphPlan.from_coo(row, c, a, B, V, with_transpose=False) if c.numel() else None)


def _device_csr(tfidf, n_vocab: int, device) -> Tuple[Tensor, Tensor, Tensor]:
    """What every fold-in class takes as a batch: device tensors (rowptr int64 [B + 1], col int32, val float32), which are
    trusted, or a scipy sparse matrix [B, n_vocab], which `_host_csr` checks before the copy."""
    if isinstance(tfidf, (tuple, list)) and len(tfidf) == 3 and all(torch.is_tensor(t) for t in tfidf):
        rowptr, col, val = tfidf
        for name, t, dt in (("rowptr", rowptr, torch.int64), ("col", col, torch.int32), ("val", val, torch.float32)):
            _require_cuda(t, name)
            if t.dtype != dt or t.dim() != 1 or t.device != device or not t.is_contiguous():
                raise TypeError(f"FoldIn: `{name}` must be a contiguous 1-D {dt} tensor on {device}")
        if rowptr.numel() < 1 or col.numel() != val.numel():
            raise ValueError("FoldIn: rowptr needs n_docs + 1 entries, col and val one per stored entry")
        return rowptr, col, val
    rowptr, col, val = _host_csr(tfidf, n_vocab)
    return tuple(torch.from_numpy(a).to(device) for a in (rowptr, col, val))


class FoldIn:
    """`FoldIn(model, g)`: classify documents outside the training graph `g` with the trained `model` -- `models.GCN` (linear,
    or `apply_activation=True` with `nn.ReLU`) or `models.EGCN`, two GCNConv layers, sparse identity features.  The tables
    are frozen from the model's current parameters by one eval forward; call `refresh()` after more training.  Inputs are a
    scipy sparse matrix [B, g.n_vocab] (`Text2GraphTransformer.transform`; shape and largest column id are checked before
    the copy) or device tensors `(rowptr int64 [B + 1], col int32, val float32)`, which are trusted."""

    def __init__(self, model, g):
        self.model, self.g = model, g
        self._check(model, g)
        self.refresh()

    # -- what is supported ------------------------------------------------------------------------------------------
    @staticmethod
    def _check(model, g) -> None:
        from . import models as M
        kind = type(model)
        if kind not in (M.GCN, M.EGCN):
            from . import crossval, perlabel, sharded          # (the classes themselves, so that a renamed one cannot slip by)
            causes = (((perlabel.PerLabelGCN,), "the K-member networks: a PerLabelGCN folds in through FoldInPerLabel"),
                      ((crossval.CrossValGCN, crossval.CrossValEGCN, perlabel.PerLabelMLP), "the K-member networks"),
                      ((sharded.ShardedGCN,), "ShardedGCN: multi-GPU models"),
                      ((M.JumpingKnowledgeNetwork,), "JKN: the jumping-knowledge aggregation has no closed form here"),
                      ((M.MLP,), "MLP has no graph to fold into"))
            why = next((text for classes, text in causes if isinstance(model, classes)), "unsupported model type")
            raise NotImplementedError(f"FoldIn takes models.GCN and models.EGCN, not {kind.__name__} ({why})")
        convs = list(model.layers)[(1 if kind is M.EGCN else 0):]
        between = model.activation if (kind is M.GCN and getattr(model, "apply_activation", False)) else None
        h, C = _check_two_layer("FoldIn", convs, between, layers_note="; the closed form is the two-layer network's")
        _check_identity_features("FoldIn", g.x)
        _check_widths("FoldIn", h, C)

    # -- the frozen tables ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self) -> "FoldIn":
        """Freeze dis, T1, s1, P, W2 and the biases again from the model's current parameters (one eval forward)."""
        from . import models as M
        model, g = self.model, self.g
        egcn = type(model) is M.EGCN
        first, second = list(model.layers)[(1 if egcn else 0):]
        V, N = int(g.n_vocab), g.x.size(0)
        dev = g.x.device
        plan = first.plan(g.x, g.edge_index, g.edge_attr)
        self.degree_sum = plan.degree_sum
        self.n_vocab, self.h, self.C = V, first.out_channels, second.out_channels
        self.device = dev
        was_training = model.training
        model.eval()
        try:
            if egcn:
                emb = model.layers[0]
                if model.takes_fused_path(g.x):
                    xw = embed.embed_xw(emb.weight, emb.bias, first.weight, 0.0)
                else:
                    xw = dense.xw(torch.selu(emb(g.x)), first.weight)
                s1 = dense.xw(torch.selu(emb.bias.detach()).unsqueeze(0).contiguous(), first.weight).squeeze(0)
                self.act = _lib.ACT_NONE
                h1 = propagate(plan, xw, first.bias)
            else:
                xw, s1 = first.weight, None              # identity features: x @ W1 is W1; a new row of x is empty
                relu = bool(getattr(model, "apply_activation", False))
                self.act = _lib.ACT_RELU if relu else _lib.ACT_NONE
                h1 = propagate(plan, xw, first.bias, model.activation if relu else None)
            p = dense.xw(h1, second.weight)
        finally:
            model.train(was_training)
        h, C = self.h, self.C
        H4, C4 = _r4(h), _r4(C)
        # one row-padded table: a word's T1 row and P row are one contiguous read
        tab = torch.zeros(V, H4 + C4, dtype=torch.float32, device=dev)
        tab[:, :h] = xw.detach()[:V]
        tab[:, H4:H4 + C] = p.detach()[:V]
        self._tab, self.T1, self.P = tab, tab[:, :h], tab[:, H4:H4 + C]
        self.W2 = torch.zeros(h, C4, dtype=torch.float32, device=dev)
        self.W2[:, :C] = second.weight.detach()
        self.s1 = None if s1 is None else s1.detach().float().clone()
        self.b1, self.b2 = _bias_of(first, h, dev), _bias_of(second, C, dev)
        self.dis = gcn_norm_factors(g.edge_index, g.edge_attr, N, 1, self.degree_sum)[0][:V].clone()
        return self

    # -- inputs -----------------------------------------------------------------------------------------------------
    def _device_csr(self, tfidf) -> Tuple[Tensor, Tensor, Tensor]:
        return _device_csr(tfidf, self.n_vocab, self.device)

    # -- compute ----------------------------------------------------------------------------------------------------
    def _run(self, tfidf, want_pred: bool, want_hidden: bool = False):
        rowptr, col, val = self._device_csr(tfidf)
        B = rowptr.numel() - 1
        if not _FUSED_FOLDIN:
            return self._composed(rowptr, col, val, want_pred, want_hidden)
        h, C = self.h, self.C
        H4, C4 = _r4(h), _r4(C)
        dev = self.device
        logits = torch.empty(B, C4, dtype=torch.float32, device=dev)
        pred = torch.empty(B, dtype=torch.int32, device=dev) if want_pred else None
        hidden = torch.empty(B, H4, dtype=torch.float32, device=dev) if want_hidden else None
        if col.numel() == 0:                       # (data_ptr() of an empty tensor is null)
            col = torch.zeros(1, dtype=torch.int32, device=dev)
            val = torch.zeros(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().tgcn_foldin_two_layer(
                B, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), self.n_vocab, self.dis.data_ptr(),
                _lib.DEGREE_SUMS[self.degree_sum], self.T1.data_ptr(), self._tab.stride(0), h,
                self.s1.data_ptr() if self.s1 is not None else None, self.b1.data_ptr(), self.act, self.P.data_ptr(),
                self._tab.stride(0), C, self.W2.data_ptr(), self.W2.stride(0), self.b2.data_ptr(),
                logits.data_ptr() if B else None, C4, pred.data_ptr() if (want_pred and B) else None,
                hidden.data_ptr() if (want_hidden and B) else None, H4, _stream_ptr(dev)))
        return logits[:, :C], pred, (hidden[:, :h] if want_hidden else None)

    def _composed(self, rowptr: Tensor, col: Tensor, val: Tensor, want_pred: bool, want_hidden: bool):
        """The same definition from the package's other pieces: the document scalars and a plan of the [B, V] matrix of a_j
        (`_doc_scalars`: a plan per batch), two SpMMs, one dense product and a row scale."""
        B, dev = rowptr.numel() - 1, self.device
        a_dd, op = _doc_scalars(rowptr, col, val, self.dis, self.n_vocab, self.degree_sum)
        if op is not None:
            u, zg = op.spmm(self.T1), op.spmm(self.P)
        else:
            u = torch.zeros(B, self.h, dtype=torch.float32, device=dev)
            zg = torch.zeros(B, self.C, dtype=torch.float32, device=dev)
        if self.s1 is not None:
            u = u + a_dd * self.s1
        u = u + self.b1
        if self.act == _lib.ACT_RELU:
            u = torch.relu(u)
        if B:
            z = (zg + a_dd * dense.xw(u.contiguous(), self.W2[:, :self.C])) + self.b2
        else:
            z = zg
        pred = z.argmax(dim=1).to(torch.int32) if want_pred else None
        return z, pred, (u if want_hidden else None)

    @torch.no_grad()
    def logits(self, tfidf) -> Tensor:
        """float32 [B, C]: row i holds what the model's eval forward gives node N + i of `extended_graph(g, tfidf)`."""
        return self._run(tfidf, False)[0]

    @torch.no_grad()
    def predict(self, tfidf) -> Tensor:
        """int64 [B]: the first arg-max of every row of `logits(tfidf)`, taken inside the same launch."""
        return self._run(tfidf, True)[1].long()

    def predict_text(self, t2g, docs) -> Tensor:
        """`predict(t2g.transform(docs))` for the fitted `Text2GraphTransformer` that built `g`."""
        return self.predict(t2g.transform(docs))


class FoldInLevels:
    """`FoldInLevels(models, graphs, link="softmax")`: classify documents outside the training graph through the per-level
    strategy.  `models` are the L = 2 or 3 trained two-layer `models.GCN` (linear, or `apply_activation=True` with `nn.ReLU`),
    `graphs` the graphs they run on: `g` with its sparse identity features for level 1, `with_hierarchy(g, ...)` -- a
    `HierarchyFeatures` with as many columns as the level above has classes -- for every further level, all on the same
    edges.  Which H the old documents carry there (their true labels, or `predicted_hierarchy`) is the caller's choice: it
    fixes the frozen P of that level.  A new document's H is `link` of its own logits one level up: "softmax", or "one_hot"
    of the first arg-max (one value for all levels, or one per level from the second on).  Inputs are as on `FoldIn`."""

    def __init__(self, models: Sequence, graphs: Sequence, link="softmax"):
        self.models, self.graphs = list(models), list(graphs)
        L = len(self.models)
        links = [link] * (L - 1) if isinstance(link, str) else list(link)
        self._check(self.models, self.graphs, links)
        self.links = links
        self.refresh()

    # -- what is supported ------------------------------------------------------------------------------------------
    @staticmethod
    def _check(models, graphs, links) -> None:
        from . import models as M
        L = len(models)
        if not 2 <= L <= _lib.FOLDIN_MAX_LEVELS or len(graphs) != L:
            raise ValueError(f"FoldInLevels: 2 or {_lib.FOLDIN_MAX_LEVELS} levels, one graph per model ({L} models, "
                             f"{len(graphs)} graphs)")
        if len(links) != L - 1 or any(k not in _lib.LINKS for k in links):
            raise ValueError(f"FoldInLevels: link is one of {sorted(_lib.LINKS)}, or one per level from the second on ({links})")
        g0 = graphs[0]
        hs, Cs = [], []
        for l, (model, g) in enumerate(zip(models, graphs)):
            if type(model) is not M.GCN:
                why = {M.EGCN: "EGCN levels: a new document's embedding row is a dense product per document",
                       M.JumpingKnowledgeNetwork: "JKN"}.get(type(model), "unsupported model type")
                raise NotImplementedError(f"FoldInLevels: level {l + 1} is a {type(model).__name__}, every level must be a "
                                          f"two-layer models.GCN ({why})")
            convs = list(model.layers)
            between = model.activation if getattr(model, "apply_activation", False) else None
            h, C = _check_two_layer("FoldInLevels", convs, between, at=f" level {l + 1}:")
            if l > 0:
                for name in ("edge_index", "edge_attr"):
                    a, b = getattr(g0, name), getattr(g, name)
                    if a is not b and (a is None or b is None or a.shape != b.shape or not torch.equal(a, b)):
                        raise ValueError(f"FoldInLevels: level {l + 1}'s graph has another `{name}` than level 1's: the levels "
                                         "share one graph")
                if int(g.n_vocab) != int(g0.n_vocab):
                    raise ValueError(f"FoldInLevels: level {l + 1}'s graph has another `n_vocab` ({g.n_vocab}) than level 1's "
                                     f"({g0.n_vocab})")
            x = g.x
            N = g0.x.size(0)
            if l == 0:
                if isinstance(x, hier.HierarchyFeatures) or not x.is_sparse or not is_sparse_identity(x):
                    raise NotImplementedError("FoldInLevels: level 1 takes sparse identity features")
                _require_cuda(x, "graphs[0].x")
            else:
                if not isinstance(x, hier.HierarchyFeatures):
                    raise NotImplementedError(f"FoldInLevels: level {l + 1} takes HierarchyFeatures (with_hierarchy(g, ...)), "
                                              f"not {type(x).__name__}")
                if x.n_features != Cs[l - 1] or x.h_row0 != int(g0.n_vocab) or x.n_nodes != N:
                    raise ValueError(f"FoldInLevels: level {l + 1}'s HierarchyFeatures must have n_features == {Cs[l - 1]} (the "
                                     f"classes of level {l}), h_row0 == n_vocab == {int(g0.n_vocab)} and {N} nodes; it has "
                                     f"n_features={x.n_features}, h_row0={x.h_row0}, n_nodes={x.n_nodes}")
                _require_cuda(x, f"graphs[{l}].x")
            if convs[0].in_channels != x.size(1):
                raise ValueError(f"FoldInLevels: level {l + 1}'s model takes {convs[0].in_channels} features, its graph has "
                                 f"{x.size(1)}")
            hs.append(h)
            Cs.append(C)
            _check_widths("FoldInLevels", h, C, at=f" level {l + 1}:")
        need = levels_lds_bytes(hs, Cs)
        if need > _lib.FOLDIN_LEVELS_LDS_LIMIT:
            raise NotImplementedError(f"FoldInLevels: the levels' W2 and Wh need {need} bytes of LDS next to the waves' slices, "
                                      f"a compute unit has {_lib.FOLDIN_LEVELS_LDS_LIMIT}")

    # -- the frozen tables ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self) -> "FoldInLevels":
        """Freeze dis, the combined table, W2, Wh and the biases again from the models' current parameters: one eval forward
        per level on that level's own graph."""
        g0 = self.graphs[0]
        V, N, dev = int(g0.n_vocab), g0.x.size(0), g0.x.device
        self.n_vocab, self.device = V, dev
        self.h, self.C, self.act = [], [], []
        self.W2, self.Wh, self.b1, self.b2 = [], [], [], []
        xws, ps = [], []
        for l, (model, g) in enumerate(zip(self.models, self.graphs)):
            first, second = list(model.layers)
            plan = first.plan(g.x, g.edge_index, g.edge_attr)
            if l == 0:
                self.degree_sum = plan.degree_sum
            relu = bool(getattr(model, "apply_activation", False))
            was_training = model.training
            model.eval()
            try:
                xw = first.features_times(g.x, first.weight)             # W1 itself, or hier.xw on [I | H]
                h1 = propagate(plan, xw, first.bias, model.activation if relu else None)
                ps.append(dense.xw(h1, second.weight).detach()[:V])
            finally:
                model.train(was_training)
            h, C = first.out_channels, second.out_channels
            xws.append(first.weight.detach()[:V])                         # word rows have H = 0: their row of x W1 is W1's
            self.h.append(h), self.C.append(C), self.act.append(_lib.ACT_RELU if relu else _lib.ACT_NONE)
            w2 = torch.zeros(h, _r4(C), dtype=torch.float32, device=dev)
            w2[:, :C] = second.weight.detach()
            self.W2.append(w2)
            wh = None
            if l > 0:
                wh = torch.zeros(self.C[l - 1], _r4(h), dtype=torch.float32, device=dev)
                wh[:, :h] = first.weight.detach()[N:N + self.C[l - 1]]
            self.Wh.append(wh)
            self.b1.append(_bias_of(first, h, dev)), self.b2.append(_bias_of(second, C, dev))
        # one row-padded table: a word's 2L rows are one contiguous read
        self.t1_col, self.p_col, at = [], [], 0
        for h, C in zip(self.h, self.C):
            self.t1_col.append(at)
            self.p_col.append(at + _r4(h))
            at += _r4(h) + _r4(C)
        tab = torch.zeros(V, at, dtype=torch.float32, device=dev)
        for l in range(len(self.h)):
            tab[:, self.t1_col[l]:self.t1_col[l] + self.h[l]] = xws[l]
            tab[:, self.p_col[l]:self.p_col[l] + self.C[l]] = ps[l]
        self._tab = tab
        self.dis = gcn_norm_factors(g0.edge_index, g0.edge_attr, N, 1, self.degree_sum)[0][:V].clone()
        return self

    _device_csr = FoldIn._device_csr

    # -- compute ----------------------------------------------------------------------------------------------------
    def _run(self, tfidf, want_pred: bool = False, want_link: bool = False, want_hidden: bool = False, want_logits: bool = True):
        """(logits, pred, links, hidden): lists per level (links from the second level on), None where not asked for."""
        rowptr, col, val = self._device_csr(tfidf)
        B, L, dev = rowptr.numel() - 1, len(self.h), self.device
        if not _FUSED_FOLDIN:
            return self._composed(rowptr, col, val, want_pred)

        def out(width, want, dtype=torch.float32):
            return torch.empty(B, _r4(width), dtype=dtype, device=dev) if want else None
        logits = [out(C, want_logits) for C in self.C]
        hidden = [out(h, want_hidden) for h in self.h]
        links = [None] + [out(self.C[l - 1], want_link) for l in range(1, L)]
        pred = torch.empty(L, max(B, 1), dtype=torch.int32, device=dev) if want_pred else None
        if col.numel() == 0:                       # (data_ptr() of an empty tensor is null)
            col = torch.zeros(1, dtype=torch.int32, device=dev)
            val = torch.zeros(1, dtype=torch.float32, device=dev)

        def ptr(t):
            return t.data_ptr() if (t is not None and B) else None
        lv = (_lib.FoldinLevel * L)()
        for l in range(L):
            lv[l] = _lib.FoldinLevel(
                self.t1_col[l], self.p_col[l], self.W2[l].data_ptr(), self.W2[l].stride(0),
                self.Wh[l].data_ptr() if l else None, self.Wh[l].stride(0) if l else 0, self.b1[l].data_ptr(),
                self.b2[l].data_ptr(), ptr(logits[l]), _r4(self.C[l]), ptr(pred[l]) if want_pred else None, ptr(hidden[l]),
                _r4(self.h[l]), ptr(links[l]), _r4(self.C[l - 1]) if l else 0, self.h[l], self.C[l], self.act[l],
                _lib.LINKS[self.links[l - 1]] if l else 0)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().tgcn_foldin_levels(
                B, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), self.n_vocab, self.dis.data_ptr(),
                _lib.DEGREE_SUMS[self.degree_sum], self._tab.data_ptr(), self._tab.stride(0), L, lv, _stream_ptr(dev)))

        def cut(ts, widths):
            return [None if t is None else t[:, :w] for t, w in zip(ts, widths)]
        return (cut(logits, self.C), None if pred is None else pred[:, :B], cut(links, [0] + self.C[:-1])[1:],
                cut(hidden, self.h))

    def _composed(self, rowptr: Tensor, col: Tensor, val: Tensor, want_pred: bool):
        """The same definition from the package's other pieces: the document scalars and ONE plan of the [B, V] matrix
        of a_j per batch (`_doc_scalars`; the levels share it), ONE SpMM at the combined table's width, then per level
        `dense.xw` for H_d Wh and u W2 and torch's softmax / arg-max for the link."""
        B, L, dev = rowptr.numel() - 1, len(self.h), self.device
        a_dd, op = _doc_scalars(rowptr, col, val, self.dis, self.n_vocab, self.degree_sum)
        if op is not None:
            sums = op.spmm(self._tab)
        else:
            sums = torch.zeros(B, self._tab.size(1), dtype=torch.float32, device=dev)
        logits, links, hidden, preds = [], [], [], []
        for l in range(L):
            h, C = self.h[l], self.C[l]
            u = sums[:, self.t1_col[l]:self.t1_col[l] + h]
            if l:
                z_up = logits[l - 1]
                if self.links[l - 1] == "softmax":
                    p = torch.softmax(z_up, dim=1)
                else:
                    p = torch.zeros_like(z_up)
                    if B:
                        p[torch.arange(B, device=dev), z_up.argmax(dim=1)] = 1.0
                links.append(p)
                if B:
                    u = u + a_dd * dense.xw(p.contiguous(), self.Wh[l][:, :h])
            u = u + self.b1[l]
            if self.act[l] == _lib.ACT_RELU:
                u = torch.relu(u)
            z = sums[:, self.p_col[l]:self.p_col[l] + C]
            if B:
                z = (z + a_dd * dense.xw(u.contiguous(), self.W2[l][:, :C])) + self.b2[l]
            logits.append(z), hidden.append(u)
            if want_pred:
                preds.append(z.argmax(dim=1).to(torch.int32) if B else torch.zeros(0, dtype=torch.int32, device=dev))
        return logits, (torch.stack(preds) if want_pred else None), links, hidden

    @torch.no_grad()
    def logits(self, tfidf) -> List[Tensor]:
        """L tensors float32 [B, C_l]: row i of level l holds what that level's eval forward gives node N + i of
        `extended_graph(graphs[l], tfidf, hierarchy=probabilities(tfidf)[l - 1])`."""
        return self._run(tfidf)[0]

    @torch.no_grad()
    def predict(self, tfidf) -> Tensor:
        """int64 [B, L]: every level's first arg-max, all from the one launch."""
        return self._run(tfidf, want_pred=True, want_logits=False)[1].t().long()

    @torch.no_grad()
    def probabilities(self, tfidf) -> List[Tensor]:
        """L - 1 tensors float32 [B, C_{l-1}]: the link rows -- the H a new document carries into level l = 2 .. L."""
        return self._run(tfidf, want_link=True, want_logits=False)[2]

    def predict_text(self, t2g, docs) -> Tensor:
        """`predict(t2g.transform(docs))` for the fitted `Text2GraphTransformer` that built the graph."""
        return self.predict(t2g.transform(docs))


class FoldInPerLabel:
    """`FoldInPerLabel(top_model, net, g, class_map=None)`: classify documents outside the training graph `g` through the
    per-label strategy (eval_perlabel.py:57-78).  `top_model` is the two-layer `models.GCN` (linear, or
    `apply_activation=True` with `nn.ReLU`) trained on the top labels of `g`, whose arg-max picks the member; it may be None
    when every call passes `route=`.  `net` is the `PerLabelGCN` of the K per-label classifiers on the same `g`, or a sequence
    of K two-layer linear `GCN` members (eval_perlabel.py:16-19 loads those), which goes through `PerLabelGCN.from_members`.
    `class_map` is `relabel`'s: K lists, local class -> global class.  The tables are frozen by one eval forward of each
    network; call `refresh()` after more training (a `net` given as members is rebuilt from them).  Inputs are as on `FoldIn`.
    Member k's row for document i is what `net.export_members()[k]`'s eval forward gives node N + i of
    `extended_graph(g, tfidf)`."""

    def __init__(self, top_model, net, g, class_map=None):
        from . import perlabel
        self.top_model, self.g = top_model, g
        self._members = None
        if isinstance(net, (list, tuple)):
            self._check_members(net)
            self._members = list(net)
            net = perlabel.PerLabelGCN.from_members(self._members)
        self.net = net
        self._check(top_model, net, g)
        self.class_map = None
        if class_map is not None:
            counts = [len(m) for m in class_map]
            if counts != list(net.class_counts):
                raise ValueError(f"FoldInPerLabel: class_map lists {counts} classes per member, the network has "
                                 f"{list(net.class_counts)}")
            self.class_map = perlabel.column_class_map(class_map, g.x.device)
        self.refresh()

    # -- what is supported ------------------------------------------------------------------------------------------
    @staticmethod
    def _check_members(members) -> None:
        from . import models as M
        for k, m in enumerate(members):
            if type(m) is not M.GCN:
                why = {M.EGCN: "EGCN members: a new document's embedding row is a dense product per document",
                       M.JumpingKnowledgeNetwork: "JKN members: the jumping-knowledge aggregation has no closed form here",
                       M.MLP: "MLP members have no graph to fold into"}.get(type(m), "unsupported model type")
                raise NotImplementedError(f"FoldInPerLabel: member {k} is a {type(m).__name__}, every member must be a two-layer "
                                          f"models.GCN ({why})")
            _check_two_layer("FoldInPerLabel", list(m.layers), None, at=f" member {k}:")
            if getattr(m, "apply_activation", False):
                raise NotImplementedError(f"FoldInPerLabel: member {k}: other activations than none are not supported between "
                                          "a member's layers (PerLabelGCN's members are linear)")

    @staticmethod
    def _check(top_model, net, g) -> None:
        from . import models as M
        from . import perlabel, sharded
        if isinstance(net, perlabel.PerLabelMLP):
            raise NotImplementedError("FoldInPerLabel: PerLabelMLP needs no fold-in: its members see features only, and "
                                      "PerLabelMLP.predict on the new rows already is its fold-in")
        if isinstance(net, sharded.ShardedGCN) or isinstance(top_model, sharded.ShardedGCN):
            raise NotImplementedError("FoldInPerLabel: ShardedGCN (multi-GPU models) is not supported")
        if type(net) is not perlabel.PerLabelGCN:
            raise NotImplementedError(f"FoldInPerLabel takes a PerLabelGCN or a sequence of GCN members, not "
                                      f"{type(net).__name__}")
        K, h = net.n_groups, net.n_hidden
        if K > _lib.FOLDIN_MAX_MEMBERS:
            raise NotImplementedError(f"FoldInPerLabel: K = {K} members, the kernel takes {_lib.FOLDIN_MAX_MEMBERS}")
        for k, C in enumerate(net.class_counts):
            _check_widths("FoldInPerLabel", h, C, at=f" member {k}:")
        hs, Cs = [0] + [h] * K, [0] + list(net.class_counts)
        if top_model is not None:
            if type(top_model) is not M.GCN:
                why = {M.EGCN: "EGCN", M.JumpingKnowledgeNetwork: "JKN", M.MLP: "MLP has no graph to fold into"}.get(
                    type(top_model), "unsupported model type")
                raise NotImplementedError(f"FoldInPerLabel: the top model is a {type(top_model).__name__}, it must be a "
                                          f"two-layer models.GCN ({why})")
            between = top_model.activation if getattr(top_model, "apply_activation", False) else None
            h0, C0 = _check_two_layer("FoldInPerLabel", list(top_model.layers), between, at=" top model:")
            if C0 != K:
                raise ValueError(f"FoldInPerLabel: the top model has {C0} classes, the network has K = {K} members")
            _check_widths("FoldInPerLabel", h0, C0, at=" top model:")
            hs[0], Cs[0] = h0, C0
        x = g.x
        _check_identity_features("FoldInPerLabel", x)
        for who, m in (("the top model", top_model), ("the network", net)):
            if m is not None and m.layers[0].in_channels != x.size(1):
                raise ValueError(f"FoldInPerLabel: {who} takes {m.layers[0].in_channels} features, the graph has {x.size(1)}")
        need = routed_lds_bytes(hs, Cs)
        if need > _lib.FOLDIN_LEVELS_LDS_LIMIT:
            raise NotImplementedError(f"FoldInPerLabel: the W2 of the top model and of all {K} members need {need} bytes of LDS "
                                      f"next to the waves' slices, a compute unit has {_lib.FOLDIN_LEVELS_LDS_LIMIT}")

    # -- the frozen tables ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self) -> "FoldInPerLabel":
        """Freeze dis, the combined table, W2 and the biases again from the current parameters: ONE eval forward of the top
        model and ONE of the K-member network."""
        from . import perlabel
        if self._members is not None:
            self.net = perlabel.PerLabelGCN.from_members(self._members)
        top, net, g = self.top_model, self.net, self.g
        V, N, dev = int(g.n_vocab), g.x.size(0), g.x.device
        first, second = net.layers
        K, h = net.n_groups, net.n_hidden
        plan = first.plan(g.x, g.edge_index, g.edge_attr)
        self.degree_sum, self.n_vocab, self.device = plan.degree_sum, V, dev
        self.K, self.h, self.C = K, h, list(net.class_counts)
        self.seg_start = list(net.seg_start)
        was = net.training
        net.eval()
        try:
            h1 = propagate(plan, first.weight, first.bias)
            pcat = perlabel.block_diag_xw(h1, second.weight, net.seg_start, net.seg_width).detach()[:V]
        finally:
            net.train(was)
        self.h_top = self.act_top = 0
        p0 = None
        if top is not None:
            t1, t2 = list(top.layers)
            relu = bool(getattr(top, "apply_activation", False))
            self.h_top, self.act_top = t1.out_channels, (_lib.ACT_RELU if relu else _lib.ACT_NONE)
            was = top.training
            top.eval()
            try:
                h0 = propagate(t1.plan(g.x, g.edge_index, g.edge_attr), t1.weight, t1.bias, top.activation if relu else None)
                p0 = dense.xw(h0, t2.weight).detach()[:V]
            finally:
                top.train(was)
        # one row-padded table: [T1^0 | P^0] and per member [T1^k | P^k]; a document reads two of these pairs
        h4 = _r4(h)
        self.t1_col, self.p_col, at = [0], [_r4(self.h_top)], _r4(self.h_top) + (_r4(K) if top is not None else 0)
        for C in self.C:
            self.t1_col.append(at)
            self.p_col.append(at + h4)
            at += h4 + _r4(C)
        tab = torch.zeros(V, at, dtype=torch.float32, device=dev)
        if top is not None:
            tab[:, :self.h_top] = t1.weight.detach()[:V]
            tab[:, self.p_col[0]:self.p_col[0] + K] = p0
            self.W2_top = torch.zeros(self.h_top, _r4(K), dtype=torch.float32, device=dev)
            self.W2_top[:, :K] = t2.weight.detach()
            self.b1_top, self.b2_top = _bias_of(t1, self.h_top, dev), _bias_of(t2, K, dev)
        w1 = first.weight.detach()
        for k, (s, C) in enumerate(zip(self.seg_start, self.C)):
            tab[:, self.t1_col[k + 1]:self.t1_col[k + 1] + h] = w1[:V, k * h:(k + 1) * h]
            tab[:, self.p_col[k + 1]:self.p_col[k + 1] + C] = pcat[:, s:s + C]
        self._tab = tab
        self.W2 = second.weight.detach().float().clone()                 # [h, n_cols]: member k's W2 in its segment
        self.b2 = _bias_of(second, second.weight.size(1), dev)           # [n_cols] likewise
        self.b1 = torch.zeros(K, h4, dtype=torch.float32, device=dev)    # a 16-byte aligned row per member
        self.b1[:, :h] = _bias_of(first, K * h, dev).view(K, h)
        self.dis = gcn_norm_factors(g.edge_index, g.edge_attr, N, 1, self.degree_sum)[0][:V].clone()
        return self

    _device_csr = FoldIn._device_csr

    def _route(self, route, B: int) -> Optional[Tensor]:
        if route is None:
            if self.top_model is None:
                raise ValueError("FoldInPerLabel: without a top model every call needs `route=`")
            return None
        route = torch.as_tensor(route, device=self.device).to(torch.int32).contiguous()
        if tuple(route.shape) != (B,):
            raise ValueError(f"FoldInPerLabel: `route` needs one entry per document ({B}), got {tuple(route.shape)}")
        return route

    # -- compute ----------------------------------------------------------------------------------------------------
    def _run(self, tfidf, route=None, want_pred=False, want_logits=False, want_top=False, want_hidden=False):
        """(route int32 [B], top logits, logits, pred int64, hidden): None where not asked for."""
        rowptr, col, val = self._device_csr(tfidf)
        B, K, dev = rowptr.numel() - 1, self.K, self.device
        route = self._route(route, B)
        if not _FUSED_FOLDIN:
            return self._composed(rowptr, col, val, route, want_top, want_hidden)
        c_max = max(self.C)

        def out(width, want):
            return torch.empty(B, _r4(width), dtype=torch.float32, device=dev) if want else None
        top_logits, logits, hidden = out(K, want_top), out(c_max, want_logits), out(self.h, want_hidden)
        pred = torch.empty(B, dtype=torch.int64, device=dev) if want_pred else None
        route_out = torch.empty(max(B, 1), dtype=torch.int32, device=dev)       # (an output is always asked for)
        if col.numel() == 0:                       # (data_ptr() of an empty tensor is null)
            col = torch.zeros(1, dtype=torch.int32, device=dev)
            val = torch.zeros(1, dtype=torch.float32, device=dev)

        def ptr(t):
            return t.data_ptr() if (t is not None and B) else None
        mb = (_lib.FoldinMember * (K + 1))()
        if self.top_model is not None:
            mb[0] = _lib.FoldinMember(0, self.p_col[0], self.W2_top.data_ptr(), self.W2_top.stride(0), self.b1_top.data_ptr(),
                                      self.b2_top.data_ptr(), self.h_top, K, self.act_top, 0)
        esz = 4
        for k, (s, C) in enumerate(zip(self.seg_start, self.C)):
            mb[k + 1] = _lib.FoldinMember(self.t1_col[k + 1], self.p_col[k + 1], self.W2.data_ptr() + esz * s, self.W2.stride(0),
                                          self.b1[k].data_ptr(), self.b2.data_ptr() + esz * s, self.h, C, _lib.ACT_NONE, 0)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().tgcn_foldin_routed(
                B, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), self.n_vocab, self.dis.data_ptr(),
                _lib.DEGREE_SUMS[self.degree_sum], self._tab.data_ptr(), self._tab.stride(0), K, mb, ptr(route),
                self.class_map.data_ptr() if self.class_map is not None else None, route_out.data_ptr(),
                ptr(top_logits), _r4(K), ptr(logits), _r4(c_max), ptr(pred), ptr(hidden), _r4(self.h), _stream_ptr(dev)))
        return (route_out[:B], None if top_logits is None else top_logits[:, :K], None if logits is None else logits[:, :c_max],
                pred, None if hidden is None else hidden[:, :self.h])

    def _composed(self, rowptr: Tensor, col: Tensor, val: Tensor, route: Optional[Tensor], want_top: bool, want_hidden: bool):
        """The same definition from the package's other pieces: the document scalars and ONE plan of the [B, V] matrix of
        a_j per batch (`_doc_scalars`), ONE SpMM over the whole combined table, `dense.xw` for u^0 W2^0, torch's arg-max, a
        per-row gather of the member's columns and `dense.xw` per member present in the batch."""
        B, K, h, dev = rowptr.numel() - 1, self.K, self.h, self.device
        c_max = max(self.C)
        a_dd, op = _doc_scalars(rowptr, col, val, self.dis, self.n_vocab, self.degree_sum)
        if op is not None:
            sums = op.spmm(self._tab)
        else:
            sums = torch.zeros(B, self._tab.size(1), dtype=torch.float32, device=dev)
        z0 = None
        if route is None:
            u0 = sums[:, :self.h_top] + self.b1_top
            if self.act_top == _lib.ACT_RELU:
                u0 = torch.relu(u0)
            z0 = sums[:, self.p_col[0]:self.p_col[0] + K]
            if B:
                z0 = (z0 + a_dd * dense.xw(u0.contiguous(), self.W2_top[:, :K])) + self.b2_top
            route = z0.argmax(dim=1).to(torch.int32) if B else torch.zeros(0, dtype=torch.int32, device=dev)
        elif want_top:
            raise ValueError("FoldInPerLabel: with `route=` the top model is not evaluated")
        logits = torch.full((B, c_max), float("-inf"), dtype=torch.float32, device=dev)
        hidden = torch.zeros(B, h, dtype=torch.float32, device=dev) if want_hidden else None
        pred = torch.full((B,), -1, dtype=torch.int64, device=dev)
        for k in torch.unique(route).tolist():
            if not 0 <= k < K:
                continue
            rows = torch.nonzero(route == k).squeeze(1)
            s, C = self.seg_start[k], self.C[k]
            u = sums[rows, self.t1_col[k + 1]:self.t1_col[k + 1] + h] + self.b1[k, :h]
            z = sums[rows, self.p_col[k + 1]:self.p_col[k + 1] + C]
            z = (z + a_dd[rows] * dense.xw(u.contiguous(), self.W2[:, s:s + C])) + self.b2[s:s + C]
            logits[rows, :C] = z
            local = z.argmax(dim=1)
            pred[rows] = local if self.class_map is None else self.class_map[s + local]
            if want_hidden:
                hidden[rows] = u
        return route, (z0 if want_top else None), logits, pred, hidden

    @torch.no_grad()
    def predict(self, tfidf, route=None) -> Tensor:
        """int64 [B]: the routed member's first arg-max -- the global class when `class_map` was given, else the local one;
        -1 where `route` names nobody.  `route` (int [B]) replaces the top model's arg-max (eval_perlabel.py:73 routes by a
        known top label); the top model is then not evaluated."""
        return self._run(tfidf, route, want_pred=True)[3]

    @torch.no_grad()
    def predict_levels(self, tfidf) -> Tensor:
        """int64 [B, 2]: the top label and the class, both from the one launch."""
        r = self._run(tfidf, None, want_pred=True)
        return torch.stack([r[0].long(), r[3]], dim=1)

    @torch.no_grad()
    def logits(self, tfidf, route=None) -> Tuple[Tensor, Tensor]:
        """(route int64 [B], float32 [B, max C_k]): row i holds the C_k logits of member k = route[i] and -inf behind them,
        so that arg-max and softmax of the row are the member's own."""
        r = self._run(tfidf, route, want_logits=True)
        return r[0].long(), r[2]

    @torch.no_grad()
    def top_logits(self, tfidf) -> Tensor:
        """float32 [B, K]: the top model's logits, what `FoldIn(top_model, g).logits(tfidf)` gives."""
        return self._run(tfidf, None, want_top=True)[1]

    def predict_text(self, t2g, docs) -> Tensor:
        """`predict(t2g.transform(docs))` for the fitted `Text2GraphTransformer` that built `g`."""
        return self.predict(t2g.transform(docs))


class FoldInDeep:
    """`FoldInDeep(model, g)`: classify documents outside the training graph `g` with a trained network of 2 to 4 GCNConv
    layers -- `models.GCN` (linear, or `apply_activation=True` with `nn.ReLU`), `models.EGCN` or
    `models.JumpingKnowledgeNetwork`, sparse identity features.  The chain of layers is ONE kernel launch
    (`tgcn_foldin_layers`); a JKN's aggregation (`jk.lstm_forward`), activation and `lin` then run on the B x L rows it wrote.
    Everything is frozen from the model's current parameters by one eval forward, layer by layer; call `refresh()` after more
    training.  Inputs are as on `FoldIn`."""

    def __init__(self, model, g):
        self.model, self.g = model, g
        self._check(model, g)
        self.refresh()

    # -- what is supported ------------------------------------------------------------------------------------------
    @staticmethod
    def _convs(model):
        from . import models as M
        return list(model.layers)[(1 if type(model) is M.EGCN else 0):]

    @staticmethod
    def _check(model, g) -> None:
        from . import models as M
        kind = type(model)
        if kind not in (M.GCN, M.EGCN, M.JumpingKnowledgeNetwork):
            from . import crossval, perlabel, sharded
            causes = (((perlabel.PerLabelGCN,), "the K-member networks: a PerLabelGCN folds in through FoldInPerLabel"),
                      ((crossval.CrossValGCN, crossval.CrossValEGCN, perlabel.PerLabelMLP), "the K-member networks"),
                      ((sharded.ShardedGCN,), "ShardedGCN: multi-GPU models"),
                      ((M.MLP,), "MLP has no graph to fold into"))
            why = next((text for classes, text in causes if isinstance(model, classes)), "unsupported model type")
            raise NotImplementedError(f"FoldInDeep takes models.GCN, models.EGCN and models.JumpingKnowledgeNetwork, not "
                                      f"{kind.__name__} ({why})")
        convs = FoldInDeep._convs(model)
        L = len(convs)
        if not 2 <= L <= _lib.FOLDIN_MAX_LAYERS:
            raise NotImplementedError(f"FoldInDeep: n_gcn outside 2..{_lib.FOLDIN_MAX_LAYERS} (the model has {L} GCNConv "
                                      "layers)")
        for c in convs:
            if not (c.add_self_loops and c.normalize) or c.improved:
                raise NotImplementedError("FoldInDeep: GCNConv(add_self_loops=True, normalize=True, improved=False) only")
        if kind is M.GCN and getattr(model, "apply_activation", False) and type(model.activation) is not nn.ReLU:
            raise NotImplementedError("FoldInDeep: other activations than nn.ReLU are not supported between GCN layers "
                                      f"({type(model.activation).__name__})")
        _check_identity_features("FoldInDeep", g.x)
        first_in = model.layers[0].in_features if kind is M.EGCN else convs[0].in_channels
        if first_in != g.x.size(1):
            raise ValueError(f"FoldInDeep: the model takes {first_in} features, the graph has {g.x.size(1)}")
        widths = [c.out_channels for c in convs]
        lib = _lib.load()
        h_max, c_max = lib.tgcn_foldin_max_hidden(), lib.tgcn_foldin_max_classes()
        if widths[0] > h_max or any(w > c_max for w in widths[1:]):
            raise NotImplementedError(f"FoldInDeep: layer widths {widths} exceed the kernel's {h_max} for the first layer / "
                                      f"{c_max} for every further one")
        need = layers_lds_bytes(widths)
        if need > _lib.FOLDIN_LEVELS_LDS_LIMIT:
            raise NotImplementedError(f"FoldInDeep: the layers' W_2 .. W_{L} and biases need {need} bytes of LDS next to the "
                                      f"waves' slices, a compute unit has {_lib.FOLDIN_LEVELS_LDS_LIMIT}")

    # -- the frozen tables ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self) -> "FoldInDeep":
        """Freeze dis, the combined table [T^1 | .. | T^L], W_2 .. W_L, the biases, s1 and -- for a JKN -- the LSTM,
        attention and `lin` parameters again from the model's current parameters: ONE eval forward, layer by layer."""
        from . import models as M
        model, g = self.model, self.g
        kind = type(model)
        convs = self._convs(model)
        L = len(convs)
        V, N, dev = int(g.n_vocab), g.x.size(0), g.x.device
        plan = convs[0].plan(g.x, g.edge_index, g.edge_attr)
        self.degree_sum, self.n_vocab, self.device = plan.degree_sum, V, dev
        self.widths = [c.out_channels for c in convs]
        self.jkn = kind is M.JumpingKnowledgeNetwork
        relu = kind is M.GCN and bool(getattr(model, "apply_activation", False))
        self.act = [(_lib.ACT_RELU if (relu and l < L - 1) else _lib.ACT_NONE) for l in range(L)]
        was_training = model.training
        model.eval()
        try:
            s1 = None
            if kind is M.EGCN:
                emb = model.layers[0]
                if model.takes_fused_path(g.x):
                    xw = embed.embed_xw(emb.weight, emb.bias, convs[0].weight, 0.0)
                else:
                    xw = dense.xw(torch.selu(emb(g.x)), convs[0].weight)
                s1 = dense.xw(torch.selu(emb.bias.detach()).unsqueeze(0).contiguous(), convs[0].weight).squeeze(0)
            else:
                xw = convs[0].weight                     # identity features: x @ W1 is W1; a new row of x is empty
            segs = [xw.detach()[:V]]
            for l in range(1, L):
                h = propagate(plan, xw, convs[l - 1].bias, model.activation if self.act[l - 1] == _lib.ACT_RELU else None)
                xw = dense.xw(h, convs[l].weight)
                segs.append(xw.detach()[:V])
        finally:
            model.train(was_training)
        # one row-padded table: a word's L segments are one contiguous read
        self.t_col, at = [], 0
        for w in self.widths:
            self.t_col.append(at)
            at += _r4(w)
        tab = torch.zeros(V, at, dtype=torch.float32, device=dev)
        for l, w in enumerate(self.widths):
            tab[:, self.t_col[l]:self.t_col[l] + w] = segs[l]
        self._tab = tab
        self.W = [None]
        for l in range(1, L):
            wl = torch.zeros(self.widths[l - 1], _r4(self.widths[l]), dtype=torch.float32, device=dev)
            wl[:, :self.widths[l]] = convs[l].weight.detach()
            self.W.append(wl)
        self.b = [_bias_of(c, w, dev) for c, w in zip(convs, self.widths)]
        self.s1 = None if s1 is None else s1.detach().float().clone()
        self.dis = gcn_norm_factors(g.edge_index, g.edge_attr, N, 1, self.degree_sum)[0][:V].clone()
        if self.jkn:
            agg, lin = model.jk, model.lin
            self._jk_params = [p.detach().clone().contiguous() for p in agg._lstm_parameters()]
            self._att_w = agg.att.weight.detach().clone().reshape(-1)
            self._att_b = agg.att.bias.detach().clone()
            self._lin_wt = lin.weight.detach().clone().t()           # (the layout `lin` itself hands to the product)
            self._lin_b = None if lin.bias is None else lin.bias.detach().clone()
            self.n_classes = lin.out_features
        else:
            self.n_classes = self.widths[-1]
        return self

    def _device_csr(self, tfidf) -> Tuple[Tensor, Tensor, Tensor]:
        return _device_csr(tfidf, self.n_vocab, self.device)

    # -- compute ----------------------------------------------------------------------------------------------------
    def _chain(self, tfidf, want: Sequence[bool], want_pred: bool):
        """(the L activations [B, w_l], None where not asked for; pred int32 [B] of x^L or None)."""
        rowptr, col, val = self._device_csr(tfidf)
        B, L, dev = rowptr.numel() - 1, len(self.widths), self.device
        if not _FUSED_FOLDIN:
            return self._composed(rowptr, col, val, want, want_pred)
        outs = [torch.empty(B, _r4(w), dtype=torch.float32, device=dev) if on else None for w, on in zip(self.widths, want)]
        pred = torch.empty(B, dtype=torch.int32, device=dev) if want_pred else None
        if col.numel() == 0:                       # (data_ptr() of an empty tensor is null)
            col = torch.zeros(1, dtype=torch.int32, device=dev)
            val = torch.zeros(1, dtype=torch.float32, device=dev)

        def ptr(t):
            return t.data_ptr() if (t is not None and B) else None
        ly = (_lib.FoldinLayer * L)()
        for l in range(L):
            ly[l] = _lib.FoldinLayer(self.W[l].data_ptr() if l else None, self.W[l].stride(0) if l else 0, self.b[l].data_ptr(),
                                     ptr(outs[l]), _r4(self.widths[l]), self.t_col[l], self.widths[l], self.act[l], 0)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().tgcn_foldin_layers(
                B, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), self.n_vocab, self.dis.data_ptr(),
                _lib.DEGREE_SUMS[self.degree_sum], self._tab.data_ptr(), self._tab.stride(0),
                self.s1.data_ptr() if self.s1 is not None else None, L, ly, ptr(pred), _stream_ptr(dev)))
        return [None if t is None else t[:, :w] for t, w in zip(outs, self.widths)], pred

    def _composed(self, rowptr: Tensor, col: Tensor, val: Tensor, want: Sequence[bool], want_pred: bool):
        """The same definition from the package's other pieces: the document scalars and ONE plan of the [B, V] matrix of
        a_j per batch (`_doc_scalars`), one SpMM per layer on that layer's segment, `dense.xw` for x^{l-1} W_l and torch for
        the bias and the activation."""
        B, dev = rowptr.numel() - 1, self.device
        a_dd, op = _doc_scalars(rowptr, col, val, self.dis, self.n_vocab, self.degree_sum)
        acts, x = [], None
        for l, w in enumerate(self.widths):
            if op is not None:
                s = op.spmm(self._tab[:, self.t_col[l]:self.t_col[l] + w])
            else:
                s = torch.zeros(B, w, dtype=torch.float32, device=dev)
            if l == 0:
                if self.s1 is not None:
                    s = s + a_dd * self.s1
            elif B:
                s = s + a_dd * dense.xw(x.contiguous(), self.W[l][:, :w])
            x = s + self.b[l]
            if self.act[l] == _lib.ACT_RELU:
                x = torch.relu(x)
            acts.append(x)
        pred = x.argmax(dim=1).to(torch.int32) if want_pred else None
        return [a if on else None for a, on in zip(acts, want)], pred

    def _aggregate(self, acts: List[Tensor]):
        """A JKN's rows after the chain: (logits [B, C], alpha [B, L]) -- `jk.lstm_forward` (the fused kernel where the model's
        own forward takes it, the ReLU in its epilogue), any other activation module, then `lin` on the package's kernels."""
        from . import jk
        from .conv import features_times
        model = self.model
        relu = type(model.activation) is nn.ReLU
        x, alpha = jk.lstm_forward(acts, self._jk_params, self._att_w, self._att_b, relu, model.jk.takes_fused_path(),
                                   model.jk.chunk_rows)
        if not relu:
            x = model.activation(x)
        if x.size(0) == 0:
            return torch.zeros(0, self.n_classes, dtype=torch.float32, device=self.device), alpha
        z = features_times(x, self._lin_wt, self._lin_wt.size(0))
        return (z if self._lin_b is None else z + self._lin_b), alpha

    def _run(self, tfidf, want_pred: bool):
        """(logits, pred int64 or None)."""
        L = len(self.widths)
        if self.jkn:
            z = self._aggregate(self._chain(tfidf, [True] * L, False)[0])[0]
            return z, (z.argmax(dim=1) if want_pred else None)
        acts, pred = self._chain(tfidf, [False] * (L - 1) + [True], want_pred)
        return acts[-1], (pred.long() if want_pred else None)

    @torch.no_grad()
    def logits(self, tfidf) -> Tensor:
        """float32 [B, C]: row i holds what the model's eval forward gives node N + i of `extended_graph(g, tfidf)`."""
        return self._run(tfidf, False)[0]

    @torch.no_grad()
    def predict(self, tfidf) -> Tensor:
        """int64 [B]: the first arg-max of every row of `logits(tfidf)` (GCN / EGCN: taken inside the same launch)."""
        return self._run(tfidf, True)[1]

    @torch.no_grad()
    def activations(self, tfidf) -> List[Tensor]:
        """L tensors float32 [B, w_l]: row i of the l-th holds layer l's eval-mode output for node N + i of
        `extended_graph(g, tfidf)` -- what a JKN's aggregation sees."""
        return self._chain(tfidf, [True] * len(self.widths), False)[0]

    @torch.no_grad()
    def alpha(self, tfidf) -> Tensor:
        """float32 [B, L]: a JKN's attention weights over the layers for every new document."""
        if not self.jkn:
            raise TypeError("FoldInDeep.alpha: the model is not a JumpingKnowledgeNetwork")
        return self._aggregate(self._chain(tfidf, [True] * len(self.widths), False)[0])[1]

    def predict_text(self, t2g, docs) -> Tensor:
        """`predict(t2g.transform(docs))` for the fitted `Text2GraphTransformer` that built `g`."""
        return self.predict(t2g.transform(docs))


def layers_lds_bytes(widths: Sequence[int]) -> int:
    """`tgcn_foldin_layers_lds_bytes`: the LDS a workgroup of the layer-chain kernel needs for these widths (-1: not a shape it
    takes).  Host arithmetic."""
    import ctypes
    n = len(widths)
    arr = ctypes.c_int32 * max(n, 1)
    return int(_lib.load().tgcn_foldin_layers_lds_bytes(n, arr(*[int(v) for v in widths])))


def routed_lds_bytes(h: Sequence[int], C: Sequence[int]) -> int:
    """`tgcn_foldin_routed_lds_bytes`: the LDS a workgroup of the routed kernel needs for the K + 1 networks of these widths,
    the top model first (h[0] == 0: none); -1: not a shape it takes.  Host arithmetic."""
    import ctypes
    n = len(h)
    arr = ctypes.c_int32 * max(n, 1)
    return int(_lib.load().tgcn_foldin_routed_lds_bytes(n - 1, arr(*[int(v) for v in h]), arr(*[int(v) for v in C])))


def levels_lds_bytes(h: Sequence[int], C: Sequence[int]) -> int:
    """`tgcn_foldin_levels_lds_bytes`: the LDS a workgroup of the fused kernel needs for these widths (-1: not a shape it
    takes).  Host arithmetic."""
    import ctypes
    n = len(h)
    arr = ctypes.c_int32 * max(n, 1)
    return int(_lib.load().tgcn_foldin_levels_lds_bytes(n, arr(*[int(v) for v in h]), arr(*[int(v) for v in C])))
