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
