"""`textgcn.lib.models` import path (flat_amazon.py:14 `from textgcn.lib.models import *`;
perlevel_amazon.py:14 `from textgcn.lib.models import JumpingKnowledgeNetwork, GCN, EGCN`;
MLP_flat.py `from textgcn.lib.models import MLP`).  `PerLabelGCN` has no counterpart there: it is the K `GCN`s of
perlabel_amazon.py:113 as one network (pytextgcn_amd/perlabel.py); `CrossValGCN` likewise is the len(lrs) x KFold `GCN`s of one
cell of old/h_o_train.py as one network (pytextgcn_amd/crossval.py), and `CrossValEGCN` the `EGCN`s of the same cell."""
from ..models import EGCN, GCN, MLP, JumpingKnowledgeNetwork
from ..crossval import CrossValEGCN, CrossValGCN
from ..perlabel import PerLabelGCN, PerLabelMLP

__all__ = ["GCN", "EGCN", "JumpingKnowledgeNetwork", "MLP", "PerLabelGCN", "PerLabelMLP", "CrossValGCN", "CrossValEGCN"]
