"""`textgcn.lib.models` import path (flat_amazon.py:14 `from textgcn.lib.models import *`;
perlevel_amazon.py:14 `from textgcn.lib.models import JumpingKnowledgeNetwork, GCN, EGCN`;
MLP_flat.py `from textgcn.lib.models import MLP`)."""
from ..models import EGCN, GCN, MLP, JumpingKnowledgeNetwork

__all__ = ["GCN", "EGCN", "JumpingKnowledgeNetwork", "MLP"]
