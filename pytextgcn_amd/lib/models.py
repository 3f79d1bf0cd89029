"""`textgcn.lib.models` import path (flat_amazon.py:14 `from textgcn.lib.models import *`;
perlevel_amazon.py:14 `from textgcn.lib.models import JumpingKnowledgeNetwork, GCN, EGCN`)."""
from ..models import EGCN, GCN, JumpingKnowledgeNetwork

__all__ = ["GCN", "EGCN", "JumpingKnowledgeNetwork"]
