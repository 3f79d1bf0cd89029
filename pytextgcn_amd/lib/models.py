"""`textgcn.lib.models` import path (flat_amazon.py:14 `from textgcn.lib.models import *`;
perlevel_amazon.py:14 `from textgcn.lib.models import JumpingKnowledgeNetwork, GCN, EGCN` -- the JumpingKnowledgeNetwork
is not part of this package)."""
from ..models import EGCN, GCN

__all__ = ["GCN", "EGCN"]
