"""The reference's JumpingKnowledgeNetwork (textgcn/lib/models.py:55-81) restated for the tests: the JK step as PyG 1.6.3
writes it -- `torch.stack`, `nn.LSTM`, `nn.Linear`, softmax, weighted sum -- on the CPU (in float64 for the kernel tests'
truth), the network from the CPU oracle's GCNConv.  Test infrastructure; nothing under pytextgcn_amd/ imports this."""
import torch
from torch import nn

from oracle.gcn_oracle import GCNConvOracle

LSTM_KEYS = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
             "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse"]


class JKRef(nn.Module):
    """`JumpingKnowledge("lstm", channels, num_layers)` of PyG 1.6.3 (jumping_knowledge.py)."""

    def __init__(self, channels, num_layers):
        super().__init__()
        self.lstm = nn.LSTM(channels, (num_layers * channels) // 2, bidirectional=True, batch_first=True)
        self.att = nn.Linear(2 * ((num_layers * channels) // 2), 1)

    def forward(self, xs):
        x = torch.stack(xs, dim=1)                         # [N, L, C]
        alpha, _ = self.lstm(x)
        alpha = self.att(alpha).squeeze(-1)                # [N, L]
        alpha = torch.softmax(alpha, dim=-1)
        return (x * alpha.unsqueeze(-1)).sum(dim=1)


class JKNRef(nn.Module):
    def __init__(self, in_channels, out_channels, n_gcn=2, n_hidden_gcn=64, activation=nn.ReLU, dropout=0.5):
        super().__init__()
        self.activation = activation()
        self.dropout = dropout
        self.layers = nn.ModuleList([GCNConvOracle(in_channels, n_hidden_gcn)])
        for _ in range(n_gcn - 2):
            self.layers.append(GCNConvOracle(n_hidden_gcn, n_hidden_gcn))
        self.layers.append(GCNConvOracle(n_hidden_gcn, n_hidden_gcn))
        self.jk = JKRef(n_hidden_gcn, n_gcn)
        self.lin = nn.Linear(n_hidden_gcn, out_channels)

    def forward(self, g):
        x = g.x
        acts = []
        for layer in self.layers:
            x = layer(x, g.edge_index, g.edge_attr)
            x = nn.functional.dropout(x, p=self.dropout, training=self.training)
            acts += [x]
        x = self.jk(acts)
        x = self.activation(x)
        x = nn.functional.dropout(x, p=self.dropout, training=self.training)
        return self.lin(x)


def jk_truth(xs, jk_state, G=None, relu=False):
    """float64: out of the JK step for the inputs `xs` and the parameters `jk_state` (a state_dict with `lstm.*` / `att.*`
    keys); given G = d out also the gradients {"x": [L], "lstm": [8, in LSTM_KEYS order], "att.weight", "att.bias"}."""
    xs = [x.detach().cpu().double().requires_grad_() for x in xs]
    L, C = len(xs), xs[0].size(1)
    ref = JKRef(C, L).double()
    H = jk_state["lstm.weight_hh_l0"].shape[1]
    assert ref.lstm.hidden_size == H
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in jk_state.items()})
    out = ref(xs)
    if relu:
        out = torch.relu(out)
    if G is None:
        return out.detach()
    lstm = [getattr(ref.lstm, k) for k in LSTM_KEYS]
    grads = torch.autograd.grad(out, xs + lstm + [ref.att.weight, ref.att.bias], G.detach().cpu().double())
    return out.detach(), {"x": list(grads[:L]), "lstm": list(grads[L:L + 8]), "att.weight": grads[L + 8],
                          "att.bias": grads[L + 9]}


def rel_err(a, b):
    """BASELINE.json's measure: max|a - b| / max|b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
