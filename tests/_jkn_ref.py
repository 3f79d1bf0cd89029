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

    def forward_with_alpha(self, xs):
        x = torch.stack(xs, dim=1)                         # [N, L, C]
        alpha, _ = self.lstm(x)
        alpha = self.att(alpha).squeeze(-1)                # [N, L]
        alpha = torch.softmax(alpha, dim=-1)
        return (x * alpha.unsqueeze(-1)).sum(dim=1), alpha

    def forward(self, xs):
        return self.forward_with_alpha(xs)[0]


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


def jk_truth(xs, jk_state, G=None, relu=False, with_alpha=False):
    """float64: out of the JK step for the inputs `xs` and the parameters `jk_state` (a state_dict with `lstm.*` / `att.*`
    keys); given G = d out also the gradients {"x": [L], "lstm": [8, in LSTM_KEYS order], "att.weight", "att.bias"};
    `with_alpha`: the attention weights alpha [N, L] as one more, last, result."""
    xs = [x.detach().cpu().double().requires_grad_() for x in xs]
    L, C = len(xs), xs[0].size(1)
    ref = JKRef(C, L).double()
    H = jk_state["lstm.weight_hh_l0"].shape[1]
    assert ref.lstm.hidden_size == H
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in jk_state.items()})
    out, alpha = ref.forward_with_alpha(xs)
    alpha = (alpha.detach(),) if with_alpha else ()
    if relu:
        out = torch.relu(out)
    if G is None:
        return (out.detach(),) + alpha if with_alpha else out.detach()
    lstm = [getattr(ref.lstm, k) for k in LSTM_KEYS]
    grads = torch.autograd.grad(out, xs + lstm + [ref.att.weight, ref.att.bias], G.detach().cpu().double())
    return (out.detach(), {"x": list(grads[:L]), "lstm": list(grads[L:L + 8]), "att.weight": grads[L + 8],
                           "att.bias": grads[L + 9]}) + alpha


def jk_values(N, C, L, seed, scale=1.0):
    """The L inputs [N, C] ~ N(0, scale^2) and G = d out ~ N(0, 1) of a kernel test, on the CPU in float32."""
    gen = torch.Generator().manual_seed(seed)
    vs = [torch.randn(N, C, generator=gen) * scale for _ in range(L)]
    return vs, torch.randn(N, C, generator=gen)


# The dispatch of the fused forward (pytextgcn_amd/csrc/jk.hip): k_jk_fwd<NHB> with NHB = ceil(H / 32) in 1 .. 8 blocks of
# 32 hidden units, H = L C // 2, on workgroups of 4 waves (128 nodes) or 2 waves (64 nodes).  (C, L, waves): every NHB with
# full blocks and with a one-unit tail, both workgroup shapes on either side of their boundary, L up to the cap of 8 (the
# score tile in LDS has stride 8), the widest H.
LEAF_SHAPES = [
    (32, 2, 4),      # H =  32, NHB 1: one full block
    (33, 2, 4),      # H =  33, NHB 2: the second block holds one unit
    (11, 6, 4),      # H =  33, NHB 2, L = 6
    (24, 8, 4),      # H =  96, NHB 3: full blocks, L = 8
    (97, 2, 4),      # H =  97, NHB 4: one-unit tail
    (32, 8, 4),      # H = 128, NHB 4: full, L = 8
    (139, 2, 4),     # H = 139, NHB 5: the last width on 4 waves
    (35, 8, 2),      # H = 140, NHB 5: the first width on 2 waves
    (46, 7, 2),      # H = 161, NHB 6, L = 7
    (90, 5, 2),      # H = 225, NHB 8: one-unit tail, L = 5
    (64, 8, 2),      # H = 256, NHB 8: the widest, L = 8
    (128, 4, 2),     # H = 256, NHB 8: the widest, C = 4 chunks of k
]


def fwd_waves(H):
    """`fwd_waves()` of jk.hip restated (the library has no query for it): the most waves of {4, 2, 1} whose LDS fits 160
    KiB, 0 beyond 8 blocks.  LDS holds the staged weight chunk, 128 x 33 floats, and per wave two h tiles of 32 x (H | 1)
    floats and the 32 x 8 score tile: 4 (4224 + w (64 (H | 1) + 256)) bytes.  H = 139: 4 (4224 + 4 x 9152) = 163328 <=
    163840, four waves; H = 140 (H | 1 = 141): 4 (4224 + 4 x 9280) = 165376 > 163840, two."""
    if (H + 31) // 32 > 8:
        return 0
    for w in (4, 2, 1):
        if 4 * (128 * 33 + w * (2 * 32 * (H | 1) + 32 * 8)) <= 160 * 1024:
            return w
    return 0


def leaf_seeds(N, C, L):
    """(seed of the module's parameters, seed of `jk_values`) of the leaf tests: tests/test_jkn_host.py shows on these very
    parameters and inputs that the bar sees a one-unit defect, tests/test_gpu_jkn.py runs the kernels on them."""
    return C + L, 1000 + N + C + L


def rel_err(a, b):
    """BASELINE.json's measure: max|a - b| / max|b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
