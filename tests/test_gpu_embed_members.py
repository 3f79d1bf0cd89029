"""GPU tests of the member-batched embedding front end, libtgcn.so `tgcn_embed_xw_members` / `tgcn_embed_xw_members_grad`
(pytextgcn_amd/csrc/embed.hip), through ctypes.

The contract is the oracle: member m's blocks of C, dE, db, dEh and dW are BIT FOR BIT what the single-member entry
points (`tgcn_embed_xw[_h]`, `tgcn_embed_xw[_h]_grad`) give with `seeds + m`, `p[m]` and the member's slices, because the
same kernel bodies run with the member as one more grid dimension.  Both sides write into poisoned buffers of the same
padded layout (every leading dimension above its width, a spare row behind the last member), and the WHOLE buffers are
compared on their int32 view: the results agree and the poison around and between the members' outputs is where it was.

The shapes: N in {0, 1, 127, 129, 300} (nothing; one partial wave; a partial workgroup; two workgroups; three), D in
{1, 31, 33, 70} (a k tile of 32 would straddle two members if a member's rows were not offset), n in {1, 33, 100, 257}
(257: a second column group and the accumulate path of dE), Fh in {0, 1, 17, 128} (17 reads H past the 8 register
pairs), h_row0 in {0, 70, N}, M in {1, 3, 64}; every value of every axis in at least one case.  Rates mix 0, 0.3 and 0.7
in one call.

One forward and one gradient call on identity and on [I | H] features are also held to the float64 expressions of
tests/_egcn_ref.py / tests/_egcn_hier_ref.py with the mask of tests/_dropout_hash.py per member, at the project's bar
max|a - b| / max|b| <= 1e-5 (BASELINE.json; the bar of tests/test_gpu_egcn.py)."""
import ctypes

import pytest
import torch

import _egcn_hier_ref as RH
import _egcn_ref as R
from pytextgcn_amd import _lib
from pytextgcn_amd import plan as plan_mod

pytestmark = pytest.mark.gpu
TOL = 1e-5
POISON = -777.25
PAD = 3                     # floats behind every row
RATES = (0.0, 0.3, 0.7)

#        M   N    D   n    Fh   h_row0 (None: N)
CASES = [(3, 127, 31, 33, 1, 70),
         (1, 127, 31, 33, 1, 70),
         (64, 127, 1, 1, 0, 0),
         (3, 0, 31, 33, 1, 0),
         (3, 1, 31, 33, 1, 0),
         (3, 129, 31, 33, 1, 70),
         (3, 300, 31, 33, 1, 70),
         (3, 127, 1, 33, 1, 70),
         (3, 127, 33, 33, 1, 70),
         (3, 127, 70, 33, 1, 70),
         (3, 127, 31, 1, 1, 70),
         (3, 127, 31, 100, 1, 70),
         (3, 127, 31, 257, 1, 70),
         (3, 127, 31, 33, 0, 0),
         (3, 127, 31, 33, 17, 70),
         (3, 127, 31, 33, 128, 70),
         (3, 127, 31, 33, 1, 0),
         (3, 127, 31, 33, 1, None),
         (3, 300, 70, 257, 17, 70)]


def _id(c):
    return "M{}-N{}-D{}-n{}-Fh{}-h{}".format(*c)


def test_the_cases_cover_every_value_of_every_axis():
    axes = list(zip(*[(M, N, D, n, Fh, "N" if h0 is None else h0) for M, N, D, n, Fh, h0 in CASES]))
    want = [{1, 3, 64}, {0, 1, 127, 129, 300}, {1, 31, 33, 70}, {1, 33, 100, 257}, {0, 1, 17, 128}, {0, 70, "N"}]
    assert [set(a) for a in axes] == want


class Operands:
    """The operands of one case on the device, padded: one [M D, N + Fh] parameter [E | Eh] as `nn.Linear` keeps it."""

    def __init__(self, case, dev, seed=3):
        M, N, D, n, Fh, h0 = case
        h0 = N if h0 is None else h0
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        self.M, self.N, self.D, self.n, self.Fh, self.h0 = M, N, D, n, Fh, h0
        self.lde, self.ldw, self.ldh, self.ldc = N + Fh + PAD, n + PAD, Fh + PAD, M * n + PAD
        self.weight = (rnd(M * D, self.lde) * 0.7).to(dev)               # E = [:, :N], Eh = [:, N:N + Fh]
        self.b = (rnd(M * D) * 0.5).to(dev)
        self.W = (rnd(M * D, self.ldw) * 0.5).to(dev)
        self.Hd = rnd(max(N - h0, 1), self.ldh).to(dev)
        self.G = rnd(max(N, 1), self.ldc).to(dev)
        self.rates = [RATES[m % 3] for m in range(M)]
        self.seed_values = [int(v) for v in torch.randint(-2 ** 62, 2 ** 62, (M,), generator=gen)]
        self.seeds = torch.tensor(self.seed_values, dtype=torch.int64, device=dev)
        self.p_host = (ctypes.c_double * M)(*self.rates)
        self.dev, self.stream = dev, plan_mod._stream_ptr(dev)

    def outputs(self):
        """poisoned C, dE (the whole [E | Eh] layout), db and dW, a spare row behind the last member"""
        full = lambda *s: torch.full(s, POISON, device=self.dev)
        rows = self.M * self.D + 1
        return dict(C=full(self.N + 1, self.ldc), dE=full(rows, self.lde), db=full(rows), dW=full(rows, self.ldw))


def _ptr(t, offset=0):
    return t.data_ptr() + 4 * offset


def members_forward(o, out, train=True):
    lib = _lib.load()
    st = lib.tgcn_embed_xw_members(_ptr(o.weight), o.lde, _ptr(o.b), _ptr(o.weight, o.N) if o.Fh else None, o.lde,
                                   _ptr(o.Hd) if o.Fh else None, o.ldh, o.h0, o.Fh, _ptr(o.W), o.ldw, _ptr(out["C"]), o.ldc,
                                   o.N, o.D, o.n, o.M, o.p_host, _ptr(o.seeds) if train else None, 0, o.stream)
    assert st == _lib.OK, lib.tgcn_last_error()


def single_forward(o, out, train=True):
    lib = _lib.load()
    for m in range(o.M):
        r0 = m * o.D
        E, b, W, C = _ptr(o.weight, r0 * o.lde), _ptr(o.b, r0), _ptr(o.W, r0 * o.ldw), _ptr(out["C"], m * o.n)
        seed = _ptr(o.seeds, 2 * m) if train else None          # (an int64 is two floats)
        if o.Fh:
            st = lib.tgcn_embed_xw_h(E, o.lde, b, E + 4 * o.N, o.lde, _ptr(o.Hd), o.ldh, o.h0, o.Fh, W, o.ldw, C, o.ldc,
                                     o.N, o.D, o.n, o.rates[m], seed, 0, o.stream)
        else:
            st = lib.tgcn_embed_xw(E, o.lde, b, W, o.ldw, C, o.ldc, o.N, o.D, o.n, o.rates[m], seed, 0, o.stream)
        assert st == _lib.OK, lib.tgcn_last_error()


def _workspace(nbytes, dev):
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)


def members_grad(o, out, want_e=True, want_w=True, train=True):
    lib = _lib.load()
    need = lib.tgcn_embed_xw_members_grad_workspace_bytes(o.N, o.D, o.n, o.Fh, o.M)
    assert need > 0
    ws = _workspace(need, o.dev)
    st = lib.tgcn_embed_xw_members_grad(
        _ptr(o.weight), o.lde, _ptr(o.b), _ptr(o.weight, o.N) if o.Fh else None, o.lde, _ptr(o.Hd) if o.Fh else None, o.ldh,
        o.h0, o.Fh, _ptr(o.W), o.ldw, _ptr(o.G), o.ldc, _ptr(out["dE"]) if want_e else None, o.lde,
        _ptr(out["db"]) if want_e else None, _ptr(out["dE"], o.N) if want_e and o.Fh else None, o.lde,
        _ptr(out["dW"]) if want_w else None, o.ldw, o.N, o.D, o.n, o.M, o.p_host, _ptr(o.seeds) if train else None, 0,
        ws.data_ptr(), need, o.stream)
    assert st == _lib.OK, lib.tgcn_last_error()
    return ws


def single_grad(o, out, want_e=True, want_w=True, train=True):
    lib = _lib.load()
    keep = []
    for m in range(o.M):
        r0 = m * o.D
        E, b, W, G = _ptr(o.weight, r0 * o.lde), _ptr(o.b, r0), _ptr(o.W, r0 * o.ldw), _ptr(o.G, m * o.n)
        dE = _ptr(out["dE"], r0 * o.lde) if want_e else None
        db = _ptr(out["db"], r0) if want_e else None
        dW = _ptr(out["dW"], r0 * o.ldw) if want_w else None
        seed = _ptr(o.seeds, 2 * m) if train else None
        if o.Fh:
            need = lib.tgcn_embed_xw_h_grad_workspace_bytes(o.N, o.D, o.n, o.Fh)
            ws = _workspace(need, o.dev)
            st = lib.tgcn_embed_xw_h_grad(E, o.lde, b, E + 4 * o.N, o.lde, _ptr(o.Hd), o.ldh, o.h0, o.Fh, W, o.ldw, G, o.ldc,
                                          dE, o.lde, db, dE + 4 * o.N if want_e else None, o.lde, dW, o.ldw, o.N, o.D, o.n,
                                          o.rates[m], seed, 0, ws.data_ptr(), ws.numel(), o.stream)
        else:
            need = lib.tgcn_embed_xw_grad_workspace_bytes(o.N, o.D, o.n)
            ws = _workspace(need, o.dev)
            st = lib.tgcn_embed_xw_grad(E, o.lde, b, W, o.ldw, G, o.ldc, dE, o.lde, db, dW, o.ldw, o.N, o.D, o.n, o.rates[m],
                                        seed, 0, ws.data_ptr(), ws.numel(), o.stream)
        assert st == _lib.OK, lib.tgcn_last_error()
        keep.append(ws)
    return keep


def same_bits(got, want):
    torch.cuda.synchronize()
    for name in want:
        assert torch.equal(got[name].view(torch.int32), want[name].view(torch.int32)), name


def poison_intact(o, out, wrote):
    """everything outside the members' blocks of the outputs named in `wrote` holds the poison; the others all of it"""
    M, N, D, n, Fh = o.M, o.N, o.D, o.n, o.Fh
    for name, t in out.items():
        t = t.cpu()
        if name not in wrote:
            assert bool((t == POISON).all()), name
        elif name == "C":
            assert bool((t[N:] == POISON).all()) and bool((t[:, M * n:] == POISON).all())
            assert not bool((t[:N, :M * n] == POISON).any())
        elif name == "dE":
            assert bool((t[M * D:] == POISON).all()) and bool((t[:, N + Fh:] == POISON).all())
            assert not bool((t[:M * D, :N + Fh] == POISON).any())
        elif name == "db":
            assert bool((t[M * D:] == POISON).all()) and not bool((t[:M * D] == POISON).any())
        else:
            assert bool((t[M * D:] == POISON).all()) and bool((t[:, n:] == POISON).all())
            assert not bool((t[:M * D, :n] == POISON).any())


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("train", [True, False], ids=["mixed-rates", "eval"])
def test_forward_is_the_single_call_per_member_bit_for_bit(cuda, case, train):
    o = Operands(case, cuda)
    got, want = o.outputs(), o.outputs()
    members_forward(o, got, train)
    single_forward(o, want, train)
    same_bits(got, want)
    poison_intact(o, got, {"C"})


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("which", ["both", "dE-only", "dW-only"])
def test_gradients_are_the_single_call_per_member_bit_for_bit(cuda, case, which):
    o = Operands(case, cuda)
    want_e, want_w = which != "dW-only", which != "dE-only"
    got, want = o.outputs(), o.outputs()
    held = members_grad(o, got, want_e, want_w), single_grad(o, want, want_e, want_w)
    same_bits(got, want)
    del held
    poison_intact(o, got, ({"dE", "db"} if want_e else set()) | ({"dW"} if want_w else set()))


def test_gradients_in_eval_mode_are_the_single_call_per_member(cuda):
    o = Operands((3, 129, 33, 33, 17, 70), cuda)
    got, want = o.outputs(), o.outputs()
    held = members_grad(o, got, train=False), single_grad(o, want, train=False)
    same_bits(got, want)
    del held
    poison_intact(o, got, {"dE", "db", "dW"})


def test_two_seeds_give_two_masks_and_a_member_at_rate_zero_none(cuda):
    o = Operands((3, 129, 33, 33, 0, 0), cuda)
    a, b, plain = o.outputs(), o.outputs(), o.outputs()
    members_forward(o, a)
    members_forward(o, plain, train=False)
    o.seeds += 1
    members_forward(o, b)
    torch.cuda.synchronize()
    n = o.n
    assert torch.equal(a["C"][:, :n], b["C"][:, :n]) and torch.equal(a["C"][:, :n], plain["C"][:, :n])     # rate 0
    for m in (1, 2):
        assert not torch.equal(a["C"][:, m * n:(m + 1) * n], b["C"][:, m * n:(m + 1) * n])
        assert not torch.equal(a["C"][:, m * n:(m + 1) * n], plain["C"][:, m * n:(m + 1) * n])
    for out in (a, b, plain):
        poison_intact(o, out, {"C"})


@pytest.mark.parametrize("case", [(3, 300, 70, 40, 0, 0), (3, 300, 70, 40, 17, 70)], ids=_id)
def test_forward_and_gradients_against_float64_with_the_mask_per_member(cuda, case):
    o = Operands(case, cuda)
    M, N, D, n, Fh, h0 = o.M, o.N, o.D, o.n, o.Fh, o.h0
    out = o.outputs()
    members_forward(o, out)
    held = members_grad(o, out)
    torch.cuda.synchronize()
    del held
    poison_intact(o, out, {"C", "dE", "db", "dW"})
    errs = {}
    for m in range(M):
        rows, cols = slice(m * D, (m + 1) * D), slice(m * n, (m + 1) * n)
        p = o.rates[m]
        keep = R.keep_matrix(o.seed_values[m], N, D, p) if p > 0 else None
        weight, b, W, G = o.weight[rows, :N + Fh], o.b[rows], o.W[rows, :n], o.G[:N, cols]
        if Fh:
            C, dE, db, dW = RH.truth(weight, b, o.Hd[:, :Fh], h0, W, G, keep, p)
        else:
            C, dE, db, dW = R.fused_truth(weight, b, W, G, keep, p)
        got = dict(C=out["C"][:N, cols], dE=out["dE"][rows, :N + Fh], db=out["db"][rows], dW=out["dW"][rows, :n])
        for name, t in dict(C=C, dE=dE, db=db, dW=dW).items():
            errs[name] = max(errs.get(name, 0.0), R.rel_err(got[name], t))
    print("rel_err against float64:", errs)
    assert all(v <= TOL for v in errs.values()), errs
