"""GPU tests of Adam with one learning rate per ROW block, libtgcn.so `tgcn_adam_member_rows` and its capturable form
(pytextgcn_amd/csrc/crossval.hip): the update of a `CrossValEGCN`'s stacked tensors.

Adam is elementwise, so everything is compared bit for bit: block k of the flat tensor after a step must be what
`tgcn_adam_step` with lr[k] makes of a contiguous copy of that range, and the capturable form must leave what the host
form leaves, its K + 1 device scalars included.  block in {1, 3, 4, 1023, 4096}: 4-byte accesses (block % 4 != 0) and
16-byte bodies; M in {1, 3, 64}.  One case per path runs past 2^31 elements, where a 32-bit index would wrap."""
import ctypes

import pytest
import torch

import _train_cases as tc
from pytextgcn_amd import _lib
from pytextgcn_amd import plan as plan_mod

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
FILL = -777.25
BLOCKS = (1, 3, 4, 1023, 4096)
MEMBERS = (1, 3, 64)
AMS_WD = ((False, 0.0), (True, 0.0), (False, 0.01), (True, 0.01))


def _rates(K):
    return [(0.1, 0.05, 0.01, 0.001)[k % 4] * (1.0 + k // 4) for k in range(K)]


def _state(n, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    f = lambda: torch.randn(n, generator=gen)
    p, m = f(), f()
    v = torch.rand(n, generator=gen) + 0.1
    vmax = v * (0.5 + torch.rand(n, generator=gen))
    grads = [f() * s for s in (1.0, 0.1, 3.0)]
    return [t.to(dev) for t in (p, m, v, vmax)], [g.to(dev) for g in grads]


def _run(lib, dev, block, K, ams, wd):
    """three steps of the host form, of the capturable form and of K `tgcn_adam_step` calls on contiguous copies of the
    blocks; everything compared bit for bit after every step"""
    n = block * K
    lrs = _rates(K)
    state, grads = _state(n, 1000 * block + K, dev)
    host, capt = [t.clone() for t in state], [t.clone() for t in state]
    blocks = [[t[k * block:(k + 1) * block].clone() for t in state] for k in range(K)]
    lr_host = (ctypes.c_double * K)(*lrs)
    step_dev = torch.zeros((), dtype=I64, device=dev)
    scalars = torch.full((K + 2,), FILL, dtype=F32, device=dev)
    stream = plan_mod._stream_ptr(dev)
    ptrs = lambda ts: [t.data_ptr() for t in ts[:3]] + [ts[3].data_ptr() if ams else None]
    for step, g in enumerate(grads, 1):
        p, m, v, x = ptrs(host)
        assert lib.tgcn_adam_member_rows(p, g.data_ptr(), m, v, x, n, block, K, lr_host, BETA1, BETA2, EPS, wd, step,
                                         stream) == _lib.OK, lib.tgcn_last_error()
        p, m, v, x = ptrs(capt)
        assert lib.tgcn_adam_member_rows_capturable(p, g.data_ptr(), m, v, x, n, block, K, lr_host, BETA1, BETA2, EPS, wd,
                                                    step_dev.data_ptr(), scalars.data_ptr(), stream) == _lib.OK
        for k, blk in enumerate(blocks):
            gk = g[k * block:(k + 1) * block].clone()                     # (a 16-byte aligned copy: tgcn_adam_step asks for one)
            p, m, v, x = ptrs(blk)
            assert lib.tgcn_adam_step(p, gk.data_ptr(), m, v, x, block, lrs[k], BETA1, BETA2, EPS, wd, step, stream) == _lib.OK
        torch.cuda.synchronize()
        assert int(step_dev) == step
        want = [tc.adam_scalars(step, lr, BETA1, BETA2) for lr in lrs]
        got = scalars.cpu().numpy()
        assert [got[k] for k in range(K)] == [w[0] for w in want] and got[K] == want[0][1] and got[K + 1] == FILL
        for i, name in enumerate(("param", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")):
            if i == 3 and not ams:
                assert torch.equal(host[3], state[3]) and torch.equal(capt[3], state[3])              # untouched
                continue
            assert torch.equal(host[i].view(torch.int32), capt[i].view(torch.int32)), (name, step)
            for k, blk in enumerate(blocks):
                assert torch.equal(host[i][k * block:(k + 1) * block].view(torch.int32), blk[i].view(torch.int32)), \
                    (name, step, k)
    assert not torch.equal(host[0], state[0])


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("K", MEMBERS)
def test_adam_member_rows_is_adam_step_on_every_row_block_bit_for_bit(cuda, block, K):
    lib = _lib.load()
    for ams, wd in AMS_WD:
        _run(lib, cuda, block, K, ams, wd)


def test_adam_member_rows_of_size_zero(cuda):
    """a no-op; the capturable form still advances the device step and leaves its scalars"""
    lib = _lib.load()
    lrs = _rates(3)
    lr_host = (ctypes.c_double * 3)(*lrs)
    step_dev = torch.zeros((), dtype=I64, device=cuda)
    scalars = torch.full((5,), FILL, device=cuda)
    stream = plan_mod._stream_ptr(cuda)
    assert lib.tgcn_adam_member_rows(None, None, None, None, None, 0, 0, 3, lr_host, BETA1, BETA2, EPS, 0.0, 1, stream) == _lib.OK
    assert lib.tgcn_adam_member_rows_capturable(None, None, None, None, None, 0, 0, 3, lr_host, BETA1, BETA2, EPS, 0.0,
                                                step_dev.data_ptr(), scalars.data_ptr(), stream) == _lib.OK
    torch.cuda.synchronize()
    assert int(step_dev) == 1
    want = [tc.adam_scalars(1, lr, BETA1, BETA2) for lr in lrs]
    got = scalars.cpu().numpy()
    assert [got[k] for k in range(3)] == [w[0] for w in want] and got[3] == want[0][1] and got[4] == FILL


def test_adam_member_rows_refuses_what_does_not_fit(cuda):
    lib = _lib.load()
    lr_host = (ctypes.c_double * 3)(0.1, 0.1, 0.1)
    t = torch.zeros(16, device=cuda)
    p = t.data_ptr()
    stream = plan_mod._stream_ptr(cuda)
    for n, block, K, lr in ((13, 4, 3, lr_host), (12, 4, 0, lr_host), (12, 4, 65, lr_host), (12, 4, 3, None), (-3, -1, 3, lr_host)):
        assert lib.tgcn_adam_member_rows(p, p, p, p, None, n, block, K, lr, BETA1, BETA2, EPS, 0.0, 1, stream) == _lib.E_INVALID
    assert lib.tgcn_adam_member_rows(p + 4, p, p, p, None, 12, 4, 3, lr_host, BETA1, BETA2, EPS, 0.0, 1, stream) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert not bool(t.any())


@pytest.mark.parametrize("block", [2 ** 30 + 4, 2 ** 30 + 5], ids=["16-byte", "4-byte"])
def test_adam_member_rows_past_two_to_the_31_elements(cuda, block):
    """M = 2 blocks of 2^30 + 4 elements (16-byte bodies) and of 2^30 + 5 (the 4-byte path, whose member counter runs in
    64 bits too).  The update is elementwise, so 1024-element windows at both ends and across the block boundary are
    initialised and compared; the rest of the `torch.empty` buffers is whatever it was."""
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2 ** 30:
        pytest.skip("less than 40 GB of device memory free")
    lib = _lib.load()
    K = 2
    n = block * K
    assert n > 2 ** 31
    lrs = [0.1, 0.001]
    lr_host = (ctypes.c_double * K)(*lrs)
    stream = plan_mod._stream_ptr(cuda)
    big = [torch.empty(n, dtype=F32, device=cuda) for _ in range(4)]             # p, g, m, v: 4 x 8.6 GB (no amsgrad)
    windows = [(0, 1024), (block - 512, block + 512), (n - 1024, n)]
    gen = torch.Generator().manual_seed(31)
    kept = []
    for a, b in windows:
        vals = [torch.randn(b - a, generator=gen).to(cuda) for _ in range(3)] + \
               [(torch.rand(b - a, generator=gen) + 0.1).to(cuda)]
        for t, val in zip(big, vals):
            t[a:b] = val
        kept.append(vals)
    assert lib.tgcn_adam_member_rows(*[t.data_ptr() for t in big], None, n, block, K, lr_host,
                                     BETA1, BETA2, EPS, 0.01, 1, stream) == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    for (a, b), vals in zip(windows, kept):
        for lo, hi in ((a, min(b, block)), (max(a, block), b)):           # the parts of the window in block 0 and in block 1
            if lo >= hi:
                continue
            k = 0 if hi <= block else 1
            want = [t[lo - a:hi - a].clone() for t in vals]
            assert lib.tgcn_adam_step(want[0].data_ptr(), want[1].data_ptr(), want[2].data_ptr(), want[3].data_ptr(),
                                      None, hi - lo, lrs[k], BETA1, BETA2, EPS, 0.01, 1, stream) == _lib.OK
            torch.cuda.synchronize()
            for i in (0, 2, 3):
                assert torch.equal(big[i][lo:hi].view(torch.int32), want[i].view(torch.int32)), (lo, hi, i)
    del big
