"""Guarded device buffers of the exact sweeps (tests/test_gpu_dense_exact.py, tests/test_gpu_spmm_exact.py).  Test
infrastructure."""
import torch


class _Arena:
    """Views carved out of one 1-D pool, each with a guard of more than two rows in front and behind; `fill` sets the part
    in use, `untouched` checks that everything outside the views still holds the fill value."""

    def __init__(self, owner, attr, dtype):
        self.owner, self.attr, self.dtype = owner, attr, dtype
        self.views, self.used = [], 0

    def take(self, rows, width, ld, misalign):
        guard = 2 * ld + 8
        start = (self.used + guard + 3) // 4 * 4 + misalign
        self.views.append((rows, width, ld, start))
        self.used = start + (max(rows - 1, 0) * ld + width if rows else 0) + guard
        return len(self.views) - 1

    def fill(self, value):
        pool = getattr(self.owner, self.attr)
        if pool is None or pool.numel() < self.used:
            setattr(self.owner, self.attr, None)
            pool = torch.empty(max(self.used, 1 << 20), dtype=self.dtype, device=self.owner.dev)
            setattr(self.owner, self.attr, pool)
        assert pool.data_ptr() % 16 == 0
        self.pool, self.value = pool, value
        pool[:self.used].fill_(value)

    def view(self, i, pool=None):
        rows, width, ld, start = self.views[i]
        return (self.pool if pool is None else pool).as_strided((rows, width), (ld, 1), start)

    def ptr(self, i):                  # (data_ptr() of an empty view is null: N = 0 still passes real addresses)
        return self.pool.data_ptr() + self.pool.element_size() * self.views[i][3]

    def untouched(self):
        chk = self.pool[:self.used].clone()
        for i in range(len(self.views)):
            self.view(i, chk).fill_(self.value)
        return bool((chk == self.value).all())
