"""The fused dropout's keep decision restated in numpy (csrc/dense.hip: drop_row_key, drop_col_term, drop_elem), shared by
the host test of its statistics and the GPU tests that read the kernels' mask back.  Test infrastructure; nothing under
pytextgcn_amd/ imports this."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return x & _M32


def row_key(s_lo, s_hi, rows):
    """murmur3-style mixing of the 64-bit mask row (uint64 array) with the seed's two halves"""
    h = _u32(rows ^ np.uint64(s_lo))
    h = _u32(h * np.uint64(0xCC9E2D51))
    h = _u32((h << np.uint64(15)) | (h >> np.uint64(17)))
    h = _u32(h * np.uint64(0x1B873593))
    h = h ^ _u32((rows >> np.uint64(32)) + np.uint64(s_hi))
    h = h ^ (h >> np.uint64(16))
    return _u32(h * np.uint64(0x85EBCA6B))


def elem(key, cols):
    """the per-element finaliser of a row key and a column (uint64 array)"""
    h = _u32(key + _u32(cols * np.uint64(0x9E3779B1)))
    h = h ^ (h >> np.uint64(15))
    h = _u32(h * np.uint64(0x2C1B3C6D))
    h = h ^ (h >> np.uint64(12))
    h = _u32(h * np.uint64(0x297A2D39))
    return h ^ (h >> np.uint64(15))


def element_hash(seed, rows, cols):
    """32-bit hash of (seed, mask row, column) for every pair of `rows` [R, 1] x `cols` [1, C] (uint64 arrays); `seed`
    is the 64-bit seed as a Python int (the int64 seed tensor's value modulo 2^64)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    return elem(row_key(seed & 0xFFFFFFFF, seed >> 32, rows), cols)


def keep_mask(seed, rows, cols, p):
    """The kernels' keep decision at rate p: hash >= p * 2^32 (the threshold clamped as tgcn_gemm_*_dropout does)."""
    return element_hash(seed, rows, cols) >= np.uint64(min(int(p * 4294967296.0), 4294967295))
