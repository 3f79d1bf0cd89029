// The keep decision of the fused dropout, shared by every kernel that regenerates a mask from its 8-byte seed (dense.hip:
// the tgcn_gemm_*_dropout products; embed.hip: the fused embedding front end of EGCN), so that all of them -- and
// tests/_dropout_hash.py, which restates it in numpy -- draw the SAME mask.
//
// The hash is split so that the expensive part is paid once per ROW and lane, not once per element: a row key
// (murmur3 mixing of the 64-bit row index with the seed) and, per element, key + col * golden-ratio constant
// through a two-multiply finaliser.  (The first version hashed row * ld + col per element: 4 quarter-rate
// 32-bit multiplies and a 64-bit multiply-add each; profiles/r02_pmc_gemm_c4.md: 4x the vector-ALU instructions
// of the plain kernels.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tgcn {

__device__ __forceinline__ uint32_t drop_row_key(uint32_t s_lo, uint32_t s_hi, int64_t row) {
    uint32_t h = uint32_t(row) ^ s_lo;
    h *= 0xcc9e2d51u;
    h = (h << 15) | (h >> 17);
    h *= 0x1b873593u;
    h ^= uint32_t(uint64_t(row) >> 32) + s_hi;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    return h;
}

__device__ __forceinline__ uint32_t drop_col_term(int col) { return uint32_t(col) * 0x9E3779B1u; }

// keep iff the element's hash reaches the threshold p * 2^32
__device__ __forceinline__ bool drop_hash_keep(uint32_t row_key, uint32_t col_term, uint32_t thresh) {
    uint32_t h = row_key + col_term;
    h ^= h >> 15;
    h *= 0x2c1b3c6du;
    h ^= h >> 12;
    h *= 0x297a2d39u;
    h ^= h >> 15;
    return h >= thresh;
}

// the threshold of rate p < 1 (host side; every entry point clamps it the same way)
inline uint32_t drop_threshold(double p) {
    const double t = p * 4294967296.0;
    return static_cast<uint32_t>(t < 4294967295.0 ? t : 4294967295.0);
}

}  // namespace tgcn
