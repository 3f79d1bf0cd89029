// torch.optim.Adam's step as one elementwise sweep, shared by k_adam (train.hip: one step size for the tensor) and
// k_adam_members / k_adam_member_rows (crossval.hip: one step size per column block / per row block).  The sweep, its
// 16-byte and scalar bodies and the host launcher stand here once; a kernel supplies a rate policy that says where
// element i finds its step size, and nothing else -- so "block k after a step is bit for bit what tgcn_adam_step with
// lr[k] gives" holds by construction.
//
// torch/optim/adam.py (_single_tensor_adam), op for op (adam_element of common.h):
//   g += wd * p;  m.lerp_(g, 1-b1);  v = b2*v + (1-b2)*g*g;  vmax = max(vmax, v)   [amsgrad]
//   denom = sqrt(vmax or v) / sqrt(1 - b2^t) + eps;  p -= (lr / (1 - b1^t)) * m / denom
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace tgcn {
namespace {

constexpr int kMaxRates = 64;          // step sizes of one launch (the members of a grouped network)

struct AdamRates {
    float step_size[kMaxRates];        // lr[k] / (1 - beta1^t), derived in double and rounded once (adam_launch)
};
struct AdamLrs {
    double lr[kMaxRates];
};

// Capturable form: the step count lives on the device (torch's `capturable=True`), so that one captured HIP graph can be
// replayed for every training step.  Thread 0 advances the device step; thread k < K leaves lr[k] / bc1 in scalars[k],
// thread 0 1 / sqrt(bc2) in scalars[K] -- all in double, exactly as the host path derives them.
__global__ __launch_bounds__(64) void k_adam_scalars(int64_t *step, const AdamLrs lrs, int K, double b1, double b2,
                                                     float *scalars) {
    const int64_t s = *step + 1;
    __syncthreads();                    // every thread has read the step before thread 0 advances it
    const double bc1 = 1.0 - pow(b1, static_cast<double>(s));
    if (static_cast<int>(threadIdx.x) < K) scalars[threadIdx.x] = static_cast<float>(lrs.lr[threadIdx.x] / bc1);
    if (threadIdx.x == 0) {
        *step = s;
        const double bc2 = 1.0 - pow(b2, static_cast<double>(s));
        scalars[K] = static_cast<float>(1.0 / sqrt(bc2));
    }
}

// NT: the optimizer state (m, v, vmax) and the gradient are touched once per step -- stream them past
// the caches with non-temporal loads / stores; the parameter itself is the next SpMM's operand and
// keeps plain accesses.
typedef float adam_f4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 ld4(const float *q) {
    if constexpr (NT) {
        const adam_f4 t = __builtin_nontemporal_load(reinterpret_cast<const adam_f4 *>(q));
        return make_float4(t.x, t.y, t.z, t.w);
    } else {
        return *reinterpret_cast<const float4 *>(q);
    }
}
template <bool NT>
__device__ __forceinline__ void st4(float *q, const float4 &a) {
    if constexpr (NT) {
        adam_f4 t = {a.x, a.y, a.z, a.w};
        __builtin_nontemporal_store(t, reinterpret_cast<adam_f4 *>(q));
    } else {
        *reinterpret_cast<float4 *>(q) = a;
    }
}

// ---- rate policies: the step size of element i ---------------------------------------------------------------------
//   wide(i, n)   do the four elements from i on take the 16-byte body (one step size: at(i))?
//   at(i)        the step size of element i
//   cursor(i)    otherwise: walks the elements from i on, rate() / next()

// one step size for the whole tensor; the last one to three elements are the scalar tail
struct UniformRate {
    float step_size;
    struct Cursor {
        float step_size;
        __device__ float rate() const { return step_size; }
        __device__ void next() {}
    };
    __device__ bool wide(int64_t i, int64_t n) const { return i + 3 < n; }
    __device__ float at(int64_t) const { return step_size; }
    __device__ Cursor cursor(int64_t) const { return {step_size}; }
};

// The step sizes of the K members into LDS (the device scalars of the capturable form, or the launch's), and with them
// the device's 1 / sqrt(bc2).  Ends with a barrier: every thread of the workgroup calls it.
__device__ __forceinline__ const float *member_rate_table(const AdamRates &host, int K, const float *dev_scalars,
                                                          float &inv_bc2_sqrt) {
    __shared__ float rate[kMaxRates];
    if (static_cast<int>(threadIdx.x) < K)
        rate[threadIdx.x] = dev_scalars != nullptr ? dev_scalars[threadIdx.x] : host.step_size[threadIdx.x];
    if (dev_scalars != nullptr) inv_bc2_sqrt = dev_scalars[K];
    __syncthreads();
    return rate;
}

// A [n_rows, n_cols] tensor whose column block c / width takes rate[c / width].  V4 (width and n_cols multiples of 4):
// the four elements of a 16-byte body lie in one member, and n is a multiple of 4: no tail.  Otherwise every element
// looks its member up (4-byte accesses).  IDX32: the flat index fits 32 bits (its division is the cheaper one).
template <bool V4, bool IDX32>
struct ColumnBlockRates {
    const float *table;                // member_rate_table()
    uint32_t n_cols, width;
    struct Cursor {
        const float *table;
        uint32_t c, n_cols, width;
        __device__ float rate() const { return table[c / width]; }
        __device__ void next() {
            if (++c == n_cols) c = 0;
        }
    };
    __device__ uint32_t col_of(int64_t i) const {
        return IDX32 ? static_cast<uint32_t>(i) % n_cols : static_cast<uint32_t>(static_cast<uint64_t>(i) % n_cols);
    }
    __device__ bool wide(int64_t, int64_t) const { return V4; }
    __device__ float at(int64_t i) const { return table[col_of(i) / width]; }
    __device__ Cursor cursor(int64_t i) const { return {table, col_of(i), n_cols, width}; }
};

// The members as ROW blocks: a flat tensor of n = K * block elements, element i takes rate[i / block].  Such a tensor
// passes 2^31 elements (12 members at 100 000 nodes and D = 2000 are 2.4e9), so every index here is 64-bit.  V4 (block a
// multiple of 4, hence n too): the four elements of a 16-byte body lie in one member and there is no tail.
template <bool V4>
struct RowBlockRates {
    const float *table;                // member_rate_table()
    int64_t block;
    struct Cursor {
        const float *table;
        int64_t k, left, block;        // `left` elements of member k from here on
        __device__ float rate() const { return table[k]; }
        __device__ void next() {
            if (--left == 0) {
                ++k;
                left = block;
            }
        }
    };
    __device__ bool wide(int64_t, int64_t) const { return V4; }
    __device__ float at(int64_t i) const { return table[i / block]; }
    __device__ Cursor cursor(int64_t i) const {
        const int64_t k = i / block;
        return {table, k, (k + 1) * block - i, block};
    }
};

// ---- the sweep -----------------------------------------------------------------------------------------------------
struct AdamCoef {
    float w1 /* 1-b1 */, b2, w2 /* 1-b2 */, eps, wd, inv_bc2_sqrt;
};

// 256 threads x 4 elements per workgroup and stride: reads p, g, m, v, vmax and writes p, m, v, vmax (36 B/element).
template <bool AMSGRAD, bool NT, class Rate>
__device__ __forceinline__ void adam_sweep(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                           float *__restrict__ v, float *__restrict__ vmax, int64_t n, const AdamCoef &c,
                                           const Rate &rates) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x * 4;
    for (int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if (rates.wide(i, n)) {
            const float step_size = rates.at(i);
            float4 pp = *reinterpret_cast<float4 *>(p + i);
            const float4 gg = ld4<NT>(g + i);
            float4 mm = ld4<NT>(m + i);
            float4 vv = ld4<NT>(v + i);
            float4 xx = make_float4(0.f, 0.f, 0.f, 0.f);
            if (AMSGRAD) xx = ld4<NT>(vmax + i);
            float *P = &pp.x, *M = &mm.x, *V = &vv.x, *X = &xx.x;
            const float *G = &gg.x;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                adam_element(P[k], G[k], M[k], V[k], X[k], AMSGRAD, c.w1, c.b2, c.w2, c.eps, c.wd, step_size, c.inv_bc2_sqrt);
            *reinterpret_cast<float4 *>(p + i) = pp;
            st4<NT>(m + i, mm);
            st4<NT>(v + i, vv);
            if (AMSGRAD) st4<NT>(vmax + i, xx);
        } else {
            auto cur = rates.cursor(i);
            const int64_t end = i + 4 < n ? i + 4 : n;
            for (int64_t j = i; j < end; ++j) {
                float pj = p[j], mj = m[j], vj = v[j], xj = AMSGRAD ? vmax[j] : 0.f;
                adam_element(pj, g[j], mj, vj, xj, AMSGRAD, c.w1, c.b2, c.w2, c.eps, c.wd, cur.rate(), c.inv_bc2_sqrt);
                p[j] = pj;
                m[j] = mj;
                v[j] = vj;
                if (AMSGRAD) vmax[j] = xj;
                cur.next();
            }
        }
    }
}

// ---- host: one launcher --------------------------------------------------------------------------------------------
inline bool adam_aligned(const char *who, const float *param, const float *grad, const float *exp_avg,
                         const float *exp_avg_sq, const float *max_exp_avg_sq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                        reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq) |
                        reinterpret_cast<uintptr_t>(max_exp_avg_sq);
    if (a % 16 != 0) set_error("%s: buffers must be 16-byte aligned", who);
    return a % 16 == 0;
}

// What a launch hands its kernel besides the tensors: workgroups, the rounded constants, the K step sizes.
struct AdamLaunch {
    int grid;
    AdamCoef c;
    AdamRates rates;
};

// The step on n elements at the K rates lr[0..K) (the caller has checked its arguments): derives the constants, runs the
// scalars kernel of the capturable form (step_dev != nullptr; then `step` is 1 and the kernels read scalars_dev), and
// calls launch(AMSGRAD, NT, AdamLaunch) with the two as std::bool_constant -- the caller's kernel with its rate policy.
template <class Launch>
int adam_launch(int64_t n, bool amsgrad, const double *lr, int K, double beta1, double beta2, double eps, double weight_decay,
                int64_t step, int64_t *step_dev, float *scalars_dev, hipStream_t s, Launch &&launch) {
    if (n == 0 && step_dev == nullptr) return TGCN_OK;
    // hyper-parameters are Python floats (doubles) in torch: derive every constant in double and
    // round once, as torch does when it hands `1 - beta2`, `lr / bias_correction1`, ... to its kernels
    const double bc1 = 1.0 - std::pow(beta1, static_cast<double>(step));
    const double bc2 = 1.0 - std::pow(beta2, static_cast<double>(step));
    AdamLaunch a{};
    for (int k = 0; k < K; ++k) a.rates.step_size[k] = static_cast<float>(lr[k] / bc1);
    a.c = {static_cast<float>(1.0 - beta1), static_cast<float>(beta2), static_cast<float>(1.0 - beta2),
           static_cast<float>(eps), static_cast<float>(weight_decay), static_cast<float>(1.0 / std::sqrt(bc2))};
    if (step_dev != nullptr) {
        AdamLrs lrs{};
        for (int k = 0; k < K; ++k) lrs.lr[k] = lr[k];
        k_adam_scalars<<<1, 64, 0, s>>>(step_dev, lrs, K, beta1, beta2, scalars_dev);
        TGCN_HIP_CHECK(hipGetLastError());
        if (n == 0) return TGCN_OK;   // n = 0: only advance the device step (tgcn_spmm_adam applies the update)
    }
    a.grid = static_cast<int>(std::min<int64_t>(8192, (n / 4 + 255) / 256 + 1));
    // large tensors (W1: N x h) stream their state past the caches (measured: 2.9 -> 2.5 ms on 2 M x 200)
    const bool nt = n >= (int64_t(1) << 24);
    if (amsgrad) {
        if (nt) launch(std::true_type{}, std::true_type{}, a); else launch(std::true_type{}, std::false_type{}, a);
    } else {
        if (nt) launch(std::false_type{}, std::true_type{}, a); else launch(std::false_type{}, std::false_type{}, a);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

}  // namespace
}  // namespace tgcn
