// Training-step kernels around the GCN (row A6 of SURVEY.md 8(a): flat_amazon.py:82,89,99-106).
//
//   k_masked_ce    criterion(outputs[g.train_mask], g.y[g.train_mask]) with CrossEntropyLoss('mean')
//                  (flat_amazon.py:82,101-102) and its gradient w.r.t. the full logits matrix, in one
//                  pass over [N, C]: replaces boolean-mask indexing, log_softmax, nll_loss and their
//                  three backward kernels.  HBM-bound: reads N*C*4 (+ 9 B/row), writes N*C*4.
//   k_adam         torch.optim.Adam(..., amsgrad=True).step() (flat_amazon.py:89,106), one fused
//                  elementwise pass: reads p, g, m, v, vmax and writes p, m, v, vmax (36 B/element)
//                  instead of ~10 separate multi-tensor kernels.  HBM-bound.
// Both are deterministic (fixed-order two-stage reductions, no atomics).  The row body of the cross-entropy (masked_ce.h) and
// the sweep and launcher of Adam (adam.h) are shared with the member kernels of crossval.hip: a kernel here is a view or a
// rate policy handed to that one text.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "adam.h"
#include "common.h"
#include "masked_ce.h"

namespace tgcn {
namespace {

constexpr int kCeBlocks = 2048;

// One [n_rows, C] matrix, row r selected by mask[r]: the rows of ce_rows (masked_ce.h) with nothing padded.
struct FlatRows {
    static constexpr bool kPadded = false;
    const float *logits;
    int64_t ld;
    int C;
    const int64_t *target;
    const uint8_t *mask;
    int64_t n_rows;
    float inv_count;
    float *dlogits;
    int64_t ldd;
    float *partial;             // [gridDim.x]
    int64_t *pred;              // [n_rows] or nullptr
    float *colpart;             // [gridDim.x][C] or nullptr
    __device__ int width() const { return C; }
    __device__ bool selected(int64_t r) const { return mask[r] != 0; }
    __device__ const float *row(int64_t r) const { return logits + r * ld; }
    __device__ float *drow(int64_t r) const { return dlogits + r * ldd; }
    __device__ bool want_pred() const { return pred != nullptr; }
    __device__ void set_pred(int64_t r, int c) const { pred[r] = c; }
    __device__ float *partial_slot() const { return partial + blockIdx.x; }
    __device__ float *colpart_row() const { return colpart + int64_t(blockIdx.x) * C; }
};

template <int LPR, bool V4, int KPL = 4>
__global__ __launch_bounds__(256) void k_masked_ce(const float *__restrict__ logits, int64_t ld, int C,
                                                   const int64_t *__restrict__ target,
                                                   const uint8_t *__restrict__ mask, int64_t n_rows,
                                                   float inv_count, float *__restrict__ dlogits,
                                                   int64_t ldd, float *__restrict__ partial,
                                                   int64_t *__restrict__ pred, float *__restrict__ colpart) {
    ce_rows<LPR, V4, KPL>(FlatRows{logits, ld, C, target, mask, n_rows, inv_count, dlogits, ldd, partial, pred, colpart});
}

// x *= *scale unless the device scalar is exactly 1 (the seed `loss.backward()` hands to the loss node): the
// multiplication by 1.0f is the identity bit for bit, so skipping the pass changes nothing.
__global__ __launch_bounds__(256) void k_scale_unless_one(float *__restrict__ x, int64_t n, const float *__restrict__ scale) {
    const float s = *scale;
    if (s == 1.0f) return;
    const int64_t stride = int64_t(gridDim.x) * 256;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) x[i] *= s;
}

__global__ void k_ce_final(const float *__restrict__ partial, int n, float inv_count,
                           float *__restrict__ loss) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = red[0] * inv_count;
}

// The sweep of adam.h at one step size: the launch's, or scalars[0] of the capturable form.
template <bool AMSGRAD, bool NT>
__global__ __launch_bounds__(256) void k_adam(float *__restrict__ p, const float *__restrict__ g,
                                              float *__restrict__ m, float *__restrict__ v,
                                              float *__restrict__ vmax, int64_t n, float w1 /* 1-b1 */,
                                              float b2, float w2 /* 1-b2 */, float eps, float wd,
                                              float step_size, float inv_bc2_sqrt,
                                              const float *__restrict__ dev_scalars) {
    if (dev_scalars != nullptr) {
        step_size = dev_scalars[0];
        inv_bc2_sqrt = dev_scalars[1];
    }
    adam_sweep<AMSGRAD, NT>(p, g, m, v, vmax, n, AdamCoef{w1, b2, w2, eps, wd, inv_bc2_sqrt}, UniformRate{step_size});
}

}  // namespace
}  // namespace tgcn

extern "C" {

size_t tgcn_masked_ce_workspace_bytes(void) { return sizeof(float) * tgcn::kCeBlocks; }

int tgcn_masked_ce(const float *logits, int64_t ld, int64_t n_rows, int n_classes,
                   const int64_t *target, const uint8_t *mask, float inv_count, float *loss,
                   float *dlogits, int64_t ldd, void *workspace, size_t workspace_bytes,
                   tgcn_stream stream) {
    return tgcn_masked_ce_pred(logits, ld, n_rows, n_classes, target, mask, inv_count, loss, dlogits, ldd,
                               nullptr, workspace, workspace_bytes, stream);
}

static int masked_ce_impl(const char *who, const float *logits, int64_t ld, int64_t n_rows, int n_classes,
                          const int64_t *target, const uint8_t *mask, float inv_count, float *loss,
                          float *dlogits, int64_t ldd, float *dbias, int64_t *pred, void *workspace,
                          size_t workspace_bytes, size_t workspace_need, tgcn_stream stream) {
    using namespace tgcn;
    if (!logits || !target || !mask || !loss || n_rows < 0 || n_classes <= 0 || ld < n_classes ||
        (dlogits && ldd < n_classes) || (dbias && !dlogits)) {
        set_error("%s: bad argument (n_rows=%lld C=%d ld=%lld)", who, (long long)n_rows, n_classes, (long long)ld);
        return TGCN_E_INVALID;
    }
    if (!workspace || workspace_bytes < workspace_need) {
        set_error("%s: workspace of %zu bytes given, %zu needed", who, workspace_bytes, workspace_need);
        return TGCN_E_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *partial = static_cast<float *>(workspace);
    const int C = n_classes;
    const bool v4 = ce_v4(C, logits, ld, dlogits, ldd);
    // the column sums ride along on the register path (C <= 256); wider rows take a separate pass below
    float *colpart = (dbias && C <= 256) ? partial + kCeBlocks : nullptr;
    int grid = 0;
    ce_dispatch(C, v4, [&](auto lpr, auto kpl, auto vec) {
        grid = ce_grid(n_rows, lpr, kCeBlocks);
        k_masked_ce<lpr, vec, kpl><<<grid, 256, 0, s>>>(logits, ld, C, target, mask, n_rows, inv_count, dlogits, ldd, partial,
                                                        pred, colpart);
    });
    TGCN_HIP_CHECK(hipGetLastError());
    k_ce_final<<<1, 256, 0, s>>>(partial, grid, inv_count, loss);
    TGCN_HIP_CHECK(hipGetLastError());
    if (dbias) {
        if (colpart) return launch_colsum_final(colpart, grid, C, dbias, s);
        return launch_colsum(dlogits, ldd, n_rows, C, dbias, partial + kCeBlocks, colsum_blocks(n_rows), s);
    }
    return TGCN_OK;
}

int tgcn_masked_ce_pred(const float *logits, int64_t ld, int64_t n_rows, int n_classes,
                        const int64_t *target, const uint8_t *mask, float inv_count, float *loss,
                        float *dlogits, int64_t ldd, int64_t *pred, void *workspace,
                        size_t workspace_bytes, tgcn_stream stream) {
    return masked_ce_impl("tgcn_masked_ce", logits, ld, n_rows, n_classes, target, mask, inv_count, loss, dlogits, ldd,
                          nullptr, pred, workspace, workspace_bytes, tgcn_masked_ce_workspace_bytes(), stream);
}

size_t tgcn_masked_ce_grad_workspace_bytes(int64_t n_rows, int n_classes) {
    if (n_rows < 0 || n_classes <= 0) return 0;
    const size_t rows = std::max<size_t>(tgcn::kCeBlocks, static_cast<size_t>(tgcn::colsum_blocks(n_rows)));
    return sizeof(float) * (tgcn::kCeBlocks + rows * static_cast<size_t>(n_classes));
}

int tgcn_masked_ce_grad(const float *logits, int64_t ld, int64_t n_rows, int n_classes,
                        const int64_t *target, const uint8_t *mask, float inv_count, float *loss,
                        float *dlogits, int64_t ldd, float *dbias, int64_t *pred, void *workspace,
                        size_t workspace_bytes, tgcn_stream stream) {
    if (!dlogits || !dbias) {
        tgcn::set_error("tgcn_masked_ce_grad: dlogits and dbias are required (use tgcn_masked_ce for the loss alone)");
        return TGCN_E_INVALID;
    }
    return masked_ce_impl("tgcn_masked_ce_grad", logits, ld, n_rows, n_classes, target, mask, inv_count, loss, dlogits,
                          ldd, dbias, pred, workspace, workspace_bytes,
                          tgcn_masked_ce_grad_workspace_bytes(n_rows, n_classes), stream);
}

int tgcn_scale_by_device_scalar(float *x, int64_t n, const float *scale_dev, tgcn_stream stream) {
    using namespace tgcn;
    if (n < 0 || (n > 0 && !x) || !scale_dev) {
        set_error("tgcn_scale_by_device_scalar: bad argument (n=%lld)", (long long)n);
        return TGCN_E_INVALID;
    }
    if (n == 0) return TGCN_OK;
    const int grid = static_cast<int>(std::min<int64_t>(4096, (n + 255) / 256));
    k_scale_unless_one<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(x, n, scale_dev);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

static int adam_impl(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                     float *max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int64_t step, int64_t *step_dev, float *scalars_dev,
                     tgcn_stream stream);

int tgcn_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                   float *max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int64_t step, tgcn_stream stream) {
    return adam_impl(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                     step, nullptr, nullptr, stream);
}

int tgcn_adam_step_capturable(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                              float *max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                              double eps, double weight_decay, int64_t *step_dev, float *scalars_dev,
                              tgcn_stream stream) {
    if (!step_dev || !scalars_dev) {
        tgcn::set_error("tgcn_adam_step_capturable: step_dev / scalars_dev must be device pointers");
        return TGCN_E_INVALID;
    }
    return adam_impl(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                     1, step_dev, scalars_dev, stream);
}

static int adam_impl(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                     float *max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int64_t step, int64_t *step_dev, float *scalars_dev,
                     tgcn_stream stream) {
    using namespace tgcn;
    if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0 || step < 1) {
        set_error("tgcn_adam_step: bad argument (n=%lld step=%lld)", (long long)n, (long long)step);
        return TGCN_E_INVALID;
    }
    if (!adam_aligned("tgcn_adam_step", param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq)) return TGCN_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return adam_launch(n, max_exp_avg_sq != nullptr, &lr, 1, beta1, beta2, eps, weight_decay, step, step_dev, scalars_dev, s,
                       [&](auto ams, auto nt, const AdamLaunch &a) {
                           k_adam<ams, nt><<<a.grid, 256, 0, s>>>(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, a.c.w1,
                                                                  a.c.b2, a.c.w2, a.c.eps, a.c.wd, a.rates.step_size[0],
                                                                  a.c.inv_bc2_sqrt, scalars_dev);
                       });
}

}  // extern "C"
