/* tgcn.h -- C ABI of the MI355X-native TextGCN hot path (libtgcn.so, HIP, gfx950 only).
 *
 * The reference has no FFI on this path: the arithmetic is PyG-1.6.3 `GCNConv`, reached from
 * textgcn/lib/models.py:20 `layer(x, g.edge_index, g.edge_attr)` and differentiated by autograd at
 * flat_amazon.py:105 `loss.backward()`.  This header is the boundary a maintainer binds instead
 * (ctypes stub in INTEGRATION.md); each entry point names the reference step it replaces.
 *
 * Conventions
 *   - plain C, `extern "C"`, no torch types; every data pointer is a DEVICE pointer on the plan's
 *     device unless the comment says "host"; the caller owns every buffer it passes, the library
 *     owns only the opaque plan (which holds its own copies of the graph).
 *   - every function returns a status: 0 ok, <0 error (TGCN_E_*); tgcn_last_error() returns a
 *     thread-local, human readable message for the last failing call on this thread.  Nothing
 *     throws, nothing aborts the process.
 *   - compute entry points (tgcn_spmm, tgcn_colsum) only ENQUEUE on the caller's stream,
 *     never allocate and never synchronise (hipGraph-capturable).  tgcn_plan_create allocates and
 *     synchronises `stream` (it is a one-off per graph).
 *   - a plan is immutable after creation: safe to share between threads and streams as long as
 *     concurrent calls use distinct workspaces.
 *   - all arithmetic is IEEE fp32; results are bitwise reproducible run to run (no floating-point atomics;
 *     the word-word graph builder uses integer atomics, whose sums do not depend on the order).  The one
 *     exception is opt-in: tgcn_set_gemm_split(1) forms the products of three dense kernels from exact bf16
 *     splits of their fp32 operands (fp32-accurate and still reproducible, but not the fp32 FMA chain).
 */
#ifndef TGCN_H_
#define TGCN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGCN_ABI_VERSION 7

enum {
    TGCN_OK = 0,
    TGCN_E_INVALID = -1,   /* bad argument (null pointer, negative size, misaligned, F <= 0 ...) */
    TGCN_E_RANGE = -2,     /* edge_index entry outside [0, n_nodes) or size beyond int32 limits   */
    TGCN_E_HIP = -3,       /* a HIP runtime call failed (message carries hipGetErrorString)       */
    TGCN_E_NOMEM = -4,     /* device or host allocation failed                                    */
    TGCN_E_WORKSPACE = -5  /* workspace smaller than tgcn_*_workspace_bytes()                     */
};

typedef struct tgcn_plan tgcn_plan;   /* opaque */
typedef void *tgcn_stream;            /* a hipStream_t; NULL = the null stream */

int tgcn_abi_version(void);
const char *tgcn_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * tgcn_plan_create -- replaces PyG-1.6.3 gcn_norm (k1-k4 of SURVEY.md 2a), which the reference
 * re-runs inside every GCNConv call (models.py:11-15 never pass cached=True): drop existing
 * self-loops and re-append one per node (kept weight, else 1.0 -- add_remaining_self_loops, last
 * duplicate wins), in-degree at the TARGET `dst = edge_index[1]` incl. the loop, d^-1/2 with inf->0,
 * w_hat = d^-1/2[src] * w * d^-1/2[dst].  The result is kept as M (M[dst,src] = w_hat) in CSR sorted
 * by (dst, src) -- and M^T likewise unless M == M^T bitwise -- with (col,val) interleaved as 8-byte
 * pairs, plus the work-item partition the SpMM kernel walks.
 *
 *   n_nodes, n_edges      N and E = edge_index.shape[1]
 *   src, src_stride       edge_index[0] (int64) and its element stride: the reference passes the
 *   dst, dst_stride       non-contiguous view `coo.T` (text2graph.py:192), so strides are honoured
 *   w                     edge_attr (fp32, contiguous) or NULL for all-ones
 *   add_self_loops        GCNConv(add_self_loops=...) -- the reference always passes True; the value
 *                         is also the weight of an added loop: 1 -> 1.0, 2 -> 2.0 (improved=True)
 *   normalize             GCNConv(normalize=...)      -- the reference keeps the default True; as in
 *                         PyG, loops are added inside gcn_norm, i.e. only when normalize != 0.  The value also
 *                         selects how a node's degree is summed (enum below):
 *                           TGCN_NORM_ACCURATE (1)   float64 sum, rounded to fp32 once (the default of the Python layer);
 *                                                    w_hat = w * (d^-1/2[src] * d^-1/2[dst]): a symmetric graph stays
 *                                                    BITWISE symmetric and M^T is not stored;
 *                           TGCN_NORM_REFERENCE (2)  the bits of the reference's CPU path: ONE fp32 accumulator per node,
 *                                                    weights added sequentially in edge order, the self loop last (PyG
 *                                                    scatter_add on the CPU after add_remaining_self_loops), and PyG's
 *                                                    association (d^-1/2[src] * w) * d^-1/2[dst] -- on hub nodes with
 *                                                    ~10^6 edges this differs from the accurate sum by a few 1e-5 relative.
 *   row_begin, row_end    rows [row_begin,row_end) of M and of M^T that this plan will produce
 *                         (1-D row partition across GPUs); 0, n_nodes for the whole graph.  The
 *                         normalisation is always computed over the WHOLE edge list.
 *   device                HIP device ordinal that owns every pointer
 */
enum { TGCN_NORM_OFF = 0, TGCN_NORM_ACCURATE = 1, TGCN_NORM_REFERENCE = 2 };   /* `normalize` of tgcn_plan_create */
enum { TGCN_DEGREE_ACCURATE = 0, TGCN_DEGREE_REFERENCE = 1 };                  /* `degree_sum` of tgcn_gcn_norm    */
int tgcn_plan_create(int64_t n_nodes, int64_t n_edges,
                     const int64_t *src, int64_t src_stride,
                     const int64_t *dst, int64_t dst_stride,
                     const float *w, int add_self_loops, int normalize,
                     int64_t row_begin, int64_t row_end,
                     int device, tgcn_stream stream, tgcn_plan **out);

/* tgcn_plan_create_coo -- a plan from explicit triplets M[row[i], col[i]] = val[i] (n_rows x n_cols,
 * no loops added, no normalisation, duplicates add up).  It has no counterpart in the reference,
 * which is single-device (flat_amazon.py:84-86): this is what the 1-D partition across GPUs builds
 * its per-rank local operators from (pytextgcn_amd/sharded.py).  `val` NULL = ones.
 * with_transpose = 0 keeps only M (tgcn_spmm(transpose=1) then fails with TGCN_E_INVALID). */
int tgcn_plan_create_coo(int64_t n_rows, int64_t n_cols, int64_t nnz,
                         const int64_t *row, const int64_t *col, const float *val,
                         int with_transpose, int device, tgcn_stream stream, tgcn_plan **out);

/* tgcn_gcn_norm -- the normalisation half of tgcn_plan_create on its own (PyG-1.6.3 gcn_norm as the
 * reference runs it, models.py:11-20): for every node dis[n] = deg[n]^-1/2 (inf -> 0) with deg the weighted
 * in-degree at the target incl. the self loop, and loop_w[n] = the weight of that loop (the last input loop's,
 * else add_self_loops as 1.0 / 2.0; all zeros when add_self_loops = 0).  The normalised weight of edge e is
 * then w[e] * (dis[src] * dis[dst]) -- (dis[src] * w[e]) * dis[dst] in the reference-order mode -- the association
 * tgcn_plan_create uses.  It IS the routine tgcn_plan_create runs (degree_sum = TGCN_DEGREE_ACCURATE / _REFERENCE as
 * its normalize = TGCN_NORM_ACCURATE / _REFERENCE): same chunking, same sums, same bits.  No counterpart in the single-
 * device reference: the 1-D partition (pytextgcn_amd/sharded.py) calls it so that every rank can cut its own
 * local operators out of the edge list WITHOUT building the whole-graph plan -- the edge list is walked in
 * chunks (TGCN_NORM_CHUNK edges, default 2^25), scratch is O(chunk) + O(n_nodes); deterministic.
 *   dis, loop_w   fp32 [n_nodes] device buffers (loop_w may be NULL)
 * Allocates scratch and synchronises `stream` (one-off per graph, like tgcn_plan_create). */
int tgcn_gcn_norm(int64_t n_nodes, int64_t n_edges,
                  const int64_t *src, int64_t src_stride,
                  const int64_t *dst, int64_t dst_stride,
                  const float *w, int add_self_loops, int degree_sum, float *dis, float *loop_w,
                  int device, tgcn_stream stream);

int tgcn_plan_destroy(tgcn_plan *plan);

/* tgcn_plan_query -- integers describing a plan (host pointer `out`). */
enum {
    TGCN_Q_N_NODES = 0,      /* N (= number of columns of M and M^T)                              */
    TGCN_Q_N_ROWS = 1,       /* row_end - row_begin                                               */
    TGCN_Q_NNZ = 2,          /* stored non-zeros of the forward block (E - loops_in_input + N ...) */
    TGCN_Q_NNZ_T = 3,        /* ... of the transposed block                                       */
    TGCN_Q_SYMMETRIC = 4,    /* 1 when M == M^T bitwise (the transposed copy is then not kept)    */
    TGCN_Q_ITEMS = 5,        /* work items (wavefront tasks) of the forward block                 */
    TGCN_Q_ITEMS_T = 6,
    TGCN_Q_LONG_ROWS = 7,    /* rows split into segments (second-pass reduce), forward block      */
    TGCN_Q_LONG_ROWS_T = 8,
    TGCN_Q_SEGMENTS = 9,     /* carry rows written per SpMM, forward block                        */
    TGCN_Q_SEGMENTS_T = 10,
    TGCN_Q_DEVICE_BYTES = 11,/* device memory held by the plan                                    */
    TGCN_Q_ROW_BEGIN = 12,
    TGCN_Q_HAS_TRANSPOSE = 13,/* 0 for a tgcn_plan_create_coo(with_transpose = 0) plan                */
    TGCN_Q_N_ROWS_T = 14,    /* rows of the transposed block (= columns of the forward block)      */
    TGCN_Q_HOT_ROWS = 15,    /* rows computed by the dense hot block (0 or up to 32), forward block  */
    TGCN_Q_HOT_ROWS_T = 16
};
int tgcn_plan_query(const tgcn_plan *plan, int what, int64_t *out);

/* tgcn_plan_export -- copy the stored CSR out (device buffers sized from tgcn_plan_query); any
 * pointer may be NULL.  For tests and for the INTEGRATION.md binding; not on the hot path. */
int tgcn_plan_export(const tgcn_plan *plan, int transpose, int32_t *rowptr /* n_rows+1 */,
                     int32_t *col /* nnz */, float *val /* nnz */, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * tgcn_spmm -- replaces MessagePassing.propagate + bias of GCNConv.forward (k6-k9: index_select,
 * scale, scatter_add, `out += bias`) when transpose = 0, and its autograd (b1-b4: dXW = M^T dOut)
 * when transpose = 1:
 *       Y[r, 0:F] = sum_j  M(^T)[row_begin + r, j] * X[j, 0:F]  (+ bias[0:F])
 *   X    [n_nodes, F] fp32, row stride ldx (elements)        -- the gathered operand
 *   Y    [n_rows,  F] fp32, row stride ldy                    -- fully overwritten
 *   bias [F] or NULL
 * Fast path: F, ldx, ldy multiples of 4 and X, Y, bias 16-byte aligned; anything else takes the
 * scalar-lane kernel (same results).  Nothing of size nnz x F is ever written.
 * Plans of graphs whose 32 longest rows are nearly dense (TGCN_Q_HOT_ROWS > 0) compute those rows as a
 * dense product over all columns: with a non-finite value in X[c] they become non-finite even where
 * M[row, c] == 0 (0 * inf).  Finite operands give the reference's result; TGCN_HOT_ROWS=0 in the
 * environment at plan creation disables the dense block.
 */
size_t tgcn_spmm_workspace_bytes(const tgcn_plan *plan, int transpose, int F);
int tgcn_spmm(const tgcn_plan *plan, int transpose, const float *X, int64_t ldx, int F,
              const float *bias, float *Y, int64_t ldy, void *workspace, size_t workspace_bytes,
              tgcn_stream stream);

/* tgcn_spmm_split -- tgcn_spmm whose gathered operand lives in two buffers: rows (= columns of the
 * operator) [0, split) in X, rows [split, n_cols) in X2 (row r of X2 is column split + r).  No
 * counterpart in the reference (single device); the 1-D partition keeps the all-gathered hub block
 * and the rank's own rows apart and so avoids one copy per SpMM.  X2 = NULL is tgcn_spmm. */
int tgcn_spmm_split(const tgcn_plan *plan, int transpose, const float *X, int64_t ldx, const float *X2,
                    int64_t ldx2, int64_t split, int F, const float *bias, float *Y, int64_t ldy,
                    void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* tgcn_spmm_acc -- the ACCUMULATE form of tgcn_spmm_split:  Y[r, 0:F] += sum_j M(^T)[r, j] * X[j, 0:F]  for every row r
 * that holds at least one stored entry; a row without entries is neither read nor written, and there is no bias.  No
 * counterpart in the single-device reference: the 1-D partition of a graph WITHOUT hub structure (BASELINE config 5) cuts a
 * rank's operator by the origin of its columns into blocks and runs block k -- accumulating into the same Y -- as soon as
 * the operand rows of exchange stage k have landed, so that stage k + 1 travels under the compute of stage k
 * (pytextgcn_amd/sharded.py, `exchange="pipeline"`; SURVEY.md 8(e) "run local part while halo is in flight").  A row is owned
 * by one wavefront and launches on one stream are ordered, so the sums are reproducible run to run (their association
 * differs from the one-launch product's: block partial sums are added in launch order).  X2 = NULL: single operand.
 * Workspace: tgcn_spmm_workspace_bytes(plan, transpose, F). */
int tgcn_spmm_acc(const tgcn_plan *plan, int transpose, const float *X, int64_t ldx, const float *X2, int64_t ldx2,
                  int64_t split, int F, float *Y, int64_t ldy, void *workspace, size_t workspace_bytes,
                  tgcn_stream stream);

/* tgcn_spmm_act -- tgcn_spmm with an activation applied to M(^T) X + bias in the epilogue:
 *       Y[r, 0:F] = act( sum_j M(^T)[row_begin + r, j] * X[j, 0:F]  (+ bias[0:F]) )
 * The reference constructs `self.activation` and comments its call out (textgcn/lib/models.py:9,22); this is that line
 * restored at no extra traffic -- the finished row is in registers when the bias is added.  act = TGCN_ACT_RELU stores
 * v < 0 ? 0 : v (a NaN goes through, as torch.relu does): the same sums in the same order as tgcn_spmm and one select, so
 * the result equals relu(tgcn_spmm(...)) bit for bit; act = TGCN_ACT_NONE IS tgcn_spmm.  Any other value: TGCN_E_INVALID.
 * Same argument checks, same workspace (tgcn_spmm_workspace_bytes) as tgcn_spmm. */
enum { TGCN_ACT_NONE = 0, TGCN_ACT_RELU = 1 };
int tgcn_spmm_act(const tgcn_plan *plan, int transpose, const float *X, int64_t ldx, int F, const float *bias, int act,
                  float *Y, int64_t ldy, void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* tgcn_act_grad -- the backward of that activation, in place:  G[r, c] <- A[r, c] > 0 ? G[r, c] : 0  for the [n_rows, F]
 * gradient G (stride ldg) and A (stride lda) the activation tgcn_spmm_act STORED: relu(a) > 0 <=> a > 0, so the output is
 * its own gate and neither a mask nor the pre-activation is kept.  colsum != NULL: also colsum[c] = sum_r of the GATED
 * G[r, c] -- the bias gradient of the layer (the autograd of `out += bias` under the activation) -- from the registers
 * that hold each row, in tgcn_colsum's fixed order (no atomics: reproducible run to run).  act = TGCN_ACT_NONE leaves G
 * as it is (colsum is then tgcn_colsum's).  float4 lanes when F, lda, ldg are multiples of 4 and A, G 16-byte aligned,
 * scalar lanes otherwise (same results); row offsets are 64-bit.  The workspace is needed only with colsum. */
size_t tgcn_act_grad_workspace_bytes(int64_t n_rows, int F);
int tgcn_act_grad(int act, const float *A, int64_t lda, float *G, int64_t ldg, int64_t n_rows, int F, float *colsum,
                  void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* tgcn_spmm_adam -- tgcn_spmm whose result rows are never stored: row r of M(^T) @ G is the GRADIENT of row r of
 * `param` and is spent at once on torch.optim.Adam's update of that row (the arithmetic of tgcn_adam_step, op for
 * op; max_exp_avg_sq = NULL means amsgrad=False).  For TextGCN's one-hot features the first layer's weight
 * gradient IS such a product, dW1 = M^T dH1 (the reference computes it at
 * flat_amazon.py:105 and applies it at :106): fusing the two removes the N x h gradient and the optimizer's own pass
 * over W1 and its state.  Same bits as tgcn_spmm followed by tgcn_adam_step.
 *   G [n_cols, F] fp32 stride ldg;  param / exp_avg / exp_avg_sq / max_exp_avg_sq [n_rows, F] stride ldp
 *   F %% 4 == 0, strides multiples of 4, 16-byte aligned buffers (no scalar fallback: TGCN_E_INVALID otherwise)
 *   step  1-based step count AFTER increment; with scalars_dev != NULL the two step-dependent factors are read
 *         from that device buffer instead ({lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)}, as tgcn_adam_step_capturable
 *         leaves them in its `scalars_dev`), so that a captured HIP graph can be replayed per step.
 * Workspace: tgcn_spmm_workspace_bytes(plan, transpose, F). */
int tgcn_spmm_adam(const tgcn_plan *plan, int transpose, const float *G, int64_t ldg, int F, float *param,
                   float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq, int64_t ldp, double lr,
                   double beta1, double beta2, double eps, double weight_decay, int64_t step,
                   const float *scalars_dev, void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* tgcn_spmm_adam_split -- tgcn_spmm_adam whose gathered operand lives in two buffers, as tgcn_spmm_split's does: rows
 * [0, split) in G, rows [split, n_cols) in G2.  For the 1-D partition's backward SpMM: the regular rows of a rank's W1
 * shard are updated inside the launch that computes their gradient from the gathered hub block and the rank's own rows.
 * G2 = NULL is tgcn_spmm_adam. */
int tgcn_spmm_adam_split(const tgcn_plan *plan, int transpose, const float *G, int64_t ldg, const float *G2, int64_t ldg2,
                         int64_t split, int F, float *param, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                         int64_t ldp, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                         const float *scalars_dev, void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* Row movement of the multi-GPU exchange (pytextgcn_amd/sharded.py; nothing in the reference corresponds: it is
 * single-device, flat_amazon.py:84-86).  Row-major fp32 rows, int64 row indices on the device, enqueue only.
 *   tgcn_rows_gather          out[i, :]    = x[idx[i], :]     (pack the hub rows a peer references)
 *   tgcn_rows_scatter         y[idx[i], :] = x[i, :]          (place received rows in the gathered block; idx distinct)
 *   tgcn_rows_reduce_ranked   y[row0 + j * row_step, :] += sum over q = 0 .. n_ranks-1, IN THAT ORDER, of
 *                             recv[inv[q * n + j], :]  (inv < 0: rank q sent nothing for row j), j = 0 .. n-1:
 *                             the reduce-scatter's local sum -- starting from zero, ranks in order, one add into y:
 *                             the summation order all exchange forms share, so that they agree bit for bit.
 * n_x_rows / n_y_rows / n_recv_rows are the row counts of the INDEXED buffers: an index outside them is skipped on the
 * device (the calls only enqueue and cannot report it), so a bad list can never read or write outside a buffer;
 * tgcn_rows_reduce_ranked returns TGCN_E_RANGE when row0 + (n - 1) * row_step >= n_y_rows. */
int tgcn_rows_gather(const float *x, int64_t ldx, int64_t n_x_rows, const int64_t *idx, int64_t n, int F, float *out,
                     int64_t ldo, tgcn_stream stream);
int tgcn_rows_scatter(const float *x, int64_t ldx, const int64_t *idx, int64_t n, int F, float *y, int64_t ldy,
                      int64_t n_y_rows, tgcn_stream stream);
int tgcn_rows_reduce_ranked(const float *recv, int64_t ldr, int64_t n_recv_rows, const int32_t *inv, int n_ranks,
                            int64_t n, int F, float *y, int64_t ldy, int64_t n_y_rows, int64_t row0, int64_t row_step,
                            tgcn_stream stream);

/* tgcn_colsum -- replaces the autograd of `out += bias` (db = sum over rows of dOut).
 *   G [n_rows, F] fp32 stride ldg -> out [F]. */
size_t tgcn_colsum_workspace_bytes(int64_t n_rows, int F);
int tgcn_colsum(const float *G, int64_t ldg, int64_t n_rows, int F, float *out, void *workspace,
                size_t workspace_bytes, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Training-step helpers (the caller of the path: flat_amazon.py:82,89,99-106).
 *
 * tgcn_masked_ce -- `CrossEntropyLoss(reduction='mean')(logits[mask], target[mask])`
 * (flat_amazon.py:82,101-102) and, when dlogits != NULL, its gradient w.r.t. the FULL logits matrix
 * (rows outside the mask get zeros), in one pass.
 *   logits [n_rows, n_classes] fp32 stride ld;  target int64 [n_rows];  mask uint8/bool [n_rows]
 *   inv_count = 1 / (number of rows in the mask) -- a host value: masks are static, count them once
 *   loss      device scalar (fp32);  dlogits [n_rows, n_classes] stride ldd or NULL
 */
size_t tgcn_masked_ce_workspace_bytes(void);
int tgcn_masked_ce(const float *logits, int64_t ld, int64_t n_rows, int n_classes,
                   const int64_t *target, const uint8_t *mask, float inv_count, float *loss,
                   float *dlogits, int64_t ldd, void *workspace, size_t workspace_bytes,
                   tgcn_stream stream);
/* tgcn_masked_ce_pred -- the same pass also writes pred[r] = argmax_c logits[r, c] (first index on
 * ties) for EVERY row when pred != NULL: the predictions the reference takes on the host with
 * `np.argmax(logits[mask].cpu().numpy(), axis=1)` (flat_amazon.py:111-114), so that `pred[mask]` (8
 * bytes per row) is what crosses PCIe instead of the masked logits. */
int tgcn_masked_ce_pred(const float *logits, int64_t ld, int64_t n_rows, int n_classes,
                        const int64_t *target, const uint8_t *mask, float inv_count, float *loss,
                        float *dlogits, int64_t ldd, int64_t *pred, void *workspace,
                        size_t workspace_bytes, tgcn_stream stream);

/* tgcn_masked_ce_grad -- tgcn_masked_ce_pred that also returns dbias[c] = sum_r dlogits[r, c]: the gradient of
 * the bias of the layer that produced the logits (the autograd of `out += bias` in the last GCNConv, triggered
 * at flat_amazon.py:105), summed from the registers that hold each gradient row instead of by a second pass
 * over dlogits (tgcn_colsum).  Fixed summation order, no atomics.  dlogits and dbias [n_classes] are required;
 * pred may be NULL. */
size_t tgcn_masked_ce_grad_workspace_bytes(int64_t n_rows, int n_classes);
int tgcn_masked_ce_grad(const float *logits, int64_t ld, int64_t n_rows, int n_classes,
                        const int64_t *target, const uint8_t *mask, float inv_count, float *loss,
                        float *dlogits, int64_t ldd, float *dbias, int64_t *pred, void *workspace,
                        size_t workspace_bytes, tgcn_stream stream);
/* tgcn_scale_by_device_scalar -- x[0..n) *= *scale_dev, skipped on the device when the scalar is exactly 1
 * (multiplying by 1.0f is the identity): the chain rule through the loss node, whose incoming gradient is a
 * device scalar the host cannot read without a synchronisation (`loss.backward()` seeds it with 1). */
int tgcn_scale_by_device_scalar(float *x, int64_t n, const float *scale_dev, tgcn_stream stream);

/* tgcn_grouped_ce -- the losses of the per-label strategy (perlabel_amazon.py:90-155: one classifier per top-level label,
 * each trained on its label's documents with their classes relabelled to 0..C_k-1) for ALL K classifiers in one pass over
 * their concatenated logits [n_rows, n_cols] (fp32, stride ld).  Group k owns the column segment [seg_start[k],
 * seg_start[k] + seg_width[k]): increasing, non-overlapping, width >= 1, gaps (pad columns) allowed, any alignment.
 *   group  int32 [n_rows]   the segment a row is TRAINED on, -1 = none (word nodes)
 *   target int64 [n_rows]   the LOCAL class in [0, seg_width[group]); read only where mask is set and group >= 0
 *   mask   uint8/bool       inv_count fp32 [K] (device) = 1 / selected rows of the group, 0 for a group with none
 *   route  int32 [n_rows] or NULL (= group): the segment the PREDICTION is taken in (eval_perlabel.py:73)
 *   class_map int64 [n_cols] or NULL: column -> global class id (the `mapping` of perlabel_amazon.py:107,159)
 * Results (loss_k, dlogits, dbias and pred may be NULL; dbias needs dlogits):
 *   loss    device scalar = sum over the non-empty groups of loss_k;  loss_k [K] = the group's mean CE, NaN when empty
 *   dlogits [n_rows, n_cols] stride ldd: (softmax - one-hot) * inv_count[group] inside the row's segment, exactly 0.0f in
 *           every other column, on every unselected row and on every row of group -1
 *   dbias   [n_cols] = column sums of dlogits;  pred int64 [n_rows] = seg_start[route] + argmax inside the route's
 *           segment (first index on ties), through class_map when given, -1 where route is -1
 * The segments are given twice: seg_start / seg_width on the DEVICE for the kernel, and the same values on the HOST, from
 * which the call validates them (TGCN_E_INVALID before anything is enqueued: overlapping or decreasing segments, one past
 * n_cols, ld < n_cols, more than 128 groups) without reading device memory.  Deterministic (fixed-order reductions, no
 * atomics); only enqueues on `stream`.  Workspace: tgcn_grouped_ce_workspace_bytes. */
size_t tgcn_grouped_ce_workspace_bytes(int64_t n_rows, int n_cols, int n_groups);
int tgcn_grouped_ce(const float *logits, int64_t ld, int64_t n_rows, int n_cols, int n_groups,
                    const int32_t *seg_start_host, const int32_t *seg_width_host, const int32_t *seg_start,
                    const int32_t *seg_width, const int32_t *group, const int32_t *route, const int64_t *target,
                    const uint8_t *mask, const float *inv_count, const int64_t *class_map, float *loss, float *loss_k,
                    float *dlogits, int64_t ldd, float *dbias, int64_t *pred, void *workspace, size_t workspace_bytes,
                    tgcn_stream stream);

/* tgcn_member_ce -- masked CrossEntropyLoss('mean') of K EQUAL-WIDTH members in one pass: one cell of the reference's
 * hyper-parameter sweeps (old/h_o_train.py: len(lrs) x KFold(k) two-layer GCNs on one graph) concatenated along the class
 * axis.  Member k owns the columns [k * seg_stride, k * seg_stride + n_classes) of logits [n_rows, >= K * seg_stride] (fp32,
 * stride ld); n_classes <= seg_stride, the columns between are pad.  Unlike tgcn_grouped_ce, every row meets every segment:
 *   bits   uint64 [n_rows]  row r is selected for member k where bit k is set (bits at or above K are ignored)
 *   target int64 [n_rows]   the class in [0, n_classes), shared by the members; read only where bits[r] != 0
 *   inv_count fp32 [K] (device) = 1 / selected rows of the member, 0 for a member with none
 * Results (loss_k, dlogits, dbias and pred may be NULL; dbias needs dlogits):
 *   loss    device scalar = sum over the non-empty members, in index order, of loss_k
 *   loss_k  [K] = CrossEntropyLoss('mean')(logits[sel_k][:, seg_k], target[sel_k]), NaN for a member without a selected row
 *   dlogits stride ldd: (softmax - one-hot) * inv_count[k] inside segment k of a selected row, exactly 0.0f in every other
 *           segment, on every unselected row and in every pad column -- all written by the call (the buffer need not be
 *           cleared); nothing outside [0, K * seg_stride) of a row is written
 *   dbias   [K * seg_stride] = column sums of dlogits (exactly 0 in pad columns and in the segment of an empty member)
 *   pred    int32 [n_rows, K]: pred[r * K + k] = the LOCAL arg-max of segment k of EVERY row (first index on ties; 0 for a
 *           row of -inf).  Without pred, rows with bits == 0 (the word nodes) are not read.
 * The arithmetic is tgcn_masked_ce's (the target's term apart from the sum of the others).  The 16-byte leaf applies to any
 * n_classes when seg_stride, ld and ldd are multiples of 4 and the bases are 16-byte aligned.  Deterministic (fixed-order
 * reductions, no atomics); only enqueues on `stream`.  TGCN_E_INVALID before anything is enqueued for K outside 1..64,
 * n_classes < 1, seg_stride < n_classes, ld or ldd < K * seg_stride, dbias without dlogits; TGCN_E_WORKSPACE for a workspace
 * below tgcn_member_ce_workspace_bytes. */
size_t tgcn_member_ce_workspace_bytes(int64_t n_rows, int n_members, int n_classes);
int tgcn_member_ce(const float *logits, int64_t ld, int64_t n_rows, int n_members, int n_classes, int seg_stride,
                   const int64_t *target, const uint64_t *bits, const float *inv_count, float *loss, float *loss_k,
                   float *dlogits, int64_t ldd, float *dbias, int32_t *pred, void *workspace, size_t workspace_bytes,
                   tgcn_stream stream);

/* Device-side scores of the K-member networks: what the reference takes per member on the host with sklearn's
 * f1_score(average="macro") and accuracy_score (old/h_o_train.py:116-122).  Both need three numbers per class, not a C x C
 * confusion matrix: `counts` is int32 [K, 3, C], planes in the order tp, n_pred, n_true.
 *
 * tgcn_class_counts_members -- the members of a sweep cell (tgcn_member_ce's selection and prediction):
 *   pred   int32 [n_rows, K] stride ldp >= K   the member's local arg-max on every row
 *   target int64 [n_rows]   shared by the members; read only where bits_a | bits_b has a bit below K set
 *   bits_a uint64 [n_rows]  row r counts for member k of set a where bit k is set (bits at or above K are ignored);
 *   bits_b the same for set b, or NULL (then counts_b is NULL too).  The two sets -- training and validation rows -- are
 *          taken in one pass over pred.
 * tgcn_class_counts_groups -- the per-label form (tgcn_grouped_ce's prediction):
 *   pred   int64 [n_rows];  pred_offset int32 [K] (device) or NULL (= 0): the row's class is pred[r] - pred_offset[group[r]]
 *   group  int32 [n_rows] or NULL: the member of row r, -1 = none; NULL = every row belongs to member 0 (the flat network)
 *   target int64 [n_rows]   the LOCAL class; read only where a mask selects the row and it has a member
 *   mask_a uint8/bool [n_rows], mask_b the same or NULL (then counts_b is NULL too)
 *   C is the widest member; the planes of a narrower member are zero beyond its own width.
 * Both: counts_a / counts_b [K, 3, C] are written whole by the call (nothing to clear).  A selected row whose prediction
 * lies outside [0, C) counts in n_true and nothing else (a miss: the -1 of a route of -1).  A selected row whose target lies
 * outside [0, C) is the caller's error (pytextgcn_amd.metrics raises for it before the launch): the kernel compares the
 * target with the bounds before it uses it and counts such a row nowhere.  A group outside [-1, K) counts nowhere either.
 * Each workgroup owns tiles of TGCN_CLASS_COUNTS_ROWS_PER_WORKGROUP rows (at most TGCN_CLASS_COUNTS_WORKGROUP_CAP workgroups
 * walk the tiles), accumulates with LDS integer adds in a table of at most TGCN_CLASS_COUNTS_LDS_BYTES -- members, and for
 * wide members the two sets, are tiled over the grid when K * 3 * C * 4 bytes (twice that with set b) exceed it -- and
 * stores its partial table to the workspace (together at most TGCN_CLASS_COUNTS_PARTIAL_BYTES, or one workgroup's); a
 * second kernel sums the partials in workgroup order.  No global atomics, no handshake between workgroups; only enqueues on
 * `stream` (legal under HIP-graph capture).  TGCN_E_INVALID before anything is enqueued for K outside 1..64, C outside
 * 1..TGCN_CLASS_COUNTS_MAX_CLASSES, n_rows outside 0..2^31-1, ldp < K, a NULL pred / target / bits_a / mask_a (n_rows > 0)
 * or counts_a, or one of set b's two pointers without the other; TGCN_E_WORKSPACE for a workspace below
 * tgcn_class_counts_workspace_bytes (0 for invalid sizes).
 *
 * tgcn_class_scores -- scores double [K, 4] from counts [K, 3, C], per member:
 *   [0] accuracy = sum tp / sum n_true (NaN for a member without a row)
 *   [1] f1_macro = the mean of 2 tp / (n_pred + n_true) over the classes with n_pred + n_true > 0 -- the union of the
 *       labels that occur in either array, sklearn's f1_score(average="macro") -- NaN when there is none
 *   [2] n_rows = sum n_true    [3] n_labels = classes in that mean */
#define TGCN_CLASS_COUNTS_ROWS_PER_WORKGROUP 256
#define TGCN_CLASS_COUNTS_WORKGROUP_CAP 1024
#define TGCN_CLASS_COUNTS_LDS_BYTES 49152
#define TGCN_CLASS_COUNTS_PARTIAL_BYTES 67108864
#define TGCN_CLASS_COUNTS_MAX_CLASSES 4096
size_t tgcn_class_counts_workspace_bytes(int64_t n_rows, int n_members, int n_classes);
int tgcn_class_counts_members(const int32_t *pred, int64_t ldp, const int64_t *target, const uint64_t *bits_a,
                              const uint64_t *bits_b, int64_t n_rows, int n_members, int n_classes, int32_t *counts_a,
                              int32_t *counts_b, void *workspace, size_t workspace_bytes, tgcn_stream stream);
int tgcn_class_counts_groups(const int64_t *pred, const int32_t *pred_offset, const int64_t *target, const int32_t *group,
                             const uint8_t *mask_a, const uint8_t *mask_b, int64_t n_rows, int n_members, int n_classes,
                             int32_t *counts_a, int32_t *counts_b, void *workspace, size_t workspace_bytes,
                             tgcn_stream stream);
int tgcn_class_scores(const int32_t *counts, int n_members, int n_classes, double *scores, tgcn_stream stream);

/* tgcn_adam_step -- one `torch.optim.Adam(..., amsgrad=...)` update of a flat fp32 tensor
 * (flat_amazon.py:89,106), torch's single-tensor formula op for op, fused into one pass.
 * max_exp_avg_sq = NULL means amsgrad=False.  `step` is the 1-based step count AFTER increment. */
int tgcn_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                   float *max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int64_t step, tgcn_stream stream);

/* tgcn_adam_members -- tgcn_adam_step on a contiguous [n_rows, n_cols] tensor (a bias: n_rows = 1) whose n_cols = n_members
 * * member_width columns are K column blocks with a learning rate each: column c takes lr_host[c / member_width] (K doubles
 * on the HOST); everything else is tgcn_adam_step op for op, so block k after the call is bit for bit what tgcn_adam_step
 * with lr_host[k] gives on a contiguous copy of it.  16-byte bodies where member_width and n_cols are multiples of 4, 4-byte
 * accesses otherwise.  The capturable form advances *step_dev once and leaves lr[k] / (1 - beta1^t) in scalars_dev[k] and
 * 1 / sqrt(1 - beta2^t) in scalars_dev[K] (K + 1 floats on the device).  n_rows * n_cols == 0 is a no-op (the capturable form
 * still advances the step).  TGCN_E_INVALID before anything is enqueued for n_cols != K * member_width, K outside 1..64, a
 * NULL lr_host, a negative size or buffers that are not 16-byte aligned. */
int tgcn_adam_members(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                      int64_t n_rows, int64_t n_cols, int member_width, int n_members, const double *lr_host, double beta1,
                      double beta2, double eps, double weight_decay, int64_t step, tgcn_stream stream);
int tgcn_adam_members_capturable(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                                 int64_t n_rows, int64_t n_cols, int member_width, int n_members, const double *lr_host,
                                 double beta1, double beta2, double eps, double weight_decay, int64_t *step_dev,
                                 float *scalars_dev, tgcn_stream stream);

/* tgcn_adam_member_rows -- tgcn_adam_step on a flat tensor of n = n_members * block elements whose members are ROW blocks
 * (the stacked [M D, in] embedding weight of a CrossValEGCN): element i takes lr_host[i / block].  n and block are 64-bit
 * and so is every index: such a tensor passes 2^31 elements.  16-byte bodies where block is a multiple of 4, 4-byte
 * accesses otherwise.  Block k after the call is bit for bit what tgcn_adam_step with lr_host[k] gives on that contiguous
 * range.  The capturable form is tgcn_adam_members_capturable's (K + 1 scalars on the device).  n == 0 is a no-op (the
 * capturable form still advances the step).  TGCN_E_INVALID before anything is enqueued for n != K * block, K outside
 * 1..64, a NULL lr_host, a negative size or buffers that are not 16-byte aligned.  Additive to ABI 7. */
int tgcn_adam_member_rows(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                          int64_t n, int64_t block, int n_members, const double *lr_host, double beta1, double beta2,
                          double eps, double weight_decay, int64_t step, tgcn_stream stream);
int tgcn_adam_member_rows_capturable(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                     float *max_exp_avg_sq, int64_t n, int64_t block, int n_members, const double *lr_host,
                                     double beta1, double beta2, double eps, double weight_decay, int64_t *step_dev,
                                     float *scalars_dev, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Tall-skinny fp32 GEMMs on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32): the dense
 * `torch.matmul(x, self.weight)` of PyG-1.6.3 GCNConv.forward (reference call site models.py:20,
 * layers built at models.py:13,15) and its autograd.  N = number of nodes; k, n = layer widths, any value >= 1.
 * The small operand lives in LDS: one launch when k_pad * n_pad * 4 bytes <= 160 KB (k_pad = k rounded up to 8,
 * n_pad = n rounded up to 32; e.g. 200 x 64, 64 x 200), otherwise the product runs as column groups of <= 128 result
 * columns and k chunks of <= 256 that accumulate into C (e.g. DBpedia's 219 classes at hidden width 200, flat_dbpedia.py:80:
 * two groups) -- the tall operand is then read once per group.
 *   tgcn_gemm_nn   C[N,n] = A[N,k] @ B[k,n]        (XW  = H @ W)        A: lda % 4 == 0, 16-B aligned
 *   tgcn_gemm_nt   C[N,n] = A[N,k] @ B[n,k]^T      (dH  = dXW @ W^T)    A: lda % 4 == 0, 16-B aligned
 *   tgcn_gemm_tn   C[k,n] = A[N,k]^T @ G[N,n]      (dW  = H^T @ dXW)    deterministic; one launch covers <= 256 columns
 *                                                                        of A x <= 128 of G, wider ones run in chunks
 */
int tgcn_gemm_nn(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                 int64_t N, int k, int n, tgcn_stream stream);
int tgcn_gemm_nt(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                 int64_t N, int k, int n, tgcn_stream stream);
size_t tgcn_gemm_tn_workspace_bytes(int64_t N, int k, int n);
int tgcn_gemm_tn(const float *A, int64_t lda, const float *G, int64_t ldg, float *C, int64_t ldc,
                 int64_t N, int k, int n, void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* The same products with the inverted dropout of the reference's GCN.forward (textgcn/lib/models.py:23,
 * `x = self.dropout(x)` between the layers) fused in, so that the dropped activation and its mask are
 * never stored: element (r, c) of the masked [N x w] activation is kept iff hash(seed, r, c) >=
 * p * 2^32 and scaled by 1 / (1 - p); all three regenerate the same mask from `seed` (8 bytes in DEVICE
 * memory, read by the kernels: safe under HIP-graph capture).
 *   tgcn_gemm_nn_dropout   C = dropout(A) @ B          mask over A [N x k]   (XW = dropout(H) @ W)
 *   tgcn_gemm_tn_dropout   C = dropout(A)^T @ G        mask over A [N x k]   (dW = dropout(H)^T @ dXW)
 *   tgcn_gemm_nt_dropout   C = dropout'(A @ B^T)       mask over C [N x n]   (dH = mask * (dXW @ W^T))
 * 0 <= p <= 1 (p = 1 yields zeros).  The random stream is this library's own, not torch's. */
int tgcn_gemm_nn_dropout(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                         int64_t N, int k, int n, double p, const uint64_t *seed, tgcn_stream stream);
int tgcn_gemm_nt_dropout(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                         int64_t N, int k, int n, double p, const uint64_t *seed, tgcn_stream stream);
int tgcn_gemm_tn_dropout(const float *A, int64_t lda, const float *G, int64_t ldg, float *C, int64_t ldc,
                         int64_t N, int k, int n, double p, const uint64_t *seed, void *workspace,
                         size_t workspace_bytes, tgcn_stream stream);

/* The same two products with the keep decisions RECORDED instead of hashed twice: the nn product (forward) writes the mask
 * of its A operand, 4 bits per lane step, `tgcn_dropout_mask_words(k, n)` 32-bit words per row (the caller allocates
 * [N x mask_stride] words; 0 = a product of this shape cannot record it -- reductions longer than 256, the split-bf16 mode -- use the
 * entry points above); the tn product (weight gradient) reads it back: one load and four bit tests per 16 bytes of A in
 * place of four hashes.  Bit for bit the results of tgcn_gemm_nn_dropout / tgcn_gemm_tn_dropout with the same seed (the
 * tn side falls back on the hash wherever its kernel does not take the record).  Layout: column c of a row is bit 4 ((c / 8) % 8) + (c & 3) of word
 * ((c / 4) & 1) * (words / 2) + c / 64. */
size_t tgcn_dropout_mask_words(int k, int n);
int tgcn_gemm_nn_dropout_mask(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                              int64_t N, int k, int n, double p, const uint64_t *seed, uint32_t *mask,
                              int64_t mask_stride, tgcn_stream stream);
int tgcn_gemm_tn_dropout_mask(const float *A, int64_t lda, const float *G, int64_t ldg, float *C, int64_t ldc,
                              int64_t N, int k, int n, double p, const uint64_t *seed, const uint32_t *mask,
                              int64_t mask_stride, void *workspace, size_t workspace_bytes, tgcn_stream stream);
/* ... and the input-gradient product with the column sums, its mask (over the [N x n] RESULT: the same matrix the forward
 * product masked) read from that record instead of hashed: bit for bit tgcn_gemm_nt_colsum with the same seed (the kernel
 * falls back on the hash for shapes whose record it does not take). */
int tgcn_gemm_nt_colsum_mask(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                             int64_t N, int k, int n, double p, const uint64_t *seed, const uint32_t *mask,
                             int64_t mask_stride, float *colsum, void *workspace, size_t workspace_bytes,
                             tgcn_stream stream);
/* tgcn_set_dropout_row_keys -- which ROW of the dropout mask a row of the masked matrix is, for every tgcn_gemm_*_dropout*
 * / tgcn_gemm_nt_colsum* call this THREAD makes from now on: row i of the call's [N x ld] matrix takes the keep decisions
 * of mask row i + key0 when i < split, of mask row i + key1 otherwise (the mask is a stateless hash of (seed, mask row,
 * column)).  (0, 0, 0) -- the state of a new thread -- is the row index itself.  No reference counterpart (F.dropout at
 * textgcn/lib/models.py:23 draws an unkeyed mask over the whole activation); it exists for the 1-D partition: a hub
 * (word) row's mask must be the same function of its position in the gathered hub block on the rank that owns the row
 * (its local rows [0, hp) are mask rows rank * hp + i) and on every rank that holds a partial sum of it, so that
 * dropout(sum_q P_q) @ W2 = sum_q dropout(P_q) @ W2 can be exchanged at the class width (pytextgcn_amd/sharded.py,
 * `narrow_exchange`).  The recorded-mask entry points record / read decisions per matrix row, whatever the keys. */
int tgcn_set_dropout_row_keys(int64_t split, int64_t key0, int64_t key1);

/* tgcn_set_gemm_split -- library-wide numerical mode of tgcn_gemm_nn / _nt / _tn for the
 * shapes of the GCN layers (nn: k = 200, 33 <= n <= 64; nt: k = 64, 193 <= n <= 224; tn: k = 200, 33 <= n <= 64,
 * contiguous operands; + the _dropout forms and, for nt, the _colsum form).  Every other shape keeps the fp32 kernels.  on != 0: every fp32 product is
 * formed from an exact three-way bf16 split of both operands on the bf16 matrix cores (six partial products,
 * fp32 accumulation, dropped terms <= 2^-23 relative): fp32-accurate, NOT the fp32 FMA chain bit for bit, +-inf
 * operands give nan.  Default off (TGCN_GEMM_SPLIT=1 in the environment turns it on at load).  Returns the
 * previous setting. */
int tgcn_set_gemm_split(int on);

/* tgcn_gemm_nt_colsum -- tgcn_gemm_nt (seed == NULL) or tgcn_gemm_nt_dropout (seed != NULL) that also returns
 * colsum[j] = sum_r C[r, j], summed from the accumulator tiles as they are stored: with C = dH1 (the gradient of
 * the first layer's output) this is that layer's bias gradient (the autograd of `out += bias`, triggered at
 * flat_amazon.py:105), which otherwise costs a second pass over the N x h matrix (tgcn_colsum).  Fixed summation
 * order, no atomics. */
size_t tgcn_gemm_nt_colsum_workspace_bytes(int n);
int tgcn_gemm_nt_colsum(const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                        int64_t N, int k, int n, double p, const uint64_t *seed, float *colsum, void *workspace,
                        size_t workspace_bytes, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * The front end of the reference's EGCN (textgcn/lib/models.py:28-52: `Linear(in_channels, embedding_dim)`, SELU, dropout,
 * then the first GCNConv's x @ W) for TextGCN's one-hot features, as ONE product.  With x = I the Linear's output is
 * E^T + b for its weight E [K, N] (K = embedding_dim, row-major as nn.Linear keeps it, leading dimension lde >= N; no
 * alignment or padding is asked of it), so with
 *       a(i, k) = s * keep(i, k) * selu(E[k, i] + b[k]),      s = 1 / (1 - p),
 * keep(i, k) the decision of tgcn_gemm_*_dropout for mask row mask_row0 + i and column k (same hash, same threshold
 * clamp, same one-element int64 device seed), and selu with torch's constants:
 *   tgcn_embed_xw        C[i, 0:n]  = sum_k a(i, k) W[k, 0:n]                           C [N, n] stride ldc, W [K, n] stride ldw
 *   tgcn_embed_xw_grad   dE[k, i]   = s keep(i, k) selu'(E[k, i] + b[k]) sum_j G[i, j] W[k, j]    (E's layout, stride ldde)
 *                        db[k]      = sum_i dE[k, i]
 *                        dW[k, j]   = sum_i a(i, k) G[i, j]                             G = dC [N, n] stride ldg
 * The N x K activation is never stored: a is formed in registers on its way into the fp32 matrix cores, and recomputed
 * (same mask) for dW.  p = 0 or seed = NULL: no mask, s = 1.  0 <= p < 1.  N >= 0, K >= 1, n >= 1; all offsets are 64-bit.
 * Unlike tgcn_gemm_*_dropout these calls take the mask row offset as an argument and read no thread-local state.
 * tgcn_embed_xw_grad: dE and db are computed together (both or neither), dW on its own; the workspace is needed for dW only
 * and holds partial sums of dW, nothing of size N x K.  Fixed summation orders, no atomics: reproducible run to run. */
int tgcn_embed_xw(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, float *C, int64_t ldc,
                  int64_t N, int K, int n, double p, const uint64_t *seed, int64_t mask_row0, tgcn_stream stream);
size_t tgcn_embed_xw_grad_workspace_bytes(int64_t N, int K, int n);
int tgcn_embed_xw_grad(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, const float *G,
                       int64_t ldg, float *dE, int64_t ldde, float *db, float *dW, int64_t lddw, int64_t N, int K, int n,
                       double p, const uint64_t *seed, int64_t mask_row0, void *workspace, size_t workspace_bytes,
                       tgcn_stream stream);

/* The same front end on [I_N | H] features (text2graph.py:226-246: the hierarchy features of the per-level scripts).  The
 * Linear's weight is then ONE parameter [K, N + Fh]: E points at its first N columns and Eh at its last Fh, so lde ==
 * ldeh == N + Fh in practice (any leading dimensions >= N and >= Fh are taken; no alignment is asked).  Hd [N - h_row0,
 * Fh] (row stride ldh >= Fh) holds the DENSE rows of H for the nodes i >= h_row0; the nodes below (the word rows) have
 * no H term, and h_row0 == N means that nobody has one (Hd may then be NULL).  1 <= Fh <= tgcn_embed_xw_h_max_features()
 * (128).  With
 *       z(i, k) = (E[k, i] + b[k]) + t(i, k),   t(i, k) = sum over f ascending of H[i, f] Eh[k, f]   (i >= h_row0; else no t)
 *       a(i, k) = s * keep(i, k) * selu(z(i, k))             (keep, s, selu: as above)
 *   tgcn_embed_xw_h        C[i, 0:n]  = sum_k a(i, k) W[k, 0:n]
 *   tgcn_embed_xw_h_grad   dE[k, i]   = s keep(i, k) selu'(z(i, k)) sum_j G[i, j] W[k, j]       (E's layout, stride ldde)
 *                          db[k]      = sum_i dE[k, i]
 *                          dEh[k, f]  = sum_{i >= h_row0} dE[k, i] H[i, f]                      (Eh's layout, stride lddeh)
 *                          dW[k, j]   = sum_i a(i, k) G[i, j]
 * H gets no gradient.  dE, db and dEh are computed together (all three or none), dW on its own.  t runs on the matrix
 * cores too, in the registers of the product that consumes it; a wave whose 32 nodes all lie below h_row0 skips it and
 * computes what tgcn_embed_xw* compute, bit for bit.  The workspace (tgcn_embed_xw_h_grad_workspace_bytes) holds the
 * partial sums of dW and, after them, those of dEh over a fixed number of slices of the nodes, added in slice order: no
 * atomics, nothing of size N x K, the same bits every run.  The calls only enqueue on `stream`.  NULL operands, Fh outside
 * [1, cap], h_row0 outside [0, N], a leading dimension below the width, p outside [0, 1), mask_row0 < 0 and a short
 * workspace are TGCN_E_INVALID before anything is enqueued; N == 0 launches no kernel; n > 256 runs as column groups. */
int tgcn_embed_xw_h_max_features(void);
int tgcn_embed_xw_h(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd, int64_t ldh,
                    int64_t h_row0, int Fh, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N, int K, int n,
                    double p, const uint64_t *seed, int64_t mask_row0, tgcn_stream stream);
size_t tgcn_embed_xw_h_grad_workspace_bytes(int64_t N, int K, int n, int Fh);
int tgcn_embed_xw_h_grad(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd,
                         int64_t ldh, int64_t h_row0, int Fh, const float *W, int64_t ldw, const float *G, int64_t ldg,
                         float *dE, int64_t ldde, float *db, float *dEh, int64_t lddeh, float *dW, int64_t lddw, int64_t N,
                         int K, int n, double p, const uint64_t *seed, int64_t mask_row0, void *workspace,
                         size_t workspace_bytes, tgcn_stream stream);

/* The same front end for M = n_members (1..64) networks of equal widths in one call: the EGCN members of a sweep cell
 * (pytextgcn_amd/crossval.py: CrossValEGCN).  Additive to ABI 7.  E, b, Eh and W are stacked by ROWS -- member m owns the
 * rows [m K, (m + 1) K) of E [M K, N], b [M K], Eh [M K, Fh] and W [M K, n] -- and so are dE, db, dEh and dW; C and G are
 * [N, M n] (ldc, ldg >= M n) and member m owns their columns [m n, (m + 1) n).  Hd, h_row0 and Fh are the members' common
 * ones; Fh == 0 (Eh and Hd are then not looked at) means identity features.  p_host: M rates on the HOST, each in
 * [0, 1); seeds: M seeds on the DEVICE, NULL for the eval product.  keep_m(i, k) is the decision of tgcn_gemm_*_dropout
 * for seeds[m], mask row mask_row0 + i and column k < K inside the member, at p_host[m]; a member at rate 0 keeps
 * everything at scale 1.  Member m's blocks of every result are BIT FOR BIT what tgcn_embed_xw[_h][_grad] gives with
 * seeds + m, p_host[m] and the member's slices: the same kernels run with the member as one more grid dimension, so the
 * number of launches does not depend on M.  The nodes are cut into slices as the single call cuts them for (N, K); the
 * workspace is M times the single call's.  No atomics, fixed summation orders; the calls only enqueue on `stream` (N == 0:
 * memsets of the sums).  TGCN_E_INVALID before anything is enqueued for M outside 1..64, a rate outside [0, 1), a leading
 * dimension below the width, NULL operands with N > 0, dE without db (or, with Fh > 0, dEh), Fh outside [0, 128] and
 * h_row0 outside [0, N]; TGCN_E_WORKSPACE for a short workspace. */
int tgcn_embed_xw_members(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd,
                          int64_t ldh, int64_t h_row0, int Fh, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N,
                          int K, int n, int n_members, const double *p_host, const uint64_t *seeds, int64_t mask_row0,
                          tgcn_stream stream);
size_t tgcn_embed_xw_members_grad_workspace_bytes(int64_t N, int K, int n, int Fh, int n_members);
int tgcn_embed_xw_members_grad(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd,
                               int64_t ldh, int64_t h_row0, int Fh, const float *W, int64_t ldw, const float *G, int64_t ldg,
                               float *dE, int64_t ldde, float *db, float *dEh, int64_t lddeh, float *dW, int64_t lddw,
                               int64_t N, int K, int n, int n_members, const double *p_host, const uint64_t *seeds,
                               int64_t mask_row0, void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * The first GCNConv's x @ W on [I_N | H] features for the plain GCN of the per-level scripts (perlevel_amazon.py:122,156;
 * both set `model = GCN`).  Additive to ABI 7.  W [N + Fh, F] (row stride ldw >= F) is the layer's whole weight and
 * Wh = W + N * ldw its last Fh rows, so X @ W = W[0:N] + H @ Wh.  The nodes below h_row0 (the word rows) have no
 * hierarchy term; h_row0 == N means that nobody has one.  1 <= Fh <= tgcn_hier_max_features() (128), F >= 1.
 *   tgcn_hier_xw        C[i, 0:F] = W[i, 0:F] + t(i, :),  i in [0, N)                    C [N, F] stride ldc
 *     TGCN_HIER_ONEHOT  cls int32 [N - h_row0]: t(i, :) = Wh[cls[i - h_row0], :] (formed as Wh + 0).  A class id outside
 *                       [0, Fh) contributes nothing: it is skipped on the device, never read through (the rule of
 *                       tgcn_rows_gather).  Hd is not read.
 *     TGCN_HIER_DENSE   Hd [N - h_row0, Fh] stride ldh >= Fh: t(i, c) = fmaf(Hd[i, f], Wh[f, c], t) over f ascending from
 *                       t = 0, then C = W + t: a one-hot Hd gives the ONEHOT form's bits exactly (finite weights).  cls
 *                       is not read.  The rows below h_row0 are a copy of W's rows.
 *   tgcn_hier_xw_grad   for G = dC [N, F] stride ldg and dW [N + Fh, F] stride lddw:  dW[0:N] = G, and
 *     TGCN_HIER_ONEHOT  dW[N + f, :] = sum over the rows i >= h_row0 with cls = f of G[i, :]; a class without a row gets
 *                       exact zeros.  The document rows are cut into a fixed number of slices whose partial sums
 *                       [slices, Fh, F] -- nothing of size N x F -- go to the workspace
 *                       (tgcn_hier_xw_grad_workspace_bytes) and are added in slice order: no atomics, the same bits
 *                       every run.
 *     TGCN_HIER_DENSE   dW[N:] is NOT written: it is Hd^T @ G[h_row0:], the caller's tgcn_gemm_tn.  No workspace.
 * H gets no gradient.  Streaming kernels in float4 lanes where F, the strides and the pointers allow, in dword lanes with
 * the same results otherwise.  The calls only enqueue on `stream`; all offsets are 64-bit.  NULL operands, Fh outside
 * [1, cap], h_row0 outside [0, N], a leading dimension below the width, a short workspace and an unknown form are
 * TGCN_E_INVALID before anything is enqueued; N == 0 launches no kernel. */
enum { TGCN_HIER_ONEHOT = 0, TGCN_HIER_DENSE = 1 };
int tgcn_hier_max_features(void);
int tgcn_hier_xw(const float *W, int64_t ldw, int form, const int32_t *cls, const float *Hd, int64_t ldh, int64_t h_row0,
                 int Fh, float *C, int64_t ldc, int64_t N, int F, tgcn_stream stream);
size_t tgcn_hier_xw_grad_workspace_bytes(int64_t N, int F, int Fh, int64_t h_row0, int form);
int tgcn_hier_xw_grad(const float *G, int64_t ldg, int form, const int32_t *cls, int64_t h_row0, int Fh, float *dW,
                      int64_t lddw, int64_t N, int F, void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * The middle of the reference's MLP (textgcn/lib/models.py:83-102: `x = dropout(selu(Linear(x)))` feeding the next
 * Linear), as ONE product per layer.  Z [N, k] (row-major, leading dimension ldz >= k) is a layer's stored
 * pre-activation WITHOUT its bias b [k]; W [n, k] (leading dimension ldw >= k) is the next nn.Linear's weight in torch's
 * own [out, in] layout and c [n] its bias (NULL: none).  With
 *       a(i, j) = s * keep(i, j) * selu(Z[i, j] + b[j]),      s = 1 / (1 - p),
 * keep(i, j) the decision of tgcn_gemm_*_dropout for mask row mask_row0 + i and column j (same hash, same threshold
 * clamp, same one-element int64 device seed), and selu with torch's constants:
 *   tgcn_mlp_act_linear        C[i, 0:n]  = sum_j a(i, j) W[0:n, j] (+ c[0:n])               C [N, n] stride ldc
 *   tgcn_mlp_act_linear_grad   dZ[i, j]   = s keep(i, j) selu'(Z[i, j] + b[j]) sum_m G[i, m] W[m, j]    (Z's layout, stride lddz)
 *                              db[j]      = sum_i dZ[i, j]
 *                              dW[m, j]   = sum_i G[i, m] a(i, j)      (W's layout, stride lddw)   G = dC [N, n] stride ldg
 * The N x k activation is never stored: a is formed in registers on its way into the fp32 matrix cores, and recomputed
 * (same mask) for dW.  p = 0 or seed = NULL: no mask, s = 1.  0 <= p < 1.  N >= 0, k >= 1, n >= 1 (wider operands run as
 * column groups of 256 and chunks of k inside the call); all offsets are 64-bit.  Z, G, C, dZ, W and dW are taken with ANY
 * leading dimension >= their width and any 4-byte alignment: every load and store of these kernels is a dword, so there is
 * no vector path with % 4 or 16-byte conditions and hence one result whatever the strides are (db's column sums take
 * tgcn_colsum's float4 loads where dZ allows them).  The mask row offset is an argument; no thread-local state is read.
 * tgcn_mlp_act_linear_grad: dZ and db are computed together (both or neither), dW on its own.  The workspace
 * (tgcn_mlp_act_linear_grad_workspace_bytes; needed whenever N > 0) holds partial sums of db and dW, nothing of size N x k.
 * Fixed summation orders, no atomics: reproducible run to run.  The calls only enqueue on `stream`.  NULL operands, p
 * outside [0, 1), mask_row0 < 0, a leading dimension below the width and a short workspace are TGCN_E_INVALID before
 * anything is enqueued. */
int tgcn_mlp_act_linear(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *c, float *C,
                        int64_t ldc, int64_t N, int k, int n, double p, const uint64_t *seed, int64_t mask_row0,
                        tgcn_stream stream);
size_t tgcn_mlp_act_linear_grad_workspace_bytes(int64_t N, int k, int n);
int tgcn_mlp_act_linear_grad(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *G,
                             int64_t ldg, float *dZ, int64_t lddz, float *db, float *dW, int64_t lddw, int64_t N, int k,
                             int n, double p, const uint64_t *seed, int64_t mask_row0, void *workspace,
                             size_t workspace_bytes, tgcn_stream stream);

/* The same products with a bias that depends on the ROW: the first hidden layer of the per-level MLP (MLP_level.py trains
 * every level after the first on append_feats(X, H), H the one-hot columns of the levels above).  Additive to ABI 7.
 * [X | H] @ W1.t() = X @ W1[:, :F].t() + Wh[class], so the class features are S <= 2 rows of a small table: cls int32
 * [N, S] (row-major, leading dimension ldcls >= S, S in {1, 2}) holds row indices into T [Fh, k] (leading dimension
 * ldt >= k, 1 <= Fh <= tgcn_hier_max_features() = 128), and the pre-activation of element (i, j) is
 *       z(i, j) = ((Z[i, j] + T[cls[i, 0], j]) + T[cls[i, 1], j]) + b[j]          (S == 1: no second term)
 * in exactly this order, in all three products: a(i, j) = s keep(i, j) selu(z(i, j)) in C and dW, selu'(z(i, j)) in dZ.
 * An id outside [0, Fh) selects nothing: it is skipped on the device, never read through (the rule of tgcn_hier_xw and
 * tgcn_rows_gather).  T is read through the caches; nothing of size N x k is formed or stored.  The backward also returns
 *       dT[f, j] = the sum of dZ[i, j] over the rows i and slots s with cls[i, s] == f              (T's layout, stride lddt)
 * (NULL: not wanted; it needs dZ), a grouped column sum of the finished dZ like db: the rows are cut into a fixed number of
 * slices whose partial sums [slices, Fh, k] go to the workspace (tgcn_mlp_act_linear_cls_grad_workspace_bytes) and are
 * added in slice order: no atomics, the same bits every run, exact zeros for a row of T that no id selects.  N == 0 gives
 * zero db, dW and dT.  Everything else is tgcn_mlp_act_linear*'s: with T == 0 or no valid id the results are its bits.
 * S outside {1, 2}, Fh outside [1, 128], ldcls < S, ldt < k, lddt < k, a NULL cls or T with N > 0 and dT without dZ are
 * TGCN_E_INVALID before anything is enqueued, like the conditions above. */
int tgcn_mlp_act_linear_cls(const float *Z, int64_t ldz, const int32_t *cls, int64_t ldcls, int S, const float *T,
                            int64_t ldt, int Fh, const float *b, const float *W, int64_t ldw, const float *c, float *C,
                            int64_t ldc, int64_t N, int k, int n, double p, const uint64_t *seed, int64_t mask_row0,
                            tgcn_stream stream);
size_t tgcn_mlp_act_linear_cls_grad_workspace_bytes(int64_t N, int k, int n, int Fh);
int tgcn_mlp_act_linear_cls_grad(const float *Z, int64_t ldz, const int32_t *cls, int64_t ldcls, int S, const float *T,
                                 int64_t ldt, int Fh, const float *b, const float *W, int64_t ldw, const float *G,
                                 int64_t ldg, float *dZ, int64_t lddz, float *db, float *dT, int64_t lddt, float *dW,
                                 int64_t lddw, int64_t N, int k, int n, double p, const uint64_t *seed, int64_t mask_row0,
                                 void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * The same products with a weight that depends on the row's GROUP: the K per-label MLPs of the reference's MLP_label.py
 * as one network.  The N rows lie in grouped order: rows [row_ptr[g], row_ptr[g + 1]) belong to group g (0 <= g < K <= 128;
 * an empty group is legal), rows at or past row_ptr[K] to nobody: they are neither read nor written.  Group g reads rows
 * [w_row0[g], w_row0[g] + n[g]) of the stacked weight W [w_rows, k], entries [b_off[g], b_off[g] + k) of the stacked bias
 * b [b_len], and owns columns [col0[g], col0[g] + n[g]) of C and G [N, c_cols] (and of c [c_cols]).  For row i of group g,
 * with a(i, j) = s * keep(i, j) * selu(Z[i, j] + b[b_off[g] + j]) and keep the hash above for mask row mask_row0 + i:
 *   tgcn_mlp_grouped_act_linear        C[i, col0[g] + m] = sum_j a(i, j) W[w_row0[g] + m, j] (+ c[col0[g] + m])    m < n[g]
 *   tgcn_mlp_grouped_act_linear_grad   dZ[i, j] = s keep selu'(.) sum_m G[i, col0[g] + m] W[w_row0[g] + m, j]
 *                                      db[b_off[g] + j]      = the sum of dZ[i, j] over the rows of group g
 *                                      dW[w_row0[g] + m, j]  = the sum of G[i, col0[g] + m] a(i, j) over the rows of group g
 *                                      dc[col0[g] + m]       = the sum of G[i, col0[g] + m] over the rows of group g
 *                                                              (the gradient of c; dc [c_cols] or NULL; asks for column
 *                                                              ranges that do not overlap, as the class segments are)
 * Every other element of C, dZ, db, dW and dc keeps what it held; db, dW and dc of a group without rows are exact zeros.  Group
 * g's slices of C and dZ carry the bits of tgcn_mlp_act_linear / _grad on rows [row_ptr[g], row_ptr[g + 1]) with mask_row0
 * + row_ptr[g]: the same kernels (v_mfma_f32_32x32x2_f32), a workgroup serving one tile of at most 128 rows of one group.
 *
 * tgcn_mlp_grouped_layout (HOST only: no device is touched, nothing is enqueued) validates the description and fills
 * `out` (tgcn_mlp_grouped_layout_bytes(K, row_ptr) bytes, an upper bound that does not depend on k; 0 for an invalid K or
 * row_ptr) with the tables the kernels read: the groups, the row tiles and the slices of the dW reduction.  The caller
 * copies the blob to the device once and passes BOTH copies to the products (`layout_host` is read during the call for the
 * grid sizes and the checks, `layout_dev` by the kernels), so the products enqueue on `stream` only: no allocation, no
 * copy, no synchronisation, legal under HIP-graph capture.  The launch count depends on max n[g] and k (column groups of
 * 256, 128 and 256 as above), never on K.  Fixed summation orders, no atomics.  K outside [1, 128], a decreasing row_ptr,
 * row_ptr[K] > N, n[g] < 1, a range of W, C or b outside w_rows, c_cols or b_len, a short `out`, and in the products a
 * layout built for another N or k, a leading dimension below the width (ldc, ldg >= c_cols), NULL operands and a short
 * workspace are TGCN_E_INVALID before anything is enqueued.  dZ and db together or neither, dW on its own, as above. */
size_t tgcn_mlp_grouped_layout_bytes(int K, const int64_t *row_ptr);
int tgcn_mlp_grouped_layout(int K, const int64_t *row_ptr, const int32_t *w_row0, const int32_t *n, const int32_t *col0,
                            const int32_t *b_off, int64_t N, int k, int64_t w_rows, int64_t c_cols, int64_t b_len, void *out,
                            size_t out_bytes);
int tgcn_mlp_grouped_act_linear(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *c,
                                float *C, int64_t ldc, int64_t N, int k, const void *layout_host, const void *layout_dev,
                                double p, const uint64_t *seed, int64_t mask_row0, tgcn_stream stream);
size_t tgcn_mlp_grouped_act_linear_grad_workspace_bytes(const void *layout_host);
int tgcn_mlp_grouped_act_linear_grad(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *G,
                                     int64_t ldg, float *dZ, int64_t lddz, float *db, float *dW, int64_t lddw, float *dc,
                                     int64_t N, int k, const void *layout_host, const void *layout_dev, double p, const uint64_t *seed,
                                     int64_t mask_row0, void *workspace, size_t workspace_bytes, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * The layer-2 products of the grouped GCNs (PerLabelGCN, CrossValGCN) for all K members at once, with a dropout rate and a
 * seed PER MEMBER.  Additive to ABI 7.  X [N, K h] (row stride ldx >= K h) is the concatenated hidden activation: member k
 * owns columns [k h, (k + 1) h).  W [h, n_cols] (ldw >= n_cols) holds W_k in the column segment [col0[k], col0[k] + n[k]);
 * the segments increase and do not overlap, pad columns may lie between, before and behind them.  C and G are [N, n_cols]
 * (ldc, ldg >= n_cols).  Member k has a rate p[k] in [0, 1) (0: everything is kept at scale 1) and the 64-bit seed
 * seeds[k] (DEVICE array of K, read by the kernels; seeds == NULL: no member drops anything, the eval product).  With
 * s_k = 1 / (1 - p[k]), keep_k(i, j) the decision of tgcn_gemm_*_dropout's hash for seeds[k], mask row mask_row0 + i and
 * column j INSIDE the member's block at the threshold of p[k], and a(i, j) = s_k keep_k(i, j) X[i, k h + j]:
 *   tgcn_blockdiag_xw        C[i, col0[k] + m]  = sum_j a(i, j) W[j, col0[k] + m]                       m < n[k]
 *                            every column of C that belongs to no segment is written as 0.0f: no zero fill by the caller
 *   tgcn_blockdiag_xw_grad   dX[i, k h + j]     = s_k keep_k(i, j) sum_m G[i, col0[k] + m] W[j, col0[k] + m]
 *                            colsum[k h + j]    = the column sums of the dX that is stored (colsum [K h])
 *                            dW[j, col0[k] + m] = sum_i a(i, j) G[i, col0[k] + m]; pad columns of dW are 0.0f
 *   dX and colsum together or neither, dW on its own (NULL = not wanted).  These are the decisions and, in exact
 *   arithmetic, the values of K calls of tgcn_gemm_nn_dropout / _nt_ / _tn_ on the members' slices; the sums run in
 *   another order, so the bits differ.  The mask is regenerated from the seed in all three products.
 * The member table reaches the kernels as a BLOB, like tgcn_mlp_grouped_layout: tgcn_blockdiag_layout (HOST only: no device
 * is touched, nothing is enqueued) validates the description and fills `out` (tgcn_blockdiag_layout_bytes(K) bytes; 0 for K
 * outside [1, 128]); the caller copies the blob to the device once and passes BOTH copies (`layout_host` is read during the
 * call, `layout_dev` by the kernels).  The rates are part of the blob (p == NULL: all 0).  The products only enqueue on
 * `stream`: no allocation, no copy, no synchronisation, legal under HIP-graph capture.  v_mfma_f32_32x32x2_f32 (exact
 * fp32); fixed-order reductions through `workspace` (tgcn_blockdiag_xw_grad_workspace_bytes(layout_host, N) bytes), no
 * atomics, the same bits every run.  The launch count depends on max n[k] (column groups of 256 forward, 128 in dX and dW),
 * never on K; X and G are read once per product and column group.  Operands: float32, unit column stride, any row stride
 * at or above the width, 4-byte alignment (plain dword accesses: no padding or 16-byte rows are asked for).
 * TGCN_E_INVALID before anything is enqueued: in tgcn_blockdiag_layout K outside [1, 128], h outside [1,
 * tgcn_blockdiag_max_hidden()] (256: one workgroup of dW holds all h rows of a member's dW), n[k] < 1, a segment that
 * starts before the end of the one before it or ends past n_cols, p[k] outside [0, 1), a short `out`; in the products a
 * blob that is not a layout, N < 0 or N > 128 * (2^24 - 1) (the row tiles are one grid dimension), mask_row0 < 0, a leading dimension below the width, NULL operands with N > 0, dX
 * without colsum (or the reverse), nothing wanted.  A short workspace is TGCN_E_WORKSPACE.  N == 0 is legal: C gets no row,
 * dW and colsum are exact zeros. */
int tgcn_blockdiag_max_hidden(void);
size_t tgcn_blockdiag_layout_bytes(int K);
int tgcn_blockdiag_layout(int K, int h, int64_t n_cols, const int32_t *col0, const int32_t *n, const double *p, void *out,
                          size_t out_bytes);
int tgcn_blockdiag_xw(const float *X, int64_t ldx, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N,
                      const void *layout_host, const void *layout_dev, const uint64_t *seeds, int64_t mask_row0,
                      tgcn_stream stream);
size_t tgcn_blockdiag_xw_grad_workspace_bytes(const void *layout_host, int64_t N);
int tgcn_blockdiag_xw_grad(const float *X, int64_t ldx, const float *W, int64_t ldw, const float *G, int64_t ldg, float *dX,
                           int64_t lddx, float *colsum, float *dW, int64_t lddw, int64_t N, const void *layout_host,
                           const void *layout_dev, const uint64_t *seeds, int64_t mask_row0, void *workspace,
                           size_t workspace_bytes, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * JumpingKnowledge(mode="lstm") of the reference's JumpingKnowledgeNetwork (textgcn/lib/models.py:64,75; PyG 1.6.3): a
 * bidirectional LSTM of hidden width H over the L per-layer activations x_t [N, C] of every node, a Linear(2 H -> 1) on
 * [h_fwd_t | h_bwd_t], a softmax over the layers and the weighted sum
 *       alpha[i, :] = softmax_t(att_w . [h_fwd_t(i) | h_bwd_t(i)] + att_b),      out[i, :] = sum_t alpha[i, t] x_t[i, :].
 * The L inputs are L separate matrices: `xs` and `ldxs` are HOST arrays of L device pointers / leading dimensions (read
 * during the call), 1 <= L <= TGCN_JK_MAX_LAYERS; no alignment or padding is asked of them.  `lstm` is a HOST array of the
 * 8 device pointers {weight_ih [4 H, C] stride ldwi, weight_hh [4 H, H] stride ldwh, bias_ih [4 H], bias_hh [4 H]} of the
 * forward direction followed by the same four of the reverse direction, torch's nn.LSTM layout and gate order i, f, g, o.
 * att_w [2 H], att_b [1].  relu != 0: out = max(out, 0).  C, H >= 1, N >= 0; all offsets are 64-bit; no atomics.
 *
 *   tgcn_jk_lstm_forward   the whole step as one kernel on v_mfma_f32_32x32x2_f32: writes out [N, C] and alpha [N, L] and
 *                          nothing else -- no gate, cell or hidden value reaches memory.  H <= 256
 *                          (tgcn_jk_lstm_forward_supported(H) != 0); a wider one is TGCN_E_INVALID.
 *
 * The same arithmetic in pieces, for the backward by recomputation over row chunks and for the composed forward (R = rows of
 * the chunk; the products x_t W_ih^T, h W_hh^T, d gates W_hh, d gates W_ih and the weight gradients are tgcn_gemm_nt / _nn /
 * _tn, the bias gradients tgcn_colsum):
 *   tgcn_jk_cell            gates [R, 4 H] <- (sigmoid, sigmoid, tanh, sigmoid)(pre_x + pre_h + b_ih + b_hh), c = f c_prev + i g,
 *                           h = o tanh(c).  pre_h = NULL / c_prev = NULL: the first step (h = c = 0).  gates may be pre_x.
 *   tgcn_jk_attention       alpha and out from stored hidden states: h_fwd / h_bwd + t * hstep is h_t [R, H] stride ldh.
 *   tgcn_jk_attention_grad  dscore [R, L]: d score_t = alpha_t (d alpha_t - sum_s alpha_s d alpha_s), d alpha_t = G' . x_t,
 *                           G' = G where out > 0 (out != NULL: the relu epilogue) or G.
 *   tgcn_jk_cell_grad       d gates_t [R, 4 H] (at the pre-activations) from d h_t = dh_rec (NULL: none) + dscore_t att_w_dir
 *                           (dscore_t: column t of dscore, stride ldds; att_w_dir: the direction's H entries of att_w) and
 *                           dc = d c_t (dc_zero != 0: none yet); dc leaves as d c_{t-1}.
 *   tgcn_jk_input_grad      d x_t [R, C] = alpha_t G' + T    (alpha_t: column t of alpha, stride lda; T = d gates_t @ W_ih).
 */
#define TGCN_JK_MAX_LAYERS 8
int tgcn_jk_lstm_forward_supported(int H);
int tgcn_jk_lstm_forward(const float *const *xs, const int64_t *ldxs, int L, int64_t N, int C, int H,
                         const float *const *lstm, int64_t ldwi, int64_t ldwh, const float *att_w, const float *att_b,
                         float *out, int64_t ldo, float *alpha, int64_t lda, int relu, tgcn_stream stream);
int tgcn_jk_cell(const float *pre_x, int64_t ldpx, const float *pre_h, int64_t ldph, const float *b_ih, const float *b_hh,
                 const float *c_prev, int64_t ldcp, float *gates, int64_t ldg, float *c, int64_t ldc, float *h, int64_t ldh,
                 int64_t R, int H, tgcn_stream stream);
int tgcn_jk_attention(const float *const *xs, const int64_t *ldxs, int L, int64_t R, int C, int H, const float *h_fwd,
                      const float *h_bwd, int64_t ldh, int64_t hstep, const float *att_w, const float *att_b, float *out,
                      int64_t ldo, float *alpha, int64_t lda, int relu, tgcn_stream stream);
int tgcn_jk_attention_grad(const float *const *xs, const int64_t *ldxs, int L, int64_t R, int C, const float *G, int64_t ldg,
                           const float *out, int64_t ldo, const float *alpha, int64_t lda, float *dscore, int64_t ldds,
                           tgcn_stream stream);
int tgcn_jk_cell_grad(const float *gates, int64_t ldg, const float *c, int64_t ldc, const float *c_prev, int64_t ldcp,
                      const float *dh_rec, int64_t lddh, const float *dscore_t, int64_t ldds, const float *att_w_dir, float *dc,
                      int64_t lddc, int dc_zero, float *dgates, int64_t lddg, int64_t R, int H, tgcn_stream stream);
int tgcn_jk_input_grad(float *dx, int64_t lddx, const float *T, int64_t ldt, const float *G, int64_t ldg, const float *out,
                       int64_t ldo, const float *alpha_t, int64_t lda, int64_t R, int C, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Word-word PMI edges (graph construction). Replaces the reference's Cython
 * entry point `compute_word_word_edges(X, n_vocab, n_documents, seq_len, window_size, n_jobs, verbose)`
 * (textgcn/lib/clib/graphbuilder.pyx:23-25, called at text2graph.py:156-160) and its test hook
 * `sliding_window_tester` (:263-275).  Results are bit-identical to the reference: same uint32
 * counts, same edge order ((i,j),(j,i) interleaved, upper triangle row-major), same float32 PMI.
 *   X   int32 [n_docs, seq_len] row-major DEVICE pointer, tokens in [0, n_vocab), -1 = padding
 * Memory: the reference keeps the counts in a dense V(V+1)/2 array (graphbuilder.pyx:44,134) and wraps its uint32 index
 * beyond V = 65 535 (:250).  Here the dense triangle serves while it takes <= 16 GiB (V <= ~92 000); larger vocabularies
 * take the SPARSE counter -- (i << 32 | j, count) records of bounded chunks of documents, sorted, summed by key and merged
 * into one sorted list of distinct pairs: O(chunk + distinct pairs) memory, the same counts, edges, order and weights.
 * Environment (read at create): TGCN_WW_COUNTER=dense|sparse pins the counter, TGCN_WW_CHUNK_PAIRS the records per chunk
 * (default 2^27).  With the sparse counter the `cij` export builds the triangle on demand (small vocabularies only).
 * The handle owns its outputs (the reference leaks its malloc'd arrays, :65-66); export copies
 * them to host or device buffers (hipMemcpyDefault) and synchronises the stream.
 */
typedef struct tgcn_wwedges tgcn_wwedges;
enum { TGCN_WW_N_EDGES = 0, TGCN_WW_N_WINDOWS = 1, TGCN_WW_N_COUNTS = 2 /* n_vocab*(n_vocab+1)/2 */,
       TGCN_WW_SPARSE = 3 /* 1: the sorted-pair-list counter ran (large vocabularies), 0: the dense triangle */,
       TGCN_WW_N_PAIRS = 4 /* distinct pairs i <= j with a count (sparse counter; -1 for the dense one) */ };
int tgcn_wwedges_create(const int32_t *X, int64_t n_docs, int64_t seq_len, int64_t n_vocab,
                        int64_t window, int device, tgcn_stream stream, tgcn_wwedges **out);
int tgcn_wwedges_query(const tgcn_wwedges *we, int what, int64_t *out);
int tgcn_wwedges_export(const tgcn_wwedges *we, int32_t *coo /* [n_edges][2] */,
                        float *weights /* [n_edges] */, uint32_t *cij /* packed triangle or NULL */,
                        tgcn_stream stream);
int tgcn_wwedges_destroy(tgcn_wwedges *we);

/* tgcn_adam_step_capturable -- the same update with the step count on the DEVICE (torch's
 * `capturable=True`): `step_dev` (int64) is incremented by the call and `scalars_dev` (2 floats of
 * scratch) receives the step-dependent factors, so a captured HIP graph can be replayed per step. */
int tgcn_adam_step_capturable(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                              float *max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                              double eps, double weight_decay, int64_t *step_dev, float *scalars_dev,
                              tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * tgcn_foldin_two_layer -- the logits of documents that are NOT nodes of the training graph, from tables frozen out of a
 * trained two-layer network.  No counterpart in the reference: its Text2GraphTransformer has fit_transform
 * only and test documents must be nodes of the graph (flat_amazon.py:57-71).  A new document d is added with edges
 * word -> d only, weighted by its TF-IDF row, plus PyG's self loop: gcn_norm sums the degree at the TARGET, so no old node's
 * degree, weight or activation changes and d's row of the two-layer forward is a closed form.  For document d with the
 * entries (w_j, t_j), j in CSR order (rowptr int64 [n_docs + 1], col int32, val fp32):
 *     deg_d = (sum_j t_j) + 1     degree_sum = TGCN_DEGREE_REFERENCE: ONE fp32 accumulator, j in order, the loop's 1.0 last;
 *                                 TGCN_DEGREE_ACCURATE: float64 sum (lane j % 64 sums its entries in order, then a butterfly
 *                                 over the 64 partial sums, distances 32 .. 1) + 1.0, rounded to fp32 once
 *     dis_d = 1.0f / sqrtf(deg_d) (correctly rounded; inf -> 0)
 *     a_j   = (dis[w_j] * t_j) * dis_d   (reference)      t_j * (dis[w_j] * dis_d)   (accurate)      a_dd = dis_d * dis_d
 *     u     = act( sum_j a_j T1[w_j, 0:h]  +  a_dd s1  +  b1 )                                  -> hidden[d, 0:h]
 *     z     =      sum_j a_j P[w_j, 0:C]   +  a_dd (u W2)  +  b2                                -> logits[d, 0:C]
 * with every sum over j in CSR order from zero (one fused multiply-add per term), u W2 summed over k = 0 .. h-1 in order,
 * and the three terms of u and of z added left to right.  Duplicate columns add up; a document without entries has deg 1.
 *   dis  fp32 [n_vocab]   deg^-1/2 of the word nodes of the TRAINING graph (tgcn_gcn_norm in the same degree_sum)
 *   T1   [n_vocab, h] stride ldt1   word rows of the operand the first GCNConv propagates (x W1)
 *   s1   [h] or NULL (= zeros)      a new document's own row of that operand;   b1 [h], b2 [C] the biases
 *   P    [n_vocab, C] stride ldp    word rows of H1 W2, H1 the eval-mode output of the first layer after its activation
 *   W2   [h, C] stride ldw2;  act   TGCN_ACT_NONE / TGCN_ACT_RELU
 *   logits [n_docs, C] stride ldl;  pred int32 [n_docs] or NULL: the first arg-max of the row, as tgcn_masked_ce_pred breaks
 *   ties;  hidden [n_docs, h] stride ldh or NULL.  Nothing outside columns [0, C) / [0, h) of a row is written.
 * A document's result depends on its own row and the tables only -- not on the batch, its size or the position in it; no
 * atomics.  An entry whose column lies outside [0, n_vocab) is skipped in the two sums over j on the device (it still counts
 * in deg_d); rowptr is trusted.  One launch: a wavefront per document, TGCN_FOLDIN_DOCS_PER_WORKGROUP documents per workgroup
 * pass (at most TGCN_FOLDIN_WORKGROUP_CAP workgroups walk the batch), W2 in LDS, column ids and weights handed out through
 * v_readlane, 16-byte row loads.  Needs no plan, no workspace and no synchronisation; only enqueues on `stream` (legal under
 * HIP-graph capture).  TGCN_E_INVALID before anything is enqueued for h outside 1..tgcn_foldin_max_hidden() (256), C outside
 * 1..tgcn_foldin_max_classes() (128), n_vocab outside 1..2^31-1, n_docs < 0, a leading dimension below its width or not a
 * multiple of 4, an unknown act / degree_sum, and (n_docs > 0) a NULL pointer other than s1 / pred / hidden or a table,
 * bias or output that is not 16-byte aligned.  n_docs == 0 launches nothing.  Additive to ABI 7. */
#define TGCN_FOLDIN_DOCS_PER_WORKGROUP 16
#define TGCN_FOLDIN_WORKGROUP_CAP 512
int tgcn_foldin_max_hidden(void);
int tgcn_foldin_max_classes(void);
int tgcn_foldin_two_layer(int64_t n_docs, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_vocab,
                          const float *dis, int degree_sum, const float *T1, int64_t ldt1, int h, const float *s1,
                          const float *b1, int act, const float *P, int64_t ldp, int C, const float *W2, int64_t ldw2,
                          const float *b2, float *logits, int64_t ldl, int32_t *pred, float *hidden, int64_t ldh,
                          tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * tgcn_foldin_levels -- the same for the per-level strategy (perlevel_amazon.py, perlevel_dbpedia.py): L = 2
 * or 3 two-layer networks on ONE graph, level 1 on identity features, level l >= 2 on [I_N | H] with H a document's link of
 * the previous level's logits (C_{l-1} columns).  A new document has no identity column, so its feature row is [0 | p] and
 * its row of the first layer's operand is p Wh, Wh = W1[N : N + C_{l-1}].  The document's scalars deg_d, dis_d, a_j, a_dd
 * are those of tgcn_foldin_two_layer bit for bit (the same device code), computed once; for level 1
 *     u^1 = act( sum_j a_j T1^1[w_j] + b1^1 )         z^1 = (sum_j a_j P^1[w_j] + a_dd (u^1 W2^1)) + b2^1
 * -- tgcn_foldin_two_layer with s1 = NULL, bit for bit -- and for l >= 2
 *     p^l = link(z^{l-1})                             fp32 [C_{l-1}]                            -> link_out[d, 0:C_{l-1}]
 *     s^l = sum_c p^l_c Wh^l[c, :]                    c = 0 .. C_{l-1}-1 in order from zero, one FMA per term
 *     u^l = act( (sum_j a_j T1^l[w_j] + a_dd s^l) + b1^l )                                      -> hidden[d, 0:h_l]
 *     z^l = (sum_j a_j P^l[w_j] + a_dd (u^l W2^l)) + b2^l                                       -> logits[d, 0:C_l]
 * with the sums over j and k and the association of the terms as stated for tgcn_foldin_two_layer (a_dd s^l enters with one
 * FMA).  link, per level:
 *   TGCN_FOLDIN_LINK_SOFTMAX  m = max_c z_c;  e_c = expf(z_c - m) (the accurate expf);  S = the sum of the e_c in this order,
 *       which depends on C alone: t_i = e_i + e_{i+64} for i + 64 < C, t_i = e_i for the other i < C, t_i = 0 for
 *       C <= i < 64 (nothing is added there for C <= 64), then the butterfly t_i <- t_i + t_{i ^ off} over all 64 i at once
 *       for off = 32, 16, 8, 4, 2, 1;  p_c = e_c / S, a correctly rounded division.  All in fp32.
 *   TGCN_FOLDIN_LINK_ONE_HOT  p = the one-hot of the first arg-max of z (ties as tgcn_masked_ce_pred breaks them), so that
 *       s^l is the row Wh^l[k] itself (it is read, not summed: a non-finite entry of another row does not reach it).
 * `table` [n_vocab, ldt] is ONE combined table: a word's row holds, for every level, the segment T1^l = W1^l[w, 0:h_l] from
 * column t1_col on and the segment P^l = (H1^l W2^l)[w, 0:C_l] (H1^l the level's own eval-mode first layer) from column p_col
 * on; the segments begin at multiples of 4, lie in any order and may have gaps between them.  A word's 2L rows are then one
 * contiguous read from one row address.  Each level is one tgcn_foldin_level:  t1_col, p_col;  W2 [h, C] stride ldw2;  Wh [C_{l-1}, h] stride ldwh (level 1: ignored);  b1 [h], b2 [C];  act;
 * link (level 1: ignored);  outputs, EACH of which may be NULL: logits [n_docs, C] stride ldl, pred int32 [n_docs] (the first
 * arg-max), hidden [n_docs, h] stride ldh, link_out [n_docs, C_{l-1}] stride ldk (level 1: must be NULL).
 * Nothing beyond column h_l / C_l of a segment is read and nothing outside a result row's own columns is written.
 * One launch for all levels: a wavefront per document, TGCN_FOLDIN_DOCS_PER_WORKGROUP documents per workgroup pass, at most
 * TGCN_FOLDIN_WORKGROUP_CAP workgroups; one pass over the document's words gathers all 2L rows (lane l holds columns
 * 4l .. 4l+3 of each, 16-byte loads); the levels are then resolved in the wave's LDS slice against W2^l, Wh^l and the biases,
 * which the workgroup stages in LDS once.  No atomics, no workspace, no synchronisation; enqueues on `stream` only (legal under
 * HIP-graph capture); a document's bits do not depend on the batch.
 * LDS: tgcn_foldin_levels_lds_bytes(L, h[], C[]) = 4 * ( sum_l r4(h_l C_l) + sum_{l>=2} C_{l-1} r4(h_l)
 *      + (1 + TGCN_FOLDIN_DOCS_PER_WORKGROUP) * sum_l (r4(h_l) + r4(C_l)) ), r4 = rounded up to a multiple of 4: W2, Wh, the
 * biases once, and per wave a slice that holds every level's u and z -- host
 * arithmetic, callable without a GPU; -1 for L outside 2..3 or a width outside 1..256 / 1..128.  A need above
 * TGCN_FOLDIN_LEVELS_LDS_LIMIT is refused.  TGCN_E_INVALID before anything is enqueued, with the cause in tgcn_last_error, for
 * that, n_levels outside 2..3, ldt outside 4..2^31-1 or not a multiple of 4, a segment that begins off a multiple of 4 or ends
 * beyond ldt, the size, leading-dimension, alignment and enum rules of tgcn_foldin_two_layer applied to every level, and
 * (n_docs > 0) a NULL rowptr, col, val, dis, table, W2, b1, b2 or (l >= 2) Wh.  n_docs == 0 launches nothing.
 * Additive to ABI 7. */
#define TGCN_FOLDIN_LINK_SOFTMAX 0
#define TGCN_FOLDIN_LINK_ONE_HOT 1
#define TGCN_FOLDIN_MAX_LEVELS 3
#define TGCN_FOLDIN_LEVELS_LDS_LIMIT 163840 /* the 160 KiB of a CU */
typedef struct tgcn_foldin_level {
    int64_t t1_col;
    int64_t p_col;
    const float *W2;
    int64_t ldw2;
    const float *Wh;
    int64_t ldwh;
    const float *b1;
    const float *b2;
    float *logits;
    int64_t ldl;
    int32_t *pred;
    float *hidden;
    int64_t ldh;
    float *link_out;
    int64_t ldk;
    int32_t h, C, act, link;
} tgcn_foldin_level;
int64_t tgcn_foldin_levels_lds_bytes(int n_levels, const int32_t *h, const int32_t *C);
int tgcn_foldin_levels(int64_t n_docs, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_vocab,
                       const float *dis, int degree_sum, const float *table, int64_t ldt, int n_levels,
                       const tgcn_foldin_level *levels, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * tgcn_foldin_routed -- the same for the per-label strategy (perlabel_amazon.py, eval_perlabel.py:57-78): a
 * top two-layer network on identity features picks the top label k of a document, and the document's class is the arg-max
 * of label k's own two-layer network on the same graph.  `members` holds K + 1 networks: members[0] is the top network (its
 * C must equal K), members[1 + k] is routed member k; the K routed members share one h, the top network may have another.
 * The document's scalars deg_d, dis_d, a_j, a_dd are those of tgcn_foldin_two_layer bit for bit (the same device code).
 *     z^0   = tgcn_foldin_two_layer on the top network's segments, s1 = NULL, bit for bit         -> top_logits[d, 0:K]
 *     k     = route_in[d] when route_in is given, else the first arg-max of z^0                   -> route_out[d]
 *     u^k, z^k = tgcn_foldin_two_layer on member k's segments, s1 = NULL, bit for bit             -> hidden[d, 0:h]
 *     logits[d, 0:C_k] = z^k,  logits[d, C_k:Cmax] = -inf,  Cmax = max_k C_k  (argmax and softmax of the row are member k's)
 *     pred[d] = the first arg-max of z^k, or class_map[seg_k + that] when class_map is given, seg_k = sum_{j<k} r4(C_j)
 * With route_in (int32 [n_docs]) the top network is NOT evaluated: members[0] is not looked at (its h may be 0), top_logits
 * must be NULL and no column of the top network's segments is read.  A route outside [0, K) -- -1 means "nobody", as in
 * PerLabelGCN.predict -- gives pred = -1, a logits row of -inf, a hidden row of zeros, and no table row is read for it.
 * `table` [n_vocab, ldt] is ONE combined table as tgcn_foldin_levels takes it: a word's row holds every network's segments
 * T1 = W1[w, 0:h] from column t1_col and P = (H1 W2)[w, 0:C] from column p_col, each beginning at a multiple of 4; ONLY the
 * segments of the networks a document meets are read for it -- never the K h-wide row.  Each network is one
 * tgcn_foldin_member: t1_col, p_col; W2 [h, C] stride ldw2; b1 [h]; b2 [C]; h, C, act.  class_map int64 [sum_k r4(C_k)] or
 * NULL is perlabel.column_class_map's output.  Outputs, each of which may be NULL but not all: route_out int32 [n_docs],
 * top_logits [n_docs, K] stride ldtl, logits [n_docs, Cmax] stride ldl, pred int64 [n_docs], hidden [n_docs, h] stride ldh.
 * One launch: a wavefront per document, TGCN_FOLDIN_DOCS_PER_WORKGROUP documents per workgroup pass, at most
 * TGCN_FOLDIN_WORKGROUP_CAP workgroups; a pass over the document's words for the top network, the route through
 * readfirstlane, a second pass over the same words for member k alone.  W2 and b2 of every network that takes part are
 * staged in LDS once per workgroup.  No atomics, no workspace, no synchronisation; enqueues on `stream` only (legal under
 * HIP-graph capture); a document's bits depend on the widths, its own row and its route -- not on the batch.
 * LDS: tgcn_foldin_routed_lds_bytes(K, h[K + 1], C[K + 1]) = 4 * ( sum_m (r4(h_m C_m) + r4(C_m))
 *      + TGCN_FOLDIN_DOCS_PER_WORKGROUP * (max_m r4(h_m) + max_m r4(C_m)) ) over the networks that take part (h[0] == 0: no
 * top network) -- host arithmetic, callable without a GPU; -1 for K outside 1..TGCN_FOLDIN_MAX_MEMBERS, a width outside
 * 1..256 / 1..128 or routed members of unequal h.  A need above TGCN_FOLDIN_LEVELS_LDS_LIMIT is refused.  TGCN_E_INVALID
 * before anything is enqueued, with the cause in tgcn_last_error, for that, the size, segment, leading-dimension, alignment
 * and enum rules of tgcn_foldin_levels applied to every network that takes part, a top network whose C is not K, unequal
 * member h, no output at all, top_logits together with route_in, and (n_docs > 0) a NULL rowptr, col, val, dis, table, W2,
 * b1 or b2.  n_docs == 0 launches nothing.  Additive to ABI 7. */
#define TGCN_FOLDIN_MAX_MEMBERS 64
typedef struct tgcn_foldin_member {
    int64_t t1_col;
    int64_t p_col;
    const float *W2;
    int64_t ldw2;
    const float *b1;
    const float *b2;
    int32_t h, C, act, reserved;
} tgcn_foldin_member;
int64_t tgcn_foldin_routed_lds_bytes(int n_members, const int32_t *h, const int32_t *C);
int tgcn_foldin_routed(int64_t n_docs, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_vocab,
                       const float *dis, int degree_sum, const float *table, int64_t ldt, int n_members,
                       const tgcn_foldin_member *members, const int32_t *route_in, const int64_t *class_map,
                       int32_t *route_out, float *top_logits, int64_t ldtl, float *logits, int64_t ldl, int64_t *pred,
                       float *hidden, int64_t ldh, tgcn_stream stream);

/* ---------------------------------------------------------------------------------------------
 * tgcn_foldin_layers -- the same for a chain of L = 2, 3 or 4 GCNConv layers: models.py's GCN and EGCN at
 * n_gcn up to 4, and the layers of its JumpingKnowledgeNetwork, whose row-wise aggregation (JK-LSTM, attention, lin) then
 * runs on the L output rows.  A new document only receives edges, so no old node's activation changes in ANY layer and d's
 * row of layer l is a closed form over the frozen word table T^l = (H^{l-1} W_l)[0:n_vocab] (H^0 = x) and d's own previous
 * row.  The document's scalars deg_d, dis_d, a_j, a_dd are those of tgcn_foldin_two_layer bit for bit (the same device
 * code), computed once.  With the layer widths w_1 .. w_L:
 *     x^1 = act_1( (sum_j a_j T^1[w_j, 0:w_1]  +  a_dd s1)            +  b_1 )      s1 NULL = zeros     -> out_1[d, 0:w_1]
 *     x^l = act_l( (sum_j a_j T^l[w_j, 0:w_l]  +  a_dd (x^{l-1} W_l)) +  b_l )      l = 2 .. L          -> out_l[d, 0:w_l]
 * with every sum over j in CSR order from zero (one FMA per term), x^{l-1} W_l summed over k = 0 .. w_{l-1}-1 in order (one
 * FMA per term) and the three terms associated as tgcn_foldin_two_layer associates those of u and z: for l >= 2
 * fmaf(a_dd, y, sum) + b.  At L = 2 with act_2 = TGCN_ACT_NONE, out_1 / out_2 / pred are tgcn_foldin_two_layer's hidden /
 * logits / pred bit for bit; the first l outputs of an L-layer call are the l-layer call's on the same segments.
 * `table` [n_vocab, ldt] is ONE combined table as tgcn_foldin_levels takes it: a word's row holds the segment T^l from column
 * t_col on, each beginning at a multiple of 4, in any order, gaps allowed; a word's L rows are one contiguous read.  Each
 * layer is one tgcn_foldin_layer:  W [w_{l-1}, w_l] stride ldw (layer 1: ignored);  b [w_l];  out [n_docs, w_l] stride ldo or
 * NULL;  t_col, width;  act TGCN_ACT_NONE / TGCN_ACT_RELU;  reserved (ignored).  s1 [w_1] or NULL;  pred int32 [n_docs] or
 * NULL: the first arg-max of x^L, as tgcn_masked_ce_pred breaks ties.  Nothing beyond column w_l of a segment is read and
 * nothing outside columns [0, w_l) of an output row is written.  An entry whose column lies outside [0, n_vocab) is skipped
 * in the sums over j (it still counts in deg_d); rowptr is trusted.
 * One launch for all layers: a wavefront per document, TGCN_FOLDIN_DOCS_PER_WORKGROUP documents per workgroup pass, at most
 * TGCN_FOLDIN_WORKGROUP_CAP workgroups; one pass over the document's words gathers all L rows (lane i holds columns
 * 4i .. 4i+3 of each, 16-byte loads); the layers are then resolved in the wave's LDS slice against W_2 .. W_L and the biases,
 * which the workgroup stages in LDS once.  No atomics, no workspace, no synchronisation; enqueues on `stream` only (legal under
 * HIP-graph capture); a document's bits depend on the widths and its own row, not on the batch.
 * LDS: tgcn_foldin_layers_lds_bytes(L, w[]) = 4 * ( sum_{l>=2} r4(w_{l-1} w_l) + (1 + TGCN_FOLDIN_DOCS_PER_WORKGROUP) *
 *      sum_l r4(w_l) ), r4 = rounded up to a multiple of 4: W_2 .. W_L, the biases once, and per wave a slice that holds every
 * layer's row -- host arithmetic, callable without a GPU; -1 for L outside 2..TGCN_FOLDIN_MAX_LAYERS, w_1 outside 1..256 or a
 * further width outside 1..128 (x W gives a lane two columns).  A need above TGCN_FOLDIN_LEVELS_LDS_LIMIT is refused, the
 * bytes in the message.  TGCN_E_INVALID before anything is enqueued, with the cause in tgcn_last_error, for that, n_layers
 * outside 2..4, a width outside its range, ldt outside 4..2^31-1 or not a multiple of 4, a segment that begins off a multiple
 * of 4 or ends beyond ldt, n_vocab outside 1..2^31-1, n_docs < 0, ldw (l >= 2) or ldo (out given) below the width or not a
 * multiple of 4, an unknown act / degree_sum, and (n_docs > 0) a NULL rowptr, col, val, dis, table, b or (l >= 2) W, or a
 * table, s1, W, b or out that is not 16-byte aligned.  n_docs == 0 launches nothing.  Additive to ABI 7. */
#define TGCN_FOLDIN_MAX_LAYERS 4
typedef struct tgcn_foldin_layer {
    const float *W;
    int64_t ldw;
    const float *b;
    float *out;
    int64_t ldo;
    int32_t t_col, width, act, reserved;
} tgcn_foldin_layer;
int64_t tgcn_foldin_layers_lds_bytes(int n_layers, const int32_t *width);
int tgcn_foldin_layers(int64_t n_docs, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_vocab,
                       const float *dis, int degree_sum, const float *table, int64_t ldt, const float *s1, int n_layers,
                       const tgcn_foldin_layer *layers, int32_t *pred, tgcn_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* TGCN_H_ */
