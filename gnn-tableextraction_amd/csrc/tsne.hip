// Exact t-SNE on a precomputed distance matrix: the numerical stages of scikit-learn 1.7.2's method='exact'
// (sklearn/manifold/_t_sne.py: _joint_probabilities, _kl_divergence, _gradient_descent; _utils.pyx: _binary_search_perplexity),
// which Preprocessor.train_repr of the reference runs on the host through sklearn.manifold.TSNE.  The contract -- every formula,
// the stop rule, the state block, the deviations from scikit-learn -- is the definition in include/gte.h; tests/tsne_ref.py
// (numpy float64, written from it and pinned on scikit-learn's own functions) is the oracle.  t-SNE's descent is chaotic, so
// parity is bounded rounding per stage and per step, not equality of embeddings; what IS exact is the decision path of the
// perplexity search, the gains, the stop rule, and the bits of a second run.
//
// Structure.
//   cond_p    one workgroup of 256 lanes per row: the row's float32 distances in LDS (32 KB at the cap), the <= 100 steps of
//             the search inside the kernel.  Every lane holds the same two block sums, so the decision is uniform.  The row
//             of C doubles as the store of the unnormalised p_j between the two passes of a step (each lane re-reads only
//             what it wrote itself).
//   joint_p   two launches: row totals of C + C^T, then the rows of P (every workgroup adds the row totals in the same order).
//   iterate   three launches per iteration, every hand-off a kernel boundary:
//     z         a workgroup owns TS_Z_ROWS rows, a lane a column of every 256-column tile: one partial sum per workgroup.
//     grad      a workgroup owns TS_G_ROWS rows.  It first adds the z partials (every workgroup in the same order), then walks
//               the columns in tiles of 256: a lane keeps its column's y_j in registers for all rows of the block, the rows'
//               own y_i sit in LDS, P is read row-major (a wave reads 512 contiguous bytes).  Row sums: per lane over the
//               tiles, a wave butterfly, the four waves in order.  The epilogue applies the update to the block's own rows and
//               writes the new Y into the OTHER Y buffer: no workgroup ever reads a half-updated embedding.
//     decide    ONE workgroup: on check iterations (and the last) it finishes KL and the gradient norm from the per-workgroup
//               partials and applies the stop rule; always: advances the iteration count and flips the current Y buffer.
// The stop lives on the device, as affprop's: every kernel reads the state block first and returns untouched when `stopped` is
// set or max_iter is reached, so iterations enqueued behind the stopping one change nothing.
//
// Addition chains (what the tests' bounds use).  Z: a lane adds TS_Z_ROWS terms per column tile, ceil(n / 256) tiles; 6 butterfly
// levels and 3 adds merge the workgroup; in the gradient pass a lane adds up to ceil(G / 256) of the G = ceil(n / TS_Z_ROWS)
// partials (G <= 512: at most 2), then again 6 + 3.  The longest chain into Z is therefore
//     L(n) = TS_Z_ROWS * ceil(n / 256) + ceil(ceil(n / TS_Z_ROWS) / 256) + 18            (52 at n = 300, 532 at n = 8192; <= n from n = 36)
// additions.  A row sum of the gradient: ceil(n / 256) + 9.  KL: TS_G_ROWS * ceil(n / 256) + 9 per workgroup, then
// ceil(ceil(n / TS_G_ROWS) / 256) + 9 in the decision.  No floating-point atomics anywhere: two runs give the same bits.
// All arithmetic is float64 with contraction off (every product and sum is rounded on its own, as numpy does); num's power
// -(alpha + 1) / 2 is an integer or half-integer, so it is products, one sqrt and one division: a few ulp, no pow.
#include "gte_common.h"

#include <float.h>

namespace {

constexpr int TS_MAX_N = 8192;                        // P alone is 512 MB at the cap; the row of cond_p is 32 KB of LDS
constexpr int TS_MAX_D = 8;
constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / gte::kWave;
constexpr int TS_Z_ROWS = 16;                         // rows per workgroup of the Z pass
constexpr int TS_G_ROWS = 4;                          // rows per workgroup of the gradient pass
constexpr int TS_SEARCH_STEPS = 100;
constexpr int TS_CHECK_EVERY = 50;                    // scikit-learn's _N_ITER_CHECK
constexpr double TS_EPS = DBL_EPSILON;                // np.finfo(np.double).eps
static_assert(TS_MAX_N * 4 <= 48 * 1024, "the row of distances fits LDS without an opt-in");
static_assert(TS_G_ROWS * TS_MAX_D <= gte::kWave, "the epilogue is one lane per (row, component) inside the first wave");

// state block (float64 [8], device memory; the integers are held exactly)
enum { ST_IT = 0, ST_STOPPED = 1, ST_REASON = 2, ST_BEST_ITER = 3, ST_CUR = 4, ST_ERROR = 5, ST_BEST_ERROR = 6, ST_GRAD_NORM = 7 };
enum { REASON_NONE = 0, REASON_NO_PROGRESS = 1, REASON_GRAD_NORM = 2 };

__device__ __forceinline__ bool frozen(const double* state, int max_iter) {
    return state[ST_STOPPED] != 0.0 || state[ST_IT] >= (double)max_iter;
}
__device__ __forceinline__ bool wants_error(int it, int max_iter) { return (it + 1) % TS_CHECK_EVERY == 0 || it == max_iter - 1; }

// The sum of v over the 256 lanes of the workgroup, the same bits in every lane: a wave butterfly (6 levels), then the four wave
// sums in wave order.  `s_red` is TS_WAVES doubles of LDS; two barriers, so it may be reused right after the call.
__device__ __forceinline__ double block_sum(double v, double* s_red) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 1; off < gte::kWave; off <<= 1) v = v + __shfl_xor(v, off, gte::kWave);
    __syncthreads();                                                     // s_red is free (a previous call has been read)
    if ((threadIdx.x & (gte::kWave - 1)) == 0) s_red[threadIdx.x / gte::kWave] = v;
    __syncthreads();
    double total = s_red[0];
#pragma unroll
    for (int w = 1; w < TS_WAVES; ++w) total = total + s_red[w];
    return total;
}

// ---- conditional probabilities ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TS_THREADS)
tsne_cond_p_kernel(const float* __restrict__ D2, int n, float perplexity, double* __restrict__ C, double* __restrict__ beta_out) {
#pragma clang fp contract(off)
    __shared__ float s_d[TS_MAX_N];
    __shared__ double s_red[TS_WAVES];
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    const float* __restrict__ d_row = D2 + (int64_t)i * n;
    double* c_row = C + (int64_t)i * n;
    for (int j = tid; j < n; j += TS_THREADS) s_d[j] = d_row[j];
    __syncthreads();

    const double target = log((double)perplexity);
    const double tol = (double)1e-5f;
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
    for (int step = 0; step < TS_SEARCH_STEPS; ++step) {                 // (every lane takes the same path: s and t are block sums)
        double part = 0.0;
        for (int j = tid; j < n; j += TS_THREADS) {
            const double p = j == i ? 0.0 : exp(-(double)s_d[j] * beta);
            c_row[j] = p;
            part = part + p;
        }
        double s = block_sum(part, s_red);
        if (s == 0.0) s = (double)1e-8f;
        part = 0.0;
        for (int j = tid; j < n; j += TS_THREADS) {
            const double p = c_row[j] / s;                               // (this lane's own store of the pass above)
            c_row[j] = p;
            part = part + (double)s_d[j] * p;
        }
        const double t = block_sum(part, s_red);
        const double diff = (log(s) + beta * t) - target;
        if (fabs(diff) <= tol) break;
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
    if (tid == 0) beta_out[i] = beta;
}

// ---- joint probabilities ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TS_THREADS)
tsne_joint_rows_kernel(const double* __restrict__ C, int n, double* __restrict__ row_total) {
#pragma clang fp contract(off)
    __shared__ double s_red[TS_WAVES];
    const int i = blockIdx.x;
    double part = 0.0;
    for (int j = threadIdx.x; j < n; j += TS_THREADS) part = part + (C[(int64_t)i * n + j] + C[(int64_t)j * n + i]);
    const double total = block_sum(part, s_red);
    if (threadIdx.x == 0) row_total[i] = total;
}

__global__ void __launch_bounds__(TS_THREADS)
tsne_joint_p_kernel(const double* __restrict__ C, int n, const double* __restrict__ row_total, double* __restrict__ P) {
#pragma clang fp contract(off)
    __shared__ double s_red[TS_WAVES];
    const int i = blockIdx.x;
    double part = 0.0;
    for (int r = threadIdx.x; r < n; r += TS_THREADS) part = part + row_total[r];
    double total = block_sum(part, s_red);
    if (!(total > TS_EPS)) total = TS_EPS;
    for (int j = threadIdx.x; j < n; j += TS_THREADS) {
        const double p = (C[(int64_t)i * n + j] + C[(int64_t)j * n + i]) / total;
        P[(int64_t)i * n + j] = j == i ? 0.0 : (p > TS_EPS ? p : TS_EPS);
    }
}

// ---- one iteration ----------------------------------------------------------------------------------------------------------------
// alpha = max(D - 1, 1); num = x^(-(alpha + 1) / 2): x^(K / 2) with K = alpha + 1 as K / 2 products and, for odd K, one sqrt
template <int D>
__device__ __forceinline__ double num_of(double dist) {
#pragma clang fp contract(off)
    constexpr int ALPHA = D > 1 ? D - 1 : 1;
    constexpr int K = ALPHA + 1;
    const double x = 1.0 + dist / (double)ALPHA;
    double pw = 1.0;
#pragma unroll
    for (int k = 0; k < K / 2; ++k) pw = pw * x;
    if constexpr (K % 2 == 1) pw = pw * sqrt(x);
    return 1.0 / pw;
}

template <int D>
__global__ void __launch_bounds__(TS_THREADS)
tsne_z_kernel(const double* __restrict__ Y, int n, double* __restrict__ z_part, const double* __restrict__ state, int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;                                 // (uniform: ahead of every barrier)
    __shared__ double s_yi[TS_Z_ROWS * D];
    __shared__ double s_red[TS_WAVES];
    const int tid = threadIdx.x;
    const double* __restrict__ y = Y + (state[ST_CUR] != 0.0 ? (int64_t)n * D : 0);
    const int i0 = blockIdx.x * TS_Z_ROWS;
    const int rows = min(TS_Z_ROWS, n - i0);
    for (int k = tid; k < rows * D; k += TS_THREADS) s_yi[k] = y[(int64_t)i0 * D + k];
    __syncthreads();
    double part = 0.0;
    for (int j = tid; j < n; j += TS_THREADS) {
        double yj[D];
#pragma unroll
        for (int c = 0; c < D; ++c) yj[c] = y[(int64_t)j * D + c];
        for (int r = 0; r < rows; ++r) {
            double dist = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const double diff = s_yi[r * D + c] - yj[c];
                dist = dist + diff * diff;
            }
            const double num = num_of<D>(dist);
            part = part + (i0 + r == j ? 0.0 : num);
        }
    }
    const double total = block_sum(part, s_red);
    if (tid == 0) z_part[blockIdx.x] = total;
}

template <int D>
__global__ void __launch_bounds__(TS_THREADS)
tsne_grad_kernel(const double* __restrict__ P, double* __restrict__ Y, double* __restrict__ update, double* __restrict__ gains, int n,
                 double lr, double momentum, double exaggeration, const double* __restrict__ z_part, int n_z_part,
                 double* __restrict__ z_out, double* __restrict__ kl_part, double* __restrict__ gn2_part, const double* __restrict__ state, int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;                                 // (uniform: ahead of every barrier)
    constexpr int ALPHA = D > 1 ? D - 1 : 1;
    __shared__ double s_yi[TS_G_ROWS * D];
    __shared__ double s_red[TS_WAVES];
    __shared__ double s_g[TS_G_ROWS * D];
    const int tid = threadIdx.x;
    const bool cur = state[ST_CUR] != 0.0;
    const double* __restrict__ y = Y + (cur ? (int64_t)n * D : 0);
    double* __restrict__ y_new = Y + (cur ? 0 : (int64_t)n * D);
    const bool with_error = wants_error((int)state[ST_IT], max_iter);
    const int i0 = blockIdx.x * TS_G_ROWS;
    const int rows = min(TS_G_ROWS, n - i0);
    for (int k = tid; k < rows * D; k += TS_THREADS) s_yi[k] = y[(int64_t)i0 * D + k];

    double zp = 0.0;
    for (int k = tid; k < n_z_part; k += TS_THREADS) zp = zp + z_part[k];
    const double Z = block_sum(zp, s_red);                               // (its barriers also publish s_yi)
    if (blockIdx.x == 0 && tid == 0) z_out[0] = Z;                       // (a record for the tests: nothing reads it)

    double acc[TS_G_ROWS][D];
#pragma unroll
    for (int r = 0; r < TS_G_ROWS; ++r)
#pragma unroll
        for (int c = 0; c < D; ++c) acc[r][c] = 0.0;
    double kl = 0.0;
    for (int j = tid; j < n; j += TS_THREADS) {
        double yj[D];
#pragma unroll
        for (int c = 0; c < D; ++c) yj[c] = y[(int64_t)j * D + c];
#pragma unroll
        for (int r = 0; r < TS_G_ROWS; ++r) {
            if (r < rows && i0 + r != j) {
                double diff[D];
                double dist = 0.0;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    diff[c] = s_yi[r * D + c] - yj[c];
                    dist = dist + diff[c] * diff[c];
                }
                const double num = num_of<D>(dist);
                const double qr = num / Z;
                const double q = qr > TS_EPS ? qr : TS_EPS;
                const double pe = exaggeration * P[(int64_t)(i0 + r) * n + j];
                const double w = (pe - q) * num;
#pragma unroll
                for (int c = 0; c < D; ++c) acc[r][c] = acc[r][c] + w * diff[c];
                if (with_error) kl = kl + pe * log((pe > TS_EPS ? pe : TS_EPS) / q);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < TS_G_ROWS; ++r)
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const double total = block_sum(acc[r][c], s_red);
            if (tid == 0) s_g[r * D + c] = total;
        }
    if (with_error) {                                                    // (uniform)
        const double total = block_sum(kl, s_red);
        if (tid == 0) kl_part[blockIdx.x] = total;
    }
    __syncthreads();                                                     // s_g is complete

    // the update of the block's own rows: one lane per (row, component), all inside the first wave
    double g2 = 0.0;
    if (tid < rows * D) {
        const int64_t at = (int64_t)i0 * D + tid;
        const double grad = s_g[tid] * (2.0 * (ALPHA + 1.0) / ALPHA);
        const double upd = update[at];
        double gain = gains[at];
        gain = upd * grad < 0.0 ? gain + 0.2 : gain * 0.8;
        gain = gain > 0.01 ? gain : 0.01;                                // (np.clip: a NaN gain stays NaN there, becomes 0.01 here)
        const double g = grad * gain;
        const double keep = momentum * upd;
        const double step = lr * g;
        const double upd_new = keep - step;
        gains[at] = gain;
        update[at] = upd_new;
        y_new[at] = y[at] + upd_new;
        g2 = g * g;
    }
    if (tid < gte::kWave) {                                              // (the whole first wave: no divergence inside the butterfly)
#pragma unroll
        for (int off = 1; off < gte::kWave; off <<= 1) g2 = g2 + __shfl_xor(g2, off, gte::kWave);
        if (tid == 0) gn2_part[blockIdx.x] = g2;
    }
}

__global__ void __launch_bounds__(TS_THREADS)
tsne_decide_kernel(const double* __restrict__ kl_part, const double* __restrict__ gn2_part, int n_part, int n_iter_without_progress,
                   double min_grad_norm, int max_iter, double* state) {
#pragma clang fp contract(off)
    __shared__ double s_red[TS_WAVES];
    if (frozen(state, max_iter)) return;                                 // (uniform; block_sum's barriers come before any write)
    const int it = (int)state[ST_IT];
    const bool check = (it + 1) % TS_CHECK_EVERY == 0;
    double error = 0.0, gn2 = 0.0;
    if (wants_error(it, max_iter)) {
        double part = 0.0;
        for (int k = threadIdx.x; k < n_part; k += TS_THREADS) part = part + kl_part[k];
        error = block_sum(part, s_red);
    }
    if (check) {
        double part = 0.0;
        for (int k = threadIdx.x; k < n_part; k += TS_THREADS) part = part + gn2_part[k];
        gn2 = block_sum(part, s_red);
    }
    __syncthreads();                                                     // every lane has read the state
    if (threadIdx.x != 0) return;
    if (wants_error(it, max_iter)) state[ST_ERROR] = error;
    if (check) {
        const double grad_norm = sqrt(gn2);
        state[ST_GRAD_NORM] = grad_norm;
        bool stop = false;
        if (error < state[ST_BEST_ERROR]) {
            state[ST_BEST_ERROR] = error;
            state[ST_BEST_ITER] = (double)it;
        } else if ((double)it - state[ST_BEST_ITER] > (double)n_iter_without_progress) {
            state[ST_REASON] = REASON_NO_PROGRESS;
            stop = true;
        }
        if (!stop && grad_norm <= min_grad_norm) {
            state[ST_REASON] = REASON_GRAD_NORM;
            stop = true;
        }
        if (stop) state[ST_STOPPED] = 1.0;
    }
    state[ST_IT] = (double)(it + 1);
    state[ST_CUR] = state[ST_CUR] != 0.0 ? 0.0 : 1.0;
}

constexpr int64_t TS_ALIGN = 256;
int64_t z_parts(int64_t n) { return gte::ceil_div(n, TS_Z_ROWS); }
int64_t g_parts(int64_t n) { return gte::ceil_div(n, TS_G_ROWS); }
int64_t z_bytes(int64_t n) { return gte::round_up((z_parts(n) + 1) * 8, TS_ALIGN); }   // the partials, then Z itself
int64_t g_bytes(int64_t n) { return gte::round_up(g_parts(n) * 8, TS_ALIGN); }

template <int D>
void launch_iterations(const double* P, double* Y, double* update, double* gains, int n, double lr, double momentum, double exaggeration,
                       int n_iter_without_progress, double min_grad_norm, int max_iter, int n_iters, double* z_part, double* kl_part,
                       double* gn2_part, double* state, hipStream_t st) {
    const int nz = (int)z_parts(n), ng = (int)g_parts(n);
    for (int s = 0; s < n_iters; ++s) {
        hipLaunchKernelGGL(tsne_z_kernel<D>, dim3((unsigned)nz), dim3(TS_THREADS), 0, st, Y, n, z_part, state, max_iter);
        hipLaunchKernelGGL(tsne_grad_kernel<D>, dim3((unsigned)ng), dim3(TS_THREADS), 0, st, P, Y, update, gains, n, lr, momentum,
                           exaggeration, z_part, nz, z_part + nz, kl_part, gn2_part, state, max_iter);
        hipLaunchKernelGGL(tsne_decide_kernel, dim3(1), dim3(TS_THREADS), 0, st, kl_part, gn2_part, ng, n_iter_without_progress,
                           min_grad_norm, max_iter, state);
    }
}

}  // namespace

extern "C" int gte_tsne_max_n(void) { return TS_MAX_N; }
extern "C" int gte_tsne_max_components(void) { return TS_MAX_D; }

extern "C" int64_t gte_tsne_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    const int64_t iterate = z_bytes(n) + 2 * g_bytes(n);                 // z, KL and |g|^2 partials
    const int64_t joint = gte::round_up(n * 8, TS_ALIGN);                // row totals
    return iterate > joint ? iterate : joint;
}

extern "C" int gte_tsne_cond_p(const float* sq_dist, int64_t n, float perplexity, double* cond_p, double* beta, void* stream) {
    if (n < 0) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_cond_p: n %lld < 0", (long long)n);
    if (!(perplexity > 0.f) || !(perplexity < INFINITY))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_cond_p: perplexity %g must be positive and finite", (double)perplexity);
    if (n > TS_MAX_N) return gte::fail(GTE_ERR_UNSUPPORTED, "tsne_cond_p: n %lld (limit %d)", (long long)n, TS_MAX_N);
    if (n == 0) return GTE_OK;
    if (!sq_dist || !cond_p || !beta) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_cond_p: null pointer");
    if (((uintptr_t)sq_dist & 3) != 0 || (((uintptr_t)cond_p | (uintptr_t)beta) & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_cond_p: float32 arrays must be 4-byte aligned, float64 arrays 8-byte");
    hipLaunchKernelGGL(tsne_cond_p_kernel, dim3((unsigned)n), dim3(TS_THREADS), 0, gte::as_stream(stream), sq_dist, (int)n, perplexity,
                       cond_p, beta);
    return gte::check_launch("tsne_cond_p");
}

extern "C" int gte_tsne_joint_p(const double* cond_p, int64_t n, double* P, void* workspace, int64_t workspace_bytes, void* stream) {
    if (n < 0) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_joint_p: n %lld < 0", (long long)n);
    if (n > TS_MAX_N) return gte::fail(GTE_ERR_UNSUPPORTED, "tsne_joint_p: n %lld (limit %d)", (long long)n, TS_MAX_N);
    if (n == 0) return GTE_OK;
    if (!cond_p || !P || !workspace) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_joint_p: null pointer");
    if ((((uintptr_t)cond_p | (uintptr_t)P | (uintptr_t)workspace) & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_joint_p: float64 arrays and the workspace must be 8-byte aligned");
    const int64_t need = gte_tsne_workspace_bytes(n);
    if (workspace_bytes < need)
        return gte::fail(GTE_ERR_WORKSPACE_TOO_SMALL, "tsne_joint_p: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                         (long long)need);
    double* row_total = static_cast<double*>(workspace);
    hipStream_t st = gte::as_stream(stream);
    hipLaunchKernelGGL(tsne_joint_rows_kernel, dim3((unsigned)n), dim3(TS_THREADS), 0, st, cond_p, (int)n, row_total);
    hipLaunchKernelGGL(tsne_joint_p_kernel, dim3((unsigned)n), dim3(TS_THREADS), 0, st, cond_p, (int)n, row_total, P);
    return gte::check_launch("tsne_joint_p");
}

extern "C" int gte_tsne_iterate(const double* P, double* Y, double* update, double* gains, int64_t n, int n_components, double learning_rate,
                                double momentum, double exaggeration, int n_iter_without_progress, double min_grad_norm, int max_iter,
                                int n_iters, void* workspace, int64_t workspace_bytes, double* state, void* stream) {
    if (n < 0 || n_components < 1 || max_iter < 0 || n_iters < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_iterate: bad sizes (n %lld, n_components %d, max_iter %d, n_iters %d)",
                         (long long)n, n_components, max_iter, n_iters);
    if (n > TS_MAX_N || n_components > TS_MAX_D)
        return gte::fail(GTE_ERR_UNSUPPORTED, "tsne_iterate: n %lld, n_components %d (limits %d, %d)", (long long)n, n_components,
                         TS_MAX_N, TS_MAX_D);
    if (n == 0 || n_iters == 0) return GTE_OK;
    if (!P || !Y || !update || !gains || !workspace || !state) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_iterate: null pointer");
    if ((((uintptr_t)P | (uintptr_t)Y | (uintptr_t)update | (uintptr_t)gains | (uintptr_t)workspace | (uintptr_t)state) & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "tsne_iterate: float64 arrays, the workspace and the state must be 8-byte aligned");
    const int64_t need = gte_tsne_workspace_bytes(n);
    if (workspace_bytes < need)
        return gte::fail(GTE_ERR_WORKSPACE_TOO_SMALL, "tsne_iterate: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                         (long long)need);
    double* z_part = static_cast<double*>(workspace);
    double* kl_part = reinterpret_cast<double*>(static_cast<char*>(workspace) + z_bytes(n));
    double* gn2_part = reinterpret_cast<double*>(static_cast<char*>(workspace) + z_bytes(n) + g_bytes(n));
    hipStream_t st = gte::as_stream(stream);
#define TS_CASE(D)                                                                                                                   \
    case D:                                                                                                                          \
        launch_iterations<D>(P, Y, update, gains, (int)n, learning_rate, momentum, exaggeration, n_iter_without_progress, min_grad_norm, \
                             max_iter, n_iters, z_part, kl_part, gn2_part, state, st);                                               \
        break;
    switch (n_components) {
        TS_CASE(1) TS_CASE(2) TS_CASE(3) TS_CASE(4) TS_CASE(5) TS_CASE(6) TS_CASE(7) TS_CASE(8)
    }
#undef TS_CASE
    return gte::check_launch("tsne_iterate");
}
