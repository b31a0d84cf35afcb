// EM for a one-dimensional Gaussian mixture: the loop body of scikit-learn 1.7.2's BaseMixture.fit_predict with
// covariance_type='full' and one feature (sklearn/mixture/_base.py, _gaussian_mixture.py), soft, and the hard variant of the
// reference's HardEMGaussianMixture, which Preprocessor.train_gmm of the reference runs on the host over up to 2 000 000 numerals x
// 20 components x 100 iterations.  The contract -- every formula, the addition order, the state block, the limits -- is the
// definition in include/gte.h; tests/gmm_ref.py (numpy float64, written from it and pinned on scikit-learn) is the oracle.
//
// Structure.  One iteration is four launches, every hand-off a kernel boundary; no [n, K] buffer exists anywhere.
//   pass A      a workgroup of 256 lanes owns GM_WG_SAMPLES = 2048 consecutive samples, a lane 8 of them (sample base + s * 256 + lane:
//               a wave reads 512 contiguous bytes), held in registers with their lse.  The components' constants (pc, mu * pc,
//               log pc, log w) sit in LDS and are read as broadcasts.  Every loop is component-outer, sample-inner: the eight
//               samples are eight independent chains.  E step (maximum, sum of exp, lse, in hard mode the label), lse / label
//               stored, then per component the lane's sums of resp and resp * x.
//   finalise A  ONE workgroup: nk and the means from the per-workgroup partials, the sum of lse.
//   pass B      same ownership; resp recomputed as exp(wlp - lse) from the stored lse (hard: the stored label), the lane's sums of
//               (resp * (x - mean)) * (x - mean).
//   finalise B  ONE workgroup: covariances, pc, weights into P; lower bound, change, stop decision into the state.
// How the K accumulators are held: they are not.  With the component loop outside, a lane carries the two running sums of ONE
// component at a time (4 VGPRs); what it keeps across components are its 8 samples and their lse (32 VGPRs).  Per-lane registers for
// all K (2 x 64 doubles = 256 VGPRs) would spill; a per-lane LDS column acc[k][lane] (2 x K x 256 x 8 B) passes 160 KB at K = 40.
// The price is one wave butterfly per component and sum instead of one per sum, 12 shuffles against 16 exp of the lanes.
//
// Addition order (the contract's): a lane adds its own samples in index order; a wave butterfly (6 levels, xor 1 .. 32), then the
// four waves in wave order merge the workgroup; the partials go to the workspace as part[item][workgroup]; in the finalising
// workgroup a wave owns a sum, its lane l adds the partials of workgroups l, l + 64, ... in that order, and a butterfly merges the 64
// lanes.  The grid is ceil(n / 2048): a function of n only, never of the device.  The longest addition chain into any sum over the
// samples is therefore
//     L(n) = 8 + 6 + 3 + ceil(ceil(n / 2048) / 64) + 6 = 23 + ceil(ceil(n / 2048) / 64)         (24 up to n = 131 072, 39 at n = 2 000 000)
// additions.  No floating-point atomics: two runs give the same bits.  All arithmetic is float64 with contraction off.
#include "gte_common.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int GM_MAX_K = 64;
constexpr int GM_THREADS = 256;
constexpr int GM_WAVES = GM_THREADS / gte::kWave;
constexpr int GM_LANE_SAMPLES = 8;
constexpr int GM_WG_SAMPLES = GM_THREADS * GM_LANE_SAMPLES;
constexpr double GM_EPS = DBL_EPSILON;
constexpr double GM_LOG_2PI = 0x1.d67f1c864beb4p+0;   // np.log(2 * np.pi)
constexpr int64_t GM_ALIGN = 256;

// state block (float64 [8], device memory; the integers are held exactly)
enum { ST_IT = 0, ST_STOPPED = 1, ST_CONVERGED = 2, ST_ERROR = 3, ST_LB = 4, ST_PREV = 5, ST_CHANGE = 6, ST_RESERVED = 7 };

__device__ __forceinline__ bool frozen(const double* state, int max_iter) {
    return state[ST_STOPPED] != 0.0 || state[ST_IT] >= (double)max_iter;
}

// what the E step needs of a component, from P = (weights, means, covariances, precisions_cholesky) [4, K]
struct CompTable {
    double pc[GM_MAX_K], mupc[GM_MAX_K], logpc[GM_MAX_K], logw[GM_MAX_K];
};

__device__ __forceinline__ void load_components(const double* __restrict__ P, int K, CompTable& t) {
#pragma clang fp contract(off)
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const double w = P[k], mu = P[K + k], pc = P[3 * K + k];
        t.pc[k] = pc;
        t.mupc[k] = mu * pc;
        t.logpc[k] = log(pc);
        t.logw[k] = log(w);
    }
}

// wlp[i,k] = -0.5 * (log(2 pi) + (x_i * pc_k - mu_k * pc_k)^2) + log(pc_k) + log(w_k): THE one definition (pass A, pass B, posterior)
__device__ __forceinline__ double wlp_of(double x, const CompTable& t, int k) {
#pragma clang fp contract(off)
    const double y = x * t.pc[k] - t.mupc[k];
    return ((-0.5 * (GM_LOG_2PI + y * y)) + t.logpc[k]) + t.logw[k];
}

// The E step of NS samples of one lane: lse and, in hard mode, the first-index arg-max of the rounded wlp - lse.
template <int NS>
__device__ __forceinline__ void e_step(const double (&x)[NS], const CompTable& t, int K, bool want_label, double (&lse)[NS], int (&label)[NS]) {
#pragma clang fp contract(off)
    double m[NS], sum[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) m[s] = -INFINITY;
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double w = wlp_of(x[s], t, k);
            m[s] = w > m[s] ? w : m[s];
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (!(fabs(m[s]) < INFINITY)) m[s] = 0.0;                         // (scipy's logsumexp: a maximum that is not finite counts as 0)
        sum[s] = 0.0;
    }
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int s = 0; s < NS; ++s) sum[s] = sum[s] + exp(wlp_of(x[s], t, k) - m[s]);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        lse[s] = log(sum[s]) + m[s];
        label[s] = 0;
    }
    if (want_label) {
        double best[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) best[s] = -INFINITY;
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double v = wlp_of(x[s], t, k) - lse[s];
                if (v > best[s]) {                                       // (strictly greater: ties stay with the first index, as np.argmax)
                    best[s] = v;
                    label[s] = k;
                }
            }
        }
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 1; off < gte::kWave; off <<= 1) v = v + __shfl_xor(v, off, gte::kWave);
    return v;
}

// the samples of this lane: base + s * 256 + lane; past n: x = 0 and every contribution is an exact 0
__device__ __forceinline__ void load_samples(const double* __restrict__ x, int64_t n, double (&xs)[GM_LANE_SAMPLES], bool (&valid)[GM_LANE_SAMPLES]) {
    const int64_t base = (int64_t)blockIdx.x * GM_WG_SAMPLES + threadIdx.x;
#pragma unroll
    for (int s = 0; s < GM_LANE_SAMPLES; ++s) {
        const int64_t i = base + (int64_t)s * GM_THREADS;
        valid[s] = i < n;
        xs[s] = valid[s] ? x[i] : 0.0;
    }
}

// ---- pass A: E step, partials of nk, sum resp * x and sum lse -------------------------------------------------------------------------
// part: items 0 .. K-1 = nk, K .. 2K-1 = sum resp * x, 2K = sum lse; item j of workgroup g at part[j * G + g]
__global__ void __launch_bounds__(GM_THREADS)
gmm_pass_a_kernel(const double* __restrict__ x, int64_t n, int K, const double* __restrict__ P, int hard, double* __restrict__ lse_out,
                  int32_t* __restrict__ label_out, double* __restrict__ part, const double* __restrict__ state, int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;                                 // (uniform: ahead of every barrier)
    __shared__ CompTable t;
    __shared__ double s_w[2 * GM_MAX_K + 1][GM_WAVES];
    const int tid = threadIdx.x, lane = tid & (gte::kWave - 1), wave = tid / gte::kWave;
    const int64_t G = gridDim.x;
    load_components(P, K, t);
    double xs[GM_LANE_SAMPLES], lse[GM_LANE_SAMPLES];
    int label[GM_LANE_SAMPLES];
    bool valid[GM_LANE_SAMPLES];
    load_samples(x, n, xs, valid);
    __syncthreads();
    e_step<GM_LANE_SAMPLES>(xs, t, K, hard != 0, lse, label);

    const int64_t base = (int64_t)blockIdx.x * GM_WG_SAMPLES + tid;
    double ls = 0.0;
#pragma unroll
    for (int s = 0; s < GM_LANE_SAMPLES; ++s) {
        if (valid[s]) {
            const int64_t i = base + (int64_t)s * GM_THREADS;
            lse_out[i] = lse[s];
            if (hard) label_out[i] = label[s];
            ls = ls + lse[s];
        }
    }
    ls = wave_sum(ls);
    if (lane == 0) s_w[2 * K][wave] = ls;
    for (int k = 0; k < K; ++k) {
        double nk = 0.0, sx = 0.0;
#pragma unroll
        for (int s = 0; s < GM_LANE_SAMPLES; ++s) {
            double r;
            if (hard) r = label[s] == k ? 1.0 : 0.0;
            else r = exp(wlp_of(xs[s], t, k) - lse[s]);
            if (!valid[s]) r = 0.0;
            nk = nk + r;
            sx = sx + r * xs[s];
        }
        nk = wave_sum(nk);
        sx = wave_sum(sx);
        if (lane == 0) {
            s_w[k][wave] = nk;
            s_w[K + k][wave] = sx;
        }
    }
    __syncthreads();
    for (int j = tid; j < 2 * K + 1; j += GM_THREADS) {
        double total = s_w[j][0];
#pragma unroll
        for (int w = 1; w < GM_WAVES; ++w) total = total + s_w[j][w];
        part[(int64_t)j * G + blockIdx.x] = total;
    }
}

// the sum of item j over the G workgroups, by the wave that owns it: lane l adds workgroups l, l + 64, ..., then a butterfly
__device__ __forceinline__ double item_sum(const double* __restrict__ part, int64_t G, int j, int lane) {
#pragma clang fp contract(off)
    double v = 0.0;
    for (int64_t g = lane; g < G; g += gte::kWave) v = v + part[(int64_t)j * G + g];
    return wave_sum(v);
}

// ---- finalise A: nk, means, sum lse -> small = (nk [64], mean [64], sum lse) ------------------------------------------------------------
__global__ void __launch_bounds__(GM_THREADS)
gmm_finalise_a_kernel(const double* __restrict__ part, int64_t G, int K, double* __restrict__ small, const double* __restrict__ state,
                      int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;
    __shared__ double s_tot[2 * GM_MAX_K + 1];
    const int tid = threadIdx.x, lane = tid & (gte::kWave - 1), wave = tid / gte::kWave;
    for (int j = wave; j < 2 * K + 1; j += GM_WAVES) {                   // (uniform per wave)
        const double total = item_sum(part, G, j, lane);
        if (lane == 0) s_tot[j] = total;
    }
    __syncthreads();
    if (tid < K) {
        const double nk = s_tot[tid] + 10.0 * GM_EPS;
        small[tid] = nk;
        small[GM_MAX_K + tid] = s_tot[K + tid] / nk;
    }
    if (tid == 0) small[2 * GM_MAX_K] = s_tot[2 * K];
}

// ---- pass B: partials of sum resp * (x - mean)^2 around the NEW means, resp from the OLD parameters ------------------------------------
__global__ void __launch_bounds__(GM_THREADS)
gmm_pass_b_kernel(const double* __restrict__ x, int64_t n, int K, const double* __restrict__ P, int hard, const double* __restrict__ lse_in,
                  const int32_t* __restrict__ label_in, const double* __restrict__ small, double* __restrict__ part_cov,
                  const double* __restrict__ state, int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;
    __shared__ CompTable t;
    __shared__ double s_mean[GM_MAX_K];
    __shared__ double s_w[GM_MAX_K][GM_WAVES];
    const int tid = threadIdx.x, lane = tid & (gte::kWave - 1), wave = tid / gte::kWave;
    const int64_t G = gridDim.x;
    load_components(P, K, t);
    if (tid < K) s_mean[tid] = small[GM_MAX_K + tid];
    double xs[GM_LANE_SAMPLES], lse[GM_LANE_SAMPLES];
    int label[GM_LANE_SAMPLES];
    bool valid[GM_LANE_SAMPLES];
    load_samples(x, n, xs, valid);
    const int64_t base = (int64_t)blockIdx.x * GM_WG_SAMPLES + tid;
#pragma unroll
    for (int s = 0; s < GM_LANE_SAMPLES; ++s) {
        const int64_t i = base + (int64_t)s * GM_THREADS;
        lse[s] = valid[s] ? lse_in[i] : 0.0;
        label[s] = valid[s] && hard ? label_in[i] : 0;
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const double mean = s_mean[k];
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < GM_LANE_SAMPLES; ++s) {
            double r;
            if (hard) r = label[s] == k ? 1.0 : 0.0;
            else r = exp(wlp_of(xs[s], t, k) - lse[s]);
            if (!valid[s]) r = 0.0;
            const double d = xs[s] - mean;
            acc = acc + (r * d) * d;
        }
        acc = wave_sum(acc);
        if (lane == 0) s_w[k][wave] = acc;
    }
    __syncthreads();
    if (tid < K) {
        double total = s_w[tid][0];
#pragma unroll
        for (int w = 1; w < GM_WAVES; ++w) total = total + s_w[tid][w];
        part_cov[(int64_t)tid * G + blockIdx.x] = total;
    }
}

// ---- finalise B: covariances, pc, weights into P; lower bound and the stop into the state -----------------------------------------------
__global__ void __launch_bounds__(GM_THREADS)
gmm_finalise_b_kernel(const double* __restrict__ part_cov, int64_t G, int K, int64_t n, int hard, double tol, double reg_covar,
                      const double* __restrict__ small, double* __restrict__ P, double* state, int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;
    __shared__ double s_tot[GM_MAX_K];
    __shared__ double s_nk[GM_MAX_K];
    __shared__ int s_bad[GM_MAX_K];
    __shared__ double s_wsum;
    const int tid = threadIdx.x, lane = tid & (gte::kWave - 1), wave = tid / gte::kWave;
    for (int k = wave; k < K; k += GM_WAVES) {
        const double total = item_sum(part_cov, G, k, lane);
        if (lane == 0) s_tot[k] = total;
    }
    __syncthreads();                                                     // every lane has read the state
    if (tid < K) {
        const double nk = small[tid];
        const double cov = s_tot[tid] / nk + reg_covar;
        s_nk[tid] = nk;
        s_bad[tid] = !(cov > 0.0) || !(cov < INFINITY);
        P[K + tid] = small[GM_MAX_K + tid];
        P[2 * K + tid] = cov;
        P[3 * K + tid] = 1.0 / sqrt(cov);
    }
    __syncthreads();
    if (tid == 0) {
        double wsum = s_nk[0];
        int bad = s_bad[0];
        for (int k = 1; k < K; ++k) {
            wsum = wsum + s_nk[k];
            bad |= s_bad[k];
        }
        s_wsum = hard ? (double)n : wsum;
        const double prev = state[ST_LB];
        const double lb = small[2 * GM_MAX_K] / (double)n;
        const double change = lb - prev;
        state[ST_PREV] = prev;
        state[ST_LB] = lb;
        state[ST_CHANGE] = change;
        state[ST_IT] = state[ST_IT] + 1.0;
        if (bad) {
            state[ST_ERROR] = 1.0;
            state[ST_STOPPED] = 1.0;
        } else if (fabs(change) < tol) {
            state[ST_CONVERGED] = 1.0;
            state[ST_STOPPED] = 1.0;
        }
    }
    __syncthreads();
    if (tid < K) P[tid] = s_nk[tid] / s_wsum;
}

// ---- the E step alone ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GM_THREADS)
gmm_posterior_kernel(const double* __restrict__ x, int64_t m, int K, const double* __restrict__ P, double* __restrict__ resp,
                     double* __restrict__ lse_out, int32_t* __restrict__ label_out) {
#pragma clang fp contract(off)
    __shared__ CompTable t;
    load_components(P, K, t);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
    if (i >= m) return;
    double xs[1] = {x[i]}, lse[1];
    int label[1];
    e_step<1>(xs, t, K, label_out != nullptr, lse, label);
    if (lse_out) lse_out[i] = lse[0];
    if (label_out) label_out[i] = label[0];
    if (resp)
        for (int k = 0; k < K; ++k) resp[i * K + k] = exp(wlp_of(xs[0], t, k) - lse[0]);
}

int64_t groups(int64_t n) { return gte::ceil_div(n, GM_WG_SAMPLES); }
int64_t lse_bytes(int64_t n) { return gte::round_up(n * 8, GM_ALIGN); }
int64_t label_bytes(int64_t n) { return gte::round_up(n * 4, GM_ALIGN); }
int64_t part_a_bytes(int64_t n, int K) { return gte::round_up((2 * (int64_t)K + 1) * groups(n) * 8, GM_ALIGN); }
int64_t part_b_bytes(int64_t n, int K) { return gte::round_up((int64_t)K * groups(n) * 8, GM_ALIGN); }
int64_t small_bytes() { return gte::round_up((2 * GM_MAX_K + 1) * 8, GM_ALIGN); }

}  // namespace

extern "C" int gte_gmm_max_components(void) { return GM_MAX_K; }
extern "C" int gte_gmm_workgroup_samples(void) { return GM_WG_SAMPLES; }

extern "C" int64_t gte_gmm_workspace_bytes(int64_t n, int K) {
    if (n < 1 || n > INT32_MAX || K < 1 || K > GM_MAX_K) return 0;
    return lse_bytes(n) + label_bytes(n) + part_a_bytes(n, K) + part_b_bytes(n, K) + small_bytes();
}

extern "C" int gte_gmm_iterate(const double* x, int64_t n, int K, double* P, int hard, double tol, double reg_covar, int max_iter,
                               int n_iters, void* workspace, int64_t workspace_bytes, double* state, void* stream) {
    if (n < 1 || K < 1 || K > GM_MAX_K || max_iter < 1 || n_iters < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "gmm_iterate: bad sizes (n %lld, K %d of 1 .. %d, max_iter %d, n_iters %d)", (long long)n,
                         K, GM_MAX_K, max_iter, n_iters);
    if (!(tol >= 0.0) || !(reg_covar >= 0.0) || !(reg_covar < INFINITY))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "gmm_iterate: tol %g and reg_covar %g must be >= 0", tol, reg_covar);
    if (n > INT32_MAX) return gte::fail(GTE_ERR_UNSUPPORTED, "gmm_iterate: n %lld (limit 2^31 - 1)", (long long)n);
    if (!x || !P || !workspace || !state) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "gmm_iterate: null pointer");
    if ((((uintptr_t)x | (uintptr_t)P | (uintptr_t)workspace | (uintptr_t)state) & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "gmm_iterate: float64 arrays, the workspace and the state must be 8-byte aligned");
    const int64_t need = gte_gmm_workspace_bytes(n, K);
    if (workspace_bytes < need)
        return gte::fail(GTE_ERR_WORKSPACE_TOO_SMALL, "gmm_iterate: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                         (long long)need);
    if (n_iters == 0) return GTE_OK;
    char* ws = static_cast<char*>(workspace);
    double* lse = reinterpret_cast<double*>(ws);
    int32_t* label = reinterpret_cast<int32_t*>(ws + lse_bytes(n));
    double* part_a = reinterpret_cast<double*>(ws + lse_bytes(n) + label_bytes(n));
    double* part_b = reinterpret_cast<double*>(ws + lse_bytes(n) + label_bytes(n) + part_a_bytes(n, K));
    double* small = reinterpret_cast<double*>(ws + lse_bytes(n) + label_bytes(n) + part_a_bytes(n, K) + part_b_bytes(n, K));
    const int64_t G = groups(n);
    hipStream_t st = gte::as_stream(stream);
    for (int s = 0; s < n_iters; ++s) {
        hipLaunchKernelGGL(gmm_pass_a_kernel, dim3((unsigned)G), dim3(GM_THREADS), 0, st, x, n, K, (const double*)P, hard != 0, lse, label,
                           part_a, (const double*)state, max_iter);
        hipLaunchKernelGGL(gmm_finalise_a_kernel, dim3(1), dim3(GM_THREADS), 0, st, (const double*)part_a, G, K, small,
                           (const double*)state, max_iter);
        hipLaunchKernelGGL(gmm_pass_b_kernel, dim3((unsigned)G), dim3(GM_THREADS), 0, st, x, n, K, (const double*)P, hard != 0,
                           (const double*)lse, (const int32_t*)label, (const double*)small, part_b, (const double*)state, max_iter);
        hipLaunchKernelGGL(gmm_finalise_b_kernel, dim3(1), dim3(GM_THREADS), 0, st, (const double*)part_b, G, K, n, hard != 0, tol,
                           reg_covar, (const double*)small, P, state, max_iter);
    }
    return gte::check_launch("gmm_iterate");
}

extern "C" int gte_gmm_posterior(const double* x, int64_t m, int K, const double* P, double* resp, double* lse, int32_t* label,
                                 void* stream) {
    if (m < 1 || K < 1 || K > GM_MAX_K)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "gmm_posterior: bad sizes (m %lld, K %d of 1 .. %d)", (long long)m, K, GM_MAX_K);
    if (m > INT32_MAX) return gte::fail(GTE_ERR_UNSUPPORTED, "gmm_posterior: m %lld (limit 2^31 - 1)", (long long)m);
    if (!x || !P) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "gmm_posterior: null pointer");
    if (!resp && !lse && !label) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "gmm_posterior: no output asked for");
    if ((((uintptr_t)x | (uintptr_t)P | (uintptr_t)resp | (uintptr_t)lse) & 7) != 0 || ((uintptr_t)label & 3) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "gmm_posterior: float64 arrays must be 8-byte aligned, label 4-byte");
    hipLaunchKernelGGL(gmm_posterior_kernel, dim3((unsigned)gte::ceil_div(m, GM_THREADS)), dim3(GM_THREADS), 0, gte::as_stream(stream), x, m,
                       K, P, resp, lse, label);
    return gte::check_launch("gmm_posterior");
}
