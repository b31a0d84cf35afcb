// Affinity propagation sweeps on dense float64 [n, n] matrices: the loop of scikit-learn's _affinity_propagation
// (sklearn/cluster/_affinity_propagation.py), which Preprocessor.train_repr of the reference runs on the host through
// src/utils/matrixes.py: affinity().  The contract -- every formula, the order of the column sum, the stop rule -- is the
// definition in include/gte.h; tests/affprop_ref.py (numpy, written from it and pinned on scikit-learn) is the oracle, and parity
// is equality.
//
// Structure.  One sweep is four launches on the caller's stream; nothing is exchanged inside a launch, every hand-off is a
// kernel boundary.
//   rows      one workgroup of 256 lanes per row i: a first pass over t[k] = A[i,k] + S[i,k] keeps (max, first index of it,
//             second max) per lane in ascending k, a wave butterfly and one LDS step merge them (the lower index wins a tie), a
//             second pass writes R.  Any n: both passes are stride loops.
//   colsum    one lane per column adds rows 0 .. n-1 IN ORDER: cs[k] = ((Rp[0,k] + Rp[1,k]) + ...), which is what np.sum(axis=0)
//             computes on a C-contiguous matrix and therefore part of the contract.  The adds are a dependent chain of length n;
//             the loads are not: a workgroup of 256 lanes owns 16 columns and stages tiles of 256 rows through LDS, 16 row loads
//             in flight per lane, the next tile's loads issued before the current tile is summed.  Rp = max(R, 0) off the
//             diagonal is formed on the fly from R, it is never stored in memory.
//   avail     the A update, elementwise: blockIdx.y strides over rows, a lane per column.  The lane of a diagonal entry also
//             writes E[i], the ring slot of this sweep and a flag "node i's ring is uniform".
//   decide    ONE workgroup: K and the number of uniform nodes (integer counts: no order dependence), then the state block
//             {n_iter_done, stopped, converged, K}.
// The stop lives on the device: every kernel reads the state block first and returns untouched when `stopped` is set or max_iter
// sweeps are done, so sweeps enqueued behind the stopping one change nothing and the chunk size of the host loop cannot change a
// bit.  All arithmetic is float64 with contraction off: every product, sum and difference is rounded on its own, as numpy does.
#include "gte_common.h"

namespace {

constexpr int AP_MAX_N = 8192;                        // three n x n float64 matrices: 1.5 GB at the cap
constexpr int AP_MAX_CONV = 256;                      // ring slots (uint8 per node and slot)
constexpr int AP_ROW_THREADS = 256;
constexpr int AP_ROW_WAVES = AP_ROW_THREADS / gte::kWave;
constexpr int AP_CS_THREADS = 256;                    // column sums: lanes per workgroup,
constexpr int AP_CS_COLS = 16;                        //   columns per workgroup (128 contiguous bytes of a row),
constexpr int AP_CS_GROUPS = AP_CS_THREADS / AP_CS_COLS;  // row groups,
constexpr int AP_CS_UNROLL = 16;                      //   independent row loads in flight per lane,
constexpr int AP_CS_TILE = AP_CS_GROUPS * AP_CS_UNROLL;   // rows per LDS tile (256 x 16 doubles = 32 KB)
static_assert(AP_CS_THREADS % AP_CS_COLS == 0 && AP_CS_TILE * AP_CS_COLS * 8 <= 48 * 1024, "the tile fits LDS without an opt-in");
constexpr int AP_AV_THREADS = 256;
constexpr int AP_AV_MAX_ROWS = 65535;                 // gridDim.y
constexpr int AP_DEC_THREADS = 1024;
constexpr int AP_NO_INDEX = 0x7fffffff;

// state block (int32 [4], device memory)
enum { ST_DONE = 0, ST_STOPPED = 1, ST_CONVERGED = 2, ST_K = 3 };

__device__ __forceinline__ bool frozen(const int32_t* state, int max_iter) {
    return state[ST_STOPPED] != 0 || state[ST_DONE] >= max_iter;
}

// (max, first index of the max, max of the rest) of a set of entries; merging two sets: the lower index wins a tie
struct Top2 { double m1; int i1; double m2; };
__device__ __forceinline__ Top2 merge(const Top2& a, const Top2& b) {
    const bool take_b = b.m1 > a.m1 || (b.m1 == a.m1 && b.i1 < a.i1);
    const Top2& w = take_b ? b : a;
    const Top2& l = take_b ? a : b;
    return Top2{w.m1, w.i1, w.m2 > l.m1 ? w.m2 : l.m1};
}

__global__ void __launch_bounds__(AP_ROW_THREADS)
affprop_rows_kernel(const double* __restrict__ S, const double* __restrict__ A, double* __restrict__ R, int n, double d, double omd,
                    const int32_t* __restrict__ state, int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;                                 // (uniform: ahead of every barrier)
    __shared__ double s_m1[AP_ROW_WAVES], s_m2[AP_ROW_WAVES];
    __shared__ int s_i1[AP_ROW_WAVES];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * n;
    const double* __restrict__ s_row = S + base;
    const double* __restrict__ a_row = A + base;
    double* __restrict__ r_row = R + base;

    Top2 t2{-INFINITY, AP_NO_INDEX, -INFINITY};
    for (int k = tid; k < n; k += AP_ROW_THREADS) {                      // ascending k: a later equal entry never replaces i1
        const double t = a_row[k] + s_row[k];
        if (t > t2.m1) {
            t2.m2 = t2.m1;
            t2.m1 = t;
            t2.i1 = k;
        } else if (t > t2.m2) {
            t2.m2 = t;
        }
    }
#pragma unroll
    for (int off = 1; off < gte::kWave; off <<= 1)
        t2 = merge(t2, Top2{__shfl_xor(t2.m1, off, gte::kWave), __shfl_xor(t2.i1, off, gte::kWave), __shfl_xor(t2.m2, off, gte::kWave)});
    if ((tid & (gte::kWave - 1)) == 0) {
        s_m1[tid / gte::kWave] = t2.m1;
        s_i1[tid / gte::kWave] = t2.i1;
        s_m2[tid / gte::kWave] = t2.m2;
    }
    __syncthreads();
    t2 = Top2{s_m1[0], s_i1[0], s_m2[0]};
#pragma unroll
    for (int w = 1; w < AP_ROW_WAVES; ++w) t2 = merge(t2, Top2{s_m1[w], s_i1[w], s_m2[w]});

    const double y = t2.m1, y2 = t2.m2;
    const int arg = t2.i1;
    for (int k = tid; k < n; k += AP_ROW_THREADS) {
        const double fresh = s_row[k] - (k == arg ? y2 : y);
        const double keep = r_row[k] * d;
        const double add = fresh * omd;
        r_row[k] = keep + add;
    }
}

// Rp[i, k] of the contract from R[i, k]
__device__ __forceinline__ double rp_of(double r, bool diagonal) { return diagonal || r > 0.0 ? r : 0.0; }

// A workgroup owns AP_CS_COLS adjacent columns.  Its AP_CS_THREADS lanes form AP_CS_GROUPS row groups of one lane per column; a
// tile is AP_CS_TILE = AP_CS_GROUPS * AP_CS_UNROLL consecutive rows: every lane loads AP_CS_UNROLL of them (independent loads, all
// in flight together), turns them into Rp and puts them into LDS as tile[row][column]; the first AP_CS_COLS lanes then add the
// tile's rows to their column's sum ONE AFTER THE OTHER, in row order.  The loads of tile t + 1 are issued before tile t is summed
// and land while the dependent chain of adds runs.
__global__ void __launch_bounds__(AP_CS_THREADS)
affprop_colsum_kernel(const double* __restrict__ R, double* __restrict__ cs, int n, const int32_t* __restrict__ state, int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;                                 // (uniform: ahead of every barrier)
    __shared__ double s_tile[AP_CS_TILE * AP_CS_COLS];
    const int tid = threadIdx.x;
    const int c = tid % AP_CS_COLS, g = tid / AP_CS_COLS;
    const int k = blockIdx.x * AP_CS_COLS + c;
    const bool live = k < n;
    const double* __restrict__ col = R + (live ? k : 0);
    double v[AP_CS_UNROLL];
    double acc = 0.0;                                                    // (0.0 + x == x: the sum starts at Rp[0, k])

    // row r of the tile that starts at row0 is loaded by group r % AP_CS_GROUPS as its load number r / AP_CS_GROUPS
#define AP_CS_LOAD(row0)                                                                   \
    _Pragma("unroll") for (int u = 0; u < AP_CS_UNROLL; ++u) {                             \
        const int row = (row0) + u * AP_CS_GROUPS + g;                                     \
        v[u] = live && row < n ? col[(int64_t)row * n] : 0.0;                              \
    }
    AP_CS_LOAD(0)
    for (int row0 = 0; row0 < n; row0 += AP_CS_TILE) {
#pragma unroll
        for (int u = 0; u < AP_CS_UNROLL; ++u) {
            const int r = u * AP_CS_GROUPS + g;
            s_tile[r * AP_CS_COLS + c] = rp_of(v[u], row0 + r == k);
        }
        __syncthreads();                                                 // the tile is complete
        if (row0 + AP_CS_TILE < n) { AP_CS_LOAD(row0 + AP_CS_TILE) }     // the next tile's loads: in flight during the adds
        if (tid < AP_CS_COLS) {
            const int rows = min(AP_CS_TILE, n - row0);
#pragma unroll 8
            for (int r = 0; r < rows; ++r) acc = acc + s_tile[r * AP_CS_COLS + c];       // strictly in row order
        }
        __syncthreads();                                                 // the tile has been read: it may be overwritten
    }
#undef AP_CS_LOAD
    if (tid < AP_CS_COLS && live) cs[k] = acc;
}

__global__ void __launch_bounds__(AP_AV_THREADS)
affprop_avail_kernel(const double* __restrict__ R, const double* __restrict__ cs, double* __restrict__ A, int n, double d, double omd,
                     int conv_iter, uint8_t* __restrict__ ring, uint8_t* __restrict__ exemplar, uint8_t* __restrict__ uniform,
                     const int32_t* __restrict__ state, int max_iter) {
#pragma clang fp contract(off)
    if (frozen(state, max_iter)) return;
    const int k = blockIdx.x * AP_AV_THREADS + threadIdx.x;
    if (k >= n) return;                                                  // (no barrier in this kernel)
    const double c = cs[k];
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const int64_t at = (int64_t)i * n + k;
        const double r = R[at];
        double u = rp_of(r, i == k) - c;
        if (i != k && !(u > 0.0)) u = 0.0;
        const double keep = A[at] * d;
        const double sub = u * omd;
        const double fresh = keep - sub;
        A[at] = fresh;
        if (i == k) {
            // the lane of a diagonal entry holds the new A[i,i] and R[i,i]: E[i], its ring slot, and whether node i's ring is uniform
            const int e = (fresh + r) > 0.0 ? 1 : 0;
            const int slot = state[ST_DONE] % conv_iter;
            int sum = e;
            for (int j = 0; j < conv_iter; ++j)
                if (j != slot) sum += ring[(int64_t)j * n + i];
            ring[(int64_t)slot * n + i] = (uint8_t)e;
            exemplar[i] = (uint8_t)e;
            uniform[i] = (sum == conv_iter || sum == 0) ? 1 : 0;
        }
    }
}

__global__ void __launch_bounds__(AP_DEC_THREADS)
affprop_decide_kernel(const uint8_t* __restrict__ exemplar, const uint8_t* __restrict__ uniform, int n, int conv_iter, int max_iter,
                      int32_t* state) {
    __shared__ int s_k, s_uniform;
    const int it = state[ST_DONE];
    if (state[ST_STOPPED] != 0 || it >= max_iter) return;                // (uniform; every lane has read the state by the barrier below)
    if (threadIdx.x == 0) {
        s_k = 0;
        s_uniform = 0;
    }
    __syncthreads();
    int my_k = 0, my_uniform = 0;
    for (int i = threadIdx.x; i < n; i += AP_DEC_THREADS) {
        my_k += exemplar[i];
        my_uniform += uniform[i];
    }
    if (my_k) atomicAdd(&s_k, my_k);
    if (my_uniform) atomicAdd(&s_uniform, my_uniform);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int k = s_k;
        state[ST_DONE] = it + 1;
        state[ST_K] = k;
        if (it >= conv_iter && s_uniform == n && k > 0) {
            state[ST_STOPPED] = 1;
            state[ST_CONVERGED] = 1;
        } else if (it + 1 >= max_iter) {
            state[ST_STOPPED] = 1;                                       // scikit-learn's never_converged
        }
    }
}

constexpr int64_t AP_ALIGN = 256;
int64_t cs_bytes(int64_t n) { return gte::round_up(n * 8, AP_ALIGN); }
int64_t ring_bytes(int64_t n, int conv_iter) { return gte::round_up(n * (int64_t)conv_iter, AP_ALIGN); }

}  // namespace

extern "C" int gte_affprop_max_n(void) { return AP_MAX_N; }
extern "C" int gte_affprop_max_convergence_iter(void) { return AP_MAX_CONV; }

extern "C" int64_t gte_affprop_workspace_bytes(int64_t n, int convergence_iter) {
    if (n < 0 || convergence_iter < 1) return 0;
    return cs_bytes(n) + ring_bytes(n, convergence_iter) + gte::round_up(n, AP_ALIGN);         // column sums, ring, uniform flags
}

extern "C" int gte_affprop_iterate(const double* S, double* A, double* R, int64_t n, double damping, double one_minus_damping,
                                   int convergence_iter, int max_iter, int n_sweeps, uint8_t* exemplar, void* workspace,
                                   int64_t workspace_bytes, int32_t* state, void* stream) {
    if (n < 0 || convergence_iter < 1 || max_iter < 1 || n_sweeps < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "affprop: bad sizes (n %lld, convergence_iter %d, max_iter %d, n_sweeps %d)",
                         (long long)n, convergence_iter, max_iter, n_sweeps);
    if (!(damping >= 0.0 && damping <= 1.0) || !(one_minus_damping >= 0.0 && one_minus_damping <= 1.0))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "affprop: damping %g and 1 - damping %g must lie in [0, 1]", damping, one_minus_damping);
    if (n > AP_MAX_N || convergence_iter > AP_MAX_CONV)
        return gte::fail(GTE_ERR_UNSUPPORTED, "affprop: n %lld, convergence_iter %d (limits %d, %d)", (long long)n, convergence_iter,
                         AP_MAX_N, AP_MAX_CONV);
    if (n == 0 || n_sweeps == 0) return GTE_OK;
    if (!S || !A || !R || !exemplar || !workspace || !state) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "affprop: null pointer");
    if ((((uintptr_t)S | (uintptr_t)A | (uintptr_t)R | (uintptr_t)workspace) & 7) != 0 || ((uintptr_t)state & 3) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "affprop: float64 arrays and the workspace must be 8-byte aligned, the state 4-byte");
    const int64_t need = gte_affprop_workspace_bytes(n, convergence_iter);
    if (workspace_bytes < need)
        return gte::fail(GTE_ERR_WORKSPACE_TOO_SMALL, "affprop: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);

    double* cs = static_cast<double*>(workspace);
    uint8_t* ring = static_cast<uint8_t*>(workspace) + cs_bytes(n);
    uint8_t* uniform = ring + ring_bytes(n, convergence_iter);
    const int ni = (int)n;
    hipStream_t st = gte::as_stream(stream);
    const dim3 av_grid((unsigned)gte::ceil_div(n, AP_AV_THREADS), (unsigned)(ni < AP_AV_MAX_ROWS ? ni : AP_AV_MAX_ROWS));
    for (int s = 0; s < n_sweeps; ++s) {
        hipLaunchKernelGGL(affprop_rows_kernel, dim3((unsigned)ni), dim3(AP_ROW_THREADS), 0, st, S, A, R, ni, damping, one_minus_damping,
                           state, max_iter);
        hipLaunchKernelGGL(affprop_colsum_kernel, dim3((unsigned)gte::ceil_div(n, AP_CS_COLS)), dim3(AP_CS_THREADS), 0, st, R, cs, ni,
                           state, max_iter);
        hipLaunchKernelGGL(affprop_avail_kernel, av_grid, dim3(AP_AV_THREADS), 0, st, R, cs, A, ni, damping, one_minus_damping,
                           convergence_iter, ring, exemplar, uniform, state, max_iter);
        hipLaunchKernelGGL(affprop_decide_kernel, dim3(1), dim3(AP_DEC_THREADS), 0, st, exemplar, uniform, ni, convergence_iter,
                           max_iter, state);
    }
    return gte::check_launch("affprop");
}
