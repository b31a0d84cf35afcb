// ReLU + row L2-normalise (torch.nn.functional.normalize(relu?(z), p=2, dim=1, eps)), forward and backward: what follows every
// hidden layer of MeanSAGE (models.py:166-168 of the reference).
//
// Forward, per row:   r = relu ? max(z, 0) : z ;  s = sqrt(sum r^2) ;  y = r / max(s, eps) ;  norm[row] = s (unclamped).
// Backward, per row:  d = max(s, eps) ;  proj = s >= eps ? sum y dy : 0   (clamp_min passes no gradient into a clamped norm) ;
//                     dr = (dy - y proj) / d ;  dz = relu ? (y > 0 ? dr : 0) : dr   (a select: dr may be huge when d = eps) ;
//                     dbias[c] = sum over the rows of dz[.][c].
//
// One wave64 per row, four rows per 256-thread workgroup; the row sums are DPP butterflies inside the wave (gte_group_sum<64>).
// Rows of up to 1024 columns are read ONCE and stay in registers; wider rows are read twice (the second read hits L1 / L2).
// Lane l owns the columns VW (l + 64 t) .. + VW - 1: VW = 4 (16-byte accesses) when every base pointer is 16-byte aligned and
// every leading dimension and n_out are multiples of 4, VW = 1 otherwise.  Columns beyond n_out are neither read nor written.
// Both directions work in place (y == z, dz == dy): a lane reads an element before it writes it and nobody else touches it.
// HBM-bound: forward 2 M n 4 bytes, backward 3 M n 4 bytes (+ 4 M for the norms).
//
// dbias never touches atomics: every wave keeps the sums of its columns over the rows it owns in registers, the four waves of a
// workgroup are folded through LDS in a fixed order into partial[workgroup][n_out] (the caller's workspace) and a second launch
// folds the <= L2N_MAX_BLOCKS partial rows in a fixed order.  Rows wider than 1024 take the column sums from the finished dz in
// a pass of their own (same partial layout, same fold).  The result is deterministic.
#include "gte_common.h"

namespace {

constexpr int L2N_REG_COLS = 1024;        // widest row kept in registers: 16 floats per lane
constexpr int L2N_MAX_BLOCKS = 512;       // workgroups of the backward = rows of the column-sum partials
constexpr int64_t L2N_MAX_COLS = 1 << 30; // (the column index of the re-reading loops is an int that steps by 256)

struct __attribute__((aligned(16))) f4a { float x, y, z, w; };

template <int VW>
__device__ __forceinline__ void l2n_load(const float* p, float (&v)[VW]) {
    if constexpr (VW == 4) {
        const f4a t = *reinterpret_cast<const f4a*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int VW>
__device__ __forceinline__ void l2n_store(float* p, const float (&v)[VW]) {
    if constexpr (VW == 4) {
        f4a t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *reinterpret_cast<f4a*>(p) = t;
    } else {
        *p = v[0];
    }
}

// NaN stays NaN, as torch.relu keeps it
__device__ __forceinline__ float l2n_relu(float v, int relu) { return (relu && v < 0.f) ? 0.f : v; }

__device__ __forceinline__ float l2n_dz(float gy, float yv, float proj, float inv, int relu) {
    const float dr = (gy - yv * proj) * inv;
    return relu ? (yv > 0.f ? dr : 0.f) : dr;
}

// ------------------------------- forward --------------------------------------------------------------------------------------
template <int VW, int NCH>                 // n <= VW * 64 * NCH: the whole row in registers
__global__ void __launch_bounds__(256)
relu_l2norm_fwd_kernel(const float* z, int64_t ldz, int relu, float eps, float* y, int64_t ldy, float* __restrict__ norm, int M,
                       int n) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* zr = z + row * ldz;
    float* yr = y + row * ldy;
    float c[NCH][VW];
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        const int j = VW * (lane + 64 * t);
#pragma unroll
        for (int e = 0; e < VW; ++e) c[t][e] = 0.f;
        if (j < n) l2n_load<VW>(zr + j, c[t]);              // (VW == 4: n % 4 == 0, the vector is whole)
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            c[t][e] = l2n_relu(c[t][e], relu);
            q = fmaf(c[t][e], c[t][e], q);
        }
    }
    const float s = sqrtf(gte_group_sum<64>(q));
    const float d = fmaxf(s, eps);
    if (norm && lane == 0) norm[row] = s;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        const int j = VW * (lane + 64 * t);
        if (j < n) {
            float o[VW];
#pragma unroll
            for (int e = 0; e < VW; ++e) o[e] = c[t][e] / d;
            l2n_store<VW>(yr + j, o);
        }
    }
}

template <int VW>                          // any width: the row is read twice
__global__ void __launch_bounds__(256)
relu_l2norm_fwd_wide_kernel(const float* z, int64_t ldz, int relu, float eps, float* y, int64_t ldy, float* __restrict__ norm,
                            int M, int n) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* zr = z + row * ldz;
    float* yr = y + row * ldy;
    float q = 0.f;
    for (int j = VW * lane; j < n; j += 64 * VW) {
        float v[VW];
        l2n_load<VW>(zr + j, v);
#pragma unroll
        for (int e = 0; e < VW; ++e) { v[e] = l2n_relu(v[e], relu); q = fmaf(v[e], v[e], q); }
    }
    const float s = sqrtf(gte_group_sum<64>(q));
    const float d = fmaxf(s, eps);
    if (norm && lane == 0) norm[row] = s;
    for (int j = VW * lane; j < n; j += 64 * VW) {
        float v[VW];
        l2n_load<VW>(zr + j, v);
#pragma unroll
        for (int e = 0; e < VW; ++e) v[e] = l2n_relu(v[e], relu) / d;
        l2n_store<VW>(yr + j, v);
    }
}

// ------------------------------- backward -------------------------------------------------------------------------------------
template <int VW, int NCH>                 // n <= VW * 64 * NCH; partial == nullptr: no column sums
__global__ void __launch_bounds__(256)
relu_l2norm_bwd_kernel(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* __restrict__ norm, int relu,
                       float eps, float* dz, int64_t lddz, float* __restrict__ partial, int M, int n) {
    constexpr int W = VW * 64 * NCH;
    __shared__ __attribute__((aligned(16))) float red[4 * W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float sb[NCH][VW];
#pragma unroll
    for (int t = 0; t < NCH; ++t)
#pragma unroll
        for (int e = 0; e < VW; ++e) sb[t][e] = 0.f;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {
        const float* gr = dy + row * lddy;
        const float* yr = y + row * ldy;
        float* dr = dz + row * lddz;
        float g[NCH][VW], yv[NCH][VW];
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < NCH; ++t) {
            const int j = VW * (lane + 64 * t);
#pragma unroll
            for (int e = 0; e < VW; ++e) g[t][e] = yv[t][e] = 0.f;
            if (j < n) { l2n_load<VW>(gr + j, g[t]); l2n_load<VW>(yr + j, yv[t]); }
#pragma unroll
            for (int e = 0; e < VW; ++e) a = fmaf(yv[t][e], g[t][e], a);
        }
        const float s = norm[row];
        const float inv = 1.0f / fmaxf(s, eps);
        const float proj = s >= eps ? gte_group_sum<64>(a) : 0.f;        // (wave-uniform)
#pragma unroll
        for (int t = 0; t < NCH; ++t) {
            const int j = VW * (lane + 64 * t);
            if (j < n) {
                float o[VW];
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    o[e] = l2n_dz(g[t][e], yv[t][e], proj, inv, relu);
                    sb[t][e] += o[e];
                }
                l2n_store<VW>(dr + j, o);
            }
        }
    }
    if (partial) {                                                       // (uniform over the grid)
#pragma unroll
        for (int t = 0; t < NCH; ++t)
#pragma unroll
            for (int e = 0; e < VW; ++e) red[wave * W + VW * (lane + 64 * t) + e] = sb[t][e];
        __syncthreads();
        float* pp = partial + (int64_t)blockIdx.x * n;
        for (int j = threadIdx.x; j < n; j += 256) pp[j] = (red[j] + red[W + j]) + (red[2 * W + j] + red[3 * W + j]);
    }
}

template <int VW>                          // any width: dy and y are read twice, no column sums here
__global__ void __launch_bounds__(256)
relu_l2norm_bwd_wide_kernel(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* __restrict__ norm, int relu,
                            float eps, float* dz, int64_t lddz, int M, int n) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* gr = dy + row * lddy;
    const float* yr = y + row * ldy;
    float* dr = dz + row * lddz;
    float a = 0.f;
    for (int j = VW * lane; j < n; j += 64 * VW) {
        float g[VW], yv[VW];
        l2n_load<VW>(gr + j, g);
        l2n_load<VW>(yr + j, yv);
#pragma unroll
        for (int e = 0; e < VW; ++e) a = fmaf(yv[e], g[e], a);
    }
    const float s = norm[row];
    const float inv = 1.0f / fmaxf(s, eps);
    const float proj = s >= eps ? gte_group_sum<64>(a) : 0.f;
    for (int j = VW * lane; j < n; j += 64 * VW) {
        float g[VW], yv[VW];
        l2n_load<VW>(gr + j, g);
        l2n_load<VW>(yr + j, yv);
#pragma unroll
        for (int e = 0; e < VW; ++e) g[e] = l2n_dz(g[e], yv[e], proj, inv, relu);
        l2n_store<VW>(dr + j, g);
    }
}

// column sums of a finished matrix, first stage (wide rows): workgroup (bx, by) sums the rows by * 4 + wave, + 4 gridDim.y, ... of
// the 64 columns bx * 64 .. into partial[by][.]
__global__ void __launch_bounds__(256)
l2n_colsum_partial_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ partial, int M, int n) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (j < n)
        for (int64_t row = (int64_t)blockIdx.y * 4 + wave; row < M; row += (int64_t)gridDim.y * 4) s += x[row * ldx + j];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && j < n) partial[(int64_t)blockIdx.y * n + j] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// second stage: out[j] = sum over the nblocks partial rows, fixed order (64 columns x 16 slices of the row list per workgroup)
__global__ void __launch_bounds__(1024)
l2n_colsum_fold_kernel(const float* __restrict__ partial, int nblocks, int n, float* __restrict__ out) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    float a = 0.f;
    if (j < n) {
#pragma unroll 4
        for (int k = slice; k < nblocks; k += 16) a += partial[(int64_t)k * n + j];
    }
    red[slice][lane] = a;
    __syncthreads();
    if (slice == 0 && j < n) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[k][lane];
        out[j] = s;
    }
}

int l2n_bwd_blocks(int64_t M) {
    const int64_t b = gte::ceil_div(M, 4);
    return (int)(b < L2N_MAX_BLOCKS ? b : L2N_MAX_BLOCKS);
}

bool l2n_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int gte_relu_l2norm_fwd(const float* z, int64_t ldz, int relu, float eps, float* y, int64_t ldy, float* norm, int64_t M,
                                   int64_t n_out, void* stream) {
    if (M < 0 || n_out <= 0 || M > INT32_MAX || n_out > L2N_MAX_COLS)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "relu_l2norm_fwd: bad sizes");
    if (!(eps > 0.f)) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "relu_l2norm_fwd: eps must be positive");
    if (M == 0) return GTE_OK;
    if (!z || !y) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "relu_l2norm_fwd: null pointer");
    if (ldz < n_out || ldy < n_out) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "relu_l2norm_fwd: ld < n_out");
    hipStream_t s = gte::as_stream(stream);
    const bool vec = n_out % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && l2n_aligned16(z) && l2n_aligned16(y);
    const dim3 grid((unsigned)gte::ceil_div(M, 4)), block(256);
#define GTE_L2F(VW, NCH)                                                                                                  \
    hipLaunchKernelGGL((relu_l2norm_fwd_kernel<VW, NCH>), grid, block, 0, s, z, ldz, relu, eps, y, ldy, norm, (int)M, (int)n_out)
    if (n_out > L2N_REG_COLS) {
        if (vec) hipLaunchKernelGGL(relu_l2norm_fwd_wide_kernel<4>, grid, block, 0, s, z, ldz, relu, eps, y, ldy, norm, (int)M, (int)n_out);
        else hipLaunchKernelGGL(relu_l2norm_fwd_wide_kernel<1>, grid, block, 0, s, z, ldz, relu, eps, y, ldy, norm, (int)M, (int)n_out);
    } else if (vec) {
        if (n_out <= 256) GTE_L2F(4, 1); else if (n_out <= 512) GTE_L2F(4, 2); else if (n_out <= 768) GTE_L2F(4, 3); else GTE_L2F(4, 4);
    } else {
        if (n_out <= 64) GTE_L2F(1, 1); else if (n_out <= 128) GTE_L2F(1, 2); else if (n_out <= 256) GTE_L2F(1, 4);
        else if (n_out <= 512) GTE_L2F(1, 8); else GTE_L2F(1, 16);
    }
#undef GTE_L2F
    return gte::check_launch("relu_l2norm_fwd");
}

extern "C" int64_t gte_relu_l2norm_bwd_workspace_bytes(int64_t M, int64_t n_out) {
    return gte::round_up((int64_t)l2n_bwd_blocks(M > 0 ? M : 1) * (n_out > 0 ? n_out : 1) * 4, 256);
}

extern "C" int gte_relu_l2norm_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* norm, int relu, float eps,
                                   float* dz, int64_t lddz, float* dbias, int64_t M, int64_t n_out, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    if (M < 0 || n_out <= 0 || M > INT32_MAX || n_out > L2N_MAX_COLS)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "relu_l2norm_bwd: bad sizes");
    if (!(eps > 0.f)) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "relu_l2norm_bwd: eps must be positive");
    if (M == 0) return GTE_OK;
    if (!dy || !y || !norm || !dz) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "relu_l2norm_bwd: null pointer");
    if (lddy < n_out || ldy < n_out || lddz < n_out) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "relu_l2norm_bwd: ld < n_out");
    if (dbias && (!workspace || workspace_bytes < gte_relu_l2norm_bwd_workspace_bytes(M, n_out)))
        return gte::fail(GTE_ERR_WORKSPACE_TOO_SMALL, "relu_l2norm_bwd: dbias needs %lld workspace bytes, got %lld",
                         (long long)gte_relu_l2norm_bwd_workspace_bytes(M, n_out), (long long)(workspace ? workspace_bytes : 0));
    hipStream_t s = gte::as_stream(stream);
    const bool vec = n_out % 4 == 0 && lddy % 4 == 0 && ldy % 4 == 0 && lddz % 4 == 0 && l2n_aligned16(dy) && l2n_aligned16(y) &&
                     l2n_aligned16(dz);
    const int nb = l2n_bwd_blocks(M);
    float* part = dbias ? reinterpret_cast<float*>(workspace) : nullptr;
    const dim3 grid((unsigned)nb), block(256);
#define GTE_L2B(VW, NCH)                                                                                                     \
    hipLaunchKernelGGL((relu_l2norm_bwd_kernel<VW, NCH>), grid, block, 0, s, dy, lddy, y, ldy, norm, relu, eps, dz, lddz, part, (int)M, \
                       (int)n_out)
    if (n_out > L2N_REG_COLS) {
        const dim3 wgrid((unsigned)gte::ceil_div(M, 4));
        if (vec) hipLaunchKernelGGL(relu_l2norm_bwd_wide_kernel<4>, wgrid, block, 0, s, dy, lddy, y, ldy, norm, relu, eps, dz, lddz, (int)M, (int)n_out);
        else hipLaunchKernelGGL(relu_l2norm_bwd_wide_kernel<1>, wgrid, block, 0, s, dy, lddy, y, ldy, norm, relu, eps, dz, lddz, (int)M, (int)n_out);
        if (part)
            hipLaunchKernelGGL(l2n_colsum_partial_kernel, dim3((unsigned)gte::ceil_div(n_out, 64), (unsigned)nb), block, 0, s, dz, lddz,
                               part, (int)M, (int)n_out);
    } else if (vec) {
        if (n_out <= 256) GTE_L2B(4, 1); else if (n_out <= 512) GTE_L2B(4, 2); else if (n_out <= 768) GTE_L2B(4, 3); else GTE_L2B(4, 4);
    } else {
        if (n_out <= 64) GTE_L2B(1, 1); else if (n_out <= 128) GTE_L2B(1, 2); else if (n_out <= 256) GTE_L2B(1, 4);
        else if (n_out <= 512) GTE_L2B(1, 8); else GTE_L2B(1, 16);
    }
#undef GTE_L2B
    if (part)
        hipLaunchKernelGGL(l2n_colsum_fold_kernel, dim3((unsigned)gte::ceil_div(n_out, 64)), dim3(1024), 0, s, part, nb, (int)n_out, dbias);
    return gte::check_launch("relu_l2norm_bwd");
}
