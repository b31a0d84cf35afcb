// Stand-alone LayerNorm(+ReLU) of GcnSAGELayer on gfx950: forward, backward and the column sums of the backward.
//
// replaces (reference src/components/graphs/models.py):
//   :64-66  nn.LayerNorm(out) + activation  -> row-wise kernels (one wave per node row) and their autograd, with the column sums
//                                              for dgamma / dbeta / dbias
// where no producer carries them as an epilogue (gemm_p3.hip, narrow_layer.hip, spmm_csr.hip, the short-K layer of sage_linear.hip
// do; the device arithmetic they share with this file is in layernorm.h).
//
// Roofline: HBM.  Forward: reads z, writes y (+ 6 bytes per value of a P3 image); backward: reads dy and z, writes dz (+ image).
//
// Kernels                                      rows x columns of a lane                      entry points
//   ln_relu_fwd_kernel                         columns l + 64 t, any width                   gte_ln_relu_fwd
//   ln_relu_fwd_vec_kernel<NV, RF, MSK>        16 bytes: columns 4 (l + 64 v) .. + 3         gte_ln_relu_fwd (!MSK), gte_ln_relu_fwd_p3 (MSK)
//   ln_relu_bwd_kernel<NCH>                    columns l + 64 t, n <= 1024                   gte_ln_relu_bwd
//   ln_relu_bwd_vec_kernel<NV>                 16 bytes: columns 4 (l + 64 v) .. + 3         gte_ln_relu_bwd(_p3) at n % 4 (16) == 0 in 128 .. 512
//   ln_relu_bwd_gen_kernel<NV, RF>             the same on padded rows, any n <= 1024         gte_ln_relu_bwd_p3 elsewhere
//   ln_relu_bwd_wide_kernel                    columns l + 64 t, n > 1024                    gte_ln_relu_bwd
//   colsum_fold_kernel                         the block partials of any backward kernel -> dgamma, dbeta, dbias
// The 16-byte forward is ONE body for every width it runs.  !MSK: n % 4 == 0, a chunk of four columns is valid or not as a whole.
// MSK: any n on rows padded to a multiple of 4 floats, per-element validity, columns n .. up to the next multiple of 4 of the fp32
// output and up to the next multiple of 16 of the P3 image are written as zeros.  The 16-byte backward keeps the same two forms as
// two kernels (vec, gen: merged, one instantiation measured slower per launch).  Both forms compute the same bits wherever both can
// run a width (tests/test_gpu_layernorm.py holds the plain and the image entry points together).  The scalar kernels sum a row in
// another order and leave contraction to the compiler: their bits differ from the 16-byte family by design.
#include "gte_common.h"
#include "layernorm.h"
#include "p3.h"

namespace {

using namespace gte_ln;

// ------------------------------- LayerNorm + ReLU, forward ----------------------------------------
// y = relu?( gamma * (z - mean) * rstd + beta ); one wave per row, two-pass mean/variance (biased
// variance, eps inside the sqrt: torch.nn.LayerNorm).  In place (y == z) is allowed.
constexpr int LN_CACHE = 16;      // elements per lane kept in registers -> rows up to 1024 wide

__global__ void __launch_bounds__(256)
ln_relu_fwd_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ gamma,
                   const float* __restrict__ beta, float eps, int relu, float* __restrict__ y, int64_t ldy,
                   float* __restrict__ stats, int M, int n) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* zr = z + (int64_t)row * ldz;
    float* yr = y + (int64_t)row * ldy;
    float c[LN_CACHE];
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < LN_CACHE; ++t) {
        const int j = lane + 64 * t;
        c[t] = j < n ? zr[j] : 0.f;
        s += c[t];
    }
    for (int j = lane + 64 * LN_CACHE; j < n; j += 64) s += zr[j];
    const float mean = wave_sum(s) / (float)n;
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < LN_CACHE; ++t) {
        const int j = lane + 64 * t;
        const float d = j < n ? c[t] - mean : 0.f;
        q = fmaf(d, d, q);
    }
    for (int j = lane + 64 * LN_CACHE; j < n; j += 64) { const float d = zr[j] - mean; q = fmaf(d, d, q); }
    const float rstd = rsqrtf(wave_sum(q) / (float)n + eps);
    if (stats && lane == 0) { stats[row] = mean; stats[M + row] = rstd; }
#pragma unroll
    for (int t = 0; t < LN_CACHE; ++t) {
        const int j = lane + 64 * t;
        if (j < n) {
            float v = ln_affine((c[t] - mean) * rstd, gamma[j], beta[j]);
            if (relu) v = fmaxf(v, 0.f);
            yr[j] = v;
        }
    }
    for (int j = lane + 64 * LN_CACHE; j < n; j += 64) {
        float v = ln_affine((zr[j] - mean) * rstd, gamma[j], beta[j]);
        if (relu) v = fmaxf(v, 0.f);
        yr[j] = v;
    }
}

// 16-byte accesses, RF rows in flight per wave: lane l owns columns 4 (l + 64 v) .. + 3, v < NV (n <= 256 NV).  Same two-pass
// statistics.  (The scalar version above moves 4 bytes per lane per instruction: 13.9 us for 50 MB, a plain device copy of the same
// bytes takes 8.3 us on this chip.)  Any width up to 1024 (the reference's own run shapes: hidden 1000, or int(calculate_hidden) =
// 96 ... 218) runs the MSK form, which writes y as fp32 (nullable) and / or as a P3 image (nullable); the !MSK form writes y alone.
template <int NV, int RF, bool MSK>
__global__ void __launch_bounds__(256)
ln_relu_fwd_vec_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ gamma, const float* __restrict__ beta,
                       float eps, int relu, float* __restrict__ y, int64_t ldy, char* __restrict__ yp3, int64_t ldyp3,
                       float* __restrict__ stats, int M, int n) {
    const int lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RF;
    if (row0 >= M) return;
    const int nw = MSK ? (n + 15) & ~15 : n;               // columns written
    float g[NV][4], b[NV][4];
    bool okv[NV], wrv[NV];
    const auto oke = [&](int v, int e) { return MSK ? 4 * (lane + 64 * v) + e < n : okv[v]; };      // column 4 (lane + 64 v) + e is valid
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int j = 4 * (lane + 64 * v);
        okv[v] = j < n;
        wrv[v] = j < nw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            g[v][e] = oke(v, e) ? gamma[j + e] : 0.f;
            b[v][e] = oke(v, e) ? beta[j + e] : 0.f;
        }
    }
    float c[RF][NV][4];
    bool rok[RF];
#pragma unroll
    for (int u = 0; u < RF; ++u) {
        rok[u] = row0 + u < M;
        const int r = rok[u] ? row0 + u : row0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            f4u t{0.f, 0.f, 0.f, 0.f};
            if (okv[v]) t = *reinterpret_cast<const f4u*>(z + (int64_t)r * ldz + 4 * (lane + 64 * v));
            c[u][v][0] = t.x; c[u][v][1] = oke(v, 1) ? t.y : 0.f; c[u][v][2] = oke(v, 2) ? t.z : 0.f; c[u][v][3] = oke(v, 3) ? t.w : 0.f;
        }
    }
    const float inv_n = 1.0f / (float)n;
#pragma unroll
    for (int u = 0; u < RF; ++u) {
        if (!rok[u]) continue;                             // wave-uniform
        const int r = row0 + u;
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) s += c[u][v][e];
        // (z - mean as ONE fused multiply-add of the row sum, written out: hipcc contracts `c - wave_sum(s) * inv_n` this way, and
        // the LayerNorm-forward epilogue of the planes GEMM -- gemm_p3.hip, LNB == 4 -- is held bit for bit to this kernel)
        const float wsum = wave_sum(s);
        const float mean = wsum * inv_n;
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = oke(v, e) ? fmaf(-inv_n, wsum, c[u][v][e]) : 0.f; q = fmaf(d, d, q); }
        const float rstd = rsqrtf(wave_sum(q) * inv_n + eps);
        if (stats && lane == 0) { stats[r] = mean; stats[M + r] = rstd; }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (!wrv[v]) continue;
            const int j = 4 * (lane + 64 * v);
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = ln_affine(fmaf(-inv_n, wsum, c[u][v][e]) * rstd, g[v][e], b[v][e]);
                if (relu) o[e] = fmaxf(o[e], 0.f);
                if (!oke(v, e)) o[e] = 0.f;
            }
            if ((!MSK || y) && okv[v]) {
                f4u t; t.x = o[0]; t.y = o[1]; t.z = o[2]; t.w = o[3];
                *reinterpret_cast<f4u*>(y + (int64_t)r * ldy + j) = t;
            }
            if (MSK && yp3) p3::store4(yp3 + (int64_t)r * ldyp3, j, o[0], o[1], o[2], o[3]);
        }
    }
}

// ------------------------------- LayerNorm + ReLU, backward ---------------------------------------
// Per row: g = relu ? (pre > 0 ? dy : 0) : dy ; dxhat = g*gamma ;
//          dz = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat*xhat))
// Column sums (dgamma = sum g*xhat, dbeta = sum g, dbias = sum dz) never touch atomics: every wave
// keeps its partial sums for its columns in registers over the rows it owns, the four
// waves of a block are folded through LDS, the block writes partial[block][3][n], and a second kernel
// folds the (<= LNB_MAX_BLOCKS) block partials in a fixed order.  HBM-bound: reads dy and z once,
// writes dz once.
constexpr int LNB_MAX_BLOCKS = 512;

// The column partials of a block.  Every wave has left its three sums per column in LDS (red: [4 waves][3][W], W = the columns the
// block's lanes cover); after the barrier the block adds the four waves in wave order and writes partial[block][3][n].  (The kernels
// store their registers to LDS themselves: handing the register arrays to this function by reference made hipcc allocate and
// schedule the (3, 1) and (4, 1) instantiations of ln_relu_bwd_gen_kernel differently, 968 against 1 044 instructions at (4, 1).)
template <int W>
__device__ __forceinline__ void ln_fold_partials(const float* red, float* __restrict__ partial, int n) {
    __syncthreads();
    float* pp = partial + (int64_t)blockIdx.x * 3 * n;
    for (int i = threadIdx.x; i < 3 * W; i += 256) {
        const int q = i / W, j = i - q * W;
        if (j < n) pp[q * n + j] = red[(0 * 3 + q) * W + j] + red[(1 * 3 + q) * W + j] + red[(2 * 3 + q) * W + j] +
                                   red[(3 * 3 + q) * W + j];
    }
}

template <int NCH>                 // row width n <= 64 * NCH, whole row in registers; lane l owns columns l + 64 t
__global__ void __launch_bounds__(256)
ln_relu_bwd_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ z, int64_t ldz,
                   const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                   int relu, float* __restrict__ dz, int64_t lddz, float* __restrict__ partial, int M, int n) {
    extern __shared__ __attribute__((aligned(16))) float red[];      // [4 waves][3][NCH*64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has_ln = gamma != nullptr;
    float gam[NCH], bet[NCH], s_dg[NCH], s_db[NCH], s_dbias[NCH];
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        const int j = lane + 64 * t;
        gam[t] = (has_ln && j < n) ? gamma[j] : 1.f;
        bet[t] = (has_ln && j < n) ? beta[j] : 0.f;
        s_dg[t] = s_db[t] = s_dbias[t] = 0.f;
    }
    const float inv_n = 1.0f / (float)n;
    for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
        const float* dyr = dy + (int64_t)row * lddy;
        const float* zr = z + (int64_t)row * ldz;
        float* dzr = dz + (int64_t)row * lddz;
        float g[NCH], xh[NCH];
        if (has_ln) {
            const float mean = stats[row], rstd = stats[M + row];
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int t = 0; t < NCH; ++t) {
                const int j = lane + 64 * t;
                const bool ok = j < n;
                xh[t] = ok ? (zr[j] - mean) * rstd : 0.f;
                float gv = ok ? dyr[j] : 0.f;
                if (relu && ln_affine(xh[t], gam[t], bet[t]) <= 0.f) gv = 0.f;
                g[t] = gv;
                const float dxh = gv * gam[t];
                a += dxh;
                b = fmaf(dxh, xh[t], b);
            }
            const float c1 = wave_sum(a) * inv_n, c2 = wave_sum(b) * inv_n;
#pragma unroll
            for (int t = 0; t < NCH; ++t) {
                const int j = lane + 64 * t;
                if (j < n) {
                    const float d = rstd * (g[t] * gam[t] - c1 - xh[t] * c2);
                    s_dg[t] = fmaf(g[t], xh[t], s_dg[t]);
                    s_db[t] += g[t];
                    s_dbias[t] += d;
                    dzr[j] = d;
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < NCH; ++t) {
                const int j = lane + 64 * t;
                if (j < n) {
                    float gv = dyr[j];
                    if (relu && zr[j] <= 0.f) gv = 0.f;
                    s_dbias[t] += gv;
                    dzr[j] = gv;
                }
            }
        }
    }
    constexpr int W = NCH * 64;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        red[(wave * 3 + 0) * W + lane + 64 * t] = s_dg[t];
        red[(wave * 3 + 1) * W + lane + 64 * t] = s_db[t];
        red[(wave * 3 + 2) * W + lane + 64 * t] = s_dbias[t];
    }
    ln_fold_partials<W>(red, partial, n);
}

// Same maths with 16-byte accesses: lane l owns columns 4 (l + 64 v) .. + 3, v < NV (n % 4 == 0, n <= 256 NV).  The scalar
// version above moves 4 bytes per lane per instruction (12 memory instructions per 256-wide row): 30 us for the 75 MB
// of a 24 k x 256 layer, 2.5 TB/s; two rows are in flight per wave here.  The row arithmetic is gte_ln_bwd_pre4 / _post4 (layernorm.h),
// shared with the fused backward forms.
template <int NV>
__global__ void __launch_bounds__(256)
ln_relu_bwd_vec_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ z, int64_t ldz,
                       const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                       int relu, float* __restrict__ dz, int64_t lddz, float* __restrict__ partial, int M, int n,
                       char* __restrict__ dzp3 = nullptr, int64_t ldp3 = 0) {
    extern __shared__ __attribute__((aligned(16))) float red[];      // [4 waves][3][NV*256]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has_ln = gamma != nullptr;
    float gam[NV][4], bet[NV][4], s_dg[NV][4], s_db[NV][4], s_dbias[NV][4];
    bool okv[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int j = 4 * (lane + 64 * v);
        okv[v] = j < n;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            gam[v][e] = (has_ln && okv[v]) ? gamma[j + e] : 1.f;
            bet[v][e] = (has_ln && okv[v]) ? beta[j + e] : 0.f;
            s_dg[v][e] = s_db[v][e] = s_dbias[v][e] = 0.f;
        }
    }
    const float inv_n = 1.0f / (float)n;
    const int stride = gridDim.x * 4;
    for (int row = blockIdx.x * 4 + wave; row < M; row += 2 * stride) {
        // two rows per trip: all four 16-byte loads are issued before the first reduction
        float gy[2][NV][4], zz[2][NV][4];
        float mean[2] = {0.f, 0.f}, rstd[2] = {1.f, 1.f};
        bool rok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = row + u * stride;
            rok[u] = r < M;
            const int rc = rok[u] ? r : row;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int j = 4 * (lane + 64 * v);
                f4u a{0.f, 0.f, 0.f, 0.f}, b{0.f, 0.f, 0.f, 0.f};
                if (okv[v]) {
                    a = *reinterpret_cast<const f4u*>(dy + (int64_t)rc * lddy + j);
                    b = *reinterpret_cast<const f4u*>(z + (int64_t)rc * ldz + j);
                }
                gy[u][v][0] = a.x; gy[u][v][1] = a.y; gy[u][v][2] = a.z; gy[u][v][3] = a.w;
                zz[u][v][0] = b.x; zz[u][v][1] = b.y; zz[u][v][2] = b.z; zz[u][v][3] = b.w;
            }
            if (has_ln) { mean[u] = stats[rc]; rstd[u] = stats[M + rc]; }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!rok[u]) continue;                       // wave-uniform
            float* dzr = dz + (int64_t)(row + u * stride) * lddz;
            if (has_ln) {
                float xh[NV][4], g[NV][4];
                float a = 0.f, b = 0.f;
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    gte_ln_bwd_pre4(gy[u][v], zz[u][v], mean[u], rstd[u], gam[v], bet[v], okv[v], relu, xh[v], g[v], a, b);
                const float c1 = wave_sum(a) * inv_n, c2 = wave_sum(b) * inv_n;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    float d[4];
                    gte_ln_bwd_post4(g[v], xh[v], gam[v], rstd[u], c1, c2, okv[v], d, s_dg[v], s_db[v], s_dbias[v]);
                    if (okv[v]) {
                        f4u o; o.x = d[0]; o.y = d[1]; o.z = d[2]; o.w = d[3];
                        *reinterpret_cast<f4u*>(dzr + 4 * (lane + 64 * v)) = o;
                        // ... and as a P3 image: dz is the A operand of the dX and dW planes GEMMs
                        if (dzp3) p3::store4(dzp3 + (int64_t)(row + u * stride) * ldp3, 4 * (lane + 64 * v), d[0], d[1], d[2], d[3]);
                    }
                }
            } else {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    float d[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        d[e] = (relu && zz[u][v][e] <= 0.f) ? 0.f : gy[u][v][e];
                        s_dbias[v][e] += d[e];
                    }
                    if (okv[v]) {
                        f4u o; o.x = d[0]; o.y = d[1]; o.z = d[2]; o.w = d[3];
                        *reinterpret_cast<f4u*>(dzr + 4 * (lane + 64 * v)) = o;
                        if (dzp3) p3::store4(dzp3 + (int64_t)(row + u * stride) * ldp3, 4 * (lane + 64 * v), d[0], d[1], d[2], d[3]);
                    }
                }
            }
        }
    }
    constexpr int W = NV * 256;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * (lane + 64 * v) + e;
            red[(wave * 3 + 0) * W + j] = s_dg[v][e];
            red[(wave * 3 + 1) * W + j] = s_db[v][e];
            red[(wave * 3 + 2) * W + j] = s_dbias[v][e];
        }
    ln_fold_partials<W>(red, partial, n);
}

// ... any width up to 1024 on rows PADDED to a multiple of 4 floats, LayerNorm layers only, RF rows in flight: per-element validity
// instead of the per-chunk validity above; columns n .. up to the next multiple of 4 of dz and up to the next multiple of 16 of its
// P3 image are written as zeros.  The row arithmetic is spelled out here; gte_ln_bwd_pre4m / _post4m (layernorm.h) restate it for the
// fused forms.  Kept apart from the kernel above and off the helpers on purpose: as one template over the helpers, and equally as
// this kernel calling them, hipcc schedules the (4, 1) instantiation differently (906 against 1 044 instructions) and it measured
// slower per launch at 24.3 k x 1000 than this text (profiles/r12/layernorm_split_ab.txt).
template <int NV, int RF>
__global__ void __launch_bounds__(256)
ln_relu_bwd_gen_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ z, int64_t ldz,
                       const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                       int relu, float* __restrict__ dz, int64_t lddz, float* __restrict__ partial, int M, int n,
                       char* __restrict__ dzp3, int64_t ldp3) {
    extern __shared__ __attribute__((aligned(16))) float red[];      // [4 waves][3][NV*256]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n16 = (n + 15) & ~15;
    float gam[NV][4], bet[NV][4], s_dg[NV][4], s_db[NV][4], s_dbias[NV][4];
    bool okv[NV], imv[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int j = 4 * (lane + 64 * v);
        okv[v] = j < n;
        imv[v] = j < n16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            gam[v][e] = j + e < n ? gamma[j + e] : 1.f;
            bet[v][e] = j + e < n ? beta[j + e] : 0.f;
            s_dg[v][e] = s_db[v][e] = s_dbias[v][e] = 0.f;
        }
    }
    const float inv_n = 1.0f / (float)n;
    const int stride = gridDim.x * 4;
    for (int row = blockIdx.x * 4 + wave; row < M; row += RF * stride) {
        float gy[RF][NV][4], zz[RF][NV][4];
        float mean[RF], rstd[RF];
        bool rok[RF];
#pragma unroll
        for (int u = 0; u < RF; ++u) {
            const int r = row + u * stride;
            rok[u] = r < M;
            const int rc = rok[u] ? r : row;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int j = 4 * (lane + 64 * v);
                f4u a{0.f, 0.f, 0.f, 0.f}, b{0.f, 0.f, 0.f, 0.f};
                if (okv[v]) {
                    a = *reinterpret_cast<const f4u*>(dy + (int64_t)rc * lddy + j);
                    b = *reinterpret_cast<const f4u*>(z + (int64_t)rc * ldz + j);
                }
                gy[u][v][0] = a.x; gy[u][v][1] = a.y; gy[u][v][2] = a.z; gy[u][v][3] = a.w;
                zz[u][v][0] = b.x; zz[u][v][1] = b.y; zz[u][v][2] = b.z; zz[u][v][3] = b.w;
            }
            mean[u] = stats[rc]; rstd[u] = stats[M + rc];
        }
#pragma unroll
        for (int u = 0; u < RF; ++u) {
            if (!rok[u]) continue;                       // wave-uniform
            const int64_t r = row + u * stride;
            float xh[NV][4], g[NV][4];
            float a = 0.f, b = 0.f;
            {
#pragma clang fp contract(off)
#pragma unroll
                for (int v = 0; v < NV; ++v)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool ok = 4 * (lane + 64 * v) + e < n;
                        xh[v][e] = ok ? (zz[u][v][e] - mean[u]) * rstd[u] : 0.f;
                        float gv = ok ? gy[u][v][e] : 0.f;
                        if (relu && fmaf(xh[v][e], gam[v][e], bet[v][e]) <= 0.f) gv = 0.f;
                        g[v][e] = gv;
                        const float dxh = gv * gam[v][e];
                        a = a + dxh;
                        b = fmaf(dxh, xh[v][e], b);
                    }
            }
            const float c1 = wave_sum(a) * inv_n, c2 = wave_sum(b) * inv_n;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                if (!imv[v]) continue;
                const int j = 4 * (lane + 64 * v);
                float d[4];
                {
#pragma clang fp contract(off)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float t0 = g[v][e] * gam[v][e];
                        const float t1 = xh[v][e] * c2;
                        d[e] = j + e < n ? rstd[u] * ((t0 - c1) - t1) : 0.f;
                        s_dg[v][e] = fmaf(g[v][e], xh[v][e], s_dg[v][e]);
                        s_db[v][e] = s_db[v][e] + g[v][e];
                        s_dbias[v][e] = s_dbias[v][e] + d[e];
                    }
                }
                if (okv[v]) {
                    f4u o; o.x = d[0]; o.y = d[1]; o.z = d[2]; o.w = d[3];
                    *reinterpret_cast<f4u*>(dz + r * lddz + j) = o;
                }
                if (dzp3) p3::store4(dzp3 + r * ldp3, j, d[0], d[1], d[2], d[3]);
            }
        }
    }
    constexpr int W = NV * 256;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * (lane + 64 * v) + e;
            red[(wave * 3 + 0) * W + j] = s_dg[v][e];
            red[(wave * 3 + 1) * W + j] = s_db[v][e];
            red[(wave * 3 + 2) * W + j] = s_dbias[v][e];
        }
    ln_fold_partials<W>(red, partial, n);
}

// Rows wider than 1024: same maths, the row is re-read from L1/L2 instead of cached in registers, and
// the column partials are produced 64 columns at a time.  dz must not alias dy here.
__global__ void __launch_bounds__(256)
ln_relu_bwd_wide_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ z, int64_t ldz,
                        const float* __restrict__ stats, const float* __restrict__ gamma,
                        const float* __restrict__ beta, int relu, float* __restrict__ dz, int64_t lddz,
                        float* __restrict__ partial, int M, int n) {
    __shared__ float red[3][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has_ln = gamma != nullptr;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const bool jok = j < n;
        const float gj = (has_ln && jok) ? gamma[j] : 1.f;
        const float bj = (has_ln && jok) ? beta[j] : 0.f;
        float s_dg = 0.f, s_db = 0.f, s_dbias = 0.f;
        for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
            const float* dyr = dy + (int64_t)row * lddy;
            const float* zr = z + (int64_t)row * ldz;
            float* dzr = dz + (int64_t)row * lddz;
            if (has_ln) {
                const float mean = stats[row], rstd = stats[M + row];
                float a = 0.f, b = 0.f;
                for (int jj = lane; jj < n; jj += 64) {
                    const float xh = (zr[jj] - mean) * rstd;
                    float g = dyr[jj];
                    if (relu && ln_affine(xh, gamma[jj], beta[jj]) <= 0.f) g = 0.f;
                    const float dxh = g * gamma[jj];
                    a += dxh;
                    b = fmaf(dxh, xh, b);
                }
                const float c1 = wave_sum(a) / (float)n, c2 = wave_sum(b) / (float)n;
                if (jok) {
                    const float xh = (zr[j] - mean) * rstd;
                    float g = dyr[j];
                    if (relu && ln_affine(xh, gj, bj) <= 0.f) g = 0.f;
                    const float d = rstd * (g * gj - c1 - xh * c2);
                    s_dg = fmaf(g, xh, s_dg);
                    s_db += g;
                    s_dbias += d;
                    dzr[j] = d;
                }
            } else if (jok) {
                float g = dyr[j];
                if (relu && zr[j] <= 0.f) g = 0.f;
                s_dbias += g;
                dzr[j] = g;
            }
        }
        red[0][wave][lane] = s_dg; red[1][wave][lane] = s_db; red[2][wave][lane] = s_dbias;
        __syncthreads();
        if (wave == 0 && jok) {
            float* pp = partial + (int64_t)blockIdx.x * 3 * n;
#pragma unroll
            for (int q = 0; q < 3; ++q)
                pp[q * n + j] = red[q][0][lane] + red[q][1][lane] + red[q][2][lane] + red[q][3][lane];
        }
        __syncthreads();
    }
}

// fold the block partials: block = 64 columns x 16 slices of the block list; fixed order; WRITES results
__global__ void __launch_bounds__(1024)
colsum_fold_kernel(const float* __restrict__ partial, int nblocks, int n, float* __restrict__ dgamma,
                   float* __restrict__ dbeta, float* __restrict__ dbias) {
    __shared__ float red[3][16][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    float a = 0.f, b = 0.f, c = 0.f;
    if (j < n) {
#pragma unroll 4
        for (int k = slice; k < nblocks; k += 16) {               // 4 x 3 independent loads in flight
            const float* pp = partial + (int64_t)k * 3 * n;
            a += pp[j]; b += pp[n + j]; c += pp[2 * n + j];
        }
    }
    red[0][slice][lane] = a; red[1][slice][lane] = b; red[2][slice][lane] = c;
    __syncthreads();
    if (slice < 3 && j < n) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[slice][k][lane];
        float* dst = slice == 0 ? dgamma : slice == 1 ? dbeta : dbias;
        if (dst) dst[j] = s;
    }
}

int ln_bwd_blocks(int64_t M) {
    static const int forced = GTE_MEASURE_INT("GTE_LNB_BLOCKS", 0);
    const int cap = forced > 0 ? forced : LNB_MAX_BLOCKS;
    const int64_t b = gte::ceil_div(M, 4);
    return (int)(b < cap ? b : cap);
}

// (NV, RF) of the 16-byte kernels by the width rounded up to 16: two rows in flight while the registers allow it
#define GTE_LN_LADDER(n16, LAUNCH)                                                                                          \
    do {                                                                                                                    \
        if ((n16) <= 256) LAUNCH(1, 2); else if ((n16) <= 512) LAUNCH(2, 2); else if ((n16) <= 768) LAUNCH(3, 1); else LAUNCH(4, 1); \
    } while (0)

}  // namespace

// ------------------------------------------ C ABI -------------------------------------------------
extern "C" int gte_ln_relu_fwd(const float* z, int64_t ldz, const float* gamma, const float* beta, float eps, int relu,
                               float* y, int64_t ldy, float* stats, int64_t M, int64_t n_out, void* stream) {
    if (M < 0 || n_out <= 0 || M > INT32_MAX || n_out > INT32_MAX)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_fwd: bad sizes");
    if (M == 0) return GTE_OK;
    if (!z || !y || !gamma || !beta) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_fwd: null pointer");
    if (ldz < n_out || ldy < n_out) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_fwd: ld < n_out");
    hipStream_t s = gte::as_stream(stream);
    if (n_out % 4 == 0 && n_out >= 128 && n_out <= 512) {          // 16-byte accesses, two rows per wave
#define GTE_LNF(NV, RF)                                                                                                        \
    hipLaunchKernelGGL((ln_relu_fwd_vec_kernel<NV, RF, false>), dim3((unsigned)gte::ceil_div(M, 4 * RF)), dim3(256), 0, s, z, ldz, gamma, \
                       beta, eps, relu, y, ldy, (char*)nullptr, (int64_t)0, stats, (int)M, (int)n_out)
        if (n_out <= 256) GTE_LNF(1, 2); else GTE_LNF(2, 2);
#undef GTE_LNF
    } else {
        hipLaunchKernelGGL(ln_relu_fwd_kernel, dim3((unsigned)gte::ceil_div(M, 4)), dim3(256), 0, s, z, ldz, gamma, beta, eps, relu, y,
                           ldy, stats, (int)M, (int)n_out);
    }
    return gte::check_launch("ln_relu_fwd");
}

// ... any width up to 1024 on PADDED rows (ldz, ldy >= n_out rounded up to 4), y as fp32 (nullable) and / or as a P3 image
// (nullable): the LayerNorm(+ReLU) of an aggregate-first planes layer, whose output feeds the next layer's planes GEMM
extern "C" int gte_ln_relu_fwd_p3(const float* z, int64_t ldz, const float* gamma, const float* beta, float eps, int relu,
                                  float* y, int64_t ldy, void* yp3, int64_t ldyp3, float* stats, int64_t M, int64_t n_out,
                                  void* stream) {
    if (M < 0 || n_out <= 0 || M > INT32_MAX || n_out > 1024)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_fwd_p3: bad sizes (n_out <= 1024)");
    if (M == 0) return GTE_OK;
    if (!z || !gamma || !beta || (!y && !yp3)) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_fwd_p3: null pointer");
    const int64_t n4 = gte::round_up(n_out, 4);
    if (ldz < n4 || (y && ldy < n4) || (yp3 && (ldyp3 < p3::row_bytes(n_out) || ldyp3 % 16 != 0)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_fwd_p3: rows must be padded to a multiple of 4 floats; ldp >= 96 ceil(n_out / 16)");
    hipStream_t s = gte::as_stream(stream);
    char* yp = reinterpret_cast<char*>(yp3);
#define GTE_LNF(NV, RF)                                                                                                       \
    hipLaunchKernelGGL((ln_relu_fwd_vec_kernel<NV, RF, true>), dim3((unsigned)gte::ceil_div(M, 4 * RF)), dim3(256), 0, s, z, ldz, gamma, \
                       beta, eps, relu, y, ldy, yp, ldyp3, stats, (int)M, (int)n_out)
    GTE_LN_LADDER(gte::round_up(n_out, 16), GTE_LNF);
#undef GTE_LNF
    return gte::check_launch("ln_relu_fwd_p3");
}

extern "C" int64_t gte_ln_relu_bwd_workspace_bytes(int64_t M, int64_t n_out) {
    return gte::round_up((int64_t)ln_bwd_blocks(M > 0 ? M : 1) * 3 * (n_out > 0 ? n_out : 1) * 4, 256);
}

static int ln_relu_bwd_impl(const float* dy, int64_t lddy, const float* z, int64_t ldz, const float* stats,
                            const float* gamma, const float* beta, int relu, float* dz, int64_t lddz,
                            float* dgamma, float* dbeta, float* dbias, int64_t M, int64_t n_out, void* workspace,
                            int64_t workspace_bytes, void* stream, char* dzp3, int64_t ldp3) {
    if (M < 0 || n_out <= 0 || M > INT32_MAX || n_out > INT32_MAX)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_bwd: bad sizes");
    if (M == 0) return GTE_OK;
    if (!dy || !dz || !workspace) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_bwd: null pointer");
    if ((gamma || relu) && !z) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_bwd: z is required");
    if (gamma && (!beta || !stats)) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_bwd: LayerNorm needs beta and stats");
    if (gamma && n_out > 1024 && dz == dy)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_bwd: dz must not alias dy when n_out > 1024 with LayerNorm");
    if (workspace_bytes < gte_ln_relu_bwd_workspace_bytes(M, n_out))
        return gte::fail(GTE_ERR_WORKSPACE_TOO_SMALL, "ln_relu_bwd: workspace too small");
    hipStream_t s = gte::as_stream(stream);
    const int nb = ln_bwd_blocks(M);
    const float* zz = z ? z : dy;
    const int64_t ldzz = z ? ldz : lddy;
    float* part = reinterpret_cast<float*>(workspace);
    dim3 grid((unsigned)nb), block(256);
#define GTE_LNB(NCH)                                                                                              \
    hipLaunchKernelGGL((ln_relu_bwd_kernel<NCH>), grid, block, (size_t)(4 * 3 * NCH * 64) * sizeof(float), s, dy, lddy, \
                       zz, ldzz, stats, gamma, beta, relu, dz, lddz, part, (int)M, (int)n_out)
#define GTE_LNV(NV)                                                                                                 \
    hipLaunchKernelGGL((ln_relu_bwd_vec_kernel<NV>), grid, block, (size_t)(4 * 3 * NV * 256) * sizeof(float), s, dy, lddy, \
                       zz, ldzz, stats, gamma, beta, relu, dz, lddz, part, (int)M, (int)n_out, dzp3, ldp3)
#define GTE_LNG(NV, RF)                                                                                                  \
    hipLaunchKernelGGL((ln_relu_bwd_gen_kernel<NV, RF>), grid, block, (size_t)(4 * 3 * NV * 256) * sizeof(float), s, dy, lddy, \
                       zz, ldzz, stats, gamma, beta, relu, dz, lddz, part, (int)M, (int)n_out, dzp3, ldp3)
    if (dzp3 && (ldp3 < p3::row_bytes(n_out) || ldp3 % 16 != 0))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_bwd: the P3 image needs ldp >= 96 ceil(n_out / 16)");
    if (dzp3 && !(n_out % 16 == 0 && n_out >= 128 && n_out <= 512)) {
        // any other width up to 1024 with the image: padded rows (ld >= n_out rounded up to 4), LayerNorm layers only
        const int64_t n4 = gte::round_up(n_out, 4);
        if (!gamma || n_out > 1024 || lddy < n4 || ldzz < n4 || lddz < n4)
            return gte::fail(GTE_ERR_UNSUPPORTED, "ln_relu_bwd: the P3 image at this width needs LayerNorm, n_out <= 1024 and rows padded "
                                                  "to a multiple of 4 floats");
        GTE_LN_LADDER(gte::round_up(n_out, 16), GTE_LNG);
    } else
    if (n_out % 4 == 0 && n_out >= 128 && n_out <= 512) {              // 16-byte accesses
        if (n_out <= 256) GTE_LNV(1); else GTE_LNV(2);
    } else
    if (n_out <= 64) GTE_LNB(1);
    else if (n_out <= 128) GTE_LNB(2);
    else if (n_out <= 256) GTE_LNB(4);
    else if (n_out <= 512) GTE_LNB(8);
    else if (n_out <= 1024) GTE_LNB(16);
    else
        hipLaunchKernelGGL(ln_relu_bwd_wide_kernel, grid, block, 0, s, dy, lddy, zz, ldzz, stats, gamma, beta, relu, dz,
                           lddz, part, (int)M, (int)n_out);
#undef GTE_LNB
#undef GTE_LNV
#undef GTE_LNG
    if (dgamma || dbeta || dbias) {
        // deferred (gte_fold_defer_begin): the three column sums join the step's fold batch
        if (gte::defer_fold(part, 3 * n_out, nb, 1, (int)n_out, dgamma, n_out)) {
            gte::defer_fold(part + n_out, 3 * n_out, nb, 1, (int)n_out, dbeta, n_out);
            gte::defer_fold(part + 2 * n_out, 3 * n_out, nb, 1, (int)n_out, dbias, n_out);
        } else {
            hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)gte::ceil_div(n_out, 64)), dim3(1024), 0, s, part, nb,
                               (int)n_out, dgamma, dbeta, dbias);
        }
    }
    return gte::check_launch("ln_relu_bwd");
}

extern "C" int gte_ln_relu_bwd(const float* dy, int64_t lddy, const float* z, int64_t ldz, const float* stats,
                               const float* gamma, const float* beta, int relu, float* dz, int64_t lddz,
                               float* dgamma, float* dbeta, float* dbias, int64_t M, int64_t n_out, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    return ln_relu_bwd_impl(dy, lddy, z, ldz, stats, gamma, beta, relu, dz, lddz, dgamma, dbeta, dbias, M, n_out, workspace,
                            workspace_bytes, stream, nullptr, 0);
}

// ... dz additionally as a P3 image (csrc/p3.h): the A operand of the layer's dX / dW planes GEMMs
extern "C" int gte_ln_relu_bwd_p3(const float* dy, int64_t lddy, const float* z, int64_t ldz, const float* stats,
                                  const float* gamma, const float* beta, int relu, float* dz, int64_t lddz, void* dzp3,
                                  int64_t ldp3, float* dgamma, float* dbeta, float* dbias, int64_t M, int64_t n_out,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (!dzp3) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "ln_relu_bwd_p3: null image");
    return ln_relu_bwd_impl(dy, lddy, z, ldz, stats, gamma, beta, relu, dz, lddz, dgamma, dbeta, dbias, M, n_out, workspace,
                            workspace_bytes, stream, reinterpret_cast<char*>(dzp3), ldp3);
}
