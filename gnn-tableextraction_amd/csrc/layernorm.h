// Device arithmetic of LayerNorm(+ReLU) that more than one translation unit uses: the stand-alone kernels (layernorm.hip), the
// one-pass short-K layer (sage_linear.hip) and the fused backward forms (gemm_p3.hip, narrow_layer.hip), which tests/test_gemm_p3.py
// and tests/test_gpu_parity.py hold bit for bit to the stand-alone kernels.
#pragma once
#include "gte_common.h"

namespace gte_ln {

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };      // 16-byte access at 4-byte alignment

__device__ __forceinline__ float wave_sum(float v) { return gte_group_sum<64>(v); }

// pre = xhat gamma + beta.  The backward's ReLU mask is DEFINED on the stored stats: pre from xhat = (z - stats.mean) * stats.rstd,
// gradient where pre > 0.  The 16-byte forward (ln_relu_fwd_vec_kernel, layernorm.hip) forms z - mean as fma(-1 / n, sum, z) instead,
// about |mean| / std * 2^-24 away, so its y > 0 can disagree with that mask where |pre| is that close to zero (counted, and bounded, by
// tests/test_gpu_layernorm.py).
__device__ __forceinline__ float ln_affine(float xhat, float g, float b) { return fmaf(xhat, g, b); }

// mean = sum / n ROUNDED to float32, i.e. the value the statistics store, for a forward whose backward recomputes z and must find the
// mask the forward took (sage_smallk_fwd_kernel / gte_smallk_bwd_step).  Written as `sum * inv_n` next to `z - mean` the product is
// contracted into fma(-inv_n, sum, z): an unrounded mean, and on a constant row (where z - mean is nothing but that rounding) an xhat
// the backward cannot rebuild from the stats -- tests/test_gpu_smallk_bwd.py found y > 0 on such rows at n = 100, 200, 252 where the
// backward's mask was false.  At n = 2^k the product is exact and both forms are the same bits.  The empty asm makes the rounded
// product opaque, so no contraction setting can fuse it: a `#pragma clang fp contract(off)` is ignored under -ffp-contract=fast, and
// this toolchain's __fmul_rn is a plain `x * y` that is contracted like any other once inlined.
__device__ __forceinline__ float ln_mean_rounded(float sum, float inv_n) {
    float mean = sum * inv_n;
    asm volatile("" : "+v"(mean));
    return mean;
}

}  // namespace gte_ln

// ---- LayerNorm(+ReLU) backward of four columns of one row (device) ------------------------------------------------------------
// Shared by ln_relu_bwd_vec_kernel (layernorm.hip), the LayerNorm-backward epilogue of the planes NT GEMM (gemm_p3.hip) and the narrow
// layer's fused backward (narrow_layer.hip): the same instruction sequence at every call site (explicit fmaf, contraction off for
// everything else), so the fused launch is bit for bit the two launches.  pre: xhat, masked gradient g and this lane's share of the
// two row sums; post (after the row sums c1 = mean(dxhat), c2 = mean(dxhat xhat) are known): dz and the column partials.
__device__ __forceinline__ void gte_ln_bwd_pre4(const float (&gy)[4], const float (&zz)[4], float mean, float rstd, const float (&gam)[4],
                                                const float (&bet)[4], bool okc, int relu, float (&xh)[4], float (&g)[4], float& a,
                                                float& b) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        xh[e] = okc ? (zz[e] - mean) * rstd : 0.f;
        float gv = gy[e];
        if (relu && fmaf(xh[e], gam[e], bet[e]) <= 0.f) gv = 0.f;
        g[e] = gv;
        const float dxh = gv * gam[e];
        a = a + dxh;
        b = fmaf(dxh, xh[e], b);
    }
}
__device__ __forceinline__ void gte_ln_bwd_post4(const float (&g)[4], const float (&xh)[4], const float (&gam)[4], float rstd, float c1,
                                                 float c2, bool okc, float (&d)[4], float (&s_dg)[4], float (&s_db)[4],
                                                 float (&s_dbias)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t0 = g[e] * gam[e];
        const float t1 = xh[e] * c2;
        d[e] = rstd * ((t0 - c1) - t1);
        s_dg[e] = fmaf(g[e], xh[e], s_dg[e]);
        s_db[e] = s_db[e] + g[e];
        s_dbias[e] = s_dbias[e] + (okc ? d[e] : 0.f);
    }
}
// ... for a LayerNorm width that is not a multiple of 4 (16): per-element validity; the arithmetic of ln_relu_bwd_gen_kernel (layernorm.hip)
__device__ __forceinline__ void gte_ln_bwd_pre4m(const float (&gy)[4], const float (&zz)[4], float mean, float rstd, const float (&gam)[4],
                                                 const float (&bet)[4], const bool (&ok)[4], int relu, float (&xh)[4], float (&g)[4],
                                                 float& a, float& b) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        xh[e] = ok[e] ? (zz[e] - mean) * rstd : 0.f;
        float gv = ok[e] ? gy[e] : 0.f;
        if (relu && fmaf(xh[e], gam[e], bet[e]) <= 0.f) gv = 0.f;
        g[e] = gv;
        const float dxh = gv * gam[e];
        a = a + dxh;
        b = fmaf(dxh, xh[e], b);
    }
}
__device__ __forceinline__ void gte_ln_bwd_post4m(const float (&g)[4], const float (&xh)[4], const float (&gam)[4], float rstd, float c1,
                                                  float c2, const bool (&ok)[4], float (&d)[4], float (&s_dg)[4], float (&s_db)[4],
                                                  float (&s_dbias)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t0 = g[e] * gam[e];
        const float t1 = xh[e] * c2;
        d[e] = ok[e] ? rstd * ((t0 - c1) - t1) : 0.f;
        s_dg[e] = fmaf(g[e], xh[e], s_dg[e]);
        s_db[e] = s_db[e] + g[e];
        s_dbias[e] = s_dbias[e] + d[e];
    }
}
