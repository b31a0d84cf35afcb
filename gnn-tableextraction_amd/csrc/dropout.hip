// Dropout on the fused train step (models.py:46-66 with dropout > 0, :105-113): the producer of a dropout layer's two P3 operand
// images, the transpose aggregation of its backward, and the masks themselves as a test hook.  Keep bits from csrc/dropout.h:
// regenerated wherever they are needed, never stored.
//
// Mapping (both aggregation kernels): one wave per destination row (the row index, its CSR range and its edge list are
// wave-uniform: scalar loads); a lane owns one quarter block (four consecutive features, one Philox call) of up to CPL column
// stretches of 256 features; four source rows in flight per iteration.  Fixed summation order (CSR order): bit-reproducible.
#include "gte_common.h"
#include "dropout.h"
#include "p3.h"

#define GTE_DROP_TRY(call)        \
    do {                          \
        const int rc_ = (call);   \
        if (rc_ != GTE_OK) return rc_; \
    } while (0)

namespace {

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };

constexpr int kEdgeUnroll = 4;

struct DropArgs {
    dropout::Key key;
    uint32_t thr;
    float scale;
    const int64_t* step_counter;
    uint32_t site;
};

__device__ __forceinline__ void apply4(unsigned bits, float scale, float (&v)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = ((bits >> q) & 1u) ? v[q] * scale : 0.f;
}

// four features 4 qi .. 4 qi + 3 of batch row u; features >= n_feat read as zeros.  fp32 rows, or a P3 image (exact: (h + m) + l)
// whose rows are the rows x_rows[u] of a resident image (x_rows NULL: row u)
__device__ __forceinline__ void load4(const float* __restrict__ x, int64_t ldx, const char* __restrict__ xp, int64_t ldpx,
                                      const int32_t* __restrict__ x_rows, int u, int qi, int n_feat, float (&v)[4]) {
    const int c0 = qi * 4;
    if (xp) {
        const int64_t row = x_rows ? (int64_t)x_rows[u] : (int64_t)u;
        const char* p = xp + row * ldpx + (int64_t)(qi >> 2) * p3::BLOCK_BYTES + (qi & 3) * 8;
        const uint2 h = *reinterpret_cast<const uint2*>(p);
        const uint2 m = *reinterpret_cast<const uint2*>(p + p3::PLANE_BYTES);
        const uint2 l = *reinterpret_cast<const uint2*>(p + 2 * p3::PLANE_BYTES);
        v[0] = (__uint_as_float(h.x << 16) + __uint_as_float(m.x << 16)) + __uint_as_float(l.x << 16);
        v[1] = (__uint_as_float(h.x & 0xffff0000u) + __uint_as_float(m.x & 0xffff0000u)) + __uint_as_float(l.x & 0xffff0000u);
        v[2] = (__uint_as_float(h.y << 16) + __uint_as_float(m.y << 16)) + __uint_as_float(l.y << 16);
        v[3] = (__uint_as_float(h.y & 0xffff0000u) + __uint_as_float(m.y & 0xffff0000u)) + __uint_as_float(l.y & 0xffff0000u);
        return;                                          // (image columns >= n_feat are zero by construction)
    }
    const float* r = x + (int64_t)u * ldx + c0;
    if (c0 + 4 <= n_feat) {
        const f4u t = *reinterpret_cast<const f4u*>(r);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = c0 + q < n_feat ? r[q] : 0.f;
    }
}

// self image = D_site(D_in?(x[v])), agg image = D_site(scale_v sum_{u -> v} w D_in?(x[u])) with the mask columns of the agg half
// at n_feat + c (ONE mask over cat(h, ah * norm): models.py:60-61)
template <int CPL>
__global__ void __launch_bounds__(256)
spmm_dropout_p3_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices, const float* __restrict__ ew,
                       const float* __restrict__ x, int64_t ldx, const char* __restrict__ xp, int64_t ldpx,
                       const int32_t* __restrict__ x_rows, int in_drop, DropArgs d, char* __restrict__ selfp, int64_t ldps,
                       char* __restrict__ aggp, int64_t ldpa, int n_rows, int n_feat) {
    const uint32_t step = (uint32_t)*d.step_counter;
    const int lane = threadIdx.x & (gte::kWave - 1);
    const int nq = (n_feat + 3) >> 2;                        // quarters holding features
    const int nqp = (int)p3::blocks(n_feat) * 4;             // quarters of an image row (the rest of the last block: zeros)
    const int waves = gridDim.x * (blockDim.x >> 6);
    for (int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += waves) {
        const int v = __builtin_amdgcn_readfirstlane(r);
        const int lo = indptr[v], hi = indptr[v + 1];
        const float sv = hi > lo ? 1.0f / (float)(hi - lo) : 0.0f;
        for (int qb = 0; qb < nqp; qb += gte::kWave * CPL) {
            float acc[CPL][4], self[CPL][4];
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int qi = qb + lane + j * gte::kWave;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[j][q] = self[j][q] = 0.f;
                if (qi < nq) {
                    load4(x, ldx, xp, ldpx, x_rows, v, qi, n_feat, self[j]);
                    if (in_drop) apply4(dropout::keep4(d.key, d.thr, step, 0u, (uint32_t)v, (uint32_t)qi * 4), d.scale, self[j]);
                }
            }
            for (int e0 = lo; e0 < hi; e0 += kEdgeUnroll) {
                int u[kEdgeUnroll];
                float w[kEdgeUnroll];
#pragma unroll
                for (int k = 0; k < kEdgeUnroll; ++k) {
                    const int e = min(e0 + k, hi - 1);           // past the row's end: the last edge again with w = 0
                    u[k] = indices[e];
                    w[k] = e0 + k < hi ? (ew ? ew[e] : 1.0f) : 0.f;
                }
                float t[kEdgeUnroll][CPL][4];
#pragma unroll
                for (int k = 0; k < kEdgeUnroll; ++k)
#pragma unroll
                    for (int j = 0; j < CPL; ++j) {
                        const int qi = qb + lane + j * gte::kWave;
#pragma unroll
                        for (int q = 0; q < 4; ++q) t[k][j][q] = 0.f;
                        if (qi < nq) load4(x, ldx, xp, ldpx, x_rows, u[k], qi, n_feat, t[k][j]);
                    }
#pragma unroll
                for (int k = 0; k < kEdgeUnroll; ++k)
#pragma unroll
                    for (int j = 0; j < CPL; ++j) {
                        const int qi = qb + lane + j * gte::kWave;
                        if (qi < nq && in_drop)
                            apply4(dropout::keep4(d.key, d.thr, step, 0u, (uint32_t)u[k], (uint32_t)qi * 4), d.scale, t[k][j]);
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[j][q] = fmaf(w[k], t[k][j][q], acc[j][q]);
                    }
            }
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int qi = qb + lane + j * gte::kWave;
                if (qi >= nqp) continue;
                float a[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = acc[j][q] * sv;
                if (qi < nq) {
                    apply4(dropout::keep4(d.key, d.thr, step, d.site, (uint32_t)v, (uint32_t)qi * 4), d.scale, self[j]);
                    apply4(dropout::keep4(d.key, d.thr, step, d.site, (uint32_t)v, (uint32_t)(n_feat + qi * 4)), d.scale, a);
                }
                p3::store4(selfp + (int64_t)v * ldps, qi * 4, self[j][0], self[j][1], self[j][2], self[j][3]);
                p3::store4(aggp + (int64_t)v * ldpa, qi * 4, a[0], a[1], a[2], a[3]);
            }
        }
    }
}

// dx[v] = D_self(g[v, 0:n]) + sum_{v -> u} w_out D_agg(g[u, agg_col:agg_col + n]) with the masks of the forward (row u's agg half:
// mask columns n_feat + c).  Columns n_feat .. round_up(n_feat, 4) of dx are written as zeros.
template <int CPL>
__global__ void __launch_bounds__(256)
spmm_dropout_bwd_kernel(const int32_t* __restrict__ rindptr, const int32_t* __restrict__ rindices, const float* __restrict__ w_out,
                        const float* __restrict__ g, int64_t ldg, int64_t agg_col, DropArgs d, float* __restrict__ dx, int64_t lddx,
                        int n_rows, int n_feat) {
    const uint32_t step = (uint32_t)*d.step_counter;
    const int lane = threadIdx.x & (gte::kWave - 1);
    const int nq = (n_feat + 3) >> 2;
    const int waves = gridDim.x * (blockDim.x >> 6);
    for (int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += waves) {
        const int v = __builtin_amdgcn_readfirstlane(r);
        const int lo = rindptr[v], hi = rindptr[v + 1];
        for (int qb = 0; qb < nq; qb += gte::kWave * CPL) {
            float acc[CPL][4];
#pragma unroll
            for (int j = 0; j < CPL; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[j][q] = 0.f;
            for (int e0 = lo; e0 < hi; e0 += kEdgeUnroll) {
                int u[kEdgeUnroll];
                float w[kEdgeUnroll];
#pragma unroll
                for (int k = 0; k < kEdgeUnroll; ++k) {
                    const int e = min(e0 + k, hi - 1);
                    u[k] = rindices[e];
                    w[k] = e0 + k < hi ? w_out[e] : 0.f;
                }
                float t[kEdgeUnroll][CPL][4];
#pragma unroll
                for (int k = 0; k < kEdgeUnroll; ++k)
#pragma unroll
                    for (int j = 0; j < CPL; ++j) {
                        const int qi = qb + lane + j * gte::kWave;
                        if (qi < nq) {
                            const float4 q4 = *reinterpret_cast<const float4*>(g + (int64_t)u[k] * ldg + agg_col + qi * 4);
                            t[k][j][0] = q4.x; t[k][j][1] = q4.y; t[k][j][2] = q4.z; t[k][j][3] = q4.w;
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; ++q) t[k][j][q] = 0.f;
                        }
                    }
#pragma unroll
                for (int k = 0; k < kEdgeUnroll; ++k)
#pragma unroll
                    for (int j = 0; j < CPL; ++j) {
                        const int qi = qb + lane + j * gte::kWave;
                        if (qi < nq)
                            apply4(dropout::keep4(d.key, d.thr, step, d.site, (uint32_t)u[k], (uint32_t)(n_feat + qi * 4)), d.scale, t[k][j]);
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[j][q] = fmaf(w[k], t[k][j][q], acc[j][q]);
                    }
            }
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int qi = qb + lane + j * gte::kWave;
                if (qi >= nq) continue;
                const float4 s4 = *reinterpret_cast<const float4*>(g + (int64_t)v * ldg + qi * 4);
                float s[4] = {s4.x, s4.y, s4.z, s4.w};
                apply4(dropout::keep4(d.key, d.thr, step, d.site, (uint32_t)v, (uint32_t)qi * 4), d.scale, s);
                float4 o;
                o.x = qi * 4 + 0 < n_feat ? s[0] + acc[j][0] : 0.f;
                o.y = qi * 4 + 1 < n_feat ? s[1] + acc[j][1] : 0.f;
                o.z = qi * 4 + 2 < n_feat ? s[2] + acc[j][2] : 0.f;
                o.w = qi * 4 + 3 < n_feat ? s[3] + acc[j][3] : 0.f;
                *reinterpret_cast<float4*>(dx + (int64_t)v * lddx + qi * 4) = o;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
dropout_mask_kernel(dropout::Key key, uint32_t thr, uint32_t step, uint32_t site, int64_t n_rows, int64_t n_cols, uint8_t* __restrict__ mask,
                    int64_t ldm) {
    const int64_t nq = (n_cols + 3) >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * nq) return;
    const int64_t r = i / nq, qi = i - r * nq;
    const unsigned bits = dropout::keep4(key, thr, step, site, (uint32_t)r, (uint32_t)(qi * 4));
    uint8_t* m = mask + r * ldm + qi * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (qi * 4 + q < n_cols) m[q] = (uint8_t)((bits >> q) & 1u);
}

int check_p(float p, const char* what) {
    if (!(p > 0.f && p < 1.f)) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: dropout probability must lie in (0, 1), got %g", what, (double)p);
    return GTE_OK;
}

DropArgs drop_args(float p, uint64_t seed, int rank, const int64_t* step_counter, int site) {
    return DropArgs{dropout::make_key(seed, rank), dropout::threshold(p), dropout::scale(p), step_counter, (uint32_t)site};
}

int grid_rows(int64_t n_rows) { return (int)gte::ceil_div(n_rows, 4); }      // one wave per row, four waves per block

// Rows of a launch: row indices, the grid-stride sum r + waves (waves <= n_rows + 3) and the Philox row word are 32-bit, so
// n_rows <= 2^30 keeps every one of them below 2^31.  Everything that is multiplied by a row stride is 64-bit per lane already
// (the gathers reach arbitrary rows: no window to rebase), so no image or row buffer has a byte bound.
int check_rows(int64_t n_rows, const char* what) {
    if (n_rows > GTE_DROPOUT_MAX_ROWS)
        return gte::fail(GTE_ERR_UNSUPPORTED, "%s: %lld rows; a dropout launch holds at most 2^30 rows (32-bit row indices)", what, (long long)n_rows);
    return GTE_OK;
}

thread_local int g_wide_forced = 0;          // gte_dropout_set_wide
thread_local int g_wide_scope = 0;           // open WideScope(true) objects of this thread

}  // namespace

bool gte::wide_forced() { return g_wide_forced != 0 || g_wide_scope > 0; }
gte::WideScope::WideScope(bool on) : prev_(g_wide_scope) { if (on) ++g_wide_scope; }
gte::WideScope::~WideScope() { g_wide_scope = prev_; }

extern "C" int gte_dropout_set_wide(int mode) {
    if (mode != 0 && mode != 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "dropout_set_wide: mode must be 0 (by size) or 1 (always)");
    g_wide_forced = mode;
    return GTE_OK;
}
extern "C" int gte_dropout_get_wide(void) { return g_wide_forced; }

extern "C" int gte_dropout_mask(float p, uint64_t seed, int rank, int64_t step, int site, int64_t n_rows, int64_t n_cols, uint8_t* mask,
                                int64_t ldm, void* stream) {
    GTE_DROP_TRY(check_p(p, "dropout_mask"));
    if (n_rows < 0 || n_cols < 0 || n_rows > INT32_MAX || site < 0 || ldm < n_cols) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "dropout_mask: bad sizes");
    if (n_rows == 0 || n_cols == 0) return GTE_OK;
    if (!mask) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "dropout_mask: null pointer");
    const int64_t total = n_rows * ((n_cols + 3) / 4);
    if (total > ((int64_t)1 << 38)) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "dropout_mask: too many elements");
    dropout_mask_kernel<<<(unsigned)gte::ceil_div(total, 256), 256, 0, gte::as_stream(stream)>>>(
        dropout::make_key(seed, rank), dropout::threshold(p), (uint32_t)step, (uint32_t)site, n_rows, n_cols, mask, ldm);
    return gte::check_launch("dropout_mask");
}

extern "C" int gte_dropout_mask_host(float p, uint64_t seed, int rank, int64_t step, int site, int64_t n_rows, int64_t n_cols, uint8_t* mask,
                                     int64_t ldm) {
    GTE_DROP_TRY(check_p(p, "dropout_mask_host"));
    if (n_rows < 0 || n_cols < 0 || n_rows > INT32_MAX || site < 0 || ldm < n_cols) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "dropout_mask_host: bad sizes");
    if (n_rows > 0 && n_cols > 0 && !mask) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "dropout_mask_host: null pointer");
    const dropout::Key key = dropout::make_key(seed, rank);
    const uint32_t thr = dropout::threshold(p);
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t c = 0; c < n_cols; c += 4) {
            const unsigned bits = dropout::keep4(key, thr, (uint32_t)step, (uint32_t)site, (uint32_t)r, (uint32_t)c);
            for (int q = 0; q < 4 && c + q < n_cols; ++q) mask[r * ldm + c + q] = (uint8_t)((bits >> q) & 1u);
        }
    return GTE_OK;
}

extern "C" int gte_spmm_dropout_p3(const int32_t* indptr, const int32_t* indices, const float* eweight, const float* x, int64_t ldx,
                                   const void* xp, int64_t ldpx, const int32_t* x_rows, int64_t n_res_rows, int in_dropout, float p,
                                   uint64_t seed, int rank, const int64_t* step_counter, int site, void* selfp3, int64_t ldp_self,
                                   void* aggp3, int64_t ldp_agg, int64_t n_rows, int64_t n_feat, void* stream) {
    GTE_DROP_TRY(check_p(p, "spmm_dropout_p3"));
    if (n_rows < 0 || n_feat <= 0 || n_rows > INT32_MAX || n_feat > (1 << 24) || site < 1)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "spmm_dropout_p3: bad sizes or site");
    GTE_DROP_TRY(check_rows(n_rows, "spmm_dropout_p3"));
    if (n_rows == 0) return GTE_OK;
    if (!indptr || !step_counter || !selfp3 || !aggp3 || (!x == !xp))          // indices may be NULL for an edgeless graph
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "spmm_dropout_p3: null pointer (exactly one of x / xp is the input)");
    if (x && ldx < n_feat) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "spmm_dropout_p3: ldx < n_feat");
    if (xp && (ldpx < p3::row_bytes(n_feat) || ldpx % 16 != 0 || (x_rows && n_res_rows <= 0)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "spmm_dropout_p3: input image row stride / resident rows");
    if (ldp_self < p3::row_bytes(n_feat) || ldp_self % 16 != 0 || ldp_agg < p3::row_bytes(n_feat) || ldp_agg % 16 != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "spmm_dropout_p3: output image row stride");
    const DropArgs d = drop_args(p, seed, rank, step_counter, site);
    const int64_t nqp = p3::blocks(n_feat) * 4;
    hipStream_t s = gte::as_stream(stream);
    const char* xc = static_cast<const char*>(xp);
    char* sp = static_cast<char*>(selfp3);
    char* ap = static_cast<char*>(aggp3);
#define GTE_DROP_FWD(C) spmm_dropout_p3_kernel<C><<<grid_rows(n_rows), 256, 0, s>>>(indptr, indices, eweight, x, ldx, xc, ldpx, x_rows, \
                                                    in_dropout ? 1 : 0, d, sp, ldp_self, ap, ldp_agg, (int)n_rows, (int)n_feat)
    if (nqp <= gte::kWave) GTE_DROP_FWD(1);
    else if (nqp <= 2 * gte::kWave) GTE_DROP_FWD(2);
    else GTE_DROP_FWD(4);
#undef GTE_DROP_FWD
    return gte::check_launch("spmm_dropout_p3");
}

extern "C" int gte_spmm_dropout_bwd(const int32_t* rindptr, const int32_t* rindices, const float* w_out, const float* g, int64_t ldg,
                                    int64_t agg_col, float p, uint64_t seed, int rank, const int64_t* step_counter, int site, float* dx,
                                    int64_t lddx, int64_t n_rows, int64_t n_feat, void* stream) {
    GTE_DROP_TRY(check_p(p, "spmm_dropout_bwd"));
    if (n_rows < 0 || n_feat <= 0 || n_rows > INT32_MAX || n_feat > (1 << 24) || site < 1)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "spmm_dropout_bwd: bad sizes or site");
    GTE_DROP_TRY(check_rows(n_rows, "spmm_dropout_bwd"));
    if (n_rows == 0) return GTE_OK;
    if (!rindptr || !g || !step_counter || !dx)                                // rindices, w_out may be NULL for an edgeless graph
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "spmm_dropout_bwd: null pointer");
    const int64_t n4 = gte::round_up(n_feat, 4);
    if (agg_col % 4 != 0 || ldg % 4 != 0 || agg_col < n4 || ldg < agg_col + n4 || lddx % 4 != 0 || lddx < n4 ||
        reinterpret_cast<uintptr_t>(g) % 16 != 0 || reinterpret_cast<uintptr_t>(dx) % 16 != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "spmm_dropout_bwd: g / dx need 16-byte aligned rows of at least round_up(n_feat, 4) floats "
                                                   "per half (agg_col, ldg, lddx multiples of 4)");
    const DropArgs d = drop_args(p, seed, rank, step_counter, site);
    hipStream_t s = gte::as_stream(stream);
#define GTE_DROP_BWD(C) spmm_dropout_bwd_kernel<C><<<grid_rows(n_rows), 256, 0, s>>>(rindptr, rindices, w_out, g, ldg, agg_col, d, dx, \
                                                     lddx, (int)n_rows, (int)n_feat)
    const int64_t nq = n4 / 4;
    if (nq <= gte::kWave) GTE_DROP_BWD(1);
    else if (nq <= 2 * gte::kWave) GTE_DROP_BWD(2);
    else GTE_DROP_BWD(4);
#undef GTE_DROP_BWD
    return gte::check_launch("spmm_dropout_bwd");
}
