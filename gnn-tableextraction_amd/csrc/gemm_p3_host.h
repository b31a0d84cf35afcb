// The planes GEMMs (csrc/gemm_p3.hip) as the library's own C++ callers see them (csrc/step.hip).
//
// The C ABI (include/gte.h) names an entry point per WAY an operand is reached (gte_gemm_p3_nt / _nt_rows / _nt_rows2, ...).  Here the
// operands of a product are ONE descriptor, the row map a field of it, and there is one function per product; the C entry points
// are thin wrappers that fill a descriptor.  Arguments, checks, return codes and arithmetic: include/gte.h.
#pragma once
#include <stdint.h>

namespace gte {

// [a1 | a2] b^T: a1 = P3 [m][k1], a2 = P3 [m][k2] (nullptr, 0, 0: one K segment), b = P3 [n][ceil16(k1) + k2] (ldb < 0: block-major).
// rows != nullptr: a1 -- and a2, when present -- are RESIDENT images of n_res_rows rows, row i of the product is their row rows[i].
struct P3NtOperands {
    const void* a1; int64_t lda1, k1;
    const void* a2; int64_t lda2, k2;
    const void* b; int64_t ldb;
    const int32_t* rows; int64_t n_res_rows;
};

// a^T b over k rows; nseg > 0: two column segments of nseg columns, c[:, 0:nseg] = a^T b, c[:, nseg:] = a2^T b2 (a2 / b2 nullptr:
// the operand of segment 0).  rows != nullptr: b -- and b2 -- are RESIDENT images (the same row stride), k row i is their row rows[i].
struct P3TnOperands {
    const void* a; int64_t lda; const void* a2; int64_t lda2;
    const void* b; int64_t ldb; const void* b2; int64_t ldb2; int64_t nseg;
    const int32_t* rows; int64_t n_res_rows;
};

// (`name`: the entry point the error messages speak of)
// gte_gemm_p3_nt / _nt_rows / _nt_rows2
int gemm_p3_nt(const P3NtOperands& op, const float* bias, int64_t bias_cols, float* c, int64_t ldc, int64_t m, int64_t n, int relu,
               int accumulate, void* stream, const char* name = "gemm_p3_nt");
// gte_gemm_p3_nt_ln_fwd / _nt_rows2_ln_fwd
int gemm_p3_nt_ln_fwd(const P3NtOperands& op, const float* bias, const float* gamma, const float* beta, float eps, int relu, float* z,
                      int64_t ldz, float* y, int64_t ldy, void* yp3, int64_t ldyp3, float* stats, int64_t m, int64_t n, void* stream,
                      const char* name = "gemm_p3_nt_ln_fwd");
// gte_gemm_p3_nt_ln_bwd (no row map)
int gemm_p3_nt_ln_bwd(const P3NtOperands& op, const float* z, int64_t ldz, const float* stats, const float* gamma, const float* beta,
                      int relu, float* dz, int64_t lddz, void* dzp3, int64_t ldp3, float* dgamma, float* dbeta, float* dbias, int64_t m,
                      int64_t n, void* workspace, int64_t workspace_bytes, void* stream);
// gte_gemm_p3_nt_smallk_bwd (no row map)
int gemm_p3_nt_smallk_bwd(const P3NtOperands& op, const float* x, int64_t ldx, int64_t k1, const float* ahn, int64_t ldahn, int64_t k2,
                          const float* W, int64_t ldw, const float* bias, const float* gamma, const float* beta, const float* stats,
                          int relu, float* dW, int64_t lddw, float* dbias, float* dgamma, float* dbeta, int64_t m, int64_t n,
                          void* workspace, int64_t workspace_bytes, void* stream);
// gte_gemm_p3_tn / _tn_rows / _tn_rows2
int gemm_p3_tn(const P3TnOperands& op, float* c, int64_t ldc, int64_t m, int64_t n, int64_t k, void* workspace, int64_t workspace_bytes,
               void* stream, const char* name = "gemm_p3_tn");

}  // namespace gte
