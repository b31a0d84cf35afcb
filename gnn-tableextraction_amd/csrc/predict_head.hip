// The per-word head of label-free prediction: from the logits of a node its class (arg-max), the confidence of that class (its
// softmax probability) and, on request, the whole softmax row -- one launch in place of torch.argmax + torch.softmax + max.
//
// The contract is the definition in include/gte.h; tests/predict_head_ref.py (numpy float64, written from it) is the oracle.
//
// Structure.  One launch, ONE LANE PER NODE, grid-stride over nodes.  A lane holds its row in registers (C <= 16 floats; every
// loop over classes is unrolled to the limit and guarded by the wave-uniform C, so the row is never indexed dynamically: no
// scratch), scans it once for the arg-max and once, in float64 and in index order, for the exponentials and their sum.
// Why a lane per node and not a tile staged through LDS: the 64 rows of a wave are one contiguous span of 64 * ld floats, so
// every cache line that the wave's strided loads touch is consumed whole by the same wave within its C loads.  The traffic to HBM
// is that of the coalesced form; what the strided form costs is more L1 transactions per wave.  At the sizes this is called at --
// the nodes of one batch of pages, a few thousand to a few ten thousand -- the launch is latency, not traffic, and the staged form
// would add an LDS image and two barriers per workgroup to save none of it.  pred and conf are written at consecutive addresses
// by consecutive lanes, prob as the logits are read.
// No atomics, no LDS, no workspace, no synchronisation: deterministic.
#include "gte_common.h"

#include <math.h>

namespace {

constexpr int PH_THREADS = 256;
constexpr int PH_MAX_C = 16;                          // the step engine's class limit
constexpr int PH_MAX_BLOCKS = 4096;

__global__ void __launch_bounds__(PH_THREADS)
predict_head_kernel(const float* __restrict__ logits, int64_t ld_logits, int64_t n_nodes, int n_classes, int64_t* __restrict__ pred,
                    float* __restrict__ conf, float* __restrict__ prob, int64_t ld_prob) {
    const int64_t stride = (int64_t)gridDim.x * PH_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PH_THREADS + threadIdx.x; i < n_nodes; i += stride) {
        const float* __restrict__ row = logits + i * ld_logits;
        float l[PH_MAX_C];
#pragma unroll
        for (int j = 0; j < PH_MAX_C; ++j) l[j] = j < n_classes ? row[j] : 0.f;      // columns C .. ld-1 are never read

        // torch.argmax on the CPU: the first index of the maximum; a NaN is greater than every number and the first NaN stays
        float m = l[0];
        int arg = 0;
#pragma unroll
        for (int j = 1; j < PH_MAX_C; ++j) {
            if (j < n_classes && !(m != m) && (l[j] > m || l[j] != l[j])) { m = l[j]; arg = j; }
        }

        // float64, index order.  inf - inf and NaN propagate by themselves: a row with NaN or +inf, or of -inf only, gives NaN
        double e[PH_MAX_C];
        double s = 0.0, e_pred = 0.0;
#pragma unroll
        for (int j = 0; j < PH_MAX_C; ++j) {
            e[j] = 0.0;
            if (j < n_classes) {
                e[j] = exp((double)l[j] - (double)m);
                s += e[j];
                if (j == arg) e_pred = e[j];
            }
        }
        pred[i] = arg;
        conf[i] = (float)(e_pred / s);
        if (prob != nullptr) {
            float* __restrict__ out = prob + i * ld_prob;
#pragma unroll
            for (int j = 0; j < PH_MAX_C; ++j)
                if (j < n_classes) out[j] = (float)(e[j] / s);
        }
    }
}

}  // namespace

extern "C" int gte_predict_head(const float* logits, int64_t ld_logits, int64_t n_nodes, int n_classes, int64_t* pred, float* conf,
                                float* prob, int64_t ld_prob, void* stream) {
    if (n_nodes < 0 || n_classes < 1 || n_classes > PH_MAX_C)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "predict_head: bad sizes (n_nodes %lld, n_classes %d: 1 .. %d)", (long long)n_nodes,
                         n_classes, PH_MAX_C);
    if (ld_logits < n_classes)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "predict_head: ld_logits %lld < n_classes %d", (long long)ld_logits, n_classes);
    if (prob != nullptr && ld_prob < n_classes)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "predict_head: ld_prob %lld < n_classes %d", (long long)ld_prob, n_classes);
    if (n_nodes == 0) return GTE_OK;
    if (!logits || !pred || !conf) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "predict_head: null pointer");
    if ((((uintptr_t)logits | (uintptr_t)conf | (uintptr_t)prob) & 3) != 0 || ((uintptr_t)pred & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "predict_head: logits, conf and prob must be 4-byte aligned, pred 8-byte");
    const int64_t blocks = gte::ceil_div(n_nodes, PH_THREADS);
    hipLaunchKernelGGL(predict_head_kernel, dim3((unsigned)(blocks < PH_MAX_BLOCKS ? blocks : PH_MAX_BLOCKS)), dim3(PH_THREADS), 0,
                       gte::as_stream(stream), logits, ld_logits, n_nodes, n_classes, pred, conf, prob, ld_prob);
    return gte::check_launch("predict_head");
}
