// Box matching for the box-level evaluation of predicted regions (AP at IoU thresholds): per cell = one (page, kind) pair, the
// number of greedy matches between the cell's ground-truth boxes and every score-pruned suffix of its predictions.
//
// Reference: get_single_image_results() / calc_iou_individual() of src/utils/metrics.py:20-114, which the reference's
// get_avg_precision_at_iou() calls again for a page whenever its lowest-scored boxes are pruned.  The contract is the definition in
// include/gte.h; tests/boxeval_ref.py (pure Python, written from it) is the oracle, every output is an integer and compared exactly.
//
// Structure.  One workgroup per cell, everything in LDS.
//   phase 1  IoU of every (prediction, ground truth) pair in fp64 from exact integer areas (+1 pixel convention; the disjointness
//            test comes first, so touching boxes overlap).  The operands are integers below 2^53 and the division is IEEE: the
//            quotient is the correctly rounded one, as Python's int / int.  Pairs with iou > iou_thr[0] (the smallest threshold)
//            are appended to a list through an LDS counter.
//   phase 2  bitonic sort of the list by (IoU descending, pair index p * G + g descending): a total order, so the arrival order of
//            phase 1 does not reach the result.  A positive double orders as its bit pattern, the list is padded to a power of two
//            with zeros (a candidate's IoU is > 0), which sort behind every candidate.
//   phase 3  the candidates at iou_thr[j] are a prefix of the sorted list, and the matching after pruning the k lowest-scored
//            predictions is the greedy walk that skips the pairs with p < k.  The n_thr x R walks are independent: one thread
//            per walk with its two bit sets (matched predictions, matched ground truths) in LDS, 256 walks at a time.
// Every loop bound that stands in front of a barrier is a value all threads read from the same LDS word or argument; the walks
// diverge, no barrier stands inside them.  Integer outputs only, no float atomics, no allocation, no synchronisation.
#include "gte_common.h"

#include <cmath>

namespace {

constexpr int BM_THREADS = 256;
constexpr int BM_MAX_BOXES = 256;                     // per cell and side: p * G + g < 2^16
constexpr int BM_MAX_CAND = 4096;                     // per cell (a power of two: the padded length of the sort)
constexpr int BM_MAX_THR = 16;
constexpr int BM_SET_WORDS = BM_MAX_BOXES / 32;       // one bit set of a walk
constexpr int BM_MAX_EXTENT = 1 << 25;                // width / height (+1 convention) of a box: areas <= 2^50, their sum < 2^53
static_assert((BM_MAX_CAND & (BM_MAX_CAND - 1)) == 0, "the sort pads to a power of two");
static_assert(BM_MAX_BOXES * BM_MAX_BOXES <= 65536, "a pair index is a 16-bit word");
static_assert(BM_THREADS * 2 * BM_SET_WORDS * 4 >= 2 * BM_MAX_BOXES * 16, "the bit sets reuse the boxes' LDS");

struct Thresholds { double v[BM_MAX_THR]; };

// (x1 - x0 + 1, y1 - y0 + 1) of a well-formed box whose extents the exact arithmetic covers; (0, 0) otherwise: such a box overlaps
// nothing
__device__ __forceinline__ bool box_ok(const int4& b) {
    const int64_t w = (int64_t)b.z - b.x + 1, h = (int64_t)b.w - b.y + 1;
    return w >= 1 && h >= 1 && w <= BM_MAX_EXTENT && h <= BM_MAX_EXTENT;
}

__device__ __forceinline__ double box_iou(const int4& p, const int4& t) {
    if (t.z < p.x || p.z < t.x || t.w < p.y || p.w < t.y) return 0.0;            // metrics.py:42 (before anything else)
    const int64_t far_x = min(t.z, p.z), near_x = max(t.x, p.x), far_y = min(t.w, p.w), near_y = max(t.y, p.y);       // (int min / max)
    const int64_t inter = (far_x - near_x + 1) * (far_y - near_y + 1);
    const int64_t ta = ((int64_t)t.z - t.x + 1) * ((int64_t)t.w - t.y + 1);
    const int64_t pa = ((int64_t)p.z - p.x + 1) * ((int64_t)p.w - p.y + 1);
    return (double)inter / (double)(ta + pa - inter);
}

// list order: IoU descending, then pair index descending
__device__ __forceinline__ bool cand_before(unsigned long long ia, unsigned pa, unsigned long long ib, unsigned pb) {
    return ia > ib || (ia == ib && pa > pb);
}

// grid = cells
__global__ void __launch_bounds__(BM_THREADS)
box_match_kernel(const int32_t* __restrict__ pred_box, const int32_t* __restrict__ pred_off, const int32_t* __restrict__ gt_box,
                 const int32_t* __restrict__ gt_off, int n_cells, int cap_pred, int cap_gt, Thresholds thr, int n_thr,
                 int32_t* __restrict__ tp, int32_t* __restrict__ cell_status) {
    __shared__ __attribute__((aligned(16))) unsigned long long s_iou[BM_MAX_CAND];       // 32 KB
    __shared__ __attribute__((aligned(16))) int s_scratch[BM_THREADS * 2 * BM_SET_WORDS];   // 16 KB: boxes, then the walks' bit sets
    __shared__ unsigned short s_pair[BM_MAX_CAND];                                       // 8 KB
    __shared__ double s_thr[BM_MAX_THR];                  // (the walks index it by a per-thread j)
    __shared__ unsigned s_count;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int64_t r_all = pred_off[n_cells], g_all = gt_off[n_cells];
    const int64_t r0 = pred_off[b], r1 = pred_off[b + 1], g0 = gt_off[b], g1 = gt_off[b + 1];
    if (r0 < 0 || r1 < r0 || r1 > r_all || g0 < 0 || g1 < g0 || g1 > g_all) {            // offsets that name no row: nothing to write to
        if (tid == 0) cell_status[b] = 2;
        return;
    }
    const int R = r1 - r0 < INT32_MAX ? (int)(r1 - r0) : INT32_MAX, G = g1 - g0 < INT32_MAX ? (int)(g1 - g0) : INT32_MAX;
    if (R > cap_pred || G > cap_gt || R > BM_MAX_BOXES || G > BM_MAX_BOXES) {             // the caller's maxima were wrong
        for (int64_t i = tid; i < (int64_t)n_thr * R; i += BM_THREADS) tp[(i / R) * r_all + r0 + i % R] = -1;
        if (tid == 0) cell_status[b] = 2;
        return;
    }
    if (R == 0 || G == 0) {                                                              // no pair: no match
        for (int i = tid; i < n_thr * R; i += BM_THREADS) tp[(int64_t)(i / R) * r_all + r0 + i % R] = 0;
        if (tid == 0) cell_status[b] = 0;
        return;
    }

    // ---- phase 1 --------------------------------------------------------------------------------------------------------
    int4* s_pbox = reinterpret_cast<int4*>(s_scratch);
    int4* s_gbox = s_pbox + BM_MAX_BOXES;
    for (int i = tid; i < R; i += BM_THREADS) s_pbox[i] = *reinterpret_cast<const int4*>(pred_box + (r0 + i) * 4);
    for (int i = tid; i < G; i += BM_THREADS) s_gbox[i] = *reinterpret_cast<const int4*>(gt_box + (g0 + i) * 4);
    if (tid == 0) s_count = 0;
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < BM_MAX_THR; ++j) s_thr[j] = thr.v[j];
    }
    __syncthreads();
    const double thr0 = thr.v[0];
    for (int i = tid; i < R * G; i += BM_THREADS) {
        const int p = i / G, g = i - p * G;
        const int4 pb = s_pbox[p], gb = s_gbox[g];
        if (!box_ok(pb) || !box_ok(gb)) continue;
        const double iou = box_iou(pb, gb);
        if (iou > thr0) {
            const unsigned slot = atomicAdd(&s_count, 1u);
            if (slot < (unsigned)BM_MAX_CAND) {
                s_iou[slot] = (unsigned long long)__double_as_longlong(iou);
                s_pair[slot] = (unsigned short)i;
            }
        }
    }
    __syncthreads();
    const unsigned count = s_count;                       // the same word for every thread
    if (count > (unsigned)BM_MAX_CAND) {
        for (int i = tid; i < n_thr * R; i += BM_THREADS) tp[(int64_t)(i / R) * r_all + r0 + i % R] = -1;
        if (tid == 0) cell_status[b] = 1;
        return;
    }

    // ---- phase 2 --------------------------------------------------------------------------------------------------------
    unsigned n2 = 1;
    while (n2 < count) n2 <<= 1;
    for (unsigned i = count + tid; i < n2; i += BM_THREADS) { s_iou[i] = 0ull; s_pair[i] = 0; }
    __syncthreads();
    for (unsigned k = 2; k <= n2; k <<= 1) {
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned t = tid; t < (n2 >> 1); t += BM_THREADS) {
                const unsigned lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;      // the t-th pair at distance j
                const unsigned long long il = s_iou[lo], ih = s_iou[hi];
                const unsigned pl = s_pair[lo], ph = s_pair[hi];
                const bool forward = (lo & k) == 0;       // this run ends in list order, its neighbour in the reverse
                const bool swap = forward ? cand_before(ih, ph, il, pl) : cand_before(il, pl, ih, ph);
                if (swap) {
                    s_iou[lo] = ih; s_iou[hi] = il;
                    s_pair[lo] = (unsigned short)ph; s_pair[hi] = (unsigned short)pl;
                }
            }
            __syncthreads();
        }
    }

    // ---- phase 3 (the boxes are dead: their LDS holds the bit sets, word w of thread t at [w * BM_THREADS + t]) ------------
    unsigned* s_set = reinterpret_cast<unsigned*>(s_scratch);
    const int walks = n_thr * R;
    for (int w = tid; w < walks; w += BM_THREADS) {
        const int j = w / R, k = w - j * R;
#pragma unroll
        for (int q = 0; q < 2 * BM_SET_WORDS; ++q) s_set[q * BM_THREADS + tid] = 0u;
        const double t = s_thr[j];
        const int most = min(R - k, G);
        int matched = 0;
        for (unsigned i = 0; i < count && matched < most; ++i) {
            if (!(__longlong_as_double((long long)s_iou[i]) > t)) break;
            const int pair = s_pair[i];
            const int p = pair / G, g = pair - p * G;
            if (p < k) continue;
            unsigned* pw = s_set + (p >> 5) * BM_THREADS + tid;
            unsigned* gw = s_set + (BM_SET_WORDS + (g >> 5)) * BM_THREADS + tid;
            const unsigned pbit = 1u << (p & 31), gbit = 1u << (g & 31);
            const unsigned pv = *pw, gv = *gw;
            if ((pv & pbit) || (gv & gbit)) continue;
            *pw = pv | pbit;
            *gw = gv | gbit;
            ++matched;
        }
        tp[(int64_t)j * r_all + r0 + k] = matched;
    }
    if (tid == 0) cell_status[b] = 0;
}

}  // namespace

extern "C" int gte_box_match_max_boxes(void) { return BM_MAX_BOXES; }
extern "C" int gte_box_match_max_candidates(void) { return BM_MAX_CAND; }

extern "C" int gte_box_match(const int32_t* pred_box, const int32_t* pred_off, const int32_t* gt_box, const int32_t* gt_off,
                             int64_t n_cells, int64_t max_pred_per_cell, int64_t max_gt_per_cell, const double* iou_thr, int n_thr,
                             int32_t* tp, int32_t* cell_status, void* stream) {
    if (n_cells < 0 || n_cells >= INT32_MAX || max_pred_per_cell < 0 || max_gt_per_cell < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "box_match: bad sizes");
    if (n_thr < 1 || n_thr > BM_MAX_THR)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "box_match: %d thresholds (1 .. %d)", n_thr, BM_MAX_THR);
    if (!iou_thr) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "box_match: null pointer");
    Thresholds thr{};
    for (int j = 0; j < n_thr; ++j) {
        thr.v[j] = iou_thr[j];
        if (!std::isfinite(thr.v[j]) || thr.v[j] < 0.0 || (j > 0 && thr.v[j] < thr.v[j - 1]))
            return gte::fail(GTE_ERR_INVALID_ARGUMENT, "box_match: the thresholds must be finite, >= 0 and ascending");
    }
    if (max_pred_per_cell > BM_MAX_BOXES || max_gt_per_cell > BM_MAX_BOXES)
        return gte::fail(GTE_ERR_UNSUPPORTED, "box_match: a cell of %lld x %lld boxes exceeds %d a side", (long long)max_pred_per_cell,
                         (long long)max_gt_per_cell, BM_MAX_BOXES);
    if (n_cells == 0) return GTE_OK;
    if (!pred_off || !gt_off || !cell_status || (max_pred_per_cell > 0 && (!pred_box || !tp)) || (max_gt_per_cell > 0 && !gt_box))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "box_match: null pointer");
    if ((((uintptr_t)pred_box | (uintptr_t)gt_box) & 15) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "box_match: pred_box and gt_box must be 16-byte aligned");
    hipLaunchKernelGGL(box_match_kernel, dim3((unsigned)n_cells), dim3(BM_THREADS), 0, gte::as_stream(stream), pred_box, pred_off, gt_box,
                       gt_off, (int)n_cells, (int)max_pred_per_cell, (int)max_gt_per_cell, thr, n_thr, tp, cell_status);
    return gte::check_launch("box_match");
}
