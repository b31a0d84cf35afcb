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
//
// Two instantiations of the one body, by box type.  int32 boxes (gte_box_match): phase 1 as above.  double boxes
// (gte_box_match_f64: the block route's document, coordinates / 0.36): the IoU is calc_iou_individual() of metrics.py:20-54 in
// IEEE double, operation by operation in the reference's order and with contraction OFF -- every intermediate rounds, so the bits
// depend on both (left alone, the compiler fuses the union's last subtraction into an fma) -- and the launch can write every
// pair's IoU out, which is how tests/test_gpu_box_match_f64.py checks those bits.  2 x 256 double boxes are exactly the 16 KB of
// the bit sets; phases 2 and 3 do not know the box type.
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

constexpr double BM_MAX_COORD = 16777216.0;            // |v| of a float box: 2^24
struct Thresholds { double v[BM_MAX_THR]; };
struct alignas(16) BoxF { double x, y, z, w; };       // a float box (x0, y0, x1, y1): two 16-byte halves
template <typename T> struct BoxOf;
template <> struct BoxOf<int32_t> { using type = int4; };
template <> struct BoxOf<double> { using type = BoxF; };
static_assert(2 * BM_MAX_BOXES * sizeof(BoxF) <= BM_THREADS * 2 * BM_SET_WORDS * 4, "the float boxes fit the bit sets' LDS");

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

// a float box is well formed when its four values are finite and within +-2^24 and its corners are in order (a NaN fails every
// comparison); any other box overlaps nothing
__device__ __forceinline__ bool box_ok(const BoxF& b) {
    return fabs(b.x) <= BM_MAX_COORD && fabs(b.y) <= BM_MAX_COORD && fabs(b.z) <= BM_MAX_COORD && fabs(b.w) <= BM_MAX_COORD &&
           b.x <= b.z && b.y <= b.w;
}

// metrics.py:42-53 on doubles: one rounding per operation, in the reference's order (np.min / np.max of two finite values pick one
// of them: no rounding)
__device__ __forceinline__ double box_iou(const BoxF& p, const BoxF& t) {
#pragma clang fp contract(off)
    if (t.z < p.x || p.z < t.x || t.w < p.y || p.w < t.y) return 0.0;
    const double far_x = t.z < p.z ? t.z : p.z, near_x = t.x > p.x ? t.x : p.x;
    const double far_y = t.w < p.w ? t.w : p.w, near_y = t.y > p.y ? t.y : p.y;
    const double inter = ((far_x - near_x) + 1.0) * ((far_y - near_y) + 1.0);
    const double ta = ((t.z - t.x) + 1.0) * ((t.w - t.y) + 1.0);
    const double pa = ((p.z - p.x) + 1.0) * ((p.w - p.y) + 1.0);
    return inter / ((ta + pa) - inter);
}

// list order: IoU descending, then pair index descending
__device__ __forceinline__ bool cand_before(unsigned long long ia, unsigned pa, unsigned long long ib, unsigned pb) {
    return ia > ib || (ia == ib && pa > pb);
}

// grid = cells.  T = int32_t or double, the boxes' type; iou_out / iou_off: the double instantiation's optional IoU matrices
template <typename T>
__global__ void __launch_bounds__(BM_THREADS)
box_match_kernel(const T* __restrict__ pred_box, const int32_t* __restrict__ pred_off, const T* __restrict__ gt_box,
                 const int32_t* __restrict__ gt_off, int n_cells, int cap_pred, int cap_gt, Thresholds thr, int n_thr,
                 int32_t* __restrict__ tp, int32_t* __restrict__ cell_status, double* __restrict__ iou_out,
                 const int64_t* __restrict__ iou_off) {
    constexpr bool F64 = sizeof(T) == 8;
    using Box = typename BoxOf<T>::type;
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
    int64_t i0 = 0;
    bool iou_rows = true;                                 // the cell's IoU matrix has its R x G rows inside [0, iou_off[n_cells]]
    if constexpr (F64) {
        if (iou_out) {
            i0 = iou_off[b];
            iou_rows = i0 >= 0 && iou_off[b + 1] - i0 == (int64_t)R * G && iou_off[b + 1] <= iou_off[n_cells];
        }
    }
    if (R > cap_pred || G > cap_gt || R > BM_MAX_BOXES || G > BM_MAX_BOXES || !iou_rows) {   // the caller's maxima / offsets were wrong
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
    Box* s_pbox = reinterpret_cast<Box*>(s_scratch);
    Box* s_gbox = s_pbox + BM_MAX_BOXES;
    for (int i = tid; i < R; i += BM_THREADS) s_pbox[i] = *reinterpret_cast<const Box*>(pred_box + (r0 + i) * 4);
    for (int i = tid; i < G; i += BM_THREADS) s_gbox[i] = *reinterpret_cast<const Box*>(gt_box + (g0 + i) * 4);
    if (tid == 0) s_count = 0;
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < BM_MAX_THR; ++j) s_thr[j] = thr.v[j];
    }
    __syncthreads();
    const double thr0 = thr.v[0];
    for (int i = tid; i < R * G; i += BM_THREADS) {
        const int p = i / G, g = i - p * G;
        const Box pb = s_pbox[p], gb = s_gbox[g];
        const bool ok = box_ok(pb) && box_ok(gb);
        const double iou = ok ? box_iou(pb, gb) : 0.0;
        if constexpr (F64) {
            if (iou_out) iou_out[i0 + i] = iou;           // every pair, whatever the thresholds
            if (!isfinite(iou)) continue;                 // a non-finite quotient is no candidate
        }
        if (ok && iou > thr0) {
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

namespace {

// the checks and the launch of both entries (double boxes: + the two IoU arguments)
template <typename T>
int box_match_launch(const char* what, const T* pred_box, const int32_t* pred_off, const T* gt_box, const int32_t* gt_off, int64_t n_cells,
                     int64_t max_pred_per_cell, int64_t max_gt_per_cell, const double* iou_thr, int n_thr, int32_t* tp,
                     int32_t* cell_status, double* iou, const int64_t* iou_off, void* stream) {
    if (n_cells < 0 || n_cells >= INT32_MAX || max_pred_per_cell < 0 || max_gt_per_cell < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: bad sizes", what);
    if (n_thr < 1 || n_thr > BM_MAX_THR)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: %d thresholds (1 .. %d)", what, n_thr, BM_MAX_THR);
    if (!iou_thr) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    Thresholds thr{};
    for (int j = 0; j < n_thr; ++j) {
        thr.v[j] = iou_thr[j];
        if (!std::isfinite(thr.v[j]) || thr.v[j] < 0.0 || (j > 0 && thr.v[j] < thr.v[j - 1]))
            return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: the thresholds must be finite, >= 0 and ascending", what);
    }
    if (max_pred_per_cell > BM_MAX_BOXES || max_gt_per_cell > BM_MAX_BOXES)
        return gte::fail(GTE_ERR_UNSUPPORTED, "%s: a cell of %lld x %lld boxes exceeds %d a side", what, (long long)max_pred_per_cell,
                         (long long)max_gt_per_cell, BM_MAX_BOXES);
    if (n_cells == 0) return GTE_OK;
    if (!pred_off || !gt_off || !cell_status || (max_pred_per_cell > 0 && (!pred_box || !tp)) || (max_gt_per_cell > 0 && !gt_box) ||
        (iou && !iou_off))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if ((((uintptr_t)pred_box | (uintptr_t)gt_box) & 15) != 0 || ((uintptr_t)iou & 7) != 0 || ((uintptr_t)iou_off & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: pred_box and gt_box must be 16-byte aligned (iou and iou_off 8-byte)", what);
    hipLaunchKernelGGL(box_match_kernel<T>, dim3((unsigned)n_cells), dim3(BM_THREADS), 0, gte::as_stream(stream), pred_box, pred_off, gt_box,
                       gt_off, (int)n_cells, (int)max_pred_per_cell, (int)max_gt_per_cell, thr, n_thr, tp, cell_status, iou, iou_off);
    return gte::check_launch(what);
}

}  // namespace

extern "C" int gte_box_match(const int32_t* pred_box, const int32_t* pred_off, const int32_t* gt_box, const int32_t* gt_off,
                             int64_t n_cells, int64_t max_pred_per_cell, int64_t max_gt_per_cell, const double* iou_thr, int n_thr,
                             int32_t* tp, int32_t* cell_status, void* stream) {
    return box_match_launch<int32_t>("box_match", pred_box, pred_off, gt_box, gt_off, n_cells, max_pred_per_cell, max_gt_per_cell, iou_thr,
                                     n_thr, tp, cell_status, nullptr, nullptr, stream);
}

extern "C" int gte_box_match_f64(const double* pred_box, const int32_t* pred_off, const double* gt_box, const int32_t* gt_off,
                                 int64_t n_cells, int64_t max_pred_per_cell, int64_t max_gt_per_cell, const double* iou_thr, int n_thr,
                                 int32_t* tp, int32_t* cell_status, double* iou, const int64_t* iou_off, void* stream) {
    return box_match_launch<double>("box_match_f64", pred_box, pred_off, gt_box, gt_off, n_cells, max_pred_per_cell, max_gt_per_cell,
                                    iou_thr, n_thr, tp, cell_status, iou, iou_off, stream);
}
