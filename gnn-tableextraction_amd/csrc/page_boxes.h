// The shared pieces of the page-box kernels (block_vote.hip, block_scores.hip, word_labels.hip): one workgroup per page, the
// page's rectangles in an LDS table, the page's words strided over the workgroup.
//
// The table is [rows][4] doubles, read back as double2 corner pairs: [2 j] = (lo x, lo y), [2 j + 1] = (hi x, hi y).  A word tests
// kScan rows between two looks at its result -- the rows' loads are independent of the tests; a scan that left after every row
// would wait for one LDS round trip per row -- and every lane reads the same address, a broadcast.  So a table always holds whole
// scan groups: the rows behind the page's last rectangle are quiet NaNs, and so is a rectangle that must meet nothing.  Every
// comparison with a NaN is false: such a row is never a hit and needs no index test.  The tests are four fp64 comparisons on
// values that are exact (int32 -> double) or the caller's own doubles: no arithmetic, nothing to round.
#pragma once
#include "gte_common.h"

namespace page_boxes {

constexpr int kThreads = 1024;                        // per page workgroup: a page has hundreds of words, the largest a few thousand
constexpr int kMaxBlocks = 512;                       // per page
constexpr int kMaxCat = 16;
constexpr int kScan = 4;                              // rows a word tests between two looks at its result
constexpr int kRowBytes = 4 * 8;
static_assert(kMaxBlocks % kScan == 0, "the largest page is whole scan groups");

__host__ __device__ inline int scan_rows(int n) { return (n + kScan - 1) / kScan * kScan; }
// bytes of a table that takes up to `cap` rectangles
__host__ __device__ inline size_t table_bytes(int cap) { return (size_t)scan_rows(cap) * kRowBytes; }

// a page's run [lo, hi) of an array of n rows, as its offsets give it
__device__ __forceinline__ bool run_ok(int lo, int hi, int n) { return lo >= 0 && hi >= lo && hi <= n; }

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ const double2* corners(const double* s_box) { return reinterpret_cast<const double2*>(s_box); }

// rows [n, scan_rows(n)) of the table: rectangles that meet nothing.  The caller owns the barrier.
__device__ __forceinline__ void pad_scan_group(double* s_box, int n) {
    for (int i = n * 4 + threadIdx.x; i < scan_rows(n) * 4; i += kThreads) s_box[i] = quiet_nan();
}

// rows [0, B) of the table from the rectangles src[B][4], corners normalised: (min x, min y, max x, max y), four NaNs for a
// rectangle with a NaN corner; the padding behind them.  The caller owns the barrier.
__device__ __forceinline__ void stage_normalised(double* s_box, const double* __restrict__ src, int B) {
    const double q = quiet_nan();
    for (int i = threadIdx.x; i < B; i += kThreads) {
        const double x0 = src[i * 4 + 0], y0 = src[i * 4 + 1], x1 = src[i * 4 + 2], y1 = src[i * 4 + 3];
        const bool nan = x0 != x0 || y0 != y0 || x1 != x1 || y1 != y1;
        s_box[i * 4 + 0] = nan ? q : (x0 < x1 ? x0 : x1);
        s_box[i * 4 + 1] = nan ? q : (y0 < y1 ? y0 : y1);
        s_box[i * 4 + 2] = nan ? q : (x0 < x1 ? x1 : x0);
        s_box[i * 4 + 3] = nan ? q : (y0 < y1 ? y1 : y0);
    }
    pad_scan_group(s_box, B);
}

// The closed test of a word's rectangle (row `row` of bbox[.][4]: one int4 load, min / max per axis) against a normalised row:
// max(lo, lo') <= min(hi, hi') on both axes, with lo <= hi on either side -- touching counts.
struct Meets {
    double x0, y0, x1, y1;
    __device__ __forceinline__ Meets(const int32_t* __restrict__ bbox, int64_t row) {
        const int4 w = *reinterpret_cast<const int4*>(bbox + row * 4);
        x0 = (double)min(w.x, w.z); y0 = (double)min(w.y, w.w); x1 = (double)max(w.x, w.z); y1 = (double)max(w.y, w.w);
    }
    __device__ __forceinline__ bool operator()(double2 lo, double2 hi) const {
        return lo.x <= x1 && x0 <= hi.x && lo.y <= y1 && y0 <= hi.y;
    }
};

// The strict test of a point against a row AS GIVEN (a row whose corners are the other way round holds nothing).
struct HoldsCentre {
    double cx, cy;
    __device__ __forceinline__ bool operator()(double2 lo, double2 hi) const { return cx > lo.x && cx < hi.x && cy > lo.y && cy < hi.y; }
};

// The lowest of the table's first n rows that `test` accepts, -1 for none: a scan group at a time, descending inside a group so
// that the lowest hit survives, leaving after the group with the first hit.
template <typename Test>
__device__ __forceinline__ int first_hit(const double2* s_corner, int n, const Test& test) {
    int hit = -1;
    for (int j0 = 0; j0 < n && hit < 0; j0 += kScan) {
#pragma unroll
        for (int u = kScan - 1; u >= 0; --u)
            if (test(s_corner[2 * (j0 + u)], s_corner[2 * (j0 + u) + 1])) hit = j0 + u;
    }
    return hit;
}

// ---- host: the entries' shared argument checks ----
template <typename... T>
inline bool counts_ok(T... count) { return ((count >= 0 && count < INT32_MAX) && ...); }      // every count indexes with an int32
inline bool boxes_aligned(const void* bbox, const void* rect) { return ((uintptr_t)bbox & 15) == 0 && ((uintptr_t)rect & 7) == 0; }
// rectangles the launch's table takes per page, from the caller's max_page_blocks (a launch always carries one scan group)
inline int page_cap(int64_t max_page_blocks) { return max_page_blocks > 0 ? (int)max_page_blocks : 1; }

}  // namespace page_boxes
