// Table grids: the rows, columns and cells of the tables whose words another stage has named -- the classical
// projection profile, stated as exact integer arithmetic.
//
// No reference counterpart: the reference stops at where a table is (get_tables_bbox; get_subgraph_bbox() is a stub).  The contract
// is the rule in include/gte.h; tests/table_grid_ref.py (numpy: a boolean occupancy array and the cumsum of its run starts, written
// from that rule) is the oracle, every output is an integer and compared exactly.
//
// Structure.  One workgroup per listed table.  It scans the words of the table's page for its members three times (the page has
// no image in LDS: only the two profiles live there, so a page may have any number of words):
//   reduce   min lo / max hi1 per axis, the member count and the coordinate range, thread-local first, then one LDS integer atomic
//            per thread and value;
//   mark     every profile word ORs the word-wise masks of its pixels [lo, hi1 + gap) - origin into the axis' bitmap (LDS atomic-or);
//   span     every member looks up the bands of the first and last occupied pixel inside [lo, hi1) and the ends of their runs.
// Between mark and span, per axis: first[w] = occ[w] & ~(occ[w] << 1 | carry of occ[w - 1]) holds a bit where a run starts, and
// pre[w] = the number of run starts in the words below w (one wave per axis: five words per lane, a shuffle scan over the lanes).
// The band of an occupied pixel p is then pre[p / 32] + popcount(first[p / 32] up to bit p % 32) - 1.
//
// Every loop has a bound known before it starts -- the page's nodes, the GRID_WORDS words of a bitmap -- and none waits on
// another thread's write: a logic error ends in a wrong answer, never in a hang.  All arithmetic is integer, every LDS atomic is
// min / max / add / or: the order of arrival does not matter and two runs give the same bits.  A bitmap index is always
// coordinate - origin with 0 <= index < extent + gap <= GRID_BITS, established by the status-2 test before the first bitmap access.
#include "gte_common.h"

#include <climits>

namespace {

constexpr int GRID_MAX_EXTENT = 8192;                     // pixels per axis between the first and the last member pixel
constexpr int GRID_MAX_GAP = 1024;
constexpr int GRID_BITS = GRID_MAX_EXTENT + GRID_MAX_GAP;
constexpr int GRID_WORDS = GRID_BITS / 32;                // 288 bitmap words per axis
constexpr int GRID_THREADS = 256;
constexpr int GRID_LANE_WORDS = (GRID_WORDS + gte::kWave - 1) / gte::kWave;      // words per lane of the scan: 5
constexpr int GRID_COORD_MAX = 1 << 30;                   // |coordinate| above it: status 2 (lo + 1 and hi + gap stay inside int32)
static_assert(GRID_BITS % 32 == 0, "a bitmap is whole words");
static_assert(GRID_THREADS >= 2 * gte::kWave, "one wave per axis scans the run starts");
// static LDS: occ, first, pre per axis (6 x 288 words = 6 912 bytes) + the reduction words

enum { RED_MIN_X, RED_MIN_Y, RED_MAX_X, RED_MAX_Y, RED_COUNT, RED_N };

// bits lo .. hi (inclusive, 0 <= lo <= hi <= 31) of a word; no shift by the word width
__device__ __forceinline__ uint32_t bits_between(int lo, int hi) { return (0xFFFFFFFFu << lo) & (0xFFFFFFFFu >> (31 - hi)); }

// a member's interval on one axis: lo = min, hi1 = max(max, lo + 1) of the two corners (unsigned add: no overflow trap; a table
// whose coordinates leave +-2^30 ends with status 2 before lo + 1 is used for anything)
__device__ __forceinline__ void interval(int a, int b, int& lo, int& hi1) {
    lo = min(a, b);
    hi1 = max(max(a, b), (int)((unsigned)lo + 1u));
}

// OR the pixels [a, b) into the bitmap (0 <= a < b <= GRID_BITS)
__device__ __forceinline__ void mark(uint32_t* occ, int a, int b) {
    const int w0 = a >> 5, w1 = (b - 1) >> 5;
    for (int w = w0; w <= w1; ++w)
        atomicOr(occ + w, bits_between(w == w0 ? (a & 31) : 0, w == w1 ? ((b - 1) & 31) : 31));
}

// (c0, c1, start of band c0, end of band c1 before the gap is taken off) of the pixels [a, b) (0 <= a < b <= GRID_BITS); false when
// none of them is occupied
__device__ __forceinline__ bool span(const uint32_t* occ, const uint32_t* first, const int* pre, int a, int b, int& c0, int& c1,
                                     int& start, int& end) {
    const int w0 = a >> 5, w1 = (b - 1) >> 5;
    int f = -1, l = -1;                                   // first / last occupied pixel inside [a, b)
    for (int w = w0; w <= w1; ++w) {
        const uint32_t m = occ[w] & bits_between(w == w0 ? (a & 31) : 0, w == w1 ? ((b - 1) & 31) : 31);
        if (m) { f = (w << 5) + __ffs((int)m) - 1; break; }
    }
    if (f < 0) return false;
    for (int w = w1; w >= w0; --w) {
        const uint32_t m = occ[w] & bits_between(w == w0 ? (a & 31) : 0, w == w1 ? ((b - 1) & 31) : 31);
        if (m) { l = (w << 5) + 31 - __clz((int)m); break; }
    }
    c0 = pre[f >> 5] + __popc(first[f >> 5] & bits_between(0, f & 31)) - 1;
    c1 = pre[l >> 5] + __popc(first[l >> 5] & bits_between(0, l & 31)) - 1;
    start = 0;                                            // the run start at or below f (f is occupied: there is one)
    for (int w = f >> 5; w >= 0; --w) {
        const uint32_t m = first[w] & (w == (f >> 5) ? bits_between(0, f & 31) : 0xFFFFFFFFu);
        if (m) { start = (w << 5) + 31 - __clz((int)m); break; }
    }
    end = GRID_BITS;                                      // the first free pixel above l (a run may reach the bitmap's last bit)
    for (int w = l >> 5; w < GRID_WORDS; ++w) {
        const uint32_t m = ~occ[w] & (w == (l >> 5) ? bits_between(l & 31, 31) : 0xFFFFFFFFu);
        if (m) { end = (w << 5) + __ffs((int)m) - 1; break; }
    }
    return true;
}

// grid = listed tables
__global__ void __launch_bounds__(GRID_THREADS)
table_grid_kernel(const int32_t* __restrict__ bbox, const int32_t* __restrict__ node_off, int n_pages, int n_nodes,
                  const int32_t* __restrict__ table, const int32_t* __restrict__ role, const int32_t* __restrict__ table_root,
                  const int32_t* __restrict__ table_page, const int32_t* __restrict__ table_gap, uint32_t col_roles,
                  uint32_t row_roles, int32_t* __restrict__ cell, int32_t* __restrict__ cell_box, int32_t* __restrict__ table_shape,
                  int32_t* __restrict__ table_box, int32_t* __restrict__ table_words, int32_t* __restrict__ table_status) {
    __shared__ uint32_t occ[2][GRID_WORDS];               // [0]: x axis (columns), [1]: y axis (rows)
    __shared__ uint32_t first[2][GRID_WORDS];
    __shared__ int pre[2][GRID_WORDS];
    __shared__ int red[RED_N];
    __shared__ int bands[2];
    const int tid = threadIdx.x, t = blockIdx.x;
    const int root = table_root[t], page = table_page[t];
    const int gap_x = table_gap[2 * t], gap_y = table_gap[2 * t + 1];
    const int4 zero4 = make_int4(0, 0, 0, 0);

    // every exit below is taken by the whole workgroup: the values it depends on are the same for every thread
    auto finish = [&](int status, int n_rows, int n_cols, int4 box, int words) {
        if (tid == 0) {
            table_shape[2 * t] = n_rows;
            table_shape[2 * t + 1] = n_cols;
            *reinterpret_cast<int4*>(table_box + (int64_t)t * 4) = box;
            table_words[t] = words;
            table_status[t] = status;
        }
    };
    if (page < 0 || page >= n_pages) { finish(3, 0, 0, zero4, 0); return; }
    const int n0 = node_off[page], n1 = node_off[page + 1];
    if (n0 < 0 || n1 > n_nodes || n1 < n0) { finish(3, 0, 0, zero4, 0); return; }
    const int np = root >= 0 ? n1 - n0 : 0;               // (a negative id names no table: table[v] < 0 is "none")

    if (tid == 0) {
        red[RED_MIN_X] = INT_MAX; red[RED_MIN_Y] = INT_MAX; red[RED_MAX_X] = INT_MIN; red[RED_MAX_Y] = INT_MIN; red[RED_COUNT] = 0;
    }
    for (int w = tid; w < GRID_WORDS; w += GRID_THREADS) { occ[0][w] = 0u; occ[1][w] = 0u; }
    __syncthreads();

    // reduce
    {
        int mnx = INT_MAX, mny = INT_MAX, mxx = INT_MIN, mxy = INT_MIN, cnt = 0;
        for (int j = tid; j < np; j += GRID_THREADS) {
            if (table[n0 + j] != root) continue;
            const int4 b = *reinterpret_cast<const int4*>(bbox + (int64_t)(n0 + j) * 4);
            int lo, hi1;
            interval(b.x, b.z, lo, hi1);
            mnx = min(mnx, lo); mxx = max(mxx, hi1);
            interval(b.y, b.w, lo, hi1);
            mny = min(mny, lo); mxy = max(mxy, hi1);
            ++cnt;
        }
        if (cnt) {
            atomicMin(red + RED_MIN_X, mnx); atomicMin(red + RED_MIN_Y, mny);
            atomicMax(red + RED_MAX_X, mxx); atomicMax(red + RED_MAX_Y, mxy);
            atomicAdd(red + RED_COUNT, cnt);
        }
    }
    __syncthreads();
    const int ox = red[RED_MIN_X], oy = red[RED_MIN_Y], ex = red[RED_MAX_X], ey = red[RED_MAX_Y], words = red[RED_COUNT];
    if (words == 0) { finish(1, 0, 0, zero4, 0); return; }
    // min lo is the smallest and max hi1 (> every lo, >= every hi) the largest value the table holds: the range test needs no more.
    // Inside the range the two differences below cannot overflow.
    const bool in_range = min(ox, oy) >= -GRID_COORD_MAX && max(ex, ey) <= GRID_COORD_MAX;
    const bool fits = in_range && ex - ox <= GRID_MAX_EXTENT && ey - oy <= GRID_MAX_EXTENT && gap_x >= 0 && gap_x <= GRID_MAX_GAP &&
                      gap_y >= 0 && gap_y <= GRID_MAX_GAP;
    if (!fits) {                                          // status 2: no grid; the members' rows say so
        for (int j = tid; j < np; j += GRID_THREADS) {
            if (table[n0 + j] != root) continue;
            *reinterpret_cast<int4*>(cell + (int64_t)(n0 + j) * 4) = make_int4(-1, -1, -1, -1);
            *reinterpret_cast<int4*>(cell_box + (int64_t)(n0 + j) * 4) = zero4;
        }
        finish(2, 0, 0, in_range ? make_int4(ox, oy, ex, ey) : zero4, words);
        return;
    }

    // mark: lo - origin >= 0 and hi1 + gap - origin <= extent + gap <= GRID_BITS
    for (int j = tid; j < np; j += GRID_THREADS) {
        if (table[n0 + j] != root) continue;
        const int r = role[n0 + j];
        if ((unsigned)r >= 32u) continue;
        const bool in_x = (col_roles >> r) & 1u, in_y = (row_roles >> r) & 1u;
        if (!in_x && !in_y) continue;
        const int4 b = *reinterpret_cast<const int4*>(bbox + (int64_t)(n0 + j) * 4);
        int lo, hi1;
        if (in_x) { interval(b.x, b.z, lo, hi1); mark(occ[0], lo - ox, hi1 + gap_x - ox); }
        if (in_y) { interval(b.y, b.w, lo, hi1); mark(occ[1], lo - oy, hi1 + gap_y - oy); }
    }
    __syncthreads();

    // run starts and their exclusive scan: wave 0 the x axis, wave 1 the y axis, lane l the words 5 l .. 5 l + 4
    if (tid < 2 * gte::kWave) {
        const int axis = tid / gte::kWave, lane = tid % gte::kWave;
        uint32_t st[GRID_LANE_WORDS];
        int mine = 0;
#pragma unroll
        for (int k = 0; k < GRID_LANE_WORDS; ++k) {
            const int w = lane * GRID_LANE_WORDS + k;
            st[k] = 0u;
            if (w < GRID_WORDS) {
                const uint32_t o = occ[axis][w], below = w > 0 ? occ[axis][w - 1] >> 31 : 0u;
                st[k] = o & ~((o << 1) | below);
            }
            mine += __popc(st[k]);
        }
        int incl = mine;                                  // inclusive scan over the wave's 64 lanes
#pragma unroll
        for (int d = 1; d < gte::kWave; d <<= 1) {
            const int up = __shfl_up(incl, d, gte::kWave);
            if (lane >= d) incl += up;
        }
        int run = incl - mine;
#pragma unroll
        for (int k = 0; k < GRID_LANE_WORDS; ++k) {
            const int w = lane * GRID_LANE_WORDS + k;
            if (w < GRID_WORDS) { first[axis][w] = st[k]; pre[axis][w] = run; }
            run += __popc(st[k]);
        }
        if (lane == gte::kWave - 1) bands[axis] = incl;
    }
    __syncthreads();

    // span: every member, profile word or not
    for (int j = tid; j < np; j += GRID_THREADS) {
        if (table[n0 + j] != root) continue;
        const int4 b = *reinterpret_cast<const int4*>(bbox + (int64_t)(n0 + j) * 4);
        int lo, hi1, c0 = -1, c1 = -1, r0 = -1, r1 = -1, xs = 0, xe = 0, ys = 0, ye = 0;      // (span leaves them alone when it finds no pixel)
        interval(b.x, b.z, lo, hi1);
        if (span(occ[0], first[0], pre[0], lo - ox, hi1 - ox, c0, c1, xs, xe)) { xs += ox; xe += ox - gap_x; }
        interval(b.y, b.w, lo, hi1);
        if (span(occ[1], first[1], pre[1], lo - oy, hi1 - oy, r0, r1, ys, ye)) { ys += oy; ye += oy - gap_y; }
        *reinterpret_cast<int4*>(cell + (int64_t)(n0 + j) * 4) = make_int4(r0, r1, c0, c1);
        *reinterpret_cast<int4*>(cell_box + (int64_t)(n0 + j) * 4) = make_int4(xs, ys, xe, ye);
    }
    finish(0, bands[1], bands[0], make_int4(ox, oy, ex, ey), words);
}

}  // namespace

extern "C" int gte_table_grid_max_extent(void) { return GRID_MAX_EXTENT; }
extern "C" int gte_table_grid_max_gap(void) { return GRID_MAX_GAP; }

extern "C" int gte_table_grid(const int32_t* bbox, const int32_t* node_off, int64_t n_pages, int64_t n_nodes, const int32_t* table,
                              const int32_t* role, const int32_t* table_root, const int32_t* table_page, const int32_t* table_gap,
                              int64_t n_tables, uint32_t col_roles, uint32_t row_roles, int32_t* cell, int32_t* cell_box,
                              int32_t* table_shape, int32_t* table_box, int32_t* table_words, int32_t* table_status, void* stream) {
    const char* what = "table_grid";
    if (n_pages < 0 || n_nodes < 0 || n_tables < 0 || n_pages >= INT32_MAX || n_nodes >= INT32_MAX || (n_pages == 0 && n_nodes > 0))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: bad sizes", what);
    if (n_tables >= INT32_MAX)
        return gte::fail(GTE_ERR_UNSUPPORTED, "%s: %lld tables exceed one launch's grid", what, (long long)n_tables);
    if (n_tables == 0) return GTE_OK;
    if (!node_off || !table_root || !table_page || !table_gap || !table_shape || !table_box || !table_words || !table_status ||
        (n_nodes > 0 && (!bbox || !table || !role || !cell || !cell_box)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if ((((uintptr_t)bbox | (uintptr_t)cell | (uintptr_t)cell_box | (uintptr_t)table_box) & 15) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: bbox, cell, cell_box and table_box must be 16-byte aligned", what);
    hipLaunchKernelGGL(table_grid_kernel, dim3((unsigned)n_tables), dim3(GRID_THREADS), 0, gte::as_stream(stream), bbox, node_off,
                       (int)n_pages, (int)n_nodes, table, role, table_root, table_page, table_gap, col_roles, row_roles, cell,
                       cell_box, table_shape, table_box, table_words, table_status);
    return gte::check_launch(what);
}
