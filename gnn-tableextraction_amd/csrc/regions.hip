// Page regions from node predictions: connected components of the page graph restricted to words of one
// predicted kind, and the union box of every component.
//
// No reference counterpart: src/components/graphs/utils.py get_subgraph_bbox() is a stub ("still need to understand how to extract
// bbox from subgraphs"), and postprocessing.py votes over PyMuPDF blocks instead (out of scope).  The contract is the
// definition in include/gte.h; tests/regions_ref.py (a numpy union-find written from it) is the oracle, every output is an
// integer and compared exactly.
//
// Structure.  One workgroup per page (pages are block-diagonal: a component never leaves its page), the page-local labels, the
// groups and the per-root accumulators in LDS.  lbl[v] starts at v and only ever decreases, and it always names a node of v's own
// component, so min(component) is the only fixed point.  A round
//   hook   every CSR entry u -> v with group[u] == group[v] takes m = min(lbl[u], lbl[v]) onto BOTH endpoints and onto the larger of
//          the two labels (LDS atomic-min): the direction of the entry does not matter, a directed CSR gives the answer of its
//          symmetric closure;
//   jump   lbl[v] = the fixed point of the chain lbl[lbl[...]] (strictly decreasing, so it ends);
// and the rounds stop after the first hook pass that found every entry's endpoints equal.  Plain label propagation alone settles in
// <= diameter rounds, the hook onto the larger label and the jump only speed that up, so nodes + 1 rounds always suffice: that is
// the loop's hard bound -- a logic error ends in a wrong answer, never in a hang.  The exit decision is one LDS word (one per
// round parity) that every thread reads behind the barrier: the loop is uniform and no barrier stands under divergent control.
// Counts and boxes are reduced per root with LDS atomics (integer add / min / max: order-free, deterministic).
//
// The SCORED instantiation (gte_page_regions_scored) adds a region confidence in the same launch: every member word adds the
// softmax mass its logits give to the classes of its own kind, in 2^-19 fixed point, to one more LDS word of its root (an integer
// add: the sum does not depend on the arrival order), and the root row receives the mean.  Everything else is the one body.
#include "gte_common.h"
#include "word_score.h"

#include <climits>

namespace {

constexpr int REGION_PAGE_MAX = 4096;                 // == the k-NN builder's page limit (knn_graph.hip: KNN_PAGE_MAX)
constexpr int REGION_THREADS = 256;
// LDS of a page of `cap` nodes: box[cap] (int4: min x0, min y0, max x1, max y1), lbl[cap], grp[cap], cnt[cap], flag[2] (+ pad)
// (+ acc[cap], the fixed-point score sums, in the SCORED instantiation only: it follows flag, so the plain layout is unchanged)
constexpr int REGION_NODE_BYTES = 16 + 4 + 4 + 4;
constexpr int REGION_SCORE_BYTES = 4;
constexpr int REGION_TAIL_BYTES = 16;
constexpr int region_node_bytes(bool scored) { return REGION_NODE_BYTES + (scored ? REGION_SCORE_BYTES : 0); }
constexpr int REGION_LDS_MAX = REGION_PAGE_MAX * REGION_NODE_BYTES + REGION_TAIL_BYTES;      // 114 704 of the CU's 160 KB
constexpr int REGION_LDS_MAX_SCORED = REGION_PAGE_MAX * region_node_bytes(true) + REGION_TAIL_BYTES;      // 131 088
static_assert(REGION_LDS_MAX_SCORED <= 160 * 1024, "a page of REGION_PAGE_MAX nodes must fit the CU's LDS");
// (the fixed-point word score q(v) = p(v) * 2^19 rounded and its 32-bit sum bound: word_score.h)
constexpr float REGION_SCORE_ONE = GTE_SCORE_ONE;
static_assert(REGION_PAGE_MAX <= GTE_SCORE_PAGE_MAX, "the fixed-point sum must fit 32 bits");

__device__ __forceinline__ int lds_get(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_put(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// grid = pages.  cap = the caller's max_page_nodes (the LDS the launch carries).
template <bool SCORED>
__global__ void __launch_bounds__(REGION_THREADS)
page_regions_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices, const int32_t* __restrict__ node_off,
                    const int32_t* __restrict__ group, const int32_t* __restrict__ bbox, int cap, int n_nodes,
                    int32_t* __restrict__ comp, int32_t* __restrict__ region_box, int32_t* __restrict__ region_count,
                    const float* __restrict__ logits, int n_classes, const int32_t* __restrict__ class_group,
                    float* __restrict__ region_score) {
    extern __shared__ __attribute__((aligned(16))) int smem[];
    int* box = smem;
    int* lbl = smem + 4 * cap;
    int* grp = lbl + cap;
    int* cnt = grp + cap;
    int* flag = cnt + cap;
    unsigned* acc = reinterpret_cast<unsigned*>(flag + REGION_TAIL_BYTES / 4);      // SCORED only
    const int tid = threadIdx.x;
    const int n0 = node_off[blockIdx.x], n1 = node_off[blockIdx.x + 1];
    if (n0 < 0 || n1 > n_nodes || n1 <= n0) return;       // an empty page (or offsets that name no row of the outputs)
    const int np = n1 - n0;
    const int4 zero4 = make_int4(0, 0, 0, 0);
    if (np > cap) {                                       // the caller's max_page_nodes was wrong: no LDS for this page -- no regions
        for (int j = tid; j < np; j += REGION_THREADS) {
            comp[n0 + j] = -1;
            region_count[n0 + j] = 0;
            *reinterpret_cast<int4*>(region_box + (int64_t)(n0 + j) * 4) = zero4;
            if constexpr (SCORED) region_score[n0 + j] = 0.f;
        }
        return;
    }
    for (int j = tid; j < np; j += REGION_THREADS) {
        lbl[j] = j;
        grp[j] = group[n0 + j];
        cnt[j] = 0;
        if constexpr (SCORED) acc[j] = 0u;
        *reinterpret_cast<int4*>(box + 4 * j) = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
    }
    if (tid == 0) { flag[0] = 0; flag[1] = 0; }
    __syncthreads();

    for (int round = 0; round <= np; ++round) {
        bool changed = false;
        for (int v = tid; v < np; v += REGION_THREADS) {
            const int gv = grp[v];
            if (gv < 0) continue;
            const int e1 = indptr[n0 + v + 1];
            for (int e = indptr[n0 + v]; e < e1; ++e) {
                const int u = indices[e] - n0;
                if ((unsigned)u >= (unsigned)np || u == v) continue;      // outside the page: never an LDS address
                if (grp[u] != gv) continue;
                const int lu = lds_get(lbl + u), lv = lds_get(lbl + v);
                if (lu == lv) continue;
                const int m = min(lu, lv);
                atomicMin(lbl + u, m);
                atomicMin(lbl + v, m);
                atomicMin(lbl + max(lu, lv), m);          // (a label is a node of the same component: hooks its tree as well)
                changed = true;
            }
        }
        if (changed) lds_put(flag + (round & 1), 1);
        __syncthreads();
        const int again = flag[round & 1];                // the same word for every thread: a uniform exit
        if (tid == 0) flag[(round + 1) & 1] = 0;          // (nobody reads or sets the other parity's word before the next barrier)
        if (!again) break;
        for (int v = tid; v < np; v += REGION_THREADS) {
            if (grp[v] < 0) continue;
            int l = lds_get(lbl + v);
            for (;;) {                                    // lbl[x] <= x: the chain falls strictly until its fixed point
                const int ll = lds_get(lbl + l);
                if (ll == l) break;
                l = ll;
            }
            lds_put(lbl + v, l);
        }
        __syncthreads();
    }

    // every label is now its component's smallest node: members add themselves to their root's count and box
    for (int j = tid; j < np; j += REGION_THREADS) {
        if (grp[j] < 0) continue;
        const int r = lbl[j];
        const int4 b = *reinterpret_cast<const int4*>(bbox + (int64_t)(n0 + j) * 4);
        atomicAdd(cnt + r, 1);
        atomicMin(box + 4 * r + 0, b.x);
        atomicMin(box + 4 * r + 1, b.y);
        atomicMax(box + 4 * r + 2, b.z);
        atomicMax(box + 4 * r + 3, b.w);
        if constexpr (SCORED)
            atomicAdd(acc + r, region_word_score(logits + (int64_t)(n0 + j) * n_classes, n_classes, class_group, grp[j]));
    }
    __syncthreads();
    for (int j = tid; j < np; j += REGION_THREADS) {
        const bool member = grp[j] >= 0, root = member && lbl[j] == j;
        comp[n0 + j] = member ? n0 + lbl[j] : -1;
        region_count[n0 + j] = root ? cnt[j] : 0;
        const int4 b = *reinterpret_cast<const int4*>(box + 4 * j);
        *reinterpret_cast<int4*>(region_box + (int64_t)(n0 + j) * 4) =
            make_int4(root ? b.x : 0, root ? b.y : 0, root ? b.z : 0, root ? b.w : 0);
        if constexpr (SCORED) region_score[n0 + j] = root ? (float)((double)acc[j] / ((double)cnt[j] * (double)REGION_SCORE_ONE)) : 0.f;
    }
}

// the checks and the launch of both entries (SCORED: + the three score arguments)
template <bool SCORED>
int page_regions_launch(const char* what, const int32_t* indptr, const int32_t* indices, const int32_t* node_off, int64_t n_pages,
                        int64_t n_nodes, int64_t max_page_nodes, const int32_t* group, const int32_t* bbox, int32_t* comp,
                        int32_t* region_box, int32_t* region_count, const float* logits, int n_classes, const int32_t* class_group,
                        float* region_score, void* stream) {
    if (n_pages < 0 || n_nodes < 0 || max_page_nodes < 0 || n_pages >= INT32_MAX || n_nodes >= INT32_MAX || (n_pages == 0 && n_nodes > 0))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: bad sizes", what);
    if (SCORED && n_classes < 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: n_classes = %d", what, n_classes);
    if (max_page_nodes > REGION_PAGE_MAX)
        return gte::fail(GTE_ERR_UNSUPPORTED, "%s: a page of %lld nodes exceeds %d", what, (long long)max_page_nodes, REGION_PAGE_MAX);
    if (n_nodes == 0) return GTE_OK;
    if (!indptr || !indices || !node_off || !group || !bbox || !comp || !region_box || !region_count ||
        (SCORED && (!logits || !class_group || !region_score)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if ((((uintptr_t)bbox | (uintptr_t)region_box) & 15) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: bbox and region_box must be 16-byte aligned", what);
    if (SCORED && ((((uintptr_t)logits | (uintptr_t)region_score) & 3) != 0))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: logits and region_score must be 4-byte aligned", what);
    const int cap = (int)(max_page_nodes > 0 ? max_page_nodes : 1);
    const size_t shm = (size_t)cap * region_node_bytes(SCORED) + REGION_TAIL_BYTES;
    static gte::LdsOptIn opt_in;                          // (one per instantiation)
    gte::allow_dynamic_lds(opt_in, &page_regions_kernel<SCORED>, SCORED ? REGION_LDS_MAX_SCORED : REGION_LDS_MAX);
    hipLaunchKernelGGL(page_regions_kernel<SCORED>, dim3((unsigned)n_pages), dim3(REGION_THREADS), shm, gte::as_stream(stream), indptr,
                       indices, node_off, group, bbox, cap, (int)n_nodes, comp, region_box, region_count, logits, n_classes,
                       class_group, region_score);
    return gte::check_launch(what);
}

}  // namespace

extern "C" int gte_region_max_page_nodes(void) { return REGION_PAGE_MAX; }

extern "C" int gte_page_regions(const int32_t* indptr, const int32_t* indices, const int32_t* node_off, int64_t n_pages,
                                int64_t n_nodes, int64_t max_page_nodes, const int32_t* group, const int32_t* bbox, int32_t* comp,
                                int32_t* region_box, int32_t* region_count, void* stream) {
    return page_regions_launch<false>("page_regions", indptr, indices, node_off, n_pages, n_nodes, max_page_nodes, group, bbox, comp,
                                      region_box, region_count, nullptr, 0, nullptr, nullptr, stream);
}

extern "C" int gte_page_regions_scored(const int32_t* indptr, const int32_t* indices, const int32_t* node_off, int64_t n_pages,
                                       int64_t n_nodes, int64_t max_page_nodes, const int32_t* group, const int32_t* bbox,
                                       const float* logits, int n_classes, const int32_t* class_group, int32_t* comp,
                                       int32_t* region_box, int32_t* region_count, float* region_score, void* stream) {
    return page_regions_launch<true>("page_regions_scored", indptr, indices, node_off, n_pages, n_nodes, max_page_nodes, group, bbox,
                                     comp, region_box, region_count, logits, n_classes, class_group, region_score, stream);
}
