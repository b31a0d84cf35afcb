// Word labels and figure nodes from page annotations: every word of a page takes the category of the FIRST annotation of the page
// whose rectangle strictly contains the word's centre (the categories of skip_mask are passed over), a word inside a FIGURE
// annotation is dropped, and every FIGURE annotation becomes a node of its own in front of the page's words.
//
// Reference: get_label() and the two loops of get_nodes() in GraphBuilder.get_graph(set_labels=True)
// (src/components/graphs/builder.py:151-167, 195-216) with center() of src/components/graphs/utils.py:107-108, pure Python there.
// The contract is the definition in include/gte.h; tests/wordlabels_ref.py (plain Python, written from it) is the oracle, every
// output is an integer and compared exactly.
//
// Structure.  Two launches with the caller's cumulative sum between them, one workgroup per page in both.
//   word_labels_kernel   the page-box skeleton of page_boxes.h, the table restaged per chunk: the page's annotations go through
//       LDS WL_CHUNK rectangles at a time, AS GIVEN (no normalisation); an annotation that is passed over is stored as four NaNs,
//       so it contains nothing and indices stay aligned.  A word takes the first hit of each chunk's table until it has one; it
//       still meets the barriers that restage LDS for the later chunks.  The page's two counts are LDS integer atomics on
//       per-thread partial counts: the sums do not depend on the order of arrival.
//   word_labels_compact_kernel   counts the page's figures and kept words (wave ballots), compares with the caller's run of
//       out_off, and only then writes: tiles of WL_THREADS candidates, a candidate's rank = the running base + the totals of the
//       lower waves (LDS) + the number of lower lanes of its wave that hold one (ballot, popcount).  No atomics: the order is exact.
// No float atomics, no allocation, no synchronisation.
#include "page_boxes.h"

namespace {

namespace pb = page_boxes;
constexpr int WL_THREADS = pb::kThreads;
constexpr int WL_WAVES = WL_THREADS / gte::kWave;
constexpr int WL_CHUNK = 1024;                        // annotations in LDS at a time: 32 KB
constexpr int WL_MAX_CAT = 32;                        // skip_mask is 32 bits
static_assert(WL_CHUNK % pb::kScan == 0, "a chunk is whole scan groups");
static_assert(WL_CHUNK * pb::kRowBytes + 64 <= 48 * 1024, "a chunk fits LDS without an opt-in attribute");

// popcount of the bits of `mask` below the calling lane
__device__ __forceinline__ int lower_lanes(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// grid = pages
__global__ void __launch_bounds__(WL_THREADS)
word_labels_kernel(const int32_t* __restrict__ bbox, const int32_t* __restrict__ node_off, const double* __restrict__ ann_box,
                   const int32_t* __restrict__ ann_cat, const int32_t* __restrict__ ann_off, int n_nodes, int n_ann, int n_cat,
                   uint32_t skip_mask, int figure_cat, int32_t* __restrict__ word_label, int32_t* __restrict__ word_ann,
                   int32_t* __restrict__ page_counts) {
    __shared__ __attribute__((aligned(16))) double s_box[WL_CHUNK * 4];   // [j] = r0, r1, r2, r3 as given, or four NaNs
    __shared__ int s_count[2];                                           // figures, kept words
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int n0 = node_off[p], n1 = node_off[p + 1], a0 = ann_off[p], a1 = ann_off[p + 1];
    if (!pb::run_ok(n0, n1, n_nodes) || !pb::run_ok(a0, a1, n_ann)) {            // offsets that name no row: nothing to label
        if (tid < 2) page_counts[2 * (int64_t)p + tid] = 0;
        return;
    }
    const int N = n1 - n0, A = a1 - a0;
    const int n_chunks = (A + WL_CHUNK - 1) / WL_CHUNK;
    const int n_tiles = N > 0 ? (N + WL_THREADS - 1) / WL_THREADS : 1;   // a page without words still counts its figures
    const double q = pb::quiet_nan();
    if (tid < 2) s_count[tid] = 0;
    int figures = 0, kept = 0;

    for (int t = 0; t < n_tiles; ++t) {
        const int i = t * WL_THREADS + tid;
        const bool word = i < N;
        double cx = 0.0, cy = 0.0;
        if (word) {
            const int4 w = *reinterpret_cast<const int4*>(bbox + (int64_t)(n0 + i) * 4);
            cx = (double)(((long long)w.x + (long long)w.z) / 2);        // C's division: towards zero; |.| < 2^31, exact in fp64
            cy = (double)(((long long)w.y + (long long)w.w) / 2);
        }
        int hit = -1;                                                    // index inside the page
        for (int c = 0; c < n_chunks; ++c) {
            const int c0 = c * WL_CHUNK;
            const int len = min(WL_CHUNK, A - c0);
            if (t == 0 || n_chunks > 1) {                                // a page of one chunk is staged once for all its tiles
                if (t > 0 || c > 0) __syncthreads();                     // every word is done with the chunk that is in LDS
                for (int j = tid; j < len; j += WL_THREADS) {
                    double r0 = q, r1 = q, r2 = q, r3 = q;
                    const int cat = ann_cat[a0 + c0 + j];
                    if (t == 0 && cat == figure_cat) ++figures;
                    if (cat >= 0 && cat < n_cat && !((skip_mask >> cat) & 1u)) {
                        const double* src = ann_box + (int64_t)(a0 + c0 + j) * 4;
                        r0 = src[0]; r1 = src[1]; r2 = src[2]; r3 = src[3];
                    }
                    s_box[j * 4 + 0] = r0; s_box[j * 4 + 1] = r1; s_box[j * 4 + 2] = r2; s_box[j * 4 + 3] = r3;
                }
                pb::pad_scan_group(s_box, len);
                __syncthreads();
            }
            if (word && hit < 0) {
                const int h = pb::first_hit(pb::corners(s_box), len, pb::HoldsCentre{cx, cy});
                if (h >= 0) hit = c0 + h;
            }
        }
        if (word) {
            int label = 0;                                               // OTHER: no annotation holds the centre
            if (hit >= 0) {
                const int cat = ann_cat[a0 + hit];
                label = cat == figure_cat ? -1 : cat;
            }
            word_label[n0 + i] = label;
            word_ann[n0 + i] = hit < 0 ? -1 : a0 + hit;
            if (label >= 0) ++kept;
        }
    }
    __syncthreads();                                                     // s_count is zero for every thread
    if (figures) atomicAdd(&s_count[0], figures);
    if (kept) atomicAdd(&s_count[1], kept);
    __syncthreads();
    if (tid < 2) page_counts[2 * (int64_t)p + tid] = s_count[tid];
}

// the number of threads of the workgroup with `flag`, in every thread (two barriers; s_wave: WL_WAVES ints)
__device__ __forceinline__ int block_count(bool flag, int* s_wave) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & (gte::kWave - 1)) == 0) s_wave[threadIdx.x / gte::kWave] = __popcll(m);
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < WL_WAVES; ++w) total += s_wave[w];
    __syncthreads();                                                     // s_wave may be written again
    return total;
}

// the rank of the calling thread among the threads with `flag` (thread order), and the workgroup's total
__device__ __forceinline__ int block_rank(bool flag, int* s_wave, int& total) {
    const unsigned long long m = __ballot(flag);
    const int wave = threadIdx.x / gte::kWave;
    if ((threadIdx.x & (gte::kWave - 1)) == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int below = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WL_WAVES; ++w) {
        const int c = s_wave[w];
        below += w < wave ? c : 0;
        total += c;
    }
    __syncthreads();
    return below + lower_lanes(m);
}

__device__ __forceinline__ int clamp_coord(double v) {
    const double lim = 1073741824.0;                                     // 2^30
    if (v != v) return 0;
    return (int)(v < -lim ? -lim : (v > lim ? lim : v));
}

// grid = pages
__global__ void __launch_bounds__(WL_THREADS)
word_labels_compact_kernel(const int32_t* __restrict__ bbox, const int32_t* __restrict__ node_off,
                           const int32_t* __restrict__ word_label, const double* __restrict__ ann_box,
                           const int32_t* __restrict__ ann_cat, const int32_t* __restrict__ ann_off,
                           const int32_t* __restrict__ out_off, const int32_t* __restrict__ cat_map, int n_nodes, int n_ann,
                           int n_cat, int figure_cat, int n_out, int32_t* __restrict__ out_bbox, int32_t* __restrict__ out_label,
                           int32_t* __restrict__ out_src, int32_t* __restrict__ page_status) {
    __shared__ int s_wave[WL_WAVES];
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int n0 = node_off[p], n1 = node_off[p + 1], a0 = ann_off[p], a1 = ann_off[p + 1], o0 = out_off[p], o1 = out_off[p + 1];
    if (!pb::run_ok(n0, n1, n_nodes) || !pb::run_ok(a0, a1, n_ann)) {            // offsets that name no row: nothing to write
        if (tid == 0) page_status[p] = 2;
        return;
    }
    const int N = n1 - n0, A = a1 - a0;
    // what the page holds, before a single row is written
    int figures = 0, kept = 0;
    for (int j0 = 0; j0 < A; j0 += WL_THREADS) {
        const int j = j0 + tid;
        figures += block_count(j < A && ann_cat[a0 + j] == figure_cat, s_wave);
    }
    for (int i0 = 0; i0 < N; i0 += WL_THREADS) {
        const int i = i0 + tid;
        kept += block_count(i < N && word_label[n0 + i] >= 0, s_wave);
    }
    if (!pb::run_ok(o0, o1, n_out) || o1 - o0 != figures + kept) {           // the caller's run is not this page's: write nothing
        if (tid == 0) page_status[p] = 2;
        return;
    }
    if (tid == 0) page_status[p] = 0;

    const int fig_label = cat_map ? cat_map[figure_cat] : figure_cat;
    int base = o0;
    for (int j0 = 0; j0 < A; j0 += WL_THREADS) {                         // the figures, in annotation order
        const int j = j0 + tid;
        const bool fig = j < A && ann_cat[a0 + j] == figure_cat;
        int total;
        const int row = base + block_rank(fig, s_wave, total);
        if (fig) {
            const double* src = ann_box + (int64_t)(a0 + j) * 4;
            *reinterpret_cast<int4*>(out_bbox + (int64_t)row * 4) =
                make_int4(clamp_coord(src[0]), clamp_coord(src[1]), clamp_coord(src[2]), clamp_coord(src[3]));
            out_label[row] = fig_label;
            out_src[row] = -1 - (a0 + j);
        }
        base += total;
    }
    for (int i0 = 0; i0 < N; i0 += WL_THREADS) {                         // then the kept words, in word order
        const int i = i0 + tid;
        const int cat = i < N ? word_label[n0 + i] : -1;
        int total;
        const int row = base + block_rank(cat >= 0, s_wave, total);
        if (cat >= 0) {
            *reinterpret_cast<int4*>(out_bbox + (int64_t)row * 4) = *reinterpret_cast<const int4*>(bbox + (int64_t)(n0 + i) * 4);
            out_label[row] = cat < n_cat ? (cat_map ? cat_map[cat] : cat) : -1;
            out_src[row] = n0 + i;
        }
        base += total;
    }
}

int check_sizes(const char* what, int64_t n_pages, int64_t n_nodes, int64_t n_ann, int n_cat, int figure_cat) {
    if (!pb::counts_ok(n_pages, n_nodes, n_ann))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: bad sizes", what);
    if (n_cat < 1 || n_cat > WL_MAX_CAT) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: %d categories (1 .. %d)", what, n_cat, WL_MAX_CAT);
    if (figure_cat < 0 || figure_cat >= n_cat)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "%s: figure_cat %d outside [0, %d)", what, figure_cat, n_cat);
    return GTE_OK;
}

}  // namespace

extern "C" int gte_word_labels_chunk(void) { return WL_CHUNK; }

extern "C" int gte_word_labels(const int32_t* bbox, const int32_t* node_off, const double* ann_box, const int32_t* ann_cat,
                               const int32_t* ann_off, int64_t n_pages, int64_t n_nodes, int64_t n_ann, int n_cat,
                               uint32_t skip_mask, int figure_cat, int32_t* word_label, int32_t* word_ann, int32_t* page_counts,
                               void* stream) {
    if (int rc = check_sizes("word_labels", n_pages, n_nodes, n_ann, n_cat, figure_cat)) return rc;
    if (n_pages == 0) return GTE_OK;
    if (!node_off || !ann_off || !page_counts || (n_nodes > 0 && (!bbox || !word_label || !word_ann)) ||
        (n_ann > 0 && (!ann_box || !ann_cat)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "word_labels: null pointer");
    if (!pb::boxes_aligned(bbox, ann_box) ||
        (((uintptr_t)node_off | (uintptr_t)ann_off | (uintptr_t)ann_cat | (uintptr_t)word_label | (uintptr_t)word_ann |
          (uintptr_t)page_counts) & 3) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "word_labels: bbox must be 16-byte aligned, ann_box 8-byte, int32 arrays 4-byte");
    hipLaunchKernelGGL(word_labels_kernel, dim3((unsigned)n_pages), dim3(WL_THREADS), 0, gte::as_stream(stream), bbox, node_off,
                       ann_box, ann_cat, ann_off, (int)n_nodes, (int)n_ann, n_cat, skip_mask, figure_cat, word_label, word_ann,
                       page_counts);
    return gte::check_launch("word_labels");
}

extern "C" int gte_word_labels_compact(const int32_t* bbox, const int32_t* node_off, const int32_t* word_label,
                                       const double* ann_box, const int32_t* ann_cat, const int32_t* ann_off,
                                       const int32_t* out_off, const int32_t* cat_map, int64_t n_pages, int64_t n_nodes,
                                       int64_t n_ann, int n_cat, int figure_cat, int64_t n_out, int32_t* out_bbox,
                                       int32_t* out_label, int32_t* out_src, int32_t* page_status, void* stream) {
    if (int rc = check_sizes("word_labels_compact", n_pages, n_nodes, n_ann, n_cat, figure_cat)) return rc;
    if (!pb::counts_ok(n_out)) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "word_labels_compact: bad sizes");
    if (n_pages == 0) return GTE_OK;
    if (!node_off || !ann_off || !out_off || !page_status || (n_nodes > 0 && (!bbox || !word_label)) ||
        (n_ann > 0 && (!ann_box || !ann_cat)) || (n_out > 0 && (!out_bbox || !out_label || !out_src)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "word_labels_compact: null pointer");
    if (!pb::boxes_aligned(bbox, ann_box) || ((uintptr_t)out_bbox & 15) != 0 ||
        (((uintptr_t)node_off | (uintptr_t)ann_off | (uintptr_t)ann_cat | (uintptr_t)word_label | (uintptr_t)out_off |
          (uintptr_t)cat_map | (uintptr_t)out_label | (uintptr_t)out_src | (uintptr_t)page_status) & 3) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT,
                         "word_labels_compact: bbox and out_bbox must be 16-byte aligned, ann_box 8-byte, int32 arrays 4-byte");
    hipLaunchKernelGGL(word_labels_compact_kernel, dim3((unsigned)n_pages), dim3(WL_THREADS), 0, gte::as_stream(stream), bbox,
                       node_off, word_label, ann_box, ann_cat, ann_off, out_off, cat_map, (int)n_nodes, (int)n_ann, n_cat,
                       figure_cat, (int)n_out, out_bbox, out_label, out_src, page_status);
    return gte::check_launch("word_labels_compact");
}
