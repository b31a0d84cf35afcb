// Confidence of a page's FINAL layout blocks (after table assembly and figures): the mean over the words that meet the block of
// the softmax mass their logits give to the classes of the block's category.
//
// Reference: none -- write_json() of src/components/graphs/postprocessing_2.py:337 gives every block the score 1.0, which is
// also what a block that no word meets receives here (image-derived FIGURE blocks are the usual case).  The contract is the
// definition in include/gte.h; tests/blockscore_ref.py (float64, written from it) is the oracle.
//
// Structure.  One workgroup per page.  The page's blocks, corners normalised (min / max per axis; a block with a NaN corner is
// four NaNs, so every comparison with it is false), each block's class mask and two u32 accumulators per block live in LDS
// (dynamic: 44 bytes per block, blocks rounded up to whole scan groups; at most 22 KB).  Words are strided over the workgroup.
// A word forms its exponentials ONCE (word_score.h: WordExps, sixteen registers) and scans ALL blocks in index order, four at a
// time -- every lane reads the same LDS address, a broadcast; unlike the vote (block_vote.hip: the first block only) it counts in
// every block it meets: final blocks overlap (tables absorb what they touch) and their order means nothing.  Per hit one
// quantised score (the region confidence's q, word_score.h) and a 1 are added with LDS integer atomics: the sums do not depend on
// the order of arrival.  No float atomics, no allocation, no synchronisation.
#include "gte_common.h"
#include "word_score.h"

namespace {

constexpr int BS_THREADS = 1024;                      // a page has hundreds of words, the largest a few thousand
constexpr int BS_MAX_BLOCKS = 512;                    // per page
constexpr int BS_MAX_CAT = 16;
constexpr int BS_SCAN = 4;                            // blocks a word tests per round of LDS loads
constexpr int BS_BLOCK_BYTES = 4 * 8 + 3 * 4;         // corners, mask, sum, count
static_assert(BS_MAX_BLOCKS % BS_SCAN == 0, "the largest page is whole scan groups");
static_assert(BS_MAX_BLOCKS * BS_BLOCK_BYTES <= 48 * 1024, "the largest page fits LDS without an opt-in attribute");

__host__ __device__ inline int scan_rows(int blocks) { return (blocks + BS_SCAN - 1) / BS_SCAN * BS_SCAN; }

// grid = pages; dynamic LDS = scan_rows(cap) * (32 + 12) bytes
__global__ void __launch_bounds__(BS_THREADS)
block_scores_kernel(const int32_t* __restrict__ bbox, const int32_t* __restrict__ node_off, const float* __restrict__ logits,
                    int64_t ld_logits, int n_classes, const double* __restrict__ block_box, const int32_t* __restrict__ block_off,
                    const int32_t* __restrict__ block_cat, const uint32_t* __restrict__ cat_classes, int n_cat, int n_nodes,
                    int n_blocks, int cap_words, int cap, float* __restrict__ score, int32_t* __restrict__ n_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int rows = scan_rows(cap);
    double* s_box = reinterpret_cast<double*>(s_raw);                    // [rows][4]: lo x, lo y, hi x, hi y
    unsigned* s_mask = reinterpret_cast<unsigned*>(s_raw + (size_t)rows * 32);           // [rows]
    unsigned* s_sum = s_mask + rows;                                     // [rows]
    unsigned* s_cnt = s_sum + rows;                                      // [rows]
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int n0 = node_off[p], n1 = node_off[p + 1], b0 = block_off[p], b1 = block_off[p + 1];
    if (n0 < 0 || n1 < n0 || n1 > n_nodes || b0 < 0 || b1 < b0 || b1 > n_blocks) return;   // offsets that name no row: nothing to write to
    const int N = n1 - n0, B = b1 - b0;
    if (B > cap || N > cap_words) {                                      // the caller's maxima were wrong: the page takes no score
        for (int i = tid; i < B; i += BS_THREADS) { n_words[b0 + i] = -1; score[b0 + i] = 0.f; }
        return;
    }
    const unsigned live = n_classes >= 32 ? 0xFFFFFFFFu : (1u << n_classes) - 1u;        // (n_classes <= 16: the entry's check)
    for (int i = tid; i < B; i += BS_THREADS) {
        const double* src = block_box + (int64_t)(b0 + i) * 4;
        const double x0 = src[0], y0 = src[1], x1 = src[2], y1 = src[3];
        const bool nan = x0 != x0 || y0 != y0 || x1 != x1 || y1 != y1;
        const double q = __longlong_as_double(0x7ff8000000000000ll);
        s_box[i * 4 + 0] = nan ? q : (x0 < x1 ? x0 : x1);
        s_box[i * 4 + 1] = nan ? q : (y0 < y1 ? y0 : y1);
        s_box[i * 4 + 2] = nan ? q : (x0 < x1 ? x1 : x0);
        s_box[i * 4 + 3] = nan ? q : (y0 < y1 ? y1 : y0);
        const int k = block_cat[b0 + i];
        s_mask[i] = (k >= 0 && k < n_cat) ? (cat_classes[k] & live) : 0u;               // a category outside the table: the empty set
        s_sum[i] = 0u;
        s_cnt[i] = 0u;
    }
    for (int i = B * 4 + tid; i < scan_rows(B) * 4; i += BS_THREADS)     // pad to whole scan groups: blocks that meet nothing
        s_box[i] = __longlong_as_double(0x7ff8000000000000ll);
    __syncthreads();

    const double2* s_corner = reinterpret_cast<const double2*>(s_raw);  // [2 j] = (lo x, lo y), [2 j + 1] = (hi x, hi y)
    for (int i = tid; i < N; i += BS_THREADS) {
        const int4 w = *reinterpret_cast<const int4*>(bbox + (int64_t)(n0 + i) * 4);
        const double wx0 = (double)min(w.x, w.z), wy0 = (double)min(w.y, w.w), wx1 = (double)max(w.x, w.z), wy1 = (double)max(w.y, w.w);
        WordExps ex;
        ex.load(logits + (int64_t)(n0 + i) * ld_logits, n_classes);
        for (int j0 = 0; j0 < B; j0 += BS_SCAN) {
            bool hit[BS_SCAN];
#pragma unroll
            for (int u = 0; u < BS_SCAN; ++u) {
                const double2 lo = s_corner[2 * (j0 + u)], hi = s_corner[2 * (j0 + u) + 1];
                // max(lo, lo') <= min(hi, hi') on both axes, with lo <= hi on either side: closed, touching counts
                hit[u] = lo.x <= wx1 && wx0 <= hi.x && lo.y <= wy1 && wy0 <= hi.y;
            }
#pragma unroll
            for (int u = 0; u < BS_SCAN; ++u) {
                if (!hit[u]) continue;                                   // (a padding row is NaNs: never a hit, so j0 + u < B here)
                atomicAdd(&s_sum[j0 + u], ex.score(s_mask[j0 + u]));
                atomicAdd(&s_cnt[j0 + u], 1u);
            }
        }
    }
    __syncthreads();

    for (int i = tid; i < B; i += BS_THREADS) {
        const unsigned cnt = s_cnt[i];
        n_words[b0 + i] = (int32_t)cnt;
        score[b0 + i] = cnt ? (float)((double)s_sum[i] / ((double)cnt * (double)GTE_SCORE_ONE)) : 1.0f;      // postprocessing_2.py:337
    }
}

}  // namespace

extern "C" int gte_block_scores_max_page_blocks(void) { return BS_MAX_BLOCKS; }
extern "C" int gte_block_scores_max_page_words(void) { return GTE_SCORE_PAGE_MAX; }
extern "C" int gte_block_scores_max_classes(void) { return GTE_SCORE_MAX_CLASSES; }
extern "C" int gte_block_scores_max_categories(void) { return BS_MAX_CAT; }

extern "C" int gte_block_scores(const int32_t* bbox, const int32_t* node_off, const float* logits, int64_t ld_logits, int n_classes,
                                const double* block_box, const int32_t* block_off, const int32_t* block_cat,
                                const uint32_t* cat_classes, int n_cat, int64_t n_pages, int64_t n_nodes, int64_t n_blocks,
                                int64_t max_page_words, int64_t max_page_blocks, float* score, int32_t* n_words, void* stream) {
    if (n_pages < 0 || n_pages >= INT32_MAX || n_nodes < 0 || n_nodes >= INT32_MAX || n_blocks < 0 || n_blocks >= INT32_MAX ||
        max_page_words < 0 || max_page_blocks < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: bad sizes");
    if (n_classes < 1 || n_cat < 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: %d classes, %d categories", n_classes, n_cat);
    if (n_classes > GTE_SCORE_MAX_CLASSES)
        return gte::fail(GTE_ERR_UNSUPPORTED, "block_scores: %d classes exceed %d", n_classes, GTE_SCORE_MAX_CLASSES);
    if (n_cat > BS_MAX_CAT) return gte::fail(GTE_ERR_UNSUPPORTED, "block_scores: %d categories exceed %d", n_cat, BS_MAX_CAT);
    if (ld_logits < n_classes) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: row stride %lld below %d classes", (long long)ld_logits, n_classes);
    if (max_page_blocks > BS_MAX_BLOCKS)
        return gte::fail(GTE_ERR_UNSUPPORTED, "block_scores: a page of %lld blocks exceeds %d", (long long)max_page_blocks, BS_MAX_BLOCKS);
    if (max_page_words > GTE_SCORE_PAGE_MAX)
        return gte::fail(GTE_ERR_UNSUPPORTED, "block_scores: a page of %lld words exceeds %d", (long long)max_page_words, GTE_SCORE_PAGE_MAX);
    if (n_pages == 0 || n_blocks == 0) return GTE_OK;                    // no block: nothing to write
    if (!node_off || !block_off || !cat_classes || (n_nodes > 0 && (!bbox || !logits)) || !block_box || !block_cat || !score || !n_words)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: null pointer");
    if (((uintptr_t)bbox & 15) != 0 || ((uintptr_t)block_box & 7) != 0 || ((uintptr_t)logits & 3) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: bbox must be 16-byte aligned, block_box 8-byte, logits 4-byte");
    const int cap = max_page_blocks > 0 ? (int)max_page_blocks : 1;
    const size_t lds = (size_t)scan_rows(cap) * BS_BLOCK_BYTES;
    hipLaunchKernelGGL(block_scores_kernel, dim3((unsigned)n_pages), dim3(BS_THREADS), lds, gte::as_stream(stream), bbox, node_off, logits,
                       ld_logits, n_classes, block_box, block_off, block_cat, cat_classes, n_cat, (int)n_nodes, (int)n_blocks,
                       (int)max_page_words, cap, score, n_words);
    return gte::check_launch("block_scores");
}
