// Confidence of a page's FINAL layout blocks (after table assembly and figures): the mean over the words that meet the block of
// the softmax mass their logits give to the classes of the block's category.
//
// Reference: none -- write_json() of src/components/graphs/postprocessing_2.py:337 gives every block the score 1.0, which is
// also what a block that no word meets receives here (image-derived FIGURE blocks are the usual case).  The contract is the
// definition in include/gte.h; tests/blockscore_ref.py (float64, written from it) is the oracle.
//
// Structure.  The page-box skeleton of page_boxes.h: the page's blocks, corners normalised, are the LDS table; beside it each
// block's class mask and two u32 accumulators (dynamic LDS: the table + 12 bytes per block; at most 22 KB).  A word forms its
// exponentials ONCE (word_score.h: WordExps, sixteen registers) and scans ALL blocks in index order, a scan group at a time;
// unlike the vote (block_vote.hip: the first hit only) it counts in every block it meets: final blocks overlap (tables absorb
// what they touch) and their order means nothing.  Per hit one quantised score (the region confidence's q, word_score.h) and a
// 1 are added with LDS integer atomics: the sums do not depend on the order of arrival.  No float atomics, no allocation, no
// synchronisation.
#include "page_boxes.h"
#include "word_score.h"

namespace {

namespace pb = page_boxes;
constexpr int BS_WORD_BYTES = 3 * 4;                  // mask, sum, count
static_assert(pb::kMaxBlocks * (pb::kRowBytes + BS_WORD_BYTES) <= 48 * 1024, "the largest page fits LDS without an opt-in attribute");

// grid = pages; dynamic LDS = table_bytes(cap) + cap * 12 bytes
__global__ void __launch_bounds__(pb::kThreads)
block_scores_kernel(const int32_t* __restrict__ bbox, const int32_t* __restrict__ node_off, const float* __restrict__ logits,
                    int64_t ld_logits, int n_classes, const double* __restrict__ block_box, const int32_t* __restrict__ block_off,
                    const int32_t* __restrict__ block_cat, const uint32_t* __restrict__ cat_classes, int n_cat, int n_nodes,
                    int n_blocks, int cap_words, int cap, float* __restrict__ score, int32_t* __restrict__ n_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* s_box = reinterpret_cast<double*>(s_raw);                    // the table
    unsigned* s_mask = reinterpret_cast<unsigned*>(s_raw + pb::table_bytes(cap));       // [cap]
    unsigned* s_sum = s_mask + cap;                                      // [cap]
    unsigned* s_cnt = s_sum + cap;                                       // [cap]
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int n0 = node_off[p], n1 = node_off[p + 1], b0 = block_off[p], b1 = block_off[p + 1];
    if (!pb::run_ok(n0, n1, n_nodes) || !pb::run_ok(b0, b1, n_blocks)) return;          // offsets that name no row: nothing to write to
    const int N = n1 - n0, B = b1 - b0;
    if (B > cap || N > cap_words) {                                      // the caller's maxima were wrong: the page takes no score
        for (int i = tid; i < B; i += pb::kThreads) { n_words[b0 + i] = -1; score[b0 + i] = 0.f; }
        return;
    }
    const unsigned live = n_classes >= 32 ? 0xFFFFFFFFu : (1u << n_classes) - 1u;        // (n_classes <= 16: the entry's check)
    pb::stage_normalised(s_box, block_box + (int64_t)b0 * 4, B);
    for (int i = tid; i < B; i += pb::kThreads) {
        const int k = block_cat[b0 + i];
        s_mask[i] = (k >= 0 && k < n_cat) ? (cat_classes[k] & live) : 0u;               // a category outside the table: the empty set
        s_sum[i] = 0u;
        s_cnt[i] = 0u;
    }
    __syncthreads();

    const double2* s_corner = pb::corners(s_box);
    for (int i = tid; i < N; i += pb::kThreads) {
        const pb::Meets meets(bbox, n0 + i);
        WordExps ex;
        ex.load(logits + (int64_t)(n0 + i) * ld_logits, n_classes);
        for (int j0 = 0; j0 < B; j0 += pb::kScan) {
            bool hit[pb::kScan];
#pragma unroll
            for (int u = 0; u < pb::kScan; ++u) hit[u] = meets(s_corner[2 * (j0 + u)], s_corner[2 * (j0 + u) + 1]);
#pragma unroll
            for (int u = 0; u < pb::kScan; ++u) {
                if (!hit[u]) continue;                                   // (a padding row is NaNs: never a hit, so j0 + u < B here)
                atomicAdd(&s_sum[j0 + u], ex.score(s_mask[j0 + u]));
                atomicAdd(&s_cnt[j0 + u], 1u);
            }
        }
    }
    __syncthreads();

    for (int i = tid; i < B; i += pb::kThreads) {
        const unsigned cnt = s_cnt[i];
        n_words[b0 + i] = (int32_t)cnt;
        score[b0 + i] = cnt ? (float)((double)s_sum[i] / ((double)cnt * (double)GTE_SCORE_ONE)) : 1.0f;      // postprocessing_2.py:337
    }
}

}  // namespace

extern "C" int gte_block_scores_max_page_blocks(void) { return pb::kMaxBlocks; }
extern "C" int gte_block_scores_max_page_words(void) { return GTE_SCORE_PAGE_MAX; }
extern "C" int gte_block_scores_max_classes(void) { return GTE_SCORE_MAX_CLASSES; }
extern "C" int gte_block_scores_max_categories(void) { return pb::kMaxCat; }

extern "C" int gte_block_scores(const int32_t* bbox, const int32_t* node_off, const float* logits, int64_t ld_logits, int n_classes,
                                const double* block_box, const int32_t* block_off, const int32_t* block_cat,
                                const uint32_t* cat_classes, int n_cat, int64_t n_pages, int64_t n_nodes, int64_t n_blocks,
                                int64_t max_page_words, int64_t max_page_blocks, float* score, int32_t* n_words, void* stream) {
    if (!pb::counts_ok(n_pages, n_nodes, n_blocks) || max_page_words < 0 || max_page_blocks < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: bad sizes");
    if (n_classes < 1 || n_cat < 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: %d classes, %d categories", n_classes, n_cat);
    if (n_classes > GTE_SCORE_MAX_CLASSES)
        return gte::fail(GTE_ERR_UNSUPPORTED, "block_scores: %d classes exceed %d", n_classes, GTE_SCORE_MAX_CLASSES);
    if (n_cat > pb::kMaxCat) return gte::fail(GTE_ERR_UNSUPPORTED, "block_scores: %d categories exceed %d", n_cat, pb::kMaxCat);
    if (ld_logits < n_classes) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: row stride %lld below %d classes", (long long)ld_logits, n_classes);
    if (max_page_blocks > pb::kMaxBlocks)
        return gte::fail(GTE_ERR_UNSUPPORTED, "block_scores: a page of %lld blocks exceeds %d", (long long)max_page_blocks, pb::kMaxBlocks);
    if (max_page_words > GTE_SCORE_PAGE_MAX)
        return gte::fail(GTE_ERR_UNSUPPORTED, "block_scores: a page of %lld words exceeds %d", (long long)max_page_words, GTE_SCORE_PAGE_MAX);
    if (n_pages == 0 || n_blocks == 0) return GTE_OK;                    // no block: nothing to write
    if (!node_off || !block_off || !cat_classes || (n_nodes > 0 && (!bbox || !logits)) || !block_box || !block_cat || !score || !n_words)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: null pointer");
    if (!pb::boxes_aligned(bbox, block_box) || ((uintptr_t)logits & 3) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_scores: bbox must be 16-byte aligned, block_box 8-byte, logits 4-byte");
    const int cap = pb::page_cap(max_page_blocks);
    const size_t lds = pb::table_bytes(cap) + (size_t)cap * BS_WORD_BYTES;
    hipLaunchKernelGGL(block_scores_kernel, dim3((unsigned)n_pages), dim3(pb::kThreads), lds, gte::as_stream(stream), bbox, node_off, logits,
                       ld_logits, n_classes, block_box, block_off, block_cat, cat_classes, n_cat, (int)n_nodes, (int)n_blocks,
                       (int)max_page_words, cap, score, n_words);
    return gte::check_launch("block_scores");
}
