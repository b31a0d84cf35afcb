// Layout blocks labelled by the vote of their words: every word of a page goes to the FIRST block of the page whose rectangle
// meets the word's, and adds its predicted category to that block's counters (a title word counts double); the block's label is
// the lowest category with the largest count.
//
// Reference: the words x blocks double loop of get_objects_bboxs() (src/components/graphs/postprocessing_2.py:240-258), pure
// Python there.  The contract is the definition in include/gte.h; tests/blocks_ref.py (plain Python, written from it) is the
// oracle, every output is an integer and compared exactly.
//
// Structure.  The page-box skeleton of page_boxes.h: the page's blocks, corners normalised, are the LDS table; beside it the
// page's counters (dynamic LDS: the table + 4 * n_cat bytes per block; at most 48 KB).  A word takes the table's first hit over
// the page.  Votes are LDS integer atomics: the sums do not depend on the order of arrival.  No float atomics, no allocation, no
// synchronisation.
#include "page_boxes.h"

namespace {

namespace pb = page_boxes;
static_assert(pb::kMaxBlocks * (pb::kRowBytes + pb::kMaxCat * 4) <= 48 * 1024, "the largest page fits LDS without an opt-in attribute");

// grid = pages; dynamic LDS = table_bytes(cap) + cap * 4 * n_cat bytes
__global__ void __launch_bounds__(pb::kThreads)
block_vote_kernel(const int32_t* __restrict__ bbox, const int32_t* __restrict__ node_off, const int32_t* __restrict__ word_cat,
                  const double* __restrict__ block_box, const int32_t* __restrict__ block_off, int n_nodes, int n_blocks, int cap,
                  int n_cat, int double_cat, int32_t* __restrict__ word_block, int32_t* __restrict__ votes,
                  int32_t* __restrict__ block_label) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* s_box = reinterpret_cast<double*>(s_raw);                    // the table
    int* s_votes = reinterpret_cast<int*>(s_raw + pb::table_bytes(cap));                // [cap][n_cat]
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int n0 = node_off[p], n1 = node_off[p + 1], b0 = block_off[p], b1 = block_off[p + 1];
    if (!pb::run_ok(n0, n1, n_nodes) || !pb::run_ok(b0, b1, n_blocks)) return;          // offsets that name no row: nothing to write to
    const int N = n1 - n0, B = b1 - b0;
    if (B > cap) {                                                       // the caller's maximum was wrong: the page takes no vote
        for (int i = tid; i < N; i += pb::kThreads) word_block[n0 + i] = -1;
        for (int64_t i = tid; i < (int64_t)B * n_cat; i += pb::kThreads) votes[(int64_t)b0 * n_cat + i] = 0;
        for (int i = tid; i < B; i += pb::kThreads) block_label[b0 + i] = 0;
        return;
    }
    pb::stage_normalised(s_box, block_box + (int64_t)b0 * 4, B);
    for (int i = tid; i < B * n_cat; i += pb::kThreads) s_votes[i] = 0;
    __syncthreads();

    for (int i = tid; i < N; i += pb::kThreads) {
        const int hit = pb::first_hit(pb::corners(s_box), B, pb::Meets(bbox, n0 + i));
        word_block[n0 + i] = hit < 0 ? -1 : b0 + hit;
        const int c = word_cat[n0 + i];
        if (hit >= 0 && c >= 0 && c < n_cat) atomicAdd(&s_votes[hit * n_cat + c], c == double_cat ? 2 : 1);
    }
    __syncthreads();

    for (int i = tid; i < B * n_cat; i += pb::kThreads) votes[(int64_t)b0 * n_cat + i] = s_votes[i];
    for (int i = tid; i < B; i += pb::kThreads) {
        int best = 0, most = s_votes[i * n_cat];
        for (int c = 1; c < n_cat; ++c) {
            const int v = s_votes[i * n_cat + c];
            if (v > most) { most = v; best = c; }                        // strictly: the lowest category among equals
        }
        block_label[b0 + i] = best;
    }
}

}  // namespace

extern "C" int gte_block_vote_max_page_blocks(void) { return pb::kMaxBlocks; }
extern "C" int gte_block_vote_max_categories(void) { return pb::kMaxCat; }

extern "C" int gte_block_vote(const int32_t* bbox, const int32_t* node_off, const int32_t* word_cat, const double* block_box,
                              const int32_t* block_off, int64_t n_pages, int64_t n_nodes, int64_t n_blocks, int64_t max_page_blocks,
                              int n_cat, int double_cat, int32_t* word_block, int32_t* votes, int32_t* block_label, void* stream) {
    if (!pb::counts_ok(n_pages, n_nodes, n_blocks) || max_page_blocks < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_vote: bad sizes");
    if (n_cat < 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_vote: %d categories", n_cat);
    if (n_cat > pb::kMaxCat) return gte::fail(GTE_ERR_UNSUPPORTED, "block_vote: %d categories exceed %d", n_cat, pb::kMaxCat);
    if (max_page_blocks > pb::kMaxBlocks)
        return gte::fail(GTE_ERR_UNSUPPORTED, "block_vote: a page of %lld blocks exceeds %d", (long long)max_page_blocks, pb::kMaxBlocks);
    if (n_pages == 0) return GTE_OK;
    if (!node_off || !block_off || (n_nodes > 0 && (!bbox || !word_cat || !word_block)) ||
        (n_blocks > 0 && (!block_box || !votes || !block_label)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_vote: null pointer");
    if (!pb::boxes_aligned(bbox, block_box))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_vote: bbox must be 16-byte aligned, block_box 8-byte");
    const int cap = pb::page_cap(max_page_blocks);
    const size_t lds = pb::table_bytes(cap) + (size_t)cap * 4 * (size_t)n_cat;
    hipLaunchKernelGGL(block_vote_kernel, dim3((unsigned)n_pages), dim3(pb::kThreads), lds, gte::as_stream(stream), bbox, node_off, word_cat,
                       block_box, block_off, (int)n_nodes, (int)n_blocks, cap, n_cat, double_cat, word_block, votes, block_label);
    return gte::check_launch("block_vote");
}
