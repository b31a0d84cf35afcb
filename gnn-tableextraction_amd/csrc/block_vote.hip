// Layout blocks labelled by the vote of their words: every word of a page goes to the FIRST block of the page whose rectangle
// meets the word's, and adds its predicted category to that block's counters (a title word counts double); the block's label is
// the lowest category with the largest count.
//
// Reference: the words x blocks double loop of get_objects_bboxs() (src/components/graphs/postprocessing_2.py:240-258), pure
// Python there.  The contract is the definition in include/gte.h; tests/blocks_ref.py (plain Python, written from it) is the
// oracle, every output is an integer and compared exactly.
//
// Structure.  One workgroup per page.  The page's blocks, corners normalised (min / max per axis), and its counters live in LDS
// (dynamic: 32 bytes per block, rounded up to whole scan groups, + 4 * n_cat per block; at most 48 KB).  Words are strided over
// the workgroup; a word scans the blocks in index order, four at a time -- every lane reads the same LDS address, a broadcast --
// and stops after the group that holds its first hit.  The test is four fp64 comparisons on values that are exact (int32 ->
// double) or the caller's own doubles: no arithmetic, nothing to round.  A block with a NaN corner is stored as four NaNs, so
// every comparison with it is false.  Votes are LDS integer atomics: the sums do not depend on the order of arrival.  No float
// atomics, no allocation, no synchronisation.
#include "gte_common.h"

namespace {

constexpr int BV_THREADS = 1024;                      // a page has hundreds of words, the largest a few thousand
constexpr int BV_MAX_BLOCKS = 512;                    // per page
constexpr int BV_MAX_CAT = 16;
constexpr int BV_SCAN = 4;                            // blocks a word tests between two looks at its result
static_assert(BV_MAX_BLOCKS % BV_SCAN == 0, "the largest page is whole scan groups");
static_assert(BV_MAX_BLOCKS * (4 * 8 + BV_MAX_CAT * 4) <= 48 * 1024, "the largest page fits LDS without an opt-in attribute");

__host__ __device__ inline int scan_rows(int blocks) { return (blocks + BV_SCAN - 1) / BV_SCAN * BV_SCAN; }

// grid = pages; dynamic LDS = scan_rows(cap) * 32 + cap * 4 * n_cat bytes
__global__ void __launch_bounds__(BV_THREADS)
block_vote_kernel(const int32_t* __restrict__ bbox, const int32_t* __restrict__ node_off, const int32_t* __restrict__ word_cat,
                  const double* __restrict__ block_box, const int32_t* __restrict__ block_off, int n_nodes, int n_blocks, int cap,
                  int n_cat, int double_cat, int32_t* __restrict__ word_block, int32_t* __restrict__ votes,
                  int32_t* __restrict__ block_label) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* s_box = reinterpret_cast<double*>(s_raw);                    // [scan_rows(cap)][4]: lo x, lo y, hi x, hi y
    int* s_votes = reinterpret_cast<int*>(s_raw + (size_t)scan_rows(cap) * 32);         // [cap][n_cat]
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int n0 = node_off[p], n1 = node_off[p + 1], b0 = block_off[p], b1 = block_off[p + 1];
    if (n0 < 0 || n1 < n0 || n1 > n_nodes || b0 < 0 || b1 < b0 || b1 > n_blocks) return;   // offsets that name no row: nothing to write to
    const int N = n1 - n0, B = b1 - b0;
    if (B > cap) {                                                       // the caller's maximum was wrong: the page takes no vote
        for (int i = tid; i < N; i += BV_THREADS) word_block[n0 + i] = -1;
        for (int64_t i = tid; i < (int64_t)B * n_cat; i += BV_THREADS) votes[(int64_t)b0 * n_cat + i] = 0;
        for (int i = tid; i < B; i += BV_THREADS) block_label[b0 + i] = 0;
        return;
    }
    for (int i = tid; i < B; i += BV_THREADS) {
        const double* src = block_box + (int64_t)(b0 + i) * 4;
        const double x0 = src[0], y0 = src[1], x1 = src[2], y1 = src[3];
        const bool nan = x0 != x0 || y0 != y0 || x1 != x1 || y1 != y1;
        const double q = __longlong_as_double(0x7ff8000000000000ll);
        s_box[i * 4 + 0] = nan ? q : (x0 < x1 ? x0 : x1);
        s_box[i * 4 + 1] = nan ? q : (y0 < y1 ? y0 : y1);
        s_box[i * 4 + 2] = nan ? q : (x0 < x1 ? x1 : x0);
        s_box[i * 4 + 3] = nan ? q : (y0 < y1 ? y1 : y0);
    }
    for (int i = B * 4 + tid; i < scan_rows(B) * 4; i += BV_THREADS)     // pad to whole scan groups: blocks that meet nothing
        s_box[i] = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = tid; i < B * n_cat; i += BV_THREADS) s_votes[i] = 0;
    __syncthreads();

    const double2* s_corner = reinterpret_cast<const double2*>(s_raw);  // [2 j] = (lo x, lo y), [2 j + 1] = (hi x, hi y)
    for (int i = tid; i < N; i += BV_THREADS) {
        const int4 w = *reinterpret_cast<const int4*>(bbox + (int64_t)(n0 + i) * 4);
        const double wx0 = (double)min(w.x, w.z), wy0 = (double)min(w.y, w.w), wx1 = (double)max(w.x, w.z), wy1 = (double)max(w.y, w.w);
        // BV_SCAN blocks at a time, their loads independent of the tests (a scan that left after every block would wait for one
        // LDS round trip per block); inside a group the descending order leaves the lowest hit
        int hit = -1;
        for (int j0 = 0; j0 < B && hit < 0; j0 += BV_SCAN) {
#pragma unroll
            for (int u = BV_SCAN - 1; u >= 0; --u) {
                const double2 lo = s_corner[2 * (j0 + u)], hi = s_corner[2 * (j0 + u) + 1];
                // max(lo, lo') <= min(hi, hi') on both axes, with lo <= hi on either side: closed, touching counts
                if (lo.x <= wx1 && wx0 <= hi.x && lo.y <= wy1 && wy0 <= hi.y) hit = j0 + u;
            }
        }
        word_block[n0 + i] = hit < 0 ? -1 : b0 + hit;
        const int c = word_cat[n0 + i];
        if (hit >= 0 && c >= 0 && c < n_cat) atomicAdd(&s_votes[hit * n_cat + c], c == double_cat ? 2 : 1);
    }
    __syncthreads();

    for (int i = tid; i < B * n_cat; i += BV_THREADS) votes[(int64_t)b0 * n_cat + i] = s_votes[i];
    for (int i = tid; i < B; i += BV_THREADS) {
        int best = 0, most = s_votes[i * n_cat];
        for (int c = 1; c < n_cat; ++c) {
            const int v = s_votes[i * n_cat + c];
            if (v > most) { most = v; best = c; }                        // strictly: the lowest category among equals
        }
        block_label[b0 + i] = best;
    }
}

}  // namespace

extern "C" int gte_block_vote_max_page_blocks(void) { return BV_MAX_BLOCKS; }
extern "C" int gte_block_vote_max_categories(void) { return BV_MAX_CAT; }

extern "C" int gte_block_vote(const int32_t* bbox, const int32_t* node_off, const int32_t* word_cat, const double* block_box,
                              const int32_t* block_off, int64_t n_pages, int64_t n_nodes, int64_t n_blocks, int64_t max_page_blocks,
                              int n_cat, int double_cat, int32_t* word_block, int32_t* votes, int32_t* block_label, void* stream) {
    if (n_pages < 0 || n_pages >= INT32_MAX || n_nodes < 0 || n_nodes >= INT32_MAX || n_blocks < 0 || n_blocks >= INT32_MAX ||
        max_page_blocks < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_vote: bad sizes");
    if (n_cat < 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_vote: %d categories", n_cat);
    if (n_cat > BV_MAX_CAT) return gte::fail(GTE_ERR_UNSUPPORTED, "block_vote: %d categories exceed %d", n_cat, BV_MAX_CAT);
    if (max_page_blocks > BV_MAX_BLOCKS)
        return gte::fail(GTE_ERR_UNSUPPORTED, "block_vote: a page of %lld blocks exceeds %d", (long long)max_page_blocks, BV_MAX_BLOCKS);
    if (n_pages == 0) return GTE_OK;
    if (!node_off || !block_off || (n_nodes > 0 && (!bbox || !word_cat || !word_block)) ||
        (n_blocks > 0 && (!block_box || !votes || !block_label)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_vote: null pointer");
    if (((uintptr_t)bbox & 15) != 0 || ((uintptr_t)block_box & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "block_vote: bbox must be 16-byte aligned, block_box 8-byte");
    const int cap = max_page_blocks > 0 ? (int)max_page_blocks : 1;
    const size_t lds = (size_t)scan_rows(cap) * 32 + (size_t)cap * 4 * (size_t)n_cat;
    hipLaunchKernelGGL(block_vote_kernel, dim3((unsigned)n_pages), dim3(BV_THREADS), lds, gte::as_stream(stream), bbox, node_off, word_cat,
                       block_box, block_off, (int)n_nodes, (int)n_blocks, cap, n_cat, double_cat, word_block, votes, block_label);
    return gte::check_launch("block_vote");
}
