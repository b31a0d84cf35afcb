// Token pooling: every word carries up to `width` ids of rows of a float32 table (its word pieces); the word's output row is the
// mean, or the maximum against zero, of those rows.  The arithmetic half of the SCIBERT embedder.
//
// Reference: SciBERT.list_of_sentence with mean_pooling / max_pooling (src/components/nlp/scibert.py:53-65, 143-160): an embedding
// lookup to [words, L, D], a product with the expanded mask and a reduction over L, per page.  Here the mask is already in the ids
// (-1 wherever the reference's modified mask is 0: components/nlp/scibert.py), all pages run in one launch and the rows go straight
// to their place in the feature matrix.  The contract is the definition in include/gte.h; tests/scibert_ref.py (numpy, written from
// it) is the oracle.
//
// Structure.  One launch, ONE WAVE PER WORD, grid-stride over words; a workgroup is TP_WAVES independent waves.
//   ids      lane j reads id j of the word; the ids that take part (0 <= id < n_vocab) are picked out of the ballot mask in position
//            order through the scalar unit (v_readlane), so every row base is wave-uniform and nothing else is ever an address.
//   columns  lanes take columns: four adjacent ones per lane with 16-byte loads and stores where the table, dim, out and ldo are
//            16-byte friendly (token_pool_form), one per lane otherwise.  Per column chunk the row reads of up to TP_BATCH ids are
//            issued back to back -- independent loads, all in flight -- and then consumed in position order: s = s + x, one rounding
//            per add (mean), or m = x > m ? x : m from m = 0 (max).  Both forms perform the same operations per element: same bits.
//   rows     a 3 KB row is three chunks of a wave in the wide form.  Wave-per-word rather than workgroup-per-word: a word has a
//            handful of ids, so a word is a few KB of reads; a 256-thread workgroup would leave three of its four waves idle at
//            D = 768 and all but a few lanes at D = 12, and the waves share nothing that LDS could hold.
// No atomics, no LDS, no workspace, no synchronisation.
#include "gte_common.h"

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_WAVES = TP_THREADS / gte::kWave;     // words in flight per workgroup
constexpr int TP_MAX_WIDTH = 32;                      // ids per word: one per lane of the lower half wave (reference: 15)
constexpr int TP_MAX_DIM = 4096;
constexpr int TP_BATCH = 16;                          // row reads in flight per column chunk (the reference's 15 in one batch)
constexpr int TP_MAX_BLOCKS = 2048;
static_assert(TP_MAX_WIDTH <= 2 * TP_BATCH && TP_MAX_WIDTH <= gte::kWave, "two batches cover a word");

struct Ids { int id[TP_MAX_WIDTH]; int count; };      // wave-uniform: lives in scalar registers once the loops are unrolled

template <int MODE>
__device__ __forceinline__ float fold(float acc, float x) {
    if constexpr (MODE == 0) return acc + x;
    else return x > acc ? x : acc;
}

template <int MODE, typename V>
__device__ __forceinline__ V fold_v(V acc, V x) {
    if constexpr (sizeof(V) == 4) return fold<MODE>(acc, x);
    else {
        acc.x = fold<MODE>(acc.x, x.x); acc.y = fold<MODE>(acc.y, x.y);
        acc.z = fold<MODE>(acc.z, x.z); acc.w = fold<MODE>(acc.w, x.w);
        return acc;
    }
}

template <typename V>
__device__ __forceinline__ V scaled(V s, float c) {
    if constexpr (sizeof(V) == 4) return __fdiv_rn(s, c);
    else return V{__fdiv_rn(s.x, c), __fdiv_rn(s.y, c), __fdiv_rn(s.z, c), __fdiv_rn(s.w, c)};
}

// V = float4: the wide form, V = float: the dword form.  MODE 0 mean, 1 max.
template <int MODE, typename V>
__global__ void __launch_bounds__(TP_THREADS)
token_pool_kernel(const int32_t* __restrict__ tok, int64_t n_words, int width, const float* __restrict__ table, int64_t n_vocab,
                  int dim, const int64_t* __restrict__ row_map, float* __restrict__ out, int64_t ldo) {
    constexpr int PER = sizeof(V) / 4;                                   // columns per lane
    const int lane = threadIdx.x & (gte::kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / gte::kWave));
    const int64_t step = (int64_t)gridDim.x * TP_WAVES;

    for (int64_t i = (int64_t)blockIdx.x * TP_WAVES + wave; i < n_words; i += step) {
        const int64_t r = row_map ? row_map[i] : i;                      // i is wave-uniform: one scalar read
        if (r < 0) continue;                                             // a dropped word: nothing read, nothing written

        int mine = -1;
        if (lane < width) mine = tok[i * width + lane];
        const bool takes_part = mine >= 0 && (int64_t)mine < n_vocab;    // anything else is skipped and is never an address
        uint64_t mask = __ballot(takes_part);
        Ids ids;
        ids.count = __popcll(mask);
#pragma unroll
        for (int t = 0; t < TP_MAX_WIDTH; ++t) {                         // the ids that take part, in position order
            ids.id[t] = 0;
            if (t < ids.count) {
                ids.id[t] = __builtin_amdgcn_readlane(mine, __builtin_ctzll(mask));
                mask &= mask - 1;
            }
        }

        float* __restrict__ dst = out + r * ldo;
        for (int col = lane * PER; col < dim; col += gte::kWave * PER) {
            V acc;
            if constexpr (PER == 4) acc = V{0.f, 0.f, 0.f, 0.f}; else acc = 0.f;
#pragma unroll
            for (int b = 0; b < TP_MAX_WIDTH; b += TP_BATCH) {
                if (b < ids.count) {                                     // (wave-uniform)
                    V x[TP_BATCH];
#pragma unroll
                    for (int t = 0; t < TP_BATCH; ++t)                   // every read of the batch is issued ...
                        if (b + t < ids.count) x[t] = *reinterpret_cast<const V*>(table + (int64_t)ids.id[b + t] * dim + col);
#pragma unroll
                    for (int t = 0; t < TP_BATCH; ++t)                   // ... before the first is consumed, in position order
                        if (b + t < ids.count) acc = fold_v<MODE>(acc, x[t]);
                }
            }
            if constexpr (MODE == 0) {
                if (ids.count > 0) acc = scaled(acc, (float)ids.count);  // correctly rounded; no id at all: the 0 it holds
            }
            *reinterpret_cast<V*>(dst + col) = acc;
        }
    }
}

// 16: four columns per lane with 16-byte accesses; 4: one column per lane
int token_pool_form(const float* table, int dim, const float* out, int64_t ldo) {
    const bool wide = (dim & 3) == 0 && (ldo & 3) == 0 && (((uintptr_t)table | (uintptr_t)out) & 15) == 0;
    return wide ? 16 : 4;
}

template <int MODE, typename V>
void launch(unsigned blocks, hipStream_t stream, const int32_t* tok, int64_t n_words, int width, const float* table, int64_t n_vocab,
            int dim, const int64_t* row_map, float* out, int64_t ldo) {
    hipLaunchKernelGGL((token_pool_kernel<MODE, V>), dim3(blocks), dim3(TP_THREADS), 0, stream, tok, n_words, width, table, n_vocab,
                       dim, row_map, out, ldo);
}

}  // namespace

extern "C" int gte_token_pool_max_width(void) { return TP_MAX_WIDTH; }
extern "C" int gte_token_pool_max_dim(void) { return TP_MAX_DIM; }
extern "C" int gte_token_pool_access_bytes(const float* table, int dim, const float* out, int64_t ldo) {
    return token_pool_form(table, dim, out, ldo);
}

extern "C" int gte_token_pool_f32(const int32_t* tok, int64_t n_words, int width, const float* table, int64_t n_vocab, int dim,
                                  int mode, const int64_t* row_map, float* out, int64_t ldo, void* stream) {
    if (n_words < 0 || n_vocab < 0 || width < 1 || dim < 1)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "token_pool: bad sizes (n_words %lld, n_vocab %lld, width %d, dim %d)",
                         (long long)n_words, (long long)n_vocab, width, dim);
    if (n_vocab > 2147483647LL)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "token_pool: n_vocab %lld is beyond what an int32 id names", (long long)n_vocab);
    if (ldo < dim) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "token_pool: ldo %lld < dim %d", (long long)ldo, dim);
    if (mode != 0 && mode != 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "token_pool: mode %d (0 mean, 1 max)", mode);
    if (width > TP_MAX_WIDTH || dim > TP_MAX_DIM)
        return gte::fail(GTE_ERR_UNSUPPORTED, "token_pool: %d ids per word x %d columns (limits %d, %d)", width, dim, TP_MAX_WIDTH,
                         TP_MAX_DIM);
    if (n_words == 0) return GTE_OK;
    if (!tok || !out || (n_vocab > 0 && !table)) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "token_pool: null pointer");
    if ((((uintptr_t)tok | (uintptr_t)table | (uintptr_t)out) & 3) != 0 || ((uintptr_t)row_map & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "token_pool: tok, table and out must be 4-byte aligned, row_map 8-byte");
    const int64_t want = gte::ceil_div(n_words, TP_WAVES);
    const unsigned blocks = (unsigned)(want < TP_MAX_BLOCKS ? want : TP_MAX_BLOCKS);
    hipStream_t s = gte::as_stream(stream);
    const bool wide = token_pool_form(table, dim, out, ldo) == 16;
    if (mode == 0) {
        if (wide) launch<0, float4>(blocks, s, tok, n_words, width, table, n_vocab, dim, row_map, out, ldo);
        else launch<0, float>(blocks, s, tok, n_words, width, table, n_vocab, dim, row_map, out, ldo);
    } else {
        if (wide) launch<1, float4>(blocks, s, tok, n_words, width, table, n_vocab, dim, row_map, out, ldo);
        else launch<1, float>(blocks, s, tok, n_words, width, table, n_vocab, dim, row_map, out, ldo);
    }
    return gte::check_launch("token_pool");
}
