// All-pairs weighted Levenshtein distance: out[p, q] = lev(src[p] -> dst[q]) in float64, every pair one tiny dynamic programme.
//
// Reference: LevenshteinSimilitudes.calculate_similarity (src/components/tables/levenshtein.py:50-63), a Python double loop of
// n^2 calls into the weighted_levenshtein extension (n = 2000 in Preprocessor.train_repr).  The contract -- the recurrence, with
// its "equal characters copy the diagonal, NO minimum" rule -- is the definition in include/gte.h; tests/lev_ref.py (numpy and
// plain Python, written from it) is the oracle.
//
// Structure.  One launch, ONE WAVE PER WORKGROUP.  blockIdx.y names one src word (a stride loop above 65 535 of them), blockIdx.x
// a chunk of 64 dst words, ONE DST WORD PER LANE: the 64 results of a workgroup are 64 adjacent doubles of one row of `out`, and
// the substitution costs a step needs are 64 entries of ONE row of sub_cost (the row of the src character).
//   shared    the src word's characters and their delete costs are the same for all lanes: the wave reads them once into LDS
//             (lane i holds character i) and the loops read them back at wave-uniform addresses (a broadcast).
//   column    the rolling DP column d[0 .. la][j] lives in LDS as col[i][lane], 65 x 64 doubles: adjacent lanes hit adjacent
//             doubles (ds_read_b64 / ds_write_b64 conflict-free), no lane touches another lane's entries.
//   loops     the inner loop runs over the src word with a wave-uniform trip count; the outer loop runs over the lane's own
//             word, and lanes drop out as their word ends.  Every cell is one of three correctly rounded float64 sums or a copy:
//             there is no product to contract and no order of evaluation that could change a bit.
//   reads     a word's start and length are clamped into [0, off[n]] and to max_len, a character id to n_alpha - 1: whatever
//             offsets and ids the call is handed, nothing outside the word buffers (as off[n] describes them) and the cost
//             tables is read.
// The only barriers fence the staging of the shared word, inside a one-wave workgroup.  No atomics, no workspace, no allocation.
#include "gte_common.h"

namespace {

constexpr int LV_MAX_LEN = 64;                        // characters per word: one character of the shared word per lane
constexpr int LV_MAX_ALPHA = 1024;                    // sub_cost at the cap: 8 MB, resident in L2 / Infinity Cache
constexpr int LV_MAX_ROWS = 65535;                    // gridDim.y
static_assert(LV_MAX_LEN == gte::kWave, "the shared word is staged one character per lane");
static_assert(((LV_MAX_LEN + 1) * gte::kWave + LV_MAX_LEN) * 8 + LV_MAX_LEN * 4 <= 48 * 1024, "the column fits LDS without an opt-in");

// word w of a packed list: its first character and its length, both clamped so that [first, first + len) lies inside
// [0, off[n]) and len <= max_len
__device__ __forceinline__ void word_span(const int32_t* __restrict__ off, int64_t n, int64_t w, int max_len, int64_t& first, int& len) {
    const int64_t total = max((int64_t)off[n], (int64_t)0);
    first = min(max((int64_t)off[w], (int64_t)0), total);
    const int64_t l = (int64_t)off[w + 1] - first;
    len = (int)min(max(l, (int64_t)0), min((int64_t)max_len, total - first));
}

__global__ void __launch_bounds__(gte::kWave)
lev_matrix_kernel(const uint16_t* __restrict__ src_chars, const int32_t* __restrict__ src_off, int64_t n_src,
                  const uint16_t* __restrict__ dst_chars, const int32_t* __restrict__ dst_off, int64_t n_dst, int max_len,
                  const double* __restrict__ ins_cost, const double* __restrict__ del_cost, const double* __restrict__ sub_cost,
                  int n_alpha, double* __restrict__ out, int64_t ldo) {
    __shared__ double s_col[(LV_MAX_LEN + 1) * gte::kWave];              // [i][lane]: d[i][j - 1], then d[i][j]
    __shared__ double s_del[LV_MAX_LEN];                                 // delete cost of character i of the src word
    __shared__ int s_a[LV_MAX_LEN];                                      // character i of the src word
    const int lane = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * gte::kWave + lane;
    const bool live = q < n_dst;

    // the lane's own word: fixed for the whole workgroup
    int64_t b0 = 0;
    int lb = 0;
    if (live) word_span(dst_off, n_dst, q, max_len, b0, lb);

    for (int64_t p = blockIdx.y; p < n_src; p += gridDim.y) {
        int64_t a0;
        int la;
        word_span(src_off, n_src, p, max_len, a0, la);                   // (wave-uniform)
        if (lane < la) {
            const int a = min((int)src_chars[a0 + lane], n_alpha - 1);
            s_a[lane] = a;
            s_del[lane] = del_cost[a];
        }
        __syncthreads();                                                 // (a workgroup is one wave: p, la and the trip count are uniform)
        if (live) {
            double cur = 0.0;                                            // d[0][0]
            s_col[lane] = cur;
            for (int i = 1; i <= la; ++i) {                              // d[i][0] = d[i-1][0] + del[a[i-1]]
                cur = cur + s_del[i - 1];
                s_col[i * gte::kWave + lane] = cur;
            }
            for (int j = 1; j <= lb; ++j) {                              // lanes drop out as their word ends
                const int b = min((int)dst_chars[b0 + j - 1], n_alpha - 1);
                const double ic = ins_cost[b];
                double diag = s_col[lane];                               // d[0][j-1]
                cur = diag + ic;                                         // d[0][j] = d[0][j-1] + ins[b[j-1]]
                s_col[lane] = cur;
#pragma unroll 4
                for (int i = 1; i <= la; ++i) {                          // uniform trip count
                    const int a = s_a[i - 1];
                    const double left = s_col[i * gte::kWave + lane];    // d[i][j-1]
                    const double by_del = cur + s_del[i - 1];            // d[i-1][j] + del[a[i-1]]
                    const double by_ins = left + ic;                     // d[i][j-1] + ins[b[j-1]]
                    const double by_sub = diag + sub_cost[(int64_t)a * n_alpha + b];
                    const double least = fmin(fmin(by_del, by_ins), by_sub);
                    cur = a == b ? diag : least;                         // equal characters: a copy, NO minimum
                    s_col[i * gte::kWave + lane] = cur;
                    diag = left;
                }
            }
            out[p * ldo + q] = s_col[la * gte::kWave + lane];
        }
        __syncthreads();                                                 // the next src word overwrites s_a / s_del
    }
}

}  // namespace

extern "C" int gte_lev_max_len(void) { return LV_MAX_LEN; }
extern "C" int gte_lev_max_alphabet(void) { return LV_MAX_ALPHA; }

extern "C" int gte_lev_matrix_f64(const uint16_t* src_chars, const int32_t* src_off, int64_t n_src, const uint16_t* dst_chars,
                                  const int32_t* dst_off, int64_t n_dst, int max_len, const double* ins_cost,
                                  const double* del_cost, const double* sub_cost, int n_alpha, double* out, int64_t ldo,
                                  void* stream) {
    if (n_src < 0 || n_dst < 0 || max_len < 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "lev_matrix: bad sizes (n_src %lld, n_dst %lld, max_len %d)", (long long)n_src,
                         (long long)n_dst, max_len);
    if (ldo < n_dst) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "lev_matrix: ldo %lld < n_dst %lld", (long long)ldo, (long long)n_dst);
    if (max_len > LV_MAX_LEN || n_alpha < 1 || n_alpha > LV_MAX_ALPHA)
        return gte::fail(GTE_ERR_UNSUPPORTED, "lev_matrix: words of %d characters over an alphabet of %d (limits %d, 1 .. %d)", max_len,
                         n_alpha, LV_MAX_LEN, LV_MAX_ALPHA);
    if (n_src == 0 || n_dst == 0) return GTE_OK;
    // (an empty character buffer may be null: a list of empty words)
    if (!src_off || !dst_off || !ins_cost || !del_cost || !sub_cost || !out)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "lev_matrix: null pointer");
    if ((((uintptr_t)ins_cost | (uintptr_t)del_cost | (uintptr_t)sub_cost | (uintptr_t)out) & 7) != 0 ||
        (((uintptr_t)src_off | (uintptr_t)dst_off) & 3) != 0 || (((uintptr_t)src_chars | (uintptr_t)dst_chars) & 1) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "lev_matrix: float64 arrays must be 8-byte aligned, offsets 4-byte, characters 2-byte");
    const int64_t chunks = gte::ceil_div(n_dst, gte::kWave);
    if (chunks > 0x7fffffffLL) return gte::fail(GTE_ERR_UNSUPPORTED, "lev_matrix: %lld dst words", (long long)n_dst);
    hipLaunchKernelGGL(lev_matrix_kernel, dim3((unsigned)chunks, (unsigned)(n_src < LV_MAX_ROWS ? n_src : LV_MAX_ROWS)),
                       dim3(gte::kWave), 0, gte::as_stream(stream), src_chars, src_off, n_src, dst_chars, dst_off, n_dst, max_len,
                       ins_cost, del_cost, sub_cost, n_alpha, out, ldo);
    return gte::check_launch("lev_matrix");
}
