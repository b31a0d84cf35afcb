// REPR node features: every word carries the id of its normalised token; the token's embedding row is compared with the C
// prototypes ("centres") in float64 and the word takes the output row of the nearest one (hard mode) or the similarity-weighted
// mix of all output rows (combined mode).
//
// Reference: Repr.get_similarity and the per-page loop of Repr.__call__ (src/components/nlp/repr.py:75-87, 111-139), one tensor
// expansion per page and one Python assignment per word there.  The contract is the definition in include/gte.h;
// tests/repr_ref.py (numpy, written from it) is the oracle.
//
// Structure.  One launch.  A workgroup is RP_WAVES waves, ONE WAVE PER WORD, centre c on lane c (C <= 64).  The centres go through
// LDS in chunks of RP_DCHUNK dimensions, dimension-major with a row stride of 65 doubles (lane c reads s_centre[k * 65 + c]: adjacent
// doubles; the staging writes walk k and land two to a bank).  With D <= RP_DCHUNK -- every configuration of the reference -- the
// chunk is staged once per workgroup and the words of the workgroup's grid-stride loop run against it with no further barrier.  The
// word's token id is made wave-uniform, so its embedding row is read at uniform addresses: one value for all lanes.
//   distance   acc += (e_k - c_k)^2 for k = 0 .. D-1 in that order, the product and the sum rounded separately (no contraction):
//              the numpy oracle performs the same operations, so d_c agrees bit for bit.
//   s, arg-max every lane walks c = 0 .. C-1 with the value of lane c broadcast through the scalar unit (v_readlane): the sum has
//              the stated order, and "the first index at which q is largest" is the plain sequential scan.  Two loops of <= 64 steps.
//   output     column j on lane j % 64: a copy of one row of i_proto (hard), or C float32 FMAs in the order of c (combined).
// No atomics, no allocation, no workspace, no synchronisation.
//
// Known limitation.  The reference sums the C weights with torch.sum and the D squares with torch.norm, whose orders are not
// defined.  A word whose two best clamped distances differ by less than about 1e-12 relative may therefore be assigned another
// centre there than here.  Nothing is tested in that band: fixtures and tests keep the two best either bit-equal or 1e-9 apart.
// For alpha != 1 the weights go through pow(), which is not correctly rounded on either side; hard mode is pinned at alpha = 1,
// where w = 1 / t is used as it stands.
#include "gte_common.h"

#include <math.h>

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_WAVES = RP_THREADS / gte::kWave;     // words in flight per workgroup
constexpr int RP_MAX_C = gte::kWave;                  // one centre per lane
constexpr int RP_MAX_DIM = 1024;
constexpr int RP_MAX_OUT = 1024;
constexpr int RP_DCHUNK = 64;                         // dimensions of every centre in LDS at a time
constexpr int RP_STRIDE = RP_MAX_C + 1;               // doubles between two dimensions of the LDS image
constexpr int RP_MAX_BLOCKS = 2048;
constexpr double RP_MIN_MARGIN = 1e-4;                // repr.py:76
static_assert(RP_DCHUNK * RP_STRIDE * 8 <= 48 * 1024, "a chunk fits LDS without an opt-in attribute");

// the value that `lane` holds, in every lane (`lane` is wave-uniform)
__device__ __forceinline__ double lane_value(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

__global__ void __launch_bounds__(RP_THREADS)
repr_features_kernel(const int32_t* __restrict__ node_tok, int64_t n_nodes, const double* __restrict__ embeddings, int64_t n_vocab,
                     int dim, const double* __restrict__ centers, const double* __restrict__ i_proto, int n_centroids, int n_out,
                     double alpha, int combined, float* __restrict__ out, int64_t ldo) {
    __shared__ double s_centre[RP_DCHUNK * RP_STRIDE];                   // [k][c]: centre c, dimension k0 + k; 0 outside C x D
    const int tid = threadIdx.x;
    const int lane = tid & (gte::kWave - 1);
    const int wave = tid / gte::kWave;
    const int n_chunks = (dim + RP_DCHUNK - 1) / RP_DCHUNK;
    bool staged = false;

    // the trip count depends on blockIdx alone: every wave of the workgroup meets every barrier
    for (int64_t base = (int64_t)blockIdx.x * RP_WAVES; base < n_nodes; base += (int64_t)gridDim.x * RP_WAVES) {
        const int64_t i = base + wave;
        int tok = -1;
        if (i < n_nodes) tok = node_tok[i];
        tok = __builtin_amdgcn_readfirstlane(tok);
        const bool word = tok >= 0 && (int64_t)tok < n_vocab;            // -1, or an id that names no row: a row of zeros
        const double* __restrict__ e = embeddings + (word ? (int64_t)tok * dim : 0);

        double acc = 0.0;                                                // lane c: the squared distance to centre c
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int k0 = ch * RP_DCHUNK;
            const int len = min(RP_DCHUNK, dim - k0);
            if (!staged || n_chunks > 1) {
                if (staged) __syncthreads();                             // every wave is done with the chunk that is in LDS
                for (int idx = tid; idx < RP_MAX_C * len; idx += RP_THREADS) {
                    const int c = idx / len, k = idx - c * len;          // consecutive threads: consecutive dimensions of one centre
                    s_centre[k * RP_STRIDE + c] = c < n_centroids ? centers[(int64_t)c * dim + k0 + k] : 0.0;
                }
                __syncthreads();
                staged = true;
            }
            if (word) {
#pragma unroll 4
                for (int k = 0; k < len; ++k) {
#pragma clang fp contract(off)                                           // product and sum rounded separately, as the oracle does
                    const double diff = e[k0 + k] - s_centre[k * RP_STRIDE + lane];
                    const double sq = diff * diff;
                    acc = acc + sq;
                }
            }
        }
        if (i >= n_nodes) continue;                                      // (no barrier below this line)

        float* __restrict__ row = out + i * ldo;
        if (!word) {
            for (int j = lane; j < n_out; j += gte::kWave) row[j] = 0.f;
            continue;
        }
        const double t = fmax(sqrt(acc), RP_MIN_MARGIN);
        const double inv = 1.0 / t;
        const double w = lane < n_centroids ? (alpha == 1.0 ? inv : pow(inv, alpha)) : 0.0;
        double s = 0.0;
        for (int c = 0; c < n_centroids; ++c) s += lane_value(w, c);
        const double q = w / s;

        if (!combined) {
            double best = lane_value(q, 0);
            int arg = 0;
            for (int c = 1; c < n_centroids; ++c) {
                const double qc = lane_value(q, c);
                if (qc > best) { best = qc; arg = c; }                   // strict: the first of equal maxima stays
            }
            const double* __restrict__ src = i_proto + (int64_t)arg * n_out;
            for (int j = lane; j < n_out; j += gte::kWave) row[j] = (float)src[j];
        } else {
            const float qf = (float)q;
            for (int j0 = 0; j0 < n_out; j0 += gte::kWave) {             // uniform trip count: every lane takes part in the broadcasts
                const int j = j0 + lane;
                const bool in = j < n_out;
                float sum = 0.f;
                for (int c = 0; c < n_centroids; ++c) {
                    const float p = in ? (float)i_proto[(int64_t)c * n_out + j] : 0.f;
                    sum = fmaf(lane_value(qf, c), p, sum);
                }
                if (in) row[j] = sum;
            }
        }
    }
}

}  // namespace

extern "C" int gte_repr_max_centroids(void) { return RP_MAX_C; }
extern "C" int gte_repr_max_dim(void) { return RP_MAX_DIM; }
extern "C" int gte_repr_max_out(void) { return RP_MAX_OUT; }

extern "C" int gte_repr_features(const int32_t* node_tok, int64_t n_nodes, const double* embeddings, int64_t n_vocab, int dim,
                                 const double* centers, const double* i_proto, int n_centroids, int n_out, double alpha,
                                 int combined, float* out, int64_t ldo, void* stream) {
    if (n_nodes < 0 || n_vocab < 0 || dim < 1 || n_centroids < 1 || n_out < 1)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "repr_features: bad sizes (n_nodes %lld, n_vocab %lld, dim %d, n_centroids %d, n_out %d)",
                         (long long)n_nodes, (long long)n_vocab, dim, n_centroids, n_out);
    if (ldo < n_out) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "repr_features: ldo %lld < n_out %d", (long long)ldo, n_out);
    if (!(fabs(alpha) <= 1.7976931348623157e308))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "repr_features: alpha is not finite");
    if (combined != 0 && combined != 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "repr_features: combined %d (0 or 1)", combined);
    if (n_centroids > RP_MAX_C || dim > RP_MAX_DIM || n_out > RP_MAX_OUT)
        return gte::fail(GTE_ERR_UNSUPPORTED, "repr_features: %d centres x %d dimensions -> %d columns (limits %d, %d, %d)",
                         n_centroids, dim, n_out, RP_MAX_C, RP_MAX_DIM, RP_MAX_OUT);
    if (n_nodes == 0) return GTE_OK;
    if (!node_tok || !centers || !i_proto || !out || (n_vocab > 0 && !embeddings))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "repr_features: null pointer");
    if ((((uintptr_t)embeddings | (uintptr_t)centers | (uintptr_t)i_proto) & 7) != 0 || (((uintptr_t)node_tok | (uintptr_t)out) & 3) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "repr_features: float64 arrays must be 8-byte aligned, node_tok and out 4-byte");
    const int64_t blocks = gte::ceil_div(n_nodes, RP_WAVES);
    hipLaunchKernelGGL(repr_features_kernel, dim3((unsigned)(blocks < RP_MAX_BLOCKS ? blocks : RP_MAX_BLOCKS)), dim3(RP_THREADS), 0,
                       gte::as_stream(stream), node_tok, n_nodes, embeddings, n_vocab, dim, centers, i_proto, n_centroids, n_out,
                       alpha, combined, out, ldo);
    return gte::check_launch("repr_features");
}
