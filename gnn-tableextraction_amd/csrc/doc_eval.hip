// Area-weighted confusion of node predictions: the sums behind the DocBank token metric (a word counts with the area of its box)
// and behind what the reference's evaluate_doc makes of it.
//
// Reference: the class loop of evaluate_doc, src/models/evaluate.py:182-202, numpy on the host there.  Its np.delete calls take a
// two-column index array, so besides the true positives the FIRST t_c entries of a class's predicted (ground-truth) list leave the
// false positives (negatives) too: `lead` below is exactly the area that this loses.  The contract is the definition in
// include/gte.h; tests/doceval_ref.py (numpy, written from it) is the oracle, every output is an integer and compared exactly.
//
// Structure.  One memset and three launches on the caller's stream; kernel boundaries are the only ordering between them.
//   doc_tally_kernel   one workgroup per chunk of DE_CHUNK nodes.  The (C+1)^2 cell areas (u64) and counts go to LDS: a node adds
//       its area with one LDS atomic; the per-class |P_c|, |G_c| and the diagonal counts are popcounts of wave ballots, added once
//       per wave, and only an off-diagonal node adds a 1 of its own.  The workgroup flushes its nonzero cells with 64-bit global
//       atomics into the workspace's accumulators (zeroed by the memset) and leaves the chunk's class counts behind.
//   doc_scan_kernel    one workgroup: accumulators -> area_out / count_out, zeros to lead_out, and per class the exclusive prefix
//       of the chunks' counts in place (a wave per sequence, 64 chunks per wave scan).
//   doc_lead_kernel    one workgroup per chunk, a wave on DE_WAVE_NODES consecutive nodes held in registers.  A node's position
//       within P_c = the chunk's prefix + the lower waves' totals (LDS) + the earlier sub-tiles of its wave + the popcount of the
//       ballot's lower lanes.  A chunk whose base positions have all reached t_c leaves at once.
// Integer sums only: arrival order cannot change a bit.  No allocation, no synchronisation, no workgroup waits on another.
#include "gte_common.h"

namespace {

constexpr int DE_MAX_CLASSES = 16;
constexpr int DE_THREADS = 256;
constexpr int DE_WAVES = DE_THREADS / gte::kWave;
constexpr int DE_SUB = 8;                             // sub-tiles of 64 nodes per wave
constexpr int DE_WAVE_NODES = DE_SUB * gte::kWave;    // 512 consecutive nodes
constexpr int DE_CHUNK = DE_WAVES * DE_WAVE_NODES;    // 2048 nodes per workgroup
constexpr int DE_MAX_CELLS = (DE_MAX_CLASSES + 1) * (DE_MAX_CLASSES + 1);

typedef unsigned long long u64;

// popcount of the bits of `mask` below the calling lane
__device__ __forceinline__ int lower_lanes(u64 mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// (x1 - x0) * (y1 - y0): the differences exact in 64 bits, the product modulo 2^64 (the caller keeps it inside int64)
__device__ __forceinline__ u64 box_area(const int32_t* __restrict__ bbox, int64_t node) {
    const int4 b = *reinterpret_cast<const int4*>(bbox + node * 4);
    return (u64)((int64_t)b.z - (int64_t)b.x) * (u64)((int64_t)b.w - (int64_t)b.y);
}

// the node's first index in sub-tile s of the calling wave
__device__ __forceinline__ int64_t wave_node(int s) {
    return (int64_t)blockIdx.x * DE_CHUNK + (threadIdx.x / gte::kWave) * DE_WAVE_NODES + s * gte::kWave + (threadIdx.x & (gte::kWave - 1));
}

// grid = chunks.  accum = [2][cells] u64 (areas, counts); chunk_cnt = int32 [2 C][n_chunks]: |P_c| then |G_c| per chunk
__global__ void __launch_bounds__(DE_THREADS)
doc_tally_kernel(const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, const int32_t* __restrict__ bbox, int64_t n_nodes,
                 int C, u64* __restrict__ accum, int32_t* __restrict__ chunk_cnt, int n_chunks) {
    __shared__ u64 s_area[DE_MAX_CELLS];
    __shared__ unsigned s_cnt[DE_MAX_CELLS];
    __shared__ unsigned s_cls[2 * DE_MAX_CLASSES];
    const int tid = threadIdx.x;
    const int side = C + 1, cells = side * side;
    for (int i = tid; i < cells; i += DE_THREADS) { s_area[i] = 0; s_cnt[i] = 0u; }
    if (tid < 2 * DE_MAX_CLASSES) s_cls[tid] = 0u;
    __syncthreads();

    const bool leader = (tid & (gte::kWave - 1)) == 0;
    for (int s = 0; s < DE_SUB; ++s) {
        const int64_t node = wave_node(s);
        const bool valid = node < n_nodes;
        int g = -1, p = -1;                                              // past the end: in no class and in no cell
        if (valid) {
            g = gt[node];
            p = pred[node];
            g = (unsigned)g < (unsigned)C ? g : C;                       // index C: none of the classes
            p = (unsigned)p < (unsigned)C ? p : C;
            atomicAdd(&s_area[g * side + p], box_area(bbox, node));
            if (g != p || g == C) atomicAdd(&s_cnt[g * side + p], 1u);   // the diagonal of the classes is counted by ballot below
        }
        for (int c = 0; c < C; ++c) {
            const u64 mp = __ballot(p == c), mg = __ballot(g == c);
            if (leader && (mp | mg)) {
                atomicAdd(&s_cls[c], (unsigned)__popcll(mp));
                atomicAdd(&s_cls[DE_MAX_CLASSES + c], (unsigned)__popcll(mg));
                atomicAdd(&s_cnt[c * side + c], (unsigned)__popcll(mp & mg));
            }
        }
    }
    __syncthreads();

    for (int i = tid; i < cells; i += DE_THREADS) {
        if (s_area[i]) atomicAdd(&accum[i], s_area[i]);
        if (s_cnt[i]) atomicAdd(&accum[cells + i], (u64)s_cnt[i]);
    }
    if (tid < 2 * C) {
        const int which = tid / C, c = tid - which * C;
        chunk_cnt[(int64_t)tid * n_chunks + blockIdx.x] = (int32_t)s_cls[which * DE_MAX_CLASSES + c];
    }
}

// one workgroup
__global__ void __launch_bounds__(DE_THREADS)
doc_scan_kernel(const u64* __restrict__ accum, int C, int32_t* __restrict__ chunk_cnt, int n_chunks, int64_t* __restrict__ area_out,
                int64_t* __restrict__ count_out, int64_t* __restrict__ lead_out) {
    const int tid = threadIdx.x, lane = tid & (gte::kWave - 1);
    const int cells = (C + 1) * (C + 1);
    for (int i = tid; i < cells; i += DE_THREADS) {
        area_out[i] = (int64_t)accum[i];
        count_out[i] = (int64_t)accum[cells + i];
    }
    if (tid < 2 * C) lead_out[tid] = 0;
    for (int seq = tid / gte::kWave; seq < 2 * C; seq += DE_WAVES) {     // wave-uniform
        int32_t* row = chunk_cnt + (int64_t)seq * n_chunks;
        int running = 0;
        for (int j0 = 0; j0 < n_chunks; j0 += gte::kWave) {
            const int j = j0 + lane;
            const int v = j < n_chunks ? row[j] : 0;
            int incl = v;
#pragma unroll
            for (int d = 1; d < gte::kWave; d <<= 1) {
                const int up = __shfl_up(incl, d, gte::kWave);
                if (lane >= d) incl += up;
            }
            if (j < n_chunks) row[j] = running + incl - v;               // exclusive: the nodes of class `seq` ahead of chunk j
            running += __shfl(incl, gte::kWave - 1, gte::kWave);
        }
    }
}

// grid = chunks.  chunk_base = chunk_cnt after the scan; count = the finished cell counts (accum + cells)
__global__ void __launch_bounds__(DE_THREADS)
doc_lead_kernel(const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, const int32_t* __restrict__ bbox, int64_t n_nodes,
                int C, const u64* __restrict__ count, const int32_t* __restrict__ chunk_base, int n_chunks,
                int64_t* __restrict__ lead_out) {
    __shared__ int s_tot[2 * DE_MAX_CLASSES][DE_WAVES];
    __shared__ u64 s_lead[2 * DE_MAX_CLASSES];
    const int tid = threadIdx.x, wave = tid / gte::kWave;
    const int side = C + 1;
    const int chunk = blockIdx.x;

    bool live = false;                                                   // (uniform: every thread reads the same words)
    for (int c = 0; c < C; ++c) {
        const int64_t t = (int64_t)count[c * side + c];
        live = live || chunk_base[(int64_t)c * n_chunks + chunk] < t || chunk_base[(int64_t)(C + c) * n_chunks + chunk] < t;
    }
    if (!live) return;                                                   // positions only grow: nothing here lies below any t_c

    int g[DE_SUB], p[DE_SUB];
#pragma unroll
    for (int s = 0; s < DE_SUB; ++s) {
        const int64_t node = wave_node(s);
        g[s] = p[s] = -1;                                                // past the end, or outside the classes: in no list
        if (node < n_nodes) {
            g[s] = gt[node];
            p[s] = pred[node];
        }
    }
    if (tid < 2 * DE_MAX_CLASSES) s_lead[tid] = 0;
    const bool leader = (tid & (gte::kWave - 1)) == 0;
    for (int c = 0; c < C; ++c) {
        int tot_p = 0, tot_g = 0;
#pragma unroll
        for (int s = 0; s < DE_SUB; ++s) {
            tot_p += __popcll(__ballot(p[s] == c));
            tot_g += __popcll(__ballot(g[s] == c));
        }
        if (leader) { s_tot[c][wave] = tot_p; s_tot[DE_MAX_CLASSES + c][wave] = tot_g; }
    }
    __syncthreads();

    for (int c = 0; c < C; ++c) {
        const int64_t t = (int64_t)count[c * side + c];
        int64_t rank_p = chunk_base[(int64_t)c * n_chunks + chunk], rank_g = chunk_base[(int64_t)(C + c) * n_chunks + chunk];
        for (int w = 0; w < wave; ++w) { rank_p += s_tot[c][w]; rank_g += s_tot[DE_MAX_CLASSES + c][w]; }
        if (rank_p >= t && rank_g >= t) continue;                        // wave-uniform
#pragma unroll
        for (int s = 0; s < DE_SUB; ++s) {
            const bool in_p = p[s] == c, in_g = g[s] == c;
            const u64 mp = __ballot(in_p), mg = __ballot(in_g);
            const bool lost_p = in_p && !in_g && rank_p + lower_lanes(mp) < t;
            const bool lost_g = in_g && !in_p && rank_g + lower_lanes(mg) < t;
            if (lost_p || lost_g) {
                const u64 a = box_area(bbox, wave_node(s));
                atomicAdd(&s_lead[(lost_p ? 0 : DE_MAX_CLASSES) + c], a);
            }
            rank_p += __popcll(mp);
            rank_g += __popcll(mg);
        }
    }
    __syncthreads();
    if (tid < 2 * C) {
        const int which = tid / C, c = tid - which * C;
        const u64 v = s_lead[which * DE_MAX_CLASSES + c];
        if (v) atomicAdd(reinterpret_cast<u64*>(lead_out) + tid, v);
    }
}

int64_t chunks_of(int64_t n_nodes) { return gte::ceil_div(n_nodes, DE_CHUNK); }

}  // namespace

extern "C" int gte_doc_eval_max_classes(void) { return DE_MAX_CLASSES; }
extern "C" int gte_doc_eval_chunk_nodes(void) { return DE_CHUNK; }

extern "C" int64_t gte_doc_eval_workspace_bytes(int64_t n_nodes, int n_classes) {
    if (n_nodes < 0 || n_nodes > INT32_MAX || n_classes < 1 || n_classes > DE_MAX_CLASSES) return -1;
    const int64_t cells = (int64_t)(n_classes + 1) * (n_classes + 1);
    return 2 * cells * 8 + gte::round_up(2 * (int64_t)n_classes * chunks_of(n_nodes) * 4, 8);
}

extern "C" int gte_doc_eval(const int32_t* gt, const int32_t* pred, const int32_t* bbox, int64_t n_nodes, int n_classes,
                            int64_t* area_out, int64_t* count_out, int64_t* lead_out, void* workspace, int64_t workspace_bytes,
                            void* stream) {
    if (n_nodes < 0 || n_classes < 1) return gte::fail(GTE_ERR_INVALID_ARGUMENT, "doc_eval: %lld nodes, %d classes", (long long)n_nodes, n_classes);
    if (n_classes > DE_MAX_CLASSES) return gte::fail(GTE_ERR_UNSUPPORTED, "doc_eval: %d classes exceed %d", n_classes, DE_MAX_CLASSES);
    if (n_nodes > INT32_MAX) return gte::fail(GTE_ERR_UNSUPPORTED, "doc_eval: %lld nodes exceed 2^31 - 1", (long long)n_nodes);
    if (!area_out || !count_out || !lead_out || !workspace || (n_nodes > 0 && (!gt || !pred || !bbox)))
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "doc_eval: null pointer");
    if (((uintptr_t)bbox & 15) != 0 || (((uintptr_t)gt | (uintptr_t)pred) & 3) != 0 ||
        (((uintptr_t)area_out | (uintptr_t)count_out | (uintptr_t)lead_out | (uintptr_t)workspace) & 7) != 0)
        return gte::fail(GTE_ERR_INVALID_ARGUMENT, "doc_eval: bbox must be 16-byte aligned, gt and pred 4-byte, outputs and workspace 8-byte");
    const int64_t need = gte_doc_eval_workspace_bytes(n_nodes, n_classes);
    if (workspace_bytes < need)
        return gte::fail(GTE_ERR_WORKSPACE_TOO_SMALL, "doc_eval: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);

    const int cells = (n_classes + 1) * (n_classes + 1);
    const int n_chunks = (int)chunks_of(n_nodes);
    u64* accum = static_cast<u64*>(workspace);
    int32_t* chunk_cnt = reinterpret_cast<int32_t*>(accum + 2 * cells);
    hipStream_t st = gte::as_stream(stream);
    const hipError_t e = hipMemsetAsync(accum, 0, (size_t)2 * cells * 8, st);
    if (e != hipSuccess) return gte::fail(GTE_ERR_LAUNCH, "doc_eval: memset: %s", hipGetErrorString(e));
    if (n_chunks > 0) {
        hipLaunchKernelGGL(doc_tally_kernel, dim3((unsigned)n_chunks), dim3(DE_THREADS), 0, st, gt, pred, bbox, n_nodes, n_classes, accum,
                           chunk_cnt, n_chunks);
        if (int rc = gte::check_launch("doc_eval: tally")) return rc;
    }
    hipLaunchKernelGGL(doc_scan_kernel, dim3(1), dim3(DE_THREADS), 0, st, accum, n_classes, chunk_cnt, n_chunks, area_out, count_out,
                       lead_out);
    if (int rc = gte::check_launch("doc_eval: scan")) return rc;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(doc_lead_kernel, dim3((unsigned)n_chunks), dim3(DE_THREADS), 0, st, gt, pred, bbox, n_nodes, n_classes,
                           accum + cells, chunk_cnt, n_chunks, lead_out);
        if (int rc = gte::check_launch("doc_eval: lead")) return rc;
    }
    return GTE_OK;
}
