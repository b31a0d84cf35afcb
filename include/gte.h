/* gte.h -- C ABI of libgte_hip.so: the MI355X (gfx950) hot path of GNN-TableExtraction.
 *
 * The reference (AILab-UniFI/GNN-TableExtraction) has no FFI: its boundary for this path
 * is a Python nn.Module API (src/components/graphs/models.py:15-116) that reaches the
 * arithmetic through DGL (update_all / gSpMM) and PyTorch (Linear, LayerNorm, ReLU,
 * CrossEntropyLoss, Adam).  Each entry point below replaces one of those call sites; the
 * reference file:line it replaces is cited on the declaration.  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes; no C++/torch types, no exceptions.
 *   - every pointer is a BORROWED DEVICE pointer (hipMalloc'ed by the caller, e.g. a torch
 *     tensor's data_ptr()); the caller keeps it alive until the stream has drained.
 *   - outputs and workspaces are pre-allocated by the caller; nothing is allocated inside
 *     (graph-capture safe).  Workspace sizes come from the *_workspace_bytes() queries.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every launch
 *     goes to that stream; no call synchronises.
 *   - return 0 on success, a negative gte_status otherwise; gte_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - re-entrant and thread-safe (autograd calls backward from another thread).  Forced
 *     configurations are thread-local (each setter says so); what a kernel needs from the
 *     device it runs on -- the opt-in to more than 64 KB of dynamic LDS -- is made per DEVICE,
 *     for the device that is current at the call: a process may drive several.
 *   - "ld*" arguments are leading dimensions in ELEMENTS (row stride); rows need only be
 *     4-byte aligned (F = 831 is a first-class shape), 16-byte alignment is faster.
 */
#ifndef GTE_H_
#define GTE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTE_VERSION 400 /* major*10000 + minor*100 + patch */

enum gte_status {
    GTE_OK = 0,
    GTE_ERR_INVALID_ARGUMENT = -1,
    GTE_ERR_LAUNCH = -2,
    GTE_ERR_WORKSPACE_TOO_SMALL = -3,
    GTE_ERR_UNSUPPORTED = -4,
};

enum gte_reduce { GTE_REDUCE_SUM = 0, GTE_REDUCE_MEAN = 1 }; /* MEAN: sum * 1/in_degree, 0 if none */
enum gte_dtype { GTE_F32 = 0, GTE_BF16 = 1 };

int gte_version(void);
const char* gte_last_error(void);
/* Device facts the host side sizes launches with: compute units, wave size, LDS bytes/CU. */
int gte_device_info(int* compute_units, int* wave_size, int* lds_bytes, char* arch_name, int arch_name_len);

/* ------------------------------------------------------------------------------------------
 * A6 / A9  neighbour aggregation (CSR gather SpMM)
 * replaces  models.py:53-54  g.update_all(fn.u_mul_e('h','feat','m'), fn.sum('m','h'))
 *           models.py:146-149 (fn.mean reducer)  and  models.py:74-78 get_norm (REDUCE_MEAN
 *           folds norm = 1/in_degree, inf->0, into the epilogue; in_degree = indptr[v+1]-indptr[v])
 *   out[v, 0:F] = scale_v * sum_{e in [indptr[v], indptr[v+1])} w[e] * x[indices[e], 0:F]
 * The same entry point run on the out-edge CSR is the backward of A6 (A7, DGL GSpMM.backward).
 * indptr: int32[n_rows+1]; indices: int32[nnz] (row ids of x); eweight: f32[nnz] or NULL (=1.0).
 * dtype GTE_BF16: x/out are bf16 (uint16 storage), accumulation in f32.
 * Non-finite inputs (gte_spmm_csr, _accumulate, _accumulate_ln(_p3), _p3, _edge, _tiled): row v reads the rows of x its edges
 * name and no others -- where a kernel pads a row's edge list to its unroll it re-uses a source of THAT row at weight 0 -- so an
 * Inf or NaN in x[u, c] reaches out[v, c] of the out-neighbours v of u only (there it is Inf or NaN; 0 * Inf from the padding
 * may turn an Inf into a NaN), and every other element is bit for bit what it is with x[u, c] = 0.  A zero WEIGHT on a non-finite
 * source is a NaN, as in the reference.
 * ---------------------------------------------------------------------------------------- */
int gte_spmm_csr(const int32_t* indptr, const int32_t* indices, const float* eweight,
                 const void* x, int64_t ldx, void* out, int64_t ldo,
                 int64_t n_rows, int64_t n_feat, int dtype, int reduce, void* stream);

/* The same contraction with the work split by EDGES instead of by rows -- the edge-parallel, wavefront-level segmented
 * reduction BASELINE.json's north_star names for the call site models.py:53-54: one wave per segment of 64 consecutive edges
 * of the CSR order, reduced segmented by destination row (lanes across the features, four source rows in flight); rows cut
 * by a segment boundary leave partial sums in `workspace` and a second pass adds them in segment order (deterministic).  For
 * graphs with hub rows (max in-degree > 64): a 3 000-edge row is 47 waves instead of one lane group walking 750 rounds.  fp32;
 * equal to gte_spmm_csr up to the summation order of rows that span segments. */
int64_t gte_spmm_csr_edge_workspace_bytes(int64_t n_edges, int64_t n_feat);
int gte_spmm_csr_edge(const int32_t* indptr, const int32_t* indices, const float* eweight, const float* x, int64_t ldx,
                      float* out, int64_t ldo, int64_t n_rows, int64_t n_edges, int64_t n_feat, int reduce, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* Same contraction, but ACCUMULATING into out (out += ...): lets the backward add the
 * transpose-aggregated gradient onto the self-path gradient without a temporary. */
int gte_spmm_csr_accumulate(const int32_t* indptr, const int32_t* indices, const float* eweight,
                            const void* x, int64_t ldx, void* out, int64_t ldo,
                            int64_t n_rows, int64_t n_feat, int dtype, int reduce, void* stream);

/* LDS-staged variant of the same contraction for graphs with locality (page graphs: consecutive
 * destination rows share most sources).  A workgroup owns a tile of gte_spmm_tile_rows() consecutive
 * destination rows, stages the tile's DISTINCT source rows in LDS once per 32-float feature chunk and
 * reduces from LDS in CSR order (bit-identical to gte_spmm_csr).  Tile metadata is graph structure,
 * built once per graph by the caller:
 *   tile_ptr    int32[n_tiles+1]  offsets into tile_src        (n_tiles = ceil(n_rows / tile_rows))
 *   tile_src    int32[...]        distinct source rows of each tile
 *   local_index uint16[nnz]       position of indices[e] inside its tile's tile_src segment
 * Tiles with more than 128 distinct sources or 448 edges (or whose sources span 4 GB of x) are gathered directly (no size
 * limit on the graph).  Widths that are a multiple of 32 with at least 128 columns keep two chunks in flight (faster).
 * fp32 only.  accumulate != 0: out += ... */
int gte_spmm_tile_rows(void);
int gte_spmm_csr_tiled(const int32_t* indptr, const int32_t* indices, const uint16_t* local_index,
                       const float* eweight, const int32_t* tile_ptr, const int32_t* tile_src,
                       const float* x, int64_t ldx, float* out, int64_t ldo,
                       int64_t n_rows, int64_t n_feat, int reduce, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Graph preparation (what DGL does lazily per batched graph before gSpMM / its backward)
 * replaces  dgl.graph((u,v)) COO->CSC build (builder.py:425) and the reverse-CSR build DGL
 *           performs for GSpMM.backward; SURVEY 8(f) N1.
 * gte_coo_to_csr: stable counting sort of E edges by `key` (destination for the in-edge CSR,
 *   source for the out-edge CSR).  Writes indptr[n+1], indices[E] = other[perm], perm[E]
 *   (edge ids in row order; within a row ascending edge id => fixed summation order), and, if
 *   eweight != NULL, wout[E] = eweight[perm] * (scale_by_indeg ? 1/in_degree(dst) : 1).
 * workspace: gte_coo_to_csr_workspace_bytes(n, E).
 * ---------------------------------------------------------------------------------------- */
int64_t gte_coo_to_csr_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int gte_coo_to_csr(const int32_t* key, const int32_t* other, const float* eweight,
                   const float* row_scale /* f32[n] or NULL: multiplies wout by row_scale[other] */,
                   int64_t n_nodes, int64_t n_edges,
                   int32_t* indptr, int32_t* indices, int32_t* perm, float* wout,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* Device-side batching of RESIDENT pages (replaces dgl.batch(...).to(device), model_train.py:297, per step).
 * Dataset arrays (built once): node_off[P+1], edge_off[P+1]; indptr_loc packed per page (page p's n_p+1 entries
 * start at node_off[p] + p and count from 0); indices_loc = column ids local to the page; weight in CSR order.
 * Batch = pages[n_batch] with b_node_off[n_batch+1], b_edge_off[n_batch+1] (exclusive prefix sums of the chosen
 * pages' node / CSR-entry counts, computed by the caller from host metadata).  Writes the block-diagonal CSR:
 * indptr_out[n_out+1], indices_out[e_out] (global ids), weight_out[e_out] (nullable).  Pure index work, no sort. */
int gte_batch_csr(const int32_t* pages, int64_t n_batch, const int32_t* node_off, const int32_t* edge_off,
                  const int32_t* b_node_off, const int32_t* b_edge_off, const int32_t* indptr_loc,
                  const int32_t* indices_loc, const float* weight, int32_t* indptr_out, int32_t* indices_out,
                  float* weight_out, int64_t n_out, int64_t e_out, void* stream);
/* ---- bf16 projection of the GAT (BASELINE configs[2] "4-head GAT bf16"; SURVEY A13: no reference symbol, parity unpinned) ------
 * gte_cast_bf16     y[r, :] = bf16(act(x[r, :])), act 0 = identity, 1 = ELU (the activation between GAT layers), zero padded to a
 *                   multiple of 8 columns; y 16-byte aligned, ldy a multiple of 8.
 * gte_gemm_bf16_nt  C[M, N] (fp32) = A[M, K] B[N, K]^T with bf16 operands on v_mfma_f32_32x32x16_bf16, fp32 accumulation
 *                   (z = X W^T of a GAT layer; W stored [heads * dim, in_feats] like nn.Linear).  Operands 16-byte aligned, K and
 *                   the leading dimensions multiples of 8 (gte_cast_bf16 produces exactly that).
 * Contract (tests/test_gpu_bf16_projection.py against tests/bf16_ref.py):
 *   rounding   fp32 -> bf16 is round to nearest, ties to the even mantissa, as torch.bfloat16 converts: fp32 and bf16 subnormals are
 *              kept (nothing is flushed), +-0 keeps its sign, NaN -> NaN, |x| >= 0x7F7F8000 (above the largest bf16's tie) -> +-inf.
 *   padding    columns [cols, round_up(cols, 8)) of y are +0 whatever x holds past cols (ldx > cols); columns from there to ldy and
 *              rows >= rows are not written.
 *   ELU        act 1: v for v >= 0 (so ELU(-0) = -0, ELU(+inf) = +inf), expm1f(v) below (ELU(-inf) = -1, and -1 from about v <= -17),
 *              NaN -> NaN; the fp32 value is then rounded as above.  Against expm1 in float64 the bf16 result can differ (by one bf16
 *              neighbour) only where that value lies within a few fp32 ulps of a bf16 rounding midpoint.
 *   product    K = 0 writes zeros.  Exactly the [M, N] window of C is written for any ldc >= N and any alignment of C: rows >= M and
 *              columns >= N of the tiles are dropped (also where 0 * inf made them NaN), on the buffer-descriptor stores taken while
 *              (M + 128) * ldc * 4 < 2^31 and on the plain guarded stores beyond.  Non-finite operands follow IEEE (0 * inf = NaN,
 *              inf - inf = NaN) and reach only the outputs whose dot product holds them.
 *   accuracy   products of bf16 values are exact in fp32 and partial sums are rounded fp32 additions (subnormals kept):
 *              |C - A B^T| <= K * 2^-24 * sum_k |a_k b_k|, bit-exact where every partial sum is representable; measured <= 2 of
 *              these units up to K = 1024, not above the fp32 MFMA kernel's error + 1. */
int gte_cast_bf16(const float* x, int64_t ldx, uint16_t* y, int64_t ldy, int64_t rows, int64_t cols, int activation, void* stream);
int gte_gemm_bf16_nt(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N,
                     int64_t K, void* stream);

/* ---- k-NN page-graph construction --------------------------------------------------------------
 * Replaces GraphBuilder.get_graph(mode='knn') edge building (builder.py:240-292 over the projections of :383-395), dgl.to_simple +
 * dgl.to_bidirected (loader.py:319-320) and fast_remove_islands (builder.py:567-582) for a whole set of pages at once.
 * Inputs: bbox int32 [n_nodes, 4] (x0, y0, x1, y1; all pages concatenated, 16-byte aligned; boxes on the canvas:
 * 0 <= x0 <= x1 <= width, 0 <= y0 <= y1 <= height), node_off[n_pages + 1], page_size int32 [n_pages, 2] = (width, height).
 * Equal-distance candidates are ordered by (distance, node id) -- the reference's order among ties is an implementation detail
 * of CPython sets and numpy's argsort (oracle/knn_graph.py, pinned on the reference's own output, does the same).
 *   gte_knn_select  sel[n_nodes, k]: global ids of each node's selected neighbours (nearest first), -1 padded; k <= gte_knn_max_k(),
 *                   pages of at most gte_knn_max_page_nodes() boxes.
 *   gte_knn_csr     the in-edge CSR (rows = destinations, sources ascending, no duplicates) from sel: call with fill = 0 to get
 *                   indptr[n_nodes + 1] (workspace >= gte_knn_csr_workspace_bytes), read E = indptr[n_nodes], then with fill = 1 to
 *                   write indices[E] (sources) and dst_of[E] (the row of every entry: the COO form gte_edge_weights_bbox takes).
 *                   bidirectional != 0: symmetric closure (to_simple + to_bidirected); else the reference's directed edge list.
 *   gte_island_mask island[v] = 1 for nodes labelled text_label from which no walk of exactly khop steps over the (symmetric)
 *                   CSR ends at a node with another label; workspace >= 2 * n_nodes bytes.
 * Integer work only; no atomics, no sort: deterministic. */
/* Visibility mode of the same builder (builder.py:294-379): sel[n_nodes, 4] = every node's nearest visible box to the top /
 * right / bottom / left (global ids, -1 none; the reference's order-dependent update rules, restated in
 * oracle/visibility_graph.py and pinned on its own output) with the vertical edges that cross a horizontal edge removed
 * (remove_vertical()).  The graph is gte_knn_csr(sel, k = 4, bidirectional = 1).  bbox and sel 16-byte aligned. */
int gte_visibility_select(const int32_t* bbox, const int32_t* node_off, const int32_t* page_size, int64_t n_pages,
                          int64_t n_nodes, int64_t max_page_nodes, int max_dist, int32_t* sel, void* stream);
int gte_knn_max_k(void);
int gte_knn_max_page_nodes(void);
int gte_knn_select(const int32_t* bbox, const int32_t* node_off, const int32_t* page_size, int64_t n_pages, int64_t n_nodes,
                   int64_t max_page_nodes, int k, int max_dist, int32_t* sel, void* stream);
int64_t gte_knn_csr_workspace_bytes(int64_t n_nodes);
int gte_knn_csr(const int32_t* sel, const int32_t* node_off, const int32_t* page_of_node, int64_t n_nodes, int k,
                int bidirectional, int fill, int32_t* indptr, int32_t* indices, int32_t* dst_of, void* workspace,
                int64_t workspace_bytes, void* stream);
int gte_island_mask(const int32_t* indptr, const int32_t* indices, const int32_t* label, int64_t n_nodes, int khop,
                    int text_label, uint8_t* island, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- page regions from node predictions (no reference counterpart: graphs/utils.py get_subgraph_bbox() is a stub) -
 * Inputs: the in-edge CSR of the batch (rows = destinations; any CSR over the batch's nodes does: a directed one gives the answer
 * of its symmetric closure), node_off[n_pages + 1] (node_off[0] = 0, node_off[n_pages] = n_nodes; empty pages are legal), group
 * int32 [n_nodes] = the region kind of every node (< 0: the node belongs to no region), bbox int32 [n_nodes, 4] (x0, y0, x1, y1).
 * Take the undirected graph on the nodes with group >= 0 that has an edge {u, v} wherever the CSR holds u -> v or v -> u and
 * group[u] == group[v] (self loops and duplicate entries change nothing; an entry that leaves its page is skipped):
 *   comp[v]          the smallest node id of v's connected component (global ids); -1 where group[v] < 0.  A node with
 *                    comp[v] == v is a ROOT; a node without a same-group neighbour is a region of one word.
 *   region_count[v]  roots: the number of members of the component; every other row 0.
 *   region_box[v]    roots: (min x0, min y0, max x1, max y1) over the members; every other row (0, 0, 0, 0).
 * Every row of the three outputs is written.  One launch for the batch, one workgroup per page with the page's labels in LDS
 * (pages of at most gte_region_max_page_nodes() >= gte_knn_max_page_nodes() nodes: any page the graph builder accepts;
 * GTE_ERR_UNSUPPORTED above); max_page_nodes = the largest page of the batch (it sizes the launch's LDS).  Integer work on LDS
 * atomic min / max / add: deterministic.  No allocation, no workspace, no synchronisation.  bbox and region_box 16-byte aligned. */
int gte_region_max_page_nodes(void);
int gte_page_regions(const int32_t* indptr, const int32_t* indices, const int32_t* node_off, int64_t n_pages, int64_t n_nodes,
                     int64_t max_page_nodes, const int32_t* group, const int32_t* bbox, int32_t* comp, int32_t* region_box,
                     int32_t* region_count, void* stream);

/* gte_page_regions with a confidence per region, from the model's own logits, in the same launch.  logits float [n_nodes,
 * n_classes] (packed rows), class_group int32 [n_classes] = the region kind of every class (the table the caller derived `group`
 * from: group[v] = class_group[argmax logits[v]] is the usual choice, but `group` stays an input).  For a member word v of kind
 * k = group[v]:  p(v) = sum over the classes c with class_group[c] == k of softmax(logits[v])[c]  (fp32, max-subtracted; 0 for a
 * row that holds a non-finite logit), and
 *   region_score[v]  roots: the mean of p over the members; every other row 0.0f (a page above max_page_nodes: all 0.0f).
 * comp, region_box and region_count are bit for bit what gte_page_regions writes for the same `group`.  Deterministic: a word
 * adds q(v) = (uint32)(p(v) * 2^19 + 0.5) to its root with an LDS integer atomic (<= 4096 words of q <= 2^19: the sum fits 32
 * unsigned bits), and the score is (float)((double)sum / ((double)count * 2^19)) -- within 2^-18 of the exact mean.  n_classes
 * >= 1; the same limits, alignment and error codes as gte_page_regions. */
int gte_page_regions_scored(const int32_t* indptr, const int32_t* indices, const int32_t* node_off, int64_t n_pages, int64_t n_nodes,
                            int64_t max_page_nodes, const int32_t* group, const int32_t* bbox, const float* logits, int n_classes,
                            const int32_t* class_group, int32_t* comp, int32_t* region_box, int32_t* region_count,
                            float* region_score, void* stream);

/* ---- box matching for the box-level evaluation (AP at IoU thresholds; src/utils/metrics.py:20-114 get_single_image_results) ----
 * A CELL is one (page, kind) pair: its predicted boxes pred_box[pred_off[b] .. pred_off[b + 1]) in ASCENDING order of their score
 * and its ground-truth boxes gt_box[gt_off[b] .. gt_off[b + 1]); boxes are int32 (x0, y0, x1, y1), x0 <= x1, y0 <= y1, extents
 * (x1 - x0 + 1) <= 2^25 (a box outside that overlaps nothing).  iou_thr: HOST array of n_thr (1 .. 16) finite thresholds >= 0 in
 * ascending order.  With R_b / G_b the cell's box counts and R = pred_off[n_cells]:
 *   iou(p, g)      0 where the boxes are disjoint (x1 < x0' ...: boxes that touch are NOT disjoint), otherwise
 *                  inter / (area_p + area_g - inter) with the +1 pixel convention, exact integers divided in fp64;
 *   tp[j * R + pred_off[b] + k]   the number of matches between the ground truths and the predictions k .. R_b - 1 (what is left
 *                  after pruning the k lowest-scored boxes) at iou_thr[j]: candidates are the pairs with iou > iou_thr[j],
 *                  strictly; they are taken greedily in descending IoU, among equal IoUs the larger p * G_b + g first (p, g:
 *                  positions inside the cell), a pair is a match when neither of its boxes is matched yet.
 *                  (false positives = R_b - k - tp, false negatives = G_b - tp: the caller's arithmetic.)
 *   cell_status[b] 0: fine; 1: the cell has more than gte_box_match_max_candidates() pairs above iou_thr[0], its tp entries are
 *                  all -1; 2: the cell exceeds max_pred_per_cell / max_gt_per_cell or its offsets are not ascending inside
 *                  [0, R] / [0, G] (tp -1 where the rows exist).  Other cells are not affected.
 * A cell with R_b = 0 or G_b = 0 writes its (possibly empty) rows of zeros and status 0.  max_pred_per_cell / max_gt_per_cell =
 * the largest R_b / G_b (the offsets live on the device): above gte_box_match_max_boxes() the call returns GTE_ERR_UNSUPPORTED
 * before any launch.  One launch, one workgroup per cell, integer outputs, no workspace, no synchronisation.  pred_box and gt_box
 * 16-byte aligned. */
int gte_box_match_max_boxes(void);        /* per cell and side: 256 */
int gte_box_match_max_candidates(void);   /* per cell: 4096 */
int gte_box_match(const int32_t* pred_box, const int32_t* pred_off, const int32_t* gt_box, const int32_t* gt_off, int64_t n_cells,
                  int64_t max_pred_per_cell, int64_t max_gt_per_cell, const double* iou_thr, int n_thr, int32_t* tp,
                  int32_t* cell_status, void* stream);

/* gte_box_match on FLOAT boxes: the document of the block route (postprocessing_2.py:197-348, coordinates divided by 0.36) against
 * annotation boxes, what the reference's models/evaluate.py:64-131 scores.  The same cells, offsets, tp layout, status codes and
 * limits; pred_box / gt_box are double [., 4], 16-byte aligned.  The IoU is calc_iou_individual() of src/utils/metrics.py:20-54 in
 * IEEE double, one rounding per operation, in this order and with no contraction:
 *   disjoint (x2_t < x1_p || x2_p < x1_t || y2_t < y1_p || y2_p < y1_t): 0.0; otherwise
 *   inter = ((far_x - near_x) + 1) * ((far_y - near_y) + 1),  area = ((x2 - x1) + 1) * ((y2 - y1) + 1) per box,
 *   iou = inter / ((true_area + pred_area) - inter).
 * A box is well formed when its four values are finite, x0 <= x1, y0 <= y1 and |v| <= 2^24; any other box overlaps nothing (IoU
 * 0.0 with every box).  A non-finite quotient is no candidate.  Candidates are iou > iou_thr[j] strictly, order = IoU descending,
 * then p * G_b + g descending (the reference leaves ties unspecified: np.argsort(ious)[::-1], metrics.py:94).
 *   iou (NULL: not written, no cost)   cell b's R_b x G_b matrix, row-major (p * G_b + g), at iou[iou_off[b] ...]: every pair's
 *                  IoU whatever the thresholds.  iou_off int64 [n_cells + 1] on the device, iou_off[b + 1] - iou_off[b] ==
 *                  R_b * G_b; a cell whose entries do not say so ends with status 2 (tp -1) as for wrong maxima.  A cell that
 *                  ends with status 2 writes nothing to iou; a cell with status 1 has its matrix written. */
int gte_box_match_f64(const double* pred_box, const int32_t* pred_off, const double* gt_box, const int32_t* gt_off, int64_t n_cells,
                      int64_t max_pred_per_cell, int64_t max_gt_per_cell, const double* iou_thr, int n_thr, int32_t* tp,
                      int32_t* cell_status, double* iou, const int64_t* iou_off, void* stream);

/* ---- layout blocks labelled by the vote of their words (postprocessing_2.py:240-258, the words x blocks loop of get_objects_bboxs) -
 * Inputs: bbox int32 [n_nodes, 4] the word boxes; word_cat int32 [n_nodes] the category of every word (a value < 0 or >= n_cat:
 * the word is still assigned to a block but casts no vote); block_box double [n_blocks, 4] the layout blocks ALREADY DIVIDED by
 * the scale factor on the host (numpy float64 `blocks / 0.36`: bit for bit the reference's b / sf); node_off[n_pages + 1] and
 * block_off[n_pages + 1] the pages' runs (first entry 0, last entry n_nodes / n_blocks; empty pages and pages without blocks are
 * legal).  Both rectangles are normalised per axis (lo = min, hi = max of the two corners); a word MEETS a block when
 * max(lo, lo') <= min(hi, hi') on both axes -- closed, touching counts -- evaluated in fp64 (int32 -> double is exact); a block
 * with a NaN coordinate meets nothing.
 *   word_block[v]    the global index of the FIRST block (lowest index) of v's page that v meets; -1 where there is none.
 *   votes[b * n_cat + c]   the sum over the words v with word_block[v] == b and word_cat[v] == c of 2 if c == double_cat (the
 *                    reference: TITLE), else 1; double_cat = -1: no category counts double.
 *   block_label[b]   the LOWEST category with the largest count; 0 for a block without votes (l.index(max(l))).
 * Every row of the three outputs is written.  One launch for the batch, one workgroup per page, the page's blocks and counters in
 * LDS; max_page_blocks = the largest page's block count (it sizes the launch's LDS; a page above it gets -1 / 0 / 0): above
 * gte_block_vote_max_page_blocks() or with n_cat > gte_block_vote_max_categories() the call returns GTE_ERR_UNSUPPORTED before any
 * launch.  Integer work on LDS atomic add: deterministic.  No allocation, no workspace, no synchronisation.  bbox 16-byte aligned. */
int gte_block_vote_max_page_blocks(void);   /* 512 */
int gte_block_vote_max_categories(void);    /* 16 */
int gte_block_vote(const int32_t* bbox, const int32_t* node_off, const int32_t* word_cat, const double* block_box,
                   const int32_t* block_off, int64_t n_pages, int64_t n_nodes, int64_t n_blocks, int64_t max_page_blocks, int n_cat,
                   int double_cat, int32_t* word_block, int32_t* votes, int32_t* block_label, void* stream);

/* ---- word labels and figure nodes from page annotations (builder.py:151-167 get_label with utils.py:107-108 center; the two loops
 * of get_nodes, builder.py:195-216) ----
 * Inputs, pages concatenated: bbox int32 [n_nodes, 4] the word boxes (x0, y0, x2, y3), 16-byte aligned; node_off[n_pages + 1];
 * ann_box double [n_ann, 4] the annotation rectangles (r0, r1, r2, r3) AS GIVEN -- they are not normalised: an inverted rectangle
 * contains nothing, as in the reference, and so does one with a NaN coordinate; ann_cat int32 [n_ann] their categories;
 * ann_off[n_pages + 1]; 1 <= n_cat <= 32; skip_mask: bit c set = an annotation of category c never labels a word (the reference:
 * {4, 9, 11, 12} = TABLE, TABLE_GCELL, TABLE_COL, TABLE_ROW, builder.py:159); figure_cat in [0, n_cat) (the reference: 5).  Empty
 * pages and pages without annotations are legal.
 * For word v of page p:  cx = (x0 + x2) / 2, cy = (y0 + y3) / 2, the sums in 64-bit integers, C's division (towards zero): for
 * every int32 box that is int(x2 - (x2 - x0) / 2) of center().  The page's annotations are scanned in index order; one whose
 * category is in skip_mask or outside [0, n_cat) is passed over; the FIRST of the others with
 *     cx > r0 && cx < r2 && cy > r1 && cy < r3      (strict, fp64, on exact values)
 * WINS and the scan ends there (a FIGURE annotation behind an earlier winner does not drop the word).
 *   word_ann[v]      the winner's global index; -1 where there is none.
 *   word_label[v]    the winner's category; -1 where that is figure_cat (the word is DROPPED); 0 (OTHER) where there is none.
 *   page_counts[p]   (the page's annotations with category figure_cat -- passed over or not --, its words with word_label >= 0).
 * gte_word_labels: one launch, one workgroup per page, the annotations staged through LDS in chunks of gte_word_labels_chunk():
 * no limit on the annotations of a page, no GTE_ERR_UNSUPPORTED.  A page whose runs are not ascending inside [0, n_nodes] /
 * [0, n_ann] writes page_counts (0, 0) and nothing else.  Counts are LDS integer atomics: deterministic.
 *
 * gte_word_labels_compact: the node list of get_nodes from word_label.  out_off int32 [n_pages + 1] on the device: the caller's
 * exclusive cumulative sum of figures + kept words (page_counts summed per page); cat_map int32 [n_cat] or NULL for the identity
 * (LableModification.origin_to_conv, labels.py:13-19, with -1 for None).  Page p writes the rows out_off[p] ...:
 *   first its annotations of category figure_cat, in annotation order:  out_bbox = the four doubles clamped to [-2^30, 2^30] (NaN ->
 *     0) and converted to int32 (towards zero);  out_src = -1 - the annotation's global index;  out_label = cat_map[figure_cat];
 *   then its words with word_label >= 0, in word order:  out_bbox = the word's box;  out_src = the word's global index;
 *     out_label = cat_map[word_label] (-1 for a word_label >= n_cat).
 *   page_status[p]   0: written; 2: the page's runs are not ascending inside their arrays ([0, n_out] for out_off) or
 *     out_off[p + 1] - out_off[p] is not what the kernel counts: the page writes NOTHING.  Other pages are not affected.
 * Ranks come from a workgroup prefix scan (wave ballot, popcount of the lower lanes, per-wave totals in LDS): no atomics, the order
 * is exact.  out_bbox 16-byte aligned.
 * Both: no allocation, no workspace, no synchronisation; null or misaligned pointers, sizes >= 2^31 - 1, n_cat outside 1 .. 32 or
 * figure_cat outside [0, n_cat) return GTE_ERR_INVALID_ARGUMENT before any launch; n_pages == 0 is GTE_OK. */
int gte_word_labels_chunk(void);            /* 1024 */
int gte_word_labels(const int32_t* bbox, const int32_t* node_off, const double* ann_box, const int32_t* ann_cat,
                    const int32_t* ann_off, int64_t n_pages, int64_t n_nodes, int64_t n_ann, int n_cat, uint32_t skip_mask,
                    int figure_cat, int32_t* word_label, int32_t* word_ann, int32_t* page_counts, void* stream);
int gte_word_labels_compact(const int32_t* bbox, const int32_t* node_off, const int32_t* word_label, const double* ann_box,
                            const int32_t* ann_cat, const int32_t* ann_off, const int32_t* out_off, const int32_t* cat_map,
                            int64_t n_pages, int64_t n_nodes, int64_t n_ann, int n_cat, int figure_cat, int64_t n_out,
                            int32_t* out_bbox, int32_t* out_label, int32_t* out_src, int32_t* page_status, void* stream);

/* ---- confidence of a page's FINAL blocks (after table assembly and figures; the reference's write_json gives every block 1.0,
 * postprocessing_2.py:337) ----
 * Inputs: bbox int32 [n_nodes, 4] the word boxes; logits float [n_nodes, .] the words' logit rows, row v at logits + v * ld_logits
 * (ld_logits >= n_classes, 1 <= n_classes <= 16); block_box double [n_blocks, 4] the final blocks in WORD coordinates (already
 * divided by the scale factor where they were not yet); block_cat int32 [n_blocks] their categories; cat_classes uint32 [n_cat]
 * (device, 1 <= n_cat <= 16): bit c of cat_classes[k] set = class c counts for a block of category k (a category outside
 * [0, n_cat) has the empty mask; bits at and above n_classes are ignored); node_off / block_off [n_pages + 1] as for gte_block_vote.
 * A word MEETS a block under gte_block_vote's closed rectangle test (corners normalised, fp64, a block with a NaN corner meets
 * nothing) and counts in EVERY block of its page it meets, not only the first.  For word v and a block of category k:
 *   q(v, k) = (uint32)(num / den * 2^19 + 0.5f), the fp32 max-subtracted softmax of v's row, den the sum of all classes'
 *             exponentials and num that of the classes in cat_classes[k], both in ascending class order -- bit for bit the word
 *             score of gte_page_regions_scored for the same set; 0 for a row with a non-finite logit (which still counts as a word).
 *   n_words[b]  the number of words that meet block b.
 *   score[b]    (float)((double)sum_v q(v, k_b) / ((double)n_words[b] * 2^19)); 1.0f where no word meets b.  Within 2^-18 of the mean.
 * One launch, one workgroup per page, the blocks and two u32 sums per block in LDS (integer atomics: deterministic).
 * max_page_words / max_page_blocks = the largest page's counts: above gte_block_scores_max_page_words() (4096: the sum of q fits 32
 * bits) / gte_block_scores_max_page_blocks(), or with more classes / categories than the limits, the call returns
 * GTE_ERR_UNSUPPORTED before any launch.  A page above the stated maxima writes n_words -1 and score 0; a page whose offsets name
 * no rows writes nothing.  No allocation, no workspace, no synchronisation.  bbox 16-byte aligned. */
int gte_block_scores_max_page_blocks(void);   /* 512 */
int gte_block_scores_max_page_words(void);    /* 4096 */
int gte_block_scores_max_classes(void);       /* 16 */
int gte_block_scores_max_categories(void);    /* 16 */
int gte_block_scores(const int32_t* bbox, const int32_t* node_off, const float* logits, int64_t ld_logits, int n_classes,
                     const double* block_box, const int32_t* block_off, const int32_t* block_cat, const uint32_t* cat_classes,
                     int n_cat, int64_t n_pages, int64_t n_nodes, int64_t n_blocks, int64_t max_page_words, int64_t max_page_blocks,
                     float* score, int32_t* n_words, void* stream);

/* ---- table grids: rows, columns and cells of the tables another stage has named (no reference counterpart: the reference stops at
 * where a table is; graphs/utils.py get_subgraph_bbox() is a stub) -- the projection profile as exact integer arithmetic ----
 * Inputs, pages concatenated: bbox int32 [n_nodes, 4] the word boxes (x0, y0, x1, y1); node_off[n_pages + 1]; table int32 [n_nodes]
 * the id of every word's table (by convention the root of its region, gte_page_regions' comp; < 0: none); role int32 [n_nodes] the
 * category of every word.  The T = n_tables LISTED tables: table_root[t] the id, table_page[t] the page whose words are scanned for
 * table[v] == table_root[t] (its MEMBERS), table_gap[2 t], table_gap[2 t + 1] = (gap_x, gap_y).  col_roles / row_roles: bit k set =
 * words of category k build the column / row profile.
 * The rule, per table, for the x axis with gap = gap_x and roles = col_roles (the y axis: y0 / y1, gap_y, row_roles):
 *   interval   a member has lo = min(x0, x1), hi = max(x0, x1), hi1 = max(hi, lo + 1) (a zero-width word still occupies one pixel);
 *              origin = min lo over all members.
 *   status 2   max hi1 - origin > gte_table_grid_max_extent() on either axis, a gap outside 0 .. gte_table_grid_max_gap(), or a
 *              member coordinate outside -2^30 .. 2^30: no grid -- shape (0, 0), the members' rows get cell = -1, cell_box = 0.
 *   profile    a member is a PROFILE WORD of the axis when 0 <= role < 32 and bit role of roles is set; it occupies the pixels
 *              [lo, hi1 + gap).
 *   bands      the maximal runs of occupied pixels, numbered from 0 in ascending coordinate (two neighbouring profile words share a
 *              band exactly when the free space between them is <= gap); the EXTENT of a band is [run start, run end - gap).
 *   span       of EVERY member, profile word or not: c0 / c1 = the bands of the first / last occupied pixel inside [lo, hi1);
 *              (-1, -1) when no pixel inside is occupied.  (A profile word has c0 == c1; a word that is none and lies within gap
 *              pixels behind a band's last word meets that band, as a profile word there would have joined it.)
 * With r0 / r1 the span on the y axis:
 *   cell[v]         (r0, r1, c0, c1)
 *   cell_box[v]     (start of band c0, start of band r0, end of band c1, end of band r1), page coordinates; an axis with span
 *                   (-1, -1) gives 0 for both of its entries.
 *   table_shape[t]  (n_rows, n_cols) = the band counts of the y / x axis.
 *   table_box[t]    (min lo_x, min lo_y, max hi1_x, max hi1_y) over the members.
 *   table_words[t]  the member count.
 *   table_status[t] 0: fine (an axis without profile words simply has 0 bands);  1: no member on that page (a negative
 *                   table_root names no table) -- shape (0, 0), box 0;  2: as above (box as stated, but 0 when a coordinate is out
 *                   of range);  3: table_page[t] lies outside [0, n_pages) or its offsets leave [0, n_nodes] or descend -- shape
 *                   (0, 0), box 0, words 0.
 * Rows of cell / cell_box of words that are members of no listed table are NOT touched (the caller pre-fills: -1 / 0); the four
 * per-table outputs are written for every listed table.  A table listed twice writes the same values twice.
 * One launch for the batch, one workgroup per listed table; static LDS only (two occupancy bitmaps of max_extent + max_gap bits
 * with their run-start words and scans: < 7 KB), so a page may hold any number of words.  Integer work on LDS atomic min / max /
 * add / or: deterministic.  No allocation, no workspace, no synchronisation; n_tables == 0 returns GTE_OK without a launch.
 * bbox, cell, cell_box and table_box 16-byte aligned. */
int gte_table_grid_max_extent(void);   /* 8192 pixels per axis */
int gte_table_grid_max_gap(void);      /* 1024 */
int gte_table_grid(const int32_t* bbox, const int32_t* node_off, int64_t n_pages, int64_t n_nodes,
                   const int32_t* table,        /* [n_nodes] root id of the word's table, < 0: none */
                   const int32_t* role,         /* [n_nodes] category of the word; outside 0..31: in no profile */
                   const int32_t* table_root, const int32_t* table_page, const int32_t* table_gap /* [T, 2] = (gap_x, gap_y) */,
                   int64_t n_tables, uint32_t col_roles, uint32_t row_roles,
                   int32_t* cell /* [n_nodes, 4] */, int32_t* cell_box /* [n_nodes, 4] */,
                   int32_t* table_shape /* [T, 2] */, int32_t* table_box /* [T, 4] */, int32_t* table_words /* [T] */,
                   int32_t* table_status /* [T] */, void* stream);

/* ---- area-weighted confusion of node predictions: the sums of the DocBank token metric and of the reference's evaluate_doc
 * (models/evaluate.py:182-202) ----
 * Inputs: gt, pred int32 [n_nodes], all pages concatenated; bbox int32 [n_nodes, 4] (x0, y0, x1, y1), 16-byte aligned;
 * C = n_classes, 1 <= C <= gte_doc_eval_max_classes().  area(v) = (x1 - x0) * (y1 - y0), the differences in 64 bits, the product
 * as int64: inverted corners give negative or zero areas, and they are summed as they are.  The caller keeps every sum inside
 * int64 (max |area| * n_nodes < 2^62 is enough).  A label or prediction outside [0, C) has index C, "none of the classes".
 * With P_c = the nodes with pred == c and G_c = those with gt == c, both in node order, T_c = P_c and G_c, t_c = |T_c|:
 *   area_out[g * (C+1) + p]   int64 [(C+1)^2]: the summed area of the nodes with gt index g and pred index p.
 *   count_out[g * (C+1) + p]  the same layout: their number.  t_c = count_out[c * (C+1) + c].
 *   lead_out[c]               int64 [2 C]: the summed area of the nodes of P_c \ T_c whose 0-based position within P_c is < t_c;
 *   lead_out[C + c]           the same for G_c \ T_c within G_c.
 * lead is what the reference loses: its np.delete calls take a two-column index array, so next to the true positives the first
 * t_c entries of the predicted (ground-truth) list leave its false positives (negatives), wrong or not.
 *   DocBank:    TP_c = area[c][c], FP_c = sum_g area[g][c] - TP_c,  FN_c = sum_p area[c][p] - TP_c;
 *   reference:  FP_c - lead_out[c], FN_c - lead_out[C + c].
 * The call writes every entry of the three outputs (n_nodes == 0: zeros) and does not need them zeroed.  One memset and at most
 * three launches on `stream`: a tally of chunks of gte_doc_eval_chunk_nodes() nodes (LDS integer atomics, one flush of 64-bit
 * global atomics per workgroup), a one-workgroup scan of the chunks' class counts, and the lead pass (ranks from wave ballots and
 * the scan's prefix).  Integer sums only: deterministic.  No allocation, no synchronisation, no workgroup waits on another.
 * workspace: gte_doc_eval_workspace_bytes(n_nodes, n_classes) bytes (-1 for sizes the call refuses), 8-byte aligned.
 * A null or misaligned pointer, n_nodes < 0 or n_classes < 1 return GTE_ERR_INVALID_ARGUMENT; n_classes above the limit or
 * n_nodes > 2^31 - 1 GTE_ERR_UNSUPPORTED; a short workspace GTE_ERR_WORKSPACE_TOO_SMALL: nothing is launched or written then. */
int gte_doc_eval_max_classes(void);     /* 16 */
int gte_doc_eval_chunk_nodes(void);     /* 2048 */
int64_t gte_doc_eval_workspace_bytes(int64_t n_nodes, int n_classes);
int gte_doc_eval(const int32_t* gt, const int32_t* pred, const int32_t* bbox, int64_t n_nodes, int n_classes, int64_t* area_out,
                 int64_t* count_out, int64_t* lead_out, void* workspace, int64_t workspace_bytes, void* stream);

/* The whole batch in ONE launch (what the train loop calls every step; gte_batch_csr / gte_batch_rows are its pieces):
 * a page's rows are CONTIGUOUS in the resident arrays and in the batch, so every array of the batch is the concatenation
 * of per-page runs -- features and labels copied, indptr / indices copied with a per-page constant added.
 * Workgroups: the batch's feature rows are split EVENLY, rows_per_wg = max(1, 32 KB / row bytes) consecutive batch rows per
 * workgroup whatever the page sizes (a workgroup may cover many small pages, a large page many workgroups; one binary search
 * over b_node_off per workgroup finds the first page it overlaps).  Behind them come 7 workgroups per chosen page, one small run
 * each: the labels (and the row map of gte_batch_assemble_rows), and per direction indptr / indices / weights.  The last chosen
 * page's indptr run is one entry longer (indptr_out[n_out] = e_out).  Runs move with 16-byte stores aligned on the destination
 * (single dwords in front and behind; sources need only 4-byte alignment); no per-element search, no allocation, no
 * synchronisation.  HBM-bound: 2 * n_out * n_cols * 4 bytes dominate.
 * `in_edges` / `out_edges`: the two CSR directions; either may be NULL (nothing of that direction is written); in a given one
 * edge_off, indptr_loc, b_edge_off and indptr_out are required.  weight_out NULL: no weights are written; weight_out set and
 * weight NULL (an unweighted set): weight_out is filled with 1.0f.  label / label_out: both or neither.  feat_out has leading
 * dimension n_cols (packed), and so must feat (ld_feat == n_cols, else GTE_ERR_UNSUPPORTED).  1 <= n_batch <= 65535.
 * n_out == 0 (every chosen page is empty) is a launch like any other: it writes indptr_out[0] = 0 in every given direction (and
 * the padding entries of a row map) and nothing else.  A chosen page may be empty, and may be chosen more than once. */
typedef struct gte_batch_arrays {
    const int32_t* edge_off;      /* [P+1]  resident: first CSR entry of every page                                  */
    const int32_t* indptr_loc;    /* packed per-page indptr (see gte_batch_csr)                                        */
    const int32_t* indices_loc;   /* page-local column ids                                                             */
    const float* weight;          /* CSR-ordered weights or NULL                                                       */
    const int32_t* b_edge_off;    /* [n_batch+1] batch: first entry of every chosen page                               */
    int32_t* indptr_out;          /* [n_out+1]                                                                         */
    int32_t* indices_out;         /* [e_out]                                                                           */
    float* weight_out;            /* [e_out] or NULL                                                                   */
} gte_batch_arrays;
int gte_batch_assemble(const int32_t* pages, int64_t n_batch, const int32_t* node_off, const int32_t* b_node_off,
                       const gte_batch_arrays* in_edges, const gte_batch_arrays* out_edges,
                       const float* feat, int64_t ld_feat, int64_t n_cols, float* feat_out,
                       const float* label, float* label_out, int64_t n_out, void* stream);
/* 1: a gte_batch_assemble / gte_batch_assemble_rows call made while a fold deferral is open on its stream (i.e. from inside a
 * training step: gte_gcnsage_step's before-last-GEMM callback) is not launched; the deferral's flush -- the fold + optimiser launch
 * that ends the step -- carries it as extra workgroups (the NEXT batch's buffers are independent of everything that launch
 * touches).  One job per deferral; without an open deferral on that stream the call launches as always.  0 (default): off.
 * Per host thread; returns the previous setting. */
int gte_batch_assemble_defer(int on);
/* out[b_node_off[i] + r, 0:n_cols] = in[node_off[pages[i]] + r, 0:n_cols]  (features, labels stored as f32) */
int gte_batch_rows(const int32_t* pages, int64_t n_batch, const int32_t* node_off, const int32_t* b_node_off,
                   const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t n_out, int64_t n_cols,
                   void* stream);
/* Edge weights of loader.py:332-344: w_e = 1 - d_e / max_{e in the page} d_e with d = the reference's integer box
 * distance (graphs/utils.py:56-88).  bbox int32[N,4] (x0,y0,x1,y1; 16-byte aligned), graph_of_node int32[N].
 * A page whose distances are all 0 gets weight 1 (the reference divides by zero there).  Bit-exact vs the
 * double-precision host formula. */
int64_t gte_edge_weights_workspace_bytes(int64_t n_edges, int64_t n_graphs);
int gte_edge_weights_bbox(const int32_t* bbox, const int32_t* src, const int32_t* dst, const int32_t* graph_of_node,
                          int64_t n_edges, int64_t n_graphs, float* weight, void* workspace, int64_t workspace_bytes,
                          void* stream);
/* BBOX node features (replaces nlp/bbox.py:49-124 called at model_train.py:293): per word
 * out[i, 0:13] = [w, h, cx, cy, w*h, x0, y0, x1, y1, hist_letters, hist_digits, hist_others, hist_empty].
 * bbox int32[N,4]; char_counts int32[N,3] = (#letters, #digits, #other characters) of the word, counted on the host;
 * float64 arithmetic as the reference, stored as float32.  Bit-exact vs the host formula. */
int gte_bbox_features(const int32_t* bbox, const int32_t* char_counts, float* out, int64_t ldo, int64_t n_nodes,
                      void* stream);
/* REPR node features (replaces Repr.get_similarity and the per-page loop of Repr.__call__, nlp/repr.py:75-87, 111-139, called at
 * model_train.py:293).  node_tok int32 [n_nodes]: the id of every word's normalised token, -1 for a node without one;
 * embeddings double [n_vocab, dim]; centers double [n_centroids, dim]; i_proto double [n_centroids, n_out]; all packed.
 * For a word with token row e, all in float64:
 *   d_c = sqrt(sum_k (e_k - c_k)^2)   k = 0 .. dim-1 in that order, product and sum rounded separately
 *   t_c = max(d_c, 1e-4);  w_c = pow(1 / t_c, alpha)  (alpha == 1: 1 / t_c as it stands);  s = sum_c w_c in the order c = 0 .. C-1;
 *   q_c = w_c / s.
 * combined == 0: out[i, 0:n_out] = (float)i_proto[c*, :] with c* the FIRST index at which q is largest -- every centre closer
 *   than 1e-4 ties, and the lowest index of them wins even where a later centre matches exactly, as in the reference.
 * combined == 1: out[i, j] = sum_c (float)q_c * (float)i_proto[c, j], float32 FMAs in the order c = 0 .. C-1.
 * node_tok[i] == -1 -- or any id outside [0, n_vocab): the kernel reads no row it was not given -- writes a row of zeros.  Only the
 * columns [0, n_out) of a row are written; row i starts at out + i * ldo, ldo >= n_out (a column slice of a wider feature matrix).
 * One launch, one wave per word, centre c on lane c, the centres staged through LDS; no allocation, no workspace, no
 * synchronisation.  Invalid arguments (null or misaligned pointers, negative sizes, dim / n_centroids / n_out < 1, ldo < n_out, a
 * non-finite alpha, combined outside {0, 1}) return GTE_ERR_INVALID_ARGUMENT; above gte_repr_max_centroids() / _max_dim() /
 * _max_out() the call returns GTE_ERR_UNSUPPORTED before any launch; n_nodes == 0 is GTE_OK with nothing launched.
 * Limitation: the reference's torch.sum / torch.norm orders are not defined; a word whose two best clamped distances differ by less
 * than about 1e-12 relative may be assigned differently there. */
int gte_repr_max_centroids(void);   /* 64 */
int gte_repr_max_dim(void);         /* 1024 */
int gte_repr_max_out(void);         /* 1024 */
int gte_repr_features(const int32_t* node_tok, int64_t n_nodes, const double* embeddings, int64_t n_vocab, int dim,
                      const double* centers, const double* i_proto, int n_centroids, int n_out, double alpha,
                      int combined, float* out, int64_t ldo, void* stream);
/* Token pooling, the arithmetic of the SCIBERT embedder (replaces the embedding lookup and mean_pooling / max_pooling of
 * SciBERT.list_of_sentence, nlp/scibert.py:53-65, 143-160, called per page at model_train.py:293).  tok int32 [n_words, width],
 * packed: the ids of a word's pieces in position order; table float [n_vocab, dim], packed (for SCIBERT: the row-normalised input
 * embeddings).  An entry of tok TAKES PART if 0 <= id < n_vocab; anything else (the -1 of a masked position, an id that names no
 * row) is skipped and is never used as an address.  With c the number of entries of word i that take part, per column j:
 *   mode 0 (mean): s = 0.0f; s = s + table[id, j] for the entries that take part, in position order, every add rounded to float32;
 *                  out = s / (float)c, a correctly rounded division; c == 0 gives 0.0f.
 *   mode 1 (max):  m = 0.0f; m = x > m ? x : m with x = table[id, j], in position order: max(0, the entries); a NaN is passed over.
 * row_map int64 [n_words], or NULL for the identity: row_map[i] is the destination row of word i, negative if the word is dropped
 * (nothing is read or written for it).  The call writes exactly out[r * ldo .. r * ldo + dim) of the named rows r and nothing else:
 * out may be a column slice of the final feature matrix that holds the kept nodes only.  The caller guarantees that the named rows
 * exist and are distinct.  out and ldo need 4-byte alignment only (column 63 of an 831-float row): where table, out, ldo and dim
 * are all 16-byte friendly (gte_token_pool_access_bytes == 16) a lane takes four columns with 16-byte accesses, otherwise one with
 * dword accesses; both forms perform the same operations per element and give the same bits.
 * One launch, one wave per word, grid-stride over words, the ids wave-uniform, up to 16 row reads in flight per column chunk; no
 * atomics, no LDS, no workspace, no synchronisation.  Invalid arguments (negative sizes, width or dim < 1, n_vocab above INT32_MAX,
 * ldo < dim, mode outside {0, 1}, null or misaligned pointers) return GTE_ERR_INVALID_ARGUMENT; above gte_token_pool_max_width() /
 * _max_dim() the call returns GTE_ERR_UNSUPPORTED; both before any launch.  n_words == 0 is GTE_OK with nothing launched. */
int gte_token_pool_max_width(void);   /* 32 */
int gte_token_pool_max_dim(void);     /* 4096 */
int gte_token_pool_access_bytes(const float* table, int dim, const float* out, int64_t ldo);   /* 16 or 4; host arithmetic only */
int gte_token_pool_f32(const int32_t* tok, int64_t n_words, int width, const float* table, int64_t n_vocab, int dim, int mode,
                       const int64_t* row_map, float* out, int64_t ldo, void* stream);
/* All-pairs weighted Levenshtein distance (replaces the double loop of LevenshteinSimilitudes.calculate_similarity,
 * tables/levenshtein.py:50-63, called by Preprocessor.train_repr, tables/preprocessor.py:303-305): n_src * n_dst independent
 * dynamic programmes in one launch.  Words are concatenated COMPACT character ids (uint16, 0 <= id < n_alpha) with n + 1 int32
 * offsets: word p is chars[off[p] .. off[p+1]).  ins_cost, del_cost double [n_alpha]; sub_cost double [n_alpha, n_alpha], row-major:
 * sub_cost[x * n_alpha + y] is the cost of replacing x (of the src word) by y (of the dst word).
 * out[p * ldo + q] = lev(src[p] -> dst[q]) = d[|a|][|b|] for a = src[p], b = dst[q], all in float64, by exactly this recurrence
 * (that of the weighted_levenshtein library the reference calls):
 *   d[0][0] = 0
 *   d[i][0] = d[i-1][0] + del[a[i-1]]
 *   d[0][j] = d[0][j-1] + ins[b[j-1]]
 *   d[i][j] = d[i-1][j-1]                                   if a[i-1] == b[j-1]   (a copy: NO minimum is taken)
 *           = min(d[i-1][j]   + del[a[i-1]],
 *                 d[i][j-1]   + ins[b[j-1]],
 *                 d[i-1][j-1] + sub[a[i-1]][b[j-1]])        otherwise
 * Every cell is one of three correctly rounded sums or a copy, so the result does not depend on the order the cells are visited
 * in and equals a host evaluation of the recurrence bit for bit.  The equal-characters rule is NOT "substitution cost 0": with
 * insert + delete cheaper than the detour, the two differ.
 * Only out[p * ldo + q] for p < n_src, q < n_dst is written (ldo >= n_dst: a column slice of a wider matrix stays untouched).
 * One launch, one wave per workgroup, one dst word per lane, the rolling column in LDS; no atomics, no workspace, no allocation.
 * The kernel clamps every word's start into [0, off[n]], its length to max_len and to what off[n] leaves, and a character id to
 * n_alpha - 1: given truthful off[n] and table sizes, no offsets or ids can take a read outside the buffers (a clamped word gives
 * the distance of the clamped word).  A character buffer may be NULL when its list holds only empty words.
 * Negative sizes (n_src, n_dst, max_len), ldo < n_dst, null or misaligned pointers return GTE_ERR_INVALID_ARGUMENT; max_len >
 * gte_lev_max_len() or n_alpha outside 1 .. gte_lev_max_alphabet() GTE_ERR_UNSUPPORTED; n_src == 0 or n_dst == 0 is GTE_OK with
 * nothing launched.  All of these come before any launch, in this order: sizes and ldo, limits, the empty call, pointers. */
int gte_lev_max_len(void);        /* 64 characters per word */
int gte_lev_max_alphabet(void);   /* 1024 distinct characters */
int gte_lev_matrix_f64(const uint16_t* src_chars, const int32_t* src_off, int64_t n_src,
                       const uint16_t* dst_chars, const int32_t* dst_off, int64_t n_dst, int max_len,
                       const double* ins_cost, const double* del_cost, const double* sub_cost, int n_alpha,
                       double* out, int64_t ldo, void* stream);
/* Affinity propagation sweeps (the loop of sklearn/cluster/_affinity_propagation.py: _affinity_propagation, which
 * Preprocessor.train_repr runs through src/utils/matrixes.py: affinity) on row-major float64 S, A, R [n, n].  S carries the
 * preference on its diagonal and the degeneracy noise: both are host work (components/tables/affinity.py: prepare).
 * d = damping, omd = one_minus_damping: the host computes 1 - damping in float64 and passes it in.  Every product, sum and
 * difference below is one correctly rounded float64 operation; nothing is contracted into a fused multiply-add.  Sweep `it`:
 *   row pass, row i:   t[k] = A[i,k] + S[i,k];  I = the FIRST index of the maximum of t (ties go to the lowest k, as np.argmax);
 *                      Y = t[I];  Y2 = max over k != I of t[k] (-inf for n == 1);
 *                      new[k] = S[i,k] - Y for k != I, new[I] = S[i,I] - Y2;   R[i,k] = (R[i,k] * d) + (new[k] * omd)
 *   Rp:                Rp[i,k] = max(R[i,k], 0) for k != i, Rp[i,i] = R[i,i]
 *   column sums:       cs[k] = (((Rp[0,k] + Rp[1,k]) + Rp[2,k]) + ...) + Rp[n-1,k], STRICTLY in row order: what np.sum(axis=0) does
 *                      on a C-contiguous matrix.  The order is part of the contract; a tree or a split over row blocks is a
 *                      different function.
 *   A update:          u = Rp[i,k] - cs[k];  off the diagonal u = max(u, 0), the diagonal keeps u;   A[i,k] = (A[i,k] * d) - (u * omd)
 *   exemplars, stop:   E[i] = (A[i,i] + R[i,i]) > 0 from the new A and R, written to exemplar[i] and to slot it % convergence_iter of a
 *                      ring of the last convergence_iter vectors E;  K = sum(E).  If it >= convergence_iter, every node's ring
 *                      is all ones or all zeros, and K > 0: stop after this sweep with converged = 1, n_iter = it + 1.  If
 *                      max_iter sweeps pass without that: stop with converged = 0, n_iter = max_iter (scikit-learn's
 *                      never_converged).
 * Equality with the host evaluation is equality by value (==); the sign of a zero is not pinned.
 * state int32 [4] in device memory = {n_iter_done, stopped, converged, K of the last sweep}.  The call ENQUEUES n_sweeps sweeps on
 * `stream` and continues from `state`; it neither allocates nor synchronises.  The stop is decided on the device: every kernel of a
 * sweep reads the state first and returns without touching A, R, exemplar or the ring when `stopped` is set or n_iter_done ==
 * max_iter, so the matrices are frozen after the stopping sweep however many sweeps were enqueued behind it, and how the caller
 * cuts max_iter into calls changes no output bit.  Before the first call the caller zeroes A, R, the workspace (column sums,
 * ring and flags, gte_affprop_workspace_bytes(n, convergence_iter) bytes) and state.
 * One sweep is four launches: the row pass (a workgroup per row, any n); the column sums (a lane per column adds in row order
 * while a workgroup stages tiles of rows through LDS to keep loads in flight; Rp is formed on the fly, never stored in memory);
 * the elementwise A update, whose diagonal lanes also write E, the ring slot and a "ring is uniform" flag per node; and one
 * workgroup that counts K and the uniform nodes (integers: deterministic) and writes the state.  64-bit indexing throughout.
 * Checks, all before any launch, in this order: n < 0, convergence_iter < 1, max_iter < 1, n_sweeps < 0, damping or
 * one_minus_damping outside [0, 1] GTE_ERR_INVALID_ARGUMENT; n > gte_affprop_max_n() or convergence_iter >
 * gte_affprop_max_convergence_iter() GTE_ERR_UNSUPPORTED; n == 0 or n_sweeps == 0 GTE_OK with nothing launched; null or misaligned
 * pointers GTE_ERR_INVALID_ARGUMENT; a workspace below the size query GTE_ERR_WORKSPACE_TOO_SMALL. */
int gte_affprop_max_n(void);                  /* 8192 */
int gte_affprop_max_convergence_iter(void);   /* 256 */
int64_t gte_affprop_workspace_bytes(int64_t n, int convergence_iter);
int gte_affprop_iterate(const double* S, double* A, double* R, int64_t n, double damping, double one_minus_damping,
                        int convergence_iter, int max_iter, int n_sweeps, uint8_t* exemplar /* [n] */, void* workspace,
                        int64_t workspace_bytes, int32_t* state /* [4] */, void* stream);
/* Exact t-SNE on a precomputed distance matrix (csrc/tsne.hip): the numerical stages of scikit-learn 1.7.2's TSNE(method='exact',
 * metric='precomputed') -- sklearn/manifold/_utils.pyx: _binary_search_perplexity, _t_sne.py: _joint_probabilities, _kl_divergence,
 * _gradient_descent, _tsne -- which Preprocessor.train_repr runs on the host.  Checks, the squaring of the distances, the float32
 * cast and the initial embedding are host work (components/tables/tsne.py: prepare).  All matrices row-major; eps =
 * np.finfo(np.double).eps = 2^-52.  The order of every sum is free but fixed (csrc/tsne.hip states it): two runs give the same bits,
 * no floating-point atomics.  Every product, sum and quotient is one rounded float64 operation, nothing is contracted.
 *
 * gte_tsne_cond_p -- conditional probabilities.  sq_dist float32 [n, n] (scikit-learn casts the squared distances to float32 ahead
 * of the search), perplexity float32.  Row i: beta = 1, beta_min = -inf, beta_max = +inf; at most 100 steps of
 *     p_j = exp(-(double)d_ij * beta) for j != i, p_i = 0;   s = sum_j p_j, s = (double)1e-8f if the sum is 0;   p_j = p_j / s;
 *     H = log(s) + beta * sum_j (double)d_ij * p_j;   diff = H - log((double)perplexity);
 *     |diff| <= (double)1e-5f: leave the loop (beta unchanged);
 *     diff > 0:  beta_min = beta;  beta = beta_max == +inf ? beta * 2 : (beta + beta_max) / 2
 *     else:      beta_max = beta;  beta = beta_min == -inf ? beta / 2 : (beta + beta_min) / 2
 * cond_p[i, :] = the p of the last step that ran, beta[i] = beta as the loop leaves it (after 100 steps without a hit: the value the
 * 101st step would have used, as the .pyx leaves its variable).
 *
 * gte_tsne_joint_p -- P = (C + C^T) / max(sum_ij (C_ij + C_ji), eps); off the diagonal P_ij = max(P_ij, eps); P_ii = 0.  P is the
 * full symmetric float64 [n, n] (scikit-learn's condensed vector is an implementation detail).
 *
 * gte_tsne_iterate -- ENQUEUES n_iters iterations of _gradient_descent on _kl_divergence and continues from `state`; it neither
 * allocates nor synchronises.  d = n_components, alpha = max(d - 1, 1), e = exaggeration.  Iteration `it`, from the current
 * embedding y (Y holds TWO [n, d] buffers; state names the current one):
 *     dist_ij = ((y_i0 - y_j0)^2 + (y_i1 - y_j1)^2) + ...  in component order;   num_ij = (1 + dist_ij / alpha)^(-(alpha + 1) / 2), i != j
 *     Z = sum_{i != j} num_ij;   Q_ij = max(num_ij / Z, eps)
 *     grad_ic = (2 (alpha + 1) / alpha) * sum_j (e * P_ij - Q_ij) * num_ij * (y_ic - y_jc)
 *     KL = sum_{i != j} e * P_ij * log(max(e * P_ij, eps) / Q_ij)         only when (it + 1) % 50 == 0 or it == max_iter - 1
 *   update, per component:
 *     gains = (update * grad < 0) ? gains + 0.2 : gains * 0.8;   gains = max(gains, 0.01);   g = grad * gains;
 *     update = (momentum * update) - (learning_rate * g);   y_new = y + update   (written to the OTHER buffer, which becomes current)
 *   check, when (it + 1) % 50 == 0, with error = KL and grad_norm = ||g||_2 over all n * d components:
 *     error < best_error: best_error = error, best_iter = it;   else if it - best_iter > n_iter_without_progress: stop (reason 1);
 *     then, unless stopped: grad_norm <= min_grad_norm: stop (reason 2).
 * The power is an integer or a half-integer: it is evaluated with products, one sqrt and one division (a few ulp), never pow.
 * state float64 [8] in device memory, integers held exactly: {it = the next iteration, stopped, reason, best_iter, current buffer
 * (0 / 1), error = the last KL computed, best_error, grad_norm of the last check}.  Every kernel of an iteration reads it first and
 * returns without a write when `stopped` is set or it >= max_iter, so iterations enqueued behind the stop change nothing and how
 * the caller cuts a phase into calls changes no bit.  One call is one PHASE of scikit-learn's _tsne, which the caller sets up as
 * two calls of _gradient_descent do: update = 0, gains = 1, state = {first iteration, 0, 0, first iteration, current buffer,
 * DBL_MAX, DBL_MAX, 0}.  Phase 1: iterations 0 .. 249, momentum 0.5, e = early_exaggeration, n_iter_without_progress = 250;
 * phase 2: from the iteration after phase 1's last one to max_iter, momentum 0.8, e = 1.  n_iter = it - 1 = the last iteration run.
 * Deliberate deviations from scikit-learn: (1) y, update and gains are float64 throughout (there the float32 random init makes the
 * parameters float32 while, under numpy 2, the np.float64 learning rate makes `update` float64); (2) e * P is formed on the fly
 * (there P is scaled in place and scaled back); (3) the results are deterministic.
 * One iteration is three launches: partial sums of Z per block of rows; the gradient pass (a workgroup owns a block of rows, adds
 * the Z partials in a fixed order, walks the columns in tiles, reduces per row and updates its own rows; on check iterations it
 * leaves partial sums of KL and ||g||^2); one workgroup that finishes those sums, applies the stop rule and advances the state.
 * The workspace starts with the ceil(n / 16) float64 partial sums of Z, followed by Z itself as the last iteration used it.
 * Checks, all before any launch, in this order: negative sizes (n, max_iter, n_iters), n_components < 1, a perplexity that is not
 * positive and finite GTE_ERR_INVALID_ARGUMENT; n > gte_tsne_max_n() or n_components > gte_tsne_max_components()
 * GTE_ERR_UNSUPPORTED; n == 0 (or n_iters == 0) GTE_OK with nothing launched; null or misaligned pointers
 * GTE_ERR_INVALID_ARGUMENT; a workspace below gte_tsne_workspace_bytes(n) (joint_p and iterate) GTE_ERR_WORKSPACE_TOO_SMALL.
 * That 2 <= n and perplexity < n is the host's to check: the kernels take n = 1 (an empty sum) without a fault. */
int gte_tsne_max_n(void);            /* 8192 */
int gte_tsne_max_components(void);   /* 8 */
int64_t gte_tsne_workspace_bytes(int64_t n);
int gte_tsne_cond_p(const float* sq_dist, int64_t n, float perplexity, double* cond_p /* [n, n] */, double* beta /* [n] */, void* stream);
int gte_tsne_joint_p(const double* cond_p, int64_t n, double* P /* [n, n] */, void* workspace, int64_t workspace_bytes, void* stream);
int gte_tsne_iterate(const double* P, double* Y /* [2, n, n_components] */, double* update, double* gains, int64_t n, int n_components,
                     double learning_rate, double momentum, double exaggeration, int n_iter_without_progress, double min_grad_norm,
                     int max_iter, int n_iters, void* workspace, int64_t workspace_bytes, double* state /* [8] */, void* stream);
/* EM for a one-dimensional Gaussian mixture (csrc/gmm.hip): the loop body of scikit-learn 1.7.2's BaseMixture.fit_predict with
 * covariance_type='full' and ONE feature (sklearn/mixture/_base.py, _gaussian_mixture.py), which Preprocessor.train_gmm of the
 * reference runs on the host through GaussianMixture ("soft") or its HardEMGaussianMixture ("hard").  For one feature every matrix is
 * a scalar.  Checks and the initial parameters are host work (components/tables/gmm.py: prepare).  eps = DBL_EPSILON = 2^-52.
 * x float64 [n], the samples.  P float64 [4, K] row-major = (weights w, means mu, covariances cov, precisions_cholesky pc), read and
 * rewritten by every iteration.  Every product, sum, difference and quotient below is one rounded float64 operation, nothing is
 * contracted into a fused multiply-add; exp, log and sqrt are the device library's (exp and log within 1 - 2 ulp).
 *
 * One iteration, from the current P:
 *   E step      y = x_i * pc_k - mu_k * pc_k;   wlp[i,k] = ((-0.5 * (log(2 pi) + y * y)) + log(pc_k)) + log(w_k)
 *               m_i = max_k wlp[i,k], 0 if that is not finite;   lse_i = log(sum_k exp(wlp[i,k] - m_i)) + m_i, the sum in k order
 *               (scipy's logsumexp up to that order);   log_resp[i,k] = wlp[i,k] - lse_i
 *               soft: resp[i,k] = exp(log_resp[i,k]).   hard: resp[i,:] = the one-hot of the FIRST index of the maximum of the rounded
 *               log_resp[i,:] -- not of wlp: the subtraction can create ties, and np.argmax takes the first.
 *   M step      nk_k = sum_i resp[i,k] + 10 eps;   mean_k = (sum_i resp[i,k] * x_i) / nk_k
 *               cov_k = (sum_i (resp[i,k] * (x_i - mean_k)) * (x_i - mean_k)) / nk_k + reg_covar: two passes, around the NEW mean, as
 *               scikit-learn's _estimate_gaussian_covariances_full; never sum r x^2 - nk mean^2 (numerals reach 1e6 with tiny spreads)
 *               pc_k = 1 / sqrt(cov_k);   soft: w_k = nk_k / (nk_0 + nk_1 + ... in k order);   hard: w_k = nk_k / n
 *   bound, stop lb = (sum_i lse_i) / n, the E step's, for both types;   change = lb - prev, prev = the lb of the iteration before,
 *               -inf ahead of the first.   |change| < tol: converged = 1, stopped = 1; the M step of that iteration is kept.
 *   error       a cov_k that is not finite or not > 0: error = 1, stopped = 1 (scikit-learn raises "ill-defined empirical covariance").
 * Sums over the samples: the order is free but fixed, a function of n alone -- never of the device -- and csrc/gmm.hip states it with
 * its longest chain L(n) = 23 + ceil(ceil(n / gte_gmm_workgroup_samples()) / 64): a lane adds its own samples in index order, a wave
 * butterfly and then the waves in order merge the workgroup, per-workgroup partials go to the workspace, ONE finalising workgroup adds
 * them (lane l the workgroups l, l + 64, ... in that order, then a butterfly).  No floating-point atomics: two runs give the same bits.
 * Two passes over x per iteration, a finalising launch behind each: pass A (E step; partials of nk, sum resp * x and sum lse; stores
 * lse[i] and, hard, label[i] in the workspace), finalise A (nk, means), pass B (resp[i,k] recomputed as exp(wlp[i,k] - lse_i) from the
 * stored lse and the still-old P, or read from label; partials of the covariance sums), finalise B (cov, pc, w into P; lb and the stop
 * into the state).  No [n, K] buffer exists.
 * state float64 [8] in device memory, integers held exactly: {iterations done, stopped, converged, error, lb, prev, change, reserved}.
 * Before the first call the caller sets it to {0, 0, 0, 0, -inf, -inf, 0, 0}.  gte_gmm_iterate ENQUEUES n_iters iterations on `stream`
 * and continues from `state`; it neither allocates nor synchronises.  Every kernel reads the state first and returns without a write
 * when `stopped` is set or max_iter iterations are done, so iterations enqueued behind the stop change nothing and how the caller
 * cuts max_iter into calls changes no bit.  The workspace (gte_gmm_workspace_bytes(n, K) bytes) needs no initialisation.
 *
 * gte_gmm_posterior -- the E step alone, by the same device function as pass A, for m points: resp float64 [m, K] = exp(wlp - lse)
 * (the soft responsibilities whatever the type of the fit), lse float64 [m] (score_samples), label int32 [m] = the first-index
 * arg-max of the rounded wlp - lse (predict).  Each output may be NULL, not all three.
 *
 * Limits: 1 <= K <= gte_gmm_max_components() = 64, 1 <= n < 2^31.  Checks, all before any launch: n (m) < 1, K outside 1 .. 64,
 * max_iter < 1, n_iters < 0, tol or reg_covar negative or NaN GTE_ERR_INVALID_ARGUMENT; n >= 2^31 GTE_ERR_UNSUPPORTED; null or
 * misaligned pointers GTE_ERR_INVALID_ARGUMENT; a workspace below the size query GTE_ERR_WORKSPACE_TOO_SMALL; n_iters == 0 GTE_OK with
 * nothing launched.  gte_gmm_workspace_bytes returns 0 for sizes outside the limits. */
int gte_gmm_max_components(void);      /* 64 */
int gte_gmm_workgroup_samples(void);   /* 2048: the samples one workgroup adds; ceil(n / this) partials per sum */
int64_t gte_gmm_workspace_bytes(int64_t n, int K);
int gte_gmm_iterate(const double* x, int64_t n, int K, double* P /* [4, K] */, int hard, double tol, double reg_covar, int max_iter,
                    int n_iters, void* workspace, int64_t workspace_bytes, double* state /* [8] */, void* stream);
int gte_gmm_posterior(const double* x, int64_t m, int K, const double* P /* [4, K] */, double* resp /* [m, K] or NULL */,
                      double* lse /* [m] or NULL */, int32_t* label /* [m] or NULL */, void* stream);
/* The per-word head of label-free prediction (model_predict.predict): class, confidence and, on request, the softmax row of every
 * node in ONE pass over logits float [n_nodes, n_classes] (row i at logits + i * ld_logits, ld_logits >= n_classes,
 * 1 <= n_classes <= 16: the step engine's class limit).  Per row, with l_j its entries:
 *   m    = the row's maximum; pred[i] = the FIRST index that holds it.  A NaN counts as greater than every number and the first NaN
 *          wins; infinities compare as numbers: what torch.argmax(logits, 1) returns on the CPU ([1, nan, 3, nan] -> 1, a row
 *          of -inf -> 0).
 *   in float64, in index order j = 0 .. C-1:  e_j = exp((double)l_j - (double)m);  S = e_0 + e_1 + ...;
 *   conf[i] = (float)(e_pred / S);  prob != NULL: prob[i * ld_prob + j] = (float)(e_j / S), ld_prob >= n_classes.
 * A row that holds NaN or +inf, or -inf only, yields NaN in conf and in its prob row (inf - inf; torch.softmax does the same).
 * Columns n_classes .. ld_logits-1 of logits are never read; nothing is written past row n_nodes-1 or past column n_classes-1 of
 * prob.  pred int64 [n_nodes], conf float [n_nodes], packed.  One launch, a lane per node, grid-stride (n_nodes is not bounded by
 * the grid); no atomics, no LDS, no workspace, no synchronisation: deterministic.  n_nodes == 0 is GTE_OK with nothing launched.
 * n_classes outside 1 .. 16, ld_logits < n_classes, prob != NULL with ld_prob < n_classes, n_nodes < 0, and with n_nodes > 0 a
 * NULL logits / pred / conf or a misaligned pointer return GTE_ERR_INVALID_ARGUMENT before any launch. */
int gte_predict_head(const float* logits, int64_t ld_logits, int64_t n_nodes, int n_classes, int64_t* pred, float* conf,
                     float* prob /* may be NULL */, int64_t ld_prob, void* stream);
/* inv_deg[v] = 1/(indptr[v+1]-indptr[v]) or 0  (models.py:74-78 as a standalone vector) */
int gte_inv_degree(const int32_t* indptr, float* inv_deg, int64_t n_nodes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A8  per-node transform: split-weight linear + bias + LayerNorm + ReLU, fp32 MFMA
 * replaces  models.py:69-72 (torch.cat((h, ah*norm),1)), :63 nn.Linear(2F,out), :64 nn.LayerNorm,
 *           :65-66 activation.
 *   z = a1[M,k1] * W[:, 0:k1]^T + a2[M,k2] * W[:, k1:k1+k2]^T + bias        (W: [n_out, k1+k2])
 *   y = relu?( LN?(z) ) ; LN over n_out with eps, affine (gamma, beta)
 * a2 may be NULL (k2 = 0; use_pp=True path, models.py:49).  gamma == NULL => no LayerNorm.
 * z_save (nullable): pre-LayerNorm z for the backward; stats (nullable): f32[2*M] = mean, rstd.
 * ---------------------------------------------------------------------------------------- */
int gte_sage_linear_fwd(const float* a1, int64_t lda1, int64_t k1,
                        const float* a2, int64_t lda2, int64_t k2,
                        const float* W, int64_t ldw, const float* bias,
                        const float* gamma, const float* beta, float eps, int relu,
                        float* z_save, int64_t ldz, float* stats,
                        float* y, int64_t ldy, int64_t M, int64_t n_out, void* stream);
/* 1 when gte_sage_linear_fwd runs this shape as ONE pass (linear + LayerNorm + ReLU: k1 + k2 <= 64, n_out % 4 == 0,
 * n_out <= 256 -- the BBOX-only input layer, F0 = 13), 0 when it is an MFMA GEMM followed by the LayerNorm launch. */
int gte_sage_linear_fwd_fuses_ln(int64_t k_total, int64_t n_out);

/* Weight gradient of the split-weight linear, both halves in ONE launch:
 *   dW[n_out, k1+k2] = dZ[M, n_out]^T * [x1[M,k1] | x2[M,k2]]        (autograd of models.py:63 w.r.t. the weight)
 * The reduction runs over the M nodes (split over workgroups, deterministic slab reduction).  x2 may be
 * NULL (k2 = 0).  workspace: gte_sage_linear_dw_workspace_bytes(n_out, k1, k2, M). */
int64_t gte_sage_linear_dw_workspace_bytes(int64_t n_out, int64_t k1, int64_t k2, int64_t n_nodes);
int gte_sage_linear_dw(const float* dz, int64_t lddz, const float* x1, int64_t ldx1, int64_t k1,
                       const float* x2, int64_t ldx2, int64_t k2, float* dW, int64_t lddw,
                       int64_t n_out, int64_t n_nodes, void* workspace, int64_t workspace_bytes, void* stream);

/* gte_spmm_csr_accumulate with a LayerNorm(+ReLU) epilogue, for a layer in transform-then-aggregate order
 * (models.py:53-54 then :64-66): z[v,:] += scale_v * sum_e w[e] x[src,:] (z written back: the LayerNorm backward
 * needs it), then y[v,:] = relu?(gamma * (z - mean) / sqrt(var + eps) + beta) and stats[v] = mean,
 * stats[n_rows + v] = rstd (nullable) -- same statistics as gte_ln_relu_fwd.  f32 only, n_feat <= 1024 (a row lives in
 * the registers of one lane group; gte_spmm_csr_accumulate_ln_supported says so).  The kernel works on 16-byte chunks:
 * when n_feat % 4 != 0 (% 16 != 0 with a P3 image of y) the rows of x, z and y must be PADDED -- allocated to the next
 * multiple of 4 (16) floats, ld >= that; the padding of x is read and must hold zeros, the padding of z / y / the image is
 * written as zeros; mean and variance run over the n_feat true columns (models.py:64). */
int gte_spmm_csr_accumulate_ln_supported(int64_t n_feat);
int gte_spmm_csr_accumulate_ln(const int32_t* indptr, const int32_t* indices, const float* eweight, const float* x,
                               int64_t ldx, float* z, int64_t ldz, int64_t n_rows, int64_t n_feat, int reduce,
                               const float* gamma, const float* beta, float eps, int relu, float* y, int64_t ldy,
                               float* stats, void* stream);

/* ---- GEMM tail split ----------------------------------------------------------------------------------------------
 * A whole-K GEMM launch (gte_sage_linear_fwd, gte_sage_transform_fwd, gte_sage_qform_dx, gte_gemm_f32 without split-K)
 * whose last round of tiles would leave more than half of the compute units idle cuts those tiles' reduction range into
 * pieces that fill the idle units, and finishes them with a small fix-up launch.  It needs scratch for the partial
 * tiles: gte_gemm_set_tail_workspace registers a caller-owned device buffer (>= gte_gemm_tail_workspace_bytes()) for the
 * calling host thread; NULL / 0 unregisters (launches then never split).  Launches that may split must not run
 * concurrently on two streams with one workspace.  Results are deterministic either way (fixed summation order), but a
 * split tile sums its K range in pieces: last-bit differences against the unsplit launch. */
int64_t gte_gemm_tail_workspace_bytes(void);
int gte_gemm_set_tail_workspace(void* workspace, int64_t workspace_bytes);

/* ---- GEMM arithmetic mode ------------------------------------------------------------------------------------------
 * How the fp32 transform GEMMs (every entry point of this section and gte_gemm_f32) multiply.  Process-wide.
 *   GTE_GEMM_F32        v_mfma_f32_32x32x2_f32: bit-exact fp32 FMA chains.
 *   GTE_GEMM_SPLIT_BF16 (default since round 3) every fp32 operand is cut exactly into three bf16 pieces (24 significand bits) in the kernel and the
 *                       product is six v_mfma_f32_32x32x16_bf16 partial products accumulated in fp32 (csrc/gemm_split.h):
 *                       fp32 in, fp32 out, error against fp64 not above the fp32 kernel's, 2.67x its matrix-pipe rate.
 *                       Tiles narrower than 128 columns and the small-shape path stay on the fp32 kernel.  Non-finite
 *                       operands give NaN where the fp32 kernel returns inf.
 * The environment variable GTE_GEMM_MODE=f32 selects the fp32 MFMA kernel before the first call; gte_gemm_set_mode overrides. */
#define GTE_GEMM_F32 0
#define GTE_GEMM_SPLIT_BF16 1
int gte_gemm_set_mode(int mode);
int gte_gemm_get_mode(void);
/* Override for the calling host thread only (-1: none, the process-wide mode applies): one caller's GEMMs in another mode
 * without touching what other threads get.  gte_gemm_get_mode reports the mode the calling thread would run in. */
int gte_gemm_set_thread_mode(int mode);

/* ---- planes GEMMs (P3 operands) --------------------------------------------------------------------------------------
 * The same transform GEMMs (models.py:63 nn.Linear and its autograd) on operands their PRODUCER has already cut into the
 * three bf16 planes of the split mode (csrc/p3.h): the GEMM then moves bf16 planes memory -> LDS (LDS-DMA) and spends its
 * issue slots on the six v_mfma_f32_32x32x16_bf16 products per fragment pair only.  Results are bit-identical to the split
 * mode on the fp32 operand (same pieces, same products, same order).
 * P3 image of a logical fp32 matrix [rows][cols]: row r at byte r * ldp (ldp >= gte_p3_row_bytes(cols), a multiple of 16; the
 * image 16-byte aligned); 16-feature block fb at + 96 fb; in a block plane h (16 bf16), plane m, plane l; x = h + m + l
 * exactly; features >= cols are zero.  "ldp*" arguments of this section are row strides in BYTES.
 * BLOCK-MAJOR images (round 6; the weights -- the B operand "b, ldb" of the gte_gemm_p3_nt* entry points -- and every gte_p3_desc /
 * gte_p3_from_f32 / gte_p3_to_f32 image): a NEGATIVE ldp names an image whose 16-feature block fb is ONE contiguous run at byte
 * fb * (-ldp), row r at + 96 r inside it (-ldp >= 96 rows, a multiple of 16).  A K block of the weights is then whole cache lines
 * (row-major: 96-byte runs at the row stride, every line fetched twice), and where a product has one column of 256-wide tiles the
 * block-major-weights kernel (csrc/gemm_p3.hip gemm_p3_nt_sq_kernel) loads its weight fragments straight into registers.  Same
 * products, same bits as the row-major image.  A operands, row-mapped resident images and the TN operands stay row-major. */
int64_t gte_p3_row_bytes(int64_t cols);
/* dst(r, c) = transpose ? src[c * ld + r] : src[r * ld + c]  for r < rows, c < cols (ld in elements) */
int gte_p3_from_f32(const float* src, int64_t ld, int64_t rows, int64_t cols, int transpose, void* dst, int64_t ldp,
                    void* stream);
int gte_p3_to_f32(const void* src, int64_t ldp, int64_t rows, int64_t cols, float* dst, int64_t ld, void* stream);
/* up to 16 of them in ONE launch (the weight images of every layer, after an optimiser step) */
typedef struct gte_p3_desc {
    const float* src; int64_t ld;      /* fp32 source, leading dimension in elements */
    int64_t rows, cols;                /* of the IMAGE: dst(r, c) = transpose ? src[c * ld + r] : src[r * ld + c] */
    int transpose;
    void* dst; int64_t ldp;            /* image (first byte of its row 0 / column block 0), row stride in bytes (< 0: block-major) */
} gte_p3_desc;
int gte_p3_from_f32_batch(const gte_p3_desc* descs, int n, void* stream);
/* Producers that write their result as a P3 image: the aggregation (q = A_w^T (norm dz), aggregated inputs; any n_feat, the
 * image's columns up to the next multiple of 16 are written as zeros), the fused aggregation + LayerNorm(+ReLU) (y as image
 * and / or fp32: either may be NULL) and the LayerNorm backward (dz as fp32 AND image: fp32 feeds the transpose aggregation,
 * the image the dX / dW GEMMs; widths other than 128 <= n_out <= 512 with n_out % 16 == 0 run a masked kernel on PADDED
 * rows: LayerNorm required, n_out <= 1024, lddy / ldz / lddz >= n_out rounded up to 4).  Same arithmetic as their fp32 forms
 * (gte_spmm_csr, gte_spmm_csr_accumulate_ln, gte_ln_relu_bwd); the image holds exactly the fp32 values. */
int gte_sage_linear_fwd_p3(const float* a1, int64_t lda1, int64_t k1, const float* a2, int64_t lda2, int64_t k2, const float* W,
                           int64_t ldw, const float* bias, const float* gamma, const float* beta, float eps, int relu,
                           float* z_save, int64_t ldz, float* stats, float* y /* nullable */, int64_t ldy, void* yp3,
                           int64_t ldyp3, int64_t M, int64_t n_out, void* stream);   /* one-pass form only (fuses_ln) */
/* Backward of the short-input layer (the layer gte_sage_linear_fwd runs in one pass: k1 + k2 <= 28 here) when it is the INPUT
 * layer (no dX): LayerNorm(+ReLU) backward and dW = dz^T [a1 | a2] in ONE pass over dy.  z is recomputed from the 26 inputs
 * per row with the forward kernel's instruction sequence (bit-identical: the forward need not save z -- pass z_save = NULL
 * there), dz never reaches memory.  Replaces gte_ln_relu_bwd + gte_sage_linear_dw (models.py:63-66 autograd).
 * dgamma / dbeta / dbias nullable.  The partial sums join an open fold deferral. */
int gte_sage_smallk_bwd_supported(int64_t k_total, int64_t n_out);
int64_t gte_sage_smallk_bwd_workspace_bytes(int64_t n_nodes, int64_t k_total, int64_t n_out);
int gte_sage_smallk_bwd(const float* dy, int64_t lddy, const float* a1, int64_t lda1, int64_t k1, const float* a2, int64_t lda2,
                        int64_t k2, const float* W, int64_t ldw, const float* bias, const float* gamma, const float* beta,
                        const float* stats, int relu, float* dW, int64_t lddw, float* dbias, float* dgamma, float* dbeta,
                        int64_t n_nodes, int64_t n_out, void* workspace, int64_t workspace_bytes, void* stream);
int gte_spmm_csr_p3(const int32_t* indptr, const int32_t* indices, const float* eweight, const float* x, int64_t ldx,
                    void* outp3, int64_t ldp, int64_t n_rows, int64_t n_feat, int reduce, void* stream);
int gte_spmm_csr_accumulate_ln_p3(const int32_t* indptr, const int32_t* indices, const float* eweight, const float* x,
                                  int64_t ldx, float* z, int64_t ldz, int64_t n_rows, int64_t n_feat, int reduce,
                                  const float* gamma, const float* beta, float eps, int relu, float* y, int64_t ldy,
                                  void* yp3, int64_t ldyp3, float* stats, void* stream);
int gte_ln_relu_bwd_p3(const float* dy, int64_t lddy, const float* z, int64_t ldz, const float* stats, const float* gamma,
                       const float* beta, int relu, float* dz, int64_t lddz, void* dzp3, int64_t ldp3, float* dgamma,
                       float* dbeta, float* dbias, int64_t M, int64_t n_out, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* c[m, n] (+)= [a1 | a2] b^T (+ bias on columns < bias_cols; <= 0: all), optional relu.  a1: P3 [m][k1]; a2: P3 [m][k2]
 * (NULL, k2 = 0: one K segment); b: P3 [n][...] whose rows hold the ceil(k1 / 16) blocks of segment 1 followed by the blocks
 * of segment 2.  replaces models.py:69-72 + :63 (forward; transform-first layers use b = [W_s ; W_n] as 2 out rows) and
 * the dX product of its backward (a1 = dz, a2 = q, b = [W_s^T | W_n^T]). */
int gte_gemm_p3_nt(const void* a1, int64_t ldpa1, int64_t k1, const void* a2, int64_t ldpa2, int64_t k2, const void* b,
                   int64_t ldpb, const float* bias, int64_t bias_cols, float* c, int64_t ldc, int64_t m, int64_t n, int relu,
                   int accumulate, void* stream);
/* c[m, n] = a^T b over k rows (dW = dZ^T X; split over the rows, partial slabs in `workspace`, folded in a fixed order --
 * inside an open fold deferral by gte_fold_defer_flush).  a: P3 [k][m], b: P3 [k][n].  nseg > 0: two column segments of
 * nseg columns (n == 2 nseg): c[:, 0:nseg] = a^T b, c[:, nseg:] = a2^T b2 (a2 / b2 NULL: the operand of segment 0). */
/* ... with A = the rows a_rows[0 .. m) of a RESIDENT image a_res [n_res_rows][k] (one K segment): the input layer's forward
 * transform straight from the resident features -- no per-batch copy of the rows (gte_batch_assemble_rows writes the map).
 * Images below 4 GB are read through 32-bit buffer offsets, larger ones through 64-bit per-lane addresses (same results). */
int gte_gemm_p3_nt_rows(const void* a_res, int64_t ldpa, int64_t k, const int32_t* a_rows, int64_t n_res_rows, const void* b,
                        int64_t ldpb, const float* bias, int64_t bias_cols, float* c, int64_t ldc, int64_t m, int64_t n,
                        int relu, int accumulate, void* stream);
/* ... with BOTH K segments resident: [A | A2] = the rows a_rows[0 .. m) of two resident images of n_res_rows rows and k columns
 * each -- the input features and their CACHED mean aggregate norm . A_w x (page-local and constant over a run: made once when the
 * pages are loaded).  The forward of models.py:69-72 `linear(cat(h, ah * norm))` for the input layer without any per-batch
 * operand preparation: no aggregation launch, no image conversion, no feature copy.  b = P3 [n][2 ceil16(k)], the W_n columns at
 * block ceil(k / 16).  Both images below 4 GB (32-bit row offsets). */
int gte_gemm_p3_nt_rows2(const void* a_res, int64_t ldpa, const void* a2_res, int64_t ldpa2, int64_t k, const int32_t* a_rows,
                         int64_t n_res_rows, const void* b, int64_t ldpb, const float* bias, int64_t bias_cols, float* c, int64_t ldc,
                         int64_t m, int64_t n, int relu, int accumulate, void* stream);
/* gte_gemm_p3_nt + gte_ln_relu_fwd_p3 in ONE launch (n <= 256: a workgroup's tile holds whole rows): z = [a1 | a2] b^T + bias is
 * written as fp32 (ldz >= n rounded up to 4: the operand of the layer's LayerNorm backward) and normalised by the workgroup that
 * computed it -- models.py:63-66 `linear`, `lynorm`, `activation` of an aggregate-first layer: stats = {mean [m], rstd [m]}, y =
 * relu?(LN(z)) as fp32 (nullable) and as a P3 image (nullable; columns up to the next multiple of 16 zero).  Bit-identical to the two
 * launches.  ..._rows2_...: [a1 | a2] = mapped rows of two resident images (gte_gemm_p3_nt_rows2). */
int gte_gemm_p3_nt_ln_fwd_supported(int64_t n);
int gte_gemm_p3_nt_ln_fwd(const void* a1, int64_t ldpa1, int64_t k1, const void* a2, int64_t ldpa2, int64_t k2, const void* b,
                          int64_t ldpb, const float* bias, const float* gamma, const float* beta, float eps, int relu, float* z,
                          int64_t ldz, float* y, int64_t ldy, void* yp3, int64_t ldyp3, float* stats, int64_t m, int64_t n,
                          void* stream);
int gte_gemm_p3_nt_rows2_ln_fwd(const void* a_res, int64_t ldpa, const void* a2_res, int64_t ldpa2, int64_t k, const int32_t* a_rows,
                                int64_t n_res_rows, const void* b, int64_t ldpb, const float* bias, const float* gamma,
                                const float* beta, float eps, int relu, float* z, int64_t ldz, float* y, int64_t ldy, void* yp3,
                                int64_t ldyp3, float* stats, int64_t m, int64_t n, void* stream);
/* gte_gemm_p3_nt (no bias / relu / accumulate) whose product dy [m][n], n <= 256, is NOT stored: the workgroup that computed a
 * block of rows runs the LayerNorm(+ReLU) backward of those rows on it (models.py:64-66 autograd of the layer below): dz as fp32
 * and as a P3 image (dzp3 nullable), column sums dgamma / dbeta / dbias (nullable) into the fold deferral.  z / stats / gamma /
 * beta as gte_ln_relu_bwd.  Replaces gte_gemm_p3_nt + gte_ln_relu_bwd_p3 (one launch, 2 m n 4 bytes of traffic less); dz is
 * bit-identical to theirs.  Any n in 1 .. 256; n % 4 != 0 needs the rows of z and dz padded to a multiple of 4 floats (ldz,
 * lddz >= that, padding of dz written as zeros), and whenever n % 16 != 0 the image's columns up to the next multiple of 16 are
 * written as zeros.  dz is nullable when dzp3 is given (a layer below whose weight gradient reads the image only). */
int gte_gemm_p3_nt_ln_bwd_supported(int64_t n);
int64_t gte_gemm_p3_nt_ln_bwd_workspace_bytes(int64_t m, int64_t n);
int gte_gemm_p3_nt_ln_bwd(const void* a1, int64_t ldpa1, int64_t k1, const void* a2, int64_t ldpa2, int64_t k2, const void* b,
                          int64_t ldpb, const float* z, int64_t ldz, const float* stats, const float* gamma, const float* beta,
                          int relu, float* dz, int64_t lddz, void* dzp3, int64_t ldp3, float* dgamma, float* dbeta, float* dbias,
                          int64_t m, int64_t n, void* workspace, int64_t workspace_bytes, void* stream);
/* ... with the WHOLE backward of a short-input INPUT layer below (gte_sage_smallk_bwd: k1 + k2 <= 28) as the epilogue: dy is not
 * stored, z is recomputed per row, dW / dbias / dgamma / dbeta of that layer come out through the fold deferral (outside a
 * deferral dW must be packed, lddw == k1 + k2).  Replaces gte_gemm_p3_nt + gte_sage_smallk_bwd. */
int gte_gemm_p3_nt_smallk_bwd_supported(int64_t k_total, int64_t n);
int64_t gte_gemm_p3_nt_smallk_bwd_workspace_bytes(int64_t m, int64_t k_total, int64_t n);
int gte_gemm_p3_nt_smallk_bwd(const void* a1, int64_t ldpa1, int64_t kg1, const void* a2, int64_t ldpa2, int64_t kg2, const void* b,
                              int64_t ldpb, const float* x, int64_t ldx, int64_t k1, const float* ahn, int64_t ldahn, int64_t k2,
                              const float* W, int64_t ldw, const float* bias, const float* gamma, const float* beta,
                              const float* stats, int relu, float* dW, int64_t lddw, float* dbias, float* dgamma, float* dbeta,
                              int64_t m, int64_t n, void* workspace, int64_t workspace_bytes, void* stream);
int64_t gte_gemm_p3_tn_workspace_bytes(int64_t m, int64_t n, int64_t nseg, int64_t k);
int gte_gemm_p3_tn(const void* a, int64_t ldpa, const void* a2, int64_t ldpa2, const void* b, int64_t ldpb, const void* b2,
                   int64_t ldpb2, int64_t nseg, float* c, int64_t ldc, int64_t m, int64_t n, int64_t k, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* gte_gemm_p3_tn with b = the rows b_rows[0 .. k) of a RESIDENT image b_res (the input layer's dW).  b_rows holds k rounded up
 * to 16, plus 1, entries; the entries past k = n_res_rows (a row past the image reads as zeros).  An image of 4 GB or more is
 * read through 64-bit addresses WITHOUT a range check: its allocation must then hold row n_res_rows, filled with zeros. */
int gte_gemm_p3_tn_rows(const void* a, int64_t ldpa, const void* a2, int64_t ldpa2, const void* b_res, int64_t ldpb,
                        const int32_t* b_rows, int64_t n_res_rows, int64_t nseg, float* c, int64_t ldc, int64_t m, int64_t n,
                        int64_t k, void* workspace, int64_t workspace_bytes, void* stream);
/* ... with two resident images behind the map: c[:, 0:nseg] = a^T b_res[rows], c[:, nseg:] = a^T b2_res[rows] (n == 2 nseg; same
 * row stride; the zero-row requirement above holds for both): dW = [dz^T x | dz^T ahn] of the input layer with a cached aggregate
 * (autograd of models.py:63 for `cat(h, ah * norm)`) -- the q = A_w^T (norm dz) aggregation of layer 0 is not needed at all. */
int gte_gemm_p3_tn_rows2(const void* a, int64_t ldpa, const void* b_res, int64_t ldpb, const void* b2_res, int64_t ldpb2,
                         const int32_t* b_rows, int64_t n_res_rows, int64_t nseg, float* c, int64_t ldc, int64_t m, int64_t n,
                         int64_t k, void* workspace, int64_t workspace_bytes, void* stream);
/* Second half of the fused head (gte_head_agg_ce) when the output layer's products run on the planes GEMMs: dlq [n][>= 32] holds
 * dl in columns 0 .. C-1 WITHOUT the 1 / sum(w) of the weighted cross-entropy (model_train.py:171,327) and -- when rindptr is
 * NULL -- q = A_w^T (norm dl) in columns 16 .. 16 + C-1; with the out-edge CSR (rindptr / rindices / w_out = w / in_degree(dst))
 * the launch forms q itself (autograd of models.py:53-54 for the class-count-wide aggregation).  It folds the CE partials of
 * gte_head_agg_ce (ce_partial), publishes out3 = {loss, sum w, #correct}, writes alpha [dl | q], alpha = grad_scale / sum w, as
 * ONE P3 image [n][32] (the operand of the layer's dW / dh GEMMs) and gbias [C] = column sums of alpha dl (block partials in
 * `workspace`, folded in order -- inside an open fold deferral by gte_fold_defer_flush). */
int64_t gte_head_dlq_finish_workspace_bytes(int64_t n_nodes);
int gte_head_dlq_finish(const int32_t* rindptr, const int32_t* rindices, const float* w_out, const float* dlq, int64_t lddlq,
                        int64_t n_nodes, int64_t n_classes, const void* ce_partial, float grad_scale, float* out3, void* dlqp3,
                        int64_t ldp, float* gbias, void* workspace, int64_t workspace_bytes, void* stream);
/* Which kernel family gte_gemm_p3_nt / _rows / _rows2 (epilogue 0), gte_gemm_p3_nt_ln_bwd (1; 3 = a width that is not a multiple
 * of 16) or gte_gemm_p3_nt[_rows2]_ln_fwd (4) would launch for [m x n] = [a1 | a2] b^T with k1 + k2 columns: 1 = the
 * block-major-weights kernel (weight fragments straight into registers, A through 64-deep LDS slots; needs block-major weights, one
 * column of 256-wide tiles, at least 32 K blocks, K padded by at most 1 / 12), 0 = the loader-wave / ring kernels.  *row_tile = the row
 * tile of the launch where it is chosen by the one-round rule (32 / 64 / 96, else 128), 0 where the tile chooser picks.  Host logic
 * only: with cus > 0 no device is touched (tests run it on the CPU); cus <= 0 reads the device's CU count. */
int gte_gemm_p3_nt_plan(int64_t m, int64_t n, int64_t k1, int64_t k2, int weights_block_major, int epilogue, int cus, int* row_tile);
/* The three setters below are TEST HOOKS with THREAD-LOCAL effect: they change what the calling host thread's later launches pick,
 * nothing any other thread sees (the library keeps no mutable process-wide state besides the GEMM mode above).  Environment
 * variables: the shipped library reads GTE_GEMM_MODE only; every other switch of earlier rounds lives in the measurement build
 * (libgte_hip_measure.so, -DGTE_MEASURE: csrc/gte_common.h).
 * Tile configuration of gte_gemm_p3_nt / _rows / _rows2: -1 = chosen per problem (default), 0 ... 7 = forced (tests run every
 * configuration against the same bits; 0 - 6 the 128- and 256-column tiles, 7 a measurement tile). */
int gte_gemm_p3_set_nt_cfg(int cfg);
/* Row tile of the launches with a LayerNorm epilogue (gte_gemm_p3_nt_ln_fwd / _rows2_ln_fwd / _ln_bwd; images below 4 GB): 0 = the
 * smallest of 32 / 64 / 96 rows that covers m in one round of workgroups, else 128 (default); 32 / 64 / 96 / 128 = forced (tests run
 * every tile against the same bits). */
int gte_gemm_p3_set_ln_rows(int rows);
/* Row maps: 0 = 64-bit addresses for resident images of 4 GB or more only (default), 1 = always (tests, A/B timing; the
 * zero-row requirement of gte_gemm_p3_tn_rows then holds for every image). */
int gte_gemm_p3_set_rows64(int mode);
/* gte_batch_assemble with a ROW MAP instead of (feat == NULL) or next to the copied feature rows: row_map[r] = resident row of
 * batch row r (r < n_out), row_map[n_out .. n_out + row_map_pad) = n_res_rows. */
int gte_batch_assemble_rows(const int32_t* pages, int64_t n_batch, const int32_t* node_off, const int32_t* b_node_off,
                            const gte_batch_arrays* in_edges, const gte_batch_arrays* out_edges, const float* feat,
                            int64_t ld_feat, int64_t n_cols, float* feat_out, const float* label, float* label_out,
                            int64_t n_out, int32_t* row_map, int64_t row_map_pad, int64_t n_res_rows, void* stream);

/* ---- dropout (models.py:60-61 and :105-113 of the reference in training mode, 0 < p < 1) ---------------------------------------
 * Counter-based keep bits (csrc/dropout.h): keep(seed, rank, step, site, row, col) = Philox4x32-10 of counter {col / 4, row, step,
 * site} under key {seed_lo, seed_hi ^ rank 0x9E3779B9}, word col % 4, >= round(p 2^32).  step = completed optimiser steps (the
 * plan's device step_counter), site 0 = the model's input dropout, i + 1 = the one mask of hidden layer i over its [n][2 fin]
 * concatenation cat(h, ah * norm) (columns fin + c = the aggregate half), row = the node's position in the batch.  The bits depend
 * on nothing else: producers and consumers regenerate them, no mask is stored.  A kept value is v * fp32(1 / (1 - p)) in fp32.
 * Matching torch's own dropout stream is not a goal (its element-to-counter mapping follows its launch grid).
 * gte_dropout_mask: TEST HOOK -- mask [n_rows][ldm] (uint8, 1 = kept) of one site at a host-given step, on the device.
 * gte_dropout_mask_host: the same bits from plain C++ (no HIP call: usable without a GPU). */
int gte_dropout_mask(float p, uint64_t seed, int rank, int64_t step, int site, int64_t n_rows, int64_t n_cols, uint8_t* mask,
                     int64_t ldm, void* stream);
int gte_dropout_mask_host(float p, uint64_t seed, int rank, int64_t step, int site, int64_t n_rows, int64_t n_cols, uint8_t* mask,
                          int64_t ldm);
/* Rows of a dropout launch / nodes of a dropout plan: row indices, the kernels' grid-stride sums and the Philox row word are 32-bit,
 * and 2^30 keeps all of them below 2^31.  There is NO byte bound: gte_spmm_dropout_p3 / _bwd address every image and row buffer
 * through 64-bit per-lane addresses (their gathers reach arbitrary rows), the planes GEMMs rebase their operand windows per tile
 * and stage, and the NT product's output window is rebased per wave tile in its WIDE form -- taken by gte_gemm_p3_nt when
 * (m + 256) ldc 4 >= 2^31 and, inside gte_gcnsage_step, for every launch of a dropout layer with
 * (n + 256) x 2 x max(ceil16(fout), ceil16(fin)) x 4 >= 2^31 (gte_gcnsage_step_wide_layers).  Below that the 32-bit form runs. */
#define GTE_DROPOUT_MAX_ROWS ((int64_t)1 << 30)
/* TEST HOOK, THREAD-LOCAL like the three gte_gemm_p3_set_* setters above: 1 = the calling host thread's later launches take the
 * wide form at any size (every layer of a dropout plan, and any gte_gemm_p3_nt output), 0 = by size (default).  It does not
 * reach launches another host thread issues (e.g. PyTorch's autograd thread): force it on the thread that calls
 * gte_gcnsage_step, and assert the form taken with gte_gcnsage_step_wide_layers.  gte_dropout_get_wide: this thread's mode. */
int gte_dropout_set_wide(int mode);
int gte_dropout_get_wide(void);
/* Producer of a dropout layer's operands (models.py:53-61 in training mode): with x' = D_0(x) when in_dropout (layer 0: the
 * model's input dropout applied to every gathered row and to the row's own features) else x,
 *     selfp3 = D_site(x'[v]),   aggp3 = D_site(scale_v sum_{u -> v} w_e x'[u])     (scale_v = 1 / in-degree, 0 without in-edges)
 * as two P3 images [n_rows][n_feat] (columns up to the next multiple of 16 written as zeros), the mask of the agg half at columns
 * n_feat + c.  The aggregation is gte_spmm_csr_p3's (same weights, norm, CSR summation order).  Input: fp32 rows x (ldx) OR a P3
 * image xp (ldpx bytes per row) whose row u is resident row x_rows[u] (x_rows NULL: row u) -- the resident feature images of the
 * train loop, decoded exactly.  step = *step_counter (device memory: captured replays draw fresh masks).  site >= 1.
 * EDGELESS GRAPH (indptr all zero, e.g. a batch of one-word pages): indices may be NULL, as for gte_spmm_csr_p3 -- the kernel reads
 * indices / eweight only inside a row's edge range; selfp3 is the masked input and aggp3 all zeros.  With any edge, indices must
 * point at them (a NULL eweight is unit weights at any size). */
int gte_spmm_dropout_p3(const int32_t* indptr, const int32_t* indices, const float* eweight, const float* x, int64_t ldx,
                        const void* xp, int64_t ldpx, const int32_t* x_rows, int64_t n_res_rows, int in_dropout, float p, uint64_t seed,
                        int rank, const int64_t* step_counter, int site, void* selfp3, int64_t ldp_self, void* aggp3, int64_t ldp_agg,
                        int64_t n_rows, int64_t n_feat, void* stream);
/* Backward of the above through the masks, for a layer whose input has a gradient (layer > 0): with G = dz W [n_rows][ldg]
 * (columns 0 .. n_feat the self half, agg_col .. agg_col + n_feat the aggregate half),
 *     dx[v] = D_site(G[v, self]) + sum_{v -> u} w_out D_site(G[u, agg])   (out-edge CSR, w_out = w / in_degree(dst); row u's mask)
 * dx [n_rows][lddx] fp32, columns n_feat .. round_up(n_feat, 4) written as zeros.  g, dx 16-byte aligned; agg_col, ldg, lddx
 * multiples of 4; agg_col >= round_up(n_feat, 4), ldg >= agg_col + round_up(n_feat, 4).
 * EDGELESS GRAPH (rindptr all zero): rindices and w_out may be NULL -- neither is read outside a row's edge range -- and
 * dx = D_site(G[:, self]).  With any edge both must point at one entry per edge (there is no unit-weight default here). */
int gte_spmm_dropout_bwd(const int32_t* rindptr, const int32_t* rindices, const float* w_out, const float* g, int64_t ldg,
                         int64_t agg_col, float p, uint64_t seed, int rank, const int64_t* step_counter, int site, float* dx,
                         int64_t lddx, int64_t n_rows, int64_t n_feat, void* stream);

/* ---- one optimisation step from a prepared plan -------------------------------------------------------------------------
 * replaces the batch loop body of model_train.py:320-332 (logits = model(g); loss; zero_grad; backward; optimizer.step())
 * for GcnSAGE with ReLU + LayerNorm hidden layers and a class-count-wide output layer -- dropout 0 (every shipped run of the
 * reference), or 0 < p < 1 with every hidden layer a GTE_LAYER_DROPOUT layer (dropout_p below) -- as ONE host call: the launches of a step (see models/engine.py for the same sequence
 * issued call by call) are issued from here, so the host cost of a step no longer grows with its ~17 launches (the
 * BBOX-only configurations, F0 = 13, were host-bound at ~0.25 ms of ctypes calls per 0.37 ms step).
 * The plan only borrows device pointers; nothing is allocated or synchronised.  Layer kinds:
 *   GTE_LAYER_PLANES  t = h [W_s ; W_n]^T on the planes GEMM, z = t_self + b + mean-aggregate(t_neigh), LayerNorm, ReLU;
 *                     input / dz / q as P3 images.  Any fout <= 1024 (the reference's runs: --h_layer_dim=1000 or
 *                     int(calculate_hidden) = 96 ... 218, run_multiple_train.sh:8-113): the fp32 row buffers of the layer are
 *                     PADDED to ldf = fout rounded up to 16 floats per row (t: two halves of ldf), the weight image holds zero
 *                     rows behind the fout rows of each half, LayerNorm statistics run over the true width
 *   GTE_LAYER_SMALLK  input layer with k = 2 fin <= 64 (BBOX features): aggregate-first, linear + LayerNorm + ReLU in one pass
 *   GTE_LAYER_AGGFIRST input layer that widens (fin < fout, e.g. 13 / 63 / 363 -> 1000): x and mean-aggregate(x) as P3 images,
 *                     z = [x | ahn] W^T + b on the planes GEMM (two K segments), LayerNorm + ReLU (gte_ln_relu_fwd_p3);
 *                     dW = [dz^T x | dz^T ahn] on the TN planes GEMM
 * followed by the output layer: the narrow kernels (gte_sage_narrow_*, gte_head_agg_ce; out_fin <= 256, out_fin % 8 == 0) or,
 * out_gemm = 1, the planes GEMMs (N = 32 forward; dW_out with M = n_classes; dh with K = 32).  phase: 0 the whole step; 1
 * everything up to the last weight-gradient GEMM, 2 the rest (the train loop queues the NEXT batch's assembly on its side
 * stream in between).
 *   GTE_LAYER_CACHED  input layer whose input AND its mean aggregate are RESIDENT P3 images read through the batch's row map
 *                     (hp / ahnp + h_rows): z = [x | ahn] W^T + b (gte_gemm_p3_nt_rows2), LayerNorm + ReLU; dW = [dz^T x | dz^T ahn]
 *                     (gte_gemm_p3_tn_rows2).  No aggregation, no q, no copy of the input in the step.  Any fin >= 16, fout <= 1024
 *   GTE_LAYER_DROPOUT hidden layer of a plan with dropout_p > 0 (then EVERY hidden layer is one; any depth, any fin, fout <= 1024):
 *                     aggregate-first, because the mask sits between the aggregation and W.  gte_spmm_dropout_p3 writes hp = D(x')
 *                     and ahnp = D(norm A_w x') (layer 0 also applies the input dropout; its input is x, or the image xp through
 *                     h_rows; a layer above reads x = y of the layer below), then the GEMM + LayerNorm + ReLU of AGGFIRST, z in t.
 *                     Backward: dW = dz^T [hp | ahnp] (TN, two segments); layer > 0 also G = dz W (planes NT on wimg_bwd = P3
 *                     [2 ceil16(fin)][fout] = [W_s^T ; W_n^T], the W_n^T rows from ceil16(fin)) into g, then gte_spmm_dropout_bwd
 *                     writes dy of the layer below.  No fused dX + LayerNorm-backward GEMM across a dropout layer.
 */
enum gte_layer_kind { GTE_LAYER_PLANES = 0, GTE_LAYER_SMALLK = 1, GTE_LAYER_AGGFIRST = 2, GTE_LAYER_CACHED = 3, GTE_LAYER_DROPOUT = 4 };
typedef struct gte_step_layer {
    int kind;
    int64_t fin, fout;
    const float* W; const float* bias; const float* gamma; const float* beta; float eps; int relu;
    float* gW; float* gbias; float* ggamma; float* gbeta;
    void* wimg_fwd; int64_t ldp_wfwd;      /* PLANES: P3 [2 fout][fin]   = [W_s rows ; W_n rows]            */
    void* wimg_bwd; int64_t ldp_wbwd;      /* PLANES, layer > 0: P3 [fin][2 fout] = [W_s^T | W_n^T]         */
    const float* x; int64_t ldx;           /* fp32 input rows (SMALLK; PLANES layer 0 when hp must be made) */
    void* hp; int64_t ldp_h;               /* PLANES: P3 image of the input [n][fin]                        */
    const int32_t* h_rows; int64_t n_res_rows;   /* PLANES layer 0: hp is the RESIDENT image, read through this row map */
    int make_hp;                           /* PLANES: 1 = convert x (fp32) into hp first                    */
    float* ahn;                            /* SMALLK: aggregated input [n][fin]                             */
    float* t;                              /* PLANES: [n][2 fout]; SMALLK: z [n][fout]                      */
    float* stats;                          /* [2 n]                                                         */
    float* y;                              /* fp32 output [n][fout] (NULL when only the next image is needed) */
    void* yp; int64_t ldp_y;               /* P3 image of the output for the next PLANES layer (or NULL)    */
    float* dy;                             /* [n][fout] gradient w.r.t. the output; dz in place             */
    void* dzp; void* qp; int64_t ldp_o;    /* PLANES: images [n][fout]                                      */
    void* ws_ln; int64_t ws_ln_bytes;      /* gte_ln_relu_bwd workspace                                     */
    void* ws_dw; int64_t ws_dw_bytes;      /* split-K workspace of the layer's dW                           */
    int64_t ldf;                           /* floats per row of y / dy / z (t: 2 ldf): fout rounded up to 16; 0 = fout */
    void* ahnp; int64_t ldp_ahn;           /* AGGFIRST: P3 image of the aggregated input [n][fin]; CACHED: the RESIDENT image of it */
    const void* xp; int64_t ldp_x;         /* DROPOUT layer 0: the input as a P3 image (through h_rows when set) instead of x  */
    float* g; int64_t ldg;                 /* DROPOUT layer > 0: G = dz W [n][ldg = 2 ceil16(fin)]                            */
} gte_step_layer;
typedef struct gte_step_plan {
    int n_hidden;                          /* hidden layers (1 .. 7), followed by the output layer          */
    gte_step_layer layer[7];
    int64_t out_fin, n_classes;            /* output layer                                                  */
    const float* W_out; const float* b_out; float* gW_out; float* gb_out;
    const float* h_out; int64_t ld_h_out;  /* fp32 input of the output layer (= y of the last hidden layer) */
    float* logits; float* tn; float* q_out; float* dl; float* dh_out;
    void* ce_part; int64_t ce_part_bytes; void* ws_nar; int64_t ws_nar_bytes;
    const int32_t* indptr; const int32_t* indices; const float* w_in;         /* in-edge CSR                */
    const int32_t* rindptr; const int32_t* rindices; const float* w_out;      /* out-edge CSR, weights x 1 / in_degree(dst) */
    int64_t n_nodes;
    const void* labels; int labels_f32; const float* class_weights; float grad_scale; float* out3;
    const void* wimg_descs; int n_wimg_descs;                                /* gte_p3_desc[]: the weight images */
    float* param; float* grad; float* exp_avg; float* exp_avg_sq; int64_t n_param;   /* fused Adam (NULL param: plain flush) */
    float* hyper; int64_t* step_counter; uint32_t* ticket;
    void* tail_ws; int64_t tail_ws_bytes;
    int fuse_ln_dx;                        /* bit 0: dX of a PLANES layer above a PLANES layer runs gte_gemm_p3_nt_ln_bwd;
                                              bit 1: the output layer's backward runs gte_sage_narrow_bwd_ln_p3;
                                              bit 2: the GEMM output layer (out_gemm) runs gte_head_agg_ce + gte_head_dlq_finish;
                                              bit 3: dX of layer 1 above a SMALLK layer 0 runs gte_gemm_p3_nt_smallk_bwd;
                                              bit 4: an AGGFIRST / CACHED input layer with fout <= 256 runs its LayerNorm forward as
                                                     the epilogue of its GEMM (gte_gemm_p3_nt[_rows2]_ln_fwd)                  */
    int wimg_fresh;                        /* the weight images already hold the current parameters: the forward skips their
                                              conversion launch (set by the caller after a step that returned *adam_fused & 2) */
    int wimg_in_fold;                      /* the fold + Adam launch also writes the weight images of the UPDATED parameters
                                              (gte_fold_defer_flush_adam_images); *adam_fused & 2 reports that it did        */
    /* output layer on the planes GEMMs (out_gemm = 1): logits / tn are columns 0.. / 16.. of ONE [n][32] fp32 buffer (logits =
     * its base, tn = logits + 16), dl / q_out likewise of a second one whose other columns stay zero; ld_lg = 32 */
    int out_gemm; int64_t ld_lg;           /* ld_lg: floats per row of logits / tn / dl / q_out (0 = n_classes)             */
    void* hp_out; int64_t ldp_hout;        /* P3 image of the output layer's input [n][out_fin] (yp of the last hidden layer) */
    void* wimg_out_fwd; int64_t ldp_wout_fwd;   /* P3 [32][out_fin]: rows 0.. = W_s rows, rows 16.. = W_n rows              */
    void* wimg_out_bwd; int64_t ldp_wout_bwd;   /* P3 [out_fin][32]: columns 0.. = W_s^T, 16.. = W_n^T                      */
    void* dlqp; int64_t ldp_dlq;           /* P3 image [n + 1][32] of the dl / q buffer                                     */
    void* ws_out; int64_t ws_out_bytes;    /* split-K workspace of dW_out: gte_gemm_p3_tn_workspace_bytes(C, 2 out_fin, out_fin, n) */
    void* ws_ce; int64_t ws_ce_bytes;      /* gte_weighted_ce workspace                                                     */
    void* ws_cs; int64_t ws_cs_bytes;      /* gte_colsum workspace                                                          */
    /* measurement (NULL: off): hipEvent_t handles, recorded on `stream` in front of ([2 i]) and behind ([2 i + 1]) the forward
     * transform GEMM of hidden layer i -- the roofline figure of a shape is timed inside the loop it belongs to */
    void* const* fwd_events;
    /* dropout (0 = off): 0 < dropout_p < 1 runs every hidden layer as GTE_LAYER_DROPOUT with the masks of seed / rank at step =
     * *step_counter (which must then be set, with or without the fused optimiser) */
    float dropout_p; uint64_t dropout_seed; int rank;
} gte_step_plan;
/* *adam_fused: bit 0 = the optimiser step ran inside the fold launch, bit 1 = ... and it wrote the weight images */
/* Which hidden layers of `plan` gte_gcnsage_step would run in the wide form on the calling thread: bit i = layer i (always 0 for a
 * plan without dropout); a negative error code for a null / malformed plan.  Host logic only. */
int gte_gcnsage_step_wide_layers(const gte_step_plan* plan);
int gte_gcnsage_step(const gte_step_plan* plan, int phase, int* adam_fused, void* stream);
/* The forward pass alone from the same plan (replaces `logits = model(g)` under no_grad: src/models/model_predict.py:141-147 and
 * the validation forward src/models/model_train.py:349-353): weight images, hidden layers, the output layer; logits [n, C] in
 * plan->logits.  The same kernels in the same order as the forward half of gte_gcnsage_step (bit-identical activations);
 * labels, gradients, optimiser fields and backward workspaces of the plan are ignored. */
int gte_gcnsage_forward(const gte_step_plan* plan, void* stream);

/* ---- deferred folds -------------------------------------------------------------------------------------------
 * Several entry points end with a small "sum the per-block partials" kernel (gte_ln_relu_bwd: column sums;
 * gte_sage_narrow_bwd: dW / dbias; split-K GEMMs behind gte_sage_linear_dw / gte_sage_qform_dw).  gte_gemm_f32 NEVER defers:
 * its result (e.g. dh of a backward) is read by the next kernel of the stream.  Between
 * gte_fold_defer_begin(stream) and gte_fold_defer_flush() (same host thread) those folds are queued instead of launched
 * and the flush runs all of them in ONE launch on `stream`.  While a deferral is open every such call needs its OWN
 * workspace (it holds the partials until the flush) and its results are not final before the flush.  Fixed summation
 * order: deterministic.  No counterpart in the reference (torch autograd launches one reduction per parameter). */
int gte_fold_defer_begin(void* stream);
int gte_fold_defer_flush(void);
/* Close the deferral and, when the queued folds write every element of the flat gradient [grad, grad + n) exactly once,
 * run them AND the optimiser step of gte_adam_step_dev (same state / step_counter / ticket contract, same arithmetic) in
 * ONE launch: the thread that folds a gradient element applies its Adam update.  *fused = 1 then.  Otherwise (a gradient
 * some producer wrote directly, a deferral that overflowed) the folds run as gte_fold_defer_flush would, *fused = 0, and the
 * caller launches gte_adam_step_dev itself.  grad still receives the folded gradient either way. */
int gte_fold_defer_flush_adam(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                              int64_t* step_counter, unsigned* ticket, int* fused);
/* ... and, in the same launch, the P3 images of up to 12 sub-matrices of the UPDATED parameters (every `src` inside
 * [param, param + n); the descriptors of gte_p3_from_f32_batch): the thread that updates a parameter element writes its three
 * bf16 pieces into each image holding it -- bit for bit what gte_p3_from_f32_batch makes of the updated parameters, without
 * the launch in front of the next step's first GEMM.  Padding columns of the images are not touched (zero them once).
 * *fused = 3 when the step and the images were written, 1 when more than 12 images were asked for (or one with a single source column) (step applied, images not),
 * 0 as gte_fold_defer_flush_adam. */
int gte_fold_defer_flush_adam_images(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                                     int64_t* step_counter, unsigned* ticket, const gte_p3_desc* images, int n_images, int* fused);

/* ---- transform-then-aggregate ("q-form") of a GcnSAGELayer --------------------------------------------------
 * replaces (reference src/components/graphs/models.py:53-72, `torch.cat((h, ah * norm), 1)` -> nn.Linear) where the
 * layer narrows: by linearity  z = h W_s^T + b + norm * A_w (h W_n^T), so the aggregation moves n_out columns
 * instead of n_feat.  Backward with q = A_w^T (norm * dz):  dW = [dz^T h | q^T h],  dh = dz W_s + q W_n.
 *   gte_sage_transform_fwd : t[:, 0:n_out] = x W_s^T + bias,  t[:, n_out:2 n_out] = x W_n^T      (one GEMM launch)
 *   gte_sage_qform_dw      : dW[n_out, 2 n_feat] = [dz^T x | q^T x]                               (split over nodes)
 *   gte_sage_qform_dx      : dx[nodes, n_feat]   = dz W_s + q W_n                                 (one GEMM, K = 2 n_out)
 * W is the layer weight [n_out][2 n_feat] (ldw >= 2 n_feat).  All matrices fp32 row-major with leading dimensions. */
int gte_sage_transform_fwd(const float* x, int64_t ldx, int64_t n_feat, const float* W, int64_t ldw, const float* bias,
                           int64_t n_out, float* t, int64_t ldt, int64_t n_nodes, void* stream);
int64_t gte_sage_qform_dw_workspace_bytes(int64_t n_out, int64_t n_feat, int64_t n_nodes);
int gte_sage_qform_dw(const float* dz, int64_t lddz, const float* q, int64_t ldq, const float* x, int64_t ldx,
                      int64_t n_feat, float* dW, int64_t lddw, int64_t n_out, int64_t n_nodes, void* workspace,
                      int64_t workspace_bytes, void* stream);
int gte_sage_qform_dx(const float* dz, int64_t lddz, const float* q, int64_t ldq, const float* W, int64_t ldw,
                      int64_t n_feat, int64_t n_out, float* dx, int64_t lddx, int64_t n_nodes, void* stream);

/* The class-count-wide output layer (hidden -> n_classes, no LayerNorm / activation: models.py:101-103) in
 * transform-then-aggregate form (n_out <= 16, n_feat <= 256; gte_sage_narrow_supported says so):
 *   fwd: t_self = h W[:, 0:F]^T + bias, t_neigh = h W[:, F:2F]^T;  the caller finishes with
 *        logits = t_self + mean-aggregate(t_neigh)  (gte_spmm_csr_accumulate, REDUCE_MEAN) -- by linearity equal to
 *        [h | norm * A_w h] W^T + b of models.py:53-72, with the aggregation on n_out columns instead of n_feat.
 *   bwd: given dl = dlogits and q = A_w^T(norm * dl) (gte_spmm_csr over the out-edge CSR), writes
 *        dh = dl W_s + q W_n (nullable), dW = [dl^T h | q^T h], dbias = colsum(dl).  Reads h once. */
int gte_sage_narrow_supported(int64_t n_feat, int64_t n_out);
int gte_sage_narrow_fwd(const float* h, int64_t ldh, int64_t n_feat, const float* W, int64_t ldw, const float* bias,
                        int64_t n_out, float* t_self, int64_t ld_self, float* t_neigh, int64_t ld_neigh,
                        int64_t n_nodes, void* stream);
/* gte_sage_narrow_fwd on the output of a LayerNorm(+ReLU) that has not been applied yet: z is the pre-LayerNorm output of
 * the layer below (models.py:63); the kernel writes y = relu?(LN(z)) (models.py:64-66) and stats = {mean[n], rstd[n]} for the
 * backward and multiplies the normalised rows in the same pass -- one launch and one pass over [n, n_feat] less than
 * gte_ln_relu_fwd + gte_sage_narrow_fwd.  n_feat % 8 == 0 (gte_sage_narrow_fwd_ln_supported). */
int gte_sage_narrow_fwd_ln_supported(int64_t n_feat, int64_t n_out);
int gte_sage_narrow_fwd_ln(const float* z, int64_t ldz, int64_t n_feat, const float* gamma, const float* beta, float eps,
                           int relu, float* y, int64_t ldy, float* stats, const float* W, int64_t ldw, const float* bias,
                           int64_t n_out, float* t_self, int64_t ld_self, float* t_neigh, int64_t ld_neigh, int64_t n_nodes,
                           void* stream);
int64_t gte_sage_narrow_bwd_workspace_bytes(int64_t n_nodes, int64_t n_feat, int64_t n_out);
int gte_sage_narrow_bwd(const float* dl, int64_t lddl, const float* q, int64_t ldq, const float* h, int64_t ldh,
                        int64_t n_feat, const float* W, int64_t ldw, int64_t n_out, float* dh, int64_t lddh,
                        float* dW, int64_t lddw, float* dbias, int64_t n_nodes,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* The fused head of the train step (class-count-wide output layer + weighted cross-entropy, model_train.py:171,327-328
 * after models.py:101-103).  gte_head_supported(n_feat, n_classes): n_classes <= 16, n_feat <= 256, n_feat % 8 == 0.
 *   gte_head_agg_ce : logits[v,:] (in: t_self + bias from gte_sage_narrow_fwd) += scale_v * sum_e w[e] t_neigh[src,:]  (the
 *        same sums, bit for bit, as gte_spmm_csr_accumulate), then per node the weighted CE terms and the UNNORMALISED
 *        gradient dl'[v,:] = w_y (softmax - onehot); per-block partials {sum w nll, sum w, #correct} go to ce_partial
 *        (>= gte_head_agg_ce_workspace_bytes(n_nodes), must stay untouched until gte_sage_narrow_bwd_ce has run).
 *   caller: q' = gte_spmm_csr(out-edge CSR, mean weights, dl')   (linear: the missing 1 / sum(w) commutes with it)
 *   gte_sage_narrow_bwd_ce : gte_sage_narrow_bwd on alpha * dl', alpha * q' with alpha = grad_scale / sum(w) folded from
 *        ce_partial inside the kernel; also writes out3 = {loss, sum w, #correct} like gte_weighted_ce.
 * Three launches (aggregation, CE partial, CE gradient) become one and the loss never needs a launch of its own. */
int gte_head_supported(int64_t n_feat, int64_t n_classes);
int64_t gte_head_agg_ce_workspace_bytes(int64_t n_nodes);
int gte_head_agg_ce(const int32_t* indptr, const int32_t* indices, const float* eweight, const float* t_neigh,
                    int64_t ld_neigh, float* logits, int64_t ld_logits, const void* labels, int labels_f32,
                    const float* class_weight, int64_t n_nodes, int64_t n_classes, int reduce, float* dl_unscaled,
                    int64_t lddl, void* ce_partial, int64_t ce_partial_bytes, void* stream);
int gte_sage_narrow_bwd_ce(const float* dl_unscaled, int64_t lddl, const float* q_unscaled, int64_t ldq, const float* h,
                           int64_t ldh, int64_t n_feat, const float* W, int64_t ldw, int64_t n_out, float* dh,
                           int64_t lddh, float* dW, int64_t lddw, float* dbias, int64_t n_nodes, void* workspace,
                           int64_t workspace_bytes, const void* ce_partial, float grad_scale, float* out3, void* stream);

/* gte_sage_narrow_bwd_ce (ce_partial may be NULL: then dl / q are final and out3 is untouched) fused with the
 * LayerNorm(+ReLU) backward of the layer below, whose output h = relu?(LN(z_below)) fed the output layer: instead of dh the
 * call writes dz_below = LN'(z_below)(mask . dh) and the parameter gradients dgamma / dbeta / dbias of the layer below
 * (each nullable) -- the [N, F] matrix dh is neither written nor read back by a separate gte_ln_relu_bwd.
 * ln_workspace >= gte_sage_narrow_bwd_ln_workspace_bytes(n_nodes, n_feat); its folds join an open deferral
 * (gte_fold_defer_begin) or run as one launch.  Same support rule as gte_head_supported. */
int64_t gte_sage_narrow_bwd_ln_workspace_bytes(int64_t n_nodes, int64_t n_feat);
/* Row form: the dh tile of every 32-row block goes through LDS and whole rows get the LayerNorm(+ReLU) backward with 16-byte
 * accesses and the arithmetic of gte_ln_relu_bwd; dz_below as fp32 AND as a P3 image (dzp3 nullable; n_feat % 16 == 0).  Bit for
 * bit gte_sage_narrow_bwd[_ce] + gte_ln_relu_bwd_p3.  (Round 2's accumulator-layout form gte_sage_narrow_bwd_ln and round 3's
 * option of forming q inside the kernel measured slower than what they replaced and were removed in round 4.) */
int gte_sage_narrow_bwd_ln_p3(const float* dl, int64_t lddl, const float* q, int64_t ldq, const float* h, int64_t ldh,
                              int64_t n_feat, const float* W, int64_t ldw, int64_t n_out, float* dz_below, int64_t lddz,
                              void* dzp3, int64_t ldp3, float* dW, int64_t lddw, float* dbias, int64_t n_nodes, void* workspace,
                              int64_t workspace_bytes, const void* ce_partial, float grad_scale, float* out3,
                              const float* z_below, int64_t ldz, const float* stats_below, const float* gamma_below,
                              const float* beta_below, int relu_below, float* dgamma_below, float* dbeta_below,
                              float* dbias_below, void* ln_workspace, int64_t ln_workspace_bytes, void* stream);
/* The output layer on PADDED hidden rows (round 5: hidden widths that are not a multiple of 8 -- int(calculate_hidden) = 100 / 139 /
 * 149 / 157 / 206 / 218 of the reference's scaled runs -- keep the narrow kernels instead of three planes GEMMs): h, z_below and
 * dz_below rows hold n_feat true columns and zeros up to n_pad (a multiple of 16, <= 256); W / dW are the reference's [C][2 n_feat].
 * The products run over n_pad columns against a weight image whose padding is zero (the same sums); the fused LayerNorm backward
 * runs over the n_feat true columns with the arithmetic of gte_ln_relu_bwd_p3 at that width.  dz_below is written in whole 16-byte
 * chunks of the true width: columns n_feat .. the next multiple of 4 as zeros; the columns from there to n_pad are NOT written -- they
 * stay what the caller put there (the one-call plan zero-initialises the buffer once, and nothing else writes it).  The image is
 * written as zeros in all of its padding (n_pad / 16 blocks).  tests/test_gpu_narrow_layer.py pins both.  Workspace sizes: the
 * functions above with n_feat = n_pad. */
int gte_sage_narrow_pad_supported(int64_t n_feat, int64_t n_pad, int64_t n_out);
int gte_sage_narrow_fwd_pad(const float* h, int64_t ldh, int64_t n_feat, int64_t n_pad, const float* W, int64_t ldw, const float* bias,
                            int64_t n_out, float* t_self, int64_t ld_self, float* t_neigh, int64_t ld_neigh, int64_t n_nodes,
                            void* stream);
int gte_sage_narrow_bwd_ln_p3_pad(const float* dl, int64_t lddl, const float* q, int64_t ldq, const float* h, int64_t ldh,
                                  int64_t n_feat, int64_t n_pad, const float* W, int64_t ldw, int64_t n_out, float* dz_below,
                                  int64_t lddz, void* dzp3, int64_t ldp3, float* dW, int64_t lddw, float* dbias, int64_t n_nodes,
                                  void* workspace, int64_t workspace_bytes, const void* ce_partial, float grad_scale, float* out3,
                                  const float* z_below, int64_t ldz, const float* stats_below, const float* gamma_below,
                                  const float* beta_below, int relu_below, float* dgamma_below, float* dbeta_below,
                                  float* dbias_below, void* ln_workspace, int64_t ln_workspace_bytes, void* stream);

/* LayerNorm + ReLU alone (row-wise over n_out):  y = relu?(gamma * (z - mean) * rstd + beta).
 * replaces models.py:64-66 when the caller ran the linear part separately.  In place (y == z) is
 * allowed.  stats (nullable): f32[2*M] = mean, rstd.
 * Pinned by tests/test_gpu_layernorm.py for this entry point and every fused forward form: two-pass statistics (the mean, then the
 * sum of (z - mean)^2), the BIASED variance over the n_out true columns (never a padded width), rstd = 1 / sqrt(var + eps) with eps
 * inside the square root, y = max(pre, 0) on pre = xhat gamma + beta.  An all-zero row is exact: mean 0, y = relu?(beta). */
int gte_ln_relu_fwd(const float* z, int64_t ldz, const float* gamma, const float* beta, float eps, int relu,
                    float* y, int64_t ldy, float* stats, int64_t M, int64_t n_out, void* stream);

/* ... on PADDED rows of any width up to 1024 (ldz, ldy >= n_out rounded up to 4 floats), y as fp32 (nullable) and / or as a
 * P3 image (nullable; its columns up to the next multiple of 16 are written as zeros): the LayerNorm(+ReLU) of an
 * aggregate-first planes layer (GTE_LAYER_AGGFIRST).  Same two-pass statistics over the n_out true columns. */
int gte_ln_relu_fwd_p3(const float* z, int64_t ldz, const float* gamma, const float* beta, float eps, int relu, float* y,
                       int64_t ldy, void* yp3, int64_t ldyp3, float* stats, int64_t M, int64_t n_out, void* stream);

/* Backward of LayerNorm+ReLU (+ bias grad):  given dy, the saved z and stats, writes
 *   dz[M,n_out], and WRITES the column sums dgamma, dbeta, dbias (f32[n_out], nullable; no zero-init needed).
 * With gamma == NULL it is the backward of (relu?)(z) only.  dz may alias dy unless gamma != NULL and
 * n_out > 1024 (wide rows are re-read).
 * The ReLU mask is DEFINED on the stored stats: xhat = (z - stats.mean) * stats.rstd, pre = fma(xhat, gamma, beta), gradient where
 * pre > 0 and 0 at pre == 0 (torch.relu).  A forward form that subtracts the mean as fma(-1 / n, sum, z) (gte_ln_relu_fwd_p3,
 * gte_gemm_p3_nt_ln_fwd) can round an element whose |pre| is within about |mean| / std * 2^-24 * |gamma| of zero to the other side;
 * tests/test_gpu_layernorm.py counts those elements and holds every other one to the float64 reference.  The one-pass short-input
 * forward (gte_sage_linear_fwd / _p3 where gte_sage_linear_fwd_fuses_ln) subtracts the ROUNDED mean it stores, so its y > 0 IS this
 * mask at every element and every n_out: gte_sage_smallk_bwd and gte_gemm_p3_nt_smallk_bwd, which rebuild xhat from the stats, rest
 * on that (tests/test_gpu_smallk_bwd.py asserts it with nothing exempted).
 * workspace: gte_ln_relu_bwd_workspace_bytes(M, n_out). */
int64_t gte_ln_relu_bwd_workspace_bytes(int64_t M, int64_t n_out);
int gte_ln_relu_bwd(const float* dy, int64_t lddy, const float* z, int64_t ldz, const float* stats,
                    const float* gamma, const float* beta, int relu,
                    float* dz, int64_t lddz, float* dgamma, float* dbeta, float* dbias,
                    int64_t M, int64_t n_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ReLU + row L2-normalise (row-wise over n_out), torch.nn.functional.normalize(relu?(z), p=2, dim=1, eps):
 *   r = relu ? max(z, 0) : z;  s = sqrt(sum_j r_j^2);  y = r / max(s, eps);  norm[i] = s (unclamped; f32[M], nullable).
 * replaces models.py:166-168 (`F.normalize(F.relu(h))` between the layers of MeanSAGE).  In place (y == z) is allowed.
 * Any n_out >= 1 (<= 2^30) and any ld >= n_out; columns beyond n_out are neither read nor written.  eps > 0. */
int gte_relu_l2norm_fwd(const float* z, int64_t ldz, int relu, float eps, float* y, int64_t ldy, float* norm, int64_t M,
                        int64_t n_out, void* stream);
/* Its backward (+ bias grad), from dy, the forward's y and norm (same relu and eps):
 *   d = max(norm[i], eps);  proj = norm[i] >= eps ? sum_j y_j dy_j : 0;  dr = (dy - y proj) / d;
 *   dz = relu ? (y > 0 ? dr : 0) : dr;  dbias[c] = sum_i dz[i][c]  (f32[n_out], nullable; WRITTEN, no zero-init needed; summed
 *   in a fixed order: deterministic).  dz may alias dy.
 * workspace: gte_relu_l2norm_bwd_workspace_bytes(M, n_out), read only when dbias is given (may be NULL otherwise). */
int64_t gte_relu_l2norm_bwd_workspace_bytes(int64_t M, int64_t n_out);
int gte_relu_l2norm_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* norm, int relu, float eps,
                        float* dz, int64_t lddz, float* dbias, int64_t M, int64_t n_out, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* General fp32 MFMA GEMM used by the backward:  C[M,N] (+)= op(A)[M,K] * op(B)[K,N]
 *   trans_a = 0: A is [M,K] row-major (lda);  1: A is stored [K,M] (lda) and used transposed
 *   trans_b = 0: B is [K,N] row-major (ldb);  1: B is stored [N,K] (ldb) and used transposed
 * accumulate != 0 adds into C.  K may be huge (dW = dZ^T X reduces over the nodes): the kernel
 * splits K across workgroups and reduces the partial slabs deterministically in `workspace`
 * (gte_gemm_workspace_bytes).  replaces autograd of nn.Linear (models.py:63). */
int64_t gte_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int gte_gemm_f32(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K,
                 const float* A, int64_t lda, const float* B, int64_t ldb,
                 float* C, int64_t ldc, int accumulate,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A10  loss and optimiser
 * gte_weighted_ce: replaces nn.CrossEntropyLoss(weight)(logits, labels.long()) forward+backward
 *   (model_train.py:171,327) and the accuracy count (:328).
 *   loss = sum_i w[y_i] * nll_i / sum_i w[y_i]   (w == NULL => plain mean)
 *   dlogits (nullable) = grad_scale * d loss / d logits.
 *   out3: f32[3] = {loss, sum of weights, #correct (argmax == label)}.
 *   labels: int64[n]  (labels_f32 != 0: float32 holding integers, loader.py:350-354).
 *   A node whose label is outside [0, n_classes) is ignored: it adds nothing to the loss, the sum of
 *   weights or #correct, and its dlogits row is zero.
 *   When the sum of weights is 0 (every node ignored or of a zero-weight class) the loss is 0 and
 *   every dlogits row is zero.
 * workspace: gte_weighted_ce_workspace_bytes(n).
 * ---------------------------------------------------------------------------------------- */
int64_t gte_weighted_ce_workspace_bytes(int64_t n_nodes);
int gte_weighted_ce(const float* logits, int64_t ld, const void* labels, int labels_f32,
                    const float* class_weight, int64_t n_nodes, int n_classes, float grad_scale,
                    float* dlogits, int64_t lddl, float* out3,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* out[c] = sum_r x[r][c], c < n_cols <= 64: the bias gradient of the output layer (colsum of dlogits; autograd of the
 * nn.Linear bias, models.py:101-103) when its backward runs on the planes GEMMs.  Block partials in a fixed order; the fold
 * joins an open fold deferral.  workspace: gte_colsum_workspace_bytes(n_rows, n_cols). */
int64_t gte_colsum_workspace_bytes(int64_t n_rows, int64_t n_cols);
int gte_colsum(const float* x, int64_t ldx, int64_t n_rows, int64_t n_cols, float* out, void* workspace,
               int64_t workspace_bytes, void* stream);

/* gte_adam_step: replaces torch.optim.Adam(lr, weight_decay).step() (model_train.py:168,332) on one
 * flat fp32 buffer: g' = grad_scale*g + weight_decay*p (L2-coupled, NOT AdamW);
 * m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).
 * `step` is t (1-based).  lr is read from the host value. */
int gte_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                  float grad_scale, void* stream);
/* The same update with everything that changes from step to step read from DEVICE memory, so the launch can be captured
 * in a HIP graph.  state (8 floats, read AND advanced by the call) = {lr, beta1, beta2, eps, weight_decay, grad_scale,
 * bc1 = 1 - beta1^t, sqrt(bc2) = sqrt(1 - beta2^t)} for t = *step_counter + 1; the last block to finish sets
 * *step_counter = t and the two bias corrections for t + 1 (double arithmetic, like the host-scalar version).
 * `ticket` is gte_adam_ticket_bytes() bytes of zero-initialised scratch that the call returns to zero (sharded completion
 * counters: one counter for a thousand workgroups is a 12 - 20 us queue).  The caller initialises state and counter
 * consistently (and may rewrite lr at any time between launches). */
int64_t gte_adam_ticket_bytes(void);
int gte_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                      int64_t* step_counter, unsigned* ticket, void* stream);
/* gte_adam_step_dev + the P3 images of the UPDATED parameters in the same launch (images: sub-matrices of `param`, as
 * gte_fold_defer_flush_adam_images takes them): the optimiser launch of the data-parallel step (behind the all-reduce of
 * model_train.py:327-332's gradients, where the fold launch cannot apply the update) leaves the weight images of the next forward
 * behind.  *wrote = 1 when the images were written (a list of more than 12 images is skipped). */
int gte_adam_step_dev_images(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                             int64_t* step_counter, uint32_t* ticket, const gte_p3_desc* images, int n_images, int* wrote,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * A13  multi-head graph attention (BASELINE.json configs[2]).  The reference has NO GAT: the
 * layer is the standard formulation (DGL GATConv semantics), oracle = oracle/gat_cpu.py, parity unpinned.
 *   z [N, H*D] (= X W, computed with gte_gemm_f32);  heads <= 8, heads*dim <= 1024
 * gte_gat_scores: el[v,h] = <a_l[h], z[v,h]>, er likewise; optionally writes a bf16 copy of z for the gathers.
 * gte_gat_aggregate_fwd: e = LeakyReLU_0.2(el[u] + er[v]) over in-edges, online softmax, out[v] = sum alpha z[u] (+bias);
 *   saves the softmax max / sum per (node, head) for the backward.  dtype = storage of the gathered z (f32 / bf16).
 * gte_gat_aggregate_bwd: given dout, writes dz (incl. the el/er paths), d a_l, d a_r, d bias; ds [E,H], der, del [N,H]
 *   are caller-provided scratch outputs; pos_in[i] = position in the in-edge CSR of the i-th out-edge-CSR entry.
 * ---------------------------------------------------------------------------------------- */
int gte_gat_scores(const float* z, int64_t ldz, const float* a_l, const float* a_r, float* el, float* er,
                   void* z_bf16 /* nullable */, int64_t ldzb, int64_t n_nodes, int heads, int dim, void* stream);
int gte_gat_aggregate_fwd(const int32_t* indptr, const int32_t* indices, const void* z, int64_t ldz, int dtype,
                          const float* el, const float* er, const float* bias /* nullable */, float* out, int64_t ldo,
                          float* smax, float* ssum, int64_t n_nodes, int heads, int dim, void* stream);
/* The same with an epilogue (BASELINE configs[2]): activation 1 = ELU applied to (aggregate + bias) -- the activation between
 * GAT layers; out_bf16 (nullable): bf16 copy of that output, the next layer's gte_gemm_bf16_nt operand; out_mean (nullable):
 * [n, dim] mean over the heads + mean_bias[dim] -- the output layer (then `out` may be NULL).
 * gte_gat_dout_prepare turns the gradient w.r.t. such an output back into the gradient gte_gat_aggregate_bwd takes:
 * dfull[v, f] = (mean_heads ? dout[v, f % dim] / heads : dout[v, f]) * (act_out ? ELU'(act_out[v, f]) : 1). */
int gte_gat_aggregate_fwd_ex(const int32_t* indptr, const int32_t* indices, const void* z, int64_t ldz, int dtype,
                             const float* el, const float* er, const float* bias, float* out, int64_t ldo, float* smax,
                             float* ssum, int64_t n_nodes, int heads, int dim, int activation, void* out_bf16, int64_t ldob,
                             float* out_mean, int64_t ldom, const float* mean_bias, void* stream);
int gte_gat_dout_prepare(const float* dout, int64_t lddo, const float* act_out, int64_t ldao, float* dfull, int64_t lddf,
                         int64_t n_nodes, int heads, int dim, int mean_heads, void* stream);
int64_t gte_gat_bwd_workspace_bytes(int64_t n_nodes, int heads, int dim);
int gte_gat_aggregate_bwd(const int32_t* indptr, const int32_t* indices, const int32_t* rindptr, const int32_t* rindices,
                          const int32_t* pos_in, const void* z, int64_t ldz, int dtype, const float* z_f32, int64_t ldzf,
                          const float* el, const float* er, const float* smax, const float* ssum,
                          const float* a_l, const float* a_r, const float* dout, int64_t lddo,
                          float* ds, float* der, float* del, float* dz, int64_t lddz,
                          float* da_l, float* da_r, float* dbias, int64_t n_nodes, int heads, int dim,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* The same with gte_gat_dout_prepare folded in: dfull (nullable; [n, heads * dim] scratch) receives the effective gradient
 * (mean_heads ? dout[v, f % dim] / heads : dout[v, f]) * (act_out ? ELU'(act_out[v, f]) : 1), formed by the destination-side
 * kernel itself where the row-layout kernels apply (heads <= 4, dim <= 64: no separate pass over the three [n, heads * dim]
 * arrays) and by a gte_gat_dout_prepare launch otherwise.  dfull == NULL: dout is used as given (gte_gat_aggregate_bwd). */
int gte_gat_aggregate_bwd_ex(const int32_t* indptr, const int32_t* indices, const int32_t* rindptr, const int32_t* rindices,
                             const int32_t* pos_in, const void* z, int64_t ldz, int dtype, const float* z_f32, int64_t ldzf,
                             const float* el, const float* er, const float* smax, const float* ssum,
                             const float* a_l, const float* a_r, const float* dout, int64_t lddo,
                             const float* act_out, int64_t ldao, int mean_heads, float* dfull, int64_t lddf,
                             float* ds, float* der, float* del, float* dz, int64_t lddz,
                             float* da_l, float* da_r, float* dbias, int64_t n_nodes, int heads, int dim,
                             void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GTE_H_ */
