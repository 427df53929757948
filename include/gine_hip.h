/*
 * gine_hip.h -- C ABI of the MI355X (gfx950) GINEConv message-passing engine.
 *
 * This is the drop-in boundary for the hot path of SohirMaskey/raincast-gnn:
 *   models/gnn.py:20-29   ResGnn builds GINEConv(nn=Linear->BatchNorm1d->ReLU->Linear,
 *                          train_eps=True, edge_dim=1)
 *   models/gnn.py:41,44   conv(x, edge_index, edge_attr)   (called once per layer per step)
 * The arithmetic behind that call lives in torch_geometric (GINEConv.message /
 * MessagePassing.propagate / SumAggregation -> scatter_add_), which is not vendored in the
 * reference (environment.yml:29-31).  Every entry point below names the reference-side
 * operation it replaces.
 *
 * Conventions
 *   - All tensors are device pointers (HBM), row-major, contiguous, fp32 unless stated.
 *   - Every buffer (outputs and workspace) is allocated by the caller; no entry point
 *     allocates, frees or synchronises, so every call is legal inside hipGraph capture.
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream).
 *   - Return value: GINE_OK, a GINE_ERR_* code, or GINE_ERR_HIP_BASE + hipError_t.
 *   - No hidden global state: the library holds nothing but its immutable kernels, so
 *     calls are re-entrant from any host thread (PyTorch runs backward on its autograd
 *     device thread).
 */
#ifndef GINE_HIP_H_
#define GINE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GINE_ABI_VERSION 10 /* 2: adamw step-state query, gine_count_valid, window plan slot/edge_begin;
                              3: gine_deepset_bwd_num_partials takes the hidden width;
                              4: bn_acc grows two grid-barrier words (gine_mp_fwd_layer);
                              5: grid-barrier failure count (gine_bn_acc_barrier_failures_index),
                                 gine_mlp_bwd_layer removed;
                              6: gine_mlp_bwd_layer again, in the forward layer's role-split form;
                              7: gine_mp_fwd_layer takes the layer window plan
                                 (gine_graph_plan_layer_windows, gine_mp_fwd_layer_windows_fit);
                              8: gine_mp_fwd_layer can also run the output head (gine_layer_head);
                              9: the seven entry points of the singly folded dense chain are removed
                                 (the doubly folded form is the chain; the unfolded one stays as
                                 the tests' comparator);
                              10: gine_mp_fwd_layer_eval (the eval-mode layer in one launch); later,
                                  additive within 10: gine_mp_fwd_layer_eval_deep (any in-degree),
                                  gine_forecast_prob / _quantile / _score(_partials),
                                  gine_graph_build_ek / gine_graph_same_edges_ek and
                                  gine_mp_fwd_ek / gine_mp_bwd_ek(_num_partials, _finalize): edge_dim
                                  up to GINE_MP_MAX_EDGE_DIM and the edge_attr gradient,
                                  gine_grad_sumsq(_num_partials) / gine_adamw_step_ctl /
                                  gine_adamw_ctl_bytes: the AdamW step under a device control
                                  block (schedule, clipping, skipping of non-finite steps),
                                  gine_ensemble_score / gine_ensemble_ecc: the raw ensemble's
                                  scores and ECC members,
                                  gine_forecast_twcrps(_partials) / gine_ensemble_twcrps /
                                  gine_crps_tw_fwd / _fwd_grad / _bwd: the threshold-weighted
                                  CRPS as a score and as a loss term,
                                  gine_field_energy / _variogram / _area(_partials): member
                                  fields scored per graph,
                                  gine_batch_fill_permuted: a batch with permuted feature
                                  columns written into a forward's inputs,
                                  gine_compare_reduce / _bootstrap / _dm: paired score
                                  comparison (block bootstrap, Diebold-Mariano),
                                  gine_reliability_counts / _fit / _resample: reliability
                                  diagrams (CORP curves, consistency bands, MCB / DSC / UNC),
                                  gine_emos_predictors / _fit / _predict: the per-station EMOS
                                  baseline fitted by minimum CRPS */

#define GINE_OK 0
#define GINE_ERR_INVALID 1    /* null pointer, negative size, bad flag */
#define GINE_ERR_DIM 2        /* unsupported channel count */
#define GINE_ERR_WORKSPACE 3  /* workspace smaller than gine_graph_workspace_bytes() */
#define GINE_ERR_TOO_LARGE 4  /* num_nodes or num_edges >= 2^31 */
#define GINE_ERR_HIP_BASE 1000

/* Library identity. */
int gine_abi_version(void);
const char* gine_status_string(int status);

/* ------------------------------------------------------------------------------------
 * Graph preparation.  Replaces the implicit per-call work of PyG's gather/scatter
 * (x.index_select(0, edge_index[0]) and zeros.scatter_add_(0, edge_index[1], .)) with
 * two stable counting structures built once per distinct edge_index:
 *   CSR by destination (in-edges):  in_rowptr[N+1], in_src[E], in_attr[E]
 *   CSR by source      (out-edges): out_rowptr[N+1], out_dst[E], out_attr[E]
 * Within a node's segment edges keep their original order (stable), which is exactly
 * the order in which CPU scatter_add_ / index_add_ accumulate.
 *   edge_index: int64 [2, E] (row 0 = source j, row 1 = target i; flow source_to_target)
 *   edge_attr : fp32 [E] (edge_dim = 1) or NULL (then in_attr/out_attr are not written)
 *   d_error   : device int32, OR-ed with 1 when an index lies outside [0, N); the caller
 *               zeroes it before the call and reads it when convenient.
 * Reference: utils/data.py:261-284 (edge layout), models/gnn.py:41,44 (consumer).
 * ---------------------------------------------------------------------------------- */
int gine_graph_workspace_bytes(int64_t num_nodes, int64_t num_edges, size_t* bytes);
int gine_graph_build(const int64_t* edge_index, const float* edge_attr, int64_t num_nodes,
                     int64_t num_edges, int32_t* in_rowptr, int32_t* in_src, float* in_attr,
                     int32_t* out_rowptr, int32_t* out_dst, float* out_attr, int32_t* d_error,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Content check for the graph cache: *differ = 1 when edge_index_a [2, E] (int64, 16-byte
 * aligned) differs from edge_index_b or, if given, edge_attr_a [E] from edge_attr_b (bit
 * patterns); *differ is zeroed by the caller and otherwise left alone.  Lets a caller that
 * copies the same static graph to the device every step (train.py:62) reuse its CSRs and
 * window plans instead of rebuilding them.  differ may be mapped host memory: */
int gine_graph_same_edges(const int64_t* edge_index_a, const int64_t* edge_index_b,
                          const float* edge_attr_a, const float* edge_attr_b, int64_t num_edges,
                          int32_t* differ, void* stream);
/* gine_graph_build for edge_attr [E, K] (row-major, 1 <= K = edge_dim <= GINE_MP_MAX_EDGE_DIM,
 * GINE_ERR_INVALID otherwise; PyG GINEConv(edge_dim=K)): the same two stable sorts;
 * in_attr / out_attr are [E, K], row p holding the K attributes of the edge in CSR slot p, and
 * out_eid [E] (int32) is the position in the caller's edge list (= row of edge_attr) of the
 * edge in out-CSR slot p -- where gine_mp_bwd_ek stores that edge's attribute gradient.
 * Workspace: gine_graph_workspace_bytes.  edge_attr, in_attr, out_attr and out_eid are
 * required when num_edges > 0. */
int gine_graph_build_ek(const int64_t* edge_index, const float* edge_attr, int64_t num_nodes,
                        int64_t num_edges, int32_t edge_dim, int32_t* in_rowptr,
                        int32_t* in_src, float* in_attr, int32_t* out_rowptr, int32_t* out_dst,
                        float* out_attr, int32_t* out_eid, int32_t* d_error, void* workspace,
                        size_t workspace_bytes, void* stream);
/* gine_graph_same_edges over edge_attr [E, edge_dim]: all 4 * edge_dim * E attribute bytes
 * are compared (edge_attr 16-byte aligned, as there). */
int gine_graph_same_edges_ek(const int64_t* edge_index_a, const int64_t* edge_index_b,
                             const float* edge_attr_a, const float* edge_attr_b,
                             int64_t num_edges, int32_t edge_dim, int32_t* differ, void* stream);
/* the device address of pinned (page-locked) host memory (hipHostGetDevicePointer); an error
 * status when the memory is not mapped for the device. */
int gine_host_device_ptr(void* host_ptr, void** device_ptr);

/* ------------------------------------------------------------------------------------
 * Message passing forward.  Replaces GINEConv.forward up to (excluding) self.nn:
 *   m_e  = relu(x[src_e] + lin(a_e))                      (GINEConv.message, lin=Linear(1,D))
 *   agg_i = sum over in-edges of i, original edge order   (SumAggregation / scatter_add_)
 *   z_i  = agg_i + (1 + eps) * x_i                         (out + (1 + self.eps) * x_r)
 * Bit-identical to the CPU path (sequential per-destination order, no contraction).
 * The K=1 Linear's rounding is host-dependent in the reference itself: MKL's sgemm rounds
 * a*w+b once (fma) on Intel CPUs and twice (mul, then add) on AMD EPYC hosts, so the mode
 * is a flag: GINE_MP_LIN_MULADD selects mul-then-add, otherwise fma.
 *   x [N, D], lin_w [D] (Linear(1,D).weight flattened), lin_b [D], eps [1] (device), z [N, D]
 * Supported D: multiple of 4, 4 <= D <= 1024.
 * ---------------------------------------------------------------------------------- */
#define GINE_MP_LIN_MULADD 2
int gine_mp_fwd(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                const float* in_attr, const float* lin_w, const float* lin_b, const float* eps,
                float* z, int64_t num_nodes, int32_t channels, int32_t flags, void* stream);

/* ------------------------------------------------------------------------------------
 * Message passing backward (autograd of gine_mp_fwd), over the out-edge CSR:
 *   dm_e   = dz[dst_e] * 1[x[j] + lin(a_e) > 0]                    (gather + relu bwd)
 *   dx_j   = sum over out-edges of j in original order of dm_e   (index_add_, bit-exact)
 *            [+ (1 + eps) * dz_j  if flags & GINE_MP_BWD_SELF]
 *            [+ dres_j            if dres != NULL]
 *   partials[b] (fp64, a [3][D] row per block b): sum dm*a [D], sum dm [D], then the
 *            block's sum over channels of dz*x (one value; the rest of the row unused)
 *   flags may also carry GINE_MP_LIN_MULADD (must match the forward).
 * gine_mp_bwd_finalize reduces the partials in fixed block order into
 *   dlin_w [D], dlin_b [D], deps [1] (one launch).  Finalize calls may reduce IN PLACE:
 *   treat the partials buffer as consumed -- true of every *_finalize below too.
 * ---------------------------------------------------------------------------------- */
#define GINE_MP_BWD_SELF 1
int gine_mp_bwd_num_partials(int64_t num_nodes, int32_t channels, int32_t* num_partials);
int gine_mp_bwd(const float* dz, const float* x, const int32_t* out_rowptr,
                const int32_t* out_dst, const float* out_attr, const float* lin_w,
                const float* lin_b, const float* eps, const float* dres, float* dx,
                double* partials, int64_t num_nodes, int32_t channels, int32_t flags,
                void* stream);
int gine_mp_bwd_finalize(const double* partials, int32_t num_partials, int32_t channels,
                         float* dlin_w, float* dlin_b, float* deps, void* stream);
/* gine_mp_bwd plus, in the same launch, the fixed-order reduction of the node-MLP
 * weight-gradient slab that gine_mlp_bwd1_wgrad left when called with NULL dw1/db1/dw2/db2
 * (wg_chunks = gine_mlp_wgrad_num_chunks(num_nodes, mlp_channels)); writes dw1, db1, dw2,
 * db2 exactly as gine_mlp_wgrad would. */
int gine_mp_bwd_side(const float* dz, const float* x, const int32_t* out_rowptr,
                     const int32_t* out_dst, const float* out_attr, const float* lin_w,
                     const float* lin_b, const float* eps, const float* dres, float* dx,
                     double* partials, int64_t num_nodes, int32_t channels, int32_t flags,
                     const float* wg_slab, int32_t wg_chunks, int32_t mlp_channels, float* dw1,
                     float* db1, float* dw2, float* db2, void* stream);

/* ------------------------------------------------------------------------------------
 * Message passing with K = edge_dim attributes per edge, 1 <= K <= GINE_MP_MAX_EDGE_DIM
 * (PyG GINEConv(edge_dim=K): lin = Linear(K, D)), and the gradient of the attributes.  For an
 * edge e with attributes a_e[0..K-1], lin_w W [D, K] (lin.weight's layout) and lin_b b [D]:
 *   e_c = b_c;  for k = 0 .. K-1:  e_c = fma(a_e[k], W[c][k], e_c)   (one rounding per term, in
 *                                                                     this order)
 *   m_e = relu(x[src_e] + e)    z_i = sum over in-edges of i, original edge order, of m_e
 *                                     + (1 + eps) * x_i
 * At K = 1 this is gine_mp_fwd's fma mode, bit for bit; there is no rounding flag.  (A CPU
 * Linear(K, D) with K > 1 is an sgemm whose summation order is the BLAS's own: bit-identity
 * with torch's CPU result is not defined for K > 1.)  in_attr / out_attr [E, K] and out_eid
 * [E] as gine_graph_build_ek writes them.
 * Backward over the out-edge CSR, dm_e = (x[src_e] + e <= 0) ? 0 : dz[dst_e]:
 *   dx as gine_mp_bwd (flags: GINE_MP_BWD_SELF only; dres may be NULL)
 *   partials[b] (fp64, a row of (K + 2) * D per block b): sum dm*a_k [D*K, laid out [c][k]],
 *            sum dm [D], then the block's sum of dz*x (one value; the rest unused)
 *   dea != NULL: dea[out_eid[p] * K + k] = sum_c dm_e[c] * W[c][k] for the edge e in slot p
 *            (each lane's 4 channels in fp32, then a fixed butterfly over the row group;
 *            plain stores, every edge written once: no zero-fill needed).  NULL: not computed,
 *            and the launch is the instantiation without that code.
 * gine_mp_bwd_ek_finalize reduces the partials in fixed block order into dlin_w [D, K],
 * dlin_b [D], deps [1].
 * Supported D: multiple of 4, 4 <= D <= 256 (GINE_ERR_DIM); edge_dim outside 1..8:
 * GINE_ERR_INVALID; num_nodes * D * 4 and num_edges * K * 4 below 2^32 (GINE_ERR_TOO_LARGE);
 * num_nodes = 0: GINE_OK, nothing launched.  All checked before any HIP call.
 * ---------------------------------------------------------------------------------- */
#define GINE_MP_MAX_EDGE_DIM 8
int gine_mp_fwd_ek(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                   const float* in_attr, const float* lin_w, const float* lin_b,
                   const float* eps, float* z, int64_t num_nodes, int64_t num_edges,
                   int32_t channels, int32_t edge_dim, void* stream);
int gine_mp_bwd_ek_num_partials(int64_t num_nodes, int32_t channels, int32_t edge_dim,
                                int32_t* num_partials);
int gine_mp_bwd_ek(const float* dz, const float* x, const int32_t* out_rowptr,
                   const int32_t* out_dst, const float* out_attr, const int32_t* out_eid,
                   const float* lin_w, const float* lin_b, const float* eps, const float* dres,
                   float* dx, float* dea, double* partials, int64_t num_nodes,
                   int64_t num_edges, int32_t channels, int32_t edge_dim, int32_t flags,
                   void* stream);
int gine_mp_bwd_ek_finalize(const double* partials, int32_t num_partials, int32_t channels,
                            int32_t edge_dim, float* dlin_w, float* dlin_b, float* deps,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * Window-staged message passing (same results as gine_mp_fwd / gine_mp_bwd, bit for bit
 * for z and dx).  A PyG batch is a block-diagonal union of graphs (Batch.from_data_list,
 * train.py:155), so the neighbours of a run of consecutive nodes lie in one short run of
 * rows.  gine_graph_plan_windows (HOST pointers: a host copy of a CSR) cuts the nodes into
 * tiles of at most max_nodes nodes / max_edges edges whose neighbour window
 * [win_lo, win_lo + win_rows) spans at most max_rows rows; maxima[3] = the largest window
 * rows, tile edges and tile nodes.  *num_tiles = 0 means no plan (some node's own neighbour
 * span exceeds max_rows or its degree max_edges): use the gather entry points.
 * The kernels stage each tile's window slice of slice_channels (8, 16 or 32) channels in
 * LDS and read every neighbour row from there; channels % slice_channels == 0 and
 * channels / slice_channels <= 8.  The plan arrays are device copies.
 * gine_mp_bwd_win partials: num_tiles rows of fp64 [3][D]; gine_mp_bwd_win_finalize
 * reduces them (fixed order) into dlin_w, dlin_b, deps.
 * Replaces the same reference ops as gine_mp_fwd / gine_mp_bwd (models/gnn.py:41,44).
 * ---------------------------------------------------------------------------------- */
#define GINE_WINDOW_LDS_BYTES (80 * 1024)  /* two workgroups per CU (160 KiB LDS) */
typedef struct gine_window_plan {
  const int32_t* tile_begin; /* device [num_tiles + 1] */
  const int32_t* win_lo;     /* device [num_tiles] */
  const int32_t* win_rows;   /* device [num_tiles] */
  int32_t num_tiles;
  int32_t slice_channels;
  int32_t max_rows, max_edges, max_nodes;
  const int16_t* slot;       /* device [num_nodes] or NULL: gine_graph_plan_window_slots */
  const int32_t* edge_begin; /* device [num_tiles + 1] or NULL: rowptr[tile_begin[t]] */
} gine_window_plan;
int gine_graph_plan_windows(const int32_t* rowptr, const int32_t* nbr, int64_t num_nodes,
                            int32_t max_rows, int32_t max_nodes, int32_t max_edges,
                            int32_t* tile_begin, int32_t* win_lo, int32_t* win_rows,
                            int32_t* num_tiles, int32_t* maxima);
/* Work order inside the tiles of a backward (out-CSR) window plan (HOST pointers):
 * slot[tile_begin[t] + s] = the tile-local node a workgroup processes at position s.  A
 * lane group takes positions g and g + 64 one after the other; the order pairs each tile's
 * nodes by out-degree (heaviest with lightest, ties by index), so the groups of a wave run
 * chains of similar length.  Per-node results are unchanged (each node's edges are still
 * summed in their own order). */
int gine_graph_plan_window_slots(const int32_t* rowptr, const int32_t* tile_begin,
                                 int32_t num_tiles, int16_t* slot);
/* Locality order of a graph's nodes (HOST pointers: a host copy of a CSR, either
 * direction; the adjacency is symmetrised).  order[i] = the node placed at position i:
 * reverse Cuthill-McKee, deterministic.  Relabelling a static station graph this way before
 * batching (raincast_gnn.data.relabel_stations) narrows every tile's neighbour window (the
 * reference's dataset order, utils/data.py:261-284, scatters k-NN neighbours over the whole
 * graph).  Per-node results are unchanged: each node keeps its in/out edges in their
 * original relative order. */
int gine_graph_order_locality(const int32_t* rowptr, const int32_t* nbr, int64_t num_nodes,
                              int32_t* order);
int gine_mp_fwd_win(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                    const float* in_attr, const float* lin_w, const float* lin_b,
                    const float* eps, float* z, int64_t num_nodes, int32_t channels,
                    int32_t flags, const gine_window_plan* plan, void* stream);
int gine_mp_bwd_win(const float* dz, const float* x, const int32_t* out_rowptr,
                    const int32_t* out_dst, const float* out_attr, const float* lin_w,
                    const float* lin_b, const float* eps, const float* dres, float* dx,
                    double* partials, int64_t num_nodes, int32_t channels, int32_t flags,
                    const gine_window_plan* plan, void* stream);
int gine_mp_bwd_win_side(const float* dz, const float* x, const int32_t* out_rowptr,
                         const int32_t* out_dst, const float* out_attr, const float* lin_w,
                         const float* lin_b, const float* eps, const float* dres, float* dx,
                         double* partials, int64_t num_nodes, int32_t channels, int32_t flags,
                         const gine_window_plan* plan, const float* wg_slab, int32_t wg_chunks,
                         int32_t mlp_channels, float* dw1, float* db1, float* dw2, float* db2,
                         void* stream);
/* gine_mp_bwd_win + the node-MLP weight-gradient engine of the same GINE layer in ONE launch
 * (D = 64 or 128, slice_channels = 32): extra workgroups write the fp32 slab
 * [2][gine_mlp_wgrad_num_chunks][D*D + D] exactly as gine_mlp_wgrad does with NULL outputs
 * (operands dy, y, mask, a1, bn_save, dbn, coef, z, epilogue as for gine_mlp_wgrad), while
 * the window workgroups run the message-passing backward; the slab is then reduced by
 * gine_grad_finalize_batch.  Replaces the same reference ops as gine_mp_bwd and
 * gine_mlp_wgrad (models/gnn.py:21-26,41,44 autograd).  GINE_ERR_INVALID when the plan's
 * slice is not 32 channels. */
int gine_mp_bwd_win_mlp_wgrad(const float* dz, const float* x, const int32_t* out_rowptr,
                              const int32_t* out_dst, const float* out_attr,
                              const float* lin_w, const float* lin_b, const float* eps,
                              const float* dres, float* dx, double* partials,
                              int64_t num_nodes, int32_t channels, int32_t flags,
                              const gine_window_plan* plan, const float* dy, const float* y,
                              const uint8_t* mask, const float* a1, const float* bn_save,
                              const float* dbn, const float* coef, const float* z, float* slab,
                              int32_t epilogue, void* stream);
int gine_mp_bwd_win_finalize(const double* partials, int32_t num_tiles, int32_t channels,
                             int32_t slice_channels, float* dlin_w, float* dlin_b,
                             float* deps, void* stream);

/* ------------------------------------------------------------------------------------
 * Batched gradient finish.  The parameter-gradient reductions that nothing reads before
 * the optimizer -- dW_e/db_e/eps of every GINE layer (gine_mp_bwd*_finalize), the head's
 * and the dense chain's weight-gradient slabs, the DeepSet dW1 slab -- in ONE launch at the
 * end of the backward instead of one launch each (autograd of the Linear/GINEConv
 * parameters, models/gnn.py; reduced by the reference's autograd as separate mm/sum ops).
 *   GINE_GRAD_JOB_MP:   src = fp64 partial rows [rows][3*channels] as gine_mp_bwd (eps at
 *                       column 2D, eps_cols = 1) or gine_mp_bwd_win (eps at 2D + slice,
 *                       eps_cols = slices) write them; w[0] = dlin_w [D], w[1] = dlin_b
 *                       [D], w[2] = deps [1].
 *   GINE_GRAD_JOB_SLAB: src = fp32 slab, element e of product z < nz at
 *                       src + z*zstride + c*cstride + e for chunks c < rows; product z has
 *                       per[z] elements: e < wsize[z] -> w[z][e], else b[z][e - wsize[z]]
 *                       (times bscale[z]).  Sums in fp64, fixed order.
 * The *_grad_job entry points (host only) describe the slab a producer left when called
 * with NULL gradient outputs.  At most GINE_GRAD_MAX_JOBS jobs per launch.
 * ---------------------------------------------------------------------------------- */
#define GINE_GRAD_JOB_MP 1
#define GINE_GRAD_JOB_SLAB 2
#define GINE_GRAD_MAX_JOBS 12
typedef struct gine_grad_job {
  int32_t kind;
  int32_t rows;      /* MP: partial rows; SLAB: chunks */
  int32_t channels;  /* MP: D */
  int32_t eps_cols;  /* MP: eps columns */
  int32_t nz;        /* SLAB: products (<= 4) */
  int32_t pad_;
  const void* src;
  int64_t cstride, zstride;  /* SLAB, in floats */
  int64_t per[4];
  int64_t wsize[4];
  float bscale[4];
  float* w[4];
  float* b[4];
} gine_grad_job;
int gine_grad_finalize_batch(const gine_grad_job* jobs, int32_t num_jobs, void* stream);
int gine_head_bwd_grad_job(int64_t num_nodes, int32_t channels, int32_t kind, const float* slab,
                           float* dw, float* db, gine_grad_job* job);
int gine_chain_wgrad_grad_job(int64_t num_nodes, int32_t hidden, int32_t in_features,
                              const float* slab, float bias_scale, float* dwp2, float* dbp2,
                              float* dwr0, float* dbr0, float* dwr1, float* dbr1, float* dwdr,
                              float* dbdr, gine_grad_job* job);
int gine_deepset_bwd_grad_job(int64_t num_nodes, int32_t in_features, int32_t hidden,
                              const float* slab, float* dw1, float* db1, gine_grad_job* job);

/* ------------------------------------------------------------------------------------
 * Node MLP  nn = Sequential(Linear(D,D), BatchNorm1d(D), ReLU(), Linear(D,D))
 * (models/gnn.py:21-26), plus the ResGnn epilogue (models/gnn.py:38-44).
 * fp32 MFMA (v_mfma_f32_32x32x2_f32) row-tile GEMMs with fused prologues/epilogues.
 * Supported D: 32, 64, 128, 256.
 *
 * Forward, training mode:
 *   gine_mlp_fwd1:      a1 = z W1^T + b1; per-block fp64 partial sums of a1 and a1^2
 *   gine_bn_fwd_finalize: mean, biased var -> invstd; running stats update
 *                       (momentum, unbiased var); bn_save = [mean | invstd | alpha | shift]
 *                       with alpha = gamma*invstd, shift = beta - mean*alpha
 *                       (eval mode: from running stats, partials unused)
 *   gine_mlp_fwd2:      r = relu(a1*alpha + shift); o = r W2^T + b2;
 *                       y = o | relu(o) | x + relu(o)   (epilogue 0 | 1 | 2)
 *                       mask[n,c] = (o > 0) stored as uint8 for epilogue 2 (may be NULL else)
 * Backward:
 *   gine_mlp_bwd2:      do = dy*1[o>0] (per epilogue); dr = do W2; dbn = dr*1[bn>0];
 *                       partials of sum dbn, sum dbn*xhat
 *   gine_bn_bwd_finalize: dgamma, dbeta, and coef = [c1 | c2 | c3] with
 *                       da1 = c1*dbn + c2*xhat + c3
 *   gine_mlp_bwd1:      dz = da1 W1
 *   gine_mlp_wgrad:     dW2 = do^T r, db2 = sum do, dW1 = da1^T z, db1 = sum da1
 *                       (split over row chunks; fp32 partial slabs reduced in fixed order)
 * ---------------------------------------------------------------------------------- */
#define GINE_EPI_NONE 0
#define GINE_EPI_RELU 1
#define GINE_EPI_RESIDUAL_RELU 2

int gine_mlp_num_partials(int64_t num_nodes, int32_t channels, int32_t* num_partials);
int gine_mlp_fwd1(const float* z, const float* w1, const float* b1, float* a1, double* partials,
                  int64_t num_nodes, int32_t channels, void* stream);
int gine_bn_fwd_finalize(const double* partials, int32_t num_partials, const float* gamma,
                         const float* beta, float* running_mean, float* running_var,
                         int64_t* num_batches_tracked, float* bn_save, int64_t num_nodes,
                         int32_t channels, float momentum, float bn_eps, int32_t training,
                         int32_t update_running, void* stream);
int gine_mlp_fwd2(const float* a1, const float* bn_save, const float* w2, const float* b2,
                  const float* x, float* y, uint8_t* mask, int64_t num_nodes, int32_t channels,
                  int32_t epilogue, void* stream);

/* Fused forward message passing + first Linear (D = 128 only): z exactly as gine_mp_fwd and
 * a1 / partials exactly as gine_mlp_fwd1 (bit-identical; partials has gine_mlp_num_partials
 * rows), in one launch whose workgroups gather the next 32-row tile of z while the matrix
 * cores multiply the current one (csrc/gine_mpmlp.hip).  Requires every in-degree <=
 * GINE_MP_FUSED_MAX_DEGREE: the caller passes the graph's maximum in-degree and gets
 * GINE_ERR_INVALID above it (-> the unfused pair); GINE_ERR_DIM for channels != 128.
 * flags: GINE_MP_LIN_MULADD as for gine_mp_fwd.
 * Replaces models/gnn.py:41,44 (GINEConv.propagate + nn[0] Linear + BN batch statistics). */
#define GINE_MP_FUSED_MAX_DEGREE 32
int gine_mp_fwd_mlp1(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                     const float* in_attr, const float* lin_w, const float* lin_b,
                     const float* eps, const float* w1, const float* b1, float* z, float* a1,
                     double* partials, int64_t num_nodes, int32_t channels,
                     int32_t max_in_degree, int32_t flags, void* stream);

/* BatchNorm statistics without a finish launch (training, momentum >= 0; csrc/gine_bnacc.hpp).
 * bn_acc: int64[gine_bn_acc_words(D)] (query it: the size follows the build-time replica count
 * R = GINE_BNACC_REPLICAS, (3R + 1 + 8) * 2D + 3 + 288 words, the 288 being the one-launch
 * layer's grid barrier: 18 lines of 16 words), zeroed once by the caller at allocation,
 * then owned by the kernels (the sums only grow; each consumer differences them against a
 * snapshot the previous consumer left), so one buffer serves every step of one BatchNorm,
 * HIP-graph replays included.  Every producer launch must be followed by exactly one
 * gine_mlp_fwd2_bn on the same buffer; not shared by layers whose launches interleave.  A
 * consumer that finds the pairing broken (the producer's phase moved by more than one since
 * the last consumer) emits NaN statistics for that step; re-zero the buffer to recover.
 *   gine_mlp_fwd1_acc / gine_mp_fwd_mlp1_acc: as gine_mlp_fwd1 / gine_mp_fwd_mlp1, and the
 *     per-workgroup sums are also added into bn_acc as 3-word fixed point (2^0 / 2^-32 /
 *     2^-64) with integer atomics (order-independent: same bits every run); NaN / +Inf /
 *     -Inf workgroup sums are counted instead and give NaN / +Inf / -Inf column sums, as
 *     ATen's do.  partials may be NULL.
 *   gine_mlp_fwd2_bn: gine_bn_fwd_finalize (from bn_acc) + gine_mlp_fwd2 in one launch;
 *     writes bn_save, the running statistics and num_batches_tracked as the finalize does.
 * Each workgroup sum is rounded to 2^-64, absolutely: with G workgroups the mean is within
 * G 2^-65 / N of the partials path's and bn_save can differ from it in the last fp32 bit
 * (~1e-15 relative for activations of order 1).  A column whose sums are themselves of order
 * 2^-64 (|a1| ~ 1e-20 and below) loses them: measured on the 1e-30 column of
 * tests/test_gpu_bn_stats.py, mean = 0 here against 5e-8 relative on the partials path, both
 * inside the bounds of tests/bn_cases.py. */
int gine_bn_acc_words(int32_t channels, int64_t* words);
/* Index (int64 words into bn_acc) of the grid-barrier failure count: gine_mp_fwd_layer adds 1
 * there for every workgroup whose grid barrier timed out (~2 s: the grid was not resident at
 * once -- other work held CUs).  Such a launch's outputs are NaN in those workgroups' rows,
 * bn_save is NaN if workgroup 0 failed, and the running statistics are left as they were.
 * The caller reads the word at its synchronisation points and raises on a non-zero value;
 * re-zero the buffer afterwards (raincast_gnn.functional.check_grid_barriers). */
int gine_bn_acc_barrier_failures_index(int32_t channels, int64_t* index);
/* Backward, same scheme (a second accumulator per BatchNorm): gine_mlp_bwd2_acc = gine_mlp_bwd2
 * with the [sum dbn | sum dbn*xhat] sums into bn_acc (partials may be NULL);
 * gine_mlp_bwd1_bn = gine_bn_bwd_finalize (training) + gine_mlp_bwd1 in one launch (writes
 * coef, dgamma, dbeta; dgamma / dbeta may be NULL). */
int gine_mlp_bwd2_acc(const float* dy, const float* y, const uint8_t* mask, const float* a1,
                      const float* bn_save, const float* w2, float* dbn, double* partials,
                      int64_t* bn_acc, int64_t num_nodes, int32_t channels, int32_t epilogue,
                      void* stream);
int gine_mlp_bwd1_bn(const float* dbn, const float* a1, const float* bn_save, int64_t* bn_acc,
                     const float* gamma, float* dgamma, float* dbeta, float* coef,
                     const float* w1, float* dz, int64_t num_nodes, int32_t channels,
                     void* stream);
/* The backward pair in ONE launch (csrc/gine_mlpbwd.hip k_mlp_bwd_layer; replaces
 * gine_mlp_bwd2_acc followed by gine_mlp_bwd1_bn, models/gnn.py:21-26 autograd): phase A =
 * dbn and the BatchNorm-backward sums, grid barrier, phase B = coef (workgroup 0 also writes
 * coef, dgamma, dbeta) and dz = da1 W1 -- both row tiles of a workgroup stay in LDS, W1 is
 * loaded under phase A.  Same outputs, bit for bit, as the pair (dbn, dz, coef, dgamma,
 * dbeta) and the same pairing protocol on bn_acc (the backward accumulator); a barrier that
 * cannot complete is counted at gine_bn_acc_barrier_failures_index and makes that launch's
 * coef / dz NaN.  Applies where gine_mlp_bwd_layer_ok says so: channels = 128, at most 2
 * row tiles per workgroup and the whole grid resident at once (occupancy query, cached per
 * device); GINE_ERR_INVALID otherwise.  gamma, dgamma, dbeta may be NULL; y (GINE_EPI_RELU)
 * and mask (GINE_EPI_RESIDUAL_RELU) as for gine_mlp_bwd2. */
int gine_mlp_bwd_layer_ok(int64_t num_nodes, int32_t channels, int32_t* ok);
int gine_mlp_bwd_layer(const float* dy, const float* y, const uint8_t* mask, const float* a1,
                       const float* bn_save, const float* w2, float* dbn, int64_t* bn_acc,
                       const float* gamma, float* dgamma, float* dbeta, float* coef,
                       const float* w1, float* dz, int64_t num_nodes, int32_t channels,
                       int32_t epilogue, void* stream);
/* Testing only: `extra` workgroups added to every later gine_mlp_bwd_layer grid (0 restores
 * production), for the barrier-failure test. */
int gine_testing_bwd_layer_extra_workgroups(int32_t extra);
int gine_mlp_fwd1_acc(const float* z, const float* w1, const float* b1, float* a1,
                      double* partials, int64_t* bn_acc, int64_t num_nodes, int32_t channels,
                      void* stream);
int gine_mp_fwd_mlp1_acc(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                         const float* in_attr, const float* lin_w, const float* lin_b,
                         const float* eps, const float* w1, const float* b1, float* z,
                         float* a1, double* partials, int64_t* bn_acc, int64_t num_nodes,
                         int32_t channels, int32_t max_in_degree, int32_t flags, void* stream);
/* The whole node-MLP forward of a GINE layer in ONE launch (models/gnn.py:41-44: propagate +
 * nn + ResGnn's ReLU / residual): gine_mp_fwd_mlp1_acc and gine_mlp_fwd2_bn on the same
 * workgroups, separated by a grid barrier (csrc/gine_mpmlp.hip k_mp_fwd_layer) -- every a1
 * tile stays in LDS between the halves, W2 is staged under the barrier's wait.  Same
 * outputs, bit for bit, as the pair (z, a1, bn_save, running statistics, y, mask), same
 * pairing protocol on bn_acc (the barrier words at its end, gine_bn_acc_words; a barrier that
 * cannot complete is counted there, gine_bn_acc_barrier_failures_index).
 * Applies where gine_mp_fwd_layer_ok says so: channels = 128, max_in_degree <=
 * GINE_MP_FUSED_MAX_DEGREE, at most 2 row tiles per workgroup and the whole grid resident
 * on the device at once (occupancy query, cached per device); GINE_ERR_INVALID otherwise. */
int gine_mp_fwd_layer_ok(int64_t num_nodes, int32_t channels, int32_t max_in_degree, int32_t* ok);
/* Testing only: `extra` workgroups added to every later gine_mp_fwd_layer grid (0 restores
 * production), so a test can launch a grid the device cannot hold at once and check that the
 * barrier's failure reaches the host (gine_bn_acc_barrier_failures_index). */
int gine_testing_layer_extra_workgroups(int32_t extra);
/* Testing only: the output head's 32-lane butterfly sum (csrc/gine_headrow.hpp sum_32; mode 1)
 * against the __shfl_xor butterfly it stands for (mode 0), on `waves` x 64 floats. */
int gine_testing_sum_32(const float* in, float* out, int32_t waves, int32_t mode, void* stream);
/* With a layer window plan (tile_windows != NULL; ABI 7) every workgroup stages each of its
 * 32-row tiles' neighbour rows -- the tile's window, one contiguous run of rows -- in LDS once
 * and sums the messages from there (per-destination LDS staging; same bits as the gather);
 * window_rows is the plan's largest window and (window_rows, max_in_degree) must pass
 * gine_mp_fwd_layer_windows_fit (GINE_ERR_INVALID otherwise).  NULL: neighbour rows are
 * gathered from L2 (any graph). */
/* The output head folded into the last layer's launch (ABI 8; models/gnn.py:140-141,
 * GNN.aggr + PostProcess): with head != NULL the epilogue also evaluates gine_head_fwd on the
 * rows it writes -- raw = y W^T + b, pred = PostProcess(raw) -- with the same lane layout,
 * fma order and butterfly as k_head_fwd (same bits), and, with y_target != NULL, the loss's
 * GINE_COUNT_PARTS valid-target partial counts (gine_head_fwd_count).  One launch fewer
 * and h is not read back.  kind: GINE_LOSS_* (K = 2..5 outputs per node). */
typedef struct gine_layer_head {
  const float* weight;    /* [K, 128] (GNN.aggr.weight) */
  const float* bias;      /* [K] */
  float* raw;             /* [N, K] pre-PostProcess output (what gine_head_bwd reads) */
  float* pred;            /* [N, K] */
  const float* y_target;  /* [N] batch targets, or NULL */
  uint32_t* count_parts;  /* GINE_COUNT_PARTS partial counts (with y_target), or NULL */
  int32_t kind;           /* GINE_LOSS_* */
} gine_layer_head;
int gine_mp_fwd_layer(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                      const float* in_attr, const float* lin_w, const float* lin_b,
                      const float* eps, const float* w1, const float* b1, float* z, float* a1,
                      int64_t* bn_acc, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked,
                      float* bn_save, float momentum, float bn_eps, int32_t update_running,
                      const float* w2, const float* b2, float* y, uint8_t* mask,
                      int64_t num_nodes, int32_t channels, int32_t max_in_degree, int32_t flags,
                      int32_t epilogue, const int32_t* tile_windows, int32_t window_rows,
                      const gine_layer_head* head, void* stream);
/* The layer forward in EVAL mode in ONE launch (ABI 10; eval.py:57-69 model.eval() forward of
 * models/gnn.py:41-44): BatchNorm from the running statistics is a per-channel affine map
 * known before the launch (alpha = gamma * invstd(running_var, bn_eps), shift = beta -
 * running_mean * alpha, the eval branch of gine_bn_fwd_finalize), so no tile depends on
 * another -- no statistics, no bn_acc, no grid barrier, hence no residency requirement, no
 * size limit beyond num_nodes * 512 < 2^32 (GINE_ERR_TOO_LARGE) and no failure word.
 * Replaces gine_mp_fwd_mlp1 + gine_bn_fwd_finalize + gine_mlp_fwd2 (+ gine_head_fwd[_count]
 * with head != NULL) with the same bits in y, raw, pred and count_parts.  Nothing else is
 * written: no z, a1, mask, bn_save, partials or running statistics.  With a head, y may be
 * NULL (predictions only).  gamma / beta may be NULL.
 * Any num_nodes >= 1 (0: GINE_OK, nothing launched); channels = 128 (GINE_ERR_DIM);
 * max_in_degree <= GINE_MP_FUSED_MAX_DEGREE, flags (GINE_MP_LIN_MULADD) and epilogue as for
 * gine_mp_fwd_layer (GINE_ERR_INVALID).  A workgroup walks its 32-row tiles in rounds of two,
 * so the grid is free: max_workgroups caps it (0: one workgroup per tile up to one per CU). */
int gine_mp_fwd_layer_eval(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                           const float* in_attr, const float* lin_w, const float* lin_b,
                           const float* eps, const float* w1, const float* b1,
                           const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, float bn_eps, const float* w2,
                           const float* b2, float* y, int64_t num_nodes, int32_t channels,
                           int32_t max_in_degree, int32_t flags, int32_t epilogue,
                           const gine_layer_head* head, int32_t max_workgroups, void* stream);
/* gine_mp_fwd_layer_eval at ANY in-degree (additive in ABI 10; the reference's radius graphs,
 * utils/data.py:261-284, and k = 32 plus the self loop are past GINE_MP_FUSED_MAX_DEGREE): the
 * same launch, arguments, validation and outputs, except that max_in_degree only has to be
 * >= 0 -- the kernel takes every row's length from in_rowptr and walks its edge list in chunks
 * of 32 slots (csrc/gine_mpeval.hip gather_role_deep), a row's sum being the same sequence of
 * additions in edge order.  y, raw, pred and count_parts have the bits of the separate eval
 * launches at every degree, and of gine_mp_fwd_layer_eval where that applies.  Same LDS, grid
 * policy and max_workgroups.  Inference only: the training forms keep the degree limit. */
int gine_mp_fwd_layer_eval_deep(const float* x, const int32_t* in_rowptr, const int32_t* in_src,
                                const float* in_attr, const float* lin_w, const float* lin_b,
                                const float* eps, const float* w1, const float* b1,
                                const float* gamma, const float* beta,
                                const float* running_mean, const float* running_var,
                                float bn_eps, const float* w2, const float* b2, float* y,
                                int64_t num_nodes, int32_t channels, int32_t max_in_degree,
                                int32_t flags, int32_t epilogue, const gine_layer_head* head,
                                int32_t max_workgroups, void* stream);
/* The layer window plan of a graph (built once per graph, like its CSRs): for every 32-row
 * tile of destinations, tile_windows[2T] = first row and tile_windows[2T + 1] = number of rows
 * of the run [lo, lo + rows) holding the tile's own rows and all their in-neighbours (int32
 * [ceil(N / 32)][2], device), and maxima[0] / maxima[1] = the largest window and the largest
 * number of in-edges of a tile (int32[2], device; zeroed by the call).  The caller reads the
 * maxima back once and asks gine_mp_fwd_layer_windows_fit (largest window, the graph's largest
 * in-degree) whether the plan fits the launch's LDS: (rows + 1) x 512 B of window rows (a -inf
 * dummy row last), 32 x round_up(max_in_degree, 4) x 8 B of padded slot table and 33 rowptr
 * words within 73,712 B, rows <= 144 (cfg2's 500-station k = 10 graphs in the locality order:
 * about 129 rows, in-degree 11).
 * Replaces nothing in the reference: the data movement of PyG's x.index_select per tile. */
int gine_graph_plan_layer_windows(const int32_t* in_rowptr, const int32_t* in_src,
                                  int64_t num_nodes, int32_t* tile_windows, int32_t* maxima,
                                  void* stream);
int gine_mp_fwd_layer_windows_fit(int32_t window_rows, int32_t max_in_degree, int32_t* ok);
int gine_mlp_fwd2_bn(const float* a1, int64_t* bn_acc, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     float* bn_save, float momentum, float bn_eps, int32_t update_running,
                     const float* w2, const float* b2, const float* x, float* y,
                     uint8_t* mask, int64_t num_nodes, int32_t channels, int32_t epilogue,
                     void* stream);

int gine_mlp_bwd2(const float* dy, const float* y, const uint8_t* mask, const float* a1,
                  const float* bn_save, const float* w2, float* dbn, double* partials,
                  int64_t num_nodes, int32_t channels, int32_t epilogue, void* stream);
int gine_bn_bwd_finalize(const double* partials, int32_t num_partials, const float* gamma,
                         const float* bn_save, float* dgamma, float* dbeta, float* coef,
                         int64_t num_nodes, int32_t channels, int32_t training, void* stream);
int gine_mlp_bwd1(const float* dbn, const float* a1, const float* bn_save, const float* coef,
                  const float* w1, float* dz, int64_t num_nodes, int32_t channels,
                  void* stream);
int gine_mlp_wgrad_num_chunks(int64_t num_nodes, int32_t channels, int32_t* num_chunks);
/* dw1, db1, dw2, db2 all NULL: only the fp32 slab [2][chunks][D*D + D] is written (for a
 * batched reduction, gine_grad_finalize_batch). */
int gine_mlp_wgrad(const float* dy, const float* y, const uint8_t* mask, const float* a1,
                   const float* bn_save, const float* dbn, const float* coef, const float* z,
                   float* slab, float* dw1, float* db1, float* dw2, float* db2,
                   int64_t num_nodes, int32_t channels, int32_t epilogue, void* stream);

/* gine_mlp_bwd1 + gine_mlp_wgrad in one launch (same arguments as the two; the weight
 * gradients and dz are computed side by side on the CUs).  Same results bit for bit. */
int gine_mlp_bwd1_wgrad(const float* dy, const float* y, const uint8_t* mask, const float* a1,
                        const float* bn_save, const float* dbn, const float* coef,
                        const float* z, const float* w1, float* dz, float* slab, float* dw1,
                        float* db1, float* dw2, float* db2, int64_t num_nodes,
                        int32_t channels, int32_t epilogue, void* stream);

/* ------------------------------------------------------------------------------------
 * AdamW over one flat fp32 parameter buffer (the optimizer of the benchmarked training
 * step, train.py:67-69 with torch.optim.AdamW, lr from params.json).  Bumps the device
 * step counter `step` (fp32 [288]: the count, a ticket word, and at floats 32 + 32 g
 * (g < 8) the sub-tickets of a two-level ticket, one per 128-byte line; every ticket word
 * must start at 0 and is left at 0) and updates param / exp_avg / exp_avg_sq in place with torch.optim.AdamW's
 * default (amsgrad=False) formulation.  One launch, graph-safe; the four buffers must be
 * 16-byte aligned (float4 accesses).  Every scalar is formed from the fp32 arguments
 * (1.0f - beta in fp32, the bias corrections in double from the fp32 betas; gine_optim.hip's
 * header and DESIGN.md 6d give the exact sequence), not from torch's Python doubles: at the
 * defaults exp_avg_sq is 1.29e-5 relative below torch's, exp_avg's weight 2.2e-7 above.  The
 * count is fp32 and stays at 2^24 once it is there (the update is still applied).
 * ---------------------------------------------------------------------------------- */
int gine_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    float* step, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, void* stream);
/* Length in floats of gine_adamw_step's `step` buffer (288 since ABI 2). */
int gine_adamw_state_floats(int64_t* floats);

/* ------------------------------------------------------------------------------------
 * The AdamW step under a device control block: learning-rate schedule, clipping by the
 * global gradient norm (torch.nn.utils.clip_grad_norm_) and skipping of a step whose
 * gradient is not finite.  Every decision is taken on the device from device-resident words,
 * so a captured step follows a changed rate, bound or schedule on its next replay.
 *
 * gine_adamw_ctl (device memory, 4-byte fields, read by every launch, never written):
 *   lr             base learning rate
 *   max_norm       clipping bound; <= 0 or +inf: no clipping (the coefficient is exactly 1)
 *   schedule       GINE_LR_CONSTANT, GINE_LR_COSINE or GINE_LR_LINEAR (both with warm-up)
 *   warmup_steps   W, total_steps T, min_lr_ratio r.  With t = step count + 1 (1-based), in
 *                  double, rounded once to float:
 *                    constant            lr_t = lr
 *                    t <= W              lr_t = lr * t / W
 *                    otherwise, s = min(1, (t - W) / max(1, T - W)):
 *                    cosine              lr_t = lr * (r + (1 - r) * 0.5 * (1 + cos(pi s)))
 *                    linear              lr_t = lr * (r + (1 - r) * (1 - s))
 *   skip_nonfinite non-zero: a step whose gradient holds an inf or a NaN (or whose norm
 *                  overflows) writes nothing to param, exp_avg, exp_avg_sq or the step count
 * gine_adamw_report (device memory, written by the launch's last workgroup beside its
 * step-count store): lr_t, total_norm and clip_coef of the last launch; skipped = number of
 * skipped steps, accumulated (the caller zeroes it once).
 *
 * gine_grad_sumsq: partials [num_partials][2] fp64, row b = {sum of g*g, number of
 * non-finite g} over workgroup b's elements of grad [n] (16-byte aligned, like partials).
 * One pass, fp64 accumulation in a fixed order that depends on n alone, plain stores: no
 * atomics, no ticket, nothing to zero; the same input gives the same bits.  num_partials
 * must be gine_grad_sumsq_num_partials(n) (a function of n only, at most 512; 0 for n = 0,
 * when nothing is launched).
 * gine_adamw_step_ctl: gine_adamw_step's update (same buffers, same `step` state and
 * ticket, one launch) with lr_t from ctl and g' = g * clip_coef (one fp32 rounding; g' = g
 * bit for bit when the coefficient is 1), where every workgroup sums the partials in index
 * order in fp64, total_norm = (float)sqrt(sum) and
 * clip_coef = min(1, max_norm / (total_norm + 1e-6f)) in fp32.  partials = NULL with
 * num_partials = 0: no clipping and no non-finite test (total_norm reported as 0); then
 * the step is this one launch.  Otherwise gine_grad_sumsq of the same grad and n must
 * precede it on the stream.  ctl and report 4-byte aligned.
 * gine_adamw_ctl_bytes: sizeof the two structs, for callers that allocate them as bytes.
 * ---------------------------------------------------------------------------------- */
#define GINE_LR_CONSTANT 0
#define GINE_LR_COSINE 1
#define GINE_LR_LINEAR 2
typedef struct gine_adamw_ctl {
  float lr;
  float max_norm;
  int32_t schedule;
  float warmup_steps;
  float total_steps;
  float min_lr_ratio;
  int32_t skip_nonfinite;
} gine_adamw_ctl;
typedef struct gine_adamw_report {
  float lr_t;
  float total_norm;
  float clip_coef;
  uint32_t skipped;
} gine_adamw_report;
int gine_grad_sumsq_num_partials(int64_t n, int32_t* num_partials);
int gine_grad_sumsq(const float* grad, int64_t n, double* partials, int32_t num_partials,
                    void* stream);
int gine_adamw_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        float* step, int64_t n, const gine_adamw_ctl* ctl,
                        const double* partials, int32_t num_partials,
                        gine_adamw_report* report, float beta1, float beta2, float eps,
                        float weight_decay, void* stream);
int gine_adamw_ctl_bytes(int64_t* ctl_bytes, int64_t* report_bytes);

/* ------------------------------------------------------------------------------------
 * Fused CRPS losses (models/loss.py) over the post-processed predictions pred [N, K]
 * (models/model_utils.py PostProcess output) and targets y [N] (NaN = missing):
 *   GINE_LOSS_NORMAL        NormalCRPS.crps         (loss.py:335-369)   K = 2
 *   GINE_LOSS_MIXED_NORMAL  MixedNormalCRPS.crps    (loss.py:6-68)      K = 3
 *   GINE_LOSS_MIXED         MixedLoss(grad_u=False) (loss.py:71-272)    K = 4, u fixed
 *   GINE_LOSS_MIXED_U       MixedLoss(grad_u=True)                      K = 5, u learned
 * gine_crps_fwd: per node the closed form and its exact gradient w.r.t. pred (fp64
 * forward-mode duals) into dpred [N, K]; per-block partials [P][2]; loss_out[0] = mean over
 * non-NaN targets, count_out[0] = their number, written by the workgroup that finishes
 * last (ticket: a device uint32 the caller zeroes ONCE; every call leaves it at 0 again;
 * calls sharing a ticket must not overlap).  c = censoring point (log 0.01), t = sigmoid
 * temperature of grad_u, xi = GPD shape, u = fixed threshold.
 * gine_crps_bwd: grad_pred = gloss[0] * dpred / count (fp32).
 * gine_count_valid: the number of non-NaN y as GINE_COUNT_PARTS uint32 partial counts
 * (count_parts; their sum is the count) -- the count_parts of gine_crps_fwd_grad, recounted
 * every step (inside a captured step too).  gine_head_fwd_count writes the same partials
 * beside the head forward, so a training step needs no launch for them.
 * ---------------------------------------------------------------------------------- */
#define GINE_LOSS_NORMAL 0
#define GINE_LOSS_MIXED_NORMAL 1
#define GINE_LOSS_MIXED 2
#define GINE_LOSS_MIXED_U 3
int gine_crps_num_partials(int64_t num_nodes, int32_t* num_partials);
int gine_crps_fwd(const float* pred, const float* y, int64_t num_nodes, int32_t kind, double u,
                  double xi, double c, double t, double* dpred, double* partials,
                  double* loss_out, double* count_out, uint32_t* ticket, void* stream);
int gine_crps_bwd(const double* dpred, const double* count, const double* gloss,
                  int64_t num_nodes, int32_t kind, float* grad_pred, void* stream);
#define GINE_COUNT_PARTS 64
int gine_count_valid(const float* y, int64_t num_nodes, uint32_t* count_parts, void* stream);
/* gine_crps_fwd that also writes grad_unit = (float)(dpred / count), the gradient for
 * gloss = 1 exactly as gine_crps_bwd would round it, given the count of non-NaN targets
 * up front (count_parts: GINE_COUNT_PARTS device uint32 partial counts of y, from
 * gine_count_valid or gine_head_fwd_count) -- a backward seeded with 1 then needs no launch. */
int gine_crps_fwd_grad(const float* pred, const float* y, int64_t num_nodes, int32_t kind,
                       double u, double xi, double c, double t, double* dpred, double* partials,
                       double* loss_out, double* count_out, uint32_t* ticket,
                       const uint32_t* count_parts, float* grad_unit, void* stream);
/* gine_crps_fwd_grad that also runs the output head's backward for that unit seed (the head
 * of gine_head_fwd: raw [N, K], its input h [N, channels], weight w [K, channels]): dh
 * [N, channels] as gine_head_bwd writes it from grad_pred = grad_unit, and per-workgroup dW |
 * db partials in head_slab (gine_crps_head_slab_floats() floats; gine_crps_head_grad_job
 * describes them for gine_grad_finalize_batch).  One launch instead of three (crps, crps_bwd,
 * head_bwd) for a training step's loss.backward() seeded with 1. */
int gine_crps_head_slab_floats(int64_t num_nodes, int32_t channels, int32_t kind,
                               size_t* floats);
int gine_crps_head_fwd_grad(const float* pred, const float* y, int64_t num_nodes, int32_t kind,
                            double u, double xi, double c, double t, double* dpred,
                            double* partials, double* loss_out, double* count_out,
                            uint32_t* ticket, const uint32_t* count_parts, float* grad_unit,
                            const float* raw, const float* h, const float* w, int32_t channels,
                            float* dh, float* head_slab, void* stream);
int gine_crps_head_grad_job(int64_t num_nodes, int32_t channels, int32_t kind,
                            const float* head_slab, float* dw, float* db, gine_grad_job* job);

/* ------------------------------------------------------------------------------------
 * The predictive distribution those losses score, over pred [N, K] fp32 (kind: GINE_LOSS_*);
 * every result fp64.  c = censoring point, z(x) = (x - mu) / sigma, Phi = normal cdf:
 *   NORMAL        F(x) = Phi(z)
 *   MIXED_NORMAL  F(x) = 0 for x < c, p + (1 - p) Phi(z) for x >= c (an atom P_c = F(c) at c)
 *   MIXED(_U)     as MIXED_NORMAL below u; for x >= u  m_u + (1 - m_u) G((x - u) / sigma_u),
 *                 m_u = p + (1 - p) Phi(z(u)), G(t) = 1 - (1 + xi t)^(-1/xi); u fixed (MIXED)
 *                 or the row's own (MIXED_U)
 * Defined for c < u and 0 < xi < 1: GINE_ERR_INVALID, before any HIP call, for a fixed
 * u <= c or xi outside (0, 1) (the two MIXED kinds) and for c >= 0 with MIXED_U (its u lies in
 * (0, 2.12)); for a bad kind, flag, negative size or NULL operand too.  At most 2^24
 * thresholds or levels (GINE_ERR_TOO_LARGE).  num_nodes = 0: GINE_OK, nothing launched.  One
 * launch each, no allocation, no host synchronisation (capturable).
 * gine_forecast_prob: out[n, t] = F(x[t]) = P(Y <= x[t]); with GINE_FORECAST_UPPER
 *   P(Y > x[t]), formed from erfc and the tail power (never 1 - F), exactly 1 below c.
 *   x: device pointer, num_x values.
 * gine_forecast_quantile: out[n, j] = inf{x : F(x) >= level[j]}: c for a level up to P_c,
 *   +inf at level 1, c (NORMAL: -inf) at level 0, NaN for a level outside [0, 1] or NaN.
 *   With GINE_FORECAST_UPPER the levels are exceedance probabilities s = 1 - q, used without
 *   forming 1 - s (return levels down to s = 1e-12).
 * gine_forecast_score: the scores of targets y [N] fp32 (NaN = missing) in one launch.  Per
 *   row the CRPS (of the distribution: where(y < u, ...) for MIXED_U too, not the sigmoid
 *   blend of training) and the PIT interval [F(y-), F(y)] = [pit_lo, pit_hi], which is
 *   [0, P_c] at the atom and one point elsewhere; NaN in all three for a NaN target.  Per
 *   threshold brier[t] = mean over valid rows of (P(Y > x[t]) - 1{y > x[t]})^2, and valid[0] =
 *   their number (NaN and 0 when there is none).  For the PIT and the Brier score a target at
 *   or below c is the atom (fp32 log 0.01 lies below the fp64 one).  crps_rows, pit_lo,
 *   pit_hi, valid may be NULL; num_x = 0 is allowed.  partials:
 *   gine_forecast_score_partials() doubles; sums in a fixed order (same bits every run);
 *   ticket as for gine_crps_fwd (zeroed once, left at 0, calls sharing it must not overlap).
 * ---------------------------------------------------------------------------------- */
#define GINE_FORECAST_UPPER 1
int gine_forecast_prob(const float* pred, int64_t num_nodes, int32_t kind, double u, double xi,
                       double c, const double* x, int32_t num_x, int32_t flags, double* out,
                       void* stream);
int gine_forecast_quantile(const float* pred, int64_t num_nodes, int32_t kind, double u,
                           double xi, double c, const double* level, int32_t num_levels,
                           int32_t flags, double* out, void* stream);
int gine_forecast_score_partials(int64_t num_nodes, int32_t num_x, size_t* count);
int gine_forecast_score(const float* pred, const float* y, int64_t num_nodes, int32_t kind,
                        double u, double xi, double c, const double* x, int32_t num_x,
                        double* crps_rows, double* pit_lo, double* pit_hi, double* brier,
                        double* valid, double* partials, uint32_t* ticket, void* stream);

/* ------------------------------------------------------------------------------------
 * The linear pool of num_members checkpoint forecasts (additive in ABI 10):
 *   Fbar(x) = sum_m w_m F_m(x),  sfbar(x) = sum_m w_m sf_m(x)  (members in index order),
 * F_m the distribution above of member m's row of preds [num_members, N, K] fp32 (contiguous;
 * one kind, u, xi, c for all members).  weights: num_members fp64 on the device, > 0, summing
 * to 1 (normalised by the caller).  1 <= num_members <= 32, negative sizes and the domain
 * errors of gine_forecast_* are GINE_ERR_INVALID before any HIP call; num_nodes = 0 is
 * GINE_OK and launches nothing; more than 2^31 - 1 rows or 2^24 points GINE_ERR_TOO_LARGE.
 * One launch each, no allocation, no host synchronisation.  A pool of one member of weight
 * 1, or of 2^k copies of one member at equal weights, returns the bits of gine_forecast_*.
 * gine_pool_prob: out[n, t] = Fbar(x[t]); with GINE_FORECAST_UPPER sfbar(x[t]).
 * gine_pool_quantile: out[n, j] = inf{x : Fbar(x) >= level}: the edge levels as
 *   gine_forecast_quantile; c for a level up to sum_m w_m P_c,m (GINE_FORECAST_UPPER: for
 *   s >= sum_m w_m S_c,m); the members' common quantile where they agree; otherwise the upper
 *   end of a bracket of two adjacent doubles found by a safeguarded Newton / bisection
 *   between the members' quantiles (at most 89 evaluations of the pool; the upper form
 *   solves sfbar(x) = s).  level_row_stride 0: level[j] for every row; otherwise row n reads
 *   level[n * level_row_stride + j] (level_row_stride >= num_levels).
 * gine_pool_score: the scores of targets y [N] fp32 (NaN = missing) in one launch, one
 *   workgroup per row: crps_rows = member_crps_rows - diversity_rows, member_crps_rows =
 *   sum_m w_m crps_m(y) (the closed forms of gine_forecast_score), diversity_rows = V =
 *   int sum_m w_m (F_m - Fbar)^2 dx >= 0, which depends on no target (written for NaN targets
 *   too; exactly 0 for equal members) and is integrated by 16-point Gauss-Legendre panels
 *   between the sorted breakpoints c, u_m, mu_m + k sigma_m (k = 0, +-1, 2, 3, 5, 8) and, for
 *   the two MIXED kinds, one 32-point Gauss-Jacobi panel over [max u_m, inf): jacobi_nodes /
 *   jacobi_weights [32] are that rule's on [0, 1] for the weight w^(2/xi - 2) (device
 *   pointers; unused and may be NULL for the other kinds).  pit_lo / pit_hi, brier, valid,
 *   ticket as gine_forecast_score, from Fbar and sfbar.  Every row output may be NULL.
 *   partials: gine_pool_score_partials() doubles.
 * ---------------------------------------------------------------------------------- */
int gine_pool_prob(const float* preds, int32_t num_members, int64_t num_nodes, int32_t kind,
                   double u, double xi, double c, const double* weights, const double* x,
                   int32_t num_x, int32_t flags, double* out, void* stream);
int gine_pool_quantile(const float* preds, int32_t num_members, int64_t num_nodes, int32_t kind,
                       double u, double xi, double c, const double* weights,
                       const double* level, int32_t num_levels, int64_t level_row_stride,
                       int32_t flags, double* out, void* stream);
int gine_pool_score_partials(int64_t num_nodes, int32_t num_x, size_t* count);
int gine_pool_score(const float* preds, const float* y, int32_t num_members, int64_t num_nodes,
                    int32_t kind, double u, double xi, double c, const double* weights,
                    const double* x, int32_t num_x, const double* jacobi_nodes,
                    const double* jacobi_weights, double* crps_rows, double* member_crps_rows,
                    double* diversity_rows, double* pit_lo, double* pit_hi, double* brier,
                    double* valid, double* partials, uint32_t* ticket, void* stream);

/* ------------------------------------------------------------------------------------
 * Pair sums for fitting the pool's weights (additive in ABI 10).  Summed over
 * rows with a target, the pool's CRPS is c . w - 1/2 w' D w: c_m the sum of member m's
 * closed-form CRPS, D_ml the sum of int (F_m - F_l)^2 dx.  gine_pool_pairs gives both, and
 * the number of rows, per segment g of rows ptr[g] <= i < ptr[g + 1] (ptr [num_segments + 1]
 * int64 on the device, ptr[0] = 0, non-decreasing, ptr[num_segments] = num_nodes; the caller
 * validates it; empty segments are allowed), over the rows whose target is not NaN:
 *   count [G], member_crps [G, M], distance [G, M (M - 1) / 2] with the pairs packed
 *   (0,1), (0,2), ..., (M-2, M-1); distance may be NULL for one member.
 * Each integral by gine_pool_score's rule for the row -- the breakpoints of all M members, empty
 * panels skipped, 16-point Gauss-Legendre panels and for the MIXED kinds the Gauss-Jacobi panel
 * (jacobi_nodes / jacobi_weights as gine_pool_score), the difference there from the exceedance
 * probabilities -- every term formed as wq (F_m - F_l) (F_m - F_l): equal members give exactly
 * 0, and swapping or permuting members permutes the results bit for bit.  No weights: nothing
 * here depends on them.  One launch; rows are added in a fixed order per segment (64-row tiles
 * of the segment, then the tiles), no fp64 atomics: the bits depend on M and on the segment's
 * rows alone.  partials: gine_pool_pairs_partials() doubles (one record of 1 + M + M (M - 1) / 2
 * per tile, floor(N / 64) + G tiles at the most); ticket as gine_pool_score.  Validation as
 * gine_pool_score, and num_segments >= 1, before any HIP call; num_nodes = 0 launches nothing.
 * ---------------------------------------------------------------------------------- */
int gine_pool_pairs_partials(int64_t num_nodes, int32_t num_members, int64_t num_segments,
                             size_t* count);
int gine_pool_pairs(const float* preds, const float* y, int32_t num_members, int64_t num_nodes,
                    int32_t kind, double u, double xi, double c, const double* jacobi_nodes,
                    const double* jacobi_weights, const int64_t* ptr, int64_t num_segments,
                    double* count, double* member_crps, double* distance, double* partials,
                    uint32_t* ticket, void* stream);

/* ------------------------------------------------------------------------------------
 * The raw ensemble beside that distribution: M <= 64 members per row (one wavefront a row),
 * read in place from a strided fp32 view: member i of row n is
 *   x = shift + scale * (double)members[n * row_stride + i * member_stride]
 * (strides in elements, >= 0; the affine undoes a StandardScaler column), all arithmetic and
 * every result fp64.  A NaN member is missing: m = the row's number of valid members.  The
 * stable rank of member i among the valid ones is
 *   r_i = 1 + #{j valid : x_j < x_i or (x_j == x_i and j < i)}   (ties: lower index first).
 * GINE_ERR_INVALID, before any HIP call, for num_members outside 1..64, a negative size or
 * stride, a bad flag or a NULL operand.  num_rows = 0: GINE_OK, nothing launched.  One launch
 * each, no workspace, no allocation, no host synchronisation (capturable); member sums in a
 * fixed order (same bits every run).
 * gine_ensemble_score: against targets y [N] fp32 (NaN = missing; y may be NULL), per row
 *   crps      = (1/m) sum |x_i - y| - (1/(2 m^2)) sum_i sum_j |x_i - x_j|, the pair term formed
 *               from the ranks as (1/m^2) sum_i (2 r_i - m - 1) x_i;
 *   crps_fair = the same with 1/(2 m (m - 1)); NaN when m < 2;
 *   rank_lo = #{x_i < y}, rank_hi = #{x_i <= y}: the observation's verification rank lies in
 *               rank_lo..rank_hi of 0..m (the ensemble's pit_lo / pit_hi);
 *   all four NaN for a NaN target or m = 0; members_valid = m (0 without members).
 *   prob[n, t] = #{x_i > x[t]} / m for num_x device thresholds x (fp64): it does not read y,
 *   NaN when m = 0.  Each row output may be NULL; num_x = 0 is allowed.
 * gine_ensemble_ecc: ensemble copula coupling (ECC-Q): out[n, i] = the quantile of row n of
 *   pred [N, K] (kind, u, xi, c as gine_forecast_quantile) at the level r_i / (m + 1), or
 *   (r_i - 0.5) / m with GINE_ECC_MIDPOINT, formed by one division in double; NaN where member
 *   i is missing.  out [N, num_members] fp64.
 * ---------------------------------------------------------------------------------- */
#define GINE_ECC_MIDPOINT 1
int gine_ensemble_score(const float* members, int64_t row_stride, int64_t member_stride,
                        int32_t num_members, double scale, double shift, const float* y,
                        int64_t num_rows, const double* x, int32_t num_x, double* crps_rows,
                        double* crps_fair_rows, double* rank_lo, double* rank_hi,
                        double* members_valid, double* prob, void* stream);
int gine_ensemble_ecc(const float* pred, int64_t num_nodes, int32_t kind, double u, double xi,
                      double c, const float* members, int64_t row_stride, int64_t member_stride,
                      int32_t num_members, double scale, double shift, int32_t flags,
                      double* out, void* stream);

/* ------------------------------------------------------------------------------------
 * EMOS: the ensemble's summary statistics mapped affinely to the parameters of the loss's
 * distribution, the coefficients fitted per group of rows by minimum CRPS (additive in ABI
 * 10).  kind: GINE_LOSS_NORMAL / MIXED_NORMAL / MIXED (K = 2, 3, 4 columns,
 * P = 2 K coefficients); GINE_LOSS_MIXED_U is GINE_ERR_INVALID (its u is a per-row network
 * output).  Per row, with x_i as gine_ensemble_score (NaN = missing, m valid members):
 *   mean = (1/m) sum x_i, sd = sqrt((1/m) sum (x_i - mean)^2), dry = #{x_i <= c} / m,
 * fp64, summed in member order; z = (mean, sd, dry, sd), raw_k = theta[2k] + theta[2k+1] z_k,
 *   mu = raw_0, sigma = softplus(raw_1) + 1e-6, p = sigmoid(raw_2),
 *   sigma_u = softplus(raw_3) + 1e-6, softplus(x) = max(x, 0) + log1p(exp(-|x|)).
 * Rows are in collated order (row = day * num_stations + station); num_stations = 0 is one
 * global group.  The pack [R, 4] fp64 = (mean, sd, dry, y) is group-major: row n lies at
 * (n % S) * (N / S) + n / S (at n for S = 0).
 * gine_emos_predictors: members / strides / scale / shift as gine_ensemble_score, y [N] fp32
 *   or NULL (then NaN); writes the pack; rows without a valid member get NaN predictors.
 * gine_emos_fit: ptr [num_groups + 1] int64 on the device (contiguous segments of pack rows as
 *   gine_pool_pairs; the caller validates it, the kernel clamps it into 0..num_rows).  Per
 *   group over its valid rows (a target and m >= 1), from theta0 = (0, 1, b, 0, 0, 0, b, 0)
 *   truncated to P, b = log(e - 1):
 *     J(theta) = (1/n) sum crps(pred(theta; row), y) + ridge |theta - theta0|^2,
 *   crps the closed form of gine_crps_fwd for the kind (fixed u), minimised by BFGS on the
 *   inverse Hessian: H = I; stop with status 0 when max|g| <= gtol max(1, |J|); d = -H g, and
 *   H = I, d = -g unless g.d < 0; Armijo backtracking with c1 = 1e-4 over the steps 1, 1/2,
 *   ..., 2^-40 (a non-finite J fails); H updated when s.y > 1e-10 |s| |y|; at most max_iter
 *   iterations.  theta [G, P]; report [G, 8] fp64 = J, mean CRPS without the ridge term,
 *   max|g|, iterations, evaluations, valid rows, status, 0.  status: 0 converged, 1 iteration
 *   limit, 2 no decrease along d (theta: the last accepted point), 3 fewer than min_rows
 *   valid rows (theta = theta0; J, CRPS and max|g| NaN).  One 256-thread workgroup per group,
 *   sums in a fixed order, no atomics: a group's bits depend on its rows alone.
 * gine_emos_predict: pred [N, K] fp32 in collated order from the pack of the same rows and
 *   num_stations and theta [G, P] (G = num_stations, or 1 for 0); NaN rows where mean is NaN.
 * Before any HIP call: GINE_ERR_INVALID for a bad kind, num_members outside 1..64, a negative
 * size or stride, num_rows not a multiple of num_stations, xi outside (0, 1) or u <= c for
 * MIXED, a negative or non-finite ridge or gtol, max_iter outside 0..GINE_EMOS_MAX_ITER,
 * min_rows < 1 or a NULL operand.  Zero rows or groups: GINE_OK, nothing launched.  One launch
 * each, no workspace, no host synchronisation (capturable).
 * ---------------------------------------------------------------------------------- */
#define GINE_EMOS_MAX_ITER 10000
int gine_emos_predictors(const float* members, int64_t row_stride, int64_t member_stride,
                         int32_t num_members, double scale, double shift, double c,
                         const float* y, int64_t num_rows, int64_t num_stations, double* pack,
                         void* stream);
int gine_emos_fit(const double* pack, const int64_t* ptr, int64_t num_groups, int64_t num_rows,
                  int32_t kind, double u, double xi, double c, double ridge, double gtol,
                  int32_t max_iter, int32_t min_rows, double* theta, double* report,
                  void* stream);
int gine_emos_predict(const double* pack, const double* theta, int64_t num_rows,
                      int64_t num_stations, int32_t kind, float* pred, void* stream);

/* ------------------------------------------------------------------------------------
 * Threshold-weighted CRPS, weight 1{x >= t}, in model space, fp64 per row:
 *   twCRPS_t(F, y) = int_t^inf (F(x) - 1{x >= y})^2 dx = CRPS(F_t, max(y, t)),
 * F_t the distribution of max(Y, t).  With t' = max(t, c) for the three censored kinds
 * (t' = t for GINE_LOSS_NORMAL) and y' = max(y, t'): the closed-form CRPS of the kind with
 * c := t', y := y' (NORMAL: the MIXED_NORMAL form with p = 0); for MIXED / MIXED_U with
 * t' >= u (the row's own u for MIXED_U) only the tail is left: with a = 1 - m_u,
 * w(x) = 1 + xi (x - u) / sigma_u, e1 = -(1 - xi)/xi, e2 = -(2 - xi)/xi,
 *   (y' - t') + 2 a sigma_u/(1 - xi) (w(y')^e1 - w(t')^e1) + a^2 sigma_u/(2 - xi) w(t')^e2.
 * F is the where(y < u, ...) distribution of gine_forecast_score for MIXED_U too.
 * gine_forecast_twcrps: pred / y / kind / u / xi / c as gine_forecast_score, x [num_x] device
 *   thresholds (fp64).  rows [N, num_x] (may be NULL; NaN for a NaN target), mean [num_x] over
 *   the valid rows (NaN when there is none), valid[0] their number (may be NULL).  A threshold
 *   of -inf gives the row's CRPS at max(y, c) (at y for NORMAL), +inf gives 0, NaN gives NaN.
 *   partials: gine_forecast_twcrps_partials doubles; ticket: one zeroed uint32, left at 0.
 *   One launch, sums in a fixed order (same bits every run); num_x = 0 and num_nodes = 0
 *   (nothing launched, nothing written) are allowed.
 * gine_ensemble_twcrps: the arguments of gine_ensemble_score (y not NULL) and the crps /
 *   crps_fair formulas of that entry applied to max(x_i, x[t]) and max(y, x[t]): rows and
 *   fair_rows [N, num_x], NaN where gine_ensemble_score gives NaN and for a NaN threshold.
 *   The members are ranked once per row (clamping is monotone).  There is no c here.
 * gine_crps_tw_fwd / _fwd_grad / _bwd: gine_crps_fwd / _fwd_grad / _bwd for the per-node loss
 *   (1 - tw_weight) * L_kind(pred, y) + tw_weight * twCRPS_{tw_threshold}(pred, y),
 *   L_kind exactly the per-node loss of gine_crps_fwd (the sigmoid blend for MIXED_U), the tw
 *   term differentiated through whichever branch the row takes, and through u for MIXED_U.
 *   Both scalars are launch arguments (a captured step replays them); GINE_ERR_INVALID for
 *   tw_weight outside [0, 1] or a non-finite tw_threshold.  Same partials
 *   (gine_crps_num_partials), ticket, count_parts and outputs as the plain entries; dpred
 *   holds the weighted sum, so _bwd only checks the two scalars.  There is no head-backward
 *   form: the head backward of a tw loss is gine_head_bwd.
 * ---------------------------------------------------------------------------------- */
int gine_forecast_twcrps_partials(int64_t num_nodes, int32_t num_x, size_t* count);
int gine_forecast_twcrps(const float* pred, const float* y, int64_t num_nodes, int32_t kind,
                         double u, double xi, double c, const double* x, int32_t num_x,
                         double* rows, double* mean, double* valid, double* partials,
                         uint32_t* ticket, void* stream);
int gine_ensemble_twcrps(const float* members, int64_t row_stride, int64_t member_stride,
                         int32_t num_members, double scale, double shift, const float* y,
                         int64_t num_rows, const double* x, int32_t num_x, double* rows,
                         double* fair_rows, void* stream);
int gine_crps_tw_fwd(const float* pred, const float* y, int64_t num_nodes, int32_t kind,
                     double u, double xi, double c, double t, double tw_threshold,
                     double tw_weight, double* dpred, double* partials, double* loss_out,
                     double* count_out, uint32_t* ticket, void* stream);
int gine_crps_tw_fwd_grad(const float* pred, const float* y, int64_t num_nodes, int32_t kind,
                          double u, double xi, double c, double t, double tw_threshold,
                          double tw_weight, double* dpred, double* partials, double* loss_out,
                          double* count_out, uint32_t* ticket, const uint32_t* count_parts,
                          float* grad_unit, void* stream);
int gine_crps_tw_bwd(const double* dpred, const double* count, const double* gloss,
                     int64_t num_nodes, int32_t kind, double tw_threshold, double tw_weight,
                     float* grad_pred, void* stream);

/* ------------------------------------------------------------------------------------
 * Member fields scored per graph (csrc/gine_field.hip): members [N, M], M <= 64,
 * against targets y [N] fp32 (NaN = missing); the rows of graph g are ptr[g] .. ptr[g+1]-1
 * (ptr [G+1] int64 on the device, ptr[0] = 0, non-decreasing, ptr[G] = num_rows).  Member i of
 * row n is  x = shift + scale * (double)members[n * row_stride + i * member_stride]  (strides in
 * elements, >= 0), the element fp32 (GINE_FIELD_F32: the raw ensemble, read in place) or fp64
 * (GINE_FIELD_F64: the output of gine_ensemble_ecc).  Per graph, S = the rows with a non-NaN
 * target and at least one non-NaN member, V = the members non-NaN at every row of S (all M for
 * an empty S): rows_valid = |S|, members_valid = m = |V|, never NaN; every score is NaN when S
 * is empty or m = 0.  All [G] outputs fp64; each may be NULL.
 * gine_field_energy:  es = (1/m) sum_i |X_i - y| - (1/(2 m^2)) sum_ij |X_i - X_j|, |.| the
 *   Euclidean norm over S and i, j in V; es_fair with 1/(2 m (m - 1)), NaN for m < 2.
 * gine_field_variogram: vs = sum over the pairs a < b of S of
 *   (|y_a - y_b|^p - (1/m) sum_i |X_ai - X_bi|^p)^2, pairs = |S| (|S| - 1) / 2; p > 0 finite
 *   (0.5, 1 and 2 take sqrt, abs and the square, any other p pow).
 * gine_field_area: A_i = the max (GINE_FIELD_MAX) or mean (GINE_FIELD_MEAN) over S of
 *   mm(x) = max(exp(x) - 0.01, 0) for i in V (NaN otherwise) -> members_out [G, M]; obs = the
 *   same of mm(y); crps / crps_fair / rank_lo / rank_hi of gine_ensemble_score on (A, obs).
 * partials: gine_field_*_partials doubles of workspace (0 for the area: partials may be NULL
 *   there).  GINE_FIELD_ROW_TILE rows make one tile of the energy and variogram kernels.
 * GINE_ERR_INVALID, before any HIP call, for num_members outside 1..64, a negative size or
 * stride, an unknown dtype or stat, p <= 0 or not finite, or a NULL members / y / ptr /
 * partials.  num_graphs = 0 or num_rows = 0: GINE_OK, nothing launched, nothing written.  No
 * allocation, no host synchronisation (capturable); every sum fp64 in a fixed order, no
 * floating-point atomics (same bits every run).
 * ---------------------------------------------------------------------------------- */
#define GINE_FIELD_F32 0
#define GINE_FIELD_F64 1
#define GINE_FIELD_MAX 0
#define GINE_FIELD_MEAN 1
#define GINE_FIELD_ROW_TILE 64
int gine_field_energy_partials(int64_t num_rows, int64_t num_graphs, int32_t num_members,
                               size_t* count);
int gine_field_variogram_partials(int64_t num_rows, int64_t num_graphs, size_t* count);
int gine_field_area_partials(int64_t num_rows, int64_t num_graphs, size_t* count);
int gine_field_energy(const void* members, int32_t dtype, int64_t row_stride,
                      int64_t member_stride, int32_t num_members, double scale, double shift,
                      const float* y, int64_t num_rows, const int64_t* ptr, int64_t num_graphs,
                      double* es, double* es_fair, double* members_valid, double* rows_valid,
                      double* partials, void* stream);
int gine_field_variogram(const void* members, int32_t dtype, int64_t row_stride,
                         int64_t member_stride, int32_t num_members, double scale, double shift,
                         const float* y, int64_t num_rows, const int64_t* ptr,
                         int64_t num_graphs, double p, double* vs, double* pairs,
                         double* members_valid, double* rows_valid, double* partials,
                         void* stream);
int gine_field_area(const void* members, int32_t dtype, int64_t row_stride,
                    int64_t member_stride, int32_t num_members, double scale, double shift,
                    const float* y, int64_t num_rows, const int64_t* ptr, int64_t num_graphs,
                    int32_t stat, double* members_out, double* obs, double* crps,
                    double* crps_fair, double* rank_lo, double* rank_hi, double* members_valid,
                    double* rows_valid, double* partials, void* stream);

/* ------------------------------------------------------------------------------------
 * Paired score comparison (csrc/gine_compare.hip): two fp64 score grids a and b
 * over the same [T days, S stations].  Element (day t, station s) of a is
 *   a[t * a_day_stride + s * a_station_stride]
 * (strides in elements, >= 0; b has its own; nothing is copied, so column k of a [T*S, K]
 * result is read in place).  1 <= T < 2^31, S >= 1.  A pair is VALID when both elements are
 * non-NaN.  An optional w (fp64, own strides, finite and >= 0) is the pair's weight, NULL = 1;
 * w is only summed, it never multiplies a or b: it lets day sums be resampled together with
 * their valid counts as one column.
 *
 * Generator (counter-based: no state, no stored indices; all arithmetic mod 2^64):
 *   mix(seed, i): z = seed + (i + 1) * 0x9E3779B97F4A7C15
 *                 z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *                 z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *                 return z ^ (z >> 31)
 *   nb = ceil(T / L)                                    blocks per replicate, 1 <= L <= T
 *   start(r, j) = ((mix(seed, r * nb + j) >> 32) * T) >> 32     r = global replicate, 64-bit
 *   draws of replicate r: for j = 0 .. nb-1, for i = 0 .. L-1: day (start(r, j) + i) mod T,
 *                         cut off after T draws
 * the circular moving-block bootstrap (L = 1: the ordinary one).  The multiply-shift is biased:
 * a day's probability differs from 1/T by at most 2^-32, a relative T / 2^32.  All stations of
 * a replicate see the same days: spatial dependence is kept.
 *
 * Replicate sums (gine_compare_bootstrap): for replicate r and station s, walking the draws in
 * order, every valid pair does  A += a, B += b, W += w (or 1),  each one fp64 add from 0, in
 * no other order and with no fma;  diff = (A - B) / W,  skill = 1 - A / B;  IEEE results stand
 * (W = 0 gives NaN).  Outputs [R, S] fp64 row-major, each may be NULL but not all; row i is
 * global replicate rep_first + i, so a caller may cut a run into chunks of replicates and of
 * stations and get the same bits.  A workgroup takes GINE_COMPARE_REP_TILE / SW replicates, SW
 * (its station lanes) the power of two >= min(S, 64); unweighted grids of S >= 8, T <= 1,024
 * and R >= 128 are staged in LDS instead, 8 stations a workgroup, in passes of 128 replicates
 * (every tile edge divides GINE_COMPARE_REP_TILE).  The form does not change the bits.
 *
 * Marginal sums (gine_compare_reduce): station_a / _b / _n [S] over the days ascending,
 * sequentially (valid pairs only; n their count); day_a / _b / _n [T] over a day's stations in
 * a fixed order (lane l of a wavefront adds stations l, l + 64, ... ascending, then the 64 lane
 * sums fold in halves), the same bits every run.  Each output may be NULL, not all.
 *
 * Diebold-Mariano per station (gine_compare_dm), outputs [S] fp64, each may be NULL, not all:
 *   d_t = a - b at valid t, n = the number of valid days, dbar = (sum d_t) / n;
 *   g_k = (sum over t with t and t+k both valid of (d_t - dbar) * (d_{t+k} - dbar)) / n,
 *   k = 0 .. lags, every sum over t ascending, a term two subtractions, a multiply and an add;
 *   v = g_0; for k = 1 .. lags: v += 2.0 * (1.0 - k / (lags + 1.0)) * g_k   (Bartlett);
 *   var = v / n, stat = dbar / sqrt(var), pvalue = erfc(|stat| * 0.70710678118654752440).
 *   n < 2, var <= 0 or a non-finite var: stat and pvalue NaN; n, dbar (NaN at n = 0) and var
 *   are written as computed.
 *
 * Before any HIP call: GINE_ERR_INVALID for a NULL a or b, a negative size or stride, T < 1,
 * S < 1, block_len outside 1..T, lags outside 0..T-1, or all outputs NULL; GINE_ERR_DIM for
 * lags > GINE_COMPARE_MAX_LAGS; GINE_ERR_TOO_LARGE for T >= 2^31 or S > 65,535 * 64 in the
 * bootstrap.  R = 0: GINE_OK, nothing launched.  Caller-allocated buffers, no workspace, no
 * allocation, no host synchronisation (capturable); 64-bit offsets; no floating-point atomics.
 * ---------------------------------------------------------------------------------- */
#define GINE_COMPARE_MAX_LAGS 64
#define GINE_COMPARE_REP_TILE 256
int gine_compare_reduce(const double* a, int64_t a_day_stride, int64_t a_station_stride,
                        const double* b, int64_t b_day_stride, int64_t b_station_stride,
                        int64_t num_days, int64_t num_stations, double* day_a, double* day_b,
                        double* day_n, double* station_a, double* station_b, double* station_n,
                        void* stream);
int gine_compare_bootstrap(const double* a, int64_t a_day_stride, int64_t a_station_stride,
                           const double* b, int64_t b_day_stride, int64_t b_station_stride,
                           const double* w, int64_t w_day_stride, int64_t w_station_stride,
                           int64_t num_days, int64_t num_stations, int64_t block_len,
                           uint64_t seed, uint64_t rep_first, int64_t num_replicates,
                           double* sum_a, double* sum_b, double* sum_w, double* diff,
                           double* skill, void* stream);
int gine_compare_dm(const double* a, int64_t a_day_stride, int64_t a_station_stride,
                    const double* b, int64_t b_day_stride, int64_t b_station_stride,
                    int64_t num_days, int64_t num_stations, int32_t lags, double* n,
                    double* mean_d, double* var, double* stat, double* pvalue, void* stream);

/* ------------------------------------------------------------------------------------
 * Reliability diagrams (csrc/gine_reliability.hip): the CORP curve of
 * Dimitriadis, Gneiting and Jordan (2021) on a probability lattice, the split of the Brier
 * score into miscalibration, discrimination and uncertainty, and consistency resampling
 * (Broecker and Smith 2007).
 *
 * Inputs: p [N, T] fp64, element (row i, column t) at p[i * p_row_stride + t * p_col_stride]
 * (strides in elements, >= 0, nothing copied): the probability of "y exceeds x_t"; y [N] fp32,
 * NaN = missing; x [T] fp64; q, the lattice step count, 1 <= q <= GINE_RELIABILITY_MAX_LEVELS,
 * levels k = 0 .. q, K = q + 1; N < 2^30, T <= 65,535.
 *
 * Cells: (i, t) is VALID when y_i and x_t are not NaN and 0 <= p <= 1 (NaN and out-of-range
 * p are invalid, not an error).  Its event is o = (double)y_i > x_t (the comparison of
 * gine_ensemble_score), its level k = (int)rint(p * q): one fp64 multiply, round half to even.
 * The level's value is v_k = (double)k / (double)q.
 *
 * Counts (gine_reliability_counts), per column: n_k valid cells and e_k events among them at
 * level k, [T, K] int32 (zeroed by the call); level [T, N] int16, -1 at an invalid cell.
 * Integers: any traversal gives the same values.  n = sum n_k, E = sum e_k.
 *
 * Fit (gine_reliability_fit), per column: pool-adjacent-violators over the non-empty levels
 * ascending with a stack of blocks (E_b, N_b): push (e_k, n_k); while the block below the top
 * has a mean >= the top's, decided exactly in int64 as E_prev * N_top >= E_top * N_prev, merge
 * the two.  Block means end strictly increasing.  cal [T, K]: (double)E_b / (double)N_b of the
 * level's block, NaN at an empty level; block_id [T, K] (-1 at an empty level); block_e,
 * block_n [T, K]: entry b < num_blocks[t] is block b, the rest 0; a2 [T] int64; stats [T, 8]
 * fp64 = n, E, S, S_cal, UNC, MCB, DSC, AUC.  Every fp64 operation is rounded once, there is no
 * fma, sums start at +0:
 *   S     = (sum over non-empty k ascending of [ (double)(n_k - e_k) * (v*v)
 *                                                + (double)e_k * ((1-v)*(1-v)) ]) / (double)n
 *           (each bracket is formed, then added): the Brier score of the lattice forecast,
 *           within 1/q of the Brier score of p itself;
 *   S_cal = (sum over blocks ascending of (double)E_b * ((double)(N_b - E_b) / (double)N_b))
 *           / (double)n;
 *   UNC   = (double)E * ((double)(n - E) / (double)n) / (double)n;
 *   MCB   = S - S_cal;   DSC = UNC - S_cal;
 *   AUC   = (double)A2 / ((2.0 * (double)E) * (double)(n - E)),  A2 = sum_k e_k * (2 * C_k +
 *           (n_k - e_k)) in int64, C_k the non-events at the levels below k (Mann-Whitney, ties
 *           counted half).
 * IEEE results stand: n = 0 gives NaN everywhere, E = 0 or E = n NaN for AUC.  Each output may
 * be NULL, not all.
 *
 * Resampling (gine_reliability_resample): with mix(seed, i) of gine_compare_bootstrap above,
 *   U(r, i) = mix(seed, r * N + i) >> 11      r = global replicate index, all mod 2^64,
 * the synthetic event of cell (i, t) at level k is  U < (uint64)floor(v_k * 2^53)  (v = 0 never
 * fires, v = 1 always).  All columns share U, so the synthetic events of falling exceedance
 * probabilities are nested as real ones are, and column subsets and replicate chunks give the
 * same bits.  Per (r, t): e*_k over the valid cells, n_k unchanged, the same fit.  Row i of
 * the outputs is replicate rep_first + i: cal_rep [R, T, K] fp64 (NaN at empty levels),
 * stats_rep [R, T, 3] fp64 = S*, S*_cal, MCB* by the formulas above with e*, e_rep [R, T, K]
 * int32; each may be NULL, not all.  level and n_k are those gine_reliability_counts wrote (a
 * level outside 0 .. q counts as invalid).  A workgroup takes
 * GINE_RELIABILITY_REPS_PER_BLOCK replicate and as many columns as fit in half a CU's LDS.
 * traversal: GINE_RELIABILITY_ATOMIC counts with one LDS integer add per synthetic event,
 * GINE_RELIABILITY_BALLOT (K <= 64 only) per level with a wavefront ballot and popcount,
 * GINE_RELIABILITY_AUTO takes the faster of the two as measured (the atomic form
 * at every K).  The traversal does not change the bits.
 *
 * Before any HIP call: GINE_ERR_INVALID for q outside 1 .. GINE_RELIABILITY_MAX_LEVELS, a
 * negative size or stride, a NULL operand that the sizes need, all outputs NULL, an unknown
 * traversal or the ballot form at K > 64; GINE_ERR_TOO_LARGE for N >= 2^30, T > 65,535 or
 * R >= 2^31.  N = 0: the counts are zeroed, nothing else is launched; T = 0 or R = 0:
 * GINE_OK, nothing launched.  Caller-allocated buffers, no workspace, no allocation, no host
 * synchronisation (capturable); no floating-point atomics.
 * ---------------------------------------------------------------------------------- */
#define GINE_RELIABILITY_MAX_LEVELS 4096
#define GINE_RELIABILITY_REPS_PER_BLOCK 1
#define GINE_RELIABILITY_AUTO 0
#define GINE_RELIABILITY_ATOMIC 1
#define GINE_RELIABILITY_BALLOT 2
int gine_reliability_counts(const double* p, int64_t p_row_stride, int64_t p_col_stride,
                            const float* y, const double* x, int64_t num_rows,
                            int32_t num_thresholds, int32_t q, int32_t* n_k, int32_t* e_k,
                            int16_t* level, void* stream);
int gine_reliability_fit(const int32_t* n_k, const int32_t* e_k, int32_t num_thresholds,
                         int32_t q, double* cal, int32_t* block_id, int32_t* block_e,
                         int32_t* block_n, int32_t* num_blocks, int64_t* a2, double* stats,
                         void* stream);
int gine_reliability_resample(const int16_t* level, const int32_t* n_k, int64_t num_rows,
                              int32_t num_thresholds, int32_t q, uint64_t seed,
                              uint64_t rep_first, int64_t num_replicates, int32_t traversal,
                              double* cal_rep, double* stats_rep, int32_t* e_rep, void* stream);

/* ------------------------------------------------------------------------------------
 * Batch assembly with permuted feature columns (csrc/gine_batch.hip; the
 * reference's utils/data.py shuffle_features applied to station features and ensemble alike):
 * B samples of a device-resident dataset x [T, N, F], ens [T, N, M, F], y [T, N] written as one
 * collated batch out_x [B*N, F], out_ens [B*N, M, F], out_y [B*N].  With t = idx[b] (idx [B]
 * int64 on the device), slot b, station i, column f is read from
 *   (perm_t[t], perm_n[t * N + i])  when bit f of col_mask is set,   (t, i)  otherwise,
 * for x and for every member of ens; out_y[b, i] = y[t, i].  perm_t [T] int64 and perm_n [T, N]
 * int32 (positions as the dataset stores them) are device arrays; either may be NULL = the
 * identity.  The indices are trusted: the caller has checked that they are in range.
 * One launch, every access one dword per lane, 64-bit offsets; no allocation, no host
 * synchronisation (capturable).  Before any HIP call: GINE_ERR_INVALID for a negative size,
 * N, M or F below 1, T = 0 with B > 0, a NULL x / ens / y / idx / output, a col_mask bit at or
 * above F, or a non-zero col_mask with both permutations NULL; GINE_ERR_DIM for F > 64 (the
 * mask's width); GINE_ERR_TOO_LARGE for M * F > 2^31 - 513 or B * ceil(N / 4) >= 2^31.
 * B = 0: GINE_OK, nothing launched.
 * ---------------------------------------------------------------------------------- */
int gine_batch_fill_permuted(const float* x, const float* ens, const float* y,
                             const int64_t* idx, const int64_t* perm_t, const int32_t* perm_n,
                             uint64_t col_mask, int64_t T, int32_t N, int32_t M, int32_t F,
                             int32_t B, float* out_x, float* out_ens, float* out_y,
                             void* stream);

/* ------------------------------------------------------------------------------------
 * Weight/bias gradient of a plain Linear y = x W^T + b over many rows (the DeepSet,
 * dim_red and aggr layers around the GINE stack, models/gnn.py:48-68,112-123):
 *   dw [O, I] = dy^T x,  db [O] = bias_scale * sum_rows dy  (db may be NULL)
 * (bias_scale: y = x W^T + bias_scale * b, e.g. the DeepSet member sum of a bias)
 * dy [rows, O], x [rows, I] row-major fp32.  Rows are split into chunks
 * (gine_linear_wgrad_num_chunks); slab holds chunks * (O*I + O) floats of partials,
 * reduced in fixed order (deterministic).
 * ---------------------------------------------------------------------------------- */
int gine_linear_wgrad_num_chunks(int64_t rows, int32_t out_features, int32_t in_features,
                                 int32_t* num_chunks);
int gine_linear_wgrad(const float* dy, const float* x, int64_t rows, int32_t out_features,
                      int32_t in_features, float* slab, float* dw, float* db, float bias_scale,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * DeepSetEncoder phi first layer + ReLU + member sum, fused (models/gnn.py:48-68,
 * replaces phi[0](x) -> phi[1] ReLU -> .sum(dim=1) of the reference's Sequential; the
 * member-sum moves before phi[2] because a Linear commutes with the sum):
 *   r [N, H] = sum_m relu(ens[n, m, :] w1^T + b1)
 * ens [N, M, F] (row-major, contiguous), w1 [H, F], b1 [H], fp32.
 * H in {32, 64, 128, 256}; 1 <= F <= 64; M >= 1.  The [N, M, H] activation is never
 * written to memory; mask (optional, gine_deepset_mask_bytes bytes) receives its ReLU
 * pattern as bits, for the backward.
 * gine_deepset_bwd: weight gradients for dr = d loss / d r from the forward's mask:
 *   dw1 [H, F] = sum_{n,m} (dr[n] * 1[pre > 0])^T ens[n, m],  db1 [H] likewise summed
 * slab: gine_deepset_bwd_num_partials(N, H) * (H*F + H) floats of per-workgroup partials,
 * reduced in fixed order (deterministic).  db1 may be NULL.
 * ---------------------------------------------------------------------------------- */
int gine_deepset_mask_bytes(int64_t num_nodes, int32_t members, int32_t hidden, size_t* bytes);
/* Layout of the mask (for test-side decoding of the forward's ReLU decisions): nodes are
 * walked in groups of 2G (*nodes_per_half = G); the uint16 word
 * [(g * ceil(G*M/16) + t) * 2H + (c / 32) * 64 + 32 * h + c % 32] holds in bit q the decision
 * for hidden unit c of group row G*M*h + 16*t + q, i.e. node 2G*g + G*h + (16t+q) / M,
 * member (16t+q) % M (rows past G*M or past N are padding, bit 0). */
int gine_deepset_mask_layout(int64_t num_nodes, int32_t hidden, int32_t* nodes_per_half);
int gine_deepset_fwd(const float* ens, const float* w1, const float* b1, float* r,
                     uint16_t* mask, int64_t num_nodes, int32_t members, int32_t in_features,
                     int32_t hidden, void* stream);
/* gine_deepset_fwd plus the dense chain's two folded weights, computed from the current
 * weights by extra workgroups of the same launch, for gine_chain_fwd_folded2 (hidden = D in
 * {64, 128}, x_features = F <= 64; wr1 / br1 = rho[2], wdr / bdr = dim_red, wr0 / br0 =
 * rho[0], wp2 / bp2 = phi[2]; every pointer required):
 *   wfold  [2*D*(F+D) + D] = W' [D][F+D] | b' [D] | W'^T [F+D][D],
 *          W' = [Wdr_x | Wdr_e Wr1], b' = Wdr_e br1 + bdr;
 *   wfold2 [D*D + D] = Wf [D][D] | bf [D],  Wf = Wr0 Wp2, bf = members * Wr0 bp2 + br0. */
int gine_deepset_fwd_fold2(const float* ens, const float* w1, const float* b1, float* r,
                           uint16_t* mask, int64_t num_nodes, int32_t members,
                           int32_t in_features, int32_t hidden, const float* wr1,
                           const float* br1, const float* wdr, const float* bdr, float* wfold,
                           int32_t x_features, const float* wr0, const float* br0,
                           const float* wp2, const float* bp2, float* wfold2, void* stream);
/* Testing only: on != 0 keeps every DeepSet launch (gine_deepset_fwd, _fwd_fold2, _bwd,
 * _bwd_chain) on the generic tile stager; 0 (the default) lets a launch whose walks hold only
 * full tiles -- 16-node halves, num_nodes % 32 == 0, hidden in {64, 128}, ens on a 16-byte
 * boundary -- stage them with 16-byte loads and no per-element range tests.  Both stagers
 * give the same bits everywhere; the generic one is the tests' reference for the fast one. */
int gine_testing_deepset_generic_stager(int32_t on);
/* Testing only: *full_tiles = 1 when a DeepSet launch on this ens pointer, node count and hidden
 * width would take the full-tile stager (under the switch above as it stands), else 0. */
int gine_testing_deepset_stager(const float* ens, int64_t num_nodes, int32_t hidden,
                                int32_t* full_tiles);
int gine_deepset_bwd_num_partials(int64_t num_nodes, int32_t hidden, int32_t* num_partials);
int gine_deepset_bwd(const float* ens, const uint16_t* mask, const float* dr, float* slab,
                     float* dw1, float* db1, int64_t num_nodes, int32_t members,
                     int32_t in_features, int32_t hidden, void* stream);
/* gine_chain_bwd_folded2 followed by gine_deepset_bwd (the backward of phi[0] -> ReLU ->
 * member sum -> phi[2] -> rho -> dim_red's embedding columns) as one launch, where
 * gine_deepset_bwd_chain_ok sets *ok = 1: hidden in {64, 128}, x_features (the width of x,
 * the chain's F) <= 64, and enough nodes that the DeepSet kernels walk groups of 32 nodes
 * with one group per workgroup (hidden 128: 8,192 < N <= 16,384; hidden 64: 16,384 < N <=
 * 32,768; not hidden 64 with 41 to 48 in_features).  Each workgroup computes dt and dr of its own 32 nodes from their dh0 rows (the
 * chain kernel's arithmetic: dt, the slab, dw1 and db1 are the pair's bits); dt [N, hidden]
 * is written for gine_chain_wgrad_folded2, dr is not formed in memory.  slab, dw1, db1 as
 * gine_deepset_bwd (dw1 = NULL leaves the slab; job: gine_deepset_bwd_grad_job).  Any other
 * shape: GINE_ERR_INVALID -- run the pair. */
int gine_deepset_bwd_chain_ok(int64_t num_nodes, int32_t hidden, int32_t in_features,
                              int32_t x_features, int32_t* ok);
int gine_deepset_bwd_chain(const float* ens, const uint16_t* mask, const float* dh0,
                           const float* u, const float* wfold, const float* wfold2, float* dt,
                           float* slab, float* dw1, float* db1, int64_t num_nodes,
                           int32_t members, int32_t in_features, int32_t hidden,
                           int32_t x_features, void* stream);

/* ------------------------------------------------------------------------------------
 * Output head: aggr = Linear(D, K) + PostProcess (models/gnn.py:123,125,140-141;
 * models/model_utils.py:42-113), K and the column transforms given by the loss `kind`
 * (GINE_LOSS_*, K = 2, 3, 4, 5):  pred[:, 0] = raw (mu); sigma, sigma_u -> softplus + 1e-6;
 * p -> sigmoid; u (GINE_LOSS_MIXED_U) -> 2.12 * sigmoid.
 *   gine_head_fwd: raw [N, K] = h [N, D] W^T + b;  pred [N, K] = PostProcess(raw)
 *   gine_head_bwd: d raw = PostProcess'(raw) * grad_pred;  dh [N, D] = d raw W;
 *                  dw [K, D] = d raw^T h, db [K] = sum d raw (db may be NULL), through
 *                  gine_head_bwd_slab_floats() floats of per-workgroup partials, reduced
 *                  in fixed order (deterministic).
 * D multiple of 4, D <= 256.
 * ---------------------------------------------------------------------------------- */
int gine_head_fwd(const float* h, const float* w, const float* b, float* raw, float* pred,
                  int64_t num_nodes, int32_t channels, int32_t kind, void* stream);
/* gine_head_fwd that also counts the batch's non-NaN targets y [N] into count_parts
 * (GINE_COUNT_PARTS uint32, as gine_count_valid) for the loss pass that follows. */
int gine_head_fwd_count(const float* h, const float* w, const float* b, float* raw,
                        float* pred, int64_t num_nodes, int32_t channels, int32_t kind,
                        const float* y, uint32_t* count_parts, void* stream);
int gine_head_bwd_slab_floats(int64_t num_nodes, int32_t channels, int32_t kind,
                              size_t* floats);
int gine_head_bwd(const float* grad_pred, const float* raw, const float* h, const float* w,
                  float* dh, float* slab, float* dw, float* db, int64_t num_nodes,
                  int32_t channels, int32_t kind, void* stream);
/* dw = NULL in gine_head_bwd leaves the partial slab; this reduces it (another stream). */
int gine_head_bwd_reduce(const float* slab, float* dw, float* db, int64_t num_nodes,
                         int32_t channels, int32_t kind, void* stream);

/* ------------------------------------------------------------------------------------
 * Dense layers between the DeepSet member sum and the GINE stack (models/gnn.py:48-68,
 * 112-113, 132-135), phi's last Linear applied after the member sum:
 *   s = r Wp2^T + M bp2;  u = relu(s Wr0^T + br0);  e = u Wr1^T + br1;
 *   h0 = [x | e] Wdr^T + bdr
 * r [N, D] = the DeepSet forward's output, x [N, F] node features, M = members, D in
 * {64, 128}, F <= 64.  The chain runs doubly folded: only the ReLU separates its Linears, so
 *   u = relu(r Wf^T + bf), Wf = Wr0 Wp2, bf = M Wr0 bp2 + br0     (wfold2)
 *   h0 = [x | u] W'^T + b', W' = [Wdr_x | Wdr_e Wr1], b' = Wdr_e br1 + bdr   (wfold)
 * with wfold / wfold2 from gine_deepset_fwd_fold2; s, e and their gradients are never formed.
 * gine_chain_fwd_folded2: u (saved for the backward) and h0, one launch.
 * gine_chain_bwd_folded2, from dh0 = d loss / d h0: dt = (dh0 Wc) * 1[u > 0] (Wc = W'[:, F:]),
 *   dr = dt Wf (dr feeds gine_deepset_bwd), one launch.
 * gine_chain_wgrad_folded2: one engine launch for G = dh0^T [x | u] | g = sum_n dh0 (gfold
 *   [D*(F+D) + D]) and G2 = dt^T r | g2 = sum_n dt (g2fold [D*D + D]) through a slab of
 *   gine_chain_bwd_slab_floats() floats of partials reduced in fixed order; gfold = g2fold =
 *   NULL leaves the slab for gine_grad_finalize_batch (job:
 *   gine_chain_wgrad_folded2_grad_job).
 * gine_chain_unfold_grads2, after the reduction, one launch (fp32 MFMA; bias outputs may be
 *   NULL): dWdr = [G_x | G_u Wr1^T + g br1^T], dbdr = g, dWr1 = Wdr_e^T G_u,
 *   dbr1 = Wdr_e^T g, dWr0 = G2 Wp2^T + M g2 bp2^T, dbr0 = g2, dWp2 = Wr0^T G2,
 *   dbp2 = M Wr0^T g2.
 * ---------------------------------------------------------------------------------- */
int gine_chain_bwd_slab_floats(int64_t num_nodes, int32_t hidden, int32_t in_features,
                               size_t* floats);
int gine_chain_fwd_folded2(const float* r, const float* x, const float* wfold,
                           const float* wfold2, float* u, float* h0, int64_t num_nodes,
                           int32_t hidden, int32_t in_features, void* stream);
int gine_chain_bwd_folded2(const float* dh0, const float* u, const float* wfold,
                           const float* wfold2, float* dt, float* dr, int64_t num_nodes,
                           int32_t hidden, int32_t in_features, void* stream);
int gine_chain_wgrad_folded2(const float* dh0, const float* x, const float* r, const float* u,
                             const float* dt, float* slab, float* gfold, float* g2fold,
                             int64_t num_nodes, int32_t hidden, int32_t in_features,
                             void* stream);
int gine_chain_wgrad_folded2_grad_job(int64_t num_nodes, int32_t hidden, int32_t in_features,
                                      const float* slab, float* gfold, float* g2fold,
                                      gine_grad_job* job);
int gine_chain_unfold_grads2(const float* gfold, const float* wr1, const float* br1,
                             const float* wdr, float* dwdr, float* dbdr, float* dwr1,
                             float* dbr1, const float* g2fold, const float* wp2,
                             const float* bp2, const float* wr0, float* dwr0, float* dbr0,
                             float* dwp2, float* dbp2, float members, int32_t hidden,
                             int32_t in_features, void* stream);
/* The same chain unfolded, kept as the comparator the tests hold the folded form against
 * (raincast_gnn.chain.FOLD = False; slower): two launches each way.
 * gine_chain_fwd writes s, u, e (saved for the backward) and h0 (bias_scale = M).
 * gine_chain_bwd, from dh0: de = dh0 Wdr[:, F:], dt = (de Wr1) * 1[u > 0], ds = dt Wr0,
 *   dr = ds Wp2, and with slab != NULL all eight parameter gradients (dbp2 scaled by
 *   bias_scale; bias pointers may be NULL) through gine_chain_bwd_slab_floats() floats.
 * gine_chain_wgrad: the parameter-gradient half on its own (gine_chain_bwd with slab = NULL
 *   is the input-gradient half); all four weight outputs NULL leaves the slab for
 *   gine_grad_finalize_batch (job: gine_chain_wgrad_grad_job). */
int gine_chain_fwd(const float* r, const float* x, const float* wp2, const float* bp2,
                   float bias_scale, const float* wr0, const float* br0, const float* wr1,
                   const float* br1, const float* wdr, const float* bdr, float* s, float* u,
                   float* e, float* h0, int64_t num_nodes, int32_t hidden,
                   int32_t in_features, void* stream);
int gine_chain_bwd(const float* dh0, const float* x, const float* r, const float* s,
                   const float* u, const float* e, const float* wp2, const float* wr0,
                   const float* wr1, const float* wdr, float* de, float* dt, float* ds,
                   float* dr, float* slab, float* dwp2, float* dbp2, float bias_scale,
                   float* dwr0, float* dbr0, float* dwr1, float* dbr1, float* dwdr,
                   float* dbdr, int64_t num_nodes, int32_t hidden, int32_t in_features,
                   void* stream);
int gine_chain_wgrad(const float* dh0, const float* x, const float* r, const float* s,
                     const float* u, const float* e, const float* de, const float* dt,
                     const float* ds, float* slab, float* dwp2, float* dbp2, float bias_scale,
                     float* dwr0, float* dbr0, float* dwr1, float* dbr1, float* dwdr,
                     float* dbdr, int64_t num_nodes, int32_t hidden, int32_t in_features,
                     void* stream);


/* Measurement utility (not on the hot path): copy `bytes` (a multiple of 16) from src to dst
 * with 16-byte-per-lane streaming loads and stores -- the HBM copy ceiling bench.py prices
 * the message-passing kernels against (csrc/gine_probe.hip). */
int gine_copy_f4(const void* src, void* dst, int64_t bytes, void* stream);
/* Measurement utility (tools/chain_micro.py): `reps` 32x32 blocks of the split-bf16 row-GEMM
 * chain (K = 128) per wave in `blocks` 256-thread workgroups, in form `variant` (0: A split
 * in the loop, 1: pre-split A planes from LDS, 2: MFMAs only, 3: two chains interleaved);
 * ticks[block * 4 + wave] = shader-clock ticks of the loop, sink = [blocks * 256] sums. */
int gine_probe_chain(int32_t variant, int32_t reps, int32_t blocks, float* sink,
                     long long* ticks, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GINE_HIP_H_ */
