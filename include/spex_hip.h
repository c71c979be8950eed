/*
 * spex_hip.h — C ABI of libspexhip.so: the MI355X (gfx950) implementation of the SPEX LightGCN / NGCF graph
 * convolution + negative-sampled scoring hot path.
 *
 * The reference (XMUDM/SPEX) is pure Python on stock PyTorch: it has no FFI / plugin layer of its own, so there is no
 * existing binding to match symbol-for-symbol.  Each entry point below therefore names the reference call it
 * replaces (file:line relative to the reference root) — these are the calls a maintainer re-points at this
 * library (INTEGRATION.md shows the ctypes stub and the drop-in Python modules that already do so).
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - every dense pointer is a DEVICE pointer owned by the caller (e.g. torch.Tensor.data_ptr()); the library never
 *     frees or retains them past the call.  Row-major fp32, leading dimension == d, 16-byte aligned.
 *   - host pointers are marked `h_`.
 *   - every call is asynchronous on `stream` unless stated; no hidden device synchronisation and no allocation after
 *     spex_graph_create (safe to capture in a hipGraph) — with three documented exceptions that allocate once: the
 *     first spex_sddmm_f32 on a handle, the first spex_spmm_f32 / propagate call at d > 64 on a graph with long rows,
 *     and spex_timer_create.
 *   - return 0 on success, a negative spex_status otherwise; spex_last_error() gives the thread-local message.
 */
#ifndef SPEX_HIP_H
#define SPEX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum spex_status {
    SPEX_OK = 0,
    SPEX_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, unsorted CSR, ...) */
    SPEX_ERR_HIP = -2,         /* a HIP runtime call failed                                      */
    SPEX_ERR_COMM = -3,        /* an RCCL call of the spex_comm_* entries failed                   */
    SPEX_ERR_UNSUPPORTED = -4  /* e.g. the NGCF epilogue at d != 64                              */
} spex_status;

typedef struct spex_graph spex_graph_t;

int spex_version(void);                 /* ABI version, currently 5.  5 = 4 minus what round 3's measurements retired
                                         * (spex_graph_create_ex / SPEX_GRAPH_TILE_ROWS and spex_ngcf_spmm_layer_fwd_f32, the `flags`
                                         * argument of spex_graph_pack_digest, the tiled trust head, the one-wave NGCF kernels, the
                                         * narrow d <= 32 SpMM), plus spex_partitioned_dual_task_step_f32 (config 5 row-partitioned
                                         * as one call).  4 = 3 + the deterministic accumulation mode, per-descriptor fork / join
                                         * events, the spex_comm_* collectives, the one-launch middles, SPEX_STEP_PIPELINED. */
const char *spex_last_error(void);      /* thread-local, never NULL */

/* ------------------------------------------------------------------------------------------------ graph handle
 * Replaces: the torch sparse tensor the reference builds once and keeps on the device —
 *   LightGCN_SPEX/code/utility1/dataloader.py:179-185,221-222 (_convert_sp_mat_to_sp_tensor + coalesce + .cuda()),
 *   NGCF_SPEX/code/main_rec.py:47,102-108 (sparse_mx_to_torch_sparse_tensor).
 * Input is host CSR (rows sorted, columns ascending within a row = the coalesced COO order), copied to HBM once.
 * `h_edge_id` (optional, may be NULL = identity) gives, per stored entry, the index used to look the entry up in an
 * edge keep-mask (see spex_graph_set_edge_mask): a transposed copy of a graph passes the permutation back to the
 * original entry order so forward and backward drop the same edges.
 * The handle may hold any row block of a larger matrix (1-D row partition): n_rows local rows, column indices
 * global in [0, n_cols).
 * Synchronous (host -> device copies); builds the long-row segment table used for load balance.
 */
int spex_graph_create(const int32_t *h_rowptr, const int32_t *h_col, const float *h_val, const int32_t *h_edge_id,
                      int32_t n_rows, int32_t n_cols, int64_t nnz, spex_graph_t **out);
int spex_graph_destroy(spex_graph_t *g);
/* HOST ONLY (no device call, works without a GPU): FNV-1a fingerprints of everything spex_graph_create would upload for this
 * matrix — digest[0] the wave-task table, [1..5] the chunk arrays (source offsets, values, end-of-row masks + padding counts, edge
 * ids, output rows), [6] the long-row segment tables, [7] the hub tables and the table sizes.  The
 * host packer runs on SPEX_BUILD_THREADS threads (default min(16, cores)); the layout must not depend on that number. */
int spex_graph_pack_digest(const int32_t *h_rowptr, const int32_t *h_col, const float *h_val, int32_t n_rows, int32_t n_cols,
                           int64_t nnz, uint64_t *digest /* [8] */);
/* HOST ONLY: how the packer laid out the rows beyond 1 024 entries (hubs) — the tables the d == 64 launch folds them by.  out:
 * [n_positions, n_hubs, then per task position of the table's head (chunks, row, task word, 1 = first wave of a group, waves in
 * the group, the group's scratch row, hub), then per hub (its first scratch row, its number of groups)]; *n_out = ints needed
 * (call with out = NULL, cap = 0 to size).  Invariants: every hub starts a 16-task workgroup; its groups are 16 adjacent segments
 * (the last one shorter, the workgroup topped up with ordinary tasks); a hub's scratch rows are consecutive. */
int spex_graph_pack_hub_table(const int32_t *h_rowptr, const int32_t *h_col, const float *h_val, int32_t n_rows, int32_t n_cols,
                              int64_t nnz, int32_t *out, int64_t cap, int64_t *n_out);
/* HOST ONLY: the row-head table the handle would carry — a fixed-stride copy of every row's first min(entries, *stride) stored
 * entries in CSR order, padded with column 0 / value 0, row r at slot r * *stride (what lets the one-call BPR step's fused launch ask
 * for a row's first entries by the row id alone).  *n_out = slots needed (n_rows * *stride), 0 where none is built: source tables
 * above 16 MiB, rows beyond 1 024 entries, SPEX_ROW_HEADS=0 (read at creation).  Call with cap = 0 to size. */
int spex_graph_pack_row_heads(const int32_t *h_rowptr, const int32_t *h_col, const float *h_val, int32_t n_rows, int32_t n_cols,
                              int64_t nnz, int32_t *out_col, float *out_val, int64_t cap, int64_t *n_out, int32_t *stride);
/* n_rows, n_cols, nnz, number of long rows, number of long-row segments (any pointer may be NULL) */
int spex_graph_info(const spex_graph_t *g, int32_t *n_rows, int32_t *n_cols, int64_t *nnz, int32_t *n_long_rows,
                    int32_t *n_segments);
/* How the handle laid out its chunk table (any pointer may be NULL): bin_packed = 1 where tasks pack non-adjacent short rows
 * (source table within 16 MiB at d = 64); packed_words = 1 where such a table stores (output row << 16) | source row in one word
 * per entry (at most 65 536 rows and packs of 64 entries; SPEX_PACK_WORDS=0, read at creation, keeps a row array);
 * chunk_stride = the implied-position stride, or 0. */
int spex_graph_layout(const spex_graph_t *g, int32_t *bin_packed, int32_t *packed_words, int32_t *chunk_stride);

/* Edge dropout — replaces LightGCN.__dropout_x, utility1/model.py:46-55: keep entry e iff floor(rand_e + keep_prob),
 * kept values divided by keep_prob.  Two modes:
 *   injected : d_keep = device uint8[mask_len], indexed by edge_id (parity tests inject the reference's mask)
 *   sampled  : d_keep = NULL; the mask is counter-based: keep_e = (u + keep_prob >= 1) with u the top 24 bits of
 *              philox4x32-10(key = seed, counter = edge_id) scaled to [0,1) (torch.rand's grid), recomputed inside
 *              the SpMM, identical in forward / backward and across layers for one seed.
 * keep_prob >= 1 or mode 0 switches dropout off.  Takes effect for subsequent launches on this handle.
 */
int spex_graph_set_edge_mask(spex_graph_t *g, int mode /*0 off, 1 injected, 2 sampled*/, const uint8_t *d_keep,
                             float keep_prob, uint64_t seed);

/* ------------------------------------------------------------------------------------------------ SpMM
 * Replaces: torch.sparse.mm(Graph, all_emb) — utility1/model.py:91 (and :87 for the A_split row blocks),
 * NGCF_SPEX/code/main_rec.py:76; and its autograd backward (A^T g) when called on the transposed handle.
 *
 *   y[r,:]       = sum_e val[e] * X[col[e],:]               (fp32 fmaf chain, ascending column order)
 *   if add_in:     y += add_in[r,:] / add_div               (backward of the layer mean: g/(L+1) + A^T G)
 *   if Y:          Y[r,:] = y
 *   if acc_out:    acc_out[r,:] = (acc_in[r,:] + y) / acc_div   (running layer sum; acc_div = L+1 on the last layer)
 *
 * X: [n_cols, d]; Y, add_in, acc_in, acc_out: [n_rows, d].  acc_in may equal acc_out.  X must not alias Y / acc_out.
 * Any d >= 1 (d == 64 takes the tuned path: one lane per column).  A graph with long rows sums their segments through a
 * scratch buffer owned by the handle (rows beyond 1 024 entries: groups of 16 segments through LDS, one scratch row per group,
 * folded by the row's last group inside the d == 64 launch — in a fixed order: results repeat bit for bit; SPEX_HUB_FOLD=0,
 * edge-dropout launches and other d: a small second launch adds them): calls on ONE stream are ordered by the stream; a call on another stream is made to
 * wait (an event, inserted by the library) for everything queued on the stream that used the scratch last, so one handle
 * may be driven from several streams of one host thread.  Concurrent calls from several HOST threads on one handle are
 * not supported (one handle per thread).
 */
int spex_spmm_f32(const spex_graph_t *g, const float *X, float *Y, const float *add_in, float add_div,
                  const float *acc_in, float *acc_out, float acc_div, int32_t d, void *stream);

/* The same product for a LIST of rows only (d = 64, 128 or 256, no edge dropout):
 *   for r in { idx_a[k] + off_a : k < n_a } + { idx_b[k] + off_b : k < n_b }:
 *     y = sum_e val[e] X[col[e],:];   Y[r,:] = y (if Y);   acc_out[r,:] = (acc_in[r,:] + y) / acc_div (if acc_out)
 * Other rows of Y / acc_out are left untouched.  idx_*: device int64 (a batch's users and items as the DataLoader
 * hands them over; off_b = n_user_rows).  Duplicates allowed — every copy stores the same value — PROVIDED acc_out
 * is not acc_in (in place, a second copy could read the row the first has already finished); an index outside
 * [0, n_rows) is skipped.
 * The training step reads the last propagation layer (model.py:91-95) at the batch's rows only (model.py:115-116):
 * this replaces that layer's launch over the whole matrix.  Rows of up to 1024 entries are summed in the order
 * spex_spmm_f32 uses at the same d (bit-identical results).  d > 64: X / Y / acc_in / acc_out 16-byte aligned.
 */
int spex_spmm_rowlist_f32(const spex_graph_t *g, const float *X, const int64_t *idx_a, int32_t n_a, int64_t off_a,
                          const int64_t *idx_b, int32_t n_b, int64_t off_b, float *Y, const float *acc_in, float *acc_out,
                          float acc_div, int32_t d, void *stream);
/* The same rows on a ROW PARTITION (d == 64; the partitioned steps' last forward layer, model.py:91-97 at the rows of model.py:115-116):
 * slot k names position pos[k] of the padded global layout; `g` is the rank's block (n_local rows) and lo the rank's first position.
 * For a slot the rank owns (r = pos[k] - lo in [0, n_local)):
 *   out_prop[k] = (acc_in[r] [+ acc2[r] [+ acc3[r]]] + (A X)[r]) / acc_div  (the row-list kernel's order of sums; acc2 / acc3: further
 *                 layer tables, NULL = absent),   out_raw[k] = raw[r]  (if out_raw)
 * and ZEROS for every other slot: out_prop / out_raw ([n, 64], compact) are the operands of the owner-computes all-reduce
 * (spex_comm_allreduce_sum_f32) that leaves the batch's rows on every rank.  One launch instead of a whole-block product + two
 * spex_gather_owned_rows_f32.  A mask on the handle (edge dropout) is applied entry by entry, as spex_spmm_f32 applies it. */
int spex_spmm_owned_rows_f32(const spex_graph_t *g, const float *X, const int64_t *pos, int32_t n, int64_t lo, const float *acc_in,
                             const float *acc2, const float *acc3, float acc_div, const float *raw, float *out_prop, float *out_raw,
                             int32_t d, void *stream);

/* Whole LightGCN.computer(), utility1/model.py:66-97, for a graph held entirely on this device (n_rows == n_cols):
 *   E^{l+1} = A E^l (l < L);  mean_out = (E^0 + ... + E^L) / (L+1).
 * ws: caller-provided device workspace of 2 * n_rows * d floats (ping-pong layer buffers).
 * layers_out (optional): L * n_rows * d floats receiving E^1..E^L (then ws may be NULL).
 */
int spex_propagate_f32(const spex_graph_t *g, const float *E0, float *mean_out, float *layers_out, float *ws,
                       int32_t L, int32_t d, void *stream);

/* Backward of the above w.r.t. E0 given g_out = d loss / d mean_out  (autograd of model.py:83-95):
 *   G_L = g_out/(L+1);  G_l = g_out/(L+1) + A^T G_{l+1};  grad_E0 = G_0.
 * gt is the handle of A^T (for the symmetric LightGCN adjacency the same handle).  ws: 3 * n_rows * d floats
 * (the scaled gradient g_out/(L+1) plus two ping-pong layer buffers).
 */
int spex_propagate_bwd_f32(const spex_graph_t *gt, const float *g_out, float *grad_E0, float *ws, int32_t L,
                           int32_t d, void *stream);

/* ------------------------------------------------------------------------------------------------ bf16 gather tables
 * Mixed precision for the propagation, d == 64 only (any other d: SPEX_ERR_UNSUPPORTED): the GATHER SOURCE is a bf16 table
 * ([rows, 64] row-major, uint16_t bit patterns: 128-byte rows, one L2 line instead of two), everything else stays fp32 —
 * bf16 -> fp32 widening is exact and every product and sum is the fp32 fmaf chain of spex_spmm_f32 in the same order.  Rounding
 * enters only where a table is rounded to become a gather source.  fp32 stays the default: nothing calls these unasked.
 *
 * spex_cast_bf16_f32: X16[i] = bf16(X[i]), round to nearest even, for i < n; NaN stays NaN, +-0 and +-Inf are preserved, finite
 * values beyond the largest bf16 round to Inf (what torch.Tensor.to(torch.bfloat16) returns).  Any element-aligned pointers; 16-byte
 * aligned X and 8-byte aligned X16 take the vectorised kernel.
 */
int spex_cast_bf16_f32(const float *X, uint16_t *X16, int64_t n, void *stream);

/* spex_spmm_f32 gathering from X16 ([n_cols, 64] bf16) — with Xw = float(X16), per output element the same chain:
 *   y[r,:]       = sum_e val[e] * Xw[col[e],:]              (acc = fmaf(val, widen(x16), acc) in the task's entry order; segments of
 *                                                            rows of 65..1 024 entries added through LDS in segment order)
 *   if add_in:     y += add_in[r,:] / add_div
 *   if Y:          Y[r,:] = y                               (fp32)
 *   if Y16:        Y16[r,:] = bf16(y), round to nearest even (the next layer's gather source: no cast pass between layers)
 *   if acc_out:    acc_out[r,:] = (acc_in[r,:] + y) / acc_div
 * At least one of Y, Y16, acc_out; add_in and acc_out in one launch: SPEX_ERR_UNSUPPORTED.  The result equals spex_spmm_f32's on Xw
 * BIT FOR BIT for every row of at most 1 024 entries, also under an edge mask on the handle (applied entry by entry with
 * spex_spmm_f32's rule: a dropped entry's gathered value is replaced by 0 and it re-reads a kept entry's source row, a kept value
 * is divided by keep_prob).  Rows beyond 1 024 entries leave one partial row per 64-entry segment in the handle's scratch and a small
 * second launch adds them in segment order (spex_spmm_f32's SPEX_HUB_FOLD=0 schedule; stream ordering of the scratch as there).
 * The launch reads the handle's task and chunk tables: no second copy of the matrix; a handle without them (a source table beyond a
 * 32-bit offset) returns SPEX_ERR_UNSUPPORTED.
 * Alignment: X16, Y16, Y, add_in, acc_in, acc_out 16-byte aligned (the kernel itself needs 2 bytes for a gathered element and 8
 * for the rows it writes four columns at a time; 16 is what every row of a contiguous [*, 64] tensor has).  acc_in may equal acc_out;
 * X16 must not alias an output, nor the outputs each other.  All checks run before anything touches the device: NULL X16 / graph, no
 * output, aliasing, misalignment, a zero divisor -> SPEX_ERR_INVALID.
 */
int spex_spmm_bf16_f32(const spex_graph_t *g, const uint16_t *X16, float *Y, uint16_t *Y16, const float *add_in, float add_div,
                       const float *acc_in, float *acc_out, float acc_div, int32_t d, void *stream);

/* spex_propagate_f32 with bf16 gather sources (n_rows == n_cols):
 *   E16^0 = bf16(E0);   y_l = A E16^(l-1) in fp32 (l = 1..L);   E16^l = bf16(y_l) for l < L (written by launch l itself);
 *   mean_out = (E0 + y_1 + ... + y_L) / (L+1).
 * The running sum takes the EXACT fp32 E0 and the fp32 products y_l, formed by the acc_out epilogue exactly as spex_propagate_f32
 * forms it (acc_div = L+1 on the last launch): rounding enters only through the gather sources.  One cast launch + L SpMM launches;
 * bit-identical to spex_cast_bf16_f32 followed by L spex_spmm_bf16_f32 calls (Y16, acc_out).  L == 0: mean_out = E0.
 * ws16: 2 * n_rows * d bf16 elements (ping-pong gather tables).  E0, mean_out, ws16: distinct, 16-byte aligned.
 */
int spex_propagate_bf16_f32(const spex_graph_t *g, const float *E0, float *mean_out, uint16_t *ws16 /* 2 * n_rows * d */, int32_t L,
                            int32_t d, void *stream);

/* Backward of the above w.r.t. E0, straight-through (the rounding of a gather source is treated as the identity):
 *   G_L = g_out/(L+1);   G_l = g_out/(L+1) + A^T bf16(G_(l+1));   grad_E0 = G_0
 * — g_out/(L+1) is formed once in fp32 (ws) and is every launch's add_in operand (add_div = 1); its rounding is the first gather
 * source and each launch but the last writes bf16(G_l) for the next; the last writes grad_E0 in fp32.  gt: the handle of A^T.
 * ws: n_rows * d floats; ws16: 2 * n_rows * d bf16 elements.  g_out, grad_E0, ws, ws16: distinct, 16-byte aligned.  L == 0: a copy.
 */
int spex_propagate_bwd_bf16_f32(const spex_graph_t *gt, const float *g_out, float *grad_E0, float *ws /* n_rows * d */,
                                uint16_t *ws16 /* 2 * n_rows * d */, int32_t L, int32_t d, void *stream);

/* ------------------------------------------------------------------------------------------------ scoring
 * Replaces LightGCN.forward, utility1/model.py:111-121 (gather rows, elementwise product, sum, BCEWithLogitsLoss)
 * and NGCF compute_rec_loss, NGCF_SPEX/code/main_rec.py:89-91,96-100 — plus their autograd backward into the two
 * gathered tables.
 *   gamma[b] = <users[u_idx[b]], items[i_idx[b]]>
 *   labels != NULL: loss_sum += sum_b BCEWithLogits(gamma[b], labels[b])     (caller divides by B; *loss_sum must be
 *                   zeroed by the caller, it is accumulated with atomics)
 *   grad_users/grad_items != NULL: grad_users[u_idx[b],:] += dg_b * items[i_idx[b],:], grad_items likewise, with
 *                   dg_b = (sigmoid(gamma[b]) - labels[b]) * grad_scale   (grad_scale = upstream_grad / B).
 *                   The grad tables are accumulated into (atomics): zero them first.
 * ldu / ldi: row strides (floats) of users / items and of their grad tables (d for LightGCN, 2d.. for NGCF concat).
 * u_idx, i_idx: device int64 (what torch DataLoader hands over, main_rec.py:33-34).
 * n_user_rows / n_item_rows: table heights; a sample whose index falls outside is skipped (gamma = NaN) instead of
 * gathering out of bounds.
 */
int spex_score_bce_f32(const float *users, const float *items, int32_t ldu, int32_t ldi, int64_t n_user_rows,
                       int64_t n_item_rows, const int64_t *u_idx, const int64_t *i_idx, const float *labels, int32_t B,
                       int32_t d, float *gamma, float *loss_sum, float *grad_users, float *grad_items,
                       float grad_scale, void *stream);

/* The same scoring with the gradient ALSO (or only) as per-sample rows: grad_slots [2B, ld_slots], row b = d loss / d
 * users[u_idx[b]] of sample b alone (= dg_b * items[i_idx[b]]), row B + b = d loss / d items[i_idx[b]] of sample b — plain
 * stores, no atomics.  These are the operands of the row-sparse backward (spex_spmm_push_batch_f32,
 * spex_ngcf_layer_bwd_rows_f32).  grad_users / grad_items may be NULL (no table form wanted).
 */
int spex_score_bce_slots_f32(const float *users, const float *items, int32_t ldu, int32_t ldi, int64_t n_user_rows,
                             int64_t n_item_rows, const int64_t *u_idx, const int64_t *i_idx, const float *labels, int32_t B,
                             int32_t d, float *loss_sum, float *grad_users, float *grad_items, float grad_scale,
                             float *grad_slots, int32_t ld_slots, void *stream);

/* North-star extension (no counterpart in the reference): BPR over (u, i+, i-) triples.
 *   x_t = <U_read[u], I_read[i-] - I_read[i+]>;  loss_sum += softplus(x_t)
 * Fused gather + dot + sigmoid + SGD: with s_t = sigmoid(x_t)/T,
 *   U_w[u]  -= lr * (s_t (i- - i+) + reg u / T);  I_w[i+] -= lr * (-s_t u + reg i+ / T);  I_w[i-] -= lr * (s_t u + reg i- / T)
 * Batch-synchronous when the read tables differ from the write tables; passing the same tables gives in-place
 * (hogwild) matrix-factorisation BPR.  Updates use float atomics (duplicates in a batch accumulate).
 */
int spex_bpr_sgd_step_f32(const float *U_read, const float *I_read, float *U_w, float *I_w, int64_t n_user_rows,
                          int64_t n_item_rows, const int64_t *u, const int64_t *i_pos, const int64_t *i_neg, int64_t T,
                          int32_t d, float lr, float reg, float *loss_sum, void *stream);

/* The same triples scored for autograd instead of a fused update (bpr_loss() of the drop-in model):
 *   loss_sum += sum_t softplus(x_t);  grad_users[u] += grad_scale * sigmoid(x_t) (i- - i+);
 *   grad_items[i+] -= grad_scale * sigmoid(x_t) u;  grad_items[i-] += grad_scale * sigmoid(x_t) u.
 * grad tables may be NULL (loss only).  Accumulates with atomics: zero loss_sum / grad tables first.
 */
int spex_bpr_loss_f32(const float *users, const float *items, int64_t n_user_rows, int64_t n_item_rows,
                      const int64_t *u, const int64_t *i_pos, const int64_t *i_neg, int64_t T, int32_t d,
                      float *loss_sum, float *grad_users, float *grad_items, float grad_scale, void *stream);

/* The two BPR entry points above without one float atomic per gathered row, for large batches (d == 64).  The batch's
 * 3 T row updates are binned on the device by destination row (buckets of 64 rows of the joint [users | items] index
 * space, two-phase counting partition), accumulated per bucket in LDS and flushed to the tables once per touched row —
 * the arithmetic and the result (up to fp32 re-association of a row's contributions) are those of spex_bpr_sgd_step_f32 /
 * spex_bpr_loss_f32, which stay the right call below ~16 k triples (one launch, latency-bound).
 * Batch-synchronous only: the read tables must differ from the updated ones.
 * ws: caller-owned device scratch, 256-byte aligned, at least spex_bpr_grouped_workspace_bytes(T, n_user_rows,
 * n_item_rows) bytes; that function returns 0 when the grouped form does not apply (more than 8192 * 64 rows, T >= 2^30):
 * use the atomic form then.  Four launches on `stream`, no host synchronisation, no allocation.
 */
int64_t spex_bpr_grouped_workspace_bytes(int64_t T, int64_t n_user_rows, int64_t n_item_rows);
int spex_bpr_sgd_step_grouped_f32(const float *U_read, const float *I_read, float *U_w, float *I_w, int64_t n_user_rows,
                                  int64_t n_item_rows, const int64_t *u, const int64_t *i_pos, const int64_t *i_neg,
                                  int64_t T, int32_t d, float lr, float reg, float *loss_sum, void *ws, int64_t ws_bytes,
                                  void *stream);
int spex_bpr_loss_grouped_f32(const float *users, const float *items, int64_t n_user_rows, int64_t n_item_rows,
                              const int64_t *u, const int64_t *i_pos, const int64_t *i_neg, int64_t T, int32_t d,
                              float *loss_sum, float *grad_users, float *grad_items, float grad_scale, void *ws,
                              int64_t ws_bytes, void *stream);

/* Owner-computes exchange of a batch's rows on a 1-D row-partitioned table ("replicate the batch on all
 * ranks (owner-computes, no comm)" needs the batch's rows of the propagated table everywhere).  pos: device int64[K]
 * positions in the padded global row layout; this rank owns positions [lo, lo + n_local) = rows of `table`.
 *   gather : out[k,:] = owned(pos[k]) ? table[pos[k]-lo,:] : 0      -> one all-reduce (sum) of `out` completes it
 *   scatter: table[pos[k]-lo,:] += upd[k,:] for the owned k (atomics: positions repeat), then upd[k,:] = 0 if clear_upd
 */
int spex_gather_owned_rows_f32(const float *table, const int64_t *pos, int64_t K, int64_t lo, int64_t n_local, int32_t d,
                               float *out, void *stream);
int spex_scatter_add_owned_rows_f32(float *upd, const int64_t *pos, int64_t K, int64_t lo, int64_t n_local, int32_t d,
                                    float *table, int32_t clear_upd, void *stream);

/* ------------------------------------------------------------------------------------------------ optimiser
 * Replaces torch.optim.Adam(...).step() over the dense embedding tables — LightGCN_SPEX/code/main_rec.py:23,37.
 * One fused pass: m, v, p updated in place (bias-corrected, eps outside the sqrt as torch does), t = step count >= 1.
 * zero_buf (optional, n floats; may be g itself, may not alias p, m or v): cleared in the same pass — the caller's
 * gradient accumulation table for the next step (saves a separate fill launch per step).
 */
int spex_adam_step_f32(float *p, const float *g, float *m, float *v, int64_t n, int32_t t, float lr, float beta1,
                       float beta2, float eps, float *zero_buf, void *stream);

/* Row-sparse ("lazy") Adam over [n_rows, 64] tables: the update above, by the same code and therefore with the same roundings, at the
 * rows list[k], k < min(*count, max_count), and nowhere else — p, m, v of every other row are neither read nor written; t is the
 * global step count.  list, count: device memory (a spex_unique_rows_i32 / spex_frontier_rows_i32 list); entries must be distinct;
 * values outside [0, n_rows) are skipped.  The count is read on the device; a fixed grid strides over the list (max_count may be as
 * loose a bound as n_rows).  The masking law of torch.optim.SparseAdam with torch.optim.Adam's placement of eps (SparseAdam itself
 * puts eps elsewhere: no bit-level oracle).  d != 64: SPEX_ERR_UNSUPPORTED.  Pointers 16-byte aligned; p, g, m, v four buffers.
 * spex_zero_rows_f32: x[list[k], 0 .. d) = 0 for the same k (d a multiple of 4, x 16-byte aligned); other rows are not written. */
int spex_adam_rows_f32(float *p, const float *g, float *m, float *v, const int32_t *list, const int32_t *count, int32_t max_count,
                       int32_t n_rows, int32_t d, int32_t t, float lr, float beta1, float beta2, float eps, void *stream);
int spex_zero_rows_f32(float *x, const int32_t *list, const int32_t *count, int32_t max_count, int32_t n_rows, int32_t d, void *stream);

/* The same update for a small parameter block whose gradient arrives as n_parts partial blocks (block j at g_parts +
 * j * part_stride): g = the blocks added up in order, then Adam.  Used for NGCF's layer weights, whose gradient leaves
 * spex_ngcf_layer_bwd_rows_f32 as one block per workgroup.
 */
int spex_adam_step_sum_f32(float *p, const float *g_parts, int32_t n_parts, int64_t part_stride, float *m, float *v, int64_t n,
                           int32_t t, float lr, float beta1, float beta2, float eps, void *stream);

/* Validation hook for the NGCF entries' message dropout: while d_keep != NULL (per host thread), every NGCF layer entry called with
 * p_drop > 0 keeps element (row, col) iff d_keep[row' * 64 + col] != 0 (row' = the row in the reference's numbering, see pad_row)
 * instead of the counter-based draw — so that a run can use the REFERENCE's own nn.Dropout noise (main_rec.py:81:
 * `torch.empty(N, 64).bernoulli_(1 - p)` from the global CPU generator, drawn by the host where the reference draws it and uploaded
 * as bytes).  The pointer is read when a launch is queued; NULL restores the counter-based masks. */
int spex_ngcf_message_mask(const uint8_t *d_keep);

/* ------------------------------------------------------------------------------------------------ NGCF layer
 * Replaces NGCF_SPEX/code/main_rec.py:77-83 for one layer, given side = A ego from spex_spmm_f32 (:76):
 *   s    = LeakyReLU(side W_gc^T + b_gc);  b = LeakyReLU((ego * side) W_bi^T + b_bi);  e1 = dropout_p(s + b)
 *   out[r, 0:d] = ego[r,:] (iff write_ego);  out[r, d:2d] = e1 / max(||e1||_2, 1e-12)
 * W_*: [d,d] row-major as nn.Linear stores them (out x in); d == 64.  `out` has row stride ld_out >= 2d: layer l of a
 * deeper model passes out + l*d with write_ego = 0 and lands in its slice of the concatenated table (:85).
 * e1_out (optional, [n,d]) receives e1 after dropout — the next layer's input (:80-81).
 * Message dropout (:81, nn.Dropout(p_drop), training only; p_drop = 0 switches it off) is counter-based so that the
 * backward call reproduces the mask from (seed, step, layer) without storing it: element e = row*64 + col keeps iff
 * u_e >= p_drop, u_e = (word[e & 3] of philox4x32-10(counter = (e >> 2, step, layer, 0), key = seed) >> 8) * 2^-24; kept
 * values are multiplied by 1/(1 - p_drop).  pad_row >= 0: rows above it count one less when numbering elements (a table
 * that keeps the reference's unused pad user row, main_rec.py:67, as an isolated node; -1 = none).
 */
int spex_ngcf_layer_fwd_f32(const float *ego, const float *side, const float *W_gc, const float *b_gc, const float *W_bi,
                            const float *b_bi, float *out, int32_t ld_out, int32_t write_ego, float *e1_out, int32_t n,
                            int32_t d, float slope, float p_drop, uint64_t seed, uint32_t step, uint32_t layer,
                            int32_t pad_row, void *stream);
/* The same layer at a LIST of rows only: slot k names row idx_a[k] + off_a (k < n_a) or idx_b[k - n_a] + off_b.  `ego`, `side`
 * and `out` are the dense tables, read / written at those rows (other rows of `out` are left untouched; a row named twice is
 * stored twice with the same value; an index outside [0, n) is skipped); the dropout mask is indexed by the row.  A one-layer
 * model's training loss reads the layer's output at the batch's rows only (main_rec.py:96-104): with spex_spmm_rowlist_f32 for
 * `side` this replaces the whole-table forward of a training step (2B rows instead of N).  Bit-identical rows.
 */
int spex_ngcf_layer_fwd_rows_f32(const float *ego, const float *side, const float *W_gc, const float *b_gc, const float *W_bi,
                                 const float *b_bi, float *out, int32_t ld_out, int32_t write_ego, int32_t n, int32_t d, float slope,
                                 float p_drop, uint64_t seed, uint32_t step, uint32_t layer, int32_t pad_row, const int64_t *idx_a,
                                 int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b, void *stream);
/* The same layer in inference form (dropout off, ego written): kept for ABI-1 callers. */
int spex_ngcf_layer_f32(const float *ego, const float *side, const float *W_gc, const float *b_gc, const float *W_bi,
                        const float *b_bi, float *out, int32_t ld_out, float *e1_out, int32_t n, int32_t d,
                        float slope, void *stream);
/* Autograd backward of the layer (loss.backward(), main_rec.py:127).  The layer is recomputed from (ego, side), nothing
 * else of the forward is kept.  Upstream: g_norm = d loss / d out[:, d:2d] (row stride ld_g), g_next = d loss / d e1
 * ([n,d], from the next layer's call; NULL for the last layer), g_direct = d loss / d out[:, 0:d] (row stride
 * ld_direct; layer 0 only, else NULL).  Writes, for every row,
 *   g_side = d loss / d side   and   g_ego = the part of d loss / d ego that does not pass through side (+ g_direct);
 * the caller completes d loss / d ego = g_ego + A^T g_side with spex_spmm_f32(A^T, g_side, add_in = g_ego).
 * gW_gc, gb_gc, gW_bi, gb_bi ([d,d], [d]) are ACCUMULATED (zero them first) — since ABI 5 without a float atomic: every workgroup
 * leaves its share as one block of a per-(device, stream) scratch the library keeps, and a second small launch adds the blocks to
 * the four arrays in block order (deterministic; plain read-modify-write: two calls that accumulate into the SAME arrays must be
 * ordered, e.g. on one stream).  The scratch is allocated on the first call at a size (not inside a stream capture).
 * Rows whose upstream gradients are all zero (after a 256-sample batch: most) cost a read and two zero rows.
 */
int spex_ngcf_layer_bwd_f32(const float *ego, const float *side, const float *W_gc, const float *b_gc, const float *W_bi,
                            const float *b_bi, const float *g_norm, int32_t ld_g, const float *g_next,
                            const float *g_direct, int32_t ld_direct, int32_t n, int32_t d, float slope, float p_drop,
                            uint64_t seed, uint32_t step, uint32_t layer, int32_t pad_row, float *g_side, float *g_ego,
                            float *gW_gc, float *gb_gc, float *gW_bi, float *gb_bi, void *stream);

/* The same backward for the rows of a BATCH only — the form the LAST layer takes in training: after a B-sample batch
 * only the batch's <= 2B rows carry a gradient behind it (main_rec.py:89-90), so 2B / 16 tiles replace n / 16.
 * The batch is given as it is scored: slot k < n_a is row idx_a[k] + off_a, slot n_a + k is row idx_b[k] + off_b (device
 * int64).  EVERY slot is processed with its own upstream gradient rows — g_norm_c / g_direct_c are COMPACT, row k = slot k,
 * exactly what spex_score_bce_slots_f32 writes (the layer's backward is linear in them: a row named by several slots
 * simply gets several contributions downstream; nothing is deduplicated and no gradient table is involved).
 * g_side_c / g_ego_c: COMPACT outputs [n_a + n_b, d] — the operands of spex_spmm_push_batch_f32, which completes
 * d loss / d ego = scatter(g_ego_c) + A^T scatter(g_side_c).
 * Weight gradients leave as spex_ngcf_layer_bwd_rows_parts(n_a + n_b) partial blocks (one per 16-slot tile), block j at
 * gW_parts + j * part_stride, each laid out [dW_gc d*d | db_gc d | dW_bi d*d | db_bi d] (plain stores): add them up —
 * spex_adam_step_sum_f32 does, inside the optimiser pass.
 */
int32_t spex_ngcf_layer_bwd_rows_parts(int32_t n_slots);
int spex_ngcf_layer_bwd_rows_f32(const float *ego, const float *side, const float *W_gc, const float *b_gc,
                                 const float *W_bi, const float *b_bi, const float *g_norm_c, int32_t ld_g,
                                 const float *g_next, const float *g_direct_c, int32_t ld_direct, int32_t n, int32_t d,
                                 float slope, float p_drop, uint64_t seed, uint32_t step, uint32_t layer, int32_t pad_row,
                                 const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b,
                                 int64_t off_b, float *g_side_c, float *g_ego_c, float *gW_parts, int32_t part_stride,
                                 void *stream);

/* ------------------------------------------------------------------------------------------------ row-sparse backward
 * After a B-sample batch d loss / d (propagated table) is non-zero on <= 2B rows (model.py:115-116), so the FIRST product
 * of the backward pass, A^T g, touches only the stored entries of those rows (~14 k of Epinion2's 418 k): it is taken
 * in push form instead of a pull-form SpMM over the whole matrix ("hard parts").
 *
 * spex_unique_rows_i32: the distinct values of { idx_a[k] + off_a } U { idx_b[k] + off_b } that lie in [0, n_rows), as a
 * compact device list (arbitrary order) and its length.  stamp: caller-owned device int32[n_rows], zero-initialised once;
 * epoch: any non-zero value not used on this stamp table before (a step counter).  No sort, no host round trip.
 *
 * spex_spmm_push_rows_f32: for the k-th listed row r = list[k] (k < *count) and every stored entry e of row r of the handle:
 *   out[col[e], :] += scale * val[e] * src_k,   src_k = src[r, :] if src_indexed else src[k, :]
 *   and, if add: out[r, :] += scale * add_k (same indexing rule by add_indexed)
 * i.e. out += scale * (A^T scatter(src) + scatter(add)) for the matrix A held by the handle (scale = 1/(L+1) gives the
 * first step of the layer-mean's backward, G = (g + A^T g)/(L+1), in one launch).  out: [n_cols, d], accumulated with
 * 256-byte float atomics — initialise it first (zero, or the term the product is added to).  max_count bounds the launch
 * (one 16-wave workgroup per list slot).  A mask on the handle (edge dropout) is applied entry by entry (a kernel of its own): a
 * kept value is val[e] / keep_prob, a dropped entry issues no atomic — out += scale * (A_m^T scatter(src) + scatter(add)) for the
 * masked matrix A_m, the forward's mask.
 */
int spex_unique_rows_i32(const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b,
                         int32_t n_rows, int32_t *stamp, int32_t epoch, int32_t *list, int32_t *count, void *stream);
int spex_spmm_push_rows_f32(const spex_graph_t *g, const int32_t *list, const int32_t *count, int32_t max_count,
                            const float *src, int32_t src_indexed, const float *add, int32_t add_indexed, float scale,
                            float *out, int32_t d, void *stream);
/* spex_spmm_push_rows_f32 with a factor of its own for the add term: out += scale * A^T scatter(src) + add_scale * scatter(add)
 * (G_(l-1) = g / (L + 1) + A^T G_l over a frontier list: scale = 1, add_scale = 1 / (L + 1)).  Both calls run a grid of
 * min(max_count, 65 536) workgroups that strides over the list, so max_count may be as loose a bound as n_rows. */
int spex_spmm_push_rows_scaled_f32(const spex_graph_t *g, const int32_t *list, const int32_t *count, int32_t max_count,
                                   const float *src, int32_t src_indexed, const float *add, int32_t add_indexed, float scale,
                                   float add_scale, float *out, int32_t d, void *stream);
/* The frontier of a batch.  On entry list[0 .. *count_b) is what spex_unique_rows_i32 wrote with the same stamp table and the same
 * epoch (Bset, the batch's distinct rows; max_b >= *count_b bounds the launch: the batch's slot count).  The call appends, into the
 * same list, every column of a stored entry of those rows that the stamp table has not seen this epoch, and writes the new length
 * to *count_f (a cell other than count_b, which is left alone): afterwards the list is [Bset | F1 minus Bset] with
 * F1 = Bset U { col[e] : e a stored entry of a row in Bset }, *count_b = |Bset| and *count_f = |F1|, both on the device.
 * Every row enters the list at most once per epoch, so a list of n_rows entries always suffices: there is no overflow path.  The
 * launch reads its input length from count_b and appends through count_f, so it never walks a row it appended itself (that would
 * be the two-hop set).  No sort, no host round trip, no clearing of the stamp table between steps (the epoch does that).  The graph
 * must be square (the list indexes rows and columns alike); one wave per input row, one counter bump per wave and 64-entry run. */
int spex_frontier_rows_i32(const spex_graph_t *g, int32_t *list, const int32_t *count_b, int32_t max_b, int32_t *stamp, int32_t epoch,
                           int32_t *count_f, void *stream);
/* The frontier of a batch under the handle's edge-dropout mask: spex_frontier_rows_i32 with "stored entry" read as "stored entry
 * that the mask KEEPS" (spex_graph_set_edge_mask's rule, decided per entry by its edge id: the decision every masked product of the
 * step makes) — F1 = Bset U { col[e] : e a stored and kept entry of a row in Bset }.  A dropped entry does not stamp its column: a
 * column reached over a dropped and a kept entry is listed.  On a handle without a mask the call is spex_frontier_rows_i32;
 * spex_frontier_rows_i32 itself lists every stored column whatever the mask.  Same arguments, same errors. */
int spex_frontier_rows_masked_i32(const spex_graph_t *g, int32_t *list, const int32_t *count_b, int32_t max_b, int32_t *stamp, int32_t epoch,
                                  int32_t *count_f, void *stream);
/* The push over a LONG device list (a two-hop frontier; SPEX_STEP_FRONTIER_DEEP's second backward product):
 *   out[col[e], :] += scale * val[e] * src[r, :]  for every stored entry e of every row r = list[k], k < min(*count, max_count)
 * — spex_spmm_push_rows_f32's product with src indexed by row and no add term, in spex_spmm_rowlist_dev_f32's work split: a fixed grid
 * (<= 2 048 workgroups of 16 list slots per pass) strides over the list, the count is read on the device, a row of at most 64 entries
 * is one wave's task and longer rows are cut into 64-entry wave tasks dealt to the workgroup's 16 waves.  Every atomic
 * wave-instruction adds one contiguous 256-byte row of out.  list values outside [0, n_rows) are skipped; entries should be distinct
 * (a row listed twice is pushed twice).  out: [n_cols, 64], initialised by the caller; src: [n_rows, 64], not out.  A mask on the
 * handle (edge dropout) is applied entry by entry by a kernel of its own: a kept value is val / keep_prob, a dropped entry issues no
 * atomic.  d == 64 only: otherwise SPEX_ERR_UNSUPPORTED.  Sums arrive in arbitrary order (float atomics). */
int spex_spmm_push_list_f32(const spex_graph_t *g, const int32_t *list, const int32_t *count, int32_t max_count, const float *src,
                            float scale, float *out, int32_t d, void *stream);
/* spex_spmm_rowlist_f32 driven by such a device list: rows list[k], k < min(*count, max_count), entries distinct (acc_out may
 * therefore alias acc_in); rows outside the list are not written; list values outside [0, n_rows) are skipped.  The same per-row
 * arithmetic and epilogue (Y = y; acc_out = (acc_in + y) / acc_div): bit-identical to spex_spmm_rowlist_f32, and to spex_spmm_f32
 * on rows of up to 1 024 entries.  The work split is the frontier's: a row of at most 64 entries is one wave's task, longer rows are
 * cut into one-segment wave tasks whose sums meet in LDS in segment order; a fixed grid (<= 1 024 workgroups of 16 list slots per
 * pass) strides over the list, the count is read on the device.  d == 64 only: otherwise SPEX_ERR_UNSUPPORTED.  A mask on the handle
 * (edge dropout) is applied entry by entry by a kernel of its own: per row the masked spex_spmm_f32's fmaf chain — a kept value is
 * val / keep_prob, a dropped entry stays in its place as fmaf(0, 0, acc), its source row is never multiplied — i.e. the masked
 * spex_spmm_f32's bits on rows of up to 1 024 stored entries; a listed row whose entries are all dropped is written as 0. */
int spex_spmm_rowlist_dev_f32(const spex_graph_t *g, const float *X, const int32_t *list, const int32_t *count, int32_t max_count,
                              float *Y, const float *acc_in, float *acc_out, float acc_div, int32_t d, void *stream);
/* spex_spmm_rowlist_dev_f32 gathering from a bf16 table X16 ([n_cols, 64], rows of 128 bytes; widening is exact): the same kernel body
 * instantiated for the other element type, so on Xw = float(X16) it returns in Y what spex_spmm_rowlist_dev_f32 returns on Xw, bit for
 * bit, for EVERY listed row (hubs included: the same segments are added in the same order) — hence spex_spmm_bf16_f32's rows on rows
 * of up to 1 024 entries.  Outputs, each optional but at least one given: Y (fp32), Y16 = bf16(the same register), round to nearest
 * even (= spex_cast_bf16_f32(Y) bit for bit), acc_out = (acc_in + y) / acc_div (may alias acc_in).  Rows outside the list are written
 * in no output; list values outside [0, n_rows) are skipped; *count is cut at max_count.  d != 64 or an edge mask on the handle ->
 * SPEX_ERR_UNSUPPORTED; a NULL graph / X16 / list / count, no output, acc_out without acc_in, X16 aliasing an output or acc_in, or
 * Y / Y16 aliasing each other or the running sum -> SPEX_ERR_INVALID. */
int spex_spmm_rowlist_dev_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const int32_t *list, const int32_t *count, int32_t max_count,
                                   float *Y, uint16_t *Y16, const float *acc_in, float *acc_out, float acc_div, int32_t d, void *stream);
/* The same product driven by the batch itself (d = 64, 128 or 256), EVERY slot contributing its own row: for slot k with row
 * r = idx_a[k] + off_a (k < n_a) or idx_b[k - n_a] + off_b:
 *   out[col[e], :] += scale * val[e] * src[k, :]  over the stored entries e of row r;   out[r, :] += scale * add[k, :] (if add)
 * src / add are COMPACT per-slot arrays (row strides ld_src / ld_add) — the per-sample gradient rows
 * spex_score_bce_slots_f32 writes, or spex_ngcf_layer_bwd_rows_f32's outputs; rows named by several slots receive several
 * contributions, so nothing is deduplicated.  ONE launch (each small launch costs ~4 us on the stream: a fill + a
 * unique pass + the list form would cost more than the pull-form SpMM they replace); a slot's row is shared by 4
 * workgroups of 4 waves, so a hub row's atomics spread over several CUs.
 */
int spex_spmm_push_batch_f32(const spex_graph_t *g, const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b,
                             int32_t n_b, int64_t off_b, const float *src, int32_t ld_src, const float *add, int32_t ld_add,
                             float scale, float *out, int32_t d, void *stream);

/* The batch-sized middle of the exact LightGCN training step (L >= 2, d = 64, 128 or 256) as ONE launch (under edge dropout — a mask set on the
 * handle with spex_graph_set_edge_mask — the last layer at the batch's rows and the push apply the handle's keep rule entry by entry,
 * exactly as spex_spmm_f32 does: kept values / keep_prob, dropped entries contribute nothing): what the
 * sequence spex_spmm_rowlist_f32 -> spex_score_bce_slots_f32 -> spex_spmm_push_batch_f32 computes, i.e. for sample b with
 * rows u = users[b], i = items[b] + n_user_rows (utility1/model.py:91-97 at the batch's rows, :111-121, and autograd's first
 * backward product):
 *   light_r = (acc_in[r] + (A X)[r]) / acc_div   for r in {u, i}   — the last layer + layer mean at the two rows (same segment
 *                                                                     order as spex_spmm_rowlist_f32: bit-identical rows,
 *                                                                     and for rows of <= 1 024 entries spex_spmm_f32's at this d)
 *   x = <light_u, light_i>;   loss_b = BCEWithLogits(x, labels[b]);   dg = (sigmoid(x) - labels[b]) * grad_scale
 *   loss_per_sample[b] = loss_b (plain store) if loss_per_sample != NULL, else *loss_sum += loss_b (one atomic per sample)
 *   g_u = dg * light_i,  g_i = dg * light_u
 *   g_out[r] += g_r                                                  — dense d loss / d light_out (atomics: rows repeat)
 *   G[r] += push_scale * g_r;  G[col[e]] += push_scale * val[e] * g_r over the stored entries e of row r of `g` ITSELF:
 *                                                                    G = push_scale (g + A^T g), and A^T g in push form walks
 *                                                                    the rows of A — (A^T g)[c] = sum_r A[r, c] g[r]
 * g_out and G are accumulated into: zero them first (the step's Adam pass does).  Samples with an index out of range are
 * skipped (loss 0).  Up to SPEX_BATCH_PARTS workgroups (default 3) share a sample whose rows are long (their pushes' atomics
 * then come from several CUs).  d = 128 / 256 (X, acc_in 16-byte aligned): a lane gathers 2 / 4 consecutive columns, a segment's
 * gathers are in flight 32 / 16 at a time, the push issues 2 / 4 256-byte atomics per stored entry.
 */
int spex_lightgcn_batch_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div,
                            const int64_t *users, const int64_t *items, const float *labels, int32_t B, int32_t n_user_rows,
                            float grad_scale, float push_scale, float *loss_sum, float *loss_per_sample, float *g_out, float *G,
                            int32_t d, void *stream);
/* The same launch without the push and without any float atomic (the deterministic step): light_r, x, loss_b, dg as above, then
 *   grad_slots[b] = g_u,  grad_slots[B + b] = g_i      ([2B, d] per-sample rows, plain stores; out-of-range samples: zeros)
 * spex_reduce_slots_f32 then adds the slots per table row in ascending slot order. */
int spex_lightgcn_batch_slots_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const int64_t *users,
                                  const int64_t *items, const float *labels, int32_t B, int32_t n_user_rows, float grad_scale,
                                  float *loss_sum, float *loss_per_sample, float *grad_slots, int32_t d, void *stream);

/* The batch-sized middle of the exact BPR step as ONE launch — the three-row sibling of spex_lightgcn_batch_f32, d == 64 ONLY
 * (d = 128 / 256 are rejected here: spex_lightgcn_bpr_batch_wide_f32 below takes them).  Triple t has rows u = users[t], p = n_user_rows + pos[t],
 * n = n_user_rows + neg[t]:
 *   light_r = (acc_in[r] + (A X)[r]) / acc_div for the three rows (bit-identical to spex_spmm_f32 / spex_spmm_rowlist_f32 for rows
 *             of <= 1 024 entries, also under an edge mask on the handle)
 *   xp = <light_u, light_p>, xn = <light_u, light_n>, z = xn - xp;  dg = sigmoid(z) * grad_scale
 *   loss_t = max(z, 0) + log1p(exp(-|z|)) [+ 0.5 * weight_decay * (|E0[u]|^2 + |E0[p]|^2 + |E0[n]|^2) when weight_decay > 0]
 *   loss_per_sample[t] = loss_t if loss_per_sample != NULL, else *loss_sum += loss_t (one atomic per triple)
 *   g_u = dg (light_n - light_p), g_p = -dg light_u, g_n = dg light_u
 *   g_out[r] += g_r where g_out != NULL;  G[r] += push_scale g_r, G[col[e]] += push_scale val[e] g_r over the stored entries of
 *   the three rows of `g` (the push form of A^T g) where G != NULL (at least one of the two).  Both are accumulated into: zero them first.
 *   row_counts != NULL (int32 [N]): row_counts[r] += 1 per occurrence of r in the batch — the weight of the L2 gradient
 *   weight_decay / T * E0[r], which the caller's optimizer pass applies.  E0 may be NULL when weight_decay == 0.
 * A triple with any index out of range is skipped whole: loss 0, no gradient, no count. */
int spex_lightgcn_bpr_batch_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const int64_t *users,
                                const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows, float grad_scale,
                                float push_scale, float weight_decay, const float *E0, int32_t *row_counts, float *loss_sum,
                                float *loss_per_sample, float *g_out, float *G, int32_t d, void *stream);
/* The same launch without the push and without any float atomic (the deterministic step):
 *   grad_slots[t] = g_u, grad_slots[T + t] = g_p, grad_slots[2 T + t] = g_n   ([3 T, 64], plain stores; skipped triples: zeros) */
int spex_lightgcn_bpr_batch_slots_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const int64_t *users,
                                      const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows, float grad_scale,
                                      float weight_decay, const float *E0, int32_t *row_counts, float *loss_sum, float *loss_per_sample,
                                      float *grad_slots, int32_t d, void *stream);
/* The same two launches at d = 128 / 256 ONLY (any other d is rejected; d == 64 takes the two entry points above, which promised 64
 * and keep rejecting everything else — a caller whose tables are 64 wide must not be able to ask for a wider gather by accident).
 * Same arguments, same arithmetic per column; X, acc_in and E0 must be 16-byte aligned (rows move as dwordx2 / dwordx4 per lane).
 * A row of <= 1 024 entries is bit-identical to spex_spmm_f32's row at this width, also under an edge mask; a dot product is a lane's
 * d / 64 products (columns lane, lane + 64, ..) in ascending order and then a fixed tree; the push issues d / 64 row atomics of 256
 * bytes per stored entry.  grad_slots: [3 T, d]. */
int spex_lightgcn_bpr_batch_wide_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const int64_t *users,
                                     const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows, float grad_scale,
                                     float push_scale, float weight_decay, const float *E0, int32_t *row_counts, float *loss_sum,
                                     float *loss_per_sample, float *g_out, float *G, int32_t d, void *stream);
int spex_lightgcn_bpr_batch_slots_wide_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div,
                                           const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows,
                                           float grad_scale, float weight_decay, const float *E0, int32_t *row_counts, float *loss_sum,
                                           float *loss_per_sample, float *grad_slots, int32_t d, void *stream);

/* Deterministic accumulation of a batch's per-slot rows into a dense [n_rows, d] table — replaces the float atomics of the row-
 * sparse backward where results must repeat bit for bit (and follows the order of the reference's CPU `index_put_(accumulate)` /
 * index_select backward, LightGCN_SPEX/code/utility1/model.py:115-116 and NGCF_SPEX/code/main_rec.py:89-90 under autograd):
 *   slot k names row r_k = idx_a[k] + off_a (k < n_a) or idx_b[k - n_a] + off_b;
 *   out[r] = scale * (slots[k1] + slots[k2] + ...)  over the slots k1 < k2 < ... with r_k == r, added in ASCENDING slot order
 *   mode 0: out[r] is overwritten (rows no slot names are left alone);  mode 1: out[r] += the sum (plain read-modify-write: the
 *   wave that holds the lowest slot of a row owns it).  slots == NULL: the named rows are set to zero (clears what mode 0 wrote).
 * Rows out of range are skipped.  The duplicate scan is quadratic in the batch (n^2 * 8 bytes of cached reads): a validation-mode
 * kernel for the reference's batches of 256, not a throughput path.  d = 64, 128 or 256. */
int spex_reduce_slots_f32(const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b,
                          int32_t n_rows, const float *slots, int32_t ld_slots, float scale, float *out, int32_t mode, int32_t d,
                          void *stream);

/* Scoring + rows backward of the single-layer NGCF model as ONE launch (what spex_score_bce_slots_f32 followed by
 * spex_ngcf_layer_bwd_rows_f32 computes — NGCF_SPEX/code/main_rec.py:84-100 and autograd through :77-83 at the batch's rows):
 * sample b has rows u = users[b], i = n_user_rows + items[b] of the concatenated table all_emb [n, 2d] (= [ego | normalised layer
 * output], as spex_ngcf_layer_fwd_f32 writes it);  x = <all_emb[u], all_emb[i]>;  loss_per_sample[b] = BCEWithLogits(x, labels[b]);
 * dg = (sigmoid(x) - labels[b]) * grad_scale;  slot b (row u) receives the upstream gradient dg * all_emb[i], slot B + b (row i)
 * dg * all_emb[u] — first d columns: the direct gradient of `ego`, last d: the gradient of the normalised output — and the layer's
 * backward runs on those 2B slots exactly as in spex_ngcf_layer_bwd_rows_f32 (same outputs: g_side_c, g_ego_c [2B, d], gW_parts).
 * A sample with an index out of range contributes nothing (loss 0).  d == 64.
 */
int spex_ngcf_score_bwd_rows_f32(const float *ego, const float *side, const float *W_gc, const float *b_gc, const float *W_bi,
                                 const float *b_bi, const float *all_emb, const float *labels, float grad_scale, int32_t n, int32_t d,
                                 float slope, float p_drop, uint64_t seed, uint32_t step, uint32_t layer, int32_t pad_row,
                                 const int64_t *users, const int64_t *items, int32_t B, int64_t n_user_rows, float *loss_per_sample,
                                 float *g_side_c, float *g_ego_c, float *gW_parts, int32_t part_stride, void *stream);
/* The same WITHOUT the concatenated table: the layer's forward at the batch's rows, the scoring and the rows backward in one launch.
 * A tile of the kernel holds both rows of 8 samples (user rows and item rows of samples 8t .. 8t+7), so a sample's other row is in
 * the tile and x = <ego_u, ego_i> + <out_u, out_i> is formed from the layer output the kernel recomputes anyway (out = the
 * normalised, dropped-out layer output of main_rec.py:77-83 at that row).  Inputs: `ego` and `side` = A ego, dense tables read at the
 * batch's rows only (spex_spmm_rowlist_f32 provides `side` there).  Outputs as spex_ngcf_score_bwd_rows_f32 (slot b: users[b],
 * slot B + b: items[b]; gW_parts: spex_ngcf_layer_bwd_rows_parts(2 B) blocks).  With it a training step of the one-layer model
 * never materialises the layer's output.  d == 64.
 */
int spex_ngcf_fwd_score_bwd_rows_f32(const float *ego, const float *side, const float *W_gc, const float *b_gc, const float *W_bi,
                                     const float *b_bi, const float *labels, float grad_scale, int32_t n, int32_t d, float slope,
                                     float p_drop, uint64_t seed, uint32_t step, uint32_t layer, int32_t pad_row,
                                     const int64_t *users, const int64_t *items, int32_t B, int64_t n_user_rows,
                                     float *loss_per_sample, float *g_side_c, float *g_ego_c, float *gW_parts, int32_t part_stride,
                                     void *stream);

/* The forward half of the dual-task model's batch-sized middle (utility1/model_expert_s.py:95-126 at the batch's rows, :154-168)
 * as ONE launch — what spex_spmm_rowlist_f32 -> spex_expert_gate_rows_f32 -> spex_score_bce_slots_f32 compute: for sample b with
 * rows u = users[b], i = items[b] + n_user_rows:
 *   light_r = (acc_in[r] + (A X)[r]) / acc_div,  lo_batch[r] = light_r                       (r in {u, i}; lo_batch is [N, d])
 *   mixed_r = raw[r] * a0 + light_r * a1,  (a0, a1) = softmax([raw[r] | light_r] att)        (att_u for u, att_i for i)
 *   x = <mixed_u, mixed_i>;  loss_b = BCEWithLogits(x, labels[b]);  dg = (sigmoid(x) - labels[b]) * grad_scale
 *   loss_per_sample[b] = loss_b (plain store) if loss_per_sample != NULL, else *loss_sum += loss_b (one atomic per sample)
 *   grad_slots[b] = dg * mixed_i,  grad_slots[B + b] = dg * mixed_u                          ([2B, d], row stride d)
 * spex_expert_gate_rows_bwd_f32 and the push-form product follow as before.  d == 64; under edge dropout the last layer applies
 * the handle's keep rule (as spex_lightgcn_batch_f32 does).
 */
int spex_gated_batch_fwd_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const float *raw,
                             const float *att_u, const float *att_i, const int64_t *users, const int64_t *items, const float *labels,
                             int32_t B, int32_t n_user_rows, float grad_scale, float *loss_sum, float *loss_per_sample,
                             float *lo_batch, float *grad_slots, int32_t d, void *stream);

/* The WHOLE batch-sized middle of the dual-task rec branch as ONE launch: spex_gated_batch_fwd_f32's forward, then
 * spex_expert_gate_rows_bwd_f32 (the backward of model_expert_s.py:156-161 at the sample's two rows; linear in the incoming
 * gradient, so a row named by several samples is handled once per sample) and spex_spmm_push_batch_f32 (the first backward
 * product of the propagation, A^T g in push form over the rows of A) — three launches of a dependent chain in one kernel.
 * With d light_r / d raw_r the gate's two outputs for r in {u, i} (same arithmetic as the separate entries), it ACCUMULATES with
 * float atomics into caller-zeroed buffers:
 *   g_prop[r] += d light_r;  g_raw[r] += d raw_r;  G[r] += push_scale * d light_r;
 *   G[col[e]] += val[e] * push_scale * d light_r   over the stored entries e of row r of A;
 *   g_att[b mod n_att_copies] += the gate matrices' gradients;  *loss_sum += loss_b.
 * g_att: [n_att_copies][2][128, 2] — copy c holds [d att_u | d att_i] of the samples b = c (mod n_att_copies); the gradient is the
 * sum of the copies (all samples adding into ONE copy serialise in L2: 256 adds per word; 64 copies cost nothing).
 * g_prop, G, g_raw: [N, d], three distinct tables.  d == 64; under edge dropout the last layer and the push apply the handle's keep
 * rule.  (The deterministic step keeps the separate,
 * atomic-free entries.)
 */
int spex_gated_batch_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const float *raw,
                         const float *att_u, const float *att_i, const int64_t *users, const int64_t *items, const float *labels,
                         int32_t B, int32_t n_user_rows, float grad_scale, float push_scale, float *loss_sum, float *g_prop, float *G,
                         float *g_raw, float *g_att, int32_t n_att_copies, int32_t d, void *stream);

/* Replaces the two-expert gate of the dual-task model, utility1/model_expert_s.py:156-161:
 *   att = softmax([raw | prop] att_exp, dim=1) ([n,2d] x [2d,2]);  mixed = raw * att[:,0] + prop * att[:,1]
 */
int spex_expert_gate_f32(const float *raw, const float *prop, const float *att_exp /*[2d,2]*/, float *mixed, int32_t n,
                         int32_t d, void *stream);
/* Its autograd backward: grad_raw / grad_prop ([n,d]) are written; grad_att ([2d,2]) is ACCUMULATED (zero it first). */
int spex_expert_gate_bwd_f32(const float *raw, const float *prop, const float *att_exp, const float *grad_mixed,
                             float *grad_raw, float *grad_prop, float *grad_att, int32_t n, int32_t d, void *stream);
/* The same with the parameter gradient summed in a fixed order (no float atomics; d <= 128): every workgroup leaves its share in
 * its own block of att_parts — [spex_expert_gate_bwd_parts(n)][4 d] floats of caller-owned scratch — and the blocks are added to
 * grad_att in block order. */
int32_t spex_expert_gate_bwd_parts(int32_t n);
int spex_expert_gate_bwd_det_f32(const float *raw, const float *prop, const float *att_exp, const float *grad_mixed,
                                 float *grad_raw, float *grad_prop, float *grad_att, float *att_parts, int32_t n, int32_t d,
                                 void *stream);

/* The gate at a batch's rows only (the training loss reads the gated tables nowhere else, model_expert_s.py:163-166), d == 64.
 * Slot k names table row r = idx_a[k] + off_a (k < n_a) or idx_b[k - n_a] + off_b (raw / prop: [n_rows, 64] tables holding
 * users then items); rows below n_user_rows are gated with att_u (att_exp1), the others with att_i (att_exp2).
 *   forward : mixed_slots[k, :] = the gated row (compact [n_a + n_b, 64]); an out-of-range row gives zeros.
 *   backward: grad_slots[k, :] = d loss / d mixed_slots[k] (row stride ld_slots) ->
 *             grad_prop_slots[k, :] (compact, what spex_spmm_push_batch_f32 consumes) and, ACCUMULATED with atomics (zero them
 *             first): grad_prop[r, :] += d prop, grad_raw[r, :] += d raw (dense [n_rows, 64]), grad_att_u / grad_att_i ([128, 2]).
 *             A row named by several slots is handled once per slot (the gate's backward is linear in the incoming gradient).
 */
int spex_expert_gate_rows_f32(const float *raw, const float *prop, const float *att_u, const float *att_i, const int64_t *idx_a,
                              int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b, int64_t n_user_rows,
                              int64_t n_rows, int32_t d, float *mixed_slots, void *stream);
int spex_expert_gate_rows_bwd_f32(const float *raw, const float *prop, const float *att_u, const float *att_i, const int64_t *idx_a,
                                  int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b,
                                  int64_t n_user_rows, int64_t n_rows, int32_t d, const float *grad_slots, int32_t ld_slots,
                                  float *grad_prop_slots, float *grad_prop, float *grad_raw, float *grad_att_u, float *grad_att_i,
                                  void *stream);
/* The same backward without a float atomic (the deterministic step): grad_prop_slots AND grad_raw_slots leave as compact per-slot
 * rows ([n_a + n_b, 64]; spex_reduce_slots_f32 adds them per table row in slot order), and every workgroup writes its share of the
 * two gate gradients to its own block of att_parts — [spex_expert_gate_rows_bwd_parts(n_a + n_b)][512] floats, block p =
 * [d att_u (256) | d att_i (256)] — to be added in block order. */
int32_t spex_expert_gate_rows_bwd_parts(int32_t n_slots);
int spex_expert_gate_rows_bwd_det_f32(const float *raw, const float *prop, const float *att_u, const float *att_i, const int64_t *idx_a,
                                      int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b,
                                      int64_t n_user_rows, int64_t n_rows, int32_t d, const float *grad_slots, int32_t ld_slots,
                                      float *grad_prop_slots, float *grad_raw_slots, float *att_parts, void *stream);

/* ------------------------------------------------------------------------------------------------ negative sampler
 * Replaces LightTrainData.ng_sample, LightGCN_SPEX/code/utility1/dataloader.py:250-265 (distribution, not stream):
 * for each of n_pos positives (user d_pos_user[p]) draw num_ng items uniformly from [0, num_item), redrawing while the
 * item is in the user's sorted interaction list d_items[d_rowptr[u] : d_rowptr[u+1]] (CSR of R, device).
 * d_out: int64[n_pos * num_ng], slot p * num_ng + t.  Counter-based (philox4x32-10 keyed by `seed`): reproducible,
 * order-independent; not NumPy's stream (the host sampler of the drop-in Loader replays that one exactly).
 */
int spex_sample_negatives(const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows, const int64_t *d_pos_user,
                          int64_t n_pos, int32_t num_ng, int32_t num_item, uint64_t seed, int64_t *d_out, void *stream);

/* ------------------------------------------------------------------------------------------------ BPR triple sampler
 * One epoch's (user, positive, negative) triples drawn on the device — what trainer.bpr_epoch_triples draws on the host (law, not
 * stream).  d_rowptr int32[n_user_rows + 1] / d_items int32: CSR of R on the device, every row ascending without duplicates;
 * d_active int32[n_active]: the users with at least one stored item; num_item: catalogue size.  d_users / d_pos / d_neg: int64[n]
 * (the one-call BPR step's index type).  One thread per slot i in [0, n):
 *   mode 0, "by user" (upstream LightGCN's law):  user uniform over d_active, positive uniform over the user's stored items
 *   mode 1, "by interaction":  a stored entry e uniform over [0, nnz), nnz = d_rowptr[n_user_rows]; user = the row that holds e
 *                              (the last u with d_rowptr[u] <= e), positive = d_items[e] — users weighted by their degree
 *   negative (both modes): uniform over the items that are not among the user's stored items.
 * Randomness: standard Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85, ten rounds).
 *   key     = (seed & 0xFFFFFFFF, seed >> 32)
 *   counter = (i & 0xFFFFFFFF, i >> 32, epoch, stage)                 -> output words w0 w1 w2 w3
 *   a word w maps to [0, m) as floor(w * m / 2^32) (multiply-high)
 *   stage 0:  w0 -> the user's position in d_active (mode 0, m = n_active) or the entry e (mode 1, m = nnz)
 *             w1 -> the positive's position in the user's row (mode 0, m = the row's length; mode 1 does not read it)
 *             w2, w3 -> negative candidates 0 and 1 (m = num_item)
 *   stage 1:  w0 .. w3 -> negative candidates 2 .. 5; computed only when candidates 0 and 1 were both stored items of the user
 *   stage 2:  computed only when all six candidates were: w0 -> k (m = num_item - the row's length), the negative is the k-th item
 *             in ascending order that is not in the row (w1 .. w3 unused)
 *   The negative is the first candidate, in the order 0 .. 5, that is not in the user's row.
 * Slot i of (seed, epoch) is a function of i, seed, epoch and the tables alone — not of n, nor of the launch's shape: a draw of
 * n' < n slots is the first n' of the draw of n.  A user whose row holds every item has no negative: 0 is written (the tables of
 * trainer.bpr_sampler_tables exclude the case); an entry of d_active outside [0, n_user_rows) counts as a user with an empty row
 * (positive 0).  Returns SPEX_ERR_INVALID before any launch for a NULL pointer, n < 0, n > 0 with n_active < 1, num_item < 1,
 * n_user_rows < 0 or a mode other than 0 / 1; n == 0 launches nothing. */
int spex_sample_bpr_triples(const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows, const int32_t *d_active,
                            int32_t n_active, int32_t num_item, int64_t n, int32_t mode, uint64_t seed, uint32_t epoch,
                            int64_t *d_users, int64_t *d_pos, int64_t *d_neg, void *stream);

/* ------------------------------------------------------------------------------------------------ BCE epoch sampler
 * One BCE epoch drawn on the device, already shuffled: what LightTrainData.ng_sample() followed by the DataLoader's shuffle prepare
 * on the host (law, not stream — neither NumPy's nor torch's: for the same seed the individual samples differ from the reference's).
 * d_rowptr int32[n_user_rows + 1] / d_items int32: CSR of R on the device, every row ascending without duplicates
 * (trainer.bpr_sampler_tables); d_pos_user / d_pos_item int32[n_pos]: the positives in the caller's order, duplicates kept (each
 * occurrence is a sample); num_ng >= 1 negatives per positive; num_item: catalogue size.  With P = n_pos and n = P (1 + num_ng):
 * d_users int64[n], d_items_out int64[n], d_labels float[n] (the types spex_lightgcn_epoch_bce_f32 reads).
 * The UNSHUFFLED epoch has n source samples: source j < P is positive j (user d_pos_user[j], item d_pos_item[j], label 1); source
 * P + k, k in [0, P num_ng), is a negative of positive k / num_ng (all negatives of positive 0 first, ng_sample's order): user
 * d_pos_user[k / num_ng], label 0, item uniform over the items that are not in that user's row.  One thread per OUTPUT slot i in
 * [0, n): slot i holds source perm(i), perm a keyed bijection of [0, n) — the epoch is written in shuffled order by one launch.
 * Randomness: standard Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85, ten rounds).
 *   key     = (seed & 0xFFFFFFFF, seed >> 32)
 *   a word w maps to [0, m) as floor(w * m / 2^32) (multiply-high)
 *   negative k:  counter = (k & 0xFFFFFFFF, k >> 32 (= 0: n < 2^31), epoch, stage) -> output words w0 w1 w2 w3
 *     stage 0:  w0 .. w3 -> candidates 0 .. 3 (m = num_item)
 *     stage 1:  w0 .. w3 -> candidates 4 .. 7; computed only when candidates 0 .. 3 were all stored items of the user
 *     stage 2:  computed only when all eight candidates were: w0 -> t (m = num_item - the row's length), the negative is the t-th
 *               item in ascending order that is not in the row (w1 .. w3 unused)
 *     The negative is the first candidate, in the order 0 .. 7, that is not in the user's row.  The draw is keyed by k, not by the
 *     slot: where the shuffle puts a sample does not change it.
 *   perm:  a balanced Feistel network with cycle walking.
 *     bits = the bit length of n - 1 (0 for n = 1), h = max(1, ceil(bits / 2)), mask = 2^h - 1
 *     round keys K[0 .. 3] = w0 .. w3 of counter (0, 0, epoch, 3); K[4], K[5] = w0, w1 of counter (1, 0, epoch, 3)   (stage 3: no
 *       negative's counter)
 *     fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16   (MurmurHash3's finaliser, mod 2^32)
 *     x = i;  repeat { L = x >> h, R = x & mask;  for r = 0 .. 5: (L, R) <- (R, L ^ (fmix32(R ^ K[r]) & mask));  x = (L << h) | R }
 *     while x >= n;  perm(i) = x.
 *     Six Feistel rounds are a permutation of [0, 2^(2 h)), and n <= 2^(2 h) < 4 n (n >= 2): the walk from a point inside [0, n)
 *     follows that permutation's cycle, which returns to [0, n) (at the latest at the starting point) — it terminates without a cap,
 *     and the first return is a bijection of [0, n).
 * A slot of (seed, epoch) is a function of i, n, seed, epoch, the positives and the tables alone — not of the launch's shape.  A
 * user index outside [0, n_user_rows) reads as an empty row; a user whose row holds every item has no negative: 0 is written.
 * Returns SPEX_ERR_INVALID before any launch for a NULL pointer, n_pos < 0, num_ng < 1, num_item < 1, n_user_rows < 0 or
 * n_pos (1 + num_ng) >= 2^31; n_pos == 0 launches nothing. */
int spex_sample_bce_epoch(const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows, const int32_t *d_pos_user,
                          const int32_t *d_pos_item, int64_t n_pos, int32_t num_ng, int32_t num_item, uint64_t seed, uint32_t epoch,
                          int64_t *d_users, int64_t *d_items_out, float *d_labels, void *stream);

/* ------------------------------------------------------------------------------------------------ dual-task trust-path sampler
 * The per-batch trust-path selection of LightGCN_SPEX/code/main_auto_expert_s.py:64-71 for a whole shuffled epoch, on the device: what
 * trainer.dual_task_epoch_paths chooses on the host with random.sample (law, not stream).  One workgroup of 256 threads per batch,
 * one launch.  d_users int64[n]: the shuffled epoch (spex_sample_bce_epoch's d_users); batch k holds the samples j in [0, nb),
 * nb = min(B, n - k B), at d_users[k B + j]; max_steps < 0: all ceil(n / B) batches, else the first min(max_steps, ceil(n / B)).
 * d_path_rowptr int32[n_user_rows + 1] / d_path_idx int32[n_paths]: the path ids grouped by the path's first node, ascending within a
 * user (the reference's user_path_indx as a CSR; trainer.dual_sampler_tables); d_paths int64[n_paths, path_len]: the padded paths
 * (Data.inputs); d_path_l int64[n_paths]: their lengths (the row sums of Data.mask); d_path_tgt int64[n_paths]: their targets.
 * d_seq int64[n_batches cap, path_len], d_seq_l / d_targets int64[n_batches cap], d_count int32[n_batches].
 * The law, for batch k:
 *   first(j):  no j' < j holds the same user (d_users[k B + j'] == d_users[k B + j])
 *   c_j     =  d_path_rowptr[u + 1] - d_path_rowptr[u] for u = d_users[k B + j], if first(j) and 0 <= u < n_user_rows; else 0
 *   off_j   =  the exclusive prefix sum of c in order of j;  total = the sum of all c_j
 *   candidate q in [0, total) belongs to the j with off_j <= q < off_j + c_j and is path d_path_idx[d_path_rowptr[u_j] + q - off_j]
 *   d_count[k] = T_k = min(total, cap)
 *   slot t in [0, T_k) holds candidate q = t when total <= cap, otherwise q = perm_k(t)
 *   perm_k:  spex_sample_bce_epoch's balanced Feistel network with cycle walking, on the domain [0, total):
 *     bits = the bit length of total - 1, h = max(1, ceil(bits / 2)), mask = 2^h - 1
 *     key     = (seed & 0xFFFFFFFF, seed >> 32)   (standard Philox4x32-10, as there)
 *     round keys K[0 .. 3] = w0 .. w3 of counter (k, 0, epoch, 4); K[4], K[5] = w0, w1 of counter (k, 1, epoch, 4)   (stage 4: no counter
 *       of spex_sample_bce_epoch, whose stages are 0 .. 3 — one seed may serve both samplers)
 *     x = t;  repeat { L = x >> h, R = x & mask;  for r = 0 .. 5: (L, R) <- (R, L ^ (fmix32(R ^ K[r]) & mask));  x = (L << h) | R }
 *     while x >= total;  perm_k(t) = x.
 *     The first cap images of a keyed bijection of [0, total) are a sample without replacement in random order: random.sample's
 *     law, not its stream.
 *   slot t of batch k is written at row k cap + t: the path's row of d_paths, its d_path_l, its d_path_tgt.  Slots t >= T_k are not
 *   written.  (An entry of d_path_idx outside [0, n_paths) — no table of trainer.dual_sampler_tables holds one — writes nothing.)
 * A batch's output is a function of (its users, the tables, cap, seed, epoch, k) alone — not of n beyond the batch, nor of the order
 * in which the workgroup's threads arrive: a draw bounded by max_steps = m is the first m batches of the full draw.
 * Returns SPEX_ERR_INVALID before any launch for a NULL pointer, B outside [1, 4096] (a batch's users are held in LDS as int32), n < 0,
 * cap < 0, path_len < 1, n_user_rows < 0, n_paths < 0 or 2^31 batches and more; n == 0 launches nothing, cap == 0 writes only the
 * counts (zeros). */
int spex_sample_dual_task_paths(const int64_t *d_users, int64_t n, int32_t B, int64_t max_steps, const int32_t *d_path_rowptr,
                                int32_t n_user_rows, const int32_t *d_path_idx, int32_t n_paths, const int64_t *d_paths, int32_t path_len,
                                const int64_t *d_path_l, const int64_t *d_path_tgt, int32_t cap, uint64_t seed, uint32_t epoch,
                                int64_t *d_seq, int64_t *d_seq_l, int64_t *d_targets, int32_t *d_count, void *stream);

/* ------------------------------------------------------------------------------------------------ NGCF epoch sampler
 * One NGCF epoch drawn on the device, already shuffled: what load_train_data / train_sample of NGCF_SPEX/code/utility/load_data.py
 * (per user 5 |positives| DISTINCT negatives, random.sample from the items seen in training minus the user's own, then the positives)
 * followed by the DataLoader's shuffle prepare on the host (law, not stream: for the same seed the individual samples differ from the
 * reference's).  NOT spex_sample_bce_epoch's law: a user's negatives are drawn WITHOUT replacement, from a population that is the
 * set of items seen in training, not the whole catalogue.  Tables (device, trainer.ngcf_sampler_tables builds them):
 *   d_pop      int32[n_pop]   the population: the distinct items seen in training, ascending (ids may have gaps)
 *   d_user     int32[U]       U = n_users: the epoch's users in the reference's order (file order, whole blocks of 256 users: the
 *                             caller's cut — the kernel takes the list as given)
 *   d_pos_off  int32[U + 1]   d_pos_off[0] = 0, non-decreasing, d_pos_off[U] = n_pos;  c_q = d_pos_off[q + 1] - d_pos_off[q] >= 0
 *   d_pos_item int32[n_pos]   user q's positives in file order at [d_pos_off[q], d_pos_off[q + 1]), duplicates kept (each occurrence
 *                             is a sample)
 *   d_row_off  int32[U + 1]   d_row_off[0] = 0, non-decreasing;  m_q = d_row_off[q + 1] - d_row_off[q]
 *   d_row_rank int32[d_row_off[U]]   at [d_row_off[q], d_row_off[q + 1]): the ranks within d_pop (positions, from 0) of user q's
 *                             DISTINCT positives, ascending
 * With n = 6 n_pos: d_users int64[n], d_items_out int64[n], d_labels float[n] (the types spex_ngcf_epoch_bce_f32 reads).
 * The UNSHUFFLED epoch has n source samples.  User q owns the sources [6 d_pos_off[q], 6 d_pos_off[q + 1]); inside that block, with
 * i the index from its start and k_q = 5 c_q:
 *   i <  k_q:  negative i of user q  — user d_user[q], label 0, the item below
 *   i >= k_q:  positive i - k_q      — user d_user[q], label 1, item d_pos_item[d_pos_off[q] + i - k_q]
 * (the negatives first, then the positives: the reference's order; a user with c_q = 0 owns nothing).
 * One thread per OUTPUT slot s in [0, n): slot s holds source perm(s), perm a keyed bijection of [0, n) — the epoch is written in
 * shuffled order by one launch.
 * Randomness: standard Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85, ten rounds), key =
 * (seed & 0xFFFFFFFF, seed >> 32), counter (c0, c1, c2, c3) -> output words w0 w1 w2 w3.
 *   F(x; m, K):  spex_sample_bce_epoch's balanced six-round Feistel network with cycle walking on the domain [0, m), round keys K[0 .. 5]:
 *     bits = the bit length of m - 1 (0 for m = 1), h = max(1, ceil(bits / 2)), mask = 2^h - 1
 *     fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16   (MurmurHash3's finaliser, mod 2^32)
 *     repeat { L = x >> h, R = x & mask;  for r = 0 .. 5: (L, R) <- (R, L ^ (fmix32(R ^ K[r]) & mask));  x = (L << h) | R }
 *     while x >= m;  F = x.   (A bijection of [0, m) that terminates without a cap: see spex_sample_bce_epoch.)
 *   negative i of user q:  n_q = n_pop - m_q  (the population minus the user's distinct positives)
 *     K[0 .. 3] = w0 .. w3 of counter (q, 0, epoch, 5);  K[4], K[5] = w0, w1 of counter (q, 1, epoch, 5)
 *     r = F(i; n_q, K);  the item is d_pop[r + #{ t in [0, m_q) : d_row_rank[d_row_off[q] + t] - t <= r }] — the r-th member of the
 *     population, in ascending order, that is not one of the user's positives.
 *     The draw is keyed by (q, i) — q the user's POSITION in d_user, not the user id — and not by the slot: where the shuffle puts a
 *     sample does not change it.  The first k_q images of a keyed bijection of [0, n_q) are k_q distinct members in random order:
 *     random.sample's law, not its stream.
 *   perm(s) = F(s; n, K) with K[0 .. 3] = w0 .. w3 of counter (0, 0, epoch, 6);  K[4], K[5] = w0, w1 of counter (1, 0, epoch, 6).
 *   Stages 5 and 6 (the counter's last word) are no counter of spex_sample_bce_epoch (stages 0 .. 3) nor of
 *   spex_sample_dual_task_paths (stage 4): one seed may serve all of these samplers.
 * What is exact and what is not: a user's negatives are pairwise distinct, never one of the user's positives and always members of
 * d_pop, at EVERY size — F is a bijection whatever its keys.  That each member of the complement is equally likely is a statement about
 * domains of realistic size: on a domain of a few elements (h = 1 or 2: m <= 16) the six keyed rounds reach only a part of the m!
 * orderings, and the frequencies over many (seed, epoch) are only roughly even there.  The same holds for perm on a tiny n.
 * Guards: the caller promises k_q <= n_q for every user (random.sample raises ValueError("Sample larger than population or is
 * negative") otherwise; trainer.ngcf_sampler_tables raises the same).  A negative with n_q <= 0 or i >= n_q writes item 0 and reads
 * no table beyond the offsets; a positive whose index falls outside [0, n_pos) (offsets that break the promises above) writes item 0.
 * A slot of (seed, epoch) is a function of s, the tables, seed and epoch alone — not of the launch's shape.
 * Returns SPEX_ERR_INVALID before any launch for a NULL pointer, n_pop < 1, U < 0, n_pos < 0, n_pos > 0 with U < 1, or
 * 6 n_pos >= 2^31; n_pos == 0 launches nothing. */
int spex_sample_ngcf_epoch(const int32_t *d_pop, int32_t n_pop, const int32_t *d_user, int32_t n_users, const int32_t *d_pos_off,
                           const int32_t *d_pos_item, int64_t n_pos, const int32_t *d_row_off, const int32_t *d_row_rank, uint64_t seed,
                           uint32_t epoch, int64_t *d_users, int64_t *d_items_out, float *d_labels, void *stream);

/* ------------------------------------------------------------------------------------------------ learned edge values
 * the Diffnet++ social / interest diffusion — the same SpMM on user x user, user x item and item x user
 * graphs whose stored values are LEARNED (a per-edge parameter pushed through a row softmax), so the values change
 * every step and need a gradient.  Replaces, on fixed sparsity patterns,
 *   tf.sparse.softmax(SparseTensor(indices, values))        Diffnet++_SPEX/code/utility/Model.py:275-286
 *   tf.sparse.sparse_dense_matmul(att_matrix, embedding)    Model.py:18-83 (forward: spex_spmm_f32 after set_values)
 *   and their gradients w.r.t. the values (tape.gradient, Diffnet++_SPEX/code/main_rec.py:36).
 * Every per-edge array here is indexed by EDGE ID (h_edge_id of spex_graph_create; identity = CSR entry order), so a
 * graph and its transposed copy share one values array.  n_val = length of that array (> the largest edge id).
 */

/* Replace the stored values of the handle by d_val[edge_id] (device, fp32); later SpMM launches on the handle use them. */
int spex_graph_set_values(spex_graph_t *g, const float *d_val, int64_t n_val, void *stream);

/* Sampled dense-dense product on the handle's pattern: d_out[edge_id(e)] = <A[row(e),:], B[col(e),:]> for every stored
 * entry e.  A: [n_rows, d], B: [n_cols, d].  With A = dL/dY and B = X this is dL/dval of Y = spmm(val, X).
 * Entries are not weighted by the stored values.  The first call on a handle allocates and builds a per-entry row
 * index (4 B/entry): make that call outside any stream capture.
 */
int spex_sddmm_f32(spex_graph_t *g, const float *A, const float *B, float *d_out, int64_t n_val, int32_t d, void *stream);

/* Row softmax over the stored entries (empty rows: nothing written):
 *   d_out[id(e)] = exp(d_in[id(e)] - max_row) / sum_row exp(d_in - max_row)
 * and its backward  d_grad_in[id(e)] = d_out[id(e)] * (d_grad_out[id(e)] - sum_row d_out * d_grad_out).
 * d_in may equal d_out; d_grad_out may equal d_grad_in.
 */
int spex_edge_softmax_f32(const spex_graph_t *g, const float *d_in, float *d_out, int64_t n_val, void *stream);
int spex_edge_softmax_bwd_f32(const spex_graph_t *g, const float *d_out_val, const float *d_grad_out, float *d_grad_in,
                              int64_t n_val, void *stream);

/* Node-level attention fusion of a Diffnet++ layer — Diffnet++_SPEX/code/utility/Model.py:308-345 / 352-385 — one row
 * per wave, all of it in one launch:
 *   r_k = [U | X_k] . w1_k   (U == NULL: r_k = X_k . w1_k);   e_k = exp(LeakyReLU_0.2(w2_k tanh(r_k + b1_k) + b2_k)) + c_k
 *   out = base_coef U + mix_coef (e_1 X_1 + e_2 X_2) / (e_1 + e_2)
 * users (:308-321): U = user rows, X_1 = from consumed items (c = 0.7), X_2 = from social neighbours (c = 0.3), 1/2, 1/2;
 * items (:323-343): U = NULL, X_1 = the item rows, X_2 = from customers, c = 1, 1, base 0, mix 1.
 * p_k: device parameter block of branch k = [ w1_k ((U ? d : 0) + d floats), b1_k, w2_k, b2_k ].  d <= 256.
 * Backward: grad_U (iff U) / grad_X1 / grad_X2 are written; grad_p1 / grad_p2 are ACCUMULATED (zero them first).
 */
int spex_attn_fuse_f32(const float *U, const float *X1, const float *X2, const float *p1, const float *p2, int32_t n,
                       int32_t d, float c1, float c2, float base_coef, float mix_coef, float *out, void *stream);
int spex_attn_fuse_bwd_f32(const float *U, const float *X1, const float *X2, const float *p1, const float *p2, int32_t n,
                           int32_t d, float c1, float c2, float base_coef, float mix_coef, const float *grad_out,
                           float *grad_U, float *grad_X1, float *grad_X2, float *grad_p1, float *grad_p2, void *stream);

/* ------------------------------------------------------------------------------------------------ trust-path attention
 * SURVEY.md 8f #1.  Replaces GraphAttentionLayer.forward, LightGCN_SPEX/code/utility2/layers.py:15-71 (Python loops
 * over batch x path position), for all heads of a layer in one launch, and its autograd backward.
 *   path p = x_0 .. x_{l-1} (l = seq_l[p] <= L), position i < l - 1, head h with parameter a_h = [a1_h | a2_h] (2 d floats):
 *     positional != 0 (concat=True,  layers.py:22-31): A = src[seq[p,i]] + (l - i),  Bv = src[seq[p,i+1]] + (l - i - 1)
 *     positional == 0 (concat=False, layers.py:58-63): A = src[.., i],               Bv = src[.., i + 1]
 *     att = softmax([A.a1_h + A.a2_h, A.a1_h + Bv.a2_h]);   out[p, i, h*d : (h+1)*d] = att_0 A + att_1 Bv
 *   positions i >= l - 1 copy the raw source row into every head's slot.
 * src: [n_src_rows, d] device fp32.  seq: device int64 [B, L] of row indices into src, or NULL = dense source
 * (src is [B, L, d], row p * L + i; n_src_rows must equal B * L).  seq_l: device int64 [B].  a: [n_heads, 2 d].
 * out: [B, L, n_heads * d].  w0_out (optional, [B, L, n_heads]): att_0, which the backward reads.  d <= 256.
 * Backward: grad_src ([n_src_rows, d]) and grad_a ([n_heads, 2 d], may be NULL) are ACCUMULATED with atomics — zero
 * them first.  (The a1 halves receive nothing: A.a1 cancels in the softmax, their gradient is exactly zero.)
 */
int spex_path_attention_f32(const float *src, int64_t n_src_rows, const int64_t *seq, const int64_t *seq_l, const float *a,
                            int32_t B, int32_t L, int32_t d, int32_t n_heads, int32_t positional, float *out, float *w0_out,
                            void *stream);
int spex_path_attention_bwd_f32(const float *src, int64_t n_src_rows, const int64_t *seq, const int64_t *seq_l,
                                const float *a, int32_t B, int32_t L, int32_t d, int32_t n_heads, int32_t positional,
                                const float *w0, const float *grad_out, float *grad_src, float *grad_a, void *stream);

/* ------------------------------------------------------------------------------------------------ trust head
 * The whole trust branch of the dual-task model — replaces LightGCN_SPEX/code/utility1/model_expert_s.py:170-192 (forward,
 * flag 0 / 2): the in_att heads and out_att (utility2/layers.py:15-71), `mul_seq @ w` + ELU (:181-183), compute_scores
 * (:128-148: soft-attention readout, linear_transform, max-pool, att_t gate, logits against the user table) and
 * nn.CrossEntropyLoss (:192) with their gradients.  Hidden size must be 64; L <= 16 positions, n_heads <= 4.
 *
 * params / grad_params: ONE flat fp32 block, in this order (d = 64, H = n_heads; spex_trust_param_count gives the total):
 *   attention_0.a .. attention_{H-1}.a [H][2d] | out_att.a [2d] | w [H d, d] | linear_one.weight [d, d] | .bias [d] |
 *   linear_two.weight [d, d] | .bias [d] | linear_three.weight [d] | linear_transform.weight [d, 2d] | .bias [d] | att_t [2d, 2]
 * table: the user table incl. its pad row ([n_rows, 64]); seq: [B, L] int64 user ids padded with the pad row; seq_l: [B].
 * hybrid = !nonhybrid (model_expert_s.py:136-141).
 *
 * spex_trust_head_fwd_f32 (one launch): a2_out [B, 64] = the vector whose product with the user table gives the logits
 *   (:146-147) — the evaluation form (flag 2).
 * spex_trust_head_train_f32 (two launches: the fused path kernel — forward chain, the logits / cross-entropy / d a2 sweep of the
 *   user table shared by up to 8 workgroups per path whose last one folds the shares in a fixed order and runs the backward chain —
 *   and the reductions.  SPEX_TRUST_SPLIT=n caps the workgroups per path — a test hook, read per call): forward, logits = a2 . table[0 : n_rows - 1]^T (`b = table[:-1]`), loss =
 *   mean_b CE(logits_b, targets_b) -> *loss_out (added to it if loss_accumulate; may be NULL), and the whole backward:
 *   grad_params (flat block) is OVERWRITTEN (one thread per weight sums its contributions in a fixed order: deterministic);
 *   grad_table [n_rows, 64] is ACCUMULATED by the launch that owns the rows — the logits' part, then the rows of the paths that
 *   pass through the user in (path, position) order; no atomics: the whole head repeats bit for bit — zero it first or pass
 *   the buffer it is to be added to.  Gradients are scaled by scale * (*scale_dev if
 *   scale_dev else 1) — e.g. the multi-task precision exp(-2 s) of main_auto_expert_s.py:81-82 read on the device.
 *   Scratch (caller-owned): a2 [B, 64], dscore [B, n_rows - 1], loss_b [B], ws [spex_trust_workspace_floats(B, L, 64, H, n_rows)]
 *   (per-path blocks + the user tiles' / the shares' partials and the paths' arrival tickets; the workspace need NOT be zeroed:
 *   a ticket carries the call's tag, whatever else the word holds counts as "nobody arrived yet").  One workspace serves one
 *   call at a time (calls on one stream: fine; the same workspace on two streams at once: not).
 */
int64_t spex_trust_param_count(int32_t d, int32_t n_heads);                                /* -1: unsupported shape */
int64_t spex_trust_workspace_floats(int32_t B, int32_t L, int32_t d, int32_t n_heads,
                                    int64_t n_rows);                                        /* -1: unsupported shape */
int spex_trust_head_fwd_f32(const float *table, int64_t n_rows, const float *params, const int64_t *seq, const int64_t *seq_l,
                            int32_t B, int32_t L, int32_t d, int32_t n_heads, int32_t hybrid, float *a2_out, void *stream);
int spex_trust_head_train_f32(const float *table, int64_t n_rows, const float *params, const int64_t *seq, const int64_t *seq_l,
                              const int64_t *targets, int32_t B, int32_t L, int32_t d, int32_t n_heads, int32_t hybrid,
                              float scale, const float *scale_dev, float *a2, float *dscore, float *loss_b, float *ws,
                              float *loss_out, int32_t loss_accumulate, float *grad_params, float *grad_table, void *stream);

/* ------------------------------------------------------------------------------------------------ one-call training step
 * The exact reference training step — LightGCN_SPEX/code/main_rec.py:32-37: forward (model.py:111-121), BCE,
 * loss.backward(), optimizer.step() — as ONE call that issues the library's own launches back to back:
 *   L-1 x spex_spmm_f32 (running layer sum)
 *   spex_lightgcn_batch_f32 (last layer at the batch's rows + scores + BCE + gradient rows + (g + A^T g)/(L+1) in push form;
 *                            L == 1: spex_spmm_rowlist_f32 -> spex_score_bce_slots_f32 -> one pull-form product instead)
 *   L-1 x spex_spmm_f32 on A^T (g/(L+1) fused) -> spex_adam_step_f32 over the whole table (which clears g_out again).
 * 2 L + 1 launches (seven for L = 3).
 * The descriptor holds the step's device buffers (all caller-owned, N = graph rows; d = 64, 128 or 256 — any other width is
 * rejected; at d > 64 every table 16-byte aligned):
 *   E0, m, v, light_out, lo_batch, g_out, grad_E0: [N, d];  ws_fwd: [2, N, d];  ws_bwd: [3, N, d];
 *   grad_slots: [slot_capacity, d] with slot_capacity >= 2B (the batch's per-sample gradient rows).
 * g_out and the first [N, d] of ws_bwd must be all-zero before the first call (every call leaves them all-zero: the Adam
 * pass clears both).  t is advanced by the call.
 * users / items: device int64[B] (items index the item block: row n_user_rows + items[b]); labels: device fp32[B].
 * *loss_sum (device) accumulates the batch's BCE loss SUM.  L >= 1.  Edge dropout (`--dropout 1 --keepprob p`, the reference's
 * recommended configuration): set the step's mask on BOTH handles with spex_graph_set_edge_mask before the call — graph_t must
 * then be the transposed handle created with the edge-id permutation (a masked adjacency is not symmetric) and L >= 2; every
 * product of the step, the batch kernel's included, drops the same edges.
 * graph is walked by the forward AND by the push-form first backward product (A^T g in push form walks the rows of A); graph_t
 * (A^T) by the pull-form products.  t is advanced only when every launch of the step was queued (a failed call leaves it alone).
 *
 * flags & SPEX_STEP_DETERMINISTIC (all three step descriptors): no float atomics anywhere in the step — per-sample gradient rows
 * are added per table row in ascending slot order (spex_reduce_slots_f32: the order of the reference's CPU index backward), the
 * whole backward propagation runs in pull form (spex_propagate_bwd_f32: one chain per output row in ascending column order, like
 * the reference's sparse addmm), per-sample losses are summed in sample order.  Two runs from the same state then produce
 * bit-identical parameters; the price is one more SpMM-sized launch and two small ones per step (a validation mode: the fast
 * path's atomics only reorder sums, which Adam amplifies along NGCF's scale-invariant direction over thousands of steps).
 */
enum {
    SPEX_STEP_DETERMINISTIC = 1,        /* fixed summation order everywhere (see above) */
    SPEX_STEP_FIXED_TASK_WEIGHTS = 2,   /* dual-task step only: loss = loss1 + loss2 (LightGCN_SPEX/code/main_11.py:69) instead of the
                                         * uncertainty weighting of main_auto_expert_s.py:78-82; task_weights are left untouched */
    SPEX_STEP_PIPELINED = 4,            /* dual-task step only, with side_stream: the Adam pass split by owner over the two streams, no
                                         * fork / join on the critical cycle; see spex_dual_task_step_t and spex_dual_task_step_join */
    SPEX_STEP_BPR_DENSE = 8,            /* exact BPR step only: force the dense form of the fast path (gradient rows into g_out, all-pull
                                         * backward) ... */
    SPEX_STEP_BPR_PUSH = 16,            /* ... or the push form, whatever T; neither flag: chosen by T (see spex_lightgcn_step_bpr_adam_f32) */
    SPEX_STEP_WIDE = 32,                /* exact BPR step only: this descriptor's tables and slots are d wide with d = 128 or 256.  The BCE step
                                         * needs no such flag (it took the three widths from its first version); the BPR entry point promised
                                         * d == 64 ONLY and rejects a descriptor whose d says otherwise — callers rely on that rejection for a
                                         * 64-wide descriptor with a wrong d, which would gather out of bounds — so a wider d is an opt-in */
    SPEX_STEP_BF16_GATHER = 64,         /* the one-call LightGCN steps (BCE, exact BPR) and every epoch over them: bf16 gather tables, d == 64
                                         * and L = 2 or 3 only; the descriptor's E0_16 / ws16 fields are read (see spex_lightgcn_step_t) */
    SPEX_STEP_FRONTIER = 128,           /* the one-call LightGCN steps (BCE, exact BPR) and every epoch over them: forward layer L - 1 and the
                                         * backward product behind the batch kernel's push run over the batch's frontier, not the whole
                                         * graph; d == 64, L >= 2; the descriptor's frontier_* fields are read (see spex_lightgcn_step_t).
                                         * Combines with SPEX_STEP_BF16_GATHER (then L = 2 or 3): the frontier launches read bf16 tables */
    SPEX_STEP_SPARSE_ADAM = 256,        /* with SPEX_STEP_FRONTIER at L == 2 only: row-sparse ("lazy") Adam — p, m, v change at the rows of the
                                         * batch's two-hop set F2 and nowhere else, the step count is global; no launch of the step but the
                                         * first flagged one passes over a whole fp32 table.  Its own semantics: see spex_lightgcn_step_t */
    SPEX_STEP_GRAD_ROWS_LISTED = 512,   /* state, not a mode: "grad_E0 is zero outside the list the step that set the bit used":
                                         * frontier_list[0 .. frontier_counts[2]), or [0 .. frontier_counts[3]) where that step carried
                                         * SPEX_STEP_FRONTIER_DEEP.  Set in the descriptor by a SPEX_STEP_SPARSE_ADAM step once its launches
                                         * are queued, cleared by every other step of these entry points; a caller that writes grad_E0 or
                                         * frontier_list itself clears it */
    SPEX_STEP_FRONTIER_DEEP = 1024      /* with SPEX_STEP_FRONTIER at L == 3, d == 64, fp32 tables only: EVERY launch of the step runs over a
                                         * device list (y_1 at F2, y_2 at F1, the pushes over F1 and F2), no whole-graph launch is left;
                                         * with SPEX_STEP_SPARSE_ADAM on top, row-sparse Adam over F3.  See spex_lightgcn_step_t */
};
/* The north-star step — LightGCN L-layer propagation + the fused BPR gather + dot + sigmoid + SGD kernel over T triples — as one
 * call of at most L + 1 launches: EVERY whole-graph layer in the plain form (no epilogue operand, one output stream); the layer-1 launch also sets
 * aside, in a tail of ceil(3 T / 1024) extra workgroups, the E^0 rows of the batch's 3 T slots (a buffer owned by the graph handle,
 * grown on the first call at a batch size — make that call outside a stream capture), and the BPR kernel forms the layer mean
 * (((E^0 + E^1) + E^2) + E^3) / (L + 1) — utility1/model.py:94-95, in the fused epilogues' order — at its triples' rows only, the
 * rows of the propagated table the step reads; the updates go to E^0.  Same results as spex_propagate_f32 followed by
 * spex_bpr_sgd_step_f32 reading its output (bit-identical rows; float-atomic updates in both).
 * E0, sum1: [N, 64]; ws: [2, N, 64]; users index rows [0, n_user_rows), items rows n_user_rows + i.
 * sum1 after the call: E^1.  Where the tail would push a layer launch that fits one dispatch round (<= 512 workgroups) over 512,
 * and for T > 2^18, the step keeps layer 1 in the running-sum form instead — then sum1 = E^0 + E^1 and the kernel adds
 * ((sum1 + E^2) + E^3): the same bits.  The schedule depends on the graph and T only.
 * The LAST layer is not a whole-graph launch where it need not be: for L >= 2, on a graph whose rows all have <= 1024 entries and
 * while 6 T <= N, the step is L launches — L - 1 whole-graph launches and one that gathers layer L at the batch's <= 3 T slot rows
 * from the layer-(L-1) table (four triples per workgroup) and runs the BPR update on (((E^0 + E^1) + E^2) + that row) / (L + 1): the
 * whole-graph launch's rows bit for bit.  The step then traverses (L - 1) nnz stored entries plus the batch rows' (48 % of nnz for
 * 2048 random triples on Epinion2), and the half of ws that would receive layer L is NOT written (snapshot schedule: ws[1] for
 * L = 3, ws[0] for L = 2).  That launch keeps a few 8-byte loss cells in the graph handle (one per 16 triples, zero between
 * launches; grown like the snapshot buffer).  L = 1, graphs with longer rows and larger T keep the L + 1 launches above.
 * d == 64, 1 <= L <= 3, no edge dropout; *loss_sum accumulates the batch's softplus sum.  T == 0 (u, i_pos, i_neg may be NULL): the
 * propagation runs, nothing is updated. */
int spex_lightgcn_step_bpr_f32(const spex_graph_t *g, float *E0, float *sum1, float *ws, int32_t n_user_rows, int32_t L, int32_t d,
                               const int64_t *u, const int64_t *i_pos, const int64_t *i_neg, int64_t T, float lr, float reg,
                               float *loss_sum, void *stream);

/* The four d == 64 batch-sized middles with a bf16 gather source (SPEX_STEP_BF16_GATHER's launches): the arguments of
 * spex_lightgcn_batch_f32, spex_lightgcn_batch_slots_f32, spex_lightgcn_bpr_batch_f32 and spex_lightgcn_bpr_batch_slots_f32 with
 * X16 ([N, 64] bf16, rows of 128 bytes) for X.  Only the last layer's gather reads X16, widened exactly; acc_in, every sum, the
 * scores, the loss, the gradient rows, the L2 counts and the push (fp32 slots) are the fp32 kernel's statements: on
 * Xw = float(X16) a call returns what its fp32 sibling returns on Xw (slots forms: bit for bit; push forms: up to the order of
 * the float atomics), and a forward row of at most 1 024 entries is spex_spmm_bf16_f32's row bit for bit, under an edge mask too.
 * d != 64: SPEX_ERR_UNSUPPORTED. */
int spex_lightgcn_batch_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div, const int64_t *users,
                                 const int64_t *items, const float *labels, int32_t B, int32_t n_user_rows, float grad_scale,
                                 float push_scale, float *loss_sum, float *loss_per_sample, float *g_out, float *G, int32_t d,
                                 void *stream);
int spex_lightgcn_batch_slots_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                       const int64_t *users, const int64_t *items, const float *labels, int32_t B, int32_t n_user_rows,
                                       float grad_scale, float *loss_sum, float *loss_per_sample, float *grad_slots, int32_t d,
                                       void *stream);
int spex_lightgcn_bpr_batch_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div, const int64_t *users,
                                     const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows, float grad_scale,
                                     float push_scale, float weight_decay, const float *E0, int32_t *row_counts, float *loss_sum,
                                     float *loss_per_sample, float *g_out, float *G, int32_t d, void *stream);
int spex_lightgcn_bpr_batch_slots_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                           const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows,
                                           float grad_scale, float weight_decay, const float *E0, int32_t *row_counts, float *loss_sum,
                                           float *loss_per_sample, float *grad_slots, int32_t d, void *stream);

typedef struct spex_lightgcn_step {
    const spex_graph_t *graph, *graph_t;     /* A and A^T (the same handle for the symmetric LightGCN adjacency) */
    float *E0, *m, *v;
    float *light_out, *ws_fwd, *lo_batch, *g_out, *ws_bwd, *grad_E0, *grad_slots;
    int32_t slot_capacity, n_user_rows, L, d;
    float lr, beta1, beta2, eps;
    int32_t t;
    int32_t flags;                           /* SPEX_STEP_DETERMINISTIC, SPEX_STEP_BPR_DENSE / _PUSH, SPEX_STEP_WIDE, SPEX_STEP_BF16_GATHER, SPEX_STEP_FRONTIER,
                                              * SPEX_STEP_SPARSE_ADAM, SPEX_STEP_FRONTIER_DEEP; SPEX_STEP_GRAD_ROWS_LISTED is written back by the steps */
    /* appended for spex_lightgcn_step_bpr_adam_f32 / spex_lightgcn_epoch_bpr_f32 (the BCE entry points never read them): */
    float weight_decay;                      /* >= 0: upstream LightGCN's L2 term on the E0 rows of the batch */
    int32_t *row_counts;                     /* [2, N] int32, all-zero before the first call: per-row occurrence counts, by step parity.
                                              * Only spex_lightgcn_step_bpr_adam_f32 (and the epochs over it) keeps the tables: a caller
                                              * that advances t by ANY other call must clear both before the next BPR step */
    /* appended for SPEX_STEP_BF16_GATHER (without the flag no entry point reads them): */
    uint16_t *E0_16;                         /* [N, 64] bf16: the shadow of E0.  Contract: E0_16 == bf16(E0) (spex_cast_bf16_f32) on entry;
                                              * every call leaves it so */
    uint16_t *ws16;                          /* [2, N, 64] bf16: the later layers' gather tables, then the backward's */
    /* appended for SPEX_STEP_FRONTIER (without the flag no entry point reads them): */
    int32_t *frontier_list;                  /* [N] int32: [Bset | F1 minus Bset] of the current step (SPEX_STEP_SPARSE_ADAM: [.. | F2 minus F1]) */
    int32_t *frontier_stamp;                 /* [N] int32, all-zero before the first call; never cleared afterwards */
    int32_t *frontier_counts;                /* [2] int32: |Bset|, |F1| of the current step; with SPEX_STEP_SPARSE_ADAM or SPEX_STEP_FRONTIER_DEEP
                                              * [4] int32: |Bset|, |F1|, |F2|, |F3| (|F3| is written only by a step that carries both) */
    int32_t frontier_epoch;                  /* the last stamp used (0 at first); advanced by every flagged step */
} spex_lightgcn_step_t;
/* flags & SPEX_STEP_FRONTIER_DEEP — the L == 3 frontier step with no whole-graph launch (with SPEX_STEP_FRONTIER, d == 64, fp32 tables;
 * BCE and exact BPR, weight_decay > 0 too, under edge dropout too, and every epoch, sampled-epoch and train_*_sampled call over them;
 * DESIGN.md 4.28).  With F2 = F1 U the stored (and, under a mask, kept) columns of F1's rows, F3 likewise behind F2:
 *   lists:     Bset, F1, F2 as SPEX_STEP_SPARSE_ADAM builds them at L == 2 (frontier_counts[0 .. 2]); with SPEX_STEP_SPARSE_ADAM a third
 *              spex_frontier_rows_masked_i32 over [0, |F2|) writes |F3| to frontier_counts[3].
 *   forward:   y_1 = A E0 at the rows of F2 into ws_fwd[0], y_2 = A y_1 at the rows of F1 into ws_fwd[1], both by
 *              spex_spmm_rowlist_dev_f32 in the plain form; the batch launch is the L == 3 step's own.  It reads y_2 at the columns of
 *              Bset's rows (in F1); y_2 at F1 reads y_1 at the columns of F1's rows (in F2).  Rows of ws_fwd outside the lists hold
 *              whatever an earlier step left there: nothing reads them, and a caller must not either.
 *   backward:  P, the batch launch's push target ws_bwd[0], is supported in F1; W = A^T P is the push over the F1 list into ws_bwd[1]
 *              (supported in F2); grad_E0 = A^T W is a push over the F2 list (supported in F3; both by spex_spmm_push_list_f32); the Adam
 *              pass adds P, as in the L == 3 step without the flag.  Dense Adam: both push targets are cleared whole by launches of
 *              the step.
 *   with SPEX_STEP_SPARSE_ADAM: that flag's law with F3 in place of F2 — p, m, v change at the rows of F3 and nowhere else; P is
 *              read, added and cleared below |F1|, W is cleared below |F2|, the L2 occurrence counts stay keyed to Bset, grad_E0
 *              is cleared by list (frontier_counts[3]) at the next flagged step; then no launch passes over a whole fp32 table.
 * The results are the L == 3 step's up to the order of the float atomics (two pushes where SPEX_STEP_FRONTIER alone has one).
 * Refused before anything touches the device (t not advanced): the flag without SPEX_STEP_FRONTIER, L != 3, SPEX_STEP_BF16_GATHER,
 * SPEX_STEP_DETERMINISTIC, SPEX_STEP_BPR_DENSE -> SPEX_ERR_INVALID; d != 64 or SPEX_STEP_WIDE -> SPEX_ERR_UNSUPPORTED; a mask where
 * graph_t == graph -> SPEX_ERR_INVALID (the rule of every masked step). */
/* flags & SPEX_STEP_SPARSE_ADAM — row-sparse Adam for the L == 2 frontier steps (with SPEX_STEP_FRONTIER, d == 64; BCE and exact BPR,
 * weight_decay > 0 too, and every epoch, sampled-epoch and train_*_sampled call over them).  The step computes the forward, the loss
 * and the gradient of the SPEX_STEP_FRONTIER step.  At L == 2 that gradient's support is structural: it lies in
 *   F2 = F1 U { col[e] : e a stored entry of a row in F1 },
 * the rows the frontier push can write (a second spex_frontier_rows_masked_i32 over the same list, stamp table and epoch — under edge
 * dropout "stored" reads "stored and kept by this step's mask" in both sets: frontier_list =
 * [Bset | F1 minus Bset | F2 minus F1], frontier_counts[2] = |F2|).  Then
 *   rows in F2:       p, m, v are updated by the dense pass's own expression (spex_adam_step_f32's, shared code: the same roundings)
 *                     with the global step count t in both bias corrections; the BPR step's L2 term is included.  F2 is the structural
 *                     set whatever the values: a listed row whose gradient happens to be zero is still updated.
 *   rows outside F2:  p, m, v are neither read nor written: they stand still bit for bit and do NOT coast on their momentum, as they
 *                     do under dense Adam.  This is a different optimiser, not a faster route to the same numbers.
 * That is the masking law of torch.optim.SparseAdam with the eps placement of torch.optim.Adam (denom = sqrt(v) / sqrt(1 - beta2^t)
 * + eps); SparseAdam itself places eps elsewhere, so it is no bit-level oracle for this mode.
 * Work: the Adam pass (spex_adam_rows_f32's kernel), the clears of g_out (at Bset) and of the push target ws_bwd[0] (at F1) and the
 * loss sum (one addend in the dense pass's fixed order: the step's loss sum is the SPEX_STEP_FRONTIER step's bit for bit from the
 * same state) are proportional to |F2|.  grad_E0 holds the step's gradient afterwards (zero outside F2), so the pass cannot clear
 * it: the NEXT flagged step clears it as its first launch through the list this step left, if the descriptor still carries
 * SPEX_STEP_GRAD_ROWS_LISTED (see the flag); without the bit it clears the whole table once.  The exact BPR step clears the other
 * parity's row_counts table whole (4 N bytes) instead of in the Adam pass; the tables satisfy the same contract afterwards.
 * g_out and ws_bwd[0] are all-zero after every step, as without the flag.
 * Refused before anything touches the device (t not advanced): SPEX_STEP_SPARSE_ADAM without SPEX_STEP_FRONTIER, with L != 2 (L == 3 is taken together
 * with SPEX_STEP_FRONTIER_DEEP: see that flag), or
 * together with SPEX_STEP_BF16_GATHER (the row-sparse pass keeps no bf16 shadow of E0) -> SPEX_ERR_INVALID; everything
 * SPEX_STEP_FRONTIER refuses stays refused. */
/* flags & SPEX_STEP_FRONTIER — the exact steps with one more level taken inward (d == 64, L >= 2).  With Bset the batch's
 * distinct rows and F1 = Bset U their stored columns (spex_unique_rows_i32 + spex_frontier_rows_i32 into frontier_list):
 *   forward:   layers 1 .. L - 2 over the whole graph as without the flag; layer L - 1 at the rows of F1 only
 *              (spex_spmm_rowlist_dev_f32, the same table and, at L >= 4, the same running sum, valid at F1); the batch kernel is
 *              unchanged: everything it reads of layer L - 1 lies in F1.
 *   backward:  the batch kernel's push leaves P = G_(L-1) = (g + A^T g) / (L + 1), whose support lies in F1.  The next product
 *              A^T P is a PUSH over the F1 list (spex_spmm_push_rows_scaled_f32 over `graph`, float atomics) into a table zeroed by a
 *              launch of the step: grad_E0 at L == 2 (the Adam pass adds g_out / 3 as without the flag), ws_bwd[1] at L >= 3 (L == 3:
 *              plain, the Adam pass adds P; L >= 4: with the g_out / (L + 1) term).  The remaining L - 2 products are whole-graph pulls.
 * L == 2 has no whole-graph launch left.  The exact BPR step takes the push form at any T.  Refused before anything touches the device
 * (t not advanced): d != 64 or SPEX_STEP_WIDE -> SPEX_ERR_UNSUPPORTED; L < 2, SPEX_STEP_DETERMINISTIC (the second push uses float
 * atomics), SPEX_STEP_BPR_DENSE, a NULL frontier_* field -> SPEX_ERR_INVALID.
 * Under edge dropout (a mask on both handles, also the epochs' keep_prob < 1; fp32 tables) the step is the whole-graph
 * masked step on the masked adjacency A_m: the lists are built behind the step's mask by spex_frontier_rows_masked_i32 — F1 = Bset U
 * the columns of KEPT entries of Bset's rows, which holds everything the masked batch kernel reads and pushes into —, layer L - 1 and
 * the push over F1 follow the handle's mask (spex_spmm_rowlist_dev_f32, spex_spmm_push_rows_scaled_f32), and SPEX_STEP_SPARSE_ADAM's F2
 * is the masked two-hop set: the rows that can receive a gradient under this step's mask.  The rule of every masked step holds:
 * graph_t is the transposed handle with its edge-id permutation and the same mask, else SPEX_ERR_INVALID.  Together with
 * SPEX_STEP_BF16_GATHER a mask is refused ("does not combine with edge dropout", SPEX_ERR_INVALID): the bf16 list SpMM has no masked form.
 * With SPEX_STEP_BF16_GATHER (L = 2 or 3; that flag's own rules hold on top) the frontier launches read bf16 tables:
 *   forward:   L == 3: y_1 = A E0_16 over the whole graph (spex_spmm_bf16_f32 into ws_fwd[0] and ws16[0], the bf16 step's own launch),
 *              then y_2 at the rows of F1 from ws16[0] into ws_fwd[1] and ws16[1] (spex_spmm_rowlist_dev_bf16_f32).  L == 2: y_1 at F1
 *              from E0_16 into ws_fwd[0] and ws16[0]; no whole-graph launch is left.  The bf16 batch kernels gather from ws16[L - 2];
 *              everything they read lies in F1, and the layer sum uses the fp32 E0 and ws_fwd rows as without SPEX_STEP_FRONTIER.
 *   backward:  the frontier push reads the fp32 P.  L == 2: into grad_E0, done; the Adam pass adds g_out / 3.  L == 3: into
 *              W = ws_bwd[1], then one spex_cast_bf16_f32(W -> ws16[0]) and grad_E0 = A^T bf16(W) by one plain spex_spmm_bf16_f32 on
 *              graph_t; the Adam pass adds P.  Straight-through with ONE rounding, of W, where the whole-graph bf16 step has two
 *              (of P and of A^T bf16(P)).
 *   Adam:      the bf16 step's: E0_16 == bf16(E0) after every step.
 * Where the pair pays (one-call steps on an MI355X): at L == 3 on graphs that stream from HBM — 30.70 ms per BCE step
 * (B = 256) on a 2^24-node graph against 41.77 ms with SPEX_STEP_FRONTIER alone and 49.98 ms with SPEX_STEP_BF16_GATHER alone, 1.26 -
 * 1.39 x / 1.06 - 1.83 x over all L == 3 cells at 2^22 and 2^24 nodes.  Where it loses: at L == 2 it is 0 - 7 % slower than
 * SPEX_STEP_FRONTIER alone (9.82 against 9.18 ms; no whole-graph launch is left to halve, the Adam pass gains the shadow store), and
 * on a cache-resident graph (Epinion2) both flags lose to the plain fp32 step, together 186.9 us against 45.6 us. */
/* flags & SPEX_STEP_BF16_GATHER — the mixed-precision mode of spex_propagate_bf16_f32 carried through the one-call steps, d == 64,
 * L = 2 or 3 (spex_lightgcn_step_bce_f32, spex_lightgcn_step_bpr_adam_f32 and, through them, every epoch, sampled-epoch and
 * train_*_sampled call).  Rounding enters only where a table becomes a gather source; every product, sum and the layer mean stay
 * fp32, and the backward is straight-through, as in spex_propagate_bwd_bf16_f32.
 *   forward:   y_1 = A E0_16 (spex_spmm_bf16_f32: fp32 Y into ws_fwd[0], Y16 = bf16(y_1) into ws16[0] from the same register);
 *              L == 3: y_2 = A bf16(y_1) into ws_fwd[1] and ws16[1].  The batch kernel (spex_lightgcn_batch_bf16_f32 and its three
 *              siblings) gathers the last layer at the batch's rows from bf16(y_(L-1)) and forms
 *              light_r = (((E0[r] + y_1[r]) (+ y_2[r])) + y_L[r]) / (L + 1) with the exact fp32 E0 — spex_propagate_bf16_f32's mean_out
 *              rows; scores, loss, gradient rows, L2 counts and the push are the fp32 kernel's statements on fp32 slots.
 *   backward, push form: P = (g + A^T g) / (L + 1) arrives in fp32 as without the flag; one spex_cast_bf16_f32 launch makes it a
 *              gather source in ws16[0] (the forward's bf16 tables are dead by then).  L == 3: G16 = bf16(A^T bf16(P)) (bf16 output
 *              only, ws16[1]), grad_E0 = A^T G16, and the Adam pass adds P.  L == 2: grad_E0 = A^T bf16(P), the Adam pass adds
 *              g_out / (L + 1).  2 L + 1 launches.
 *   backward, dense form (BPR, large T) and SPEX_STEP_DETERMINISTIC: spex_propagate_bwd_bf16_f32(graph_t, g_out, grad_E0, ws_bwd,
 *              ws16, L, 64) in place of spex_propagate_bwd_f32; the same buffers are left all-zero for the next step.
 *   Adam:      writes the new E0 and E0_16 = bf16(new E0), round to nearest even, from the same register: after every step E0_16
 *              equals spex_cast_bf16_f32(E0) bit for bit, and no cast launch opens a step.
 *   Edge dropout: the handles' mask, in the whole-graph launches (spex_spmm_bf16_f32) and entry by entry in the batch kernels.
 * Refused before anything touches the device (t is not advanced): any other d or L, or a handle without chunk tables ->
 * SPEX_ERR_UNSUPPORTED; E0_16 or ws16 NULL, not 16-byte aligned, or overlapping each other or another buffer of the descriptor, and
 * SPEX_STEP_WIDE together with the flag -> SPEX_ERR_INVALID.  A caller that writes E0 itself re-casts it (spex_cast_bf16_f32) first. */
/* (On a descriptor shared with the exact BPR step: this call advances t and leaves row_counts alone.  The BPR step counts into the
 * table of its own t's parity and relies on the step before it to have cleared that table, so clear both tables — one memset of
 * 8 N bytes — between a BPR step and the next one whenever a BCE step, or a BCE epoch, ran in between; an odd number of BCE steps
 * otherwise leaves the next BPR step adding to the counts of the one before: a stale L2 gradient.) */
int spex_lightgcn_step_bce_f32(spex_lightgcn_step_t *step, const int64_t *users, const int64_t *items, const float *labels,
                               int32_t B, float *loss_sum, void *stream);
/* Train() of main_rec.py:30-37 over a whole pre-shuffled, device-resident epoch as ONE call: batch k = samples [k B, min((k+1) B, n))
 * through spex_lightgcn_step_bce_f32 (at most max_steps batches; < 0: all).  *loss_full accumulates the loss sums of the full batches,
 * *loss_ragged that of a shorter last batch (main_rec.py:36 adds per-batch MEAN losses: loss_full / B + loss_ragged / (n mod B)).
 * keep_prob < 1: edge dropout (model.py:46-55) with the in-kernel sampled mask, a fresh one per step — seed = (drop_seed << 32) | step,
 * steps counted from 1, exactly what spex_graph_set_edge_mask(g, 2, NULL, keep_prob, seed) on both handles before each step gives; the
 * handles are left unmasked.  (The descriptor's graph handles are modified by that: not const here.) */
int spex_lightgcn_epoch_bce_f32(spex_lightgcn_step_t *step, const int64_t *users, const int64_t *items, const float *labels, int64_t n,
                                int32_t B, int64_t max_steps, float keep_prob, uint32_t drop_seed, float *loss_full, float *loss_ragged,
                                void *stream);

/* The exact BPR training step — upstream LightGCN's training semantics: BPR differentiated through the propagation, an L2 term on
 * the E0 rows of the batch, Adam — as ONE call with the schedule of spex_lightgcn_step_bce_f32 and the triple-shaped batch kernel
 * (spex_lightgcn_bpr_batch_f32; at d = 128 / 256 spex_lightgcn_bpr_batch_wide_f32) in the middle.  d == 64 — any other width is
 * rejected — unless flags carries SPEX_STEP_WIDE: then d = 128 or 256 (any other width is rejected) and every table and slot of the
 * descriptor is d wide; the epoch and sampled-epoch calls below go through this step and take the same descriptors.  The descriptor's buffers as for the BCE step, with slot_capacity >= 3 T and row_counts [2, N] int32 (all-zero before the
 * first call; every call leaves the table of the next step's parity all-zero — and expects the table of its OWN parity all-zero on
 * entry: advance t by no other call without clearing both tables, see spex_lightgcn_step_t).
 *   loss = mean_t softplus(xn_t - xp_t) + weight_decay * 0.5 * sum_t (|E0[u_t]|^2 + |E0[p_t]|^2 + |E0[n_t]|^2) / T
 *   fast path: L-1 x spex_spmm_f32 (plain for L <= 3) -> spex_lightgcn_bpr_batch_f32 -> L-1 x spex_spmm_f32 on A^T (all plain at
 *   L == 3) -> Adam (sums the per-triple losses in order, adds the L2 gradient): 2 L launches.  From 768 (d = 64), 1 024 (d = 128) or 512 (d = 256) triples up (measured on Epinion2;
 *   SPEX_STEP_BPR_DENSE / SPEX_STEP_BPR_PUSH force either form) the same batch launch skips the push — its gradient rows go to the
 *   dense g_out with atomics — and spex_propagate_bwd_f32 runs the whole backward in pull form.
 *   SPEX_STEP_DETERMINISTIC: spex_lightgcn_bpr_batch_slots_f32 -> spex_reduce_slots_f32 (users; then pos and neg) ->
 *   spex_propagate_bwd_f32 -> Adam; no float atomic, two runs from one state are bit-identical.
 * The L2 gradient weight_decay / T * E0[r] per occurrence of row r in the batch is not propagated: the batch kernel counts the
 * occurrences (integer atomics) in row_counts[(t + 1) & 1] and the Adam pass adds count * E0 and clears the other table.
 * users / pos / neg: device int64[T] (items index the item block); a triple with any index out of range is skipped whole.
 * *loss_sum accumulates the batch's loss SUM (softplus plus the L2 share).  grad_E0 holds the step's whole gradient afterwards.
 * Edge dropout: the rules and argument checks of the BCE step (same mask on both handles, graph_t the transposed handle, L >= 2).
 * t is advanced only when every launch of the step was queued. */
int spex_lightgcn_step_bpr_adam_f32(spex_lightgcn_step_t *step, const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T,
                                    float *loss_sum, void *stream);
/* An epoch of pre-drawn, device-resident triples as ONE call: batch k = triples [k T, min((k+1) T, n)) through
 * spex_lightgcn_step_bpr_adam_f32 (at most max_steps batches; < 0: all); loss_full / loss_ragged, keep_prob and the mask keying
 * ((drop_seed << 32) | (k + 1)) as in spex_lightgcn_epoch_bce_f32; the handles are left unmasked. */
int spex_lightgcn_epoch_bpr_f32(spex_lightgcn_step_t *step, const int64_t *users, const int64_t *pos, const int64_t *neg, int64_t n,
                                int32_t T, int64_t max_steps, float keep_prob, uint32_t drop_seed, float *loss_full, float *loss_ragged,
                                void *stream);
/* A sampled epoch with nothing crossing the host: ONE spex_sample_bpr_triples launch (tables, num_item, n, mode, seed, epoch as
 * there) into the caller-owned index buffers users / pos / neg (device int64[n] each), then exactly the loop of
 * spex_lightgcn_epoch_bpr_f32 over them (T, max_steps, keep_prob, drop_seed, loss_full, loss_ragged as there; drop_seed is used as
 * given).  The arguments of both are checked before anything is launched (the descriptor's fields are the step's to check: a
 * descriptor it rejects ends the call after the draw, with no step run); n == 0 launches nothing. */
int spex_lightgcn_epoch_bpr_sampled_f32(spex_lightgcn_step_t *step, const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                        const int32_t *d_active, int32_t n_active, int32_t num_item, int64_t n, int32_t mode, uint64_t seed,
                                        uint32_t epoch, int32_t T, int64_t max_steps, float keep_prob, uint32_t drop_seed, int64_t *users,
                                        int64_t *pos, int64_t *neg, float *loss_full, float *loss_ragged, void *stream);
/* n_epochs sampled epochs (epoch numbers epoch0 .. epoch0 + n_epochs - 1, modulo 2^32) back to back on one stream, no host thread
 * and no synchronisation between them: epoch e's loss sums accumulate into loss_epochs[2 e] (full batches) and loss_epochs[2 e + 1]
 * (the ragged last batch); loss_epochs: device float[2 n_epochs].  One set of index buffers serves every epoch: stream order puts
 * the sampler of epoch e + 1 behind the last step of epoch e.  Under edge dropout (keep_prob < 1) epoch number E runs with the mask
 * seed  drop_seed + 0x9E3779B9 * E  (modulo 2^32)  in place of drop_seed, so that no two epochs replay one mask sequence (epoch 0:
 * drop_seed itself); step k of that epoch is keyed (that seed << 32) | (k + 1) as in spex_lightgcn_epoch_bpr_f32. */
int spex_lightgcn_train_bpr_sampled_f32(spex_lightgcn_step_t *step, const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                        const int32_t *d_active, int32_t n_active, int32_t num_item, int64_t n, int32_t mode, uint64_t seed,
                                        uint32_t epoch0, int32_t n_epochs, int32_t T, int64_t max_steps, float keep_prob, uint32_t drop_seed,
                                        int64_t *users, int64_t *pos, int64_t *neg, float *loss_epochs, void *stream);

/* A sampled BCE epoch with nothing crossing the host: ONE spex_sample_bce_epoch launch (tables, positives, num_ng, num_item, seed,
 * epoch as there) into the caller-owned buffers users / items (device int64[n] each) and labels (device float[n]),
 * n = n_pos (1 + num_ng), then exactly the loop of spex_lightgcn_epoch_bce_f32 over them (B, max_steps, keep_prob, drop_seed,
 * loss_full, loss_ragged as there; drop_seed is used as given).  The arguments of both are checked before anything is launched (the
 * descriptor's fields are the step's to check: a descriptor it rejects ends the call after the draw, with no step run); n_pos == 0
 * launches nothing. */
int spex_lightgcn_epoch_bce_sampled_f32(spex_lightgcn_step_t *step, const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                        const int32_t *d_pos_user, const int32_t *d_pos_item, int64_t n_pos, int32_t num_ng, int32_t num_item,
                                        uint64_t seed, uint32_t epoch, int32_t B, int64_t max_steps, float keep_prob, uint32_t drop_seed,
                                        int64_t *users, int64_t *items, float *labels, float *loss_full, float *loss_ragged, void *stream);
/* n_epochs sampled BCE epochs (epoch numbers epoch0 .. epoch0 + n_epochs - 1, modulo 2^32) back to back on one stream, no host
 * thread and no synchronisation between them: epoch e's loss sums accumulate into loss_epochs[2 e] (full batches) and
 * loss_epochs[2 e + 1] (the ragged last batch); loss_epochs: device float[2 n_epochs].  One set of buffers serves every epoch: stream
 * order puts the sampler of epoch e + 1 behind the last step of epoch e.  Under edge dropout (keep_prob < 1) epoch number E runs with
 * the mask seed  drop_seed + 0x9E3779B9 * E  (modulo 2^32)  in place of drop_seed — spex_lightgcn_train_bpr_sampled_f32's rule — so
 * that no two epochs replay one mask sequence; step k of that epoch is keyed (that seed << 32) | (k + 1). */
int spex_lightgcn_train_bce_sampled_f32(spex_lightgcn_step_t *step, const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                        const int32_t *d_pos_user, const int32_t *d_pos_item, int64_t n_pos, int32_t num_ng, int32_t num_item,
                                        uint64_t seed, uint32_t epoch0, int32_t n_epochs, int32_t B, int64_t max_steps, float keep_prob,
                                        uint32_t drop_seed, int64_t *users, int64_t *items, float *labels, float *loss_epochs, void *stream);

/* The single-layer NGCF training step (NGCF_SPEX/code/main_rec.py:122-128 with the default --layer_size [64]) as one call:
 *   spex_spmm_f32 (side = A ego) -> spex_ngcf_layer_fwd_f32 -> spex_ngcf_score_bwd_rows_f32 (scores, BCE, rows backward)
 *   -> spex_spmm_push_batch_f32 -> spex_adam_step_f32 (table; clears its gradient, adds the step's per-sample losses to
 *   loss_sum in a fixed order) -> spex_adam_step_sum_f32 (layer weights).  Six launches.
 * Buffers (caller-owned, N = graph rows incl. an isolated pad row if the table keeps one, d == 64):
 *   E0, mE, vE, side, grad: [N, d] (grad all-zero before the first call; every call leaves it all-zero);  all_emb: unused since ABI 5
 *   (the step no longer forms the concatenated table; the field keeps the layout, NULL is accepted);
 *   W, mW, vW: the layer's weights as one block [W_gc d*d | b_gc d | W_bi d*d | b_bi d] and its Adam moments;
 *   g_slots: [slot_capacity, 2d];  g_side_c, g_ego_c: [slot_capacity, d];  gW_parts: [slot_capacity / 16, 2 (d*d + d)].
 * users index rows [0, n_user_rows), items rows n_user_rows + items[b].  Message dropout: (p_drop, seed, dropout_step, layer 0),
 * dropout_step advanced by the call when p_drop > 0; t advanced by the call.
 */
typedef struct spex_ngcf_step {
    const spex_graph_t *graph;               /* A = D^-1 (A + I) */
    float *E0, *mE, *vE, *W, *mW, *vW;
    float *all_emb, *side, *g_slots, *g_side_c, *g_ego_c, *gW_parts, *grad;
    int32_t slot_capacity, n_user_rows, pad_row;
    float slope, p_drop;
    uint64_t seed;
    int32_t dropout_step, t;
    float lr, beta1, beta2, eps;
    void *side_stream;   /* optional second hipStream_t of the caller (NULL: one stream): the layer weights' Adam pass runs on it
                          * beside the push-form product and the table's Adam pass and is joined at the end of the call.
                          * Measured SLOWER than one stream on the MI355X (69 vs 59 us per step: a cross-stream fork + join
                          * costs ~10 us, the hidden pass takes 5) — leave NULL unless the forked work is long */
    void *ev_fork, *ev_join;   /* the two-stream form's events: zero-initialise; created by the library on first use, one pair per
                                * descriptor; release with spex_step_events_release */
    const spex_graph_t *graph_t;             /* A^T — SPEX_STEP_DETERMINISTIC only (pull-form first backward product), else NULL */
    float *g_side_dense, *g_ego_dense;       /* [N, d] each, all-zero before the first call — SPEX_STEP_DETERMINISTIC only */
    int32_t flags;
} spex_ngcf_step_t;
int spex_step_events_release(void **ev_fork, void **ev_join);   /* destroys the pair a descriptor holds (no step in flight) */
int spex_ngcf_step_bce_f32(spex_ngcf_step_t *step, const int64_t *users, const int64_t *items, const float *labels, int32_t B,
                           float *loss_sum, void *stream);
/* train() of NGCF_SPEX/code/main_rec.py:116-131 over a whole pre-shuffled, device-resident epoch as ONE call: batch k = samples
 * [k B, min((k+1) B, n)) through spex_ngcf_step_bce_f32 (at most max_steps batches; < 0: all); *loss_full / *loss_ragged as in
 * spex_lightgcn_epoch_bce_f32. */
int spex_ngcf_epoch_bce_f32(spex_ngcf_step_t *step, const int64_t *users, const int64_t *items, const float *labels, int64_t n, int32_t B,
                            int64_t max_steps, float *loss_full, float *loss_ragged, void *stream);
/* A sampled NGCF epoch with nothing crossing the host: ONE spex_sample_ngcf_epoch launch (tables, seed, epoch as there) into the
 * caller-owned buffers users / items (device int64[n] each) and labels (device float[n]), n = 6 n_pos, then exactly the loop of
 * spex_ngcf_epoch_bce_f32 over them (B, max_steps, loss_full, loss_ragged as there).  The arguments of both are checked before anything
 * is launched (the descriptor's fields are the step's to check: a descriptor it rejects ends the call after the draw, with no step
 * run); n_pos == 0 launches nothing.  Single-layer model only, like the native epoch. */
int spex_ngcf_epoch_bce_sampled_f32(spex_ngcf_step_t *step, const int32_t *d_pop, int32_t n_pop, const int32_t *d_user, int32_t n_users,
                                    const int32_t *d_pos_off, const int32_t *d_pos_item, int64_t n_pos, const int32_t *d_row_off,
                                    const int32_t *d_row_rank, uint64_t seed, uint32_t epoch, int32_t B, int64_t max_steps, int64_t *users,
                                    int64_t *items, float *labels, float *loss_full, float *loss_ragged, void *stream);
/* n_epochs sampled NGCF epochs (epoch numbers epoch0 .. epoch0 + n_epochs - 1, modulo 2^32) back to back on one stream, no host thread
 * and no synchronisation between them: epoch e's loss sums accumulate into loss_epochs[2 e] (full batches) and loss_epochs[2 e + 1]
 * (the ragged last batch); loss_epochs: device float[2 n_epochs].  One set of buffers serves every epoch: stream order puts the sampler
 * of epoch e + 1 behind the last step of epoch e.  Message dropout needs no per-epoch reseed (the LightGCN calls reseed their edge
 * masks per epoch because those are keyed by the step WITHIN the epoch): its mask is keyed by the descriptor's dropout_step, which
 * every step advances and which runs on across the epochs of one call exactly as across per-epoch calls. */
int spex_ngcf_train_bce_sampled_f32(spex_ngcf_step_t *step, const int32_t *d_pop, int32_t n_pop, const int32_t *d_user, int32_t n_users,
                                    const int32_t *d_pos_off, const int32_t *d_pos_item, int64_t n_pos, const int32_t *d_row_off,
                                    const int32_t *d_row_rank, uint64_t seed, uint32_t epoch0, int32_t n_epochs, int32_t B,
                                    int64_t max_steps, int64_t *users, int64_t *items, float *labels, float *loss_epochs, void *stream);

/* NGCF with MORE than one layer (`--layer_size [64,64,..]`, NGCF_SPEX/code/ngcf_parser.py:12; the layer loop of main_rec.py:71-93) —
 * the training step as one call of the library's own launches, L >= 2 layers of width 64:
 *   forward   layers 0 .. L-2 over the whole table (spex_spmm_f32 -> spex_ngcf_layer_fwd_f32: their outputs feed the next layer's
 *             product everywhere); the LAST layer at the batch's rows only (spex_spmm_rowlist_f32 -> spex_ngcf_layer_fwd_rows_f32: the
 *             loss reads the concatenated table nowhere else, main_rec.py:96-104)
 *   scoring   spex_score_bce_slots_f32 on the concatenated table [N, 64 (L + 1)]: per-sample gradient rows + the table form the
 *             earlier layers read
 *   backward  last layer on the batch's slots (spex_ngcf_layer_bwd_rows_f32) -> push-form A^T product (spex_spmm_push_batch_f32) ->
 *             for l = L-2 .. 0: spex_ngcf_layer_bwd_f32 (dense, four waves per tile) -> spex_spmm_f32 on A^T with g_ego added
 *   Adam      the table; the last layer's weights from their partial blocks; the other layers' weights (their pass clears gW).
 * Buffers (caller-owned; N = graph rows incl. the isolated pad row if the table keeps one; per = 2 (64 * 64 + 64)):
 *   E0, mE, vE: [N, 64];  W, mW, vW, gW: [L][per] (layer l: [W_gc | b_gc | W_bi | b_bi]; gW all-zero before the first call, every call
 *   leaves it so);  all_emb, g_all: [N, 64 (L + 1)] (g_all all-zero before the first call; every call leaves it so);
 *   sides: [L][N, 64];  egos: [L - 1][N, 64] (the inputs of layers 1 .. L-1);  g_slots: [slot_capacity, 64 (L + 1)];
 *   g_side_c, g_ego_c: [slot_capacity, 64];  gW_parts: [slot_capacity / 16, per];  g_side, g_ego: [N, 64];  g_next: [2][N, 64].
 * p_drop: host [L] (message dropout per layer), mask = (seed, dropout_step, layer); dropout_step advanced when any p_drop > 0;
 * t advanced by the call.  Float atomics in the scoring tables and the push (no deterministic mode for L >= 2). */
typedef struct spex_ngcf_deep_step {
    const spex_graph_t *graph, *graph_t;     /* A = D^-1 (A + I) and its transpose */
    float *E0, *mE, *vE, *W, *mW, *vW, *gW;
    float *all_emb, *g_all, *sides, *egos, *g_slots, *g_side_c, *g_ego_c, *gW_parts, *g_side, *g_ego, *g_next;
    const float *p_drop;
    int32_t L, slot_capacity, n_user_rows, pad_row;
    float slope;
    uint64_t seed;
    int32_t dropout_step, t;
    float lr, beta1, beta2, eps;
} spex_ngcf_deep_step_t;
int spex_ngcf_deep_step_bce_f32(spex_ngcf_deep_step_t *step, const int64_t *users, const int64_t *items, const float *labels, int32_t B,
                                float *loss_sum, void *stream);

/* The dual-task training step of LightGCN_SPEX/code/main_auto_expert_s.py:63-89 (model_expert_s.LightGCN.forward flag 0 +
 * uncertainty-weighted loss + loss.backward() + optimizer.step()) as one call issuing 2 L + 3 launches:
 *   rec branch, row-sparse like spex_lightgcn_step_bce_f32: (L-1) x spex_spmm_f32 + spex_gated_batch_f32 (last layer at the
 *   batch's rows, gate, scores, the gate's backward and the push-form first backward product: one launch; the deterministic
 *   step and L == 1: spex_gated_batch_fwd_f32 -> spex_expert_gate_rows_bwd_[det_]f32 -> push / pull) -> (L-1) x spex_spmm_f32 on
 *   A^T (L == 3: both in the plain form, the Adam pass adds the push target);   trust branch: spex_trust_head_train_f32;
 *   then one Adam pass over the whole parameter arena, which applies the task precisions exp(-2 s_k) to the two branches'
 *   gradients, forms the task weights' own gradients (d/ds0 = -2 p1 loss1 + 2 (n_rec + 1) B, d/ds1 = -2 p2 loss2 + T) and
 *   clears every accumulate-into buffer for the next step.
 * params / m / v: ONE arena (and its two Adam moments), N = graph rows, P = spex_trust_param_count(64, n_heads):
 *   [ table N*64 (users incl. pad row, then items) | trust block P | att_exp1 256 | att_exp2 256 | task_weights 2 ]
 * Work buffers (caller-owned): light, lo_batch, g_prop, g_raw, g_E0: [N, 64]; ws_fwd [2, N, 64]; ws_bwd [3, N, 64];
 *   mixed_slots, grad_slots, g_prop_slots: [slot_capacity, 64] with slot_capacity >= 2B; arange: int64 [slot_capacity] = 0, 1, ..;
 *   g_user [n_user_rows, 64]; g_small [P + 512]; a2 [path_capacity, 64]; trust_ws
 *   [spex_trust_workspace_floats(path_capacity, path_len, 64, n_heads, n_user_rows)]; dscore [path_capacity, n_user_rows - 1];
 *   loss_b [path_capacity]; loss [2], loss_acc [2], precision [2][2].
 * Before the first call: g_prop, g_raw, the first [N, 64] of ws_bwd, g_user, g_small, loss AND grad_slots all-zero (every call
 * leaves them so: on the fast path — no SPEX_STEP_DETERMINISTIC, L >= 2 — the first min(64, slot_capacity / 8) x 512 floats of
 * grad_slots hold the copies of the two gate gradients that spex_gated_batch_f32 accumulates, summed and cleared by the Adam pass;
 * the other paths use the area for per-sample rows and the Adam pass clears it behind them); precision[(t + 1) & 1] = {exp(-2 s0), exp(-2 s1)} for the current task weights (every call writes the next step's
 * slot).  loss_acc accumulates (loss1, loss2) of every call — what Train() sums with .item() per step.  t is advanced.
 * seq: [T, path_len] int64 padded with the pad row's index n_user_rows - 1; T == 0 skips the trust branch (the reference
 * would produce NaN there: CrossEntropyLoss over an empty batch).  L >= 1.  Edge dropout (model_expert_s.py:104-109; the
 * reference's recommended `--dropout 1 --keepprob 0.3`): the step's mask on BOTH handles before the call, graph_t the transposed
 * handle with the edge-id permutation, L >= 2 — as in spex_lightgcn_step_bce_f32.
 * Two streams: the rec branch (2L + 4 launches that fill the chip) and the trust branch (two launches of <= path_capacity
 * workgroups: a latency chain on a few CUs) read the same parameters and write disjoint buffers, so with side_stream set
 * the trust branch is forked onto it behind everything already queued on `stream` and joined again in front of the Adam
 * pass (two events per device, created on first use and kept by the library).  Results are identical to the one-stream
 * order; the caller keeps side_stream alive while steps are in flight.
 * flags & SPEX_STEP_PIPELINED (needs side_stream): the fork and the join above cost ~10 us each on this runtime and sit on the
 * step's critical cycle (Adam -> fork -> trust branch -> join -> Adam).  The pipelined form takes them off it by splitting the
 * Adam pass by OWNER: the user rows, the trust block and the task weights — everything the trust branch reads or writes — are
 * updated by a second Adam launch on side_stream, right behind the trust branch (it waits for the rec branch's gradients, which
 * are ready long before); the item rows and the gate matrices by the launch on `stream`.  The trust branch of step k+1 then
 * follows step k's update on its own stream with no event between them, and `stream` waits for the side update at the START
 * of the next call (its rec branch reads the user rows).  Same arithmetic, same results.  The price is the contract: when the
 * call returns, side_stream is still AHEAD of `stream` — the next pipelined call picks that up itself, anything else that reads
 * or writes the parameters, the moments, loss_acc or the work buffers must be ordered behind spex_dual_task_step_join(step,
 * stream); and seq / seq_l / targets are read on side_stream WITHOUT waiting for `stream` (only the first call after a join
 * forks from it), so they must have been complete before the last join — e.g. staged once per epoch, as Train() allows.
 */
typedef struct spex_dual_task_step {
    const spex_graph_t *graph, *graph_t;
    float *params, *m, *v;
    float *light, *ws_fwd, *lo_batch, *g_prop, *g_raw, *g_E0, *ws_bwd;
    float *mixed_slots, *grad_slots, *g_prop_slots;
    const int64_t *arange;
    float *g_user, *g_small;
    float *a2, *trust_ws, *dscore, *loss_b;
    float *loss, *loss_acc, *precision;
    int32_t slot_capacity, path_capacity, path_len, n_user_rows, L, d, n_heads, hybrid, n_rec;
    float lr, beta1, beta2, eps;
    int32_t t;
    void *side_stream;   /* optional second hipStream_t of the caller (NULL: one stream): the trust branch is issued on it and runs
                          * CONCURRENTLY with the rec branch — the two only meet in the Adam pass (see below) */
    void *ev_fork, *ev_join;   /* as in spex_ngcf_step_t: zero-initialise, release with spex_step_events_release */
    float *g_raw_slots;        /* [slot_capacity, 64]                                   — SPEX_STEP_DETERMINISTIC only */
    float *att_parts;          /* [spex_expert_gate_rows_bwd_parts(slot_capacity)][512] — SPEX_STEP_DETERMINISTIC only */
    float *loss_rows;          /* [slot_capacity / 2] per-sample rec losses             — SPEX_STEP_DETERMINISTIC only */
    int32_t flags;             /* SPEX_STEP_DETERMINISTIC | SPEX_STEP_FIXED_TASK_WEIGHTS | SPEX_STEP_PIPELINED */
    int32_t side_pending;      /* state of the pipelined form (zero-initialise): work of this descriptor is in flight on side_stream */
} spex_dual_task_step_t;
int spex_dual_task_step_f32(spex_dual_task_step_t *step, const int64_t *users, const int64_t *items, const float *labels, int32_t B,
                            const int64_t *seq, const int64_t *seq_l, const int64_t *targets, int32_t T, void *stream);
/* Train() of main_auto_expert_s.py:60-91 over a whole pre-shuffled, device-resident epoch as ONE call: batch k = samples
 * [k B, min((k+1) B, n)) (at most max_steps batches; < 0: all) with the paths [path_off[k], path_off[k+1]) of the epoch's staged path
 * arrays — seq [n_paths, path_len], seq_l, targets on the device, path_off a HOST array of n_batches + 1 ascending offsets (the
 * reference selects each batch's paths with random.sample, :64-71: done up front on the host) — through spex_dual_task_step_f32; the
 * losses accumulate in the descriptor's loss_acc.  keep_prob < 1: the rec branch's sampled edge mask, a fresh one per step, as in
 * spex_lightgcn_epoch_bce_f32.  With SPEX_STEP_PIPELINED, finish with spex_dual_task_step_join. */
int spex_dual_task_epoch_f32(spex_dual_task_step_t *step, const int64_t *users, const int64_t *items, const float *labels, int64_t n,
                             int32_t B, int64_t max_steps, const int64_t *seq, const int64_t *seq_l, const int64_t *targets,
                             const int64_t *path_off, float keep_prob, uint32_t drop_seed, void *stream);
/* spex_dual_task_epoch_f32 over paths staged with a fixed stride — the layout spex_sample_dual_task_paths writes (path_stride = its
 * cap): batch k's paths are the first h_count[k] rows from row k path_stride of seq / seq_l / targets.  h_count: a HOST int32 array of
 * one count per batch run (the step needs T on the host: the trust launch's grid and the T task_weights[1] term of the loss).
 * Returns SPEX_ERR_INVALID before any launch for a count < 0, > path_stride or > the descriptor's path_capacity.  Edge-dropout keys,
 * loss_acc and max_steps as in spex_dual_task_epoch_f32. */
int spex_dual_task_epoch_strided_f32(spex_dual_task_step_t *step, const int64_t *users, const int64_t *items, const float *labels, int64_t n,
                                     int32_t B, int64_t max_steps, const int64_t *seq, const int64_t *seq_l, const int64_t *targets,
                                     int64_t path_stride, const int32_t *h_count, float keep_prob, uint32_t drop_seed, void *stream);
/* Orders everything a pipelined step left on side_stream in front of whatever is queued on `stream` next (a no-op otherwise). */
int spex_dual_task_step_join(spex_dual_task_step_t *step, void *stream);

/* ------------------------------------------------------------------------------------------------ multi-GPU: collectives + partitioned step
 * the graph is 1-D row-partitioned over the GPUs of one node (one process per GPU): rank p owns rows
 * [r_p, r_{p+1}) of A (and of A^T), of every layer's table and of the Adam moments; a layer is an all-gather of the current
 * layer's rows over xGMI followed by the local SpMM.  The reference's analogue is the serial fold loop of --A_split
 * (LightGCN_SPEX/code/utility1/model.py:84-89, dataloader.py:167-177).  Layout: shards are padded to max_rows = the largest
 * shard, the gathered table is [world * max_rows, d] (rank q's rows in slot q), and a rank's block of A has its column indices
 * rewritten once into that layout, so the SpMM reads the gathered buffer as it arrives.
 * The collectives run on RCCL, bound at run time (dlopen: the library loads without RCCL; inside a PyTorch process the
 * librccl torch already holds is the one used).  Errors: SPEX_ERR_COMM with the RCCL message in spex_last_error().
 */
#define SPEX_COMM_ID_BYTES 128
typedef struct spex_comm spex_comm_t;
/* id_out: SPEX_COMM_ID_BYTES bytes (an ncclUniqueId), created on ONE rank and handed to all by the host (any transport). */
int spex_comm_unique_id(void *id_out);
/* Collective over all `world` ranks (ncclCommInitRank), on the calling thread's current device. */
int spex_comm_create(int32_t rank, int32_t world, const void *unique_id, spex_comm_t **out);
int spex_comm_destroy(spex_comm_t *comm);
int spex_comm_info(const spex_comm_t *comm, int32_t *rank, int32_t *world);
/* All-gather of row shards: send = this rank's rows ([<= max_rows, d], padded shard), recv = the gathered table
 * [world * max_rows, d].  rows_per_rank == NULL: one equal-size ncclAllGather of the padded shards (world * max_rows rows on
 * the wire).  rows_per_rank (host, [world]): only the REAL rows move, as one group of point-to-point sends / receives — rank p's
 * rows straight into slot p of every peer's table, world - 1 transfers in flight at once (one per xGMI link of the full mesh,
 * where a ring serialises world - 1 steps over one link); the slots' padding tails are never written nor read.  send may be
 * recv's own slot.  Asynchronous on `stream`. */
int spex_comm_allgather_rows_f32(spex_comm_t *comm, const float *send, float *recv, int64_t max_rows, int32_t d,
                                 const int32_t *rows_per_rank, void *stream);
/* In-place sum over ranks (the owner-computes exchange of a batch's rows: every rank contributes the rows it owns to a zero-filled
 * buffer). */
int spex_comm_allreduce_sum_f32(spex_comm_t *comm, float *buf, int64_t n, void *stream);

/* The row-partitioned propagation / exact training step as one native call each (what spex_amd/dist.py's PartitionedLightGCN.
 * propagate and PartitionedStepper.step_bce issue launch by launch):
 *   spex_partitioned_propagate_f32: L x (exchange of the current rows, spex_spmm_f32 on the rank's block with the running layer
 *     sum fused) -> light_out = the rank's rows of mean(E^0 .. E^L)                    (utility1/model.py:66-97)
 *   spex_partitioned_step_bce_f32: that forward; the batch's 2B propagated rows fetched owner-computes
 *     (spex_gather_owned_rows_f32 + one all-reduce of 2B rows); scores + BCE + gradient rows on the compact rows; the rows this
 *     rank owns added into its gradient block (spex_scatter_add_owned_rows_f32 — or, with SPEX_STEP_DETERMINISTIC, per-sample
 *     rows added in slot order by spex_reduce_slots_f32); backward G_l = g / (L+1) + A^T G_{l+1} as L x (exchange, SpMM on the
 *     block of A^T); Adam on the rank's rows.  2 L exchanges + 1 small all-reduce per step, no host work between launches.
 *   Every exchange is IN PLACE: a layer's SpMM writes its output into the rank's own slot (rows rank * max_rows ..) of the table the
 *   next exchange completes (gathered and gathered1 alternate), so no send buffer and no copy of a layer's rows exist (before: 2 L
 *   staging copies per step).
 *   FAST PATH of spex_partitioned_step_bce_f32 (gathered2 given, L >= 2, not deterministic; the same choice on EVERY rank — the two
 *   schedules differ in their collectives) — spex_lightgcn_step_bce_f32's schedule on the partition: forward layers 1 .. L-1 over the
 *   block (plain form for L <= 3), the LAST layer at the batch's rows on their owners (spex_spmm_owned_rows_f32) -> the all-reduce of
 *   2B rows -> scores, BCE, gradient rows, the owner-computes adds AND the backward's FIRST product in push form in ONE launch on the
 *   replicated rows — no exchange for it: every rank holds all 2B gradient rows and pushes them through graph_push = its own
 *   columns of A -> L - 1 pull-form products on A^T's block, the last one plain (Adam adds its g / (L+1) share; L == 3: both plain,
 *   Adam adds the push target).  2 L - 1 exchanges + 1 all-reduce.  graph_push: handle of the (world * max_rows) x n_local matrix
 *   whose row p holds A[p, c] for the columns c the rank owns (local column indices) = the transpose of the rank's block of A^T;
 *   gathered2 [world * max_rows, 64]: its own slot is the push target, all-zero before the first call (the Adam pass leaves it so).
 * pos: device int64 [2B] — the batch's rows in the padded gathered layout (users, then items): owner(r) * max_rows + r - r_owner.
 * The batch is replicated on every rank; every rank accumulates the same loss sum into its own *loss_sum.
 * Buffers (caller-owned): E0, m, v, light_out, g_local, gs, grad_E0: [n_local, 64] (g_local all-zero before the first call;
 * every call leaves it so); gathered, gathered1: [world * max_rows, 64] each (two tables); rows, grad_rows: [slot_capacity, 64] with
 * slot_capacity >= 2B; arange: device int64 [slot_capacity] = 0, 1, 2, ...
 * graph / graph_t: this rank's row blocks (n_local rows, world * max_rows columns).  d == 64, L >= 1.
 * Edge dropout (utility1/model.py:46-64; since round 4): set the SAME mask on graph and graph_t (spex_graph_set_edge_mask), both created
 * with the entries' GLOBAL edge ids (spex_graph_create's edge_id: the entry's index in A; for the block of A^T the permutation), graph_t a
 * handle of its own — every rank then drops the same edges of A and of A^T.  The fast path stays available when graph_push carries the
 * same mask (and, per entry, the global edge id of the entry of A it came from): its rows-only layer and its push apply the keep rule
 * entry by entry; with an unmasked graph_push a masked step takes the launch-by-launch schedule. */
typedef struct spex_partitioned_step {
    const spex_graph_t *graph, *graph_t;
    spex_comm_t *comm;
    const int32_t *rows_per_rank;      /* host [world], or NULL: see spex_comm_allgather_rows_f32 */
    float *E0, *m, *v;
    float *light_out, *g_local, *gs, *grad_E0, *gathered1, *gathered, *rows, *grad_rows;
    const int64_t *arange;
    int32_t n_local, max_rows, slot_capacity, L, d;
    float lr, beta1, beta2, eps;
    int32_t t, flags;                  /* t is advanced by spex_partitioned_step_bce_f32; flags: SPEX_STEP_DETERMINISTIC */
    const spex_graph_t *graph_push;    /* fast path of spex_partitioned_step_bce_f32 (below); NULL on a rank without rows */
    float *gathered2;                  /* NULL: the launch-by-launch schedule */
} spex_partitioned_step_t;
int spex_partitioned_propagate_f32(spex_partitioned_step_t *step, void *stream);
int spex_partitioned_step_bce_f32(spex_partitioned_step_t *step, const int64_t *pos, const float *labels, int32_t B, float *loss_sum,
                                  void *stream);

/* BASELINE config 5's multi-GPU form — the dual-task step (LightGCN_SPEX/code/main_auto_expert_s.py:53-91 with
 * utility1/model_expert_s.py) on the row partition, as ONE native call:
 *   rec branch   L x (exchange, SpMM on the rank's block, running layer sum fused); the FIRST exchange's table (= E^0 of every rank)
 *                is kept in gathered0.  The batch's 2B rows of E^0 AND of the propagated table are fetched owner-computes (two
 *                spex_gather_owned_rows_f32 into one buffer, ONE all-reduce of 4B rows), and the gate (model_expert_s.py:154-161),
 *                the scores, the BCE loss and the gate's backward run on those compact rows — replicated: every rank computes the
 *                same 2B rows, so the two gate matrices' gradients are COMPLETE on every rank and need no collective (the Python
 *                schedule of round 3 gated all local rows and all-reduced 1 KB of gate gradients instead).  Each rank adds the
 *                gradient rows it owns into its blocks (d loss / d propagated rows -> backward L x (exchange, SpMM on the block of
 *                A^T); d loss / d E^0 rows directly).
 *   trust branch the user block of gathered0 gathered into the contiguous user_table ([n_user_rows, 64], user_pos = the user rows'
 *                positions in the padded layout) and spex_trust_head_train_f32 on it — redundantly on every rank (<= path_capacity
 *                paths), identical results by construction; with side_stream set it runs beside the rec branch (forked behind the
 *                first exchange, joined in front of the Adam pass).
 *   Adam         one pass over the rank's arena [n_local x 64 table rows | trust block P | att_exp1 256 | att_exp2 256 |
 *                task_weights 2]: owner-computes on the table rows (the rank's user rows take the trust head's table gradient at
 *                rows user_lo ..), replicated — identical gradients, identical updates — on the dense parameters; the task
 *                precisions and the task weights' own gradients as in spex_dual_task_step_f32.
 * 2 L exchanges + 1 all-reduce per step, every exchange in place (see spex_partitioned_step_t).  flags: SPEX_STEP_DETERMINISTIC (owned
 * rows added in slot order, no float atomics), SPEX_STEP_FIXED_TASK_WEIGHTS.  d == 64, L >= 1.  Edge dropout on the rec branch
 * (model_expert_s.py:104-109): as for spex_partitioned_step_t — the same mask on both handles (and on graph_push for the fast path).
 * FAST PATH (graph_push and gathered2 given, L >= 2, not deterministic) — spex_dual_task_step_f32's schedule on the partition:
 *   forward layers 1 .. L-1 over the block (plain form for L <= 3), the LAST layer at the batch's rows only, on their owners
 *   (spex_spmm_owned_rows_f32: layer mean + raw rows, zeros elsewhere) -> the one all-reduce of 4B rows -> gate, scores, BCE, the
 *   gate's backward, the owner-computes adds AND the backward's FIRST product in push form, in ONE launch on the replicated compact
 *   rows — that product needs NO exchange: every rank holds all 2B gradient rows and pushes them through graph_push = its own
 *   columns of A -> L - 1 pull-form products on A^T's block.  2 L - 1 exchanges + 1 all-reduce; 2 L - 2 whole-block launches instead
 *   of 2 L and two batch-sized launches instead of nine.  (grad_slots doubles as the gate gradients' scratch copies on this path; the
 *   trust branch's user block is gathered in front of the fork.)
 *   graph_push: handle of the (world * max_rows) x n_local matrix whose row p holds the entries A[p, c] for the columns c the rank
 *   owns (local column indices) — the transpose of the rank's block of A^T; gathered2 [world * max_rows, 64]: its own slot is the
 *   push target, all-zero before the first call (the Adam pass leaves it so).  gathered2 NULL: the launch-by-launch schedule above —
 *   the same choice on EVERY rank (the two schedules differ in their collectives); a rank without rows passes graph_push = NULL.
 * Buffers (caller-owned): params / m / v: the arena above; light, g_prop, g_raw, gs, g_E0: [n_local, 64] (g_prop, g_raw all-zero
 * before the first call; every call leaves them so); gathered, gathered1, gathered0 [world * max_rows, 64] (three tables);
 * rows [2 * slot_capacity, 64]; mixed_slots, grad_slots, g_prop_slots, g_raw_slots [slot_capacity, 64], slot_capacity >= 2B;
 * loss_rows [slot_capacity]; att_parts [spex_expert_gate_rows_bwd_parts(slot_capacity) * 512]; arange int64 [slot_capacity];
 * g_user [n_user_rows, 64] and g_small [P + 512] (both all-zero before the first call; the Adam pass leaves them so); a2, trust_ws, dscore, loss_b, loss [2],
 * loss_acc [2], precision [2][2] as in spex_dual_task_step_t (trust workspace sized for n_user_rows).
 * pos: device int64 [2B], the batch's rows in the padded layout (users, then items).  t is advanced by the call. */
typedef struct spex_partitioned_dual_step {
    const spex_graph_t *graph, *graph_t;
    spex_comm_t *comm;
    const int32_t *rows_per_rank;
    float *params, *m, *v;
    float *light, *g_prop, *g_raw, *gs, *g_E0, *gathered1, *gathered, *gathered0;
    const int64_t *user_pos;
    float *user_table;
    float *rows, *mixed_slots, *grad_slots, *g_prop_slots, *g_raw_slots, *loss_rows, *att_parts;
    const int64_t *arange;
    float *g_user, *g_small;
    float *a2, *trust_ws, *dscore, *loss_b;
    float *loss, *loss_acc, *precision;
    int32_t n_local, max_rows, n_local_users, user_lo;   /* the rank's first n_local_users rows are user rows user_lo .. */
    int32_t slot_capacity, path_capacity, path_len, n_user_rows, L, d, n_heads, hybrid, n_rec;
    float lr, beta1, beta2, eps;
    int32_t t;
    void *side_stream, *ev_fork, *ev_join;   /* optional second stream + the library's event cells (zero-initialise; release with
                                              * spex_step_events_release) */
    int32_t flags;
    const spex_graph_t *graph_push;          /* fast path (see above); NULL: the launch-by-launch schedule */
    float *gathered2;
} spex_partitioned_dual_step_t;
int spex_partitioned_dual_task_step_f32(spex_partitioned_dual_step_t *step, const int64_t *pos, const float *labels, int32_t B,
                                        const int64_t *seq, const int64_t *seq_l, const int64_t *targets, int32_t T, void *stream);

/* ------------------------------------------------------------------------------------------------ profiling hook
 * Not part of any reference interface: lets a caller time the dominant kernel itself, in place, on the stream it is
 * launched on (bench.py's roofline figure).  While a timer is attached to a graph, every (or every n-th) call of
 * spex_spmm_f32 / spex_propagate_f32 / spex_propagate_bwd_f32 on it is bracketed by ONE hipEvent pair around all the
 * main SpMM launches of that call (a 3-layer propagation = one bracket of three back-to-back launches), until
 * `capacity` brackets are used.  spex_timer_read synchronises on the recorded events and returns, per bracket, the
 * elapsed milliseconds and the number of SpMM launches inside it.
 */
typedef struct spex_timer spex_timer_t;
int spex_timer_create(int32_t capacity, int32_t every /* bracket every n-th call */, spex_timer_t **out);
int spex_timer_destroy(spex_timer_t *t);
int spex_timer_attach(spex_graph_t *g, spex_timer_t *t /* NULL detaches */);
int spex_timer_read(spex_timer_t *t, float *h_ms, int32_t *h_launches, int32_t max_count, int32_t *count, int reset);

#ifdef __cplusplus
}
#endif
#endif /* SPEX_HIP_H */
