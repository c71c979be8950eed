// Internal helpers shared by the libspexhip.so translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/spex_hip.h"

namespace spex {

void set_error(const char *fmt, ...);
struct SmallAdam {          // a second, small parameter block updated by the same Adam launch; gradient = sum of n_parts partial blocks
    float *p = nullptr, *m = nullptr, *v = nullptr;
    const float *parts = nullptr;
    int32_t n_parts = 0;
    int64_t stride = 0;
    int32_t n = 0;
};
struct L2Rows {             // the exact BPR step's L2 term, applied by its Adam launch: gradient += scale * count[row] * p[row]
    const int32_t *count = nullptr;   // occurrences of every table row in this step's batch (written by the batch kernel)
    int32_t *clear = nullptr;         // the OTHER step parity's count table, cleared here (no thread clears a cell another still reads)
    float scale = 0.0f;               // weight_decay / T
    float *g_store = nullptr;         // receives the step's whole gradient (product + add_g share + L2 term); may be g itself
    int32_t shift = 4;                // log2 of a row's float4 count: 4 / 5 / 6 for rows of 64 / 128 / 256
};
int adam_step_z2(float *p, const float *g, float *m, float *v, int64_t n, int32_t t, float lr, float beta1, float beta2, float eps,
                 float *zero_buf, float *zero_buf2, void *stream, const float *loss_rows = nullptr, int32_t n_loss = 0,
                 float *loss_sum = nullptr, const SmallAdam *small = nullptr, const float *add_g = nullptr, float add_div = 1.0f,
                 const L2Rows *l2 = nullptr, uint16_t *p16 = nullptr);
                                               // add_g: gradient = g + add_g / add_div (add_g may be zero_buf: read, then cleared);   // optim.hip: spex_adam_step_f32 with a second buffer to clear and the step's
                                               // per-sample losses to fold into an accumulator
                                               // p16: also receives bf16(the updated p), round to nearest even, from the same register —
                                               // the bf16 gather table of the next step; 8-byte aligned, n % 4 == 0

struct AdamRowList {            // the rows of a row-sparse Adam pass and its side jobs by list position (optim.hip: adam_rows_kernel)
    const int32_t *list = nullptr;    // rows list[k], k < min(*count, max_count), distinct; values outside [0, n_rows) are skipped
    const int32_t *count = nullptr;   // device cell
    int32_t max_count = 0, n_rows = 0;
    const int32_t *count_b = nullptr; // device cell: positions below it read, add and clear add_g's row and carry the L2 count
    float *add_g = nullptr;           // gradient += add_g / add_div at those positions (NULL: no such term)
    float add_div = 1.0f;
    const int32_t *count_z = nullptr; // device cell: positions below it clear zero_buf's row
    float *zero_buf = nullptr;
};
int adam_rows(float *p, const float *g, float *m, float *v, const AdamRowList &rl, int32_t t, float lr, float beta1, float beta2, float eps,
              void *stream, const float *loss_rows = nullptr, int32_t n_loss = 0, float *loss_sum = nullptr,
              const L2Rows *l2 = nullptr, const int32_t *count_a = nullptr);
                                              // optim.hip: spex_adam_rows_f32 with the one-call steps' side jobs (d == 64); count_a: a device
                                              // cell for the add term's range where it is not count_b's (the deep step: P lives in F1)

int dual_task_adam(float *p, float *m, float *v, const float *g_E0, float *g_raw, float *g_user, float *g_small, float *g_prop,
                   float *push_zero, float *loss, float *loss_acc, float *prec, int64_t n_table, int64_t n_user, int64_t n_trust,
                   int32_t B, int32_t T, int32_t n_rec, int32_t t, float lr, float beta1, float beta2, float eps, int fixed_weights,
                   void *stream, float prop_div = 0.0f, float *att_copies = nullptr, int32_t n_att_copies = 0,
                   int32_t att_clear = 0, int32_t part = 0, int32_t clear_prop = 1, float *zero_a = nullptr, int64_t n_zero_a = 0,
                   float *zero_b = nullptr, int64_t n_zero_b = 0);           // optim.hip: Adam over the dual-task parameter arena (spex_dual_task_step_f32)

// trust.hip: spex_trust_head_train_f32 with a cap on the fused kernel's workgroups per path (the public entry: 8; beside other work: 1)
int trust_head_train(const float *table, int64_t n_rows, const float *params, const int64_t *seq, const int64_t *seq_l,
                     const int64_t *targets, int32_t B, int32_t L, int32_t d, int32_t n_heads, int32_t hybrid, float scale,
                     const float *scale_dev, float *a2, float *dscore, float *loss_b, float *ws, float *loss_out, int32_t loss_accumulate,
                     float *grad_params, float *grad_table, int32_t split_cap, void *stream);

// batch.hip: one launch of the batch-sized middle of an exact LightGCN step, described by value.  The layer sum is
// formed at the batch's rows from up to three tables (acc_in + acc2 + acc3, in that order; NULL = absent) — what lets the one-call
// steps run their forward layers in the plain form.  The ten spex_lightgcn_[bpr_]batch_* exports and steps.hip fill one of these.
struct BatchLaunch {
    enum Widths { kAnyWidth, kNarrow, kWide };     // the narrow / _wide BPR exports promise one width each (their callers' tables)
    const char *who = nullptr;                     // the entry's name for messages; NULL: the export that takes this form
    bool bpr = false;                              // triples (a, b, c) = (user, positive, negative), three rows; else samples (a, b, labels)
    bool push = false;                             // atomics into g_out / G and the push; else per-sample rows into `slots`, no float atomic
    bool x_bf16 = false;                           // X is a bf16 table (rows of 128 bytes, d == 64: batch_bf16.hip), else fp32
    Widths widths = kAnyWidth;
    const spex_graph_t *g = nullptr;
    const void *X = nullptr;                       // the table the last layer gathers from
    const float *acc_in = nullptr, *acc2 = nullptr, *acc3 = nullptr;
    float acc_div = 1.0f;
    const int64_t *a = nullptr, *b = nullptr, *c = nullptr;
    const float *labels = nullptr;
    int32_t n = 0, n_user_rows = 0;                // samples or triples
    float grad_scale = 0.0f, push_scale = 0.0f, weight_decay = 0.0f;
    const float *E0 = nullptr;                     // the L2 term's rows (bpr, weight_decay > 0)
    int32_t *row_counts = nullptr;                 // the L2 gradient's occurrence counts (bpr)
    float *loss_sum = nullptr, *loss_rows = nullptr, *g_out = nullptr, *G = nullptr, *slots = nullptr;
    int32_t d = 0;
    void *stream = nullptr;
};
int batch_launch(const BatchLaunch &L);                                   // batch.hip: checks the descriptor, then launches its kernel
int batch_launch_bf16(const BatchLaunch &L, int parts, int runs_per_part);  // batch_bf16.hip: the launch alone (batch_launch has checked)
int gated_batch_fwd_layers(const spex_graph_t *g, const float *X, const float *acc_in, const float *acc2, const float *acc3, float acc_div,
                           const float *raw, const float *att_u, const float *att_i, const int64_t *users, const int64_t *items,
                           const float *labels, int32_t B, int32_t n_user_rows, float grad_scale, float *loss_sum, float *loss_per_sample,
                           float *lo_batch, float *grad_slots, int32_t d, void *stream);
// (the rec branch's whole batch-sized middle — forward, gate, scores, the gate's backward, push — in one launch: batch.hip)
int gated_batch_push_layers(const spex_graph_t *g, const float *X, const float *acc_in, const float *acc2, const float *acc3, float acc_div,
                            const float *raw, const float *att_u, const float *att_i, const int64_t *users, const int64_t *items,
                            const float *labels, int32_t B, int32_t n_user_rows, float grad_scale, float push_scale, float *loss_sum,
                            float *g_prop, float *G, float *g_raw, float *g_att, int32_t n_att_copies, int32_t d, void *stream);
// (the batch-sized middle of the partitioned one-call steps on the batch's compact replicated rows — [gate,] scores, [the gate's
//  backward,] owner-computes adds, and the first backward product pushed through the rank's own columns of A: batch.hip;
//  rows_raw == NULL: the LightGCN form; push == NULL: a rank without rows)
int rows_train_push(const spex_graph_t *push, const float *rows_raw, const float *rows_prop, const float *att_u, const float *att_i,
                    const int64_t *pos, int64_t lo, int32_t n_local, const float *labels, int32_t B, float grad_scale, float push_scale,
                    float *loss_sum, float *g_prop, float *P, float *g_raw, float *g_att, int32_t n_att_copies, void *stream);
int score_bce_slots_rows(const float *users, const float *items, int32_t ldu, int32_t ldi, int64_t n_user_rows, int64_t n_item_rows,
                         const int64_t *u_idx, const int64_t *i_idx, const float *labels, int32_t B, int32_t d, float *loss_rows,
                         float grad_scale, float *grad_slots, int32_t ld_slots, void *stream);     // score.hip: per-sample rows + losses
int propagate_plain(const spex_graph_t *g, const float *E0, float *sum1, float *ws, int32_t L, int32_t d, void *stream,
                    const float **tables, const int64_t *u = nullptr, const int64_t *i_pos = nullptr, const int64_t *i_neg = nullptr,
                    int64_t T = 0, int32_t n_user_rows = 0, const float **snap = nullptr, const float **last_src = nullptr);
                                              // spmm.hip: L launches, the layer mean left to the consumer (*snap, tables[0..2]: L + 1 addends);
                                              // *last_src != NULL on return: L - 1 launches, the consumer gathers layer L from that table
int bpr_sgd_fused_last(const spex_graph_t *g, const float *Xg, const float *snap, const float *t0, const float *t1, float div,
                       float *table_w, int64_t n_user_rows, int64_t n_item_rows, const int64_t *u, const int64_t *i_pos,
                       const int64_t *i_neg, int64_t T, float lr, float reg, float *loss_sum,
                       void *stream);             // score.hip: bpr_sgd_layers with the last addend (A Xg at the triples' rows) gathered in the launch
int bpr_sgd_layers(const float *snap, const float *t0, const float *t1, const float *t2, float div, float *table_w, int64_t n_user_rows,
                   int64_t n_item_rows, const int64_t *u, const int64_t *i_pos, const int64_t *i_neg, int64_t T, float lr, float reg,
                   float *loss_sum, void *stream);    // score.hip: the fused BPR-SGD kernel reading rows as (((snap +) t0 + t1) + t2) / div
int scale_div(const float *in, float *out, float div, int64_t n, void *stream);                          // spmm.hip: out = in / div
// spmm.hip: what a launch that WRITES the handle's scratch does first (spex_graph::scratch_mu) — takes the lock into `lock` (held until the
// caller's kernels are queued), makes `stream` wait for what the scratch's last user has queued, and records `stream` as that user
int order_scratch(const spex_graph_t *g, hipStream_t stream, std::unique_lock<std::mutex> &lock);
int ensure_partial(spex_graph_t *g, int32_t d);                                                        // spmm.hip: the scratch holds n_seg partial rows of d floats
int unique_rows_more(const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b, int32_t n_rows,
                     int32_t *stamp, int32_t epoch, int32_t *list, int32_t *count, void *stream);             // rows.hip: append to a unique-rows list
int zero_f32(float *x, int64_t n, void *stream);                                                      // rows.hip: x[0 : n] = 0 (a kernel launch)
int sum_ordered(const float *x, int32_t n, float scale, float *out, int accumulate, void *stream);     // rows.hip: fixed-order sum
int sum_parts(const float *parts, int32_t n_parts, int64_t stride, int32_t n, float *out, int accumulate,
              void *stream);                                                                        // rows.hip: partial blocks, in order

#define SPEX_CHECK_ARG(cond, ...)             \
    do {                                      \
        if (!(cond)) {                        \
            ::spex::set_error(__VA_ARGS__);   \
            return SPEX_ERR_INVALID;          \
        }                                     \
    } while (0)

#define SPEX_HIP(call)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            ::spex::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SPEX_ERR_HIP;                                                                \
        }                                                                                       \
    } while (0)

// A/B switch of the one-call BPR step's fused launch (score.hip: bpr_fused_last_kernel), for scratch builds: 0 = the form before.
#ifndef SPEX_FUSED_QUADS
#define SPEX_FUSED_QUADS 1         // a segment's last chunk gathers its real entries only, four at a time (0: 52 VGPRs since the row heads)
#endif

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kWavesPerBlock = 4;  // 256-thread workgroups
constexpr int kLongRow = 128;      // generic kernel / hub path: rows with more stored entries are cut into segments
constexpr int kSegLen = 64;        // entries per such segment (partial rows go through global scratch + the fix-up launch); 64 = one
                                   // wave task of the d == 64 kernel: a hub segment of 128 made its wave run twice as long as every other
                                   // wave of a one-round launch, i.e. set the launch time (Weibo-shaped graph: 19.8 us per product)
constexpr int kTaskEntries = 64;   // entries per wave task of the d == 64 kernel (4 chunks: 4 memory round trips)
constexpr int kWgWaves = 16;       // the d == 64 kernel runs 1024-thread workgroups = 16 wave tasks
constexpr int kWgRowMax = kWgWaves * kTaskEntries;  // longest row whose segments are combined inside one workgroup
constexpr int kOpenTasks = 4;      // first-fit packing of short rows keeps this many tasks open
constexpr int kChunk = 16;         // entries per chunk = gathers a wave keeps in flight
constexpr int kRowHead = kChunk;   // entries per row of the row-head table (spex_graph::head_col): one chunk.  (A whole wave task, 64,
                                   // was built and measured too: slower, four times the bytes — DESIGN 5)
constexpr int kTileRows = 64;      // rows a workgroup completes in tile mode (4 MFMA tiles of 16)
constexpr int kSoftmaxTile = 2048; // stored entries per workgroup of the row-softmax kernels (512 on small graphs)

}  // namespace spex

// Cross-lane sums on the vector ALU's DPP path.  `__shfl_xor` compiles to ds_bpermute_b32 — an LDS-pipe instruction, one
// pipe per CU shared by four SIMDs — and a 64-lane butterfly is six of them per value: the scoring kernels' dot
// products were bound by that pipe, not by their gathers (2 M dot products of a 2^20-triple BPR batch: 184 us with the
// gathers removed).  These use DPP row shifts / broadcasts instead (no LDS traffic).
namespace spex {
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
__device__ __forceinline__ float dpp_f32(float v)   // source lane per CTRL; lanes without a valid source read 0
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, BANK_MASK, true));
}

// Sum over the 64 lanes, returned to every lane (the value is wave-uniform: it comes back through an SGPR).
__device__ __forceinline__ float wave_sum_f32(float v)
{
    v += dpp_f32<0xb1>(v);          // quad_perm [1,0,3,2]
    v += dpp_f32<0x4e>(v);          // quad_perm [2,3,0,1]   every lane: its quad's sum
    v += dpp_f32<0x114>(v);         // row_shr:4
    v += dpp_f32<0x118>(v);         // row_shr:8             lane 15 of each row: the row's sum
    v += dpp_f32<0x142, 0xa>(v);    // row_bcast:15 into rows 1 and 3
    v += dpp_f32<0x143, 0xc>(v);    // row_bcast:31 into rows 2 and 3: lane 63 holds the total
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Sum over each row of 16 lanes, returned to every lane of the row (rotations within the row).
__device__ __forceinline__ float row16_sum_f32(float v)
{
    v += dpp_f32<0x128>(v);         // row_ror:8
    v += dpp_f32<0x124>(v);         // row_ror:4
    v += dpp_f32<0x122>(v);         // row_ror:2
    v += dpp_f32<0x121>(v);         // row_ror:1
    return v;
}

// Lane src's value to every lane, through an SGPR (src is wave-uniform).
__device__ __forceinline__ float lane_bcast(float v, int src)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// fp32 -> bf16, round to nearest even; NaN stays NaN (quiet), +-0 and +-Inf are preserved, the largest finite fp32 rounds to Inf.
// The library's one rounding: spex_cast_bf16_f32, the Y16 outputs, the Adam launch's shadow table.
__device__ __forceinline__ uint16_t bf16_rne(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// bf16 -> fp32 is exact: the 16 bits become the high half of the word.  Two gathered entries share a register (low / high half):
// widening is a shift or a mask.
typedef unsigned short h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float widen_pair(h2 p, int hi)
{
    const uint32_t w = __builtin_bit_cast(uint32_t, p);
    return __uint_as_float(hi ? (w & 0xFFFF0000u) : (w << 16));
}
}  // namespace spex

namespace spex {
// philox4x32-10, counter = (edge_id, 0, 0, 0), key = seed.  Returns the first output word.
__device__ __forceinline__ uint32_t philox_first(uint32_t ctr0, uint32_t k0, uint32_t k1)
{
    uint32_t c0 = ctr0, c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// Edge dropout (model.py:46-55) as the kernels see it: mode 1 = a device keep mask indexed by edge id, mode 2 = the counter-based
// draw keyed by the edge id; a kept value is divided by keep_prob, a dropped entry contributes nothing.
struct EdgeDrop {
    const uint8_t *keep;
    const int32_t *edge_id;      // entry -> edge id (NULL: the entry index itself)
    int mode;
    float keep_prob;
    uint32_t seed_lo, seed_hi;
};
__device__ __forceinline__ bool edge_kept(const EdgeDrop &dr, int entry)
{
    const uint32_t eid = (uint32_t)(dr.edge_id ? dr.edge_id[entry] : entry);
    if (dr.mode == 1) return dr.keep[eid] != 0;
    const float u01 = (float)(philox_first(eid, dr.seed_lo, dr.seed_hi) >> 8) * 5.9604644775390625e-8f;
    return (u01 + dr.keep_prob) >= 1.0f;
}
}  // namespace spex

// Wide embeddings on the batch-sized kernels (d = 64 V, V = 2 / 4; batch.hip, the row-list kernel of spmm.hip): a lane owns V
// CONSECUTIVE columns, so a gathered row is one coalesced 256 V-byte wave load (dwordx2 / dwordx4 per lane), as in
// spmm_chunk_wide_kernel.  Tables must be 16-byte aligned (any row of a contiguous fp32 [*, 64 V] tensor is).
namespace spex {
template <int V>
struct WideVec {
    typedef float T __attribute__((ext_vector_type(V)));
};

// One 64-entry segment [e0, e0 + cnt) of a row at width 64 V — segment_sum<MASKED> of batch_kernels.h with V columns per
// lane.  The d == 64 form keeps the segment's 64 gathered floats in registers; at the same 64 result registers a wave here keeps
// 64 / V gathers in flight (32 rows of 512 B, 16 rows of 1 KB: 16 KB per wave at every width) and walks the segment in V passes —
// the kernels run 1 024-thread workgroups, i.e. 4 waves per SIMD and at most 128 VGPRs.  Every column's fmaf chain runs in entry
// order, a dropped entry (MASKED: the handle's edge-dropout rule) contributes fmaf(0, 0, acc) = acc at its place in the chain:
// the sums are spmm_chunk_wide_kernel's, bit for bit.  Xl = X + lane * V.
template <int V, bool MASKED>
__device__ __forceinline__ typename WideVec<V>::T segment_sum_wide(const int32_t *__restrict__ col, const float *__restrict__ val,
                                                                   const float *__restrict__ Xl, int e0, int cnt, int lane,
                                                                   typename WideVec<V>::T acc, const EdgeDrop &dr)
{
    typedef typename WideVec<V>::T vec;
    constexpr int kRow = kWave * V, kFly = kTaskEntries / V;
    int my_col = 0;
    float my_val = 0.0f;
    bool dropped = false;
    if (lane < cnt) {
        my_col = col[e0 + lane];
        my_val = val[e0 + lane];
        if (MASKED) {
            const bool kept = edge_kept(dr, e0 + lane);
            my_val = kept ? my_val / dr.keep_prob : 0.0f;
            dropped = !kept;
        }
    }
    const unsigned long long dbits = MASKED ? __ballot(dropped) : 0ull;
    const int last_col = __builtin_amdgcn_readlane(my_col, (cnt - 1) & 63);
    if (lane >= cnt) my_col = last_col;                    // padding: value 0 on a row already being fetched
#pragma unroll
    for (int p = 0; p < V; ++p) {
        if (p * kFly < cnt) {
            vec x[kFly];
#pragma unroll
            for (int k = 0; k < kFly; ++k)
                x[k] = *reinterpret_cast<const vec *>(Xl + (size_t)(uint32_t)__builtin_amdgcn_readlane(my_col, p * kFly + k) * kRow);
#pragma unroll
            for (int k = 0; k < kFly; ++k) {
                const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val), p * kFly + k));
                const bool gone = MASKED && ((dbits >> (p * kFly + k)) & 1ull);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = fmaf(a, gone ? 0.0f : x[k][j], acc[j]);
            }
        }
    }
    return acc;
}
}  // namespace spex

// A batch as two device index lists with offsets (users; items + n_user_rows): slot k's row.
namespace spex {
__device__ __forceinline__ long long batch_row(const int64_t *idx_a, int n_a, int64_t off_a, const int64_t *idx_b, int64_t off_b,
                                               int k)
{
    return k < n_a ? idx_a[k] + off_a : idx_b[k - n_a] + off_b;
}

}  // namespace spex

struct spex_timer {
    std::vector<hipEvent_t> start, stop;
    int32_t used = 0;
    std::vector<int32_t> launches;  // main-kernel launches inside each bracket
    int32_t every = 1;   // bracket every `every`-th API call (spmm / propagate / propagate_bwd)
    int64_t seen = 0;    // API calls seen since the last reset
    bool open = false;   // a bracket is open (launch_spmm counts its launches instead of bracketing them itself)
};

// The opaque handle.  All pointers are device memory owned by the handle.
struct spex_graph {
    int32_t n_rows = 0, n_cols = 0;
    int64_t nnz = 0;
    int32_t *rowptr = nullptr;   // [n_rows+1]
    int32_t *col = nullptr;      // [nnz]
    float *val = nullptr;        // [nnz]
    int32_t *edge_id = nullptr;  // [nnz] or null (identity)
    int64_t max_edge_id = -1;    // largest edge id (nnz - 1 for identity)
    int32_t *row_of = nullptr;   // [nnz] row of each stored entry, built by the first spex_sddmm_f32
    int32_t tile = 0;            // stored entries per row-softmax workgroup: kSoftmaxTile, or 512 when that fills < 2 k workgroups
    int32_t n_tiles = 0;         // ceil(nnz / tile)
    int32_t *tile_row = nullptr; // [n_tiles+1] first row starting at or after entry t * tile
    // long rows (> kLongRow entries): segment table + per-segment partial rows + per-row fix-up table
    int32_t n_long = 0, n_seg = 0;
    int32_t *seg_beg = nullptr;   // [n_seg] first entry of the segment
    int32_t *seg_end = nullptr;   // [n_seg]
    int32_t *long_row = nullptr;  // [n_long] row index
    int32_t *long_seg0 = nullptr; // [n_long+1] first segment of each long row
    float *partial = nullptr;     // [n_seg * d_cap] scratch, grown on demand
    int64_t partial_cap = 0;      // floats
    float *snap = nullptr;        // [snap_cap] scratch of the one-call BPR step: the E^0 rows of its triples (spmm.hip: SnapArgs), grown on demand
    int64_t snap_cap = 0;         // floats
    unsigned long long *loss_cell = nullptr;   // [loss_cell_cap] loss cells of the one-call BPR step's fused launch (score.hip: group_loss_add), zero between launches
    int64_t loss_cell_cap = 0;
    // The scratch is the one piece of a handle that launches WRITE.  Calls on one stream are ordered by the stream; a call
    // on another stream first waits (event) for everything queued on the stream that used the scratch last — so two streams
    // may share a handle, and so may two HOST threads: a launch that writes the scratch holds scratch_mu from the ordering
    // decision until its kernels are queued (otherwise the other thread's event could be recorded in front of them).
    std::mutex scratch_mu;
    hipStream_t scratch_stream = nullptr;
    bool scratch_used = false;
    hipEvent_t scratch_ev = nullptr;
    // Chunked copy of the matrix for the d == 64 kernel (built when n_cols * 256 B fits a 32-bit buffer offset).
    // A chunk is 16 stored entries: byte offsets of their source rows (col * 256), their values, and a 16-bit mask
    // marking entries that end an output row.  A wave TASK is a run of <= 4 chunks (64 entries): whole consecutive
    // short rows, or one 64-entry segment of a row with 65..1024 entries — all segments of such a row sit in ONE
    // 16-wave workgroup and are summed through LDS in segment order — or (rows > 1024 entries only) a 128-entry
    // segment whose partial row goes through global scratch and the fix-up launch.  Tasks are padded to whole chunks
    // with value-0 entries on the task's last real source row (a line already being fetched); a chunk's padding sits at
    // its end (count in chunk_pad).
    //   task.x = first chunk, .y = number of chunks, .z = (first) row or -1, .w = kind | flags (see graph.hip)
    int32_t n_tasks = 0;
    int4 *task = nullptr;          // [n_tasks], heaviest first
    int64_t n_chunks = 0;
    uint32_t *chunk_off = nullptr; // [n_chunks * 16]
    float *chunk_val = nullptr;    // [n_chunks * 16]
    uint32_t *chunk_mask = nullptr; // [n_chunks] end-of-row flags (16 bits)
    uint8_t *chunk_pad = nullptr;   // [n_chunks] number of padding entries at the end of the chunk
    uint32_t *chunk_eid = nullptr;  // [n_chunks * 16] edge id of each entry (keep-mask index); read only under dropout
    bool row_ids = false;           // tasks pack non-adjacent rows (cache-resident graphs): every entry carries its output row
    int32_t *chunk_row = nullptr;   // [n_chunks * 16] output row of each entry, only when row_ids && !packed_words
    // Packed words (bin-packed tables of at most 65 536 rows — their columns are at most 65 536 anyway — whose packs hold 64
    // entries, i.e. chunk_stride <= 4, unless SPEX_PACK_WORDS=0, read at creation): chunk_off holds (output row << 16) | source row
    // and there is NO chunk_row array — 8 bytes of metadata per entry instead of 12, one vector load per task less.  The chunk
    // kernels tell the layouts apart by the null chunk_row, once per wave, and split the word once per lane; a padding slot's row
    // half is never read.  chunk_body splits in a task's FIRST super-chunk only: a packed handle has no task beyond four chunks
    // (max_task_chunks, checked by the packer and again by every d == 64 launch).
    bool packed_words = false;
    int32_t max_task_chunks = 0;    // the largest task.y of the table (kind-3 row lists, which run no chunk, not counted)
    // Implied positions (bin-packed tables, unless SPEX_PACK_IMPLIED=0): task k's chunks start at chunk k * chunk_stride
    // (chunk_stride = the pack capacity in chunks: 4, or 5 / 6 where the packer raised it), so the d == 64 kernel requests a wave's
    // first 64 entries of metadata together with its task record; task.x is still stored (= k * chunk_stride) and the slots no task
    // fills are padding (column 0, value 0, edge 0, chunk_pad = kChunk).  0: the dense layout (tables that stream from HBM).
    int32_t chunk_stride = 0;
    // Row heads (bin-packed tables without hub rows, unless SPEX_ROW_HEADS=0): a second, fixed-stride copy of every row's first
    // min(deg, kRowHead) entries in CSR order, the tail padded with column 0 / value 0 — row r's first entries sit at r * kRowHead,
    // a position the row id alone implies, so the fused BPR launch (score.hip) requests them in the same round trip as rowptr[r]
    // instead of one trip behind it.  Static like the chunk table; spex_graph_set_values rewrites head_val with val.  NULL: no heads
    // (tables that stream from HBM, graphs with hub rows) — every reader tests for that and walks the CSR arrays.
    int32_t *head_col = nullptr;    // [n_rows * kRowHead]
    float *head_val = nullptr;      // [n_rows * kRowHead]
    // Tile mode (spex_graph_create_ex, SPEX_GRAPH_TILE_ROWS): every workgroup of the task table completes at most kTileRows rows,
    // task.w bits 16-23 = the workgroup-local slot of the task's first completed row — what the fused NGCF layer kernel needs
    // to hold a workgroup's rows in LDS.  0 = ordinary table.
    int32_t tile_rows = 0;
    int32_t n_wgs = 0;              // workgroups of the task table (tile mode)
    int32_t *wg_rows = nullptr;     // [n_wgs] rows each workgroup completes (tile mode)
    int32_t n_hub = 0;              // rows longer than kWgRowMax (global-scratch path of the d == 64 kernel)
    int32_t *hub_row = nullptr;     // [n_hub]
    int32_t *hub_seg0 = nullptr;    // [2 * n_hub] (first, one-past-last) segment of each hub in the kLongRow segment table
    // In-kernel fold of the hubs (d == 64 chunk kernel): the hub segments lead the task table, so 16 consecutive segments of a
    // hub share a workgroup — a GROUP, summed through LDS by its first wave, which publishes one partial row and takes a ticket
    // on the hub; the hub's last group to arrive folds the groups' partials in group order and runs the epilogue.
    int32_t n_hub_tasks = 0;        // hub segment tasks = task[0 : n_hub_tasks]
    int4 *hub_grp = nullptr;        // [n_hub_tasks] x: 1 = the group's first wave, y: waves in the group, z: the group's partial row, w: hub
    int2 *hub_fold = nullptr;       // [n_hub] x: the hub's first partial row, y: its number of groups
    unsigned long long *hub_ticket = nullptr;   // [n_hub] arrival counter: every folding launch adds the hub's group count (zeroed at creation, never reset)
    // edge dropout
    int mask_mode = 0;
    const uint8_t *keep = nullptr;
    float keep_prob = 1.0f;
    uint64_t seed = 0;
    spex_timer *timer = nullptr;  // profiling hook (not owned)
};

namespace spex {
inline EdgeDrop edge_drop_of(const spex_graph_t *g)      // the handle's edge-dropout state as the kernels take it
{
    return EdgeDrop{g->keep, g->edge_id, g->mask_mode, g->keep_prob, (uint32_t)g->seed, (uint32_t)(g->seed >> 32)};
}
}  // namespace spex
