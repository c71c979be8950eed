// The batch-sized middles of the exact LightGCN steps (batch.hip) with a bf16 gather source, d == 64.
//
// The last layer at the batch's rows gathers from X16 = bf16(y_{L-1}) — the table the whole-graph launch before it wrote beside its
// fp32 output (spex_spmm_bf16_f32: Y16) — in rows of 128 bytes.  Widening is exact, and everything behind the gather is the fp32
// kernel's statement (batch_kernels.h holds the one body both instantiate): the layer sum from the fp32 tables, scores, loss,
// gradient rows, L2 counts, and the push into fp32 slots.  On Xw = float(X16) a launch returns what its fp32 sibling returns on Xw;
// a row of at most 1 024 entries is spex_spmm_bf16_f32's row bit for bit, under either edge-dropout mode too.
// A segment's 64 gathers sit in 32 registers (two entries per register); the freed registers are left to the compiler.
#include "batch_kernels.h"

using namespace spex;
using namespace spex::batchk;

namespace {

template <bool PUSH>
__global__ __launch_bounds__(kWave *kWgWaves) void lightgcn_batch_bf16_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows,
    int n_user_rows, const uint16_t *__restrict__ X16, const float *__restrict__ acc_in, float acc_div,
    const int64_t *__restrict__ users, const int64_t *__restrict__ items, const float *__restrict__ labels, int parts,
    float grad_scale, float push_scale, float *loss_sum, float *__restrict__ loss_rows, float *g_out, float *G, int runs_per_part,
    float *__restrict__ grad_slots, int B, const float *__restrict__ acc2, const float *__restrict__ acc3, const spex::EdgeDrop drop)
{
    lightgcn_batch_body<PUSH>(rowptr, col, val, n_rows, n_user_rows, X16, acc_in, acc_div, users, items, labels, parts, grad_scale, push_scale,
                              loss_sum, loss_rows, g_out, G, runs_per_part, grad_slots, B, acc2, acc3, drop);
}

template <bool PUSH>
__global__ __launch_bounds__(kWave *kWgWaves) void lightgcn_bpr_batch_bf16_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows, int n_user_rows,
    const uint16_t *__restrict__ X16, const float *__restrict__ acc_in, float acc_div, const int64_t *__restrict__ users,
    const int64_t *__restrict__ pos, const int64_t *__restrict__ neg, int parts, float grad_scale, float push_scale, float *loss_sum,
    float *__restrict__ loss_rows, float *g_out, float *G, int runs_per_part, float *__restrict__ grad_slots, int T,
    const float *__restrict__ acc2, const float *__restrict__ acc3, float weight_decay, const float *__restrict__ E0,
    int32_t *row_counts, const spex::EdgeDrop drop)
{
    lightgcn_bpr_batch_body<PUSH>(rowptr, col, val, n_rows, n_user_rows, X16, acc_in, acc_div, users, pos, neg, parts, grad_scale, push_scale,
                                  loss_sum, loss_rows, g_out, G, runs_per_part, grad_slots, T, acc2, acc3, weight_decay, E0, row_counts, drop);
}

spex::EdgeDrop edge_drop_of(const spex_graph_t *g)
{
    return spex::EdgeDrop{g->keep, g->edge_id, g->mask_mode, g->keep_prob, (uint32_t)g->seed, (uint32_t)(g->seed >> 32)};
}

// What the four entries check alike.  (The kernels walk the handle's CSR arrays, not its chunk tables: any handle will do.)
int check_common(const char *who, const spex_graph_t *g, const uint16_t *X16, const float *acc_in, const float *acc2, const float *acc3,
                 float acc_div, int32_t n, int32_t n_user_rows, int32_t d)
{
    if (d != kWave) {
        spex::set_error("%s: bf16 gather tables are built for d == 64 only (d = %d): use the fp32 entries", who, d);
        return SPEX_ERR_UNSUPPORTED;
    }
    SPEX_CHECK_ARG(g && X16 && acc_in && n >= 0 && acc_div != 0.0f && (!acc3 || acc2), "%s: NULL argument, a negative count, acc_div == 0 or acc3 without acc2", who);
    SPEX_CHECK_ARG(n_user_rows >= 0 && n_user_rows <= g->n_rows && g->n_rows == g->n_cols, "%s: n_user_rows=%d on a %d x %d graph", who,
                   n_user_rows, g->n_rows, g->n_cols);
    SPEX_CHECK_ARG((((uintptr_t)X16) & 1) == 0 && (const void *)X16 != (const void *)acc_in, "%s: X16 misaligned or aliasing acc_in", who);
    return SPEX_OK;
}

}  // namespace

int spex::lightgcn_batch_slots_bf16_layers(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, const float *acc2,
                                           const float *acc3, float acc_div, const int64_t *users, const int64_t *items,
                                           const float *labels, int32_t B, int32_t n_user_rows, float grad_scale, float *loss_sum,
                                           float *loss_per_sample, float *grad_slots, int32_t d, void *stream)
{
    const char *who = "spex_lightgcn_batch_slots_bf16_f32";
    int rc = check_common(who, g, X16, acc_in, acc2, acc3, acc_div, B, n_user_rows, d);
    if (rc != SPEX_OK) return rc;
    SPEX_CHECK_ARG((B == 0 || (users && items && labels)) && (loss_sum || loss_per_sample) && grad_slots, "%s: NULL argument", who);
    if (B == 0 || g->n_rows == 0) return SPEX_OK;
    hipLaunchKernelGGL(lightgcn_batch_bf16_kernel<false>, dim3((unsigned)B), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col,
                       g->val, g->n_rows, n_user_rows, X16, acc_in, acc_div, users, items, labels, 1, grad_scale, 0.0f, loss_sum,
                       loss_per_sample, nullptr, nullptr, 1, grad_slots, B, acc2, acc3, edge_drop_of(g));
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

int spex::lightgcn_batch_bf16_layers(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, const float *acc2, const float *acc3,
                                     float acc_div, const int64_t *users, const int64_t *items, const float *labels, int32_t B,
                                     int32_t n_user_rows, float grad_scale, float push_scale, float *loss_sum, float *loss_per_sample,
                                     float *g_out, float *G, int32_t d, void *stream)
{
    const char *who = "spex_lightgcn_batch_bf16_f32";
    int rc = check_common(who, g, X16, acc_in, acc2, acc3, acc_div, B, n_user_rows, d);
    if (rc != SPEX_OK) return rc;
    SPEX_CHECK_ARG((B == 0 || (users && items && labels)) && (loss_sum || loss_per_sample) && G && G != g_out, "%s: NULL argument (or G == g_out)", who);
    if (B == 0 || g->n_rows == 0) return SPEX_OK;
    constexpr int runs_per_part = kBatchRunsPerPart, parts = kBatchParts;
    SPEX_CHECK_ARG((int64_t)B * parts < (int64_t)1 << 31, "%s: B=%d is too many samples for one launch", who, B);
    hipLaunchKernelGGL(lightgcn_batch_bf16_kernel<true>, dim3((unsigned)B * parts), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr,
                       g->col, g->val, g->n_rows, n_user_rows, X16, acc_in, acc_div, users, items, labels, parts, grad_scale, push_scale,
                       loss_sum, loss_per_sample, g_out, G, runs_per_part, nullptr, B, acc2, acc3, edge_drop_of(g));
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

int spex::lightgcn_bpr_batch_slots_bf16_layers(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, const float *acc2,
                                               const float *acc3, float acc_div, const int64_t *users, const int64_t *pos,
                                               const int64_t *neg, int32_t T, int32_t n_user_rows, float grad_scale, float weight_decay,
                                               const float *E0, int32_t *row_counts, float *loss_sum, float *loss_per_sample,
                                               float *grad_slots, int32_t d, void *stream)
{
    const char *who = "spex_lightgcn_bpr_batch_slots_bf16_f32";
    int rc = check_common(who, g, X16, acc_in, acc2, acc3, acc_div, T, n_user_rows, d);
    if (rc != SPEX_OK) return rc;
    SPEX_CHECK_ARG((T == 0 || (users && pos && neg)) && (loss_sum || loss_per_sample) && grad_slots, "%s: NULL argument", who);
    SPEX_CHECK_ARG(weight_decay >= 0.0f && (weight_decay == 0.0f || E0), "%s: weight_decay %g needs E0 (and must not be negative)", who,
                   (double)weight_decay);
    if (T == 0 || g->n_rows == 0) return SPEX_OK;
    hipLaunchKernelGGL(lightgcn_bpr_batch_bf16_kernel<false>, dim3((unsigned)T), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr,
                       g->col, g->val, g->n_rows, n_user_rows, X16, acc_in, acc_div, users, pos, neg, 1, grad_scale, 0.0f, loss_sum,
                       loss_per_sample, nullptr, nullptr, 1, grad_slots, T, acc2, acc3, weight_decay, E0, row_counts, edge_drop_of(g));
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

int spex::lightgcn_bpr_batch_bf16_layers(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, const float *acc2,
                                         const float *acc3, float acc_div, const int64_t *users, const int64_t *pos, const int64_t *neg,
                                         int32_t T, int32_t n_user_rows, float grad_scale, float push_scale, float weight_decay,
                                         const float *E0, int32_t *row_counts, float *loss_sum, float *loss_per_sample, float *g_out,
                                         float *G, int32_t d, void *stream)
{
    const char *who = "spex_lightgcn_bpr_batch_bf16_f32";
    int rc = check_common(who, g, X16, acc_in, acc2, acc3, acc_div, T, n_user_rows, d);
    if (rc != SPEX_OK) return rc;
    SPEX_CHECK_ARG((T == 0 || (users && pos && neg)) && (loss_sum || loss_per_sample) && (G || g_out) && G != g_out,
                   "%s: needs loss_sum or loss_per_sample, G and / or g_out (two tables)", who);
    SPEX_CHECK_ARG(weight_decay >= 0.0f && (weight_decay == 0.0f || E0), "%s: weight_decay %g needs E0 (and must not be negative)", who,
                   (double)weight_decay);
    if (T == 0 || g->n_rows == 0) return SPEX_OK;
    const int parts = G ? kBprBatchParts : 1, runs_per_part = kBprBatchRunsPerPart;     // (no push: one workgroup per triple)
    SPEX_CHECK_ARG((int64_t)T * parts < (int64_t)1 << 31, "%s: T=%d is too many triples for one launch", who, T);
    hipLaunchKernelGGL(lightgcn_bpr_batch_bf16_kernel<true>, dim3((unsigned)T * parts), dim3(kWave * kWgWaves), 0, (hipStream_t)stream,
                       g->rowptr, g->col, g->val, g->n_rows, n_user_rows, X16, acc_in, acc_div, users, pos, neg, parts, grad_scale, push_scale,
                       loss_sum, loss_per_sample, g_out, G, runs_per_part, nullptr, T, acc2, acc3, weight_decay, E0, row_counts,
                       edge_drop_of(g));
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_lightgcn_batch_slots_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                                  const int64_t *users, const int64_t *items, const float *labels, int32_t B,
                                                  int32_t n_user_rows, float grad_scale, float *loss_sum, float *loss_per_sample,
                                                  float *grad_slots, int32_t d, void *stream)
{
    return spex::lightgcn_batch_slots_bf16_layers(g, X16, acc_in, nullptr, nullptr, acc_div, users, items, labels, B, n_user_rows, grad_scale,
                                                  loss_sum, loss_per_sample, grad_slots, d, stream);
}

extern "C" int spex_lightgcn_batch_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                            const int64_t *users, const int64_t *items, const float *labels, int32_t B, int32_t n_user_rows,
                                            float grad_scale, float push_scale, float *loss_sum, float *loss_per_sample, float *g_out,
                                            float *G, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g_out, "spex_lightgcn_batch_bf16_f32: NULL g_out");
    return spex::lightgcn_batch_bf16_layers(g, X16, acc_in, nullptr, nullptr, acc_div, users, items, labels, B, n_user_rows, grad_scale,
                                            push_scale, loss_sum, loss_per_sample, g_out, G, d, stream);
}

extern "C" int spex_lightgcn_bpr_batch_slots_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                                      const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T,
                                                      int32_t n_user_rows, float grad_scale, float weight_decay, const float *E0,
                                                      int32_t *row_counts, float *loss_sum, float *loss_per_sample, float *grad_slots,
                                                      int32_t d, void *stream)
{
    return spex::lightgcn_bpr_batch_slots_bf16_layers(g, X16, acc_in, nullptr, nullptr, acc_div, users, pos, neg, T, n_user_rows, grad_scale,
                                                      weight_decay, E0, row_counts, loss_sum, loss_per_sample, grad_slots, d, stream);
}

extern "C" int spex_lightgcn_bpr_batch_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                                const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows,
                                                float grad_scale, float push_scale, float weight_decay, const float *E0, int32_t *row_counts,
                                                float *loss_sum, float *loss_per_sample, float *g_out, float *G, int32_t d, void *stream)
{
    return spex::lightgcn_bpr_batch_bf16_layers(g, X16, acc_in, nullptr, nullptr, acc_div, users, pos, neg, T, n_user_rows, grad_scale,
                                                push_scale, weight_decay, E0, row_counts, loss_sum, loss_per_sample, g_out, G, d, stream);
}
