// The batch-sized middles of the exact LightGCN steps (batch.hip) with a bf16 gather source, d == 64.
//
// The last layer at the batch's rows gathers from X16 = bf16(y_{L-1}) — the table the whole-graph launch before it wrote beside its
// fp32 output (spex_spmm_bf16_f32: Y16) — in rows of 128 bytes.  Widening is exact, and everything behind the gather is the fp32
// kernel's statement (batch_kernels.h holds the one body both instantiate): the layer sum from the fp32 tables, scores, loss,
// gradient rows, L2 counts, and the push into fp32 slots.  On Xw = float(X16) a launch returns what its fp32 sibling returns on Xw;
// a row of at most 1 024 entries is spex_spmm_bf16_f32's row bit for bit, under either edge-dropout mode too.
// A segment's 64 gathers sit in 32 registers (two entries per register); the freed registers are left to the compiler.
// This file holds the four kernels and their launch; the checks and the four exports are batch.hip's (spex::batch_launch).
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

}  // namespace

// The launch alone: spex::batch_launch (batch.hip) has checked the descriptor and picked the grid.
int spex::batch_launch_bf16(const BatchLaunch &L, int parts, int runs_per_part)
{
    if (!L.bpr) {
        if (L.push) launch_two_rows<uint16_t>(lightgcn_batch_bf16_kernel<true>, L, parts, runs_per_part);
        else launch_two_rows<uint16_t>(lightgcn_batch_bf16_kernel<false>, L, parts, runs_per_part);
    } else {
        if (L.push) launch_three_rows<uint16_t>(lightgcn_bpr_batch_bf16_kernel<true>, L, parts, runs_per_part);
        else launch_three_rows<uint16_t>(lightgcn_bpr_batch_bf16_kernel<false>, L, parts, runs_per_part);
    }
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}
