// The batch-sized middle of the exact LightGCN training step as ONE launch.
//
// Between the dense forward layers and the dense backward layers the step only touches the batch's rows
// (LightGCN_SPEX/code/utility1/model.py:91-97,111-121 forward, autograd backward): the last layer at the 2B rows of the
// batch, the layer mean there, B dot products + BCE, the 2B gradient rows, and the first backward product A^T g in push
// form.  Issued as three launches (spex_spmm_rowlist_f32 -> spex_score_bce_slots_f32 -> spex_spmm_push_batch_f32) each
// costs a ramp plus its own chain of dependent round trips: 6.1 + 5.2 + 9 us for ~14 k gathers, 256 dot products and
// ~14 k row atomics on Epinion2.  spex_lightgcn_batch_f32 does the three in one kernel:
//
//   workgroup (sample b, part p), 16 waves
//     1. last layer at both rows of the sample — each row's 64-entry segments go to virtual waves v = segment mod 16 exactly
//        as the row-list kernel deals them (one accumulator chain per virtual wave), the two rows' virtual waves numbered
//        jointly and dealt to the 16 waves; a segment's 64 gathers are all in flight at once; segment sums meet in LDS and
//        are added in segment order: bit-identical to spex_spmm_rowlist_f32 / the main kernel for rows of <= 1024 entries;
//     2. light = (running sum + y) / (L + 1) for both rows -> LDS; every wave forms x = <light_u, light_i>, the sample's loss
//        and both gradient rows g_u = dg * light_i, g_i = dg * light_u, dg = (sigmoid(x) - label) / B;
//     3. push: out[col[e]] += val[e] * g / (L + 1) over the stored entries of both rows OF A (A^T g in push form walks the rows
//        of A: (A^T g)[c] = sum_r A[r, c] g[r]), runs of 16 entries numbered jointly and dealt over (part, wave) — their
//        (col, val) pairs were requested before step 1 —, plus out[row] += g / (L + 1) and the dense d loss / d light rows
//        (part 0 only).
//   PUSH == false (spex_lightgcn_batch_slots_f32, the deterministic step): steps 1 and 2 only; the sample's two gradient rows
//   leave with plain stores as grad_slots[b] (user side) and grad_slots[B + b] (item side) — no float atomics anywhere.
//   Up to kBatchParts = 3 workgroups share a sample when its rows are long (more than kBatchRunsPerPart = 16 runs per part) — each repeats the cheap, L2-resident forward, the parts of a shorter sample
//   leave at once.  The longest sample's push sets the launch time, and the reference's training batches (a random observed pair
//   or one of its five same-user negatives: users and positive items arrive in proportion to their degree) carry rows of ~1 000
//   entries all the time.  Measured on Epinion2, B = 256, us per step on uniform / training-shaped batches: 1 part 81.1 / 86.5,
//   2 parts (16 runs each) 83.6 / 84.7, 3 parts 81.1 / 83.2, 4 parts 89.5 / 91.4 (1 024 workgroups of 1 024 threads).
// The pieces all of these kernels share — the segment gather, the last layer at K rows, the push pipeline, the expert gate — and the
// two d == 64 kernels' bodies live in batch_kernels.h (batch_bf16.hip instantiates the bodies over a bf16 gather source); the host
// side is one launcher over a descriptor, spex::batch_launch below.
#include "batch_kernels.h"

using namespace spex;
using namespace spex::batchk;

namespace {

// (workgroup schedule: the comment at the top of this file; body: batch_kernels.h)
template <bool PUSH>
__global__ __launch_bounds__(kWave *kWgWaves) void lightgcn_batch_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows,
    int n_user_rows, const float *__restrict__ X, const float *__restrict__ acc_in, float acc_div,
    const int64_t *__restrict__ users, const int64_t *__restrict__ items, const float *__restrict__ labels, int parts,
    float grad_scale, float push_scale, float *loss_sum, float *__restrict__ loss_rows, float *g_out, float *G, int runs_per_part,
    float *__restrict__ grad_slots, int B, const float *__restrict__ acc2, const float *__restrict__ acc3, const spex::EdgeDrop drop)
{
    lightgcn_batch_body<PUSH>(rowptr, col, val, n_rows, n_user_rows, X, acc_in, acc_div, users, items, labels, parts, grad_scale, push_scale, loss_sum,
                              loss_rows, g_out, G, runs_per_part, grad_slots, B, acc2, acc3, drop);
}

// The batch-sized middle of the exact BPR step, three rows per workgroup (described at lightgcn_bpr_batch_body, batch_kernels.h).
template <bool PUSH>
__global__ __launch_bounds__(kWave *kWgWaves) void lightgcn_bpr_batch_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows, int n_user_rows,
    const float *__restrict__ X, const float *__restrict__ acc_in, float acc_div, const int64_t *__restrict__ users,
    const int64_t *__restrict__ pos, const int64_t *__restrict__ neg, int parts, float grad_scale, float push_scale, float *loss_sum,
    float *__restrict__ loss_rows, float *g_out, float *G, int runs_per_part, float *__restrict__ grad_slots, int T,
    const float *__restrict__ acc2, const float *__restrict__ acc3, float weight_decay, const float *__restrict__ E0,
    int32_t *row_counts, const spex::EdgeDrop drop)
{
    lightgcn_bpr_batch_body<PUSH>(rowptr, col, val, n_rows, n_user_rows, X, acc_in, acc_div, users, pos, neg, parts, grad_scale, push_scale, loss_sum,
                                  loss_rows, g_out, G, runs_per_part, grad_slots, T, acc2, acc3, weight_decay, E0, row_counts, drop);
}

// lightgcn_batch_kernel for wider embeddings, d = 64 V (V = 2, 4; V = 1 is the kernel above, kept as its own source like the
// d == 64 SpMM).  In the forward a lane owns V consecutive columns: a gathered row and a running-sum row are one coalesced
// 256 V-byte wave load each; behind the layer mean it owns columns lane, lane + 64, ..  Same workgroup shape, same dealing of segments to virtual waves and of push runs to (part, wave):
//   1. a segment's gathers are in flight 64 / V at a time (segment_sum_wide: 64 result registers at every width — the workgroup
//      has 16 waves, i.e. 128 VGPRs per lane); every column's chain runs in entry order and the segment sums are added in segment
//      order, so a row of <= 1 024 entries is bit-identical to the row spex_spmm_f32 (spmm_chunk_wide_kernel) and
//      spex_spmm_rowlist_f32 produce at this width;
//   2. the dot product is a lane's V products in ascending column order (one fmaf chain) and then the fixed DPP tree over the lanes;
//   3. the push issues V 256-byte atomics per stored entry (the V column blocks of the 256 V-byte row).
// LDS: segment partials [2][16][64 V] (column-major per lane: conflict-free) + the two light rows: 8.5 V KB.
template <bool PUSH, int V>
__global__ __launch_bounds__(kWave *kWgWaves) void lightgcn_batch_wide_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows,
    int n_user_rows, const float *__restrict__ X, const float *__restrict__ acc_in, float acc_div,
    const int64_t *__restrict__ users, const int64_t *__restrict__ items, const float *__restrict__ labels, int parts,
    float grad_scale, float push_scale, float *loss_sum, float *__restrict__ loss_rows, float *g_out, float *G, int runs_per_part,
    float *__restrict__ grad_slots, int B, const float *__restrict__ acc2, const float *__restrict__ acc3, const spex::EdgeDrop drop)
{
    typedef typename LaneVec<V>::T vec;
    constexpr int kRow = kWave * V;
    __shared__ float s_part[2][kWgWaves][kRow];   // [row: user, item][virtual wave][column block j][lane]
    __shared__ float s_light[2][kRow];            // the two light rows, by column
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x / parts, part = blockIdx.x % parts;
    const int64_t u64 = users[b], i64 = items[b];
    if (u64 < 0 || u64 >= n_user_rows || i64 < 0 || i64 + n_user_rows >= n_rows) {   // workgroup-uniform: never gather out of range
        if (loss_rows && part == 0 && threadIdx.x == 0) loss_rows[b] = 0.0f;
        if (!PUSH && wave < 2) {
#pragma unroll
            for (int c = 0; c < V; ++c) grad_slots[(size_t)(wave * B + b) * kRow + c * kWave + lane] = 0.0f;
        }
        return;
    }
    const int row[2] = {(int)u64, (int)i64 + n_user_rows};
    const RowSet<2> rows = RowSet<2>::of(rowptr, row[0], row[1]);
    const float y_lab = labels[b];
    vec run = (vec)(0.0f);
    if (wave < 2) run = running_sum<V>(acc_in, acc2, acc3, (size_t)row[wave] * kRow + lane * V);
    PushRuns<2> runs;
    if (!runs.begin(rows, PUSH, parts, runs_per_part, part, wave)) return;
    if (PUSH) runs.load(rows, col, val, drop, lane);
    // ---- 1. last layer at both rows
    last_layer_partials<2, V>(rows, col, val, X, drop, wave, lane, s_part);
    __syncthreads();
    // ---- 2. layer mean at both rows (waves 0 and 1), the score, both gradient rows
    if (wave < 2) {
        last_layer_mean<V>(s_part[wave], rows.n_virt(wave), run, acc_div, lane,
                           [&](int c, float s) { s_light[wave][lane * V + c] = s; });   // by column: what follows owns columns lane + 64 c
    }
    __syncthreads();
    // (from here on a lane owns columns lane, lane + 64, ...: every store and every atomic below covers 256 contiguous bytes)
    vec lu, li;
    float dot = 0.0f;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        lu[c] = s_light[0][c * kWave + lane];
        li[c] = s_light[1][c * kWave + lane];
        dot = fmaf(lu[c], li[c], dot);                                        // the lane's columns in ascending order (spex_score_bce_slots_f32's
    }                                                                         // chain), then the fixed tree over the lanes
    const float x = wave_sum_f32(dot);
    const float dg = (sigmoid_f(x) - y_lab) * grad_scale;
    const vec g2[2] = {dg * li, dg * lu};                                    // d loss / d light at the user row, at the item row
    if (part == 0 && wave < 2) {
        if (wave == 0 && lane == 0) {
            const float bce = fmaxf(x, 0.0f) - x * y_lab + log1pf(expf(-fabsf(x)));
            if (loss_rows) loss_rows[b] = bce;
            else atomicAdd(loss_sum, bce);
        }
        const vec gw = wave ? g2[1] : g2[0];
        if (!PUSH) {
#pragma unroll
            for (int c = 0; c < V; ++c) grad_slots[(size_t)(wave * B + b) * kRow + c * kWave + lane] = gw[c];
        } else {
            const size_t o = (size_t)row[wave] * kRow + lane;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                if (g_out) atomicAdd(g_out + o + c * kWave, gw[c]);           // dense d loss / d light_out; NULL: nobody reads it (L == 3 step)
                atomicAdd(G + o + c * kWave, push_scale * gw[c]);             // the `g` of (g + A^T g) / (L + 1)
            }
        }
    }
    if (!PUSH) return;
    // ---- 3. push over both rows' entries
    const vec gs2[2] = {push_scale * g2[0], push_scale * g2[1]};
    runs.template push<V>(rows, col, val, drop, G, lane, [&](int side) { return side ? gs2[1] : gs2[0]; });
}


// lightgcn_bpr_batch_kernel for wider embeddings, d = 64 V (V = 2, 4): the cross product of the two kernels above — three rows per
// workgroup as in lightgcn_bpr_batch_kernel (rows selected by wave-uniform sel3 selects on scalars, never an indexed array: no
// scratch), V consecutive columns per lane in the forward and columns lane, lane + 64, .. behind the layer mean as in
// lightgcn_batch_wide_kernel.  Same workgroup shape, same dealing of segments to virtual waves and of push runs to (part, wave),
// same kBprBatchParts / kBprBatchRunsPerPart.
//   1. forward through segment_sum_wide<V, MASKED> (64 result registers at every width), every column's chain in entry order, segment
//      sums added in segment order through LDS: a row of <= 1 024 entries is the spex_spmm_f32 row at this width bit for bit, masked
//      or not;
//   2. xp, xn: a lane's V products in ascending column order (one fmaf chain each), then the fixed DPP tree; z, loss, dg and the three
//      gradient rows as in the V = 1 kernel; |E0[r]|^2: a lane's V consecutive columns in ascending order (one chain from the first
//      square), then the same tree;
//   3. PUSH: V 256-byte atomics per row and per stored entry; !PUSH: the slots as V plain 256-byte stores per row.
// LDS: segment partials [3][16][64 V] + the three light rows + three norms: 12.75 V KB (25.5 KB at V = 2, 51 KB at V = 4).
template <bool PUSH, int V>
__global__ __launch_bounds__(kWave *kWgWaves) void lightgcn_bpr_batch_wide_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows, int n_user_rows,
    const float *__restrict__ X, const float *__restrict__ acc_in, float acc_div, const int64_t *__restrict__ users,
    const int64_t *__restrict__ pos, const int64_t *__restrict__ neg, int parts, float grad_scale, float push_scale, float *loss_sum,
    float *__restrict__ loss_rows, float *g_out, float *G, int runs_per_part, float *__restrict__ grad_slots, int T,
    const float *__restrict__ acc2, const float *__restrict__ acc3, float weight_decay, const float *__restrict__ E0,
    int32_t *row_counts, const spex::EdgeDrop drop)
{
    typedef typename LaneVec<V>::T vec;
    constexpr int kRow = kWave * V;
    __shared__ float s_part[3][kWgWaves][kRow];   // [row: user, positive, negative][virtual wave][column block j][lane]
    __shared__ float s_light[3][kRow];            // the three light rows, by column
    __shared__ float s_norm[3];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t = blockIdx.x / parts, part = blockIdx.x % parts;
    const int64_t u64 = users[t], p64 = pos[t], n64 = neg[t];
    const int64_t n_items = (int64_t)n_rows - n_user_rows;
    if (u64 < 0 || u64 >= n_user_rows || p64 < 0 || p64 >= n_items || n64 < 0 || n64 >= n_items) {   // workgroup-uniform
        if (loss_rows && part == 0 && threadIdx.x == 0) loss_rows[t] = 0.0f;
        if (!PUSH && wave < 3) {
#pragma unroll
            for (int c = 0; c < V; ++c) grad_slots[((size_t)wave * T + t) * kRow + c * kWave + lane] = 0.0f;
        }
        return;
    }
    const int r0 = (int)u64, r1 = (int)p64 + n_user_rows, r2 = (int)n64 + n_user_rows;
    const RowSet<3> rows = RowSet<3>::of(rowptr, r0, r1, r2);
    const int my_row = sel3(wave, r0, r1, r2);             // (waves 0 .. 2 own a row each behind the forward)
    // the running layer sum at the three rows and the E^0 rows of the L2 term
    vec run = (vec)(0.0f), e0v = (vec)(0.0f);
    if (wave < 3) {
        const size_t o = (size_t)my_row * kRow + lane * V;
        run = running_sum<V>(acc_in, acc2, acc3, o);
        if (weight_decay > 0.0f) e0v = *reinterpret_cast<const vec *>(E0 + o);
    }
    const bool push = PUSH && G != nullptr;                 // (G == NULL: the dense form — gradient rows into g_out only, no push)
    PushRuns<3> runs;
    if (!runs.begin(rows, push, parts, runs_per_part, part, wave)) return;
    if (push) runs.load(rows, col, val, drop, lane);
    // ---- 1. last layer at the three rows
    last_layer_partials<3, V>(rows, col, val, X, drop, wave, lane, s_part);
    __syncthreads();
    // ---- 2. layer mean at the three rows (waves 0 .. 2), the two scores, the three gradient rows
    if (wave < 3) {
        last_layer_mean<V>(s_part[wave], rows.n_virt(wave), run, acc_div, lane,
                           [&](int c, float s) { s_light[wave][lane * V + c] = s; });   // by column: what follows owns columns lane + 64 c
        if (weight_decay > 0.0f) {
            float sq = e0v[0] * e0v[0];
#pragma unroll
            for (int c = 1; c < V; ++c) sq = fmaf(e0v[c], e0v[c], sq);        // the lane's columns in ascending order, then the fixed tree
            const float nrm = wave_sum_f32(sq);
            if (lane == 0) s_norm[wave] = nrm;
        }
    }
    __syncthreads();
    // (from here on a lane owns columns lane, lane + 64, ...: every store and every atomic below covers 256 contiguous bytes)
    vec lu, lp, ln;
    float dp = 0.0f, dn = 0.0f;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        lu[c] = s_light[0][c * kWave + lane];
        lp[c] = s_light[1][c * kWave + lane];
        ln[c] = s_light[2][c * kWave + lane];
        dp = fmaf(lu[c], lp[c], dp);
        dn = fmaf(lu[c], ln[c], dn);
    }
    const float xp = wave_sum_f32(dp), xn = wave_sum_f32(dn);
    const float z = xn - xp;
    const float dg = sigmoid_f(z) * grad_scale;
    const vec gn = dg * lu, gu = dg * (ln - lp), gp = -gn;   // d loss / d light at the negative, the user, the positive row
    if (part == 0 && wave < 3) {
        if (wave == 0 && lane == 0) {
            float loss = fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z)));
            if (weight_decay > 0.0f) loss = loss + 0.5f * weight_decay * ((s_norm[0] + s_norm[1]) + s_norm[2]);
            if (loss_rows) loss_rows[t] = loss;
            else atomicAdd(loss_sum, loss);
        }
        if (row_counts && lane == 0) atomicAdd(row_counts + my_row, 1);       // occurrences of the row in the batch: the L2 gradient's weight
        const vec gw = wave == 0 ? gu : (wave == 1 ? gp : gn);
        if (!PUSH) {
#pragma unroll
            for (int c = 0; c < V; ++c) grad_slots[((size_t)wave * T + t) * kRow + c * kWave + lane] = gw[c];
        } else {
            const size_t o = (size_t)my_row * kRow + lane;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                if (g_out) atomicAdd(g_out + o + c * kWave, gw[c]);
                if (push) atomicAdd(G + o + c * kWave, push_scale * gw[c]);   // the `g` of (g + A^T g) / (L + 1)
            }
        }
    }
    if (!push) return;
    // ---- 3. push over the three rows' entries
    const vec gsu = push_scale * gu, gsp = push_scale * gp, gsn = push_scale * gn;
    runs.template push<V>(rows, col, val, drop, G, lane, [&](int side) { return side == 0 ? gsu : (side == 1 ? gsp : gsn); });
}

// The dual-task model's rec branch has the expert gate between the layer mean and the score (utility1/model_expert_s.py:154-168),
// so its batch-sized middle cannot include the push (the gate's backward comes first).  Its FORWARD half is one launch of the
// same shape: last layer at the sample's two rows (step 1 above) -> layer mean (written to lo_batch[row]: the gate's backward
// reads it) -> waves 0 / 1 gate the user / item row (softmax([raw | light] att) two-way mix) -> score, loss, and the two
// per-sample gradient rows with respect to the GATED rows (grad_slots[b], grad_slots[B + b]) — what spex_spmm_rowlist_f32 ->
// spex_expert_gate_rows_f32 -> spex_score_bce_slots_f32 computed in three launches.
__global__ __launch_bounds__(kWave *kWgWaves) void gated_batch_fwd_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows, int n_user_rows,
    const float *__restrict__ X, const float *__restrict__ acc_in, float acc_div, const float *__restrict__ raw,
    const float *__restrict__ att_u, const float *__restrict__ att_i, const int64_t *__restrict__ users,
    const int64_t *__restrict__ items, const float *__restrict__ labels, int B, float grad_scale, float *loss_sum,
    float *__restrict__ lo_batch, float *__restrict__ grad_slots, float *__restrict__ loss_rows, const float *__restrict__ acc2,
    const float *__restrict__ acc3, const spex::EdgeDrop drop)
{
    __shared__ float s_part[2][kWgWaves][kWave];
    __shared__ float s_mixed[2][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x;
    const int64_t u64 = users[b], i64 = items[b];
    const float y_lab = labels[b];
    if (u64 < 0 || u64 >= n_user_rows || i64 < 0 || i64 + n_user_rows >= n_rows) {   // workgroup-uniform: never gather out of range
        if (wave < 2) grad_slots[(size_t)(wave * B + b) * kWave + lane] = 0.0f;       // gated rows of 0: x = 0, no gradient
        if (threadIdx.x == 0) {                                                        // (what the three launches did: BCE(0, y))
            if (loss_rows) loss_rows[b] = 0.693147180559945309f;
            else atomicAdd(loss_sum, 0.693147180559945309f);
        }
        return;
    }
    const int row[2] = {(int)u64, (int)i64 + n_user_rows};
    const RowSet<2> rows = RowSet<2>::of(rowptr, row[0], row[1]);
    float run = 0.0f, a_raw = 0.0f;
    GateW w;
    if (wave < 2) {                       // the gate's operands, requested with everything else
        const size_t o = (size_t)row[wave] * kWave + lane;
        run = running_sum<1>(acc_in, acc2, acc3, o);
        a_raw = raw[o];
        w.load(wave ? att_i : att_u, lane);
    }
    last_layer_partials<2, 1>(rows, col, val, X, drop, wave, lane, s_part);
    __syncthreads();
    if (wave < 2) {
        float s = 0.0f;
        last_layer_mean<1>(s_part[wave], rows.n_virt(wave), run, acc_div, lane, [&](int, float v) { s = v; });
        lo_batch[(size_t)row[wave] * kWave + lane] = s;                        // (a row named twice is written twice with the same value)
        float a0, a1;
        s_mixed[wave][lane] = gate_forward(w, a_raw, s, a0, a1);
    }
    __syncthreads();
    if (wave < 2) {
        const float mu = s_mixed[0][lane], mi = s_mixed[1][lane];
        const float x = wave_sum_f32(fmaf(mu, mi, 0.0f));
        const float dg = (sigmoid_f(x) - y_lab) * grad_scale;
        grad_slots[(size_t)(wave * B + b) * kWave + lane] = dg * (wave ? mu : mi);
        if (wave == 0 && lane == 0) {
            const float bce = fmaxf(x, 0.0f) - x * y_lab + log1pf(expf(-fabsf(x)));
            if (loss_rows) loss_rows[b] = bce;            // deterministic step: summed in sample order afterwards
            else atomicAdd(loss_sum, bce);
        }
    }
}


// The WHOLE batch-sized middle of the dual-task rec branch as one launch (spex_gated_batch_f32; the fast, atomic path of
// spex_dual_task_step_f32): gated_batch_fwd_kernel's forward, then — the gate's Jacobian is linear in the incoming gradient and
// local to the sample's two rows — the gate's backward in the same two waves (expert_gate_rows_bwd_kernel's arithmetic, operand
// for operand: d raw, d light, the two gate matrices' gradients), and the first backward product in push form over the rows of A
// exactly as lightgcn_batch_kernel<true> runs it (runs of 16 entries dealt over (part, wave), loaded ahead of the forward).
// Three launches (10.1 + 5.0 + 10.2 us on Epinion2, B = 256) and two launch boundaries of a dependent chain become one.
//   g_prop[r]  += d light            (dense d loss / d light: the epilogue operand of the later backward launches, Adam's share)
//   G[r]       += push_scale * d light,   G[col[e]] += val[e] * push_scale * d light over the stored entries of row r of A
//   g_raw[r]   += d raw              (the gate's direct path into E^0)
//   g_att[b mod n_att_copies] += the gate matrices' gradients ([att_u | att_i], [128, 2] each; 4 values per lane, one atomic each)
__global__ __launch_bounds__(kWave *kWgWaves) void gated_batch_push_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows, int n_user_rows,
    const float *__restrict__ X, const float *__restrict__ acc_in, float acc_div, const float *__restrict__ raw,
    const float *__restrict__ att_u, const float *__restrict__ att_i, const int64_t *__restrict__ users,
    const int64_t *__restrict__ items, const float *__restrict__ labels, int parts, int runs_per_part, float grad_scale,
    float push_scale, float *loss_sum, float *g_prop, float *G, float *g_raw, float *g_att, int n_att_copies,
    const float *__restrict__ acc2, const float *__restrict__ acc3, const spex::EdgeDrop drop)
{
    __shared__ float s_part[2][kWgWaves][kWave];
    __shared__ float s_mixed[2][kWave];
    __shared__ float s_dprop[2][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x / parts, part = blockIdx.x % parts;
    const int64_t u64 = users[b], i64 = items[b];
    const float y_lab = labels[b];
    if (u64 < 0 || u64 >= n_user_rows || i64 < 0 || i64 + n_user_rows >= n_rows) {   // workgroup-uniform: never gather out of range
        if (part == 0 && threadIdx.x == 0) atomicAdd(loss_sum, 0.693147180559945309f);   // gated rows of 0: BCE(0, y), no gradient
        return;
    }
    const int row[2] = {(int)u64, (int)i64 + n_user_rows};
    const RowSet<2> rows = RowSet<2>::of(rowptr, row[0], row[1]);
    float run = 0.0f, a_raw = 0.0f;
    GateW w;
    if (wave < 2) {                       // the gate's operands, requested with everything else
        const size_t o = (size_t)row[wave] * kWave + lane;
        run = running_sum<1>(acc_in, acc2, acc3, o);
        a_raw = raw[o];
        w.load(wave ? att_i : att_u, lane);
    }
    // the push's runs (the forward's rows again: A^T g in push form walks the rows of A), shared by up to `parts` workgroups
    PushRuns<2> runs;
    if (!runs.begin(rows, true, parts, runs_per_part, part, wave)) return;
    runs.load(rows, col, val, drop, lane);
    // ---- 1. last layer at both rows (gated_batch_fwd_kernel's / the row-list kernel's order of sums)
    last_layer_partials<2, 1>(rows, col, val, X, drop, wave, lane, s_part);
    __syncthreads();
    // ---- 2. layer mean + gate (waves 0 / 1: the user / the item row)
    float s = 0.0f, a0 = 0.0f, a1 = 0.0f;
    if (wave < 2) {
        last_layer_mean<1>(s_part[wave], rows.n_virt(wave), run, acc_div, lane, [&](int, float v) { s = v; });
        s_mixed[wave][lane] = gate_forward(w, a_raw, s, a0, a1);
    }
    __syncthreads();
    // ---- 3. score, loss, d loss / d gated rows, and the gate's backward for this sample's two rows
    if (wave < 2) {
        const float mu = s_mixed[0][lane], mi = s_mixed[1][lane];
        const float x = wave_sum_f32(fmaf(mu, mi, 0.0f));
        const float dg = (sigmoid_f(x) - y_lab) * grad_scale;
        const float gg = dg * (wave ? mu : mi);
        float d_raw, d_prop, dz0, dz1;
        gate_backward(w, a_raw, s, a0, a1, gg, d_raw, d_prop, dz0, dz1);
        s_dprop[wave][lane] = d_prop;
        if (part == 0) {
            const size_t o = (size_t)row[wave] * kWave + lane;
            if (g_prop) atomicAdd(g_prop + o, d_prop);                    // (NULL: nobody reads it — the L == 3 step)
            atomicAdd(G + o, push_scale * d_prop);
            atomicAdd(g_raw + o, d_raw);
            gate_att_add(g_att + (size_t)(b % n_att_copies) * 512 + wave * 256, lane, a_raw, s, dz0, dz1);
            if (wave == 0 && lane == 0) atomicAdd(loss_sum, fmaxf(x, 0.0f) - x * y_lab + log1pf(expf(-fabsf(x))));
        }
    }
    __syncthreads();
    // ---- 4. push over both rows' entries
    const float g2[2] = {push_scale * s_dprop[0][lane], push_scale * s_dprop[1][lane]};
    runs.template push<1>(rows, col, val, drop, G, lane, [&](int side) { return side ? g2[1] : g2[0]; });
}



// The last forward layer of a ROW-PARTITIONED step at the batch's rows (d == 64; comm.hip).  Slot k names position pos[k] of the
// padded global layout; on the rank that owns it (lo <= pos[k] < lo + n_rows) the row-list kernel's sum for the rank's local row
// r = pos[k] - lo — wave w takes segments w, w + 16, ... as one chain, the waves' sums are added in wave order: the same bits for
// every row of up to 1 024 entries — gives the layer mean (acc_in [+ acc2 + acc3] + A X)[r] / acc_div, stored COMPACT at out_prop[k]
// beside the raw row out_raw[k] = raw[r]; every other slot is ZERO-filled on this rank: the two buffers are the operands of the
// owner-computes all-reduce that hands every rank the batch's rows.  Replaces a whole-block launch + two gather launches.  Under
// edge dropout (a mask on the handle) the entries are kept / dropped by the handle's rule, exactly as spmm_chunk_kernel<.., MASKED>.
__global__ __launch_bounds__(kWave *kWgWaves) void owned_rows_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ X, const int64_t *__restrict__ pos, int64_t lo, int32_t n_rows, const float *__restrict__ acc_in,
    const float *__restrict__ acc2, const float *__restrict__ acc3, float acc_div, const float *__restrict__ raw,
    float *__restrict__ out_prop, float *__restrict__ out_raw, const spex::EdgeDrop drop)
{
    __shared__ float s_part[kWgWaves][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t ko = (size_t)blockIdx.x * kWave + lane;
    const int64_t r64 = pos[blockIdx.x] - lo;
    if (r64 < 0 || r64 >= n_rows) {                               // workgroup-uniform: another rank's row (or no row at all)
        if (wave == 0) out_prop[ko] = 0.0f;
        if (wave == 1 && out_raw) out_raw[ko] = 0.0f;
        return;
    }
    const int r = (int)r64;
    const size_t o = (size_t)r * kWave + lane;
    float run = 0.0f, r2 = 0.0f, r3 = 0.0f;
    if (wave == 0) {                                               // the epilogue's operands, requested with the row's entries
        run = acc_in[o];
        if (acc2) r2 = acc2[o];
        if (acc3) r3 = acc3[o];
    }
    if (wave == 1 && out_raw) out_raw[ko] = raw[o];
    const int beg = rowptr[r], deg = rowptr[r + 1] - beg;
    const int nseg = (deg + kTaskEntries - 1) / kTaskEntries;
    const float *__restrict__ Xl = X + lane;
    float acc = 0.0f;
    for (int sgi = wave; sgi < nseg; sgi += kWgWaves) {
        const int left = deg - sgi * kTaskEntries;
        if (drop.mode != 0)
            acc = segment_sum<true>(col, val, Xl, beg + sgi * kTaskEntries, left < kTaskEntries ? left : kTaskEntries, lane, acc, drop);
        else
            acc = segment_sum<false>(col, val, Xl, beg + sgi * kTaskEntries, left < kTaskEntries ? left : kTaskEntries, lane, acc, drop);
    }
    if (nseg > 1) {
        if (wave != 0 && wave < nseg) s_part[wave][lane] = acc;
        __syncthreads();
    }
    if (wave == 0) {
        float y = acc;
        const int lim = nseg < kWgWaves ? nseg : kWgWaves;
        for (int w = 1; w < lim; ++w) y = y + s_part[w][lane];    // wave order
        if (acc2) run = run + r2;                                  // (the layer tables in layer order, as the one-GPU batch kernels add them)
        if (acc3) run = run + r3;
        float s = run + y;
        if (acc_div != 1.0f) s = s / acc_div;
        out_prop[ko] = s;
    }
}

// The batch-sized middle of the one-call steps on a ROW PARTITION (comm.hip: the fast paths of spex_partitioned_step_bce_f32 and
// spex_partitioned_dual_task_step_f32).  The batch's rows arrive COMPACT and complete on every rank (rows_prop / rows_raw [2B, 64]:
// slot b = sample b's user row, slot B + b its item row — the owner-computes all-reduce behind spex_spmm_owned_rows_f32), so
// everything between the forward and the first backward product is one launch, computed REDUNDANTLY by every rank (which is why
// the loss and the two gate matrices' gradients are complete everywhere without a collective):
//   GATED  gate, score, loss and the gate's backward — gated_batch_push_kernel's steps 2-3, operand for operand (waves 0 / 1)
//   plain  score, loss, the two gradient rows — lightgcn_batch_kernel's step 2
//   part 0 of a sample, for a slot whose row this rank owns (lo <= pos[slot] < lo + n_local; r = pos[slot] - lo):
//          P[r] += push_scale * d_prop  (the g term of (g + A^T g) / (L+1)),  g_prop[r] += d_prop (if g_prop),  g_raw[r] += d_raw
//   then the first backward product in push form WITHOUT an exchange: every rank pushes BOTH gradient rows of EVERY sample through
//   its own columns of A — the matrix (rowptr, col, val) is the (world * max_rows) x n_local transpose of the rank's block of A^T,
//   row p = the entries A[p, c] for the rank's columns c: P[col[e]] += push_scale * val[e] * d_prop over the entries of rows
//   pos[b], pos[B + b] (runs of 16 entries dealt over (part, wave) and loaded ahead, as in lightgcn_batch_kernel<true>; under edge
//   dropout the structure carries the entries' global edge ids and the forward's mask: kept values / keep_prob, dropped ones nothing).
// rowptr == NULL: a rank without rows (nothing to push, nothing owned) — it still forms the loss and the gate gradients.
template <bool GATED>
__global__ __launch_bounds__(kWave *kWgWaves) void rows_train_push_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_push_rows,
    const float *__restrict__ rows_raw, const float *__restrict__ rows_prop, const float *__restrict__ att_u,
    const float *__restrict__ att_i, const int64_t *__restrict__ pos, int64_t lo, int n_local, const float *__restrict__ labels, int B,
    int parts, int runs_per_part, float grad_scale, float push_scale, float *loss_sum, float *g_prop, float *P, float *g_raw,
    float *g_att, int n_att_copies, const spex::EdgeDrop drop)
{
    __shared__ float s_mixed[2][kWave];
    __shared__ float s_dprop[2][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x / parts, part = blockIdx.x % parts;
    const int64_t p64[2] = {pos[b], pos[(size_t)B + b]};
    const float y_lab = labels[b];
    int beg[2] = {0, 0}, deg[2] = {0, 0};
#pragma unroll
    for (int w = 0; w < 2; ++w)
        if (rowptr && p64[w] >= 0 && p64[w] < n_push_rows) {      // (a position without a row in the push structure: an empty row)
            beg[w] = rowptr[p64[w]];
            deg[w] = rowptr[p64[w] + 1] - beg[w];
        }
    const RowSet<2> rows = {beg[0], beg[1], 0, deg[0], deg[1], 0};
    float a_raw = 0.0f, s = 0.0f;
    GateW w;
    if (wave < 2) {                       // the operands, requested with everything else
        const size_t o = ((size_t)wave * B + b) * kWave + lane;
        s = rows_prop[o];
        if (GATED) {
            a_raw = rows_raw[o];
            w.load(wave ? att_i : att_u, lane);
        }
    }
    PushRuns<2> runs;
    if (!runs.begin(rows, true, parts, runs_per_part, part, wave)) return;
    runs.load(rows, col, val, drop, lane);
    // ---- gate (GATED) -> the rows that are scored
    float a0 = 0.0f, a1 = 0.0f;
    if (wave < 2) {
        float mixed = s;
        if (GATED) mixed = gate_forward(w, a_raw, s, a0, a1);
        s_mixed[wave][lane] = mixed;
    }
    __syncthreads();
    // ---- score, loss, d loss / d scored rows (and through the gate), the owned rows' shares
    if (wave < 2) {
        const float mu = s_mixed[0][lane], mi = s_mixed[1][lane];
        const float x = wave_sum_f32(fmaf(mu, mi, 0.0f));
        const float dg = (sigmoid_f(x) - y_lab) * grad_scale;
        const float gg = dg * (wave ? mu : mi);
        float d_raw = 0.0f, d_prop = gg, dz0 = 0.0f, dz1 = 0.0f;
        if (GATED) gate_backward(w, a_raw, s, a0, a1, gg, d_raw, d_prop, dz0, dz1);
        s_dprop[wave][lane] = d_prop;
        if (part == 0) {
            const int64_t r64 = p64[wave] - lo;
            if (r64 >= 0 && r64 < n_local) {                              // wave-uniform: the rows this rank owns
                const size_t o = (size_t)r64 * kWave + lane;
                if (g_prop) atomicAdd(g_prop + o, d_prop);
                atomicAdd(P + o, push_scale * d_prop);
                if (GATED) atomicAdd(g_raw + o, d_raw);
            }
            if (GATED) gate_att_add(g_att + (size_t)(b % n_att_copies) * 512 + wave * 256, lane, a_raw, s, dz0, dz1);
            if (wave == 0 && lane == 0) atomicAdd(loss_sum, fmaxf(x, 0.0f) - x * y_lab + log1pf(expf(-fabsf(x))));
        }
    }
    if (runs.n_runs == 0) return;                                          // (workgroup-uniform)
    __syncthreads();
    // ---- push over both rows' entries in the rank's columns
    const float g2[2] = {push_scale * s_dprop[0][lane], push_scale * s_dprop[1][lane]};
    runs.template push<1>(rows, col, val, drop, P, lane, [&](int side) { return side ? g2[1] : g2[0]; });
}

}  // namespace

extern "C" int spex_gated_batch_fwd_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const float *raw,
                                       const float *att_u, const float *att_i, const int64_t *users, const int64_t *items,
                                       const float *labels, int32_t B, int32_t n_user_rows, float grad_scale, float *loss_sum,
                                       float *loss_per_sample, float *lo_batch, float *grad_slots, int32_t d, void *stream)
{
    return spex::gated_batch_fwd_layers(g, X, acc_in, nullptr, nullptr, acc_div, raw, att_u, att_i, users, items, labels, B, n_user_rows,
                                        grad_scale, loss_sum, loss_per_sample, lo_batch, grad_slots, d, stream);
}

int spex::gated_batch_fwd_layers(const spex_graph_t *g, const float *X, const float *acc_in, const float *acc2, const float *acc3,
                                 float acc_div, const float *raw, const float *att_u, const float *att_i, const int64_t *users,
                                 const int64_t *items, const float *labels, int32_t B, int32_t n_user_rows, float grad_scale,
                                 float *loss_sum, float *loss_per_sample, float *lo_batch, float *grad_slots, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && X && acc_in && raw && att_u && att_i && users && items && labels && (loss_sum || loss_per_sample) && lo_batch
                       && grad_slots,
                   "spex_gated_batch_fwd_f32: NULL argument");
    SPEX_CHECK_ARG(B >= 0 && n_user_rows >= 0 && n_user_rows <= g->n_rows && g->n_rows == g->n_cols,
                   "spex_gated_batch_fwd_f32: B=%d n_user_rows=%d on a %d x %d graph", B, n_user_rows, g->n_rows, g->n_cols);
    if (d != kWave) {
        spex::set_error("spex_gated_batch_fwd_f32: d == 64 only (got %d)", d);
        return SPEX_ERR_UNSUPPORTED;
    }
    if (B == 0 || g->n_rows == 0) return SPEX_OK;
    hipLaunchKernelGGL(gated_batch_fwd_kernel, dim3((unsigned)B), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->val,
                       g->n_rows, n_user_rows, X, acc_in, acc_div, raw, att_u, att_i, users, items, labels, B, grad_scale, loss_sum, lo_batch,
                       grad_slots, loss_per_sample, acc2, acc3, edge_drop_of(g));
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_gated_batch_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const float *raw,
                                   const float *att_u, const float *att_i, const int64_t *users, const int64_t *items,
                                   const float *labels, int32_t B, int32_t n_user_rows, float grad_scale, float push_scale,
                                   float *loss_sum, float *g_prop, float *G, float *g_raw, float *g_att, int32_t n_att_copies,
                                   int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g_prop, "spex_gated_batch_f32: NULL g_prop");
    return spex::gated_batch_push_layers(g, X, acc_in, nullptr, nullptr, acc_div, raw, att_u, att_i, users, items, labels, B, n_user_rows,
                                         grad_scale, push_scale, loss_sum, g_prop, G, g_raw, g_att, n_att_copies, d, stream);
}

int spex::gated_batch_push_layers(const spex_graph_t *g, const float *X, const float *acc_in, const float *acc2, const float *acc3,
                                  float acc_div, const float *raw, const float *att_u, const float *att_i, const int64_t *users,
                                  const int64_t *items, const float *labels, int32_t B, int32_t n_user_rows, float grad_scale,
                                  float push_scale, float *loss_sum, float *g_prop, float *G, float *g_raw, float *g_att,
                                  int32_t n_att_copies, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && X && acc_in && raw && att_u && att_i && users && items && labels && loss_sum && G && g_raw && g_att,
                   "spex_gated_batch_f32: NULL argument");
    SPEX_CHECK_ARG(n_att_copies >= 1, "spex_gated_batch_f32: n_att_copies=%d", n_att_copies);
    SPEX_CHECK_ARG(B >= 0 && n_user_rows >= 0 && n_user_rows <= g->n_rows && g->n_rows == g->n_cols,
                   "spex_gated_batch_f32: B=%d n_user_rows=%d on a %d x %d graph", B, n_user_rows, g->n_rows, g->n_cols);
    SPEX_CHECK_ARG(G != g_prop && G != g_raw && g_prop != g_raw, "spex_gated_batch_f32: g_prop, G and g_raw are three tables");
    if (d != kWave) {
        spex::set_error("spex_gated_batch_f32: d == 64 only (got %d)", d);
        return SPEX_ERR_UNSUPPORTED;
    }
    if (B == 0 || g->n_rows == 0) return SPEX_OK;
    constexpr int runs_per_part = kBatchRunsPerPart, parts = kBatchParts;
    hipLaunchKernelGGL(gated_batch_push_kernel, dim3((unsigned)B * parts), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col,
                       g->val, g->n_rows, n_user_rows, X, acc_in, acc_div, raw, att_u, att_i, users, items, labels, parts, runs_per_part,
                       grad_scale, push_scale, loss_sum, g_prop, G, g_raw, g_att, n_att_copies, acc2, acc3, edge_drop_of(g));
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

#ifdef SPEX_STAMPS
extern "C" int spex_debug_batch_stamps(unsigned long long *out)
{
    SPEX_HIP(hipDeviceSynchronize());
    SPEX_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 16));
    return SPEX_OK;
}
#endif

// ---- the one launcher of the sample / triple kernels of both translation units: checks the descriptor — each
//      family of exports keeps the order, status codes and texts of its checks —, picks the grid and the kernel, launches.

// The wide batch kernels move rows as dwordx2 / dwordx4 per lane: their source tables must be 16-byte aligned.
static bool wide_aligned(const void *a, const float *b, const float *c, const float *d)
{
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

static const char *entry_name(const spex::BatchLaunch &L)      // the export that takes this form
{
    static const char *const names[2][2][3] = {                // [bpr][push][fp32 d == 64 | fp32 d = 128, 256 | bf16]
        {{"spex_lightgcn_batch_slots_f32", "spex_lightgcn_batch_slots_f32", "spex_lightgcn_batch_slots_bf16_f32"},
         {"spex_lightgcn_batch_f32", "spex_lightgcn_batch_f32", "spex_lightgcn_batch_bf16_f32"}},
        {{"spex_lightgcn_bpr_batch_slots_f32", "spex_lightgcn_bpr_batch_slots_wide_f32", "spex_lightgcn_bpr_batch_slots_bf16_f32"},
         {"spex_lightgcn_bpr_batch_f32", "spex_lightgcn_bpr_batch_wide_f32", "spex_lightgcn_bpr_batch_bf16_f32"}}};
    return names[L.bpr][L.push][L.x_bf16 ? 2 : (L.d == kWave ? 0 : 1)];
}

template <bool PUSH>
static void launch_f32(const spex::BatchLaunch &L, int parts, int runs_per_part)
{
    if (!L.bpr) {
        if (L.d == kWave) launch_two_rows<float>(lightgcn_batch_kernel<PUSH>, L, parts, runs_per_part);
        else if (L.d == 2 * kWave) launch_two_rows<float>(lightgcn_batch_wide_kernel<PUSH, 2>, L, parts, runs_per_part);
        else launch_two_rows<float>(lightgcn_batch_wide_kernel<PUSH, 4>, L, parts, runs_per_part);
    } else {
        if (L.d == kWave) launch_three_rows<float>(lightgcn_bpr_batch_kernel<PUSH>, L, parts, runs_per_part);
        else if (L.d == 2 * kWave) launch_three_rows<float>(lightgcn_bpr_batch_wide_kernel<PUSH, 2>, L, parts, runs_per_part);
        else launch_three_rows<float>(lightgcn_bpr_batch_wide_kernel<PUSH, 4>, L, parts, runs_per_part);
    }
}

int spex::batch_launch(const BatchLaunch &L)
{
    const char *who = L.who ? L.who : entry_name(L);
    const spex_graph_t *g = L.g;
    const int32_t n = L.n, n_u = L.n_user_rows, d = L.d;
    const bool idx = L.a && L.b && (L.bpr ? L.c != nullptr : L.labels != nullptr), loss = L.loss_sum || L.loss_rows;
    const bool l2_ok = L.weight_decay >= 0.0f && (L.weight_decay == 0.0f || L.E0), any_width = d == kWave || d == 2 * kWave || d == 4 * kWave;
    if (L.x_bf16) {            // (the kernels walk the handle's CSR arrays, not its chunk tables: any handle will do)
        if (d != kWave) {
            spex::set_error("%s: bf16 gather tables are built for d == 64 only (d = %d): use the fp32 entries", who, d);
            return SPEX_ERR_UNSUPPORTED;
        }
        SPEX_CHECK_ARG(g && L.X && L.acc_in && n >= 0 && L.acc_div != 0.0f && (!L.acc3 || L.acc2),
                       "%s: NULL argument, a negative count, acc_div == 0 or acc3 without acc2", who);
        SPEX_CHECK_ARG(n_u >= 0 && n_u <= g->n_rows && g->n_rows == g->n_cols, "%s: n_user_rows=%d on a %d x %d graph", who, n_u, g->n_rows, g->n_cols);
        SPEX_CHECK_ARG((((uintptr_t)L.X) & 1) == 0 && L.X != (const void *)L.acc_in, "%s: X16 misaligned or aliasing acc_in", who);
        if (!L.push) SPEX_CHECK_ARG((n == 0 || idx) && loss && L.slots, "%s: NULL argument", who);
        else if (!L.bpr) SPEX_CHECK_ARG((n == 0 || idx) && loss && L.G && L.G != L.g_out, "%s: NULL argument (or G == g_out)", who);
        else
            SPEX_CHECK_ARG((n == 0 || idx) && loss && (L.G || L.g_out) && L.G != L.g_out,
                           "%s: needs loss_sum or loss_per_sample, G and / or g_out (two tables)", who);
        if (L.bpr) SPEX_CHECK_ARG(l2_ok, "%s: weight_decay %g needs E0 (and must not be negative)", who, (double)L.weight_decay);
    } else if (L.bpr) {
        SPEX_CHECK_ARG(g && L.X && L.acc_in && n >= 0 && (n == 0 || idx), "%s: NULL argument or T < 0", who);
        SPEX_CHECK_ARG(n_u >= 0 && n_u <= g->n_rows && g->n_rows == g->n_cols, "%s: n_user_rows=%d on a %d x %d graph", who, n_u, g->n_rows, g->n_cols);
        SPEX_CHECK_ARG(l2_ok, "%s: weight_decay %g needs E0 (and must not be negative)", who, (double)L.weight_decay);
        // (the narrow exports promised d == 64 only — their callers' tables are 64 wide: a larger d would gather out of bounds — so
        //  the wide kernel has exports of its own)
        if (L.widths == BatchLaunch::kNarrow && d != kWave) {
            spex::set_error("%s: d == 64 only (got %d); d = 128 / 256 take the _wide entry point", who, d);
            return SPEX_ERR_UNSUPPORTED;
        }
        if (L.widths == BatchLaunch::kWide && d != 2 * kWave && d != 4 * kWave) {
            spex::set_error("%s: d = 128 or 256 only (got %d); d == 64 takes the narrow entry point (the name without _wide)", who, d);
            return SPEX_ERR_UNSUPPORTED;
        }
        if (!any_width) {
            spex::set_error("%s: d = 64, 128 or 256 only (got %d)", who, d);
            return SPEX_ERR_UNSUPPORTED;
        }
        if (!L.push)
            SPEX_CHECK_ARG(loss && L.slots && L.acc_div != 0.0f && (!L.acc3 || L.acc2),
                           "%s: needs loss_sum or loss_per_sample, grad_slots, acc_div != 0 (and acc2 with acc3)", who);
        else
            SPEX_CHECK_ARG(loss && (L.G || L.g_out) && L.G != L.g_out && L.acc_div != 0.0f && (!L.acc3 || L.acc2),
                           "%s: needs loss_sum or loss_per_sample, G and / or g_out (two tables), acc_div != 0 (and acc2 with acc3)", who);
        SPEX_CHECK_ARG(d == kWave || (wide_aligned(L.X, L.acc_in, L.acc2, L.acc3) && wide_aligned(L.E0, nullptr, nullptr, nullptr)),
                       "%s: X / acc_in / E0 must be 16-byte aligned at d > 64", who);
    } else {
        SPEX_CHECK_ARG(g && L.X && L.acc_in && idx && loss && (L.push ? L.G : L.slots), "%s: NULL argument", who);
        SPEX_CHECK_ARG(n >= 0 && n_u >= 0 && n_u <= g->n_rows, "%s: B=%d n_user_rows=%d", who, n, n_u);
        SPEX_CHECK_ARG(g->n_rows == g->n_cols, "%s: square graph", who);
        if (!any_width) {
            spex::set_error("%s: d = 64, 128 or 256 only (got %d)", who, d);
            return SPEX_ERR_UNSUPPORTED;
        }
        SPEX_CHECK_ARG(d == kWave || wide_aligned(L.X, L.acc_in, L.acc2, L.acc3), "%s: X / acc_in must be 16-byte aligned at d > 64", who);
    }
    if (n == 0 || g->n_rows == 0) return SPEX_OK;
    // the slots form and the BPR form without a push (G == NULL): one workgroup per sample
    const int parts = !L.push ? 1 : (L.bpr ? (L.G ? kBprBatchParts : 1) : kBatchParts);
    const int runs_per_part = !L.push ? 1 : (L.bpr ? kBprBatchRunsPerPart : kBatchRunsPerPart);
    SPEX_CHECK_ARG((int64_t)n * parts < (int64_t)1 << 31, "%s: %c=%d is too many %s for one launch", who, L.bpr ? 'T' : 'B', n,
                   L.bpr ? "triples" : "samples");
    if (L.x_bf16) return spex::batch_launch_bf16(L, parts, runs_per_part);
    if (L.push) launch_f32<true>(L, parts, runs_per_part);
    else launch_f32<false>(L, parts, runs_per_part);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

// ---- the ten exports: fillers of the descriptor.  (acc2 / acc3 stay NULL: the exports take one running sum.)
static spex::BatchLaunch entry(const char *who, const spex_graph_t *g, const void *X, const float *acc_in, float acc_div, const int64_t *a,
                               const int64_t *b, int32_t n, int32_t n_user_rows, float grad_scale, float *loss_sum, float *loss_per_sample,
                               int32_t d, void *stream)
{
    spex::BatchLaunch L;
    L.who = who; L.g = g; L.X = X; L.acc_in = acc_in; L.acc_div = acc_div; L.a = a; L.b = b; L.n = n; L.n_user_rows = n_user_rows;
    L.grad_scale = grad_scale; L.loss_sum = loss_sum; L.loss_rows = loss_per_sample; L.d = d; L.stream = stream;
    return L;
}
static void triples(spex::BatchLaunch &L, const int64_t *neg, float weight_decay, const float *E0, int32_t *row_counts,
                    spex::BatchLaunch::Widths widths)
{
    L.bpr = true; L.c = neg; L.weight_decay = weight_decay; L.E0 = E0; L.row_counts = row_counts; L.widths = widths;
}
static void pushes(spex::BatchLaunch &L, float push_scale, float *g_out, float *G)
{
    L.push = true; L.push_scale = push_scale; L.g_out = g_out; L.G = G;
}

extern "C" int spex_lightgcn_batch_slots_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div,
                                             const int64_t *users, const int64_t *items, const float *labels, int32_t B,
                                             int32_t n_user_rows, float grad_scale, float *loss_sum, float *loss_per_sample,
                                             float *grad_slots, int32_t d, void *stream)
{
    spex::BatchLaunch L = entry("spex_lightgcn_batch_slots_f32", g, X, acc_in, acc_div, users, items, B, n_user_rows, grad_scale, loss_sum,
                                loss_per_sample, d, stream);
    L.labels = labels; L.slots = grad_slots;
    return spex::batch_launch(L);
}

extern "C" int spex_lightgcn_batch_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div,
                                       const int64_t *users, const int64_t *items, const float *labels, int32_t B,
                                       int32_t n_user_rows, float grad_scale, float push_scale, float *loss_sum, float *loss_per_sample,
                                       float *g_out, float *G, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g_out, "spex_lightgcn_batch_f32: NULL g_out");
    spex::BatchLaunch L = entry("spex_lightgcn_batch_f32", g, X, acc_in, acc_div, users, items, B, n_user_rows, grad_scale, loss_sum,
                                loss_per_sample, d, stream);
    L.labels = labels;
    pushes(L, push_scale, g_out, G);
    return spex::batch_launch(L);
}

extern "C" int spex_lightgcn_bpr_batch_slots_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div,
                                                 const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T,
                                                 int32_t n_user_rows, float grad_scale, float weight_decay, const float *E0,
                                                 int32_t *row_counts, float *loss_sum, float *loss_per_sample, float *grad_slots,
                                                 int32_t d, void *stream)
{
    spex::BatchLaunch L = entry("spex_lightgcn_bpr_batch_slots_f32", g, X, acc_in, acc_div, users, pos, T, n_user_rows, grad_scale, loss_sum,
                                loss_per_sample, d, stream);
    triples(L, neg, weight_decay, E0, row_counts, spex::BatchLaunch::kNarrow);
    L.slots = grad_slots;
    return spex::batch_launch(L);
}

extern "C" int spex_lightgcn_bpr_batch_slots_wide_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div,
                                                      const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T,
                                                      int32_t n_user_rows, float grad_scale, float weight_decay, const float *E0,
                                                      int32_t *row_counts, float *loss_sum, float *loss_per_sample, float *grad_slots,
                                                      int32_t d, void *stream)
{
    spex::BatchLaunch L = entry("spex_lightgcn_bpr_batch_slots_wide_f32", g, X, acc_in, acc_div, users, pos, T, n_user_rows, grad_scale,
                                loss_sum, loss_per_sample, d, stream);
    triples(L, neg, weight_decay, E0, row_counts, spex::BatchLaunch::kWide);
    L.slots = grad_slots;
    return spex::batch_launch(L);
}

extern "C" int spex_lightgcn_bpr_batch_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div, const int64_t *users,
                                           const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows, float grad_scale,
                                           float push_scale, float weight_decay, const float *E0, int32_t *row_counts, float *loss_sum,
                                           float *loss_per_sample, float *g_out, float *G, int32_t d, void *stream)
{
    spex::BatchLaunch L = entry("spex_lightgcn_bpr_batch_f32", g, X, acc_in, acc_div, users, pos, T, n_user_rows, grad_scale, loss_sum,
                                loss_per_sample, d, stream);
    triples(L, neg, weight_decay, E0, row_counts, spex::BatchLaunch::kNarrow);
    pushes(L, push_scale, g_out, G);
    return spex::batch_launch(L);
}

extern "C" int spex_lightgcn_bpr_batch_wide_f32(const spex_graph_t *g, const float *X, const float *acc_in, float acc_div,
                                                const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T,
                                                int32_t n_user_rows, float grad_scale, float push_scale, float weight_decay, const float *E0,
                                                int32_t *row_counts, float *loss_sum, float *loss_per_sample, float *g_out, float *G,
                                                int32_t d, void *stream)
{
    spex::BatchLaunch L = entry("spex_lightgcn_bpr_batch_wide_f32", g, X, acc_in, acc_div, users, pos, T, n_user_rows, grad_scale, loss_sum,
                                loss_per_sample, d, stream);
    triples(L, neg, weight_decay, E0, row_counts, spex::BatchLaunch::kWide);
    pushes(L, push_scale, g_out, G);
    return spex::batch_launch(L);
}

// (the four d == 64 forms with the last layer gathered from a bf16 table X16: kernels and launch in batch_bf16.hip)
extern "C" int spex_lightgcn_batch_slots_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                                  const int64_t *users, const int64_t *items, const float *labels, int32_t B,
                                                  int32_t n_user_rows, float grad_scale, float *loss_sum, float *loss_per_sample,
                                                  float *grad_slots, int32_t d, void *stream)
{
    spex::BatchLaunch L = entry("spex_lightgcn_batch_slots_bf16_f32", g, X16, acc_in, acc_div, users, items, B, n_user_rows, grad_scale,
                                loss_sum, loss_per_sample, d, stream);
    L.x_bf16 = true; L.labels = labels; L.slots = grad_slots;
    return spex::batch_launch(L);
}

extern "C" int spex_lightgcn_batch_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                            const int64_t *users, const int64_t *items, const float *labels, int32_t B, int32_t n_user_rows,
                                            float grad_scale, float push_scale, float *loss_sum, float *loss_per_sample, float *g_out,
                                            float *G, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g_out, "spex_lightgcn_batch_bf16_f32: NULL g_out");
    spex::BatchLaunch L = entry("spex_lightgcn_batch_bf16_f32", g, X16, acc_in, acc_div, users, items, B, n_user_rows, grad_scale, loss_sum,
                                loss_per_sample, d, stream);
    L.x_bf16 = true; L.labels = labels;
    pushes(L, push_scale, g_out, G);
    return spex::batch_launch(L);
}

extern "C" int spex_lightgcn_bpr_batch_slots_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                                      const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T,
                                                      int32_t n_user_rows, float grad_scale, float weight_decay, const float *E0,
                                                      int32_t *row_counts, float *loss_sum, float *loss_per_sample, float *grad_slots,
                                                      int32_t d, void *stream)
{
    spex::BatchLaunch L = entry("spex_lightgcn_bpr_batch_slots_bf16_f32", g, X16, acc_in, acc_div, users, pos, T, n_user_rows, grad_scale,
                                loss_sum, loss_per_sample, d, stream);
    triples(L, neg, weight_decay, E0, row_counts, spex::BatchLaunch::kAnyWidth);
    L.x_bf16 = true; L.slots = grad_slots;
    return spex::batch_launch(L);
}

extern "C" int spex_lightgcn_bpr_batch_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const float *acc_in, float acc_div,
                                                const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t T, int32_t n_user_rows,
                                                float grad_scale, float push_scale, float weight_decay, const float *E0, int32_t *row_counts,
                                                float *loss_sum, float *loss_per_sample, float *g_out, float *G, int32_t d, void *stream)
{
    spex::BatchLaunch L = entry("spex_lightgcn_bpr_batch_bf16_f32", g, X16, acc_in, acc_div, users, pos, T, n_user_rows, grad_scale, loss_sum,
                                loss_per_sample, d, stream);
    triples(L, neg, weight_decay, E0, row_counts, spex::BatchLaunch::kAnyWidth);
    L.x_bf16 = true;
    pushes(L, push_scale, g_out, G);
    return spex::batch_launch(L);
}

int spex::rows_train_push(const spex_graph_t *push, const float *rows_raw, const float *rows_prop, const float *att_u, const float *att_i,
                          const int64_t *pos, int64_t lo, int32_t n_local, const float *labels, int32_t B, float grad_scale, float push_scale,
                          float *loss_sum, float *g_prop, float *P, float *g_raw, float *g_att, int32_t n_att_copies, void *stream)
{
    const bool gated = rows_raw != nullptr;
    SPEX_CHECK_ARG(rows_prop && pos && labels && loss_sum && P, "rows_train_push: NULL argument");
    SPEX_CHECK_ARG(!gated || (att_u && att_i && g_raw && g_att && n_att_copies >= 1), "rows_train_push: the gated form needs att_u, att_i, g_raw, g_att");
    SPEX_CHECK_ARG(B >= 0 && n_local >= 0, "rows_train_push: B=%d n_local=%d", B, n_local);
    SPEX_CHECK_ARG(!push || push->n_cols == n_local, "rows_train_push: the push structure has %d columns for %d local rows",
                   push ? push->n_cols : 0, n_local);
    const spex::EdgeDrop drop = push ? edge_drop_of(push) : spex::EdgeDrop{nullptr, nullptr, 0, 1.0f, 0u, 0u};
    SPEX_CHECK_ARG(P != g_prop && P != g_raw && (!g_prop || g_prop != g_raw), "rows_train_push: g_prop, P and g_raw are three tables");
    if (B == 0) return SPEX_OK;
    constexpr int parts = kBatchParts, runs_per_part = kBatchRunsPerPart;
    const int32_t *rp = push && push->n_rows > 0 ? push->rowptr : nullptr;
    if (gated)
        hipLaunchKernelGGL(rows_train_push_kernel<true>, dim3((unsigned)B * parts), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, rp,
                           push ? push->col : nullptr, push ? push->val : nullptr, push ? push->n_rows : 0, rows_raw, rows_prop, att_u, att_i, pos, lo,
                           n_local, labels, B, parts, runs_per_part, grad_scale, push_scale, loss_sum, g_prop, P, g_raw, g_att, n_att_copies, drop);
    else
        hipLaunchKernelGGL(rows_train_push_kernel<false>, dim3((unsigned)B * parts), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, rp,
                           push ? push->col : nullptr, push ? push->val : nullptr, push ? push->n_rows : 0, nullptr, rows_prop, nullptr, nullptr, pos, lo,
                           n_local, labels, B, parts, runs_per_part, grad_scale, push_scale, loss_sum, g_prop, P, nullptr, nullptr, 1, drop);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_spmm_owned_rows_f32(const spex_graph_t *g, const float *X, const int64_t *pos, int32_t n, int64_t lo,
                                        const float *acc_in, const float *acc2, const float *acc3, float acc_div, const float *raw,
                                        float *out_prop, float *out_raw, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && X && out_prop && acc_in && n >= 0 && (n == 0 || pos), "spex_spmm_owned_rows_f32: NULL argument");
    SPEX_CHECK_ARG(acc_div != 0.0f && (!out_raw || raw) && (!acc3 || acc2), "spex_spmm_owned_rows_f32: acc_div == 0, out_raw without raw, or acc3 without acc2");
    if (d != kWave) {
        spex::set_error("spex_spmm_owned_rows_f32: d == 64 only (got %d)", d);
        return SPEX_ERR_UNSUPPORTED;
    }
    if (n == 0) return SPEX_OK;
    hipLaunchKernelGGL(owned_rows_kernel, dim3((unsigned)n), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->val, X, pos, lo,
                       g->n_rows, acc_in, acc2, acc3, acc_div, raw, out_prop, out_raw, edge_drop_of(g));
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}
