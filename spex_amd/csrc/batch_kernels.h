// Device code shared by the batch-sized middles of the exact LightGCN steps: batch.hip (fp32 gather source) and batch_bf16.hip
// (bf16 gather source).  The two d == 64 kernels are written once, as bodies over the element type XT of the table
// the last layer gathers from; a kernel is a __global__ wrapper around its body, so that each translation unit keeps kernel names
// of its own.  Everything but the gather (segment_sum / segment_sum_masked, overloaded on the table's type) is the same statement
// in both.  The header comment of batch.hip describes the workgroup's schedule.
#pragma once
#include "spex_common.h"

namespace spex {
namespace batchk {

constexpr int kBatchParts = 3, kBatchRunsPerPart = 16;      // measured: see the table at the top of batch.hip

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

#ifdef SPEX_STAMPS   // debug build only (tools/batch_stamps.py): phase stamps of workgroup 0 / wave 0, wall_clock64 = 100 MHz
static __device__ unsigned long long g_stamps[16];   // (per translation unit; spex_debug_batch_stamps reads batch.hip's)
#define STAMP(k)                                                           \
    do {                                                                   \
        if (blockIdx.x == 8 && threadIdx.x == 0) g_stamps[k] = wall_clock64(); \
    } while (0)
#else
#define STAMP(k)
#endif

constexpr int kPre = 2;                      // push runs a wave loads ahead (2 x 16 waves x 16 entries = 512 entries per part)

// One 64-entry segment [e0, e0 + cnt) of a row, all of its gathers in flight at once (one workgroup per CU here: the wave
// can afford 64 result registers, and the kernel is a latency chain — four dependent gather round trips became one).
// The fmaf chain runs in entry order exactly like the row-list kernel's.
__device__ __forceinline__ float segment_sum(const int32_t *__restrict__ col, const float *__restrict__ val, const float *__restrict__ Xl,
                                             int e0, int cnt, int lane, float acc)
{
    int my_col = 0;
    float my_val = 0.0f;
    if (lane < cnt) {
        my_col = col[e0 + lane];
        my_val = val[e0 + lane];
    }
    const int last_col = __builtin_amdgcn_readlane(my_col, (cnt - 1) & 63);
    if (lane >= cnt) my_col = last_col;                    // padding: value 0 on a row already being fetched
    float x[4][kChunk];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                x[c][k] = Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane(my_col, c * kChunk + k) * kWave];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) acc = fmaf(lane_bcast(my_val, c * kChunk + k), x[c][k], acc);
        }
    }
    return acc;
}

// The same segment under edge dropout (model.py:46-55): a kept entry's value is divided by keep_prob, a dropped entry contributes
// fmaf(0, 0, acc) = acc — exactly what spmm_chunk_kernel<.., MASKED> makes of it (dropped entries keep their place in the chain, so
// the row's sum is the masked main kernel's, bit for bit).
__device__ __forceinline__ float segment_sum_masked(const int32_t *__restrict__ col, const float *__restrict__ val,
                                                    const float *__restrict__ Xl, int e0, int cnt, int lane, float acc,
                                                    const spex::EdgeDrop &dr)
{
    int my_col = 0;
    float my_val = 0.0f;
    bool dropped = false;
    if (lane < cnt) {
        my_col = col[e0 + lane];
        const bool kept = spex::edge_kept(dr, e0 + lane);
        my_val = kept ? val[e0 + lane] / dr.keep_prob : 0.0f;
        dropped = !kept;
    }
    const unsigned long long dbits = __ballot(dropped);
    const int last_col = __builtin_amdgcn_readlane(my_col, (cnt - 1) & 63);
    if (lane >= cnt) my_col = last_col;
    float x[4][kChunk];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                x[c][k] = Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane(my_col, c * kChunk + k) * kWave];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                const float xv = (dbits >> (c * kChunk + k)) & 1ull ? 0.0f : x[c][k];     // a dropped entry contributes nothing
                acc = fmaf(lane_bcast(my_val, c * kChunk + k), xv, acc);
            }
        }
    }
    return acc;
}

// ---- the same two segments gathering from a bf16 table (rows of 128 bytes; Xl = X16 + lane): two gathered entries share a register
//      (low / high half, as in spmm_bf16.hip), widening is a shift or a mask and exact, and the fmaf chain is the one above — on
//      Xw = float(X16) these return what the fp32 forms return on Xw, bit for bit.
__device__ __forceinline__ float segment_sum(const int32_t *__restrict__ col, const float *__restrict__ val, const uint16_t *__restrict__ Xl,
                                             int e0, int cnt, int lane, float acc)
{
    int my_col = 0;
    float my_val = 0.0f;
    if (lane < cnt) {
        my_col = col[e0 + lane];
        my_val = val[e0 + lane];
    }
    const int last_col = __builtin_amdgcn_readlane(my_col, (cnt - 1) & 63);
    if (lane >= cnt) my_col = last_col;                    // padding: value 0 on a row already being fetched
    h2 x[4][kChunk / 2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                x[c][k >> 1][k & 1] = Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane(my_col, c * kChunk + k) * kWave];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) acc = fmaf(lane_bcast(my_val, c * kChunk + k), widen_pair(x[c][k >> 1], k & 1), acc);
        }
    }
    return acc;
}

__device__ __forceinline__ float segment_sum_masked(const int32_t *__restrict__ col, const float *__restrict__ val,
                                                    const uint16_t *__restrict__ Xl, int e0, int cnt, int lane, float acc,
                                                    const spex::EdgeDrop &dr)
{
    int my_col = 0;
    float my_val = 0.0f;
    bool dropped = false;
    if (lane < cnt) {
        my_col = col[e0 + lane];
        const bool kept = spex::edge_kept(dr, e0 + lane);
        my_val = kept ? val[e0 + lane] / dr.keep_prob : 0.0f;
        dropped = !kept;
    }
    const unsigned long long dbits = __ballot(dropped);
    const int last_col = __builtin_amdgcn_readlane(my_col, (cnt - 1) & 63);
    if (lane >= cnt) my_col = last_col;
    h2 x[4][kChunk / 2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                x[c][k >> 1][k & 1] = Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane(my_col, c * kChunk + k) * kWave];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                const float xv = (dbits >> (c * kChunk + k)) & 1ull ? 0.0f : widen_pair(x[c][k >> 1], k & 1);   // a dropped entry contributes nothing
                acc = fmaf(lane_bcast(my_val, c * kChunk + k), xv, acc);
            }
        }
    }
    return acc;
}

// The body of lightgcn_batch_kernel<PUSH> (batch.hip) and lightgcn_batch_bf16_kernel<PUSH> (batch_bf16.hip).
template <bool PUSH, typename XT>
__device__ __forceinline__ void lightgcn_batch_body(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows,
    int n_user_rows, const XT *__restrict__ X, const float *__restrict__ acc_in, float acc_div,
    const int64_t *__restrict__ users, const int64_t *__restrict__ items, const float *__restrict__ labels, int parts,
    float grad_scale, float push_scale, float *loss_sum, float *__restrict__ loss_rows, float *g_out, float *G, int runs_per_part,
    float *__restrict__ grad_slots, int B, const float *__restrict__ acc2, const float *__restrict__ acc3, const spex::EdgeDrop drop)
{
    // (the push walks the same rows of the same matrix as the forward: t_* are aliases kept for readability)
    const int32_t *__restrict__ t_rowptr = rowptr, *__restrict__ t_col = col;
    const float *__restrict__ t_val = val;
    __shared__ float s_part[2][kWgWaves][kWave];   // [row: user, item][virtual wave of the row-list kernel][column]
    __shared__ float s_light[2][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x / parts, part = blockIdx.x % parts;
    STAMP(0);
    const int64_t u64 = users[b], i64 = items[b];
    if (u64 < 0 || u64 >= n_user_rows || i64 < 0 || i64 + n_user_rows >= n_rows) {   // workgroup-uniform: never gather out of range
        if (loss_rows && part == 0 && threadIdx.x == 0) loss_rows[b] = 0.0f;
        if (!PUSH && wave < 2) grad_slots[(size_t)(wave * B + b) * kWave + lane] = 0.0f;
        return;
    }
    const int row[2] = {(int)u64, (int)i64 + n_user_rows};
    // everything whose address is known now is requested now: both rows' ranges in both matrices, the label, the running sums
    const int beg[2] = {rowptr[row[0]], rowptr[row[1]]};
    const int deg[2] = {rowptr[row[0] + 1] - beg[0], rowptr[row[1] + 1] - beg[1]};
    const int t_beg[2] = {t_rowptr[row[0]], t_rowptr[row[1]]};
    const int t_len[2] = {t_rowptr[row[0] + 1] - t_beg[0], t_rowptr[row[1] + 1] - t_beg[1]};
    const float y_lab = labels[b];
    // acc_in is the running layer sum — or, when the forward layers ran in the plain form (the one-call step: no epilogue operand,
    // no second output stream per launch), E^0 with acc2 / acc3 the later layers' tables: the sum is formed HERE, at the batch's
    // rows only, in the same order ((E^0 + E^1) + E^2) + y as the fused epilogues form it — bit-identical
    float run = 0.0f;
    if (wave < 2) {
        const size_t o = (size_t)row[wave] * kWave + lane;
        run = acc_in[o];
        float r2 = 0.0f, r3 = 0.0f;
        if (acc2) r2 = acc2[o];
        if (acc3) r3 = acc3[o];
        if (acc2) run = run + r2;
        if (acc3) run = run + r3;
    }
    // the push's runs of 16 entries, both rows' runs numbered jointly and dealt over (part, wave); the first kPre of this wave
    // are loaded here, ahead of the forward, so that their round trip is off the chain
    const int n_run0 = (t_len[0] + 15) >> 4, n_runs = n_run0 + ((t_len[1] + 15) >> 4);
    // A wave issues one 256-byte row atomic per ~150 ns, so a sample with 600 stored entries pushes for ~6 us (38 runs over 16
    // waves) while the median sample is done in 2.4.  Only such samples are shared: part p of a sample stays if the sample has more
    // than runs_per_part * p runs — the others leave here, before the forward — and the active parts split the runs.
    const int want = (n_runs + runs_per_part - 1) / runs_per_part;
    const int act = !PUSH ? 1 : (want < parts ? (want < 1 ? 1 : want) : parts);
    if (part >= act) return;
    const int q_step = act * kWgWaves;
    int q = part * kWgWaves + wave;
    int p_col[kPre], p_cnt[kPre], p_side[kPre];
    float p_val[kPre];
    auto load_runs = [&](int q0) {
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const int qq = q0 + p * q_step;
            p_col[p] = 0;
            p_val[p] = 0.0f;
            p_cnt[p] = 0;
            p_side[p] = 0;
            if (qq < n_runs) {
                const int side = qq >= n_run0, rr = side ? qq - n_run0 : qq;
                const int base = t_beg[side] + rr * 16, left = t_len[side] - rr * 16;
                p_side[p] = side;
                p_cnt[p] = left < 16 ? left : 16;
                if (lane < p_cnt[p]) {
                    p_col[p] = t_col[base + lane];
                    p_val[p] = t_val[base + lane];
                    if (drop.mode != 0) p_val[p] = spex::edge_kept(drop, base + lane) ? p_val[p] / drop.keep_prob : 0.0f;   // the forward's mask
                }
            }
        }
    };
    if (PUSH) load_runs(q);
    STAMP(1);
    // ---- 1. last layer at both rows.  Row k's segments go to its virtual waves v = segment mod 16 as in the row-list kernel
    //         (one accumulator chain per virtual wave); the two rows' virtual waves are numbered jointly and dealt to the 16 waves.
    const int nseg[2] = {(deg[0] + kTaskEntries - 1) / kTaskEntries, (deg[1] + kTaskEntries - 1) / kTaskEntries};
    const int nv0 = nseg[0] < kWgWaves ? nseg[0] : kWgWaves, nv = nv0 + (nseg[1] < kWgWaves ? nseg[1] : kWgWaves);
    const XT *__restrict__ Xl = X + lane;
    for (int j = wave; j < nv; j += kWgWaves) {
        const int side = j >= nv0, v = side ? j - nv0 : j;
        float acc = 0.0f;
        for (int sgi = v; sgi < nseg[side]; sgi += kWgWaves) {
            const int left = deg[side] - sgi * kTaskEntries;
            if (drop.mode != 0)
                acc = segment_sum_masked(col, val, Xl, beg[side] + sgi * kTaskEntries, left < kTaskEntries ? left : kTaskEntries, lane, acc, drop);
            else
                acc = segment_sum(col, val, Xl, beg[side] + sgi * kTaskEntries, left < kTaskEntries ? left : kTaskEntries, lane, acc);
        }
        s_part[side][v][lane] = acc;
    }
    STAMP(2);
    __syncthreads();
    STAMP(3);
    // ---- 2. layer mean at both rows (waves 0 and 1), the score, both gradient rows
    if (wave < 2) {
        const int lim = nseg[wave] < kWgWaves ? nseg[wave] : kWgWaves;
        float y = lim > 0 ? s_part[wave][0][lane] : 0.0f;
        for (int w = 1; w < lim; ++w) y = y + s_part[wave][w][lane];          // segment order
        float s = run + y;
        if (acc_div != 1.0f) s = s / acc_div;
        s_light[wave][lane] = s;
    }
    __syncthreads();
    STAMP(4);
    const float lu = s_light[0][lane], li = s_light[1][lane];
    const float x = wave_sum_f32(fmaf(lu, li, 0.0f));
    const float dg = (sigmoid_f(x) - y_lab) * grad_scale;
    const float g2[2] = {dg * li, dg * lu};                                  // d loss / d light at the user row, at the item row
    if (part == 0 && wave < 2) {
        if (wave == 0 && lane == 0) {
            const float bce = fmaxf(x, 0.0f) - x * y_lab + log1pf(expf(-fabsf(x)));
            if (loss_rows) loss_rows[b] = bce;
            else atomicAdd(loss_sum, bce);
        }
        if (!PUSH) {
            grad_slots[(size_t)(wave * B + b) * kWave + lane] = g2[wave];     // per-sample rows; summed per table row in slot order later
        } else {
            if (g_out) atomicAdd(g_out + (size_t)row[wave] * kWave + lane, g2[wave]);   // dense d loss / d light_out (rows may repeat in a
                                                                                         // batch); NULL: nobody reads it (L == 3 step)
            atomicAdd(G + (size_t)row[wave] * kWave + lane, push_scale * g2[wave]);   // the `g` of (g + A^T g) / (L + 1)
        }
    }
    if (!PUSH) return;
    // ---- 3. push over both rows' entries in A^T.  Lane 0 of every loaded run is read before the first atomic and the entry
    //         loop is a real loop (rows.hip explains why: one vmcnt for loads and atomics).
    float *out_l = G + lane;
    STAMP(5);
    for (;;) {
        int c0[kPre];
        float v0[kPre];
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            c0[p] = __builtin_amdgcn_readlane(p_col[p], 0);
            v0[p] = lane_bcast(p_val[p], 0);
        }
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const float gs = push_scale * (p_side[p] ? g2[1] : g2[0]);
            if (p_cnt[p] > 0) atomicAdd(out_l + (size_t)c0[p] * kWave, v0[p] * gs);
#pragma unroll 1
            for (int j = 1; j < p_cnt[p]; ++j) {
                const int c = __builtin_amdgcn_readlane(p_col[p], j);
                const float v = lane_bcast(p_val[p], j);
                atomicAdd(out_l + (size_t)c * kWave, v * gs);
            }
        }
        q += kPre * q_step;
        if (q >= n_runs) break;
        load_runs(q);
    }
    STAMP(6);
}

// The batch-sized middle of the exact BPR step (BPR differentiated through the propagation, Adam: upstream LightGCN's training
// semantics) as one launch: lightgcn_batch_kernel with THREE rows per workgroup.  d == 64 (d = 128 / 256:
// lightgcn_bpr_batch_wide_kernel below).  Workgroup (triple t, part p), rows ru = u[t], rp = n_user_rows + pos[t], rn = n_user_rows + neg[t]:
//   1. last layer at the three rows: each row's 64-entry segments go to its virtual waves v = segment mod 16, the three rows' virtual
//      waves numbered jointly and dealt to the 16 waves, segment sums added in segment order through LDS — a row of <= 1 024 entries is
//      the spex_spmm_f32 / spex_spmm_rowlist_f32 row bit for bit, also under an edge mask;
//   2. light_r = (running sum + y_r) / (L + 1);  xp = <light_u, light_p>, xn = <light_u, light_n>, z = xn - xp;
//      loss_t = softplus(z) [+ weight_decay / 2 * (|E0[ru]|^2 + |E0[rp]|^2 + |E0[rn]|^2)];  dg = sigmoid(z) * grad_scale;
//      g_u = dg (light_n - light_p), g_p = -dg light_u, g_n = dg light_u;
//   3. PUSH: G[r] += push_scale g_r, G[col[e]] += push_scale val[e] g_r over the stored entries of the three rows (runs of 16 entries
//      numbered jointly over the rows and dealt over (part, wave), the first kPre requested before step 1), g_out[r] += g_r where the
//      caller wants the dense rows (G == NULL: those only, no push — the step's dense form for large T);  !PUSH: grad_slots[t] = g_u, [T + t] = g_p, [2 T + t] = g_n with plain stores, no float atomic.
// The L2 term's gradient weight_decay / T * E0[r] per occurrence of r is NOT formed here: the kernel counts the occurrences
// (row_counts[r] += 1, an integer atomic: order-independent) and the Adam pass, which reads E0 anyway, adds count * E0.
// A triple with any index out of range is skipped whole (loss 0, zero slots, no count, nothing gathered).
// Up to kBprBatchParts workgroups share a triple whose rows hold more than kBprBatchRunsPerPart runs per part, as in
// lightgcn_batch_kernel.  Measured on Epinion2, T = 256, L = 3 (uniformly drawn users), us per one-call step, two rounds over
// library builds (profiles/bpr_exact/parts_probe.txt): 1 part 71.8 / 71.7, 2 parts 73.0 / 73.1, 3 parts 71.8 / 71.4 (24 runs per
// part 71.3 / 71.4, 8 runs 72.4 / 72.5), 4 parts 83.3 / 82.9 — the two-row kernel's constants stay.
#ifndef SPEX_BPR_BATCH_PARTS            // (-D overrides: how those builds were made)
#define SPEX_BPR_BATCH_PARTS 3
#endif
#ifndef SPEX_BPR_BATCH_RUNS_PER_PART
#define SPEX_BPR_BATCH_RUNS_PER_PART 16
#endif
constexpr int kBprBatchParts = SPEX_BPR_BATCH_PARTS, kBprBatchRunsPerPart = SPEX_BPR_BATCH_RUNS_PER_PART;

__device__ __forceinline__ int sel3(int k, int a, int b, int c) { return k == 0 ? a : (k == 1 ? b : c); }
__device__ __forceinline__ float sel3f(int k, float a, float b, float c) { return k == 0 ? a : (k == 1 ? b : c); }

// The body of lightgcn_bpr_batch_kernel<PUSH> (batch.hip) and lightgcn_bpr_batch_bf16_kernel<PUSH> (batch_bf16.hip).
template <bool PUSH, typename XT>
__device__ __forceinline__ void lightgcn_bpr_batch_body(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows, int n_user_rows,
    const XT *__restrict__ X, const float *__restrict__ acc_in, float acc_div, const int64_t *__restrict__ users,
    const int64_t *__restrict__ pos, const int64_t *__restrict__ neg, int parts, float grad_scale, float push_scale, float *loss_sum,
    float *__restrict__ loss_rows, float *g_out, float *G, int runs_per_part, float *__restrict__ grad_slots, int T,
    const float *__restrict__ acc2, const float *__restrict__ acc3, float weight_decay, const float *__restrict__ E0,
    int32_t *row_counts, const spex::EdgeDrop drop)
{
    __shared__ float s_part[3][kWgWaves][kWave];   // [row: user, positive, negative][virtual wave of the row-list kernel][column]
    __shared__ float s_light[3][kWave];
    __shared__ float s_norm[3];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t = blockIdx.x / parts, part = blockIdx.x % parts;
    const int64_t u64 = users[t], p64 = pos[t], n64 = neg[t];
    const int64_t n_items = (int64_t)n_rows - n_user_rows;
    if (u64 < 0 || u64 >= n_user_rows || p64 < 0 || p64 >= n_items || n64 < 0 || n64 >= n_items) {   // workgroup-uniform
        if (loss_rows && part == 0 && threadIdx.x == 0) loss_rows[t] = 0.0f;
        if (!PUSH && wave < 3) grad_slots[((size_t)wave * T + t) * kWave + lane] = 0.0f;
        return;
    }
    const int r0 = (int)u64, r1 = (int)p64 + n_user_rows, r2 = (int)n64 + n_user_rows;
    const int beg0 = rowptr[r0], beg1 = rowptr[r1], beg2 = rowptr[r2];
    const int deg0 = rowptr[r0 + 1] - beg0, deg1 = rowptr[r1 + 1] - beg1, deg2 = rowptr[r2 + 1] - beg2;
    const int my_row = sel3(wave, r0, r1, r2);             // (waves 0 .. 2 own a row each behind the forward)
    // the running layer sum at the three rows, formed as lightgcn_batch_kernel forms it: ((E^0 + E^1) + E^2) + y
    float run = 0.0f, e0v = 0.0f;
    if (wave < 3) {
        const size_t o = (size_t)my_row * kWave + lane;
        run = acc_in[o];
        float q2 = 0.0f, q3 = 0.0f;
        if (acc2) q2 = acc2[o];
        if (acc3) q3 = acc3[o];
        if (weight_decay > 0.0f) e0v = E0[o];
        if (acc2) run = run + q2;
        if (acc3) run = run + q3;
    }
    // the push's runs of 16 entries, the three rows' runs numbered jointly and dealt over (part, wave)
    const int n_run0 = (deg0 + 15) >> 4, n_run1 = (deg1 + 15) >> 4, n_run2 = (deg2 + 15) >> 4, n_runs = n_run0 + n_run1 + n_run2;
    const bool push = PUSH && G != nullptr;                 // (G == NULL: the dense form — gradient rows into g_out only, no push)
    const int want = (n_runs + runs_per_part - 1) / runs_per_part;
    const int act = !push ? 1 : (want < parts ? (want < 1 ? 1 : want) : parts);
    if (part >= act) return;
    const int q_step = act * kWgWaves;
    int q = part * kWgWaves + wave;
    int p_col[kPre], p_cnt[kPre], p_side[kPre];
    float p_val[kPre];
    auto load_runs = [&](int q0) {
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const int qq = q0 + p * q_step;
            p_col[p] = 0;
            p_val[p] = 0.0f;
            p_cnt[p] = 0;
            p_side[p] = 0;
            if (qq < n_runs) {
                const int side = (qq >= n_run0) + (qq >= n_run0 + n_run1), rr = qq - sel3(side, 0, n_run0, n_run0 + n_run1);
                const int base = sel3(side, beg0, beg1, beg2) + rr * 16, left = sel3(side, deg0, deg1, deg2) - rr * 16;
                p_side[p] = side;
                p_cnt[p] = left < 16 ? left : 16;
                if (lane < p_cnt[p]) {
                    p_col[p] = col[base + lane];
                    p_val[p] = val[base + lane];
                    if (drop.mode != 0) p_val[p] = spex::edge_kept(drop, base + lane) ? p_val[p] / drop.keep_prob : 0.0f;   // the forward's mask
                }
            }
        }
    };
    if (push) load_runs(q);
    // ---- 1. last layer at the three rows
    const int nseg0 = (deg0 + kTaskEntries - 1) / kTaskEntries, nseg1 = (deg1 + kTaskEntries - 1) / kTaskEntries,
              nseg2 = (deg2 + kTaskEntries - 1) / kTaskEntries;
    const int nv0 = nseg0 < kWgWaves ? nseg0 : kWgWaves, nv1 = nseg1 < kWgWaves ? nseg1 : kWgWaves, nv2 = nseg2 < kWgWaves ? nseg2 : kWgWaves;
    const int nv = nv0 + nv1 + nv2;
    const XT *__restrict__ Xl = X + lane;
    for (int j = wave; j < nv; j += kWgWaves) {
        const int side = (j >= nv0) + (j >= nv0 + nv1), v = j - sel3(side, 0, nv0, nv0 + nv1);
        const int s_beg = sel3(side, beg0, beg1, beg2), s_deg = sel3(side, deg0, deg1, deg2), s_nseg = sel3(side, nseg0, nseg1, nseg2);
        float acc = 0.0f;
        for (int sgi = v; sgi < s_nseg; sgi += kWgWaves) {
            const int left = s_deg - sgi * kTaskEntries;
            if (drop.mode != 0)
                acc = segment_sum_masked(col, val, Xl, s_beg + sgi * kTaskEntries, left < kTaskEntries ? left : kTaskEntries, lane, acc, drop);
            else
                acc = segment_sum(col, val, Xl, s_beg + sgi * kTaskEntries, left < kTaskEntries ? left : kTaskEntries, lane, acc);
        }
        s_part[side][v][lane] = acc;
    }
    __syncthreads();
    // ---- 2. layer mean at the three rows (waves 0 .. 2), the two scores, the three gradient rows
    if (wave < 3) {
        const int lim = sel3(wave, nv0, nv1, nv2);
        float y = lim > 0 ? s_part[wave][0][lane] : 0.0f;
        for (int w = 1; w < lim; ++w) y = y + s_part[wave][w][lane];          // segment order
        float s = run + y;
        if (acc_div != 1.0f) s = s / acc_div;
        s_light[wave][lane] = s;
        if (weight_decay > 0.0f) {
            const float nrm = wave_sum_f32(e0v * e0v);
            if (lane == 0) s_norm[wave] = nrm;
        }
    }
    __syncthreads();
    const float lu = s_light[0][lane], lp = s_light[1][lane], ln = s_light[2][lane];
    const float xp = wave_sum_f32(fmaf(lu, lp, 0.0f)), xn = wave_sum_f32(fmaf(lu, ln, 0.0f));
    const float z = xn - xp;
    const float dg = sigmoid_f(z) * grad_scale;
    const float gn = dg * lu;
    const float g3[3] = {dg * (ln - lp), -gn, gn};                           // d loss / d light at the user, the positive, the negative row
    if (part == 0 && wave < 3) {
        if (wave == 0 && lane == 0) {
            float loss = fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z)));
            if (weight_decay > 0.0f) loss = loss + 0.5f * weight_decay * ((s_norm[0] + s_norm[1]) + s_norm[2]);
            if (loss_rows) loss_rows[t] = loss;
            else atomicAdd(loss_sum, loss);
        }
        if (row_counts && lane == 0) atomicAdd(row_counts + my_row, 1);       // occurrences of the row in the batch: the L2 gradient's weight
        const float gw = sel3f(wave, g3[0], g3[1], g3[2]);
        if (!PUSH) {
            grad_slots[((size_t)wave * T + t) * kWave + lane] = gw;           // per-triple rows; summed per table row in slot order later
        } else {
            if (g_out) atomicAdd(g_out + (size_t)my_row * kWave + lane, gw);
            if (push) atomicAdd(G + (size_t)my_row * kWave + lane, push_scale * gw);    // the `g` of (g + A^T g) / (L + 1)
        }
    }
    if (!push) return;
    // ---- 3. push over the three rows' entries (lightgcn_batch_kernel's loop: lane 0 of every loaded run is read before the first atomic)
    float *out_l = G + lane;
    for (;;) {
        int c0[kPre];
        float v0[kPre];
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            c0[p] = __builtin_amdgcn_readlane(p_col[p], 0);
            v0[p] = lane_bcast(p_val[p], 0);
        }
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const float gs = push_scale * sel3f(p_side[p], g3[0], g3[1], g3[2]);
            if (p_cnt[p] > 0) atomicAdd(out_l + (size_t)c0[p] * kWave, v0[p] * gs);
#pragma unroll 1
            for (int j = 1; j < p_cnt[p]; ++j) {
                const int c = __builtin_amdgcn_readlane(p_col[p], j);
                const float v = lane_bcast(p_val[p], j);
                atomicAdd(out_l + (size_t)c * kWave, v * gs);
            }
        }
        q += kPre * q_step;
        if (q >= n_runs) break;
        load_runs(q);
    }
}

}  // namespace batchk
}  // namespace spex
