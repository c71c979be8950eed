// Device code shared by the batch-sized middles of the exact LightGCN steps: batch.hip (fp32 gather source) and batch_bf16.hip
// (bf16 gather source).  The pieces every such kernel is made of are written ONCE here:
//   segment_sum<MASKED, XT>     one 64-entry segment of a row, all gathers in flight (fp32 or bf16 table)
//   RowSet<K>                   the K = 1 .. 3 rows of a workgroup as scalars picked by wave-uniform selects (no indexed array: no scratch)
//   running_sum / last_layer_partials / last_layer_mean      the last layer at K rows, V columns per lane
//   PushRuns<K>                 the runs of 16 entries a wave loads kPre ahead, and the push loop over them
//   GateW / gate_forward / gate_backward / gate_att_add      the expert gate of the dual-task rec branch
// A kernel is a __global__ wrapper of its own name; the two d == 64 kernels are bodies over the element type XT of the table the
// last layer gathers from, so that each translation unit keeps kernel names of its own.  The header comment of batch.hip describes
// the workgroup's schedule.
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

// ---- a lane's V columns: a float at V == 1 (the d == 64 kernels), a vector of V floats behind WideVec at V = 2, 4
template <int V>
struct LaneVec {
    typedef typename spex::WideVec<V>::T T;
};
template <>
struct LaneVec<1> {
    typedef float T;
};
__device__ __forceinline__ float comp(float v, int) { return v; }
template <typename VT>
__device__ __forceinline__ float comp(const VT &v, int c) { return v[c]; }

// ---- one segment gather.  The 64 gathered entries of a segment in registers: one float each from an fp32 table, two to a register
//      (low / high half, as in spmm_bf16.hip) from a bf16 table (rows of 128 bytes; Xl = X16 + lane) — widening is a shift or a mask
//      and exact, so on Xw = float(X16) the bf16 form returns what the fp32 form returns on Xw, bit for bit.
template <typename XT>
struct SegRegs;
template <>
struct SegRegs<float> {
    float x[4][kChunk];
};
template <>
struct SegRegs<uint16_t> {
    h2 x[4][kChunk / 2];
};
__device__ __forceinline__ void seg_put(SegRegs<float> &r, int c, int k, float v) { r.x[c][k] = v; }
__device__ __forceinline__ float seg_get(const SegRegs<float> &r, int c, int k) { return r.x[c][k]; }
__device__ __forceinline__ void seg_put(SegRegs<uint16_t> &r, int c, int k, uint16_t v) { r.x[c][k >> 1][k & 1] = v; }
__device__ __forceinline__ float seg_get(const SegRegs<uint16_t> &r, int c, int k) { return widen_pair(r.x[c][k >> 1], k & 1); }

// One 64-entry segment [e0, e0 + cnt) of a row, all of its gathers in flight at once (one workgroup per CU here: the wave
// can afford 64 result registers, and the kernel is a latency chain — four dependent gather round trips became one).
// The fmaf chain runs in entry order exactly like the row-list kernel's.
// MASKED: the same segment under edge dropout (model.py:46-55): a kept entry's value is divided by keep_prob, a dropped entry
// contributes fmaf(0, 0, acc) = acc — exactly what spmm_chunk_kernel<.., MASKED> makes of it (dropped entries keep their place in the
// chain, so the row's sum is the masked main kernel's, bit for bit).
template <bool MASKED, typename XT>
__device__ __forceinline__ float segment_sum(const int32_t *__restrict__ col, const float *__restrict__ val, const XT *__restrict__ Xl,
                                             int e0, int cnt, int lane, float acc, const spex::EdgeDrop &dr)
{
    int my_col = 0;
    float my_val = 0.0f;
    bool dropped = false;
    if (lane < cnt) {
        my_col = col[e0 + lane];
        if (MASKED) {
            const bool kept = spex::edge_kept(dr, e0 + lane);
            my_val = kept ? val[e0 + lane] / dr.keep_prob : 0.0f;
            dropped = !kept;
        } else {
            my_val = val[e0 + lane];
        }
    }
    const unsigned long long dbits = MASKED ? __ballot(dropped) : 0ull;
    const int last_col = __builtin_amdgcn_readlane(my_col, (cnt - 1) & 63);
    if (lane >= cnt) my_col = last_col;                    // padding: value 0 on a row already being fetched
    SegRegs<XT> x;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                seg_put(x, c, k, Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane(my_col, c * kChunk + k) * kWave]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * kChunk < cnt) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                const float xv = MASKED && ((dbits >> (c * kChunk + k)) & 1ull) ? 0.0f : seg_get(x, c, k);   // a dropped entry contributes nothing
                acc = fmaf(lane_bcast(my_val, c * kChunk + k), xv, acc);
            }
        }
    }
    return acc;
}

// ---- the K rows of a workgroup (user, item | user, positive, negative | one owned row): first stored entry and length of each,
//      as scalars.  A row is picked by wave-uniform selects, never from an indexed array (at K == 3 an array lands in scratch).
__device__ __forceinline__ int sel3(int k, int a, int b, int c) { return k == 0 ? a : (k == 1 ? b : c); }
__device__ __forceinline__ float sel3f(int k, float a, float b, float c) { return k == 0 ? a : (k == 1 ? b : c); }

template <int K>
struct RowSet {
    int beg0 = 0, beg1 = 0, beg2 = 0, deg0 = 0, deg1 = 0, deg2 = 0;
    static __device__ __forceinline__ int pick(int k, int a, int b, int c) { return K == 1 ? a : (K == 2 ? (k ? b : a) : sel3(k, a, b, c)); }
    static __device__ __forceinline__ RowSet of(const int32_t *__restrict__ rowptr, int r0, int r1 = 0, int r2 = 0)
    {
        RowSet s;
        s.beg0 = rowptr[r0];
        if (K > 1) s.beg1 = rowptr[r1];
        if (K > 2) s.beg2 = rowptr[r2];
        s.deg0 = rowptr[r0 + 1] - s.beg0;
        if (K > 1) s.deg1 = rowptr[r1 + 1] - s.beg1;
        if (K > 2) s.deg2 = rowptr[r2 + 1] - s.beg2;
        return s;
    }
    __device__ __forceinline__ int beg(int k) const { return pick(k, beg0, beg1, beg2); }
    __device__ __forceinline__ int deg(int k) const { return pick(k, deg0, deg1, deg2); }
    // the push's runs of 16 entries, the forward's segments of 64, and a row's virtual waves (v = segment mod 16: the row-list kernel's)
    __device__ __forceinline__ int n_run(int k) const { return (deg(k) + 15) >> 4; }
    __device__ __forceinline__ int n_runs() const { return n_run(0) + (K > 1 ? n_run(1) : 0) + (K > 2 ? n_run(2) : 0); }
    __device__ __forceinline__ int n_seg(int k) const { return (deg(k) + kTaskEntries - 1) / kTaskEntries; }
    __device__ __forceinline__ int n_virt(int k) const { return n_seg(k) < kWgWaves ? n_seg(k) : kWgWaves; }
    // position j of the rows' jointly numbered units (n0, n1: the units of rows 0 and 1) -> its row and its number within the row
    static __device__ __forceinline__ void deal(int j, int n0, int n1, int &side, int &v)
    {
        if (K == 1) {
            side = 0;
            v = j;
        } else if (K == 2) {
            side = j >= n0;
            v = side ? j - n0 : j;
        } else {
            side = (j >= n0) + (j >= n0 + n1);
            v = j - sel3(side, 0, n0, n0 + n1);
        }
    }
};

// ---- the last layer at K rows, V columns per lane (d = 64 V).  Three calls, in this order, with whatever the kernel wants to have in
//      flight between them (the push's first runs, the gate's operands):
//   running_sum          acc_in is the running layer sum — or, when the forward layers ran in the plain form (the one-call step: no
//                        epilogue operand, no second output stream per launch), E^0 with acc2 / acc3 the later layers' tables: the sum
//                        is formed at the batch's rows only, in the same order ((E^0 + E^1) + E^2) + y as the fused epilogues form
//                        it — bit-identical.  o = the lane's first column in the row.
//   last_layer_partials  row k's 64-entry segments go to its virtual waves v = segment mod 16 as in the row-list kernel (one
//                        accumulator chain per virtual wave); the rows' virtual waves are numbered jointly and dealt to the 16
//                        waves; a virtual wave's sum is left in s_part[k][v] (column block c of the lane at [c * 64 + lane]:
//                        conflict-free).  The caller's __syncthreads follows.
//   last_layer_mean      the wave that owns row k adds the lim = n_virt(k) partial sums in segment order, adds the running sum and
//                        divides: a row of <= 1 024 entries is the spex_spmm_f32 / spex_spmm_rowlist_f32 row bit for bit, masked
//                        or not.  sink(c, s) receives the lane's V consecutive columns lane * V + c, one at a time.
template <int V>
__device__ __forceinline__ typename LaneVec<V>::T running_sum(const float *__restrict__ acc_in, const float *__restrict__ acc2,
                                                              const float *__restrict__ acc3, size_t o)
{
    typedef typename LaneVec<V>::T vec;
    vec run = *reinterpret_cast<const vec *>(acc_in + o);
    vec r2 = (vec)(0.0f), r3 = (vec)(0.0f);
    if (acc2) r2 = *reinterpret_cast<const vec *>(acc2 + o);
    if (acc3) r3 = *reinterpret_cast<const vec *>(acc3 + o);
    if (acc2) run = run + r2;
    if (acc3) run = run + r3;
    return run;
}

template <int K, int V, typename XT>
__device__ __forceinline__ void last_layer_partials(const RowSet<K> &rows, const int32_t *__restrict__ col, const float *__restrict__ val,
                                                    const XT *__restrict__ X, const spex::EdgeDrop &drop, int wave, int lane,
                                                    float (*s_part)[kWgWaves][kWave * V])
{
    typedef typename LaneVec<V>::T vec;
    const int nv0 = rows.n_virt(0), nv1 = K > 1 ? rows.n_virt(1) : 0, nv = nv0 + nv1 + (K > 2 ? rows.n_virt(2) : 0);
    const XT *__restrict__ Xl = X + lane * V;
    for (int j = wave; j < nv; j += kWgWaves) {
        int side, v;
        RowSet<K>::deal(j, nv0, nv1, side, v);
        const int s_beg = rows.beg(side), s_deg = rows.deg(side), s_nseg = rows.n_seg(side);
        vec acc = (vec)(0.0f);
        for (int sgi = v; sgi < s_nseg; sgi += kWgWaves) {
            const int left = s_deg - sgi * kTaskEntries;
            const int cnt = left < kTaskEntries ? left : kTaskEntries;
            if constexpr (V == 1) {
                if (drop.mode != 0) acc = segment_sum<true>(col, val, Xl, s_beg + sgi * kTaskEntries, cnt, lane, acc, drop);
                else acc = segment_sum<false>(col, val, Xl, s_beg + sgi * kTaskEntries, cnt, lane, acc, drop);
            } else {
                if (drop.mode != 0) acc = spex::segment_sum_wide<V, true>(col, val, Xl, s_beg + sgi * kTaskEntries, cnt, lane, acc, drop);
                else acc = spex::segment_sum_wide<V, false>(col, val, Xl, s_beg + sgi * kTaskEntries, cnt, lane, acc, drop);
            }
        }
#pragma unroll
        for (int c = 0; c < V; ++c) s_part[side][v][c * kWave + lane] = comp(acc, c);
    }
}

template <int V, class Sink>
__device__ __forceinline__ void last_layer_mean(const float (*s_row)[kWave * V], int lim, typename LaneVec<V>::T run, float acc_div, int lane,
                                                Sink sink)
{
#pragma unroll
    for (int c = 0; c < V; ++c) {
        float y = lim > 0 ? s_row[0][c * kWave + lane] : 0.0f;
        for (int w = 1; w < lim; ++w) y = y + s_row[w][c * kWave + lane];          // segment order
        float s = comp(run, c) + y;
        if (acc_div != 1.0f) s = s / acc_div;
        sink(c, s);                                                                // column lane * V + c of the row
    }
}

// ---- the push pipeline: out[col[e]] += val[e] * g over the stored entries of the workgroup's K rows (A^T g in push form walks the
//      rows of A).  The rows' runs of 16 entries are numbered jointly and dealt over (part, wave); a wave keeps kPre runs loaded
//      ahead — the first kPre before the forward, so that their round trip is off the chain.
// A wave issues one 256-byte row atomic per ~150 ns, so a sample with 600 stored entries pushes for ~6 us (38 runs over 16 waves)
// while the median sample is done in 2.4.  Only such samples are shared: part p of a sample stays if the sample has more than
// runs_per_part * p runs — the others leave before the forward (begin() returns false) — and the active parts split the runs.
template <int K>
struct PushRuns {
    int col[kPre], cnt[kPre], side[kPre];
    float val[kPre];
    int q, q_step, n_runs;       // this wave's next run, its stride (active parts x 16 waves), the rows' runs

    // push == false: no push in this launch (one part, nothing loaded).  Returns whether this part of the sample has work.
    __device__ __forceinline__ bool begin(const RowSet<K> &rows, bool push, int parts, int runs_per_part, int part, int wave)
    {
        n_runs = rows.n_runs();
        const int want = (n_runs + runs_per_part - 1) / runs_per_part;
        const int act = !push ? 1 : (want < parts ? (want < 1 ? 1 : want) : parts);
        q_step = act * kWgWaves;
        q = part * kWgWaves + wave;
        return part < act;
    }

    // runs q, q + q_step, .. of this wave: lane e < 16 holds entry e's (column, value); under edge dropout the value is the forward's
    __device__ __forceinline__ void load(const RowSet<K> &rows, const int32_t *__restrict__ t_col, const float *__restrict__ t_val,
                                         const spex::EdgeDrop &drop, int lane)
    {
        const int n_run0 = rows.n_run(0), n_run1 = K > 1 ? rows.n_run(1) : 0;
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const int qq = q + p * q_step;
            col[p] = 0;
            val[p] = 0.0f;
            cnt[p] = 0;
            side[p] = 0;
            if (qq < n_runs) {
                int sd, rr;
                RowSet<K>::deal(qq, n_run0, n_run1, sd, rr);
                const int base = rows.beg(sd) + rr * 16, left = rows.deg(sd) - rr * 16;
                side[p] = sd;
                cnt[p] = left < 16 ? left : 16;
                if (lane < cnt[p]) {
                    col[p] = t_col[base + lane];
                    val[p] = t_val[base + lane];
                    if (drop.mode != 0) val[p] = spex::edge_kept(drop, base + lane) ? val[p] / drop.keep_prob : 0.0f;   // the forward's mask
                }
            }
        }
    }

    // The push over every run of this wave into `out` (rows of 64 V floats, V 256-byte atomics per stored entry: the lane owns columns
    // lane, lane + 64, ..).  grad(side) is the gradient operand of a run of row `side`, formed where the kernel forms it.  Lane 0 of
    // every loaded run is read before the first atomic and the entry loop is a real loop (rows.hip explains why: one vmcnt for loads
    // and atomics).
    template <int V, class Grad>
    __device__ __forceinline__ void push(const RowSet<K> &rows, const int32_t *__restrict__ t_col, const float *__restrict__ t_val,
                                         const spex::EdgeDrop &drop, float *out, int lane, Grad grad)
    {
        constexpr int kRow = kWave * V;
        float *out_l = out + lane;
        for (;;) {
            int c0[kPre];
            float v0[kPre];
#pragma unroll
            for (int p = 0; p < kPre; ++p) {
                c0[p] = __builtin_amdgcn_readlane(col[p], 0);
                v0[p] = lane_bcast(val[p], 0);
            }
#pragma unroll
            for (int p = 0; p < kPre; ++p) {
                const auto gs = grad(side[p]);
                if (cnt[p] > 0) {
#pragma unroll
                    for (int c = 0; c < V; ++c) atomicAdd(out_l + (size_t)c0[p] * kRow + c * kWave, v0[p] * comp(gs, c));
                }
#pragma unroll 1
                for (int j = 1; j < cnt[p]; ++j) {
                    const int cc = __builtin_amdgcn_readlane(col[p], j);
                    const float v = lane_bcast(val[p], j);
#pragma unroll
                    for (int c = 0; c < V; ++c) atomicAdd(out_l + (size_t)cc * kRow + c * kWave, v * comp(gs, c));
                }
            }
            q += kPre * q_step;
            if (q >= n_runs) break;
            load(rows, t_col, t_val, drop, lane);
        }
    }
};

// ---- the expert gate of the dual-task rec branch (utility1/model_expert_s.py:154-168), one row per wave: softmax([raw | light] att)
//      two-way mix, as expert_gate_rows_kernel / expert_gate_rows_bwd_kernel compute it, operand for operand.
struct GateW {                  // the lane's four words of a gate matrix att [128, 2]: rows lane (raw half) and 64 + lane (light half)
    float w00 = 0.0f, w01 = 0.0f, w10 = 0.0f, w11 = 0.0f;
    __device__ __forceinline__ void load(const float *__restrict__ att, int lane)
    {
        w00 = att[2 * lane]; w01 = att[2 * lane + 1];
        w10 = att[2 * (kWave + lane)]; w11 = att[2 * (kWave + lane) + 1];
    }
};

// the gated row a_raw * a0 + s * a1; a0, a1: the two softmax weights (wave-uniform)
__device__ __forceinline__ float gate_forward(const GateW &w, float a_raw, float s, float &a0, float &a1)
{
    float z0 = fmaf(s, w.w10, fmaf(a_raw, w.w00, 0.0f)), z1 = fmaf(s, w.w11, fmaf(a_raw, w.w01, 0.0f));
    z0 = wave_sum_f32(z0);
    z1 = wave_sum_f32(z1);
    const float mx = fmaxf(z0, z1);
    const float e0 = expf(z0 - mx), e1 = expf(z1 - mx);
    a0 = e0 / (e0 + e1); a1 = e1 / (e0 + e1);
    return a_raw * a0 + s * a1;
}

// gg = d loss / d gated row  ->  d raw, d light, and d z (the gate matrices' gradients are a_raw dz, s dz: gate_att_add)
__device__ __forceinline__ void gate_backward(const GateW &w, float a_raw, float s, float a0, float a1, float gg, float &d_raw, float &d_prop,
                                              float &dz0, float &dz1)
{
    const float da0 = wave_sum_f32(gg * a_raw), da1 = wave_sum_f32(gg * s);
    const float dot = a0 * da0 + a1 * da1;
    dz0 = a0 * (da0 - dot); dz1 = a1 * (da1 - dot);
    d_raw = a0 * gg + dz0 * w.w00 + dz1 * w.w01;
    d_prop = a1 * gg + dz0 * w.w10 + dz1 * w.w11;
}

// (every sample adds to the same 512 words: 256 x 64 lane-atomics per cache line serialise in L2 — 13 us of a 25 us launch when all
//  went to ONE copy — so sample b adds into copy b mod n_att_copies and the caller sums the copies.  ga: the copy's block of this row.)
__device__ __forceinline__ void gate_att_add(float *ga, int lane, float a_raw, float s, float dz0, float dz1)
{
    atomicAdd(ga + 2 * lane, fmaf(a_raw, dz0, 0.0f));
    atomicAdd(ga + 2 * lane + 1, fmaf(a_raw, dz1, 0.0f));
    atomicAdd(ga + 2 * (kWave + lane), fmaf(s, dz0, 0.0f));
    atomicAdd(ga + 2 * (kWave + lane) + 1, fmaf(s, dz1, 0.0f));
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
    // everything whose address is known now is requested now: both rows' ranges, the label, the running sums, the push's first runs
    const RowSet<2> rows = RowSet<2>::of(rowptr, row[0], row[1]);
    const float y_lab = labels[b];
    float run = 0.0f;
    if (wave < 2) run = running_sum<1>(acc_in, acc2, acc3, (size_t)row[wave] * kWave + lane);
    PushRuns<2> runs;
    if (!runs.begin(rows, PUSH, parts, runs_per_part, part, wave)) return;
    if (PUSH) runs.load(rows, col, val, drop, lane);
    STAMP(1);
    // ---- 1. last layer at both rows
    last_layer_partials<2, 1>(rows, col, val, X, drop, wave, lane, s_part);
    STAMP(2);
    __syncthreads();
    STAMP(3);
    // ---- 2. layer mean at both rows (waves 0 and 1), the score, both gradient rows
    if (wave < 2) last_layer_mean<1>(s_part[wave], rows.n_virt(wave), run, acc_div, lane, [&](int, float s) { s_light[wave][lane] = s; });
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
    // ---- 3. push over both rows' entries (the forward's rows of the same matrix)
    STAMP(5);
    runs.template push<1>(rows, col, val, drop, G, lane, [&](int side) { return push_scale * (side ? g2[1] : g2[0]); });
    STAMP(6);
}

// The batch-sized middle of the exact BPR step (BPR differentiated through the propagation, Adam: upstream LightGCN's training
// semantics) as one launch: lightgcn_batch_kernel with THREE rows per workgroup.  d == 64 (d = 128 / 256:
// lightgcn_bpr_batch_wide_kernel, batch.hip).  Workgroup (triple t, part p), rows ru = u[t], rp = n_user_rows + pos[t], rn = n_user_rows + neg[t]:
//   1. last layer at the three rows (last_layer_partials / last_layer_mean above);
//   2. light_r = (running sum + y_r) / (L + 1);  xp = <light_u, light_p>, xn = <light_u, light_n>, z = xn - xp;
//      loss_t = softplus(z) [+ weight_decay / 2 * (|E0[ru]|^2 + |E0[rp]|^2 + |E0[rn]|^2)];  dg = sigmoid(z) * grad_scale;
//      g_u = dg (light_n - light_p), g_p = -dg light_u, g_n = dg light_u;
//   3. PUSH: G[r] += push_scale g_r, G[col[e]] += push_scale val[e] g_r over the stored entries of the three rows (PushRuns above),
//      g_out[r] += g_r where the caller wants the dense rows (G == NULL: those only, no push — the step's dense form for large T);
//      !PUSH: grad_slots[t] = g_u, [T + t] = g_p, [2 T + t] = g_n with plain stores, no float atomic.
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
    const RowSet<3> rows = RowSet<3>::of(rowptr, r0, r1, r2);
    const int my_row = sel3(wave, r0, r1, r2);             // (waves 0 .. 2 own a row each behind the forward)
    float run = 0.0f, e0v = 0.0f;
    if (wave < 3) {
        const size_t o = (size_t)my_row * kWave + lane;
        run = running_sum<1>(acc_in, acc2, acc3, o);
        if (weight_decay > 0.0f) e0v = E0[o];
    }
    const bool push = PUSH && G != nullptr;                 // (G == NULL: the dense form — gradient rows into g_out only, no push)
    PushRuns<3> runs;
    if (!runs.begin(rows, push, parts, runs_per_part, part, wave)) return;
    if (push) runs.load(rows, col, val, drop, lane);
    // ---- 1. last layer at the three rows
    last_layer_partials<3, 1>(rows, col, val, X, drop, wave, lane, s_part);
    __syncthreads();
    // ---- 2. layer mean at the three rows (waves 0 .. 2), the two scores, the three gradient rows
    if (wave < 3) {
        last_layer_mean<1>(s_part[wave], rows.n_virt(wave), run, acc_div, lane, [&](int, float s) { s_light[wave][lane] = s; });
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
    // ---- 3. push over the three rows' entries
    runs.template push<1>(rows, col, val, drop, G, lane, [&](int side) { return push_scale * sel3f(side, g3[0], g3[1], g3[2]); });
}

// ---- host side: the two launch shapes — two rows and labels, three rows and the L2 operands — over whichever kernel of either
//      translation unit.  The slots form is one workgroup per sample and has no push operands; the push form has no slots.
template <typename XT, typename KT>
inline void launch_two_rows(KT kernel, const spex::BatchLaunch &L, int parts, int runs_per_part)
{
    const spex_graph_t *g = L.g;
    hipLaunchKernelGGL(kernel, dim3((unsigned)L.n * parts), dim3(kWave * kWgWaves), 0, (hipStream_t)L.stream, g->rowptr, g->col, g->val,
                       g->n_rows, L.n_user_rows, static_cast<const XT *>(L.X), L.acc_in, L.acc_div, L.a, L.b, L.labels, parts, L.grad_scale,
                       L.push ? L.push_scale : 0.0f, L.loss_sum, L.loss_rows, L.push ? L.g_out : nullptr, L.push ? L.G : nullptr,
                       runs_per_part, L.push ? nullptr : L.slots, L.n, L.acc2, L.acc3, spex::edge_drop_of(g));
}

template <typename XT, typename KT>
inline void launch_three_rows(KT kernel, const spex::BatchLaunch &L, int parts, int runs_per_part)
{
    const spex_graph_t *g = L.g;
    hipLaunchKernelGGL(kernel, dim3((unsigned)L.n * parts), dim3(kWave * kWgWaves), 0, (hipStream_t)L.stream, g->rowptr, g->col, g->val,
                       g->n_rows, L.n_user_rows, static_cast<const XT *>(L.X), L.acc_in, L.acc_div, L.a, L.b, L.c, parts, L.grad_scale,
                       L.push ? L.push_scale : 0.0f, L.loss_sum, L.loss_rows, L.push ? L.g_out : nullptr, L.push ? L.G : nullptr,
                       runs_per_part, L.push ? nullptr : L.slots, L.n, L.acc2, L.acc3, L.weight_decay, L.E0, L.row_counts,
                       spex::edge_drop_of(g));
}

}  // namespace batchk
}  // namespace spex
