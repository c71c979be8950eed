// Device code shared by the d == 64 chunk kernels: spmm.hip (fp32 gather table) and spmm_bf16.hip (bf16 gather table).
// The kernel is written once, as chunk_body over the element type XT of the table it gathers from; spmm_chunk_kernel and
// spmm_chunk_bf16_kernel are __global__ wrappers around it, so that each translation unit keeps its kernel names, its launch
// attributes and its build flags (spmm.hip is compiled with kernel-argument preloading, spmm_bf16.hip is not).  What depends on XT:
//   * a gathered element (Gather16<XT>): a float, or half of a register that holds two bf16 entries and is widened by a shift;
//   * the outputs (ChunkSide<XT>, put / finish): Y alone, or Y and Y16 = bf16(the same fp32 value), each optional;
//   * out_div, the hub fold (FOLD) and with it the snapshot tail: fp32 only.
// Everything else — prologue, dropout decision (drop_lane / drop_stand_in: spmm_chunk_wide_kernel's too), end-of-row masks, waits, the LDS
// fold of the 65..1 024-entry rows — is one statement for both, and every product and sum is the same fp32 fmaf chain in the same order:
// on Xw = float(X16) the bf16 kernel returns what the fp32 kernel returns on Xw, bit for bit, for every row of at most 1 024 entries.
// At the end of the file, in the same manner: rowlist_dev_body, the list-driven row-list SpMM (spmm_rowlist_dev_kernel /
// spmm_rowlist_dev_bf16_kernel) — there the equality holds for every row.
#pragma once
#include "spex_common.h"

namespace spex {
namespace chunkk {

// Blocks are dealt round-robin over the 8 XCDs; remap so that each XCD walks a contiguous range of row blocks
// (neighbouring rows share the cache lines where one row's (col,val) run ends and the next begins).  Speed only.
__device__ __forceinline__ int xcd_contiguous_block(int bid, int nblk)
{
    return ((nblk & 7) == 0) ? (bid & 7) * (nblk >> 3) + (bid >> 3) : bid;
}

// Workgroups of the chunked task table's launch: whole 16-wave workgroups, a multiple of the XCD count so the remap is a bijection.
inline int64_t chunk_table_wgs(const spex_graph *g)
{
    return (((int64_t)g->n_tasks + kWgWaves - 1) / kWgWaves + 7) / 8 * 8;
}

#ifndef SPEX_EPI_NT
#define SPEX_EPI_NT 1
#endif
#if SPEX_EPI_NT
#define SPEX_EPI_LOAD(p) __builtin_nontemporal_load(p)
#else
#define SPEX_EPI_LOAD(p) (*(p))
#endif

// In-kernel fold of the rows beyond kWgRowMax entries (tag != 0; spex_common.h: hub_grp / hub_fold / hub_ticket).  tag == 0: the
// hub segments leave one partial row each and a fix-up launch adds them (the wide and bf16 kernels, and SPEX_HUB_FOLD=0).
struct HubFold {
    const int4 *grp;
    const int2 *fold;
    unsigned long long *ticket;
    uint32_t tag;
};

struct DropArgs {
    const uint32_t *chunk_eid;
    const uint8_t *keep;
    int mode;
    float keep_prob;
    uint32_t seed_lo, seed_hi;
};

inline DropArgs drop_args(const spex_graph *g)
{
    return DropArgs{g->chunk_eid, g->keep, g->mask_mode, g->keep_prob, (uint32_t)g->seed, (uint32_t)(g->seed >> 32)};
}

// Edge dropout (MASKED): lane k decides for its own entry (injected mask byte or Philox draw keyed by the entry's edge
// id, so forward / backward / every layer of a step agree); a dropped entry keeps its slot with value 0 and the
// source row of the super-chunk's first kept entry (already being fetched), so it costs no extra traffic — and its
// gathered value is REPLACED by 0 before the fmaf (a wave-uniform select per entry), so that it contributes exactly
// nothing, as in the reference, where the entry is gone from the matrix: multiplying instead would turn a stand-in row
// holding Inf / NaN (a diverged table) into 0 * Inf = NaN on a row that never referenced it.
// Two halves, because the keep rule runs under the lane's own predicate and the stand-in is a vote of the whole wave:
//   drop_lane      a lane that holds an entry (edge id, value, source row offset) decides for it; returns the offset it had, marks a dropped one
//   drop_stand_in  every lane: the entries of the super-chunk that are dropped (wave-uniform), and my_off = what the lane gathers from
__device__ __forceinline__ uint32_t drop_lane(const DropArgs &drop, uint32_t eid, float &my_val, uint32_t &my_off)
{
    bool kept;
    if (drop.mode == 1) {
        kept = drop.keep[eid] != 0;
    } else {
        const float u01 = (float)(philox_first(eid, drop.seed_lo, drop.seed_hi) >> 8) * 5.9604644775390625e-8f;
        kept = (u01 + drop.keep_prob) >= 1.0f;
    }
    my_val = kept ? my_val / drop.keep_prob : 0.0f;   // values[random_index] / keep_prob, model.py:53
    const uint32_t own_off = my_off;
    if (!kept) my_off = 0xFFFFFFFFu;
    return own_off;
}
__device__ __forceinline__ unsigned long long drop_stand_in(bool live, uint32_t own_off, uint32_t &my_off)
{
    // a dropped entry re-reads the source row of the first KEPT entry of this super-chunk (fetched anyway, so
    // it adds +0 and no traffic); if every entry was dropped each keeps its own row (value 0)
    const bool dropped = my_off == 0xFFFFFFFFu;      // (lanes past the super-chunk hold 0: neither kept nor dropped)
    const unsigned long long drop_bits = __ballot(dropped);
    const unsigned long long kept_lanes = __ballot(!dropped && live);
    const int src = kept_lanes ? (int)__builtin_ctzll(kept_lanes) : 0;
    const uint32_t stand_in = (uint32_t)__builtin_amdgcn_readlane((int)my_off, src);   // wave-uniform
    if (dropped) my_off = kept_lanes ? stand_in : own_off;
    return drop_bits;
}

// v / div for a wave-uniform divisor, as REAL branches: written `if (div != 1.0f) v = v / div;` the compiler computes the quotient
// always and selects (an fp32 division is ~11 vector instructions; two per emitted row in the backward form — 0.4 M of the launch's
// 3 M vector instructions on Epinion2, spent on divisors that are 1.0 in most launches).  A power-of-two divisor (L + 1 = 4: the
// reference's depth) is one exact multiply — x / 2^k == x * 2^-k bit for bit.  (The empty asm keeps each arm from being speculated.)
__device__ __forceinline__ float scaled(float v, float div, float inv)
{
    if (div != 1.0f) {
        if ((__float_as_uint(div) & 0x007FFFFFu) == 0u) {
            v = v * inv;
            asm volatile("" : "+v"(v));
        } else {
            v = v / div;
            asm volatile("" : "+v"(v));
        }
    }
    return v;
}

// Snapshot tail of the plain launch (the one-call BPR step's layer 1): workgroups [table_wgs, gridDim.x) run no task; they copy
// the rows of X (= E^0, the launch's gather source: already in the L2s) that the step's T triples name into the compact buffer
// out[3 T][64] — slot j: row u[j] (j < T), n_user_rows + i_pos[j - T] (T <= j < 2 T), n_user_rows + i_neg[j - 2 T] — so that
// the BPR kernel behind the propagation, which adds its updates into E^0 while other waves still read it, finds the OLD rows
// there and layer 1 needs no running-sum epilogue over the whole table.  grid == table_wgs (every other launch): no tail.
struct SnapArgs {
    const int64_t *u, *ip, *in;
    float *out;              // [ceil(3 T / 64) * 64][64]
    int64_t T;
    int32_t n_user_rows, n_item_rows;
    int32_t table_wgs;       // workgroups of the task table (the XCD remap is evaluated against this count)
};

// One wave per 64 slots: lane k resolves slot slot0 + k, then 256-byte row loads in independent batches of kChunk, each followed
// by its stores (the chunk loop's shape).  A slot of a triple the BPR kernel skips (an index out of range) never gathers: it
// re-reads row 0 and stores zeros, as do the slots beyond 3 T of the last wave (the buffer is whole waves long).
__device__ __forceinline__ void snapshot_rows(const SnapArgs &s, const float *__restrict__ X, int64_t slot0, int lane)
{
    const int64_t j = slot0 + lane;
    int my_row = -1;
    if (j < 3 * s.T) {
        const int which = j < s.T ? 0 : (j < 2 * s.T ? 1 : 2);
        const int64_t t = j - which * s.T;
        const int64_t u = s.u[t], ip = s.ip[t], in = s.in[t];
        // (one round trip for the three indices: a short-circuit chain makes the compiler load each behind the test of the one before)
        const bool ok = (int)(u >= 0) & (int)(u < s.n_user_rows) & (int)(ip >= 0) & (int)(ip < s.n_item_rows) & (int)(in >= 0) & (int)(in < s.n_item_rows);
        if (ok) my_row = which == 0 ? (int)u : s.n_user_rows + (int)(which == 1 ? ip : in);
    }
    const float *__restrict__ Xl = X + lane;
    float *__restrict__ out = s.out + (size_t)slot0 * 64 + lane;
#pragma unroll 1
    for (int b = 0; b < kWave; b += kChunk) {      // (rolled: the tail is 4 batches of code in an instantiation whose loop it must not crowd)
        float x[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            const int r = __builtin_amdgcn_readlane(my_row, b + k);
            x[k] = Xl[(size_t)(uint32_t)(r < 0 ? 0 : r) * 64];
        }
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            const int r = __builtin_amdgcn_readlane(my_row, b + k);
            __builtin_nontemporal_store(r < 0 ? 0.0f : x[k], out + (size_t)(b + k) * 64);
        }
    }
}

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned short h4 __attribute__((ext_vector_type(4)));

// A chunk's sixteen gathers, issued back to back, sit in registers of the table's type: a float each, or two bf16 entries per
// register (low / high half).  Entry u is slot u & (kPer - 1) of register u >> kShift: reg_with() returns the
// register with that slot filled, reg_value() the slot's fp32 value.  (Registers go in and out BY VALUE: with the array or a
// register handed over by reference the compiler forwards every gathered half-word to its use instead of pairing them — the bf16
// epilogue forms then take 64 VGPRs instead of 62.)
template <typename XT>
struct Gather16 {
    typedef float R;
    static constexpr int kPer = 1, kShift = 0;
};
template <>
struct Gather16<uint16_t> {
    typedef h2 R;
    static constexpr int kPer = 2, kShift = 1;
};
__device__ __forceinline__ float reg_with(const float &, int, float v) { return v; }
__device__ __forceinline__ float reg_value(float r, int) { return r; }
__device__ __forceinline__ h2 reg_with(h2 r, int k, uint16_t v) { r[k] = v; return r; }
__device__ __forceinline__ float reg_value(h2 r, int k) { return widen_pair(r, k); }

// What a launch writes beside Y and acc_out, and how.  Outputs are streamed (non-temporal): they should not evict the gather source
// from the XCD's L2.
//   fp32  Y alone — tested only where the form allows it to be absent (OPT: the running-sum form) —, and EPI 2 divides by out_div
//   bf16  Y and Y16 = bf16(the same value), round to nearest even — the next layer's gather source, written here so that no cast pass
//         runs between layers —, each optional in every form; no out_div: finish() is the identity, not a branch
template <typename XT>
struct ChunkSide {
    float out_div, out_inv;                          // (out_inv = 1 / out_div, once per wave; exact for a power of two)
};
template <>
struct ChunkSide<uint16_t> {
    uint16_t *__restrict__ Y16;
};

template <bool OPT>
__device__ __forceinline__ void put(float *__restrict__ Y, const ChunkSide<float> &, size_t o, float v)
{
    if (!OPT || Y) __builtin_nontemporal_store(v, Y + o);
}
template <bool OPT>
__device__ __forceinline__ void put(float *__restrict__ Y, const ChunkSide<float> &, size_t o, f4 v)
{
    if (!OPT || Y) __builtin_nontemporal_store(v, reinterpret_cast<f4 *>(Y + o));
}
__device__ __forceinline__ float finish(const ChunkSide<float> &s, float v) { return scaled(v, s.out_div, s.out_inv); }
__device__ __forceinline__ f4 finish(const ChunkSide<float> &s, f4 v)
{
    if (s.out_div != 1.0f) v = v / s.out_div;
    return v;
}

template <bool OPT>
__device__ __forceinline__ void put(float *__restrict__ Y, const ChunkSide<uint16_t> &s, size_t o, float v)
{
    if (Y) __builtin_nontemporal_store(v, Y + o);
    if (s.Y16) __builtin_nontemporal_store(bf16_rne(v), s.Y16 + o);
}
template <bool OPT>
__device__ __forceinline__ void put(float *__restrict__ Y, const ChunkSide<uint16_t> &s, size_t o, f4 v)
{
    if (Y) __builtin_nontemporal_store(v, reinterpret_cast<f4 *>(Y + o));
    if (s.Y16) {
        h4 hv;
#pragma unroll
        for (int q = 0; q < 4; ++q) hv[q] = bf16_rne(v[q]);
        __builtin_nontemporal_store(hv, reinterpret_cast<h4 *>(s.Y16 + o));
    }
}
__device__ __forceinline__ float finish(const ChunkSide<uint16_t> &, float v) { return v; }
__device__ __forceinline__ f4 finish(const ChunkSide<uint16_t> &, f4 v) { return v; }

// ---------------------------------------------------------------------------------------------------------------
// d == 64 kernel: 16-wave workgroups, one wave per TASK (a run of <= 4 sixteen-entry chunks, see spex_common.h),
// lane == embedding column.
//
// What was measured on MI355X on the way here (tools/gather_bench.hip, profiles/r01*):
//   * random 256-byte row gathers run at the same rate — 6.1 TB/s from HBM, 15-24 TB/s from L2 / Infinity Cache —
//     whether a row is fetched as 64 x 4 B or 16 x 16 B lanes, with 8 or 64 rows in flight per wave: the memory system,
//     not the load shape, sets the ceiling;
//   * what separates an SpMM from that ceiling is everything it issues AROUND the gathers.  The first version (one
//     wave per row, rows walked with per-entry row-boundary tests and 64-bit scalar address arithmetic) spent 15 scalar
//     + 6 vector instructions per gathered row and saturated the CU's scalar unit at a third of the gather rate;
//   * feeding the per-entry metadata through scalar loads (s_load_dwordx16) starves on scalar-cache misses as soon
//     as the matrix streams from HBM (29 ms vs 13 ms per launch on a 2^23-node graph); buffer loads with a scalar
//     offset are ~25 % slower than global loads when the source table is cache-resident.
// Hence this shape:
//   * per 64 entries the wave loads source-row index, value (and, for bin-packed tasks, output row — in the high half of the
//     source-row word where the handle packs its words, spex_common.h) with ONE coalesced vector load each — lane k holds
//     entry k — and hands them to the scalar side with v_readlane;
//   * per 16-entry chunk: 16 independent `global_load_dword` (scalar row base + lane offset; `global_load_ushort` from a bf16
//     table, whose row is 128 bytes — one L2 line where the fp32 row is two) issued back to back,
//     then 16 x { v_fmac; s_bitcmp on the chunk's end-of-row mask; branch }.  A row's epilogue operand (running layer
//     sum, or g/(L+1)) is fetched in the same batch as its last gather, so emitting a row never waits on a
//     dependent load;
//   * tasks are padded to whole chunks with value-0 entries on the task's last real source row (an L1 hit);
//   * rows of 65..1024 entries are cut into 64-entry segments that all sit in one workgroup; their sums meet in LDS
//     and are added in segment order by the row's first wave: deterministic, no atomics, no second launch.  Rows beyond
//     1024 entries (hubs) go through global scratch: their segments lead the task table in groups of 16 adjacent waves, a
//     group is summed through LDS the same way and leaves ONE partial row, and the hub's last group to arrive (a ticket in
//     memory, no waiting) adds the groups in order and runs the epilogue — inside this launch (HubFold; the wide and bf16 kernels
//     and SPEX_HUB_FOLD=0 leave one partial row per segment to a fix-up launch instead).
// The accumulation is one fmaf chain per output element in ascending column order (bit-exact vs the reference's CPU
// kernel) for every row that fits a task; segmented rows re-associate <= 16 partial sums.
//
// EPI 0: Y = y;  1: Y = y (optional), acc_out = (acc_in + y) / epi_div;  2: Y = (y + add_in / epi_div) / out_div  (Y: see ChunkSide).
// ROWIDS: a task's rows are listed per entry (bin-packed tasks) instead of being adjacent from task.z.
// FOLD: the hub fold is compiled in (fp32 only).  The unmasked instantiations always carry it (it costs their chunk loop nothing); the
// edge-dropout ones sit ~20 scalar registers higher (the Philox key schedule lives in SGPRs) and with the fold's operands live across
// the loop they schedule worse (<0, MASKED> 13.1 -> 15.7 us on Epinion2, a graph without a single hub), so a masked launch takes the
// FOLD instantiation only on a graph that HAS hubs — where it replaces a ~5 us dependent fix-up launch per product.
template <typename XT, int EPI, bool MASKED, bool ROWIDS, bool FOLD>
__device__ __forceinline__ void chunk_body(
    const uint32_t *__restrict__ chunk_off, const float *__restrict__ chunk_val, const int32_t *__restrict__ chunk_row,
    const uint32_t *__restrict__ chunk_mask, const int4 *__restrict__ task, const int n_tasks, const int xcd_contiguous,
    const int chunk_stride, const int table_wgs,
    const XT *__restrict__ X, float *__restrict__ Y, const ChunkSide<XT> side,
    const float *epi_in, float epi_div, float *acc_out,                  // may alias each other (running sum in place): no __restrict__
    float *__restrict__ partial, const DropArgs &drop, const HubFold &hf_args, const SnapArgs &snap)
{
    typedef Gather16<XT> G;
    __shared__ float s_part[kWgWaves][kWave];  // segment sums of the rows this workgroup combines
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // The unmasked plain form may carry a snapshot tail (SnapArgs): whole workgroups behind the table's, decided once, here, on
    // scalar values; they touch neither s_part nor the hub tickets.  Only these instantiations read `snap` (fp32: FOLD).
    constexpr bool kTail = EPI == 0 && !MASKED && FOLD;
    if constexpr (kTail) {
        if ((int)blockIdx.x >= table_wgs) {
            const int64_t slot0 = ((int64_t)((int)blockIdx.x - table_wgs) * kWgWaves + wave) * kWave;
            if (slot0 < 3 * snap.T) snapshot_rows(snap, X, slot0, lane);
            return;
        }
    }
    // Workgroups are sorted heaviest-first and dealt round-robin over the 8 XCDs by the dispatcher, which gives every
    // XCD the same mix of weights: right for a graph that streams from HBM (+14 % on Epinion2x538 over handing XCD 0
    // all the heavy workgroups).  A graph whose whole source table sits in cache instead prefers each XCD to walk a
    // contiguous range of workgroups (user rows and item rows of the bipartite graph then gather from different
    // halves of the table in different L2s: 76 % vs 71 % L2 hits on Epinion2).  Placement is a speed matter only.
    // (against the table's workgroups: a tail does not move them.  The fp32 kernel reads the count in FRONT of the test, as it always
    //  did; the bf16 kernel only where the remap runs — the HBM-resident tables it is for take none: read up front, +0.45 % per launch)
    constexpr bool kFront = sizeof(XT) == 4;
    const int n_wg = kFront ? (kTail ? table_wgs : (int)gridDim.x) : 0;
    const int wg = xcd_contiguous ? xcd_contiguous_block(blockIdx.x, kFront ? n_wg : (int)gridDim.x) : (int)blockIdx.x;
    const int tid = wg * kWgWaves + wave;
    if (tid >= n_tasks) return;  // whole workgroups only (n_tasks is a multiple of kWgWaves)
    // Implied positions (chunk_stride != 0, bin-packed tables: spex_common.h): task tid's chunks start at chunk tid * chunk_stride
    // whatever the task record says, so its first super-chunk's metadata — all 64 lanes, the four mask words — is requested HERE, in
    // the same round trip as the record, instead of behind it; the lanes beyond the task's chunks are cut off once the record is in (a
    // null task loads and discards: every position below n_tasks * chunk_stride chunks exists, and chunk_stride >= 4).
    const bool implied = ROWIDS && chunk_stride != 0;
    // Packed words (spex_common.h: packed_words; bin-packed tables only): the handle has no chunk_row array, an entry's word is
    // (output row << 16) | source row.  Told apart by the null pointer, a scalar test once per wave; the word is split once per lane
    // (super_chunk, in front of the dropout decision and the v_readlanes), never per gathered entry.
    // (the test is re-made from the pointer at every use, behind an empty asm: as one named value the compiler carries it across the
    //  chunk loop in an SGPR pair of its own, which costs the edge-dropout fold forms — at 100 SGPRs — their eighth wave)
    auto is_packed = [&]() __attribute__((always_inline)) {
        if (!ROWIDS) return false;
        unsigned long long p = (unsigned long long)chunk_row;
        asm volatile("" : "+s"(p));
        return p == 0ull;
    };
    const bool packed = is_packed();
    uint32_t pre_off = 0u, pre_mask = 0u, pre_eid = 0u;
    int pre_row = 0;
    float pre_val = 0.0f;
    if (implied) {
        const size_t c0 = (size_t)tid * (size_t)chunk_stride, e = c0 * kChunk + lane;
        pre_off = __builtin_nontemporal_load(chunk_off + e);
        pre_val = __builtin_nontemporal_load(chunk_val + e);
        if (!packed) pre_row = __builtin_nontemporal_load(chunk_row + e);
        if (MASKED) pre_eid = __builtin_nontemporal_load(drop.chunk_eid + e);
        pre_mask = __builtin_nontemporal_load(chunk_mask + c0 + (lane & 3));
    }
    const int4 t = task[tid];
    const int kind = t.w & 3;
    const XT *__restrict__ Xl = X + lane;
    const float *El = epi_in + lane;             // (EPI == 0: never read)
    int row = t.z;
    float acc = 0.0f;

    const float epi_inv = 1.0f / epi_div;        // (once per wave; exact for a power of two)
    auto emit = [&](int r, float y, float e) {
        const size_t o = (size_t)r * 64 + lane;
        if (EPI == 0) {
            put<false>(Y, side, o, y);
        } else if (EPI == 1) {
            const float s = scaled(e + y, epi_div, epi_inv);
            put<true>(Y, side, o, y);                         // both stores after the last use of a loaded value
            __builtin_nontemporal_store(s, acc_out + o);
        } else {
            put<false>(Y, side, o, finish(side, y + scaled(e, epi_div, epi_inv)));
        }
    };

    // Metadata of up to 4 chunks (64 entries) per vector load — lane k holds entry k — handed to the scalar side with
    // v_readlane.  (Feeding it through s_load instead starves on scalar-cache misses once the matrix streams from
    // HBM: 29 ms vs 13 ms per launch on a 2^23-node graph.)
    // A LIST of rows without stored entries (kind 3, bin-packed tables only; <= 64 rows, lane k holds the k-th row id): y = 0, the
    // epilogue still applies.  Done on the VECTOR side, four rows per instruction (16 lanes x float4 per row), sixteen rows' operands
    // in flight: taken one row at a time through the scalar emit path (load, wait, store) the list was a chain of up to 64 dependent
    // round trips — 32 us on the Weibo shape with its 2 441 empty rows, whose epilogue launches took twice as long as its plain ones —
    // and batching THAT path held sixteen row ids in SGPRs across the chunk loop (+1.5 us on Epinion2's <1> launch).
    if (ROWIDS && kind == 3) {
        const int count = t.w >> 4;
        int my_r = -1;
        if (lane < count) {
            if (packed) my_r = (int)((implied ? pre_off : chunk_off[(size_t)t.x * kChunk + lane]) >> 16);
            else my_r = implied ? pre_row : chunk_row[(size_t)t.x * kChunk + lane];
        }
        const int sub = lane & 15, grp = lane >> 4;
        const f4 zero = (f4)(0.0f);
        for (int k0 = 0; k0 < count; k0 += 16) {
            int r[4];
            f4 e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r[j] = __shfl(my_r, (k0 + 4 * j + grp) & 63, kWave);
                if (k0 + 4 * j + grp >= count) r[j] = -1;
                e[j] = zero;
                if (EPI != 0 && r[j] >= 0) e[j] = *reinterpret_cast<const f4 *>(epi_in + (size_t)r[j] * 64 + sub * 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (r[j] < 0) continue;
                const size_t o = (size_t)r[j] * 64 + sub * 4;
                if (EPI == 0) {
                    put<false>(Y, side, o, zero);
                } else if (EPI == 1) {
                    f4 sv = e[j] + zero;
                    if (epi_div != 1.0f) sv = sv / epi_div;
                    put<true>(Y, side, o, zero);
                    __builtin_nontemporal_store(sv, reinterpret_cast<f4 *>(acc_out + o));
                } else {
                    f4 ev = e[j];
                    if (epi_div != 1.0f) ev = ev / epi_div;
                    put<false>(Y, side, o, finish(side, zero + ev));
                }
            }
        }
    }
    const int n_ch = kind == 3 ? 0 : t.y;              // (kind 3: handled above)
    // One super-chunk (<= 4 chunks from chunk t.x + sc).  first: the one requested in front of the task record (implied positions) —
    // bin-packed instantiations run it as a call of its own in front of the loop, so that the requested values are not live across
    // the loop (as loop-carried values they cost the epilogue forms their 65th and 66th VGPR); a task has more than one super-chunk
    // only where the packer raised the pack capacity.
    auto super_chunk = [&](const int sc, const bool first) __attribute__((always_inline)) {
        const int nc = (n_ch - sc < 4) ? n_ch - sc : 4;  // chunks in this super-chunk (wave-uniform)
        uint32_t my_off = 0u, my_mask = 0u, own_off = 0u;
        unsigned long long drop_bits = 0ull;                 // MASKED: entries of this super-chunk that are dropped (wave-uniform)
        int my_row = 0;
        float my_val = 0.0f;
        if (lane < nc * kChunk) {
            uint32_t eid = 0u;      // (declared HERE.  In front of the block, the bin-packed forms keep the non-temporal hint on the later super-
                                    //  chunks' metadata loads, which the compiler otherwise drops: Weibo shape, plain launch +0.7 us, profiles/chunk_body)
            if (first) {
                my_off = pre_off;
                my_val = pre_val;
                my_row = pre_row;
                if (MASKED) eid = pre_eid;
            } else {
                const size_t e = (size_t)(t.x + sc) * kChunk + lane;
                my_off = __builtin_nontemporal_load(chunk_off + e);   // metadata is read once per launch
                my_val = __builtin_nontemporal_load(chunk_val + e);
                if (ROWIDS) my_row = __builtin_nontemporal_load(chunk_row + e);   // (a later super-chunk: never on a packed handle, below)
                if (MASKED) eid = __builtin_nontemporal_load(drop.chunk_eid + e);
            }
            // Packed words are split in the FIRST super-chunk only: the packer packs words only where no task has more than four
            // chunks (graph.hip: max_task_chunks, checked again at launch), so a packed handle never runs a later one, and that path
            // stays the statement it was — with the test and the split in it, the Weibo shape (tasks of 5 chunks) ran 0.4-0.9 us per
            // launch slower, packed (profiles/packed_words/any_stride_*) or not (gated_later_test_*).
            if (first && is_packed()) {      // (in front of drop_lane: 0xFFFFFFFF is a legal packed word, and its mark on a 16-bit source row)
                my_row = (int)(my_off >> 16);
                my_off &= 0xFFFFu;
            }
            if (MASKED) own_off = drop_lane(drop, eid, my_val, my_off);
        }
        if (MASKED) drop_bits = drop_stand_in(lane < nc * kChunk, own_off, my_off);
        if (first) my_mask = pre_mask;                       // (lane c < 4 holds chunk c's word; words beyond nc are not read)
        else if (lane < nc) my_mask = __builtin_nontemporal_load(chunk_mask + t.x + sc + lane);
        float ep[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u) ep[u] = 0.0f;
        for (int c = 0; c < nc; ++c) {
            const uint32_t mask = (uint32_t)__builtin_amdgcn_readlane((int)my_mask, c);
            const uint32_t dbits = MASKED ? (uint32_t)(drop_bits >> (c * kChunk)) & 0xFFFFu : 0u;
            typename G::R x[kChunk / G::kPer];
#pragma unroll
            for (int u = 0; u < kChunk; ++u)
                x[u >> G::kShift] = reg_with(x[u >> G::kShift], u & (G::kPer - 1), Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane((int)my_off, c * kChunk + u) * 64]);
            // (ep[] lives ACROSS the chunks — declared in front of the loop — and is written only where a row ends: an entry that ends
            //  no row keeps whatever the register held, which nothing reads.  Defined per chunk, every such entry cost a v_mov to
            //  zero it, and a chunk without any row end sixteen of them plus the register shuffles of the join: ~0.6 M of the
            //  1.0 M vector instructions the epilogue forms issue beyond the plain form's 2.1 M on Epinion2)
            if (EPI != 0 && mask != 0u) {
                int r = row;
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    if (mask & (1u << u)) {
                        const int rr = ROWIDS ? __builtin_amdgcn_readlane(my_row, c * kChunk + u) : r;
                        ep[u] = SPEX_EPI_LOAD(El + (size_t)rr * 64);
                        ++r;
                    }
                }
            }
            // A chunk that ends rows waits for ALL of its loads here, once.  gfx9 counts loads and stores in one vmcnt and the
            // compiler re-derives its waits at every control-flow join: without this, the wait for a row's epilogue operand
            // (loaded under the mask's branches) became `s_waitcnt vmcnt(0)` placed AFTER the previous row's stores were
            // issued, i.e. every emitted row waited out its predecessor's store round trip.
            if (EPI != 0) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0); expcnt / lgkmcnt unconstrained
            if (EPI == 0 && mask == 0u) {   // no row ends in this chunk (about every second chunk on Epinion2): sixteen fmafs, no per-entry
                                           // test (plain form only: in the epilogue forms the second copy of the loop costs the 65th VGPR)
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    const float xv = (MASKED && (dbits & (1u << u))) ? 0.0f : reg_value(x[u >> G::kShift], u & (G::kPer - 1));
                    acc = fmaf(lane_bcast(my_val, c * kChunk + u), xv, acc);
                }
                continue;
            }
#pragma unroll
            for (int u = 0; u < kChunk; ++u) {
                const float xv = (MASKED && (dbits & (1u << u))) ? 0.0f : reg_value(x[u >> G::kShift], u & (G::kPer - 1));     // a dropped entry contributes nothing
                acc = fmaf(lane_bcast(my_val, c * kChunk + u), xv, acc);
                if (mask & (1u << u)) {  // only packs of whole rows carry mask bits
                    emit(ROWIDS ? __builtin_amdgcn_readlane(my_row, c * kChunk + u) : row, acc, ep[u]);
                    acc = 0.0f;
                    ++row;
                }
            }
        }
    };
    if (ROWIDS) {
        if (n_ch > 0) {
            const int nc0 = n_ch < 4 ? n_ch : 4;
            if (!implied && lane < nc0 * kChunk) {      // the dense layout: the same values, requested behind the record
                const size_t e = (size_t)t.x * kChunk + lane;
                pre_off = __builtin_nontemporal_load(chunk_off + e);
                pre_val = __builtin_nontemporal_load(chunk_val + e);
                if (!packed) pre_row = __builtin_nontemporal_load(chunk_row + e);
                if (MASKED) pre_eid = __builtin_nontemporal_load(drop.chunk_eid + e);
                if (lane < nc0) pre_mask = __builtin_nontemporal_load(chunk_mask + t.x + lane);   // (the table ends with its last chunk)
            }
            super_chunk(0, true);
        }
        for (int sc = 4; sc < n_ch; sc += 4) super_chunk(sc, false);
    } else {
        for (int sc = 0; sc < n_ch; sc += 4) super_chunk(sc, false);
    }
    if (kind == 0 && t.y == 0 && t.z >= 0) {  // a row without stored entries: y = 0, the epilogue still applies
        float e = 0.0f;
        if (EPI != 0) e = El[(size_t)t.z * 64];
        emit(t.z, 0.0f, e);
    }
    const bool hub = FOLD && kind == 2 && hf_args.tag != 0u;
    if (kind == 2 && !hub) partial[(size_t)(t.w >> 4) * 64 + lane] = acc;  // hub segment: summed by the fix-up launch
    if (t.w & 4) {  // this workgroup combines the segments of rows with 65..1024 entries (and of hub groups) through LDS
        const bool leader = kind == 1 && (t.w & 8);
        const int slot = (t.w >> 4) & 15, nseg = (t.w >> 8) & 31;
        int4 hg = make_int4(0, 0, 0, 0);
        if (hub) hg = hf_args.grp[tid];
        const bool hub_leader = hub && hg.x != 0;
        float e = 0.0f;
        if ((leader || hub_leader) && EPI != 0) e = El[(size_t)t.z * 64];
        if (kind == 1 && !leader) s_part[slot][lane] = acc;
        if (hub && !hub_leader) s_part[wave][lane] = acc;
        __syncthreads();
        if (leader) {
            float y = acc;
            for (int sgi = 1; sgi < nseg; ++sgi) y = y + s_part[slot + sgi][lane];  // segment order: deterministic
            emit(t.z, y, e);
        }
        if (hub_leader) {
            // A hub's segments are adjacent in the table: this wave and the hg.y - 1 behind it hold consecutive segments of row t.z.
            // Their sum is ONE partial row of the hub; the hub's groups meet through memory: agent-scope store (write-through: the
            // groups may run on different XCDs), the wave's own stores acknowledged (explicit vmcnt(0)), a ticket on the hub (an arrival
            // counter, see below) and the LAST group to arrive adds the partial rows in group
            // order (whoever is last: the same order, the same bits) and runs the row's epilogue.  No fence (an agent-scope fence on
            // gfx950 writes back / invalidates the XCD's whole L2), no waiting, no second launch.
            float y = acc;
            for (int i = 1; i < hg.y; ++i) y = y + s_part[wave + i][lane];
            const int2 hf = hf_args.fold[hg.w];
            bool last = true;
            if (hf.y > 1) {
                __hip_atomic_store(partial + (size_t)hg.z * 64 + lane, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // the wave's partial-row store is ACKNOWLEDGED (sc1 write-through: visible to every XCD) before lane 0 touches the
                // ticket: an explicit s_waitcnt vmcnt(0) — a workgroup-scope release fence emits no vmcnt wait on gfx950.  One wave =
                // one instruction stream, so the wait covers all 64 lanes' stores.  tests/test_isa_folds.py asserts it in the ISA.
                __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0); expcnt / lgkmcnt unconstrained
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // (compiler ordering only)
                // The ticket is a COUNTER that is never reset: the handle zeroes it at creation and every launch that folds adds
                // exactly hf.y arrivals to it (launches on one handle are ordered: they share its scratch), so the group whose
                // increment lands on a multiple of hf.y is the launch's last — ONE read-modify-write round trip through memory on the
                // hub's tail.  (Round 3 carried a per-launch tag in the word: a load, a compare-exchange and often an add — three
                // dependent agent-scope round trips, ~2 us of the hub rows' 5.)  A replay from a captured graph adds hf.y again.
                unsigned long long arrived = 0ull;
                if (lane == 0) arrived = __hip_atomic_fetch_add(hf_args.ticket + hg.w, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull;
                const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(arrived % (unsigned long long)hf.y));
                last = lo == 0u;
                if (last) {
                    y = 0.0f;
                    const float *pr = partial + (size_t)hf.x * 64 + lane;
                    int q = 0;
                    for (; q + 8 <= hf.y; q += 8) {          // eight partial rows in flight (the kernel lives in 64 VGPRs)
                        float v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) v[u] = __hip_atomic_load(pr + (size_t)(q + u) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                        for (int u = 0; u < 8; ++u) y = y + v[u];
                    }
                    for (; q < hf.y; ++q) y = y + __hip_atomic_load(pr + (size_t)q * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (last) emit(t.z, y, e);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Row-list SpMM driven by a DEVICE list (a frontier: 10^4 .. 10^5 mostly short rows, median 13 entries): the row-list kernel's
// arithmetic in another work split.  A 16-wave workgroup takes 16 list slots per pass of a fixed grid that strides over the list (the
// count is read on the device).  Pass part 1: wave w owns slot w; a row of at most 64 entries is ONE wave task — gathered, finished
// and written by that wave.  Part 2: the longer rows of the 16 slots are cut into wave tasks of one 64-entry segment — a row beyond
// 1 024 entries into 16 tasks, task p chaining segments p, p + 16, .. as the row-list kernel's wave p does — the tasks of as many rows
// as fit kDevTasks LDS slots are dealt round-robin to the 16 waves, and each row's partial sums are added in segment order by one
// wave: the row-list kernel's summation order for every row, i.e. spex_spmm_f32's bits for rows of up to 1 024 entries.
// List entries are distinct, so acc_out may alias acc_in; rows outside the list are not written.
// Written once, as rowlist_dev_body over the element type XT of the gather table (Gather16<XT>, as chunk_body): spmm_rowlist_dev_kernel
// (spmm.hip) wraps it for a float table, spmm_rowlist_dev_bf16_kernel (spmm_bf16.hip) for a uint16_t one, whose rows are 128 bytes and
// whose elements are widened by a shift — every product and sum is the same fp32 chain in the same order.  Y16 = bf16(the register Y
// gets), bf16 wrapper only (the fp32 wrapper passes a constant NULL: the store folds away).  Outputs are plain stores: the step's next
// launch reads them back from L2.
constexpr int kDevTasks = 64;
constexpr int kDevMaxWgs = 1024;

// MASKED: the handle's edge-dropout rule per lane entry, as segment_sum<MASKED> of batch_kernels.h applies it — a kept value is
// val / keep_prob, a dropped entry keeps its place in the chain as fmaf(0, 0, acc): its gathered value is REPLACED by 0 (a ballot of
// the dropped lanes, a wave-uniform select per entry), so a source row it alone names may hold Inf.  The padding lanes count as
// dropped too: they gather the segment's last real source row, which under a mask may be such a row.
template <typename XT, bool MASKED>
__device__ __forceinline__ float rowlist_segments(const int32_t *__restrict__ col, const float *__restrict__ val, const XT *__restrict__ Xl,
                                                  int beg, int deg, int first, int nseg, int lane, float acc, const EdgeDrop &dr)
{
    typedef Gather16<XT> G;
    for (int sgi = first; sgi < nseg; sgi += kWgWaves) {
        const int e0 = beg + sgi * kTaskEntries;
        const int cnt = (deg - sgi * kTaskEntries < kTaskEntries) ? deg - sgi * kTaskEntries : kTaskEntries;
        int my_col = 0;
        float my_val = 0.0f;
        bool dropped = MASKED;                                  // (MASKED: a lane past the segment's end counts as dropped)
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
        // entries past the segment's end: value 0 on the segment's last real source row (a line already being fetched)
        const int last_col = __builtin_amdgcn_readlane(my_col, (cnt - 1) & 63);
        if (lane >= cnt) my_col = last_col;
        for (int c = 0; c * kChunk < cnt; ++c) {
            const uint32_t db = MASKED ? (uint32_t)(dbits >> (c * kChunk)) & 0xFFFFu : 0u;
            typename G::R x[kChunk / G::kPer];
#pragma unroll
            for (int u = 0; u < kChunk; ++u)
                x[u >> G::kShift] = reg_with(x[u >> G::kShift], u & (G::kPer - 1), Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane(my_col, c * kChunk + u) * 64]);
#pragma unroll
            for (int u = 0; u < kChunk; ++u) {
                const float xv = (MASKED && (db & (1u << u))) ? 0.0f : reg_value(x[u >> G::kShift], u & (G::kPer - 1));
                acc = fmaf(lane_bcast(my_val, c * kChunk + u), xv, acc);
            }
        }
    }
    return acc;
}

__device__ __forceinline__ void rowlist_dev_finish(int r, int lane, float y, float *Y, uint16_t *Y16, const float *acc_in, float *acc_out, float acc_div)
{
    const size_t o = (size_t)r * 64 + lane;
    if (Y) Y[o] = y;
    if (Y16) Y16[o] = bf16_rne(y);
    if (acc_out) {
        float s = acc_in[o] + y;
        if (acc_div != 1.0f) s = s / acc_div;
        acc_out[o] = s;
    }
}

template <typename XT, bool MASKED = false>
__device__ __forceinline__ void rowlist_dev_body(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const XT *__restrict__ X, const int32_t *__restrict__ list, const int32_t *__restrict__ count, int32_t max_count,
    int32_t n_rows, float *Y, uint16_t *Y16, const float *acc_in, float *acc_out, float acc_div,      // (acc_out may alias acc_in: unqualified)
    const EdgeDrop &dr = EdgeDrop{nullptr, nullptr, 0, 1.0f, 0u, 0u})
{
    __shared__ float s_part[kDevTasks][kWave];
    __shared__ int s_nt[kWgWaves];                 // tasks of each of the pass's 16 slots (0: no row, or a row of one segment)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = *count < max_count ? *count : max_count;
    const XT *__restrict__ Xl = X + lane;
    for (int k0 = blockIdx.x * kWgWaves; k0 < n; k0 += gridDim.x * kWgWaves) {      // workgroup-uniform
        // ---- part 1: one slot per wave
        int r = -1, beg = 0, deg = 0;
        if (k0 + wave < n) {
            r = list[k0 + wave];
            if (r < 0 || r >= n_rows) r = -1;      // never index the matrix out of range
        }
        if (r >= 0) {
            beg = rowptr[r];
            deg = rowptr[r + 1] - beg;
        }
        const int nseg = (deg + kTaskEntries - 1) / kTaskEntries;
        if (lane == 0) s_nt[wave] = nseg > 1 ? (nseg < kWgWaves ? nseg : kWgWaves) : 0;
        if (r >= 0 && nseg <= 1)
            rowlist_dev_finish(r, lane, rowlist_segments<XT, MASKED>(col, val, Xl, beg, deg, 0, nseg, lane, 0.0f, dr), Y, Y16, acc_in, acc_out, acc_div);
        __syncthreads();
        // ---- part 2: the longer rows, as many at a time as their tasks fit the LDS slots (a row has at most 16: at least 4 rows)
        for (int j0 = 0; j0 < kWgWaves;) {
            int total = 0, j1 = j0;
            while (j1 < kWgWaves && total + s_nt[j1] <= kDevTasks) total += s_nt[j1++];
            if (total > 0) {
                for (int t = wave; t < total; t += kWgWaves) {
                    int j = j0, base = 0;
                    while (t >= base + s_nt[j]) base += s_nt[j++];
                    const int rj = list[k0 + j];
                    const int bj = rowptr[rj], dj = rowptr[rj + 1] - bj;
                    s_part[t][lane] = rowlist_segments<XT, MASKED>(col, val, Xl, bj, dj, t - base, (dj + kTaskEntries - 1) / kTaskEntries, lane, 0.0f, dr);
                }
                __syncthreads();
                for (int j = j0 + wave; j < j1; j += kWgWaves) {
                    const int nt = s_nt[j];
                    if (nt == 0) continue;
                    int base = 0;
                    for (int i = j0; i < j; ++i) base += s_nt[i];
                    float y = s_part[base][lane];
                    for (int p = 1; p < nt; ++p) y = y + s_part[base + p][lane];       // segment order
                    rowlist_dev_finish(list[k0 + j], lane, y, Y, Y16, acc_in, acc_out, acc_div);
                }
                __syncthreads();                    // s_part is rewritten by the next group's tasks (workgroup-uniform: total is)
            }
            j0 = j1;
        }
        __syncthreads();                            // s_nt and s_part are rewritten by the next pass
    }
}

}  // namespace chunkk
}  // namespace spex
