// CSR x dense fp32 SpMM for CDNA4 (gfx950) — the LightGCN / NGCF propagation kernel.
//
// Replaces torch.sparse.mm(Graph, all_emb): LightGCN_SPEX/code/utility1/model.py:91, NGCF_SPEX/code/main_rec.py:76.
//
// Shape of the work: N rows, ~27 stored entries per row on Epinion2 (median 13, max 1020), each entry gathers one
// 256-byte embedding row (d = 64 fp32).  0.5 flop per byte: a gather/reduce bound by HBM (or, for the cache-resident
// named datasets, by L2 / Infinity Cache) — no MFMA, no GEMM reshaping.
//
// Two kernels share the lane mapping (lane == embedding column: one gathered row is one coalesced 256-byte wave load,
// two 128-byte lines) and the arithmetic (one fmaf chain per output element in ascending column order — bit for bit
// the order of the reference's CPU kernel):
//
//   spmm_chunk_kernel  d == 64, the tuned path: 16-wave workgroups, one wave per <= 64-entry task read from the chunked task
//                      table, long rows summed through LDS.  Its body (chunk_body) is written and described in spmm_chunk.h, which
//                      it shares with the bf16-table kernel of spmm_bf16.hip.
//   spmm_rows_kernel   any d: one wave per row (or per kSegLen-entry segment of a row with more than kLongRow entries), walking
//                      the plain CSR in column tiles of 64; segment sums go through global scratch and
//                      spmm_long_fixup_kernel adds them in segment order.  Correct everywhere, tuned nowhere.
//
// Fused epilogue (each saves a full pass over the embedding matrix per layer):
//   y += add_in / add_div            backward of the layer mean (g/(L+1) + A^T G)
//   Y = y                            next layer's input (skipped on the last layer)
//   acc_out = (acc_in + y) / acc_div running sum of layers; acc_div = L+1 on the last layer gives the mean
//
// Edge dropout (model.py:46-55) is decided per stored entry while its (col, val) pair is loaded — injected mask byte
// or Philox draw keyed by the entry's edge id — so forward, backward and all layers of a step drop the same edges.
#include <mutex>

#include "spmm_chunk.h"

using namespace spex;
using namespace spex::chunkk;

namespace {

struct SpmmParams {
    const int32_t *rowptr, *col;
    const float *val;
    const int32_t *edge_id;
    const int32_t *seg_beg, *seg_end, *long_row, *long_seg0;
    int32_t n_rows, n_seg, n_long;

    const float *X;
    float *Y;
    const float *add_in;
    float add_div;
    float out_div;  // y = (y + add_in / add_div) / out_div
    const float *acc_in;
    float *acc_out;
    float acc_div;
    float *partial;
    int32_t d;
    int mask_mode;
    const uint8_t *keep;
    float keep_prob;
    uint32_t seed_lo, seed_hi;
};

constexpr int kUnroll = 8;

__device__ __forceinline__ bool edge_kept(const SpmmParams &p, int eid)
{
    if (p.mask_mode == 1) return p.keep[eid] != 0;
    // floor(rand + keep_prob) with rand a 24-bit uniform in [0,1), as torch.rand produces (model.py:50-51)
    const float u = (float)(philox_first((uint32_t)eid, p.seed_lo, p.seed_hi) >> 8) * 5.9604644775390625e-8f;
    return (u + p.keep_prob) >= 1.0f;
}

// Accumulate entries [beg, end) of one row into acc for the column this lane owns.
//   Xl      X + (column owned by this lane)
//   ldx     row stride of X in floats
//   col_ok  false for lanes beyond d in the generic-d tile
template <bool MASKED>
__device__ __forceinline__ float accumulate_range(const SpmmParams &p, int beg, int end, int lane,
                                                  const float *__restrict__ Xl, int ldx, bool col_ok, float acc)
{
    for (int base = beg; base < end; base += kWave) {
        const int n = (end - base < kWave) ? end - base : kWave;  // wave-uniform
        int my_col = 0;
        float my_val = 0.0f;
        bool my_keep = false;
        if (lane < n) {
            my_col = p.col[base + lane];
            my_val = p.val[base + lane];
            if (MASKED) {
                const int eid = p.edge_id ? p.edge_id[base + lane] : base + lane;
                my_keep = edge_kept(p, eid);
                my_val = my_val / p.keep_prob;  // values[random_index] / keep_prob, model.py:53
            }
        }
        if (!MASKED) {
            int i = 0;
            for (; i + kUnroll <= n; i += kUnroll) {
                float x[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int c = __builtin_amdgcn_readlane(my_col, i + u);
                    x[u] = col_ok ? Xl[(size_t)c * ldx] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) acc = fmaf(lane_bcast(my_val, i + u), x[u], acc);
            }
            if (i < n) {  // ragged tail: same batch with wave-uniform predicates, loads still issue back-to-back
                float x[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    x[u] = 0.0f;
                    if (i + u < n) {
                        const int c = __builtin_amdgcn_readlane(my_col, i + u);
                        x[u] = col_ok ? Xl[(size_t)c * ldx] : 0.0f;
                    }
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u)
                    if (i + u < n) acc = fmaf(lane_bcast(my_val, i + u), x[u], acc);
            }
        } else {
            unsigned long long m = __ballot(my_keep);  // wave-uniform set of surviving entries
            while (m) {
                int idx[kUnroll];
                int cnt = 0;
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    idx[u] = 0;
                    if (m) {
                        idx[u] = __builtin_ctzll(m);
                        m &= m - 1;
                        cnt = u + 1;
                    }
                }
                float x[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    x[u] = 0.0f;
                    if (u < cnt) {
                        const int c = __builtin_amdgcn_readlane(my_col, idx[u]);
                        x[u] = col_ok ? Xl[(size_t)c * ldx] : 0.0f;
                    }
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u)
                    if (u < cnt) acc = fmaf(lane_bcast(my_val, idx[u]), x[u], acc);
            }
        }
    }
    return acc;
}

__device__ __forceinline__ void finish_row(const SpmmParams &p, int r, int c, float y)
{
    const size_t o = (size_t)r * p.d + c;
    if (p.add_in) y = y + p.add_in[o] / p.add_div;
    if (p.out_div != 1.0f) y = y / p.out_div;
    if (p.Y) p.Y[o] = y;
    if (p.acc_out) p.acc_out[o] = (p.acc_in[o] + y) / p.acc_div;
}

// Generic-d kernel: one wave per task.  Tasks [0, n_seg) are long-row segments (heaviest work first), tasks
// [n_seg, n_seg + n_rows) are rows; rows longer than kLongRow are left to their segments.
template <bool MASKED>
__global__ __launch_bounds__(kWave *kWavesPerBlock) void spmm_rows_kernel(const SpmmParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int task = xcd_contiguous_block(blockIdx.x, gridDim.x) * kWavesPerBlock + wave;
    const int d = p.d;

    if (task < p.n_seg) {
        const int beg = p.seg_beg[task], end = p.seg_end[task];
        for (int c0 = 0; c0 < d; c0 += kWave) {
            const bool ok = c0 + lane < d;
            const float y = accumulate_range<MASKED>(p, beg, end, lane, p.X + c0 + lane, d, ok, 0.0f);
            if (ok) p.partial[(size_t)task * d + c0 + lane] = y;
        }
        return;
    }
    const int r = task - p.n_seg;
    if (r >= p.n_rows) return;
    const int beg = p.rowptr[r], end = p.rowptr[r + 1];
    if (end - beg > kLongRow) return;
    for (int c0 = 0; c0 < d; c0 += kWave) {
        const bool ok = c0 + lane < d;
        const float y = accumulate_range<MASKED>(p, beg, end, lane, p.X + c0 + lane, d, ok, 0.0f);
        if (ok) finish_row(p, r, c0 + lane, y);
    }
}


// The d == 64 kernel (chunk_body, spmm_chunk.h: described there) on an fp32 gather table, with the in-kernel hub fold (FOLD).
template <int EPI, bool MASKED, bool ROWIDS, bool FOLD>
__global__ __launch_bounds__(kWave *kWgWaves) void spmm_chunk_kernel(
    // What the prologue reads comes FIRST, 14 dwords of it: this file is compiled with kernel-argument preloading (Makefile), which
    // hands a wave the leading arguments in user SGPRs — as many as fit beside the kernarg pointer, 14 — so the prologue's first
    // vector loads wait on no scalar trip at all.  (table_wgs is SnapArgs' field of the same name, out here because a struct
    // argument ends the preloaded run.)  Where the firmware does not preload, the compiler's compatibility prologue loads the same
    // registers in one trip: the form before.
    const uint32_t *__restrict__ chunk_off, const float *__restrict__ chunk_val, const int32_t *__restrict__ chunk_row,
    const uint32_t *__restrict__ chunk_mask, const int4 *__restrict__ task, const int n_tasks, const int xcd_contiguous,
    const int chunk_stride, const int table_wgs,
    const float *__restrict__ X, float *__restrict__ Y,
    const float *epi_in, float epi_div, float out_div, float *acc_out,   // may alias each other (running sum in place): no __restrict__
    float *__restrict__ partial,
    const DropArgs drop, const HubFold hf_args, const SnapArgs snap)
{
    // Every kernel argument the prologue reads, requested in ONE scalar trip: left to itself the compiler loads them where they are
    // first used — behind the tail test, behind the XCD remap, behind the bounds test: three dependent waits in front of the first
    // vector load.
    asm volatile("" ::"s"(n_tasks), "s"(xcd_contiguous), "s"(chunk_stride), "s"(table_wgs), "s"(chunk_off), "s"(chunk_val), "s"(chunk_row),
                 "s"(chunk_mask), "s"(task));
    chunk_body<float, EPI, MASKED, ROWIDS, FOLD>(chunk_off, chunk_val, chunk_row, chunk_mask, task, n_tasks, xcd_contiguous, chunk_stride,
                                                 table_wgs, X, Y, ChunkSide<float>{out_div, 1.0f / out_div},
                                                 epi_in, epi_div, acc_out, partial, drop, hf_args, snap);
}

// The same kernel for wider embeddings.
// V: consecutive embedding columns per lane — d = 64 V (128, 256; V = 1 is the d == 64 kernel above, kept as its own
// source because its inner-loop schedule is worth ~10 % there and the generic form schedules differently): a gathered
// row is one coalesced 256 V-byte wave load (dwordx2 / dwordx4 per lane).  The batch of gathers in flight shrinks with V (16 / 8 / 4 rows = 4 KB per
// wave either way) so the kernel stays inside 128 VGPRs at 16 waves per workgroup.
template <int V>
struct VecOf {
    typedef float T __attribute__((ext_vector_type(V)));
};

template <int EPI, bool MASKED, bool ROWIDS, int V>
__global__ __launch_bounds__(kWave *kWgWaves) void spmm_chunk_wide_kernel(
    const float *__restrict__ X, const uint32_t *__restrict__ chunk_off, const float *__restrict__ chunk_val,
    const uint32_t *__restrict__ chunk_mask, const int32_t *__restrict__ chunk_row, const int4 *__restrict__ task,
    int n_tasks, float *__restrict__ Y,
    const float *epi_in, float epi_div, float out_div, float *acc_out,   // may alias each other (running sum in place): no __restrict__
    float *__restrict__ partial,
    const DropArgs drop, const int xcd_contiguous)
{
    typedef typename VecOf<V>::T vec;
    constexpr int kRow = kWave * V;          // floats per embedding row
    constexpr int kBatch = kChunk / V;       // gathers issued back to back
    __shared__ float s_part[kWgWaves][kRow];  // segment sums of the rows this workgroup combines
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wg = xcd_contiguous ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;     // (placement: see chunk_body)
    const int tid = wg * kWgWaves + wave;
    if (tid >= n_tasks) return;  // whole workgroups only (n_tasks is a multiple of kWgWaves)
    const bool packed = ROWIDS && chunk_row == nullptr;   // (output row << 16) | source row in chunk_off, no chunk_row: see chunk_body
    const int4 t = task[tid];
    const int kind = t.w & 3;
    const float *__restrict__ Xl = X + lane * V;
    const float *El = (EPI ? epi_in : X) + lane * V;
    int row = t.z;
    vec acc = (vec)(0.0f);

    auto emit = [&](int r, vec y, vec e) {
        const size_t o = (size_t)r * kRow + lane * V;
        // outputs are streamed (non-temporal): they should not evict the gather source from the XCD's L2
        if (EPI == 0) {
            __builtin_nontemporal_store(y, reinterpret_cast<vec *>(Y + o));
        } else if (EPI == 1) {
            if (Y) __builtin_nontemporal_store(y, reinterpret_cast<vec *>(Y + o));
            vec s = e + y;
            if (epi_div != 1.0f) s = s / epi_div;
            __builtin_nontemporal_store(s, reinterpret_cast<vec *>(acc_out + o));
        } else {
            if (epi_div != 1.0f) e = e / epi_div;
            vec s = y + e;
            if (out_div != 1.0f) s = s / out_div;
            __builtin_nontemporal_store(s, reinterpret_cast<vec *>(Y + o));
        }
    };

    // (metadata of up to 4 chunks per vector load, handed to the scalar side with v_readlane: see chunk_body)
    const int n_ch = kind == 3 ? 0 : t.y;              // (kind 3: a list of rows without stored entries, handled after the loop)
    for (int sc = 0; sc < n_ch; sc += 4) {
        const int nc = (n_ch - sc < 4) ? n_ch - sc : 4;  // chunks in this super-chunk (wave-uniform)
        uint32_t my_off = 0u, my_mask = 0u, own_off = 0u;
        unsigned long long drop_bits = 0ull;                 // MASKED: entries of this super-chunk that are dropped (wave-uniform)
        int my_row = 0;
        float my_val = 0.0f;
        if (lane < nc * kChunk) {
            const size_t e = (size_t)(t.x + sc) * kChunk + lane;
            my_off = __builtin_nontemporal_load(chunk_off + e);   // metadata is read once per launch
            my_val = __builtin_nontemporal_load(chunk_val + e);
            if (ROWIDS && !packed) my_row = __builtin_nontemporal_load(chunk_row + e);
            uint32_t eid = 0u;
            if (MASKED) eid = __builtin_nontemporal_load(drop.chunk_eid + e);
            if (lane < nc) my_mask = __builtin_nontemporal_load(chunk_mask + t.x + sc + lane);   // (in front of the split: see chunk_body)
            if (packed) {
                my_row = (int)(my_off >> 16);
                my_off &= 0xFFFFu;
            }
            if (MASKED) own_off = drop_lane(drop, eid, my_val, my_off);
        }
        if (MASKED) drop_bits = drop_stand_in(lane < nc * kChunk, own_off, my_off);
        for (int c = 0; c < nc; ++c) {
            const uint32_t mask = (uint32_t)__builtin_amdgcn_readlane((int)my_mask, c);
            const uint32_t dbits = MASKED ? (uint32_t)(drop_bits >> (c * kChunk)) & 0xFFFFu : 0u;
#pragma unroll
            for (int u0 = 0; u0 < kChunk; u0 += kBatch) {
                vec x[kBatch], ep[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u)
                    x[u] = *reinterpret_cast<const vec *>(
                        Xl + (size_t)(uint32_t)__builtin_amdgcn_readlane((int)my_off, c * kChunk + u0 + u) * kRow);
                const uint32_t bmask = (mask >> u0) & ((1u << kBatch) - 1u);
                if (EPI != 0 && bmask != 0u) {
                    int r = row;
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) {
                        ep[u] = (vec)(0.0f);
                        if (bmask & (1u << u)) {
                            const int rr = ROWIDS ? __builtin_amdgcn_readlane(my_row, c * kChunk + u0 + u) : r;
                            ep[u] = __builtin_nontemporal_load(reinterpret_cast<const vec *>(El + (size_t)rr * kRow));
                            ++r;
                        }
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) ep[u] = (vec)(0.0f);
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    const float a = lane_bcast(my_val, c * kChunk + u0 + u);
                    const bool gone = MASKED && (dbits & (1u << (u0 + u)));          // a dropped entry contributes nothing
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] = fmaf(a, gone ? 0.0f : x[u][j], acc[j]);
                    if (bmask & (1u << u)) {  // only packs of whole rows carry mask bits
                        emit(ROWIDS ? __builtin_amdgcn_readlane(my_row, c * kChunk + u0 + u) : row, acc, ep[u]);
                        acc = (vec)(0.0f);
                        ++row;
                    }
                }
            }
        }
    }
    if (kind == 0 && t.y == 0 && t.z >= 0) {  // a row without stored entries: y = 0, the epilogue still applies
        vec e = (vec)(0.0f);
        if (EPI != 0) e = *reinterpret_cast<const vec *>(El + (size_t)t.z * kRow);
        emit(t.z, (vec)(0.0f), e);
    }
    if (ROWIDS && kind == 3) {                // a list of such rows (see the d == 64 kernel)
        const int count = t.w >> 4;
        int my_r = 0;
        if (lane < count) my_r = packed ? (int)(chunk_off[(size_t)t.x * kChunk + lane] >> 16) : chunk_row[(size_t)t.x * kChunk + lane];
        for (int k0 = 0; k0 < count; k0 += kBatch) {    // the rows' epilogue operands in flight together (see the d == 64 kernel)
            vec e[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                e[u] = (vec)(0.0f);
                if (EPI != 0 && k0 + u < count) e[u] = *reinterpret_cast<const vec *>(El + (size_t)__builtin_amdgcn_readlane(my_r, (k0 + u) & 63) * kRow);
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u)
                if (k0 + u < count) emit(__builtin_amdgcn_readlane(my_r, (k0 + u) & 63), (vec)(0.0f), e[u]);
        }
    }
    if (kind == 2) {  // hub segment: summed by the fix-up launch
#pragma unroll
        for (int j = 0; j < V; ++j) partial[(size_t)(t.w >> 4) * kRow + lane * V + j] = acc[j];
    }
    if (t.w & 4) {  // this workgroup combines the segments of rows with 65..1024 entries through LDS
        const bool leader = kind == 1 && (t.w & 8);
        const int slot = (t.w >> 4) & 15, nseg = (t.w >> 8) & 31;
        vec e = (vec)(0.0f);
        if (leader && EPI != 0) e = *reinterpret_cast<const vec *>(El + (size_t)t.z * kRow);
        if (kind == 1 && !leader) {
#pragma unroll
            for (int j = 0; j < V; ++j) s_part[slot][lane + j * kWave] = acc[j];   // column-major per lane: conflict-free
        }
        __syncthreads();
        if (leader) {
            vec y = acc;
            for (int sgi = 1; sgi < nseg; ++sgi) {  // segment order: deterministic
#pragma unroll
                for (int j = 0; j < V; ++j) y[j] = y[j] + s_part[slot + sgi][lane + j * kWave];
            }
            emit(t.z, y, e);
        }
    }
}

// Row-list SpMM (d == 64; d = 128 / 256: spmm_rowlist_wide_kernel below): y[r] = sum_e val[e] X[col[e]] for the listed rows only, with the running-sum epilogue.
// The exact training step reads the last forward layer at the batch's <= 2 B rows only; computing just those replaces
// a 15 us launch over the whole matrix by a ~6 us one.  One 16-wave workgroup per listed row: wave w takes the row's
// 64-entry segment w (w + 16, ... for rows beyond 1024 entries) straight from the CSR arrays — lane k loads entry k —
// and runs the same 16-gathers-then-16-fmaf batches; segment sums meet in LDS and are added in segment order: the
// main kernel's summation order for every row of up to 1024 entries, i.e. bit-identical results there.
// The list is two index arrays with an offset each (batch users, batch items + n_user_rows), duplicates allowed
// (the same value is stored twice).
__global__ __launch_bounds__(kWave *kWgWaves) void spmm_rowlist_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ X, const int64_t *__restrict__ idx_a, int n_a, int64_t off_a,
    const int64_t *__restrict__ idx_b, int64_t off_b, int32_t n_rows, float *__restrict__ Y,
    const float *acc_in, float *acc_out, float acc_div)   // documented NOT to alias for duplicates, but kept unqualified
{
    __shared__ float s_part[kWgWaves][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r64 = (int)blockIdx.x < n_a ? idx_a[blockIdx.x] + off_a : idx_b[blockIdx.x - n_a] + off_b;
    if (r64 < 0 || r64 >= n_rows) return;                         // workgroup-uniform: never index out of range
    const int r = (int)r64;
    const int beg = rowptr[r], deg = rowptr[r + 1] - beg;
    const int nseg = (deg + kTaskEntries - 1) / kTaskEntries;
    const float *__restrict__ Xl = X + lane;
    float acc = 0.0f;
    for (int sgi = wave; sgi < nseg; sgi += kWgWaves) {
        const int e0 = beg + sgi * kTaskEntries;
        const int cnt = (deg - sgi * kTaskEntries < kTaskEntries) ? deg - sgi * kTaskEntries : kTaskEntries;
        int my_col = 0;
        float my_val = 0.0f;
        if (lane < cnt) {
            my_col = col[e0 + lane];
            my_val = val[e0 + lane];
        }
        // entries past the segment's end: value 0 on the segment's last real source row (a line already being fetched)
        const int last_col = __builtin_amdgcn_readlane(my_col, (cnt - 1) & 63);
        if (lane >= cnt) my_col = last_col;
        for (int c = 0; c * kChunk < cnt; ++c) {
            float x[kChunk];
#pragma unroll
            for (int u = 0; u < kChunk; ++u)
                x[u] = Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane(my_col, c * kChunk + u) * 64];
#pragma unroll
            for (int u = 0; u < kChunk; ++u) acc = fmaf(lane_bcast(my_val, c * kChunk + u), x[u], acc);
        }
    }
    if (nseg > 1) {
        if (wave != 0 && wave < nseg) s_part[wave][lane] = acc;
        __syncthreads();
    }
    if (wave == 0) {
        float y = acc;
        const int lim = nseg < kWgWaves ? nseg : kWgWaves;
        for (int w = 1; w < lim; ++w) y = y + s_part[w][lane];    // segment order
        const size_t o = (size_t)r * 64 + lane;
        if (Y) Y[o] = y;
        if (acc_out) {
            float s = acc_in[o] + y;
            if (acc_div != 1.0f) s = s / acc_div;
            acc_out[o] = s;
        }
    }
}

// Row-list SpMM driven by a DEVICE list: rowlist_dev_body (spmm_chunk.h, where the work split is described) on a float table;
// spmm_bf16.hip wraps the same body for a bf16 one.
__global__ __launch_bounds__(kWave *kWgWaves) void spmm_rowlist_dev_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ X, const int32_t *__restrict__ list, const int32_t *__restrict__ count, int32_t max_count,
    int32_t n_rows, float *Y, const float *acc_in, float *acc_out, float acc_div)     // (acc_out may alias acc_in: unqualified)
{
    rowlist_dev_body<float>(rowptr, col, val, X, list, count, max_count, n_rows, Y, nullptr, acc_in, acc_out, acc_div);
}

// The same body under the handle's edge-dropout rule: per row the masked spex_spmm_f32's fmaf chain, a dropped entry in
// its place as fmaf(0, 0, acc) — the masked frontier step's forward layer L - 1 at the rows of the masked F1.  A kernel of its own name:
// spmm_rowlist_dev_kernel keeps its registers.
__global__ __launch_bounds__(kWave *kWgWaves) void spmm_rowlist_dev_masked_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ X, const int32_t *__restrict__ list, const int32_t *__restrict__ count, int32_t max_count,
    int32_t n_rows, float *Y, const float *acc_in, float *acc_out, float acc_div, const spex::EdgeDrop dr)
{
    rowlist_dev_body<float, true>(rowptr, col, val, X, list, count, max_count, n_rows, Y, nullptr, acc_in, acc_out, acc_div, dr);
}

// The row-list kernel at d = 64 V (V = 2, 4): a lane owns V consecutive columns, a segment's gathers are in flight 64 / V at a time
// (segment_sum_wide, spex_common.h), the segment sums are added in segment order — for rows of up to 1 024 entries the row
// spmm_chunk_wide_kernel produces, bit for bit.
template <int V>
__global__ __launch_bounds__(kWave *kWgWaves) void spmm_rowlist_wide_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ X, const int64_t *__restrict__ idx_a, int n_a, int64_t off_a,
    const int64_t *__restrict__ idx_b, int64_t off_b, int32_t n_rows, float *__restrict__ Y,
    const float *acc_in, float *acc_out, float acc_div)
{
    typedef typename spex::WideVec<V>::T vec;
    constexpr int kRow = kWave * V;
    __shared__ float s_part[kWgWaves][kRow];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r64 = (int)blockIdx.x < n_a ? idx_a[blockIdx.x] + off_a : idx_b[blockIdx.x - n_a] + off_b;
    if (r64 < 0 || r64 >= n_rows) return;                         // workgroup-uniform: never index out of range
    const int r = (int)r64;
    const int beg = rowptr[r], deg = rowptr[r + 1] - beg;
    const int nseg = (deg + kTaskEntries - 1) / kTaskEntries;
    const float *__restrict__ Xl = X + lane * V;
    const spex::EdgeDrop no_drop{nullptr, nullptr, 0, 1.0f, 0u, 0u};
    vec acc = (vec)(0.0f);
    for (int sgi = wave; sgi < nseg; sgi += kWgWaves) {
        const int left = deg - sgi * kTaskEntries;
        acc = spex::segment_sum_wide<V, false>(col, val, Xl, beg + sgi * kTaskEntries, left < kTaskEntries ? left : kTaskEntries, lane, acc, no_drop);
    }
    if (nseg > 1) {
        if (wave != 0 && wave < nseg) {
#pragma unroll
            for (int j = 0; j < V; ++j) s_part[wave][j * kWave + lane] = acc[j];   // column-major per lane: conflict-free
        }
        __syncthreads();
    }
    if (wave == 0) {
        vec y = acc;
        const int lim = nseg < kWgWaves ? nseg : kWgWaves;
        for (int w = 1; w < lim; ++w) {                            // segment order
#pragma unroll
            for (int j = 0; j < V; ++j) y[j] = y[j] + s_part[w][j * kWave + lane];
        }
        const size_t o = (size_t)r * kRow + lane * V;
        if (Y) *reinterpret_cast<vec *>(Y + o) = y;
        if (acc_out) {
            vec s = *reinterpret_cast<const vec *>(acc_in + o) + y;
            if (acc_div != 1.0f) s = s / acc_div;
            *reinterpret_cast<vec *>(acc_out + o) = s;
        }
    }
}

// One wave per long row: add its segment partials in order, then the shared epilogue.
__global__ __launch_bounds__(kWave *kWavesPerBlock) void spmm_long_fixup_kernel(const SpmmParams p,
                                                                               const int32_t *__restrict__ rows,
                                                                               const int32_t *__restrict__ seg_lo,
                                                                               const int32_t *__restrict__ seg_hi,
                                                                               int seg_stride, int n_list)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (i >= n_list) return;
    const int r = rows[i];
    const int s0 = seg_lo[(size_t)i * seg_stride], s1 = seg_hi[(size_t)i * seg_stride];
    for (int c = lane; c < p.d; c += kWave) {
        float y = 0.0f;
        int s = s0;
        for (; s + 32 <= s1; s += 32) {          // 32 partial rows in flight: a 6 812-entry row has 107 segments — a chain of 27
            float t[32];                         // round trips with four in flight was most of this launch's 6 us
#pragma unroll
            for (int u = 0; u < 32; ++u) t[u] = p.partial[(size_t)(s + u) * p.d + c];
#pragma unroll
            for (int u = 0; u < 32; ++u) y = y + t[u];
        }
        for (; s + 4 <= s1; s += 4) {
            float t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = p.partial[(size_t)(s + u) * p.d + c];
#pragma unroll
            for (int u = 0; u < 4; ++u) y = y + t[u];
        }
        for (; s < s1; ++s) y = y + p.partial[(size_t)s * p.d + c];
        finish_row(p, r, c, y);
    }
}

// out = in / div, float4-wide grid-stride (the mean's backward share g/(L+1), model.py:95).
__global__ __launch_bounds__(256) void div_kernel(const float *__restrict__ in, float *__restrict__ out, float div,
                                                  int64_t n4, int64_t rem)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 v = reinterpret_cast<const float4 *>(in)[i];
        v.x = v.x / div; v.y = v.y / div; v.z = v.z / div; v.w = v.w / div;
        reinterpret_cast<float4 *>(out)[i] = v;
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < rem) out[n4 * 4 + threadIdx.x] = in[n4 * 4 + threadIdx.x] / div;
}

// Pick the instantiation of the chunk kernel (epilogue form is a template argument of the caller; V = d / 64).
template <int EPI, int V>
void launch_chunk_v(bool masked, bool row_ids, dim3 grid, dim3 block, hipStream_t stream, const float *X, const spex_graph *g,
                    float *Y, const float *epi_in, float epi_div, float out_div, float *acc_out, const DropArgs &da,
                    int xcd_contig, const HubFold &hub, const SnapArgs &snap)
{
#define SPEX_D64(M, R, F)                                                                                              \
    hipLaunchKernelGGL((spmm_chunk_kernel<EPI, M, R, F>), grid, block, 0, stream, g->chunk_off, g->chunk_val, g->chunk_row,   \
                       g->chunk_mask, g->task, g->n_tasks, xcd_contig, g->chunk_stride, snap.table_wgs, X, Y, epi_in, epi_div, \
                       out_div, acc_out, g->partial, da, hub, snap)
#define SPEX_GO(M, R)                                                                                                  \
    do {                                                                                                               \
        if (V == 1 && (!M || hub.tag != 0u)) SPEX_D64(M, R, true);                                                     \
        else if (V == 1) SPEX_D64(M, R, !M);                                                                           \
        else                                                                                                           \
            hipLaunchKernelGGL((spmm_chunk_wide_kernel<EPI, M, R, (V == 1 ? 2 : V)>), grid, block, 0, stream, X,       \
                               g->chunk_off, g->chunk_val, g->chunk_mask, g->chunk_row, g->task, g->n_tasks, Y, epi_in, \
                               epi_div, out_div, acc_out, g->partial, da, xcd_contig);                                 \
    } while (0)
    if (masked) {
        if (row_ids) SPEX_GO(true, true);
        else SPEX_GO(true, false);
    } else {
        if (row_ids) SPEX_GO(false, true);
        else SPEX_GO(false, false);
    }
#undef SPEX_GO
#undef SPEX_D64
}

template <int EPI>
void launch_chunk(int d, bool masked, bool row_ids, dim3 grid, dim3 block, hipStream_t stream, const float *X,
                  const spex_graph *g, float *Y, const float *epi_in, float epi_div, float out_div, float *acc_out,
                  const DropArgs &da, int xcd_contig, const HubFold &hub, const SnapArgs &snap)
{
    if (d == 64) launch_chunk_v<EPI, 1>(masked, row_ids, grid, block, stream, X, g, Y, epi_in, epi_div, out_div, acc_out, da, xcd_contig, hub, snap);
    else if (d == 128) launch_chunk_v<EPI, 2>(masked, row_ids, grid, block, stream, X, g, Y, epi_in, epi_div, out_div, acc_out, da, xcd_contig, hub, snap);
    else launch_chunk_v<EPI, 4>(masked, row_ids, grid, block, stream, X, g, Y, epi_in, epi_div, out_div, acc_out, da, xcd_contig, hub, snap);
}

// Profiling hook: one hipEvent pair around ALL the SpMM launches of an API call (a 3-layer propagation is one bracket
// of three back-to-back launches), so the ~3 us an event pair costs on the stream is shared by the launches it
// brackets instead of being charged to each.
struct TimerBracket {
    spex_timer *tm = nullptr;
    hipStream_t stream;
    TimerBracket(const spex_graph *g, hipStream_t s) : stream(s)
    {
        spex_timer *t = g->timer;
        if (t && !t->open && t->used < (int32_t)t->start.size() && (t->seen++ % t->every) == 0) {
            if (hipEventRecord(t->start[t->used], stream) == hipSuccess) {
                tm = t;
                tm->open = true;
                tm->launches[tm->used] = 0;
            }
        }
    }
    ~TimerBracket()
    {
        if (tm) {
            (void)hipEventRecord(tm->stop[tm->used], stream);
            tm->open = false;
            tm->used++;
        }
    }
};

// snap: the plain d == 64 unmasked launch also copies the triples' rows of X into snap->out (SnapArgs; table_wgs is filled in here).
int launch_spmm(const spex_graph *g, const float *X, float *Y, const float *add_in, float add_div, const float *acc_in,
                float *acc_out, float acc_div, int32_t d, hipStream_t stream, float out_div = 1.0f, const SnapArgs *snap = nullptr)
{
    if (g->n_rows == 0) return SPEX_OK;
    SpmmParams p;
    p.rowptr = g->rowptr; p.col = g->col; p.val = g->val; p.edge_id = g->edge_id;
    p.seg_beg = g->seg_beg; p.seg_end = g->seg_end; p.long_row = g->long_row; p.long_seg0 = g->long_seg0;
    p.n_rows = g->n_rows; p.n_seg = g->n_seg; p.n_long = g->n_long;
    p.X = X; p.Y = Y; p.add_in = add_in; p.add_div = add_div; p.out_div = out_div; p.acc_in = acc_in; p.acc_out = acc_out; p.acc_div = acc_div;
    p.partial = g->partial; p.d = d;
    p.mask_mode = g->mask_mode; p.keep = g->keep; p.keep_prob = g->keep_prob;
    p.seed_lo = (uint32_t)g->seed; p.seed_hi = (uint32_t)(g->seed >> 32);

    HubFold hub{nullptr, nullptr, nullptr, 0u};
    const bool masked = g->mask_mode != 0;
    // fast path: d in {64, 128, 256}, chunked table present, and not both epilogues at once
    const bool fast = (d == 64 || d == 128 || d == 256) && g->task != nullptr && !(acc_out && add_in);
    const int per_block = fast ? kWgWaves : kWavesPerBlock;
    const int64_t tasks = fast ? (int64_t)g->n_tasks : (int64_t)g->n_seg + g->n_rows;  // waves
    int64_t blocks = (tasks + per_block - 1) / per_block;
    blocks = (blocks + 7) / 8 * 8;  // multiple of the XCD count so the remap is a bijection
    SnapArgs sa{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, (int32_t)blocks};
    int64_t tail = 0;
    if (snap) {
        SPEX_CHECK_ARG(fast && d == 64 && !masked && !acc_out && !add_in && snap->out && snap->T > 0, "launch_spmm: the snapshot tail rides on the plain d == 64 launch only");
        sa = *snap;
        sa.table_wgs = (int32_t)blocks;
        tail = (3 * snap->T + (int64_t)kWgWaves * kWave - 1) / ((int64_t)kWgWaves * kWave);
    }
    const dim3 grid((unsigned)(blocks + tail)), block(kWave * per_block), block4(kWave * kWavesPerBlock);
    spex_timer *tm = g->timer;
    if (tm && tm->open) tm->launches[tm->used]++;
    std::unique_lock<std::mutex> scratch_lock;   // (held until the launches below are queued)
    if ((fast ? g->n_hub > 0 : g->n_long > 0) || snap) {   // this launch writes the handle's scratch (the snapshot buffer is scratch too): order it behind its last user
        const int rc = order_scratch(g, stream, scratch_lock);
        if (rc) return rc;
    }
    if (fast) {
        // (rows are moved as float4 where a wave handles several rows per instruction: every table 16-byte aligned — any row of a
        //  contiguous fp32 [*, 64 V] tensor is)
        SPEX_CHECK_ARG(((((uintptr_t)X) | ((uintptr_t)Y) | ((uintptr_t)add_in) | ((uintptr_t)acc_in) | ((uintptr_t)acc_out)) & 15) == 0,
                       "spex_spmm_f32: X / Y / add_in / acc_in / acc_out must be 16-byte aligned");
        // (chunk_body splits packed words in a task's first super-chunk only and reads chunk_row in the later ones)
        SPEX_CHECK_ARG(!(g->packed_words && g->max_task_chunks > 4), "spex_spmm_f32: packed words on a table with tasks of %d chunks", g->max_task_chunks);
        const int xcd_contig = ((int64_t)g->n_cols * d * 4 <= (int64_t)16 << 20) ? 1 : 0;  // source table <= 16 MiB
        const DropArgs da = drop_args(g);
        // rows beyond kWgRowMax entries: folded inside the d == 64 launch (SPEX_HUB_FOLD=0: by the fix-up launch, as for the wide kernels)
        const char *fold_sw = g->n_hub > 0 ? getenv("SPEX_HUB_FOLD") : nullptr;      // (read per launch: the tests run both forms in one process)
        const bool fold_env = !(fold_sw && fold_sw[0] == '0');
        hub.grp = g->hub_grp; hub.fold = g->hub_fold; hub.ticket = g->hub_ticket;
        hub.tag = (d == 64 && fold_env && g->n_hub > 0 && g->hub_grp && g->hub_ticket) ? 1u : 0u;      // (on / off)
        if (acc_out) launch_chunk<1>(d, masked, g->row_ids, grid, block, stream, X, g, Y, acc_in, acc_div, 1.0f, acc_out, da, xcd_contig, hub, sa);
        else if (add_in) launch_chunk<2>(d, masked, g->row_ids, grid, block, stream, X, g, Y, add_in, add_div, out_div, nullptr, da, xcd_contig, hub, sa);
        else launch_chunk<0>(d, masked, g->row_ids, grid, block, stream, X, g, Y, nullptr, 1.0f, 1.0f, nullptr, da, xcd_contig, hub, sa);
    } else if (masked) {
        hipLaunchKernelGGL((spmm_rows_kernel<true>), grid, block, 0, stream, p);
    } else {
        hipLaunchKernelGGL((spmm_rows_kernel<false>), grid, block, 0, stream, p);
    }
    if (fast) {
        if (g->n_hub > 0 && hub.tag == 0u) {  // only rows longer than kWgRowMax go through global scratch on the fast path
            const dim3 fgrid((unsigned)((g->n_hub + kWavesPerBlock - 1) / kWavesPerBlock));
            hipLaunchKernelGGL(spmm_long_fixup_kernel, fgrid, block4, 0, stream, p, g->hub_row, g->hub_seg0, g->hub_seg0 + 1, 2,
                               g->n_hub);
        }
    } else if (g->n_long > 0) {
        const dim3 fgrid((unsigned)((g->n_long + kWavesPerBlock - 1) / kWavesPerBlock));
        hipLaunchKernelGGL(spmm_long_fixup_kernel, fgrid, block4, 0, stream, p, g->long_row, g->long_seg0, g->long_seg0 + 1, 1,
                           g->n_long);
    }
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

}  // namespace

int spex::order_scratch(const spex_graph_t *g, hipStream_t stream, std::unique_lock<std::mutex> &lock)
{
    spex_graph *gm = const_cast<spex_graph *>(g);
    lock = std::unique_lock<std::mutex>(gm->scratch_mu);
    if (gm->scratch_used && gm->scratch_stream != stream) {
        if (!gm->scratch_ev) SPEX_HIP(hipEventCreateWithFlags(&gm->scratch_ev, hipEventDisableTiming));
        SPEX_HIP(hipEventRecord(gm->scratch_ev, gm->scratch_stream));
        SPEX_HIP(hipStreamWaitEvent(stream, gm->scratch_ev, 0));
    }
    gm->scratch_stream = stream;
    gm->scratch_used = true;
    return SPEX_OK;
}

int spex::ensure_partial(spex_graph_t *g, int32_t d)
{
    const int64_t need = (int64_t)g->n_seg * d;
    if (need <= g->partial_cap) return SPEX_OK;
    // Only reached for d > 64 on a graph with long rows, on the first call at that d (allocates: do it once outside
    // any stream capture): the handle is created with its scratch sized for d == 64.
    SPEX_HIP(hipDeviceSynchronize());
    if (g->partial) SPEX_HIP(hipFree(g->partial));
    g->partial = nullptr;
    SPEX_HIP(hipMalloc((void **)&g->partial, (size_t)need * sizeof(float)));
    g->partial_cap = need;
    return SPEX_OK;
}

extern "C" int spex_spmm_f32(const spex_graph_t *g, const float *X, float *Y, const float *add_in, float add_div,
                             const float *acc_in, float *acc_out, float acc_div, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && X, "spex_spmm_f32: NULL graph or X");
    SPEX_CHECK_ARG(d >= 1, "spex_spmm_f32: d = %d", d);
    SPEX_CHECK_ARG(Y || acc_out, "spex_spmm_f32: neither Y nor acc_out given");
    SPEX_CHECK_ARG(!acc_out || acc_in, "spex_spmm_f32: acc_out needs acc_in");
    SPEX_CHECK_ARG(X != Y && X != acc_out, "spex_spmm_f32: X must not alias an output");
    SPEX_CHECK_ARG(!add_in || add_div != 0.0f, "spex_spmm_f32: add_div == 0");
    SPEX_CHECK_ARG(!acc_out || acc_div != 0.0f, "spex_spmm_f32: acc_div == 0");
    int rc = ensure_partial(const_cast<spex_graph *>(g), d);
    if (rc) return rc;
    TimerBracket bracket(g, (hipStream_t)stream);
    return launch_spmm(g, X, Y, add_in, add_div, acc_in, acc_out, acc_div, d, (hipStream_t)stream);
}

extern "C" int spex_spmm_rowlist_f32(const spex_graph_t *g, const float *X, const int64_t *idx_a, int32_t n_a, int64_t off_a,
                                     const int64_t *idx_b, int32_t n_b, int64_t off_b, float *Y, const float *acc_in,
                                     float *acc_out, float acc_div, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && X, "spex_spmm_rowlist_f32: NULL graph or X");
    SPEX_CHECK_ARG(n_a >= 0 && n_b >= 0 && (n_a == 0 || idx_a) && (n_b == 0 || idx_b), "spex_spmm_rowlist_f32: bad row lists");
    SPEX_CHECK_ARG(Y || acc_out, "spex_spmm_rowlist_f32: neither Y nor acc_out given");
    SPEX_CHECK_ARG(!acc_out || (acc_in && acc_div != 0.0f), "spex_spmm_rowlist_f32: acc_out needs acc_in and acc_div != 0");
    SPEX_CHECK_ARG(X != Y && X != acc_out, "spex_spmm_rowlist_f32: X must not alias an output");
    if ((d != 64 && d != 128 && d != 256) || g->mask_mode != 0) {
        spex::set_error("spex_spmm_rowlist_f32: d = 64, 128 or 256 without edge dropout only (d = %d, mask mode %d): use spex_spmm_f32", d,
                        g->mask_mode);
        return SPEX_ERR_UNSUPPORTED;
    }
    SPEX_CHECK_ARG(d == 64 || ((((uintptr_t)X) | ((uintptr_t)Y) | ((uintptr_t)acc_in) | ((uintptr_t)acc_out)) & 15) == 0,
                   "spex_spmm_rowlist_f32: X / Y / acc_in / acc_out must be 16-byte aligned at d > 64");
    if (n_a + n_b == 0 || g->n_rows == 0) return SPEX_OK;
#define SPEX_GO(KERNEL)                                                                                                             \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)(n_a + n_b)), dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->val, \
                       X, idx_a, n_a, off_a, idx_b, off_b, g->n_rows, Y, acc_in, acc_out, acc_div)
    if (d == 64) SPEX_GO(spmm_rowlist_kernel);
    else if (d == 128) SPEX_GO(spmm_rowlist_wide_kernel<2>);
    else SPEX_GO(spmm_rowlist_wide_kernel<4>);
#undef SPEX_GO
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

// spex_spmm_rowlist_f32 for a device list (spex_unique_rows_i32 / spex_frontier_rows_i32): rows list[0 .. min(*count, max_count)).
extern "C" int spex_spmm_rowlist_dev_f32(const spex_graph_t *g, const float *X, const int32_t *list, const int32_t *count, int32_t max_count,
                                         float *Y, const float *acc_in, float *acc_out, float acc_div, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && X && list && count && max_count >= 0, "spex_spmm_rowlist_dev_f32: NULL graph, X, list or count, or max_count < 0");
    SPEX_CHECK_ARG(Y || acc_out, "spex_spmm_rowlist_dev_f32: neither Y nor acc_out given");
    SPEX_CHECK_ARG(!acc_out || (acc_in && acc_div != 0.0f), "spex_spmm_rowlist_dev_f32: acc_out needs acc_in and acc_div != 0");
    SPEX_CHECK_ARG(X != Y && X != acc_out, "spex_spmm_rowlist_dev_f32: X must not alias an output");
    if (d != 64) {
        spex::set_error("spex_spmm_rowlist_dev_f32: d == 64 only (got %d)", d);
        return SPEX_ERR_UNSUPPORTED;
    }
    if (max_count == 0 || g->n_rows == 0) return SPEX_OK;
    const int64_t wgs = ((int64_t)max_count + kWgWaves - 1) / kWgWaves;
    if (g->mask_mode != 0)      // the handle's edge-dropout rule per entry: a kernel of its own (spmm_rowlist_dev_masked_kernel)
        hipLaunchKernelGGL(spmm_rowlist_dev_masked_kernel, dim3((unsigned)(wgs < kDevMaxWgs ? wgs : kDevMaxWgs)), dim3(kWave * kWgWaves), 0,
                           (hipStream_t)stream, g->rowptr, g->col, g->val, X, list, count, max_count, g->n_rows, Y, acc_in, acc_out, acc_div,
                           spex::edge_drop_of(g));
    else
        hipLaunchKernelGGL(spmm_rowlist_dev_kernel, dim3((unsigned)(wgs < kDevMaxWgs ? wgs : kDevMaxWgs)), dim3(kWave * kWgWaves), 0,
                           (hipStream_t)stream, g->rowptr, g->col, g->val, X, list, count, max_count, g->n_rows, Y, acc_in, acc_out, acc_div);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_propagate_f32(const spex_graph_t *g, const float *E0, float *mean_out, float *layers_out, float *ws,
                                  int32_t L, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && E0 && mean_out, "spex_propagate_f32: NULL argument");
    SPEX_CHECK_ARG(g->n_rows == g->n_cols, "spex_propagate_f32: needs a square graph (%d x %d); use spex_spmm_f32 per layer for a row block", g->n_rows, g->n_cols);
    SPEX_CHECK_ARG(L >= 0 && d >= 1, "spex_propagate_f32: L = %d, d = %d", L, d);
    SPEX_CHECK_ARG(layers_out || ws || L <= 1, "spex_propagate_f32: needs ws or layers_out");
    SPEX_CHECK_ARG(E0 != mean_out, "spex_propagate_f32: mean_out must not alias E0");
    int rc = ensure_partial(const_cast<spex_graph *>(g), d);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t sz = (size_t)g->n_rows * d;
    if (L == 0) {
        SPEX_HIP(hipMemcpyAsync(mean_out, E0, sz * sizeof(float), hipMemcpyDeviceToDevice, s));
        return SPEX_OK;
    }
    const float *cur = E0;
    TimerBracket bracket(g, s);
    for (int32_t l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        float *nxt = layers_out ? layers_out + (size_t)l * sz : (last ? nullptr : ws + (size_t)(l & 1) * sz);
        rc = launch_spmm(g, cur, nxt, nullptr, 1.0f, l == 0 ? E0 : mean_out, mean_out, last ? (float)(L + 1) : 1.0f, d, s);
        if (rc) return rc;
        cur = nxt;
    }
    return SPEX_OK;
}

namespace {

// The handle's snapshot buffer, grown on demand like `partial` (allocates: the first call at a batch size, outside any stream capture).
int ensure_snap(spex_graph *g, int64_t floats)
{
    if (floats <= g->snap_cap) return SPEX_OK;
    SPEX_HIP(hipDeviceSynchronize());
    if (g->snap) SPEX_HIP(hipFree(g->snap));
    g->snap = nullptr;
    g->snap_cap = 0;
    SPEX_HIP(hipMalloc((void **)&g->snap, (size_t)floats * sizeof(float)));
    g->snap_cap = floats;
    return SPEX_OK;
}

// Which schedule a one-call BPR step of T triples takes on this graph — decided from the graph and T only.  The snapshot tail adds
// ceil(3 T / 1024) workgroups to the layer-1 launch; a launch that fits ONE dispatch round (<= 512 workgroups: two per CU) must still
// fit it with the tail, else the step keeps the running-sum form on layer 1.  (SPEX_STEP_SNAPSHOT=0 / 1 forces either schedule where
// both are possible: the tests and the A/B timings run both in one process.)
constexpr int64_t kOneRoundWgs = 512;
constexpr int64_t kSnapMaxTriples = (int64_t)1 << 18;     // 192 MiB of snapshot rows; beyond it the grouped BPR form is the caller's anyway
bool step_takes_snapshot(const spex_graph *g, int32_t d, int64_t T)
{
    if (d != 64 || g->task == nullptr || g->mask_mode != 0 || g->n_rows == 0 || T <= 0 || T > kSnapMaxTriples) return false;
    const char *sw = getenv("SPEX_STEP_SNAPSHOT");
    if (sw && sw[0] == '0') return false;
    if (sw && sw[0] == '1') return true;
    const int64_t table = chunk_table_wgs(g), tail = (3 * T + (int64_t)kWgWaves * kWave - 1) / ((int64_t)kWgWaves * kWave);
    return !(table <= kOneRoundWgs && table + tail > kOneRoundWgs);
}

// Whether a one-call BPR step leaves its LAST layer to the BPR launch (bpr_fused_last_kernel, score.hip: layer L gathered at the
// triples' <= 3 T slot rows from the layer-(L-1) table, inside the BPR launch) — decided from the graph, L and T only.  Never for
// L == 1 (its last layer gathers from E^0, which that launch updates), never on a graph with hub rows (rows beyond kWgRowMax entries
// are summed by groups in the chunk kernel: segment order would not give the same bits) or without the chunk table (the generic
// kernel's order).  The fused launch gathers every slot's row, duplicates included, so beyond some T it does more work than a
// whole-graph layer: it is taken while kFusedRowsPerTriple * T <= n_rows.  (SPEX_STEP_FUSED_LAST=0 / 1 forces either form wherever
// both are legal.)  The constant is fixed from tools/fused_last_time.py on Epinion2 (15 593 rows: T <= 2 598), MI355X, both forms
// forced, us per step whole-graph / fused (profiles/fused_last/t_sweep.jsonl):
//   L = 3   T = 256  38.7 / 33.8   1024  39.0 / 33.5   2048  39.7 / 35.7   2304  40.1 / 38.5   2560  40.6 / 39.6   3072  41.4 / 41.9
//           4096  42.7 / 44.1   8192  48.7 / 61.1
//   L = 2   T = 256  27.3 / 21.5   1024  27.7 / 22.6   2048  28.5 / 24.1   2304  28.7 / 28.4   2560  29.3 / 28.6   3072  29.9 / 30.7
//           4096  31.3 / 34.4   8192  36.9 / 49.6
// (the step beyond T = 2048 is the fused launch's second dispatch round: more than 512 workgroups of four triples).
constexpr int64_t kFusedRowsPerTriple = 6;
bool step_fuses_last(const spex_graph *g, int32_t d, int32_t L, int64_t T)
{
    if (d != 64 || L < 2 || g->task == nullptr || g->mask_mode != 0 || g->n_hub != 0 || g->n_rows == 0 || T <= 0) return false;
    const char *sw = getenv("SPEX_STEP_FUSED_LAST");
    if (sw && sw[0] == '0') return false;
    if (sw && sw[0] == '1') return true;
    return kFusedRowsPerTriple * T <= (int64_t)g->n_rows;
}

}  // namespace

// The propagation with the layer mean LEFT TO THE CONSUMER (the fused BPR step reads the propagated table at its triples' rows
// only, and adds its updates into E^0 while it reads): what the consumer adds, in this order, before dividing by L + 1, is reported
// in (*snap, tables[0..2]).  1 <= L <= 3.  Two schedules (step_takes_snapshot), the same sums bit for bit:
//   snapshot  EVERY layer in the PLAIN form (no epilogue operand, one output stream); the layer-1 launch carries a tail of
//             workgroups that copy the E^0 rows of the step's <= 3 T slots into the handle's compact buffer (SnapArgs).  E^1 goes to
//             sum1, E^2 / E^3 to the two halves of ws: (*snap = E^0 at the slots, E^1, E^2, E^3), i.e. ((E^0 + E^1) + E^2) + E^3.
//   fallback  (no triples given, or the tail would push a one-round launch over 512 workgroups) layer 1 in the running-sum form —
//             sum1 = E^0 + E^1 over the whole table, +2.9 us on Epinion2 —, the later layers plain into the halves of ws:
//             (*snap = NULL, sum1, E^2, E^3).
// With last_src given and step_fuses_last() true, either schedule stops one launch short: L - 1 launches, *last_src = the layer-(L-1)
// table (E^1 for L = 2, E^2 for L = 3), tables[] lists the L - 1 layers in front, and the consumer gathers layer L at its rows
// (spex::bpr_sgd_fused_last).  sum1 keeps its content on both schedules.
// One timer bracket (the profiling hook) spans the whole-graph launches like spex_propagate_f32's.
int spex::propagate_plain(const spex_graph_t *g, const float *E0, float *sum1, float *ws, int32_t L, int32_t d, void *stream,
                          const float **tables, const int64_t *u, const int64_t *i_pos, const int64_t *i_neg, int64_t T,
                          int32_t n_user_rows, const float **snap, const float **last_src)
{
    SPEX_CHECK_ARG(g && E0 && sum1 && ws && tables, "propagate_plain: NULL argument");
    SPEX_CHECK_ARG(g->n_rows == g->n_cols && L >= 1 && L <= 3, "propagate_plain: square graph, 1 <= L <= 3 (L = %d)", L);
    int rc = ensure_partial(const_cast<spex_graph *>(g), d);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t sz = (size_t)g->n_rows * d;
    tables[0] = sum1; tables[1] = nullptr; tables[2] = nullptr;
    if (snap) *snap = nullptr;
    if (last_src) *last_src = nullptr;
    // (the consumer gathers layer L itself: one launch fewer, on either schedule; that layer's half of ws is not written)
    const bool fuse = last_src && u && i_pos && i_neg && n_user_rows >= 0 && n_user_rows <= g->n_rows && step_fuses_last(g, d, L, T);
    if (snap && u && i_pos && i_neg && n_user_rows >= 0 && n_user_rows <= g->n_rows && step_takes_snapshot(g, d, T)) {
        const int64_t slots = (3 * T + kWave - 1) / kWave * kWave;      // whole waves: the tail stores without a row test
        rc = ensure_snap(const_cast<spex_graph *>(g), slots * 64);
        if (rc) return rc;
        SnapArgs sa{u, i_pos, i_neg, g->snap, T, n_user_rows, g->n_rows - n_user_rows, 0};
        TimerBracket bracket(g, s);
        float *e1 = sum1, *e2 = ws, *e3 = ws + sz;
        rc = launch_spmm(g, E0, e1, nullptr, 1.0f, nullptr, nullptr, 1.0f, d, s, 1.0f, &sa);             // E^1, and the slots' E^0 rows
        *snap = g->snap;
        if (rc || L == 1) return rc;
        if (fuse && L == 2) { *last_src = e1; return rc; }
        rc = launch_spmm(g, e1, e2, nullptr, 1.0f, nullptr, nullptr, 1.0f, d, s);                         // E^2
        tables[1] = e2;
        if (rc || L == 2) return rc;
        if (fuse) { *last_src = e2; return rc; }
        rc = launch_spmm(g, e2, e3, nullptr, 1.0f, nullptr, nullptr, 1.0f, d, s);                         // E^3
        tables[2] = e3;
        return rc;
    }
    TimerBracket bracket(g, s);
    float *e1 = ws, *e2 = ws + sz;
    rc = launch_spmm(g, E0, L > 1 ? e1 : nullptr, nullptr, 1.0f, E0, sum1, 1.0f, d, s);                     // E^1, sum1 = E^0 + E^1
    if (rc || L == 1) return rc;
    if (fuse && L == 2) { *last_src = e1; return rc; }
    rc = launch_spmm(g, e1, e2, nullptr, 1.0f, nullptr, nullptr, 1.0f, d, s);                                 // E^2
    tables[1] = e2;
    if (rc || L == 2) return rc;
    if (fuse) { *last_src = e2; return rc; }
    rc = launch_spmm(g, e2, e1, nullptr, 1.0f, nullptr, nullptr, 1.0f, d, s);                                 // E^3 (E^1 is dead: in sum1)
    tables[2] = e1;
    return rc;
}

// out = in / div over n floats (the mean's backward share), for the other translation units.
int spex::scale_div(const float *in, float *out, float div, int64_t n, void *stream)
{
    if (n <= 0) return SPEX_OK;
    SPEX_CHECK_ARG(in && out && ((((uintptr_t)in) | ((uintptr_t)out)) & 15) == 0, "scale_div: NULL or unaligned pointer");
    const int64_t n4 = n / 4, rem = n % 4;
    const int64_t blocks = (n4 + 255) / 256 < 2048 ? ((n4 + 255) / 256 > 0 ? (n4 + 255) / 256 : 1) : 2048;
    hipLaunchKernelGGL(div_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, div, n4, rem);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_propagate_bwd_f32(const spex_graph_t *gt, const float *g_out, float *grad_E0, float *ws, int32_t L,
                                      int32_t d, void *stream)
{
    SPEX_CHECK_ARG(gt && g_out && grad_E0 && ws, "spex_propagate_bwd_f32: NULL argument");
    SPEX_CHECK_ARG(gt->n_rows == gt->n_cols, "spex_propagate_bwd_f32: needs a square graph");
    SPEX_CHECK_ARG(L >= 0 && d >= 1, "spex_propagate_bwd_f32: L = %d, d = %d", L, d);
    SPEX_CHECK_ARG(g_out != grad_E0, "spex_propagate_bwd_f32: grad_E0 must not alias g_out");
    int rc = ensure_partial(const_cast<spex_graph *>(gt), d);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t sz = (size_t)gt->n_rows * d;
    if (sz == 0) return SPEX_OK;
    TimerBracket bracket(gt, s);
    if (L >= 1 && ((L + 1) & L) == 0) {
        // L+1 is a power of two: scaling by it commutes with every rounding below, so carry H_l = (L+1) G_l instead
        // (H_L = g, H_l = g + A^T H_{l+1}) and divide once in the last launch's epilogue — bit-identical to the
        // general path, one elementwise pass and one launch fewer.
        const float *cur = g_out;
        for (int32_t l = L - 1; l >= 0; --l) {
            float *nxt = (l == 0) ? grad_E0 : ws + (size_t)(1 + (l & 1)) * sz;
            rc = launch_spmm(gt, cur, nxt, g_out, 1.0f, nullptr, nullptr, 1.0f, d, s, l == 0 ? (float)(L + 1) : 1.0f);
            if (rc) return rc;
            cur = nxt;
        }
        SPEX_HIP(hipGetLastError());
        return SPEX_OK;
    }
    // gs = g_out / (L+1) is every layer's share of the mean's gradient and the first gather source (= G_L).
    float *gs = (L == 0) ? grad_E0 : ws;
    {
        const int64_t n4 = (int64_t)(sz / 4), rem = (int64_t)(sz % 4);
        const int64_t blocks = (n4 + 255) / 256 < 2048 ? ((n4 + 255) / 256 > 0 ? (n4 + 255) / 256 : 1) : 2048;
        hipLaunchKernelGGL(div_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g_out, gs, (float)(L + 1), n4, rem);
    }
    const float *cur = gs;
    for (int32_t l = L - 1; l >= 0; --l) {
        float *nxt = (l == 0) ? grad_E0 : ws + (size_t)(1 + (l & 1)) * sz;
        rc = launch_spmm(gt, cur, nxt, gs, 1.0f, nullptr, nullptr, 1.0f, d, s);
        if (rc) return rc;
        cur = nxt;
    }
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}
