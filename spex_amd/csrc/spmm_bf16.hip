// Mixed-precision SpMM for CDNA4 (gfx950), d == 64: the chunk kernel of spmm.hip gathering from a bf16 table.
//
// A 64-column bf16 row is 128 bytes — one L2 line where the fp32 row is two, 136 algorithmic bytes per stored entry instead of
// 264.  Only the GATHER SOURCE is rounded: bf16 -> fp32 widening is exact (a 16-bit shift), every product and sum is the fp32
// fmaf chain of spmm_chunk_kernel in the same order — acc = fmaf(val, widen(x16), acc) in the task's entry order, segments of
// rows of 65..1 024 entries added through LDS in segment order — so on the widened table Xw = float(X16) the launch returns what
// spex_spmm_f32 returns on Xw, bit for bit, for every row of at most 1 024 entries, under either edge-dropout mode too.
//
// The kernel READS the handle's task and chunk tables (task, chunk_off, chunk_val, chunk_mask, chunk_row, chunk_eid): no second
// copy of the matrix.  Lane == embedding column: a gathered row is one 128-byte wave load of 2-byte elements.
// Outputs (any subset): Y (fp32), Y16 = bf16(the same fp32 value), round to nearest even — the next layer's gather source,
// written here so that no cast pass runs between layers —, acc_out = (acc_in + y) / acc_div.
// Rows beyond 1 024 entries (hubs): one partial row per 64-entry segment in the handle's scratch, added in segment order by
// spmm_hub_fixup_bf16_kernel behind the launch (the fp32 launch's SPEX_HUB_FOLD=0 schedule; a hub row's sum associates
// differently from the in-launch fold's).
#include <mutex>

#include "spex_common.h"

using namespace spex;

namespace {

struct DropArgs {
    const uint32_t *chunk_eid;
    const uint8_t *keep;
    int mode;
    float keep_prob;
    uint32_t seed_lo, seed_hi;
};

__device__ __forceinline__ float lane_bcast(float v, int src)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// A/B switch for scratch builds: 0 = one gathered entry per register (2 to 10 VGPRs ABOVE the fp32 kernel of the same form).
#ifndef SPEX_BF16_PACK
#define SPEX_BF16_PACK 1
#endif
typedef unsigned short h2 __attribute__((ext_vector_type(2)));
// bf16 -> fp32 is exact: the 16 bits become the high half of the word.  Two gathered entries share a register (low / high half):
// widening is a shift or a mask.
__device__ __forceinline__ float widen_pair(h2 p, int hi)
{
    const uint32_t w = __builtin_bit_cast(uint32_t, p);
    return __uint_as_float(hi ? (w & 0xFFFF0000u) : (w << 16));
}

// fp32 -> bf16, round to nearest even; NaN stays NaN (quiet), +-0 and +-Inf are preserved, the largest finite fp32 rounds to Inf.
__device__ __forceinline__ uint16_t bf16_rne(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ int xcd_contiguous_block(int bid, int nblk)
{
    return ((nblk & 7) == 0) ? (bid & 7) * (nblk >> 3) + (bid >> 3) : bid;
}

// v / div for a wave-uniform divisor, with spmm_chunk_kernel's arms (a power-of-two divisor is one exact multiply): the same bits.
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

// EPI 0: Y / Y16 = y;  1: Y / Y16 = y (optional), acc_out = (acc_in + y) / epi_div;  2: Y / Y16 = y + add_in / epi_div.
// ROWIDS: a task's rows are listed per entry (bin-packed tasks) instead of being adjacent from task.z.
template <int EPI, bool MASKED, bool ROWIDS>
__global__ __launch_bounds__(kWave *kWgWaves) __attribute__((amdgpu_waves_per_eu(8, 8))) void spmm_chunk_bf16_kernel(
    const uint16_t *__restrict__ X16, const uint32_t *__restrict__ chunk_off, const float *__restrict__ chunk_val,
    const uint32_t *__restrict__ chunk_mask, const int32_t *__restrict__ chunk_row, const int4 *__restrict__ task,
    int n_tasks, float *__restrict__ Y, uint16_t *__restrict__ Y16,
    const float *epi_in, float epi_div, float *acc_out,                  // may alias each other (running sum in place): no __restrict__
    float *__restrict__ partial, const DropArgs drop, const int xcd_contiguous, const int chunk_stride)
{
    __shared__ float s_part[kWgWaves][kWave];  // segment sums of the rows this workgroup combines
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wg = xcd_contiguous ? xcd_contiguous_block(blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int tid = wg * kWgWaves + wave;
    if (tid >= n_tasks) return;  // whole workgroups only (n_tasks is a multiple of kWgWaves)
    // Implied positions (chunk_stride != 0, bin-packed tables): the first super-chunk's metadata is requested in the same round
    // trip as the task record (spmm_chunk_kernel).
    const bool implied = ROWIDS && chunk_stride != 0;
    uint32_t pre_off = 0u, pre_mask = 0u, pre_eid = 0u;
    int pre_row = 0;
    float pre_val = 0.0f;
    if (implied) {
        const size_t c0 = (size_t)tid * (size_t)chunk_stride, e = c0 * kChunk + lane;
        pre_off = __builtin_nontemporal_load(chunk_off + e);
        pre_val = __builtin_nontemporal_load(chunk_val + e);
        pre_row = __builtin_nontemporal_load(chunk_row + e);
        if (MASKED) pre_eid = __builtin_nontemporal_load(drop.chunk_eid + e);
        pre_mask = __builtin_nontemporal_load(chunk_mask + c0 + (lane & 3));
    }
    const int4 t = task[tid];
    const int kind = t.w & 3;
    const uint16_t *__restrict__ Xl = X16 + lane;
    const float *El = epi_in + lane;             // (EPI == 0: never read)
    int row = t.z;
    float acc = 0.0f;
    const float epi_inv = 1.0f / epi_div;        // (once per wave; exact for a power of two)

    auto put = [&](size_t o, float v) {          // outputs are streamed (non-temporal): they should not evict the gather source
        if (Y) __builtin_nontemporal_store(v, Y + o);
        if (Y16) __builtin_nontemporal_store(bf16_rne(v), Y16 + o);
    };
    auto emit = [&](int r, float y, float e) {
        const size_t o = (size_t)r * 64 + lane;
        if (EPI == 0) {
            put(o, y);
        } else if (EPI == 1) {
            const float s = scaled(e + y, epi_div, epi_inv);
            put(o, y);
            __builtin_nontemporal_store(s, acc_out + o);
        } else {
            put(o, y + scaled(e, epi_div, epi_inv));
        }
    };

    // A LIST of rows without stored entries (kind 3, bin-packed tables only; <= 64 rows, lane k holds the k-th row id): y = 0, the
    // epilogue still applies.  Four rows per instruction (16 lanes x 4 columns per row), as in spmm_chunk_kernel.
    if (ROWIDS && kind == 3) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        typedef unsigned short h4 __attribute__((ext_vector_type(4)));
        const int count = t.w >> 4;
        int my_r = -1;
        if (lane < count) my_r = implied ? pre_row : chunk_row[(size_t)t.x * kChunk + lane];
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
                f4 yv = zero;
                if (EPI == 1) {
                    f4 sv = e[j] + zero;
                    if (epi_div != 1.0f) sv = sv / epi_div;
                    __builtin_nontemporal_store(sv, reinterpret_cast<f4 *>(acc_out + o));
                } else if (EPI == 2) {
                    f4 ev = e[j];
                    if (epi_div != 1.0f) ev = ev / epi_div;
                    yv = zero + ev;
                }
                if (Y) __builtin_nontemporal_store(yv, reinterpret_cast<f4 *>(Y + o));
                if (Y16) {
                    h4 hv;
#pragma unroll
                    for (int q = 0; q < 4; ++q) hv[q] = bf16_rne(yv[q]);
                    __builtin_nontemporal_store(hv, reinterpret_cast<h4 *>(Y16 + o));
                }
            }
        }
    }
    const int n_ch = kind == 3 ? 0 : t.y;              // (kind 3: handled above)
    // One super-chunk (<= 4 chunks from chunk t.x + sc).  first: the one requested in front of the task record (implied positions).
    auto super_chunk = [&](const int sc, const bool first) __attribute__((always_inline)) {
        const int nc = (n_ch - sc < 4) ? n_ch - sc : 4;  // chunks in this super-chunk (wave-uniform)
        uint32_t my_off = 0u, my_mask = 0u, own_off = 0u;
        unsigned long long drop_bits = 0ull;                 // MASKED: entries of this super-chunk that are dropped (wave-uniform)
        int my_row = 0;
        float my_val = 0.0f;
        if (lane < nc * kChunk) {
            uint32_t eid = 0u;
            if (first) {
                my_off = pre_off;
                my_val = pre_val;
                my_row = pre_row;
                if (MASKED) eid = pre_eid;
            } else {
                const size_t e = (size_t)(t.x + sc) * kChunk + lane;
                my_off = __builtin_nontemporal_load(chunk_off + e);   // metadata is read once per launch
                my_val = __builtin_nontemporal_load(chunk_val + e);
                if (ROWIDS) my_row = __builtin_nontemporal_load(chunk_row + e);
                if (MASKED) eid = __builtin_nontemporal_load(drop.chunk_eid + e);
            }
            if (MASKED) {
                bool kept;
                if (drop.mode == 1) {
                    kept = drop.keep[eid] != 0;
                } else {
                    const float u01 = (float)(philox_first(eid, drop.seed_lo, drop.seed_hi) >> 8) * 5.9604644775390625e-8f;
                    kept = (u01 + drop.keep_prob) >= 1.0f;
                }
                my_val = kept ? my_val / drop.keep_prob : 0.0f;   // values[random_index] / keep_prob, model.py:53
                own_off = my_off;
                if (!kept) my_off = 0xFFFFFFFFu;
            }
        }
        if (MASKED) {
            // a dropped entry re-reads the source row of the first KEPT entry of this super-chunk (the stand-in: fetched anyway);
            // if every entry was dropped each keeps its own row (value 0)
            const bool dropped = my_off == 0xFFFFFFFFu;      // (lanes past the super-chunk hold 0: neither kept nor dropped)
            drop_bits = __ballot(dropped);
            const unsigned long long kept_lanes = __ballot(!dropped && lane < nc * kChunk);
            const int src = kept_lanes ? (int)__builtin_ctzll(kept_lanes) : 0;
            const uint32_t stand_in = (uint32_t)__builtin_amdgcn_readlane((int)my_off, src);   // wave-uniform
            if (dropped) my_off = kept_lanes ? stand_in : own_off;
        }
        if (first) my_mask = pre_mask;                       // (lane c < 4 holds chunk c's word; words beyond nc are not read)
        else if (lane < nc) my_mask = __builtin_nontemporal_load(chunk_mask + t.x + sc + lane);
        float ep[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u) ep[u] = 0.0f;
        for (int c = 0; c < nc; ++c) {
            const uint32_t mask = (uint32_t)__builtin_amdgcn_readlane((int)my_mask, c);
            const uint32_t dbits = MASKED ? (uint32_t)(drop_bits >> (c * kChunk)) & 0xFFFFu : 0u;
#if SPEX_BF16_PACK
            h2 x[kChunk / 2];                                // sixteen 2-byte gathers issued back to back, two entries per register
#define SPEX_X16(u) x[(u) >> 1][(u) & 1]
#define SPEX_XW(u) widen_pair(x[(u) >> 1], (u) & 1)
#else
            uint16_t x[kChunk];                              // (A/B form: one entry per register, widened by a shift)
#define SPEX_X16(u) x[u]
#define SPEX_XW(u) __uint_as_float((uint32_t)x[u] << 16)
#endif
#pragma unroll
            for (int u = 0; u < kChunk; ++u)
                SPEX_X16(u) = Xl[(size_t)(uint32_t)__builtin_amdgcn_readlane((int)my_off, c * kChunk + u) * 64];
            if (EPI != 0 && mask != 0u) {
                int r = row;
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    if (mask & (1u << u)) {
                        const int rr = ROWIDS ? __builtin_amdgcn_readlane(my_row, c * kChunk + u) : r;
                        ep[u] = __builtin_nontemporal_load(El + (size_t)rr * 64);
                        ++r;
                    }
                }
            }
            // A chunk that ends rows waits for ALL of its loads here, once (spmm_chunk_kernel: a row's epilogue operand must not
            // wait out its predecessor's stores).
            if (EPI != 0) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0); expcnt / lgkmcnt unconstrained
            if (EPI == 0 && mask == 0u) {                     // no row ends in this chunk: sixteen fmafs, no per-entry test
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    const float xv = (MASKED && (dbits & (1u << u))) ? 0.0f : SPEX_XW(u);
                    acc = fmaf(lane_bcast(my_val, c * kChunk + u), xv, acc);
                }
                continue;
            }
#pragma unroll
            for (int u = 0; u < kChunk; ++u) {
                const float xv = (MASKED && (dbits & (1u << u))) ? 0.0f : SPEX_XW(u);     // a dropped entry contributes nothing
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
                pre_row = __builtin_nontemporal_load(chunk_row + e);
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
    if (kind == 2) partial[(size_t)(t.w >> 4) * 64 + lane] = acc;  // hub segment: summed by the fix-up launch
    if (t.w & 4) {  // this workgroup combines the segments of rows with 65..1024 entries through LDS
        const bool leader = kind == 1 && (t.w & 8);
        const int slot = (t.w >> 4) & 15, nseg = (t.w >> 8) & 31;
        float e = 0.0f;
        if (leader && EPI != 0) e = El[(size_t)t.z * 64];
        if (kind == 1 && !leader) s_part[slot][lane] = acc;
        __syncthreads();
        if (leader) {
            float y = acc;
            for (int sgi = 1; sgi < nseg; ++sgi) y = y + s_part[slot + sgi][lane];  // segment order: deterministic
            emit(t.z, y, e);
        }
    }
}

// One wave per hub row (more than 1 024 entries): its segments' partial rows added in segment order, then the launch's epilogue.
__global__ __launch_bounds__(kWave *kWavesPerBlock) void spmm_hub_fixup_bf16_kernel(
    const float *__restrict__ partial, const int32_t *__restrict__ rows, const int32_t *__restrict__ seg, int n_hub,
    float *__restrict__ Y, uint16_t *__restrict__ Y16, const float *add_in, float add_div, const float *acc_in, float *acc_out,
    float acc_div)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (i >= n_hub) return;
    const int r = rows[i];
    const int s0 = seg[2 * i], s1 = seg[2 * i + 1];
    float y = 0.0f;
    int s = s0;
    for (; s + 16 <= s1; s += 16) {              // sixteen partial rows in flight
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = partial[(size_t)(s + u) * 64 + lane];
#pragma unroll
        for (int u = 0; u < 16; ++u) y = y + v[u];
    }
    for (; s < s1; ++s) y = y + partial[(size_t)s * 64 + lane];
    const size_t o = (size_t)r * 64 + lane;
    if (add_in) y = y + add_in[o] / add_div;
    if (Y) Y[o] = y;
    if (Y16) Y16[o] = bf16_rne(y);
    if (acc_out) acc_out[o] = (acc_in[o] + y) / acc_div;
}

// fp32 -> bf16 over n elements, pure streaming: four elements per lane and trip (one 16-byte load, one 8-byte store).
template <bool VEC>
__global__ __launch_bounds__(256) void cast_bf16_kernel(const float *__restrict__ X, uint16_t *__restrict__ X16, int64_t n)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef unsigned short h4 __attribute__((ext_vector_type(4)));
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const int64_t n4 = n / 4;
        for (int64_t i = t0; i < n4; i += stride) {
            const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(X) + i);
            h4 h;
#pragma unroll
            for (int q = 0; q < 4; ++q) h[q] = bf16_rne(v[q]);
            __builtin_nontemporal_store(h, reinterpret_cast<h4 *>(X16) + i);
        }
        const int64_t k = n4 * 4 + t0;           // the last n % 4 elements
        if (k < n) X16[k] = bf16_rne(X[k]);
    } else {
        for (int64_t i = t0; i < n; i += stride) X16[i] = bf16_rne(X[i]);
    }
}

int launch_cast(const float *X, uint16_t *X16, int64_t n, hipStream_t stream)
{
    if (n == 0) return SPEX_OK;
    const bool vec = ((((uintptr_t)X) & 15) | (((uintptr_t)X16) & 7)) == 0;
    const int64_t work = vec ? (n + 3) / 4 : n;
    int64_t blocks = (work + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (vec) hipLaunchKernelGGL(cast_bf16_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, X, X16, n);
    else hipLaunchKernelGGL(cast_bf16_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, X, X16, n);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

template <int EPI>
void launch_chunk_bf16(bool masked, bool row_ids, dim3 grid, dim3 block, hipStream_t stream, const uint16_t *X16, const spex_graph *g,
                       float *Y, uint16_t *Y16, const float *epi_in, float epi_div, float *acc_out, const DropArgs &da, int xcd_contig)
{
#define SPEX_GO(M, R)                                                                                                         \
    hipLaunchKernelGGL((spmm_chunk_bf16_kernel<EPI, M, R>), grid, block, 0, stream, X16, g->chunk_off, g->chunk_val, g->chunk_mask, \
                       g->chunk_row, g->task, g->n_tasks, Y, Y16, epi_in, epi_div, acc_out, g->partial, da, xcd_contig, g->chunk_stride)
    if (masked) {
        if (row_ids) SPEX_GO(true, true);
        else SPEX_GO(true, false);
    } else {
        if (row_ids) SPEX_GO(false, true);
        else SPEX_GO(false, false);
    }
#undef SPEX_GO
}

// The hub segments' partial rows live in the handle's scratch: [n_seg][64] floats (allocated with the handle for d == 64; grown here
// if a caller never needed it — outside any stream capture).
int ensure_partial64(spex_graph *g)
{
    const int64_t need = (int64_t)g->n_seg * 64;
    if (g->n_hub == 0 || need <= g->partial_cap) return SPEX_OK;
    SPEX_HIP(hipDeviceSynchronize());
    if (g->partial) SPEX_HIP(hipFree(g->partial));
    g->partial = nullptr;
    g->partial_cap = 0;
    SPEX_HIP(hipMalloc((void **)&g->partial, (size_t)need * sizeof(float)));
    g->partial_cap = need;
    return SPEX_OK;
}

// Arguments are validated by the callers.  Not both epilogues at once.
int launch_spmm_bf16(const spex_graph *g, const uint16_t *X16, float *Y, uint16_t *Y16, const float *add_in, float add_div,
                     const float *acc_in, float *acc_out, float acc_div, hipStream_t stream)
{
    if (g->n_rows == 0) return SPEX_OK;
    const bool masked = g->mask_mode != 0;
    int64_t blocks = ((int64_t)g->n_tasks + kWgWaves - 1) / kWgWaves;
    blocks = (blocks + 7) / 8 * 8;  // multiple of the XCD count so the remap is a bijection
    const dim3 grid((unsigned)blocks), block(kWave * kWgWaves);
    std::unique_lock<std::mutex> scratch_lock;   // (held until the launches below are queued)
    if (g->n_hub > 0) {   // this launch writes the handle's scratch: order it behind its last user (spmm.hip: launch_spmm)
        spex_graph *gm = const_cast<spex_graph *>(g);
        scratch_lock = std::unique_lock<std::mutex>(gm->scratch_mu);
        if (gm->scratch_used && gm->scratch_stream != stream) {
            if (!gm->scratch_ev) SPEX_HIP(hipEventCreateWithFlags(&gm->scratch_ev, hipEventDisableTiming));
            SPEX_HIP(hipEventRecord(gm->scratch_ev, gm->scratch_stream));
            SPEX_HIP(hipStreamWaitEvent(stream, gm->scratch_ev, 0));
        }
        gm->scratch_stream = stream;
        gm->scratch_used = true;
    }
    const int xcd_contig = ((int64_t)g->n_cols * 64 * 2 <= (int64_t)16 << 20) ? 1 : 0;  // source table <= 16 MiB
    DropArgs da;
    da.chunk_eid = g->chunk_eid; da.keep = g->keep; da.mode = g->mask_mode; da.keep_prob = g->keep_prob;
    da.seed_lo = (uint32_t)g->seed; da.seed_hi = (uint32_t)(g->seed >> 32);
    if (acc_out) launch_chunk_bf16<1>(masked, g->row_ids, grid, block, stream, X16, g, Y, Y16, acc_in, acc_div, acc_out, da, xcd_contig);
    else if (add_in) launch_chunk_bf16<2>(masked, g->row_ids, grid, block, stream, X16, g, Y, Y16, add_in, add_div, nullptr, da, xcd_contig);
    else launch_chunk_bf16<0>(masked, g->row_ids, grid, block, stream, X16, g, Y, Y16, nullptr, 1.0f, nullptr, da, xcd_contig);
    if (g->n_hub > 0) {
        const dim3 fgrid((unsigned)((g->n_hub + kWavesPerBlock - 1) / kWavesPerBlock));
        hipLaunchKernelGGL(spmm_hub_fixup_bf16_kernel, fgrid, dim3(kWave * kWavesPerBlock), 0, stream, g->partial, g->hub_row, g->hub_seg0,
                           g->n_hub, Y, Y16, add_in, add_div, acc_in, acc_out, acc_div);
    }
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr, const void *e = nullptr,
               const void *f = nullptr)
{
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d) | ((uintptr_t)e) | ((uintptr_t)f)) & 15) == 0;
}

// What every bf16 entry checks once it may read the handle.
int check_graph_bf16(const spex_graph *g, const char *who, bool square)
{
    SPEX_CHECK_ARG(!square || g->n_rows == g->n_cols, "%s: needs a square graph (%d x %d)", who, g->n_rows, g->n_cols);
    if (g->task == nullptr && g->n_rows > 0) {
        spex::set_error("%s: the handle has no chunked task table (its source table exceeds a 32-bit offset): use the fp32 entries", who);
        return SPEX_ERR_UNSUPPORTED;
    }
    return SPEX_OK;
}

#define SPEX_BF16_D64(who, d)                                                                                            \
    do {                                                                                                                 \
        if ((d) != 64) {                                                                                                 \
            spex::set_error("%s: bf16 gather tables are built for d == 64 only (d = %d): use the fp32 entries", who, (int)(d)); \
            return SPEX_ERR_UNSUPPORTED;                                                                                 \
        }                                                                                                                \
    } while (0)

}  // namespace

extern "C" int spex_cast_bf16_f32(const float *X, uint16_t *X16, int64_t n, void *stream)
{
    SPEX_CHECK_ARG(n >= 0, "spex_cast_bf16_f32: n = %lld", (long long)n);
    SPEX_CHECK_ARG(n == 0 || (X && X16), "spex_cast_bf16_f32: NULL X or X16");
    SPEX_CHECK_ARG((((uintptr_t)X) & 3) == 0 && (((uintptr_t)X16) & 1) == 0, "spex_cast_bf16_f32: X / X16 not aligned to their element");
    SPEX_CHECK_ARG((const void *)X != (const void *)X16 || n == 0, "spex_cast_bf16_f32: X16 must not alias X");
    return launch_cast(X, X16, n, (hipStream_t)stream);
}

extern "C" int spex_spmm_bf16_f32(const spex_graph_t *g, const uint16_t *X16, float *Y, uint16_t *Y16, const float *add_in,
                                  float add_div, const float *acc_in, float *acc_out, float acc_div, int32_t d, void *stream)
{
    SPEX_BF16_D64("spex_spmm_bf16_f32", d);
    SPEX_CHECK_ARG(X16, "spex_spmm_bf16_f32: NULL X16");
    SPEX_CHECK_ARG(Y || Y16 || acc_out, "spex_spmm_bf16_f32: no output requested (Y, Y16 and acc_out are all NULL)");
    SPEX_CHECK_ARG(!acc_out || acc_in, "spex_spmm_bf16_f32: acc_out needs acc_in");
    SPEX_CHECK_ARG(X16 != Y16 && (const void *)X16 != (const void *)Y && (const void *)X16 != (const void *)acc_out,
                   "spex_spmm_bf16_f32: X16 must not alias an output");
    SPEX_CHECK_ARG((!Y16 || ((const void *)Y16 != (const void *)Y && (const void *)Y16 != (const void *)acc_out)) && (!Y || Y != acc_out),
                   "spex_spmm_bf16_f32: the outputs must not alias each other");
    SPEX_CHECK_ARG(!add_in || add_div != 0.0f, "spex_spmm_bf16_f32: add_div == 0");
    SPEX_CHECK_ARG(!acc_out || acc_div != 0.0f, "spex_spmm_bf16_f32: acc_div == 0");
    SPEX_CHECK_ARG(aligned16(X16, Y, Y16, add_in, acc_in, acc_out), "spex_spmm_bf16_f32: X16 / Y / Y16 / add_in / acc_in / acc_out must be 16-byte aligned");
    if (acc_out && add_in) {
        spex::set_error("spex_spmm_bf16_f32: add_in and acc_out in one launch are not supported: use one epilogue per launch");
        return SPEX_ERR_UNSUPPORTED;
    }
    SPEX_CHECK_ARG(g, "spex_spmm_bf16_f32: NULL graph");
    int rc = check_graph_bf16(g, "spex_spmm_bf16_f32", false);
    if (rc) return rc;
    rc = ensure_partial64(const_cast<spex_graph *>(g));
    if (rc) return rc;
    return launch_spmm_bf16(g, X16, Y, Y16, add_in, add_div, acc_in, acc_out, acc_div, (hipStream_t)stream);
}

extern "C" int spex_propagate_bf16_f32(const spex_graph_t *g, const float *E0, float *mean_out, uint16_t *ws16, int32_t L, int32_t d,
                                       void *stream)
{
    SPEX_BF16_D64("spex_propagate_bf16_f32", d);
    SPEX_CHECK_ARG(E0 && mean_out, "spex_propagate_bf16_f32: NULL E0 or mean_out");
    SPEX_CHECK_ARG(L >= 0, "spex_propagate_bf16_f32: L = %d", L);
    SPEX_CHECK_ARG(ws16 || L == 0, "spex_propagate_bf16_f32: NULL ws16");
    SPEX_CHECK_ARG(E0 != mean_out && (const void *)ws16 != (const void *)E0 && (const void *)ws16 != (const void *)mean_out,
                   "spex_propagate_bf16_f32: E0, mean_out and ws16 must not alias");
    SPEX_CHECK_ARG(aligned16(E0, mean_out, ws16), "spex_propagate_bf16_f32: E0 / mean_out / ws16 must be 16-byte aligned");
    SPEX_CHECK_ARG(g, "spex_propagate_bf16_f32: NULL graph");
    int rc = check_graph_bf16(g, "spex_propagate_bf16_f32", true);
    if (rc) return rc;
    rc = ensure_partial64(const_cast<spex_graph *>(g));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t sz = (size_t)g->n_rows * 64;
    if (sz == 0) return SPEX_OK;
    if (L == 0) {
        SPEX_HIP(hipMemcpyAsync(mean_out, E0, sz * sizeof(float), hipMemcpyDeviceToDevice, s));
        return SPEX_OK;
    }
    rc = launch_cast(E0, ws16, (int64_t)sz, s);                                       // E16^0 = bf16(E^0)
    if (rc) return rc;
    for (int32_t l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        const uint16_t *cur = ws16 + (size_t)(l & 1) * sz;
        uint16_t *nxt = last ? nullptr : ws16 + (size_t)((l + 1) & 1) * sz;           // E16^(l+1) = bf16(y), written by the launch
        rc = launch_spmm_bf16(g, cur, nullptr, nxt, nullptr, 1.0f, l == 0 ? E0 : mean_out, mean_out, last ? (float)(L + 1) : 1.0f, s);
        if (rc) return rc;
    }
    return SPEX_OK;
}

extern "C" int spex_propagate_bwd_bf16_f32(const spex_graph_t *gt, const float *g_out, float *grad_E0, float *ws, uint16_t *ws16,
                                           int32_t L, int32_t d, void *stream)
{
    SPEX_BF16_D64("spex_propagate_bwd_bf16_f32", d);
    SPEX_CHECK_ARG(g_out && grad_E0, "spex_propagate_bwd_bf16_f32: NULL g_out or grad_E0");
    SPEX_CHECK_ARG(L >= 0, "spex_propagate_bwd_bf16_f32: L = %d", L);
    SPEX_CHECK_ARG((ws && ws16) || L == 0, "spex_propagate_bwd_bf16_f32: NULL ws or ws16");
    SPEX_CHECK_ARG(g_out != grad_E0 && ws != g_out && ws != grad_E0 && (const void *)ws16 != (const void *)g_out &&
                       (const void *)ws16 != (const void *)grad_E0 && (L == 0 || (const void *)ws16 != (const void *)ws),
                   "spex_propagate_bwd_bf16_f32: g_out, grad_E0, ws and ws16 must not alias");
    SPEX_CHECK_ARG(aligned16(g_out, grad_E0, ws, ws16), "spex_propagate_bwd_bf16_f32: g_out / grad_E0 / ws / ws16 must be 16-byte aligned");
    SPEX_CHECK_ARG(gt, "spex_propagate_bwd_bf16_f32: NULL graph");
    int rc = check_graph_bf16(gt, "spex_propagate_bwd_bf16_f32", true);
    if (rc) return rc;
    rc = ensure_partial64(const_cast<spex_graph *>(gt));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t sz = (size_t)gt->n_rows * 64;
    if (sz == 0) return SPEX_OK;
    if (L == 0) {
        SPEX_HIP(hipMemcpyAsync(grad_E0, g_out, sz * sizeof(float), hipMemcpyDeviceToDevice, s));
        return SPEX_OK;
    }
    // gs = g_out / (L+1): every layer's share of the mean's gradient (the add_in operand) and, rounded, the first gather source
    rc = spex::scale_div(g_out, ws, (float)(L + 1), (int64_t)sz, stream);
    if (rc) return rc;
    rc = launch_cast(ws, ws16, (int64_t)sz, s);
    if (rc) return rc;
    int cur = 0;
    for (int32_t l = L - 1; l >= 0; --l) {
        const bool last = l == 0;
        rc = launch_spmm_bf16(gt, ws16 + (size_t)cur * sz, last ? grad_E0 : nullptr, last ? nullptr : ws16 + (size_t)(cur ^ 1) * sz, ws, 1.0f,
                              nullptr, nullptr, 1.0f, s);
        if (rc) return rc;
        cur ^= 1;
    }
    return SPEX_OK;
}
