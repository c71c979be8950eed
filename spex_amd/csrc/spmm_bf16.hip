// Mixed-precision SpMM for CDNA4 (gfx950), d == 64: the chunk kernel gathering from a bf16 table.
//
// A 64-column bf16 row is 128 bytes — one L2 line where the fp32 row is two, 136 algorithmic bytes per stored entry instead of
// 264.  Only the GATHER SOURCE is rounded: bf16 -> fp32 widening is exact (a 16-bit shift), every product and sum is the fp32
// fmaf chain of spmm_chunk_kernel in the same order, because it is the same text: spmm_chunk_bf16_kernel wraps chunk_body
// (spmm_chunk.h) instantiated for a uint16_t table, as spmm_chunk_kernel of spmm.hip wraps it for a float one.  So on the widened
// table Xw = float(X16) the launch returns what spex_spmm_f32 returns on Xw, bit for bit, for every row of at most 1 024 entries,
// under either edge-dropout mode too.
//
// The kernel READS the handle's task and chunk tables (task, chunk_off, chunk_val, chunk_mask, chunk_row, chunk_eid): no second
// copy of the matrix.  Lane == embedding column: a gathered row is one 128-byte wave load of 2-byte elements.
// Outputs (any subset): Y (fp32), Y16 = bf16(the same fp32 value), round to nearest even — the next layer's gather source,
// written here so that no cast pass runs between layers —, acc_out = (acc_in + y) / acc_div.
// Rows beyond 1 024 entries (hubs): one partial row per 64-entry segment in the handle's scratch, added in segment order by
// spmm_hub_fixup_bf16_kernel behind the launch (the fp32 launch's SPEX_HUB_FOLD=0 schedule; a hub row's sum associates
// differently from the in-launch fold's).
#include <mutex>

#include "spmm_chunk.h"

using namespace spex;
using namespace spex::chunkk;

namespace {

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
    chunk_body<uint16_t, EPI, MASKED, ROWIDS, false>(chunk_off, chunk_val, chunk_row, chunk_mask, task, n_tasks, xcd_contiguous, chunk_stride,
                                                     0, X16, Y, ChunkSide<uint16_t>{Y16}, epi_in, epi_div, acc_out, partial, drop,
                                                     HubFold{nullptr, nullptr, nullptr, 0u}, SnapArgs{});      // (no fold: no tail either)
}

// The list-driven row-list SpMM (spmm.hip: spmm_rowlist_dev_kernel) gathering from a bf16 table: the same rowlist_dev_body
// (spmm_chunk.h), so on Xw = float(X16) the fp32 kernel's bits for EVERY listed row — hubs included: the row's segments are added in
// the same order — and spmm_chunk_bf16_kernel's for rows of up to 1 024 entries.  Y16 = bf16(the register Y gets).
__global__ __launch_bounds__(kWave *kWgWaves) void spmm_rowlist_dev_bf16_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const uint16_t *__restrict__ X16, const int32_t *__restrict__ list, const int32_t *__restrict__ count, int32_t max_count,
    int32_t n_rows, float *Y, uint16_t *Y16, const float *acc_in, float *acc_out, float acc_div)   // (acc_out may alias acc_in: unqualified)
{
    rowlist_dev_body<uint16_t>(rowptr, col, val, X16, list, count, max_count, n_rows, Y, Y16, acc_in, acc_out, acc_div);
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

// Arguments are validated by the callers.  Not both epilogues at once.
int launch_spmm_bf16(const spex_graph *g, const uint16_t *X16, float *Y, uint16_t *Y16, const float *add_in, float add_div,
                     const float *acc_in, float *acc_out, float acc_div, hipStream_t stream)
{
    if (g->n_rows == 0) return SPEX_OK;
    const bool masked = g->mask_mode != 0;
    const dim3 grid((unsigned)chunk_table_wgs(g)), block(kWave * kWgWaves);
    std::unique_lock<std::mutex> scratch_lock;   // (held until the launches below are queued)
    if (g->n_hub > 0) {   // this launch writes the handle's scratch (the hub segments' partial rows): order it behind its last user
        const int rc = order_scratch(g, stream, scratch_lock);
        if (rc) return rc;
    }
    SPEX_CHECK_ARG(!(g->packed_words && g->max_task_chunks > 4), "spex_spmm_bf16_f32: packed words on a table with tasks of %d chunks", g->max_task_chunks);
    const int xcd_contig = ((int64_t)g->n_cols * 64 * 2 <= (int64_t)16 << 20) ? 1 : 0;  // source table <= 16 MiB
    const DropArgs da = drop_args(g);
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
    rc = ensure_partial(const_cast<spex_graph *>(g), 64);      // (the hub segments' partial rows; sized with the handle)
    if (rc) return rc;
    return launch_spmm_bf16(g, X16, Y, Y16, add_in, add_div, acc_in, acc_out, acc_div, (hipStream_t)stream);
}

// spex_spmm_rowlist_dev_f32 on a bf16 table: rows list[0 .. min(*count, max_count)) from the CSR arrays (no task table needed).
extern "C" int spex_spmm_rowlist_dev_bf16_f32(const spex_graph_t *g, const uint16_t *X16, const int32_t *list, const int32_t *count,
                                              int32_t max_count, float *Y, uint16_t *Y16, const float *acc_in, float *acc_out, float acc_div,
                                              int32_t d, void *stream)
{
    const char *who = "spex_spmm_rowlist_dev_bf16_f32";
    SPEX_CHECK_ARG(g && X16 && list && count && max_count >= 0, "%s: NULL graph, X16, list or count, or max_count < 0", who);
    SPEX_CHECK_ARG(Y || Y16 || acc_out, "%s: no output requested (Y, Y16 and acc_out are all NULL)", who);
    SPEX_CHECK_ARG(!acc_out || (acc_in && acc_div != 0.0f), "%s: acc_out needs acc_in and acc_div != 0", who);
    SPEX_CHECK_ARG(X16 != Y16 && (const void *)X16 != (const void *)Y && (const void *)X16 != (const void *)acc_out &&
                       (const void *)X16 != (const void *)acc_in, "%s: X16 must not alias an output or acc_in", who);
    SPEX_CHECK_ARG((!Y16 || ((const void *)Y16 != (const void *)Y && (const void *)Y16 != (const void *)acc_out &&
                             (const void *)Y16 != (const void *)acc_in)) && (!Y || (Y != acc_out && Y != acc_in)),
                   "%s: Y and Y16 must not alias each other, acc_in or acc_out (acc_out may be acc_in)", who);
    if (d != 64 || g->mask_mode != 0) {
        spex::set_error("%s: d == 64 without edge dropout only (d = %d, mask mode %d)", who, d, g->mask_mode);
        return SPEX_ERR_UNSUPPORTED;
    }
    if (max_count == 0 || g->n_rows == 0) return SPEX_OK;
    const int64_t wgs = ((int64_t)max_count + kWgWaves - 1) / kWgWaves;
    hipLaunchKernelGGL(spmm_rowlist_dev_bf16_kernel, dim3((unsigned)(wgs < kDevMaxWgs ? wgs : kDevMaxWgs)), dim3(kWave * kWgWaves), 0,
                       (hipStream_t)stream, g->rowptr, g->col, g->val, X16, list, count, max_count, g->n_rows, Y, Y16, acc_in, acc_out, acc_div);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
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
    rc = ensure_partial(const_cast<spex_graph *>(g), 64);      // (the hub segments' partial rows; sized with the handle)
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
    rc = ensure_partial(const_cast<spex_graph *>(gt), 64);
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
