// Row-sparse pieces of the training step's backward pass.
//
// After a 256-sample batch the gradient with respect to the propagated table is non-zero on at most 512 rows (the
// batch's users and items, LightGCN_SPEX/code/utility1/model.py:115-116; NGCF_SPEX/code/main_rec.py:89-90).  The first
// product of the backward pass, A^T g, therefore touches ~14 k of Epinion2's 418 k stored entries: it is evaluated in
// PUSH form — for every non-zero row r of g, out[c] += A[r, c] * g[r] over the stored entries of row r — instead of the
// pull-form SpMM over the whole matrix (15 us).  SURVEY.md 7 "hard parts" names this.
//
//   spex_unique_rows_i32      the distinct rows of a batch (two index lists with offsets) as a compact device list;
//                             deduplication by an epoch-stamp table, no sort, no host round trip
//   spex_spmm_push_rows_f32   out[col[e], :] += scale * val[e] * src_k  for every stored entry e of every listed row (k-th
//                             listed row r: src_k = src[r] or src[k]), optionally out[r, :] += scale * add_k — 256-byte float atomics
//                             (spex_spmm_push_rows_scaled_f32: a factor of its own for the add term)
//   spex_spmm_push_list_f32   the same product (src by row, no add term) over a LONG device list — a two-hop frontier — in the list
//                             SpMM's work split: a fixed grid over the list, short rows one wave task each (follows the mask too)
//   spex_frontier_rows_i32    behind such a list, the stored columns of its rows not yet stamped this epoch: the batch's frontier
//                             (spex_frontier_rows_masked_i32: the columns reached over entries the handle's edge dropout keeps)
// spex_spmm_push_rows_f32 and _scaled_f32 follow the handle's edge-dropout rule (a kept value is val / keep_prob, a dropped entry
// issues no atomic); spex_spmm_push_batch_f32 takes unmasked handles only.
// Sums arrive in arbitrary order (atomics): results agree with the pull form to fp32 re-association.
#include "spex_common.h"

using namespace spex;

namespace {

__global__ __launch_bounds__(256) void unique_rows_kernel(const int64_t *__restrict__ idx_a, int n_a, int64_t off_a,
                                                          const int64_t *__restrict__ idx_b, int n_b, int64_t off_b,
                                                          int32_t n_rows, int32_t *stamp, int32_t epoch, int32_t *list,
                                                          int32_t *count)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_a + n_b) return;
    const int64_t r = k < n_a ? idx_a[k] + off_a : idx_b[k - n_a] + off_b;
    if (r < 0 || r >= n_rows) return;
    if (atomicExch(stamp + r, epoch) != epoch) list[atomicAdd(count, 1)] = (int32_t)r;   // first visitor of the row this epoch
}

// The frontier of a batch: behind the list spex_unique_rows_i32 wrote, every column of the listed rows that the stamp table has not
// seen this epoch.  One wave per INPUT row, lanes take entries; the rows found by a wave in one 64-entry run are appended with one
// counter bump (the first new lane's atomic, the others take their rank among the new lanes).  n_in is read from a cell the launch
// does not write (count_b), the appends go behind it through count_f: the launch never walks a row it appended itself — that would
// be the two-hop set (SPEX_STEP_SPARSE_ADAM takes that set with a second launch over [0, |F1|), whose host-side bound is n_rows: a
// bounded grid strides over the input).  Every row is stamped at most once per epoch, so n_rows list entries always suffice.
constexpr int kFrontierWaves = 4;
constexpr int kFrontierMaxWgs = 1 << 14;

__global__ void frontier_init_kernel(const int32_t *__restrict__ count_b, int32_t *count_f) { *count_f = *count_b; }

// MASKED (frontier_rows_masked_kernel): only columns reached over a KEPT edge (the handle's edge-dropout rule, edge_kept) are listed.
// The keep test comes BEFORE the exchange on the stamp: a dropped edge that stamped its column would hide it from a later kept edge to
// the same column, which would find it stamped and never list it.
template <bool MASKED>
__device__ __forceinline__ void frontier_rows_body(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int32_t n_rows, const int32_t *__restrict__ count_b,
    int32_t max_b, int32_t *stamp, int32_t epoch, int32_t *list, int32_t *count_f, const EdgeDrop &dr)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int n_in = *count_b < max_b ? *count_b : max_b;
    // (a grid of at most kFrontierMaxWgs workgroups strides over the input: the second hop's host-side bound is n_rows)
    for (int64_t k = (int64_t)blockIdx.x * kFrontierWaves + (threadIdx.x >> 6); k < n_in; k += (int64_t)gridDim.x * kFrontierWaves) {
        const int r = list[k];
        if (r < 0 || r >= n_rows) continue;                    // never index the matrix out of range
        const int beg = rowptr[r], end = rowptr[r + 1];
        for (int base = beg; base < end; base += kWave) {
            const int e = base + lane;
            int c = -1;
            if (e < end) c = col[e];
            const bool fresh = c >= 0 && c < n_rows && (!MASKED || edge_kept(dr, e)) && atomicExch(stamp + c, epoch) != epoch;    // first visitor of the row this epoch
            const unsigned long long m = __ballot(fresh);
            if (m == 0) continue;
            const int leader = (int)__builtin_ctzll(m);
            int start = 0;
            if (lane == leader) start = atomicAdd(count_f, (int)__builtin_popcountll(m));
            start = __builtin_amdgcn_readlane(start, leader);
            if (fresh) list[start + (int)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = c;
        }
    }
}

__global__ __launch_bounds__(kWave *kFrontierWaves) void frontier_rows_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int32_t n_rows, const int32_t *__restrict__ count_b,
    int32_t max_b, int32_t *stamp, int32_t epoch, int32_t *list, int32_t *count_f)
{
    frontier_rows_body<false>(rowptr, col, n_rows, count_b, max_b, stamp, epoch, list, count_f, EdgeDrop{nullptr, nullptr, 0, 1.0f, 0u, 0u});
}

__global__ __launch_bounds__(kWave *kFrontierWaves) void frontier_rows_masked_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int32_t n_rows, const int32_t *__restrict__ count_b,
    int32_t max_b, int32_t *stamp, int32_t epoch, int32_t *list, int32_t *count_f, const EdgeDrop dr)
{
    frontier_rows_body<true>(rowptr, col, n_rows, count_b, max_b, stamp, epoch, list, count_f, dr);
}

// One 16-wave workgroup per listed row: wave w takes the row's entries w, w + 16, ... (a hub row of 1 000 entries is 64
// atomics per wave, not 1 000 in one).
constexpr int kPushRowsMaxWgs = 1 << 16;

// MASKED (spmm_push_rows_masked_kernel): the lanes that hold a run's (col, val) also decide `kept` (edge_kept: the handle's
// edge-dropout rule, the forward's), a kept value is val / keep_prob, and the entry loop skips a dropped entry on the wave-uniform
// ballot of the kept lanes: a dropped entry issues no atomic at all.
template <bool MASKED>
__device__ __forceinline__ void spmm_push_rows_body(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const int32_t *__restrict__ list, const int32_t *__restrict__ count, int n_rows, const float *__restrict__ src,
    int src_indexed, const float *__restrict__ add, int add_indexed, float scale, float add_scale, float *out, int d, const EdgeDrop &dr)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int n = *count;
    // (a grid of min(max_count, kPushRowsMaxWgs) workgroups strides over the list: a frontier list's host-side bound is n_rows)
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int r = list[k];
        if (r < 0 || r >= n_rows) continue;                    // never index the matrix out of range
        const int beg = rowptr[r], end = rowptr[r + 1];
        for (int c0 = 0; c0 < d; c0 += kWave) {
            const int c = c0 + lane;
            const bool col_ok = c < d;                         // (every lane stays in the loop: lanes 0..15 carry the run's metadata)
            const float g = col_ok ? scale * src[(size_t)(src_indexed ? r : k) * d + c] : 0.0f;
            for (int base = beg + wave * 16; base < end; base += kWgWaves * 16) {   // 16-entry runs: one coalesced (col, val) load each
                const int cnt = end - base < 16 ? end - base : 16;
                int my_col = 0;
                float my_val = 0.0f;
                bool kept = false;
                if (lane < cnt) {
                    my_col = col[base + lane];
                    my_val = val[base + lane];
                    if (MASKED) {
                        kept = edge_kept(dr, base + lane);
                        my_val = kept ? my_val / dr.keep_prob : 0.0f;
                    }
                }
                const unsigned long long kbits = MASKED ? __ballot(kept) : ~0ull;      // (wave-uniform)
                // lane 0 is read before the first atomic and the entry loop is a real loop: see spmm_push_batch_kernel
                const int cc0 = __builtin_amdgcn_readlane(my_col, 0);
                const float v0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val), 0));
                if (col_ok && (!MASKED || (kbits & 1ull))) atomicAdd(out + (size_t)cc0 * d + c, v0 * g);
#pragma unroll 1
                for (int j = 1; j < cnt; ++j) {
                    if (MASKED && !((kbits >> j) & 1ull)) continue;
                    const int cc = __builtin_amdgcn_readlane(my_col, j);
                    const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val), j));
                    if (col_ok) atomicAdd(out + (size_t)cc * d + c, v * g);
                }
            }
            if (add && wave == 0 && col_ok) atomicAdd(out + (size_t)r * d + c, add_scale * add[(size_t)(add_indexed ? r : k) * d + c]);
        }
    }
}

__global__ __launch_bounds__(kWave *kWgWaves) void spmm_push_rows_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const int32_t *__restrict__ list, const int32_t *__restrict__ count, int n_rows, const float *__restrict__ src,
    int src_indexed, const float *__restrict__ add, int add_indexed, float scale, float add_scale, float *out, int d)
{
    spmm_push_rows_body<false>(rowptr, col, val, list, count, n_rows, src, src_indexed, add, add_indexed, scale, add_scale, out, d,
                               EdgeDrop{nullptr, nullptr, 0, 1.0f, 0u, 0u});
}

__global__ __launch_bounds__(kWave *kWgWaves) void spmm_push_rows_masked_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const int32_t *__restrict__ list, const int32_t *__restrict__ count, int n_rows, const float *__restrict__ src,
    int src_indexed, const float *__restrict__ add, int add_indexed, float scale, float add_scale, float *out, int d, const EdgeDrop dr)
{
    spmm_push_rows_body<true>(rowptr, col, val, list, count, n_rows, src, src_indexed, add, add_indexed, scale, add_scale, out, d, dr);
}

// The push over a LONG list (a two-hop frontier F2: 10^5 .. 10^6 rows, median 13 entries) in rowlist_dev_body's work
// split (spmm_chunk.h): a fixed grid of 16-wave workgroups strides over the list in passes of 16 slots, the count is read on the
// device.  Part 1: wave w owns slot w; a row of at most 64 entries is ONE wave task — one coalesced (col, val) load, lane j holding
// entry j, the row's source in lane == column, the atomics back to back.  Part 2: the longer rows of the pass are cut into 64-entry
// wave tasks (a 1 500-entry hub row: 24), dealt round-robin to the 16 waves.  spmm_push_rows_kernel's one workgroup per row leaves
// 15 of 16 waves idle on a 13-entry row and serialises a workgroup's rows.  Every atomic wave-instruction is one contiguous 256-byte
// row of `out`.  d == 64; the source is indexed by row; no add term.
constexpr int kPushListMaxWgs = 2048;

// One wave task: entries [e0, e0 + cnt), cnt <= 64, of a row whose scaled source value this lane holds in g.  MASKED: the lanes that
// hold the run decide `kept` (edge_kept: the handle's edge-dropout rule, the forward's), a kept value is val / keep_prob, and the
// entry loop walks the wave-uniform ballot of the kept lanes: a dropped entry issues no atomic, a run with none kept issues nothing.
// The first entry is read before the first atomic and the entry loop is a real loop: see spmm_push_batch_kernel.
template <bool MASKED>
__device__ __forceinline__ void push_list_task(const int32_t *__restrict__ col, const float *__restrict__ val, int e0, int cnt, int lane, float g,
                                               float *out_l, const EdgeDrop &dr)
{
    int my_col = 0;
    float my_val = 0.0f;
    bool kept = false;
    if (lane < cnt) {
        my_col = col[e0 + lane];
        my_val = val[e0 + lane];
        kept = true;
        if (MASKED) {
            kept = edge_kept(dr, e0 + lane);
            my_val = kept ? my_val / dr.keep_prob : 0.0f;
        }
    }
    unsigned long long todo = MASKED ? __ballot(kept) : (cnt >= kWave ? ~0ull : (1ull << cnt) - 1ull);      // (wave-uniform)
    if (todo == 0) return;
    const int j0 = (int)__builtin_ctzll(todo);
    const int cc0 = __builtin_amdgcn_readlane(my_col, j0);
    const float v0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val), j0));
    atomicAdd(out_l + (size_t)(uint32_t)cc0 * kWave, v0 * g);
    todo &= todo - 1;
#pragma unroll 1
    while (todo) {
        const int j = (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        const int cc = __builtin_amdgcn_readlane(my_col, j);
        const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val), j));
        atomicAdd(out_l + (size_t)(uint32_t)cc * kWave, v * g);
    }
}

template <bool MASKED>
__device__ __forceinline__ void spmm_push_list_body(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, const int32_t *__restrict__ list,
    const int32_t *__restrict__ count, int32_t max_count, int32_t n_rows, const float *__restrict__ src, float scale, float *out,
    const EdgeDrop &dr)
{
    __shared__ int s_nt[kWgWaves];                 // 64-entry tasks of each of the pass's 16 slots (0: no row, or a row of one task)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = *count < max_count ? *count : max_count;
    float *out_l = out + lane;
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
        if (lane == 0) s_nt[wave] = nseg > 1 ? nseg : 0;
        if (r >= 0 && nseg == 1) push_list_task<MASKED>(col, val, beg, deg, lane, scale * src[(size_t)r * kWave + lane], out_l, dr);
        __syncthreads();
        // ---- part 2: the longer rows' tasks, round-robin over the 16 waves (s_nt[j] > 0 only for an in-range row)
        int total = 0;
        for (int j = 0; j < kWgWaves; ++j) total += s_nt[j];
        for (int t = wave; t < total; t += kWgWaves) {
            int j = 0, base = 0;
            while (t >= base + s_nt[j]) base += s_nt[j++];
            const int rj = list[k0 + j];
            const int bj = rowptr[rj], dj = rowptr[rj + 1] - bj, sg = t - base;
            const int cnt = dj - sg * kTaskEntries < kTaskEntries ? dj - sg * kTaskEntries : kTaskEntries;
            push_list_task<MASKED>(col, val, bj + sg * kTaskEntries, cnt, lane, scale * src[(size_t)rj * kWave + lane], out_l, dr);
        }
        __syncthreads();                            // s_nt is rewritten by the next pass
    }
}

__global__ __launch_bounds__(kWave *kWgWaves) void spmm_push_list_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, const int32_t *__restrict__ list,
    const int32_t *__restrict__ count, int32_t max_count, int32_t n_rows, const float *__restrict__ src, float scale, float *out)
{
    spmm_push_list_body<false>(rowptr, col, val, list, count, max_count, n_rows, src, scale, out, EdgeDrop{nullptr, nullptr, 0, 1.0f, 0u, 0u});
}

__global__ __launch_bounds__(kWave *kWgWaves) void spmm_push_list_masked_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, const int32_t *__restrict__ list,
    const int32_t *__restrict__ count, int32_t max_count, int32_t n_rows, const float *__restrict__ src, float scale, float *out,
    const EdgeDrop dr)
{
    spmm_push_list_body<true>(rowptr, col, val, list, count, max_count, n_rows, src, scale, out, dr);
}

// The same product driven by the batch itself, EVERY slot contributing: slot k (row idx_a[k] + off_a, then idx_b[k] + off_b)
// pushes its own source row src[k] — the slot's own gradient row as the scoring kernel leaves it — so rows named by several
// slots simply receive several contributions and nothing has to be deduplicated (a first version tested "is this the first
// slot naming the row" with a scan of the batch in every wave: 128 MB of index reads per launch, 16 us).  kPushParts
// workgroups of 4 waves share a slot's row, entry e going to (part, wave) = (e mod 4, (e div 4) mod 4): the ~50 ns a CU needs
// per 256-byte float atomic would otherwise put a 1 000-entry hub row's atomics on one CU.
constexpr int kPushParts = 4;
constexpr int kPushWaves = 4;

__global__ __launch_bounds__(kWave *kPushWaves) void spmm_push_batch_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows,
    const int64_t *__restrict__ idx_a, int n_a, int64_t off_a, const int64_t *__restrict__ idx_b, int n_b, int64_t off_b,
    const float *__restrict__ src, int ld_src, const float *__restrict__ add, int ld_add, float scale, float *out)
{
    const int k = blockIdx.x / kPushParts, part = blockIdx.x % kPushParts;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long r = batch_row(idx_a, n_a, off_a, idx_b, off_b, k);
    if (r < 0 || r >= n_rows) return;
    const int beg = rowptr[r], end = rowptr[r + 1];
    const float g = scale * src[(size_t)k * ld_src + lane];
    // 16-entry runs dealt round-robin to the slot's 16 waves: ONE coalesced load of the run's (col, val) pairs — lane j holds
    // entry j — then the atomics are issued back to back (they return nothing, so nothing waits).  The first version walked
    // the row entry by entry, each atomic behind its own col/val load: a 500-entry row took ~30 dependent round trips per wave
    // and set the launch time (11-22 us).
    // 16-entry runs dealt round-robin to the slot's 16 waves: ONE coalesced load of a run's (col, val) pairs — lane j holds
    // entry j — and v_readlane hands them to the atomics.  Two things matter for the atomics to leave back to back:
    //   * every run of the wave (4 at a time: rows of up to 1 024 entries in one go) is loaded, and lane 0 of each is read,
    //     BEFORE the first atomic — gfx9 has one vmcnt counter for loads and atomics, and the compiler's wait insertion
    //     re-waits conservatively at every control-flow join while a load is pending: with the read inside the guarded,
    //     unrolled loop it put `s_waitcnt vmcnt(0)` in front of EVERY atomic (each then waited out its predecessor's
    //     ~350 ns round trip: 13.5 us for batches whose longest row had <= 512 entries, 19 us up to 768, 25 us up to 1 024);
    //   * the entry loop is a real loop (dynamic trip count), not 16 guarded copies.
    const int w16 = part * kPushWaves + wave;
    constexpr int kStride = kPushParts * kPushWaves * 16, kPre = 4;
    float *out_l = out + lane;
    for (int base0 = beg + w16 * 16; base0 < end; base0 += kPre * kStride) {
        int my_col[kPre], c0[kPre];
        float my_val[kPre], v0[kPre];
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const int base = base0 + p * kStride;
            my_col[p] = 0;
            my_val[p] = 0.0f;
            if (base + lane < end && lane < 16) {
                my_col[p] = col[base + lane];
                my_val[p] = val[base + lane];
            }
        }
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            c0[p] = __builtin_amdgcn_readlane(my_col[p], 0);
            v0[p] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val[p]), 0));
        }
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const int base = base0 + p * kStride;
            const int cnt = end - base < 16 ? end - base : 16;           // (<= 0 past the row's end)
            if (cnt > 0) atomicAdd(out_l + (size_t)c0[p] * kWave, v0[p] * g);
#pragma unroll 1
            for (int j = 1; j < cnt; ++j) {
                const int c = __builtin_amdgcn_readlane(my_col[p], j);
                const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val[p]), j));
                atomicAdd(out_l + (size_t)c * kWave, v * g);
            }
        }
    }
    if (add && part == 0 && wave == 0) atomicAdd(out + (size_t)r * kWave + lane, scale * add[(size_t)k * ld_add + lane]);
}

// spmm_push_batch_kernel at d = 64 V (V = 2, 4): the same dealing of 16-entry runs, every lane owning columns lane, lane + 64, ..
// — V 256-byte atomics per stored entry (the V column blocks of the row).
template <int V>
__global__ __launch_bounds__(kWave *kPushWaves) void spmm_push_batch_wide_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int n_rows,
    const int64_t *__restrict__ idx_a, int n_a, int64_t off_a, const int64_t *__restrict__ idx_b, int n_b, int64_t off_b,
    const float *__restrict__ src, int ld_src, const float *__restrict__ add, int ld_add, float scale, float *out)
{
    constexpr int kRow = kWave * V;
    const int k = blockIdx.x / kPushParts, part = blockIdx.x % kPushParts;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long r = batch_row(idx_a, n_a, off_a, idx_b, off_b, k);
    if (r < 0 || r >= n_rows) return;
    const int beg = rowptr[r], end = rowptr[r + 1];
    float g[V];
#pragma unroll
    for (int c = 0; c < V; ++c) g[c] = scale * src[(size_t)k * ld_src + c * kWave + lane];
    const int w16 = part * kPushWaves + wave;
    constexpr int kStride = kPushParts * kPushWaves * 16, kPre = 4;
    float *out_l = out + lane;
    for (int base0 = beg + w16 * 16; base0 < end; base0 += kPre * kStride) {
        int my_col[kPre], c0[kPre];
        float my_val[kPre], v0[kPre];
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const int base = base0 + p * kStride;
            my_col[p] = 0;
            my_val[p] = 0.0f;
            if (base + lane < end && lane < 16) {
                my_col[p] = col[base + lane];
                my_val[p] = val[base + lane];
            }
        }
#pragma unroll
        for (int p = 0; p < kPre; ++p) {          // lane 0 of every run before the first atomic: see spmm_push_batch_kernel
            c0[p] = __builtin_amdgcn_readlane(my_col[p], 0);
            v0[p] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val[p]), 0));
        }
#pragma unroll
        for (int p = 0; p < kPre; ++p) {
            const int base = base0 + p * kStride;
            const int cnt = end - base < 16 ? end - base : 16;           // (<= 0 past the row's end)
            if (cnt > 0) {
#pragma unroll
                for (int c = 0; c < V; ++c) atomicAdd(out_l + (size_t)c0[p] * kRow + c * kWave, v0[p] * g[c]);
            }
#pragma unroll 1
            for (int j = 1; j < cnt; ++j) {
                const int cc = __builtin_amdgcn_readlane(my_col[p], j);
                const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val[p]), j));
#pragma unroll
                for (int c = 0; c < V; ++c) atomicAdd(out_l + (size_t)cc * kRow + c * kWave, v * g[c]);
            }
        }
    }
    if (add && part == 0 && wave == 0) {
#pragma unroll
        for (int c = 0; c < V; ++c) atomicAdd(out + (size_t)r * kRow + c * kWave + lane, scale * add[(size_t)k * ld_add + c * kWave + lane]);
    }
}

// Deterministic accumulation of a batch's per-slot rows into a dense table — the atomic-free alternative to the float
// atomics above (SPEX_STEP_DETERMINISTIC).  out[r] = scale * (slots[k1] + slots[k2] + ...) over the slots k1 < k2 < ... that
// name row r, in ASCENDING slot order — the order in which the reference's CPU index backward (index_put_ with accumulate,
// LightGCN_SPEX/code/utility1/model.py:115-116 under autograd) adds them, so results repeat bit for bit from run to run.
// One wave per slot: it scans the batch's row list (64 slots per load), leaves if a lower-numbered slot names the same row,
// otherwise adds the later duplicates in order and writes the row with a plain store (mode 0) or a plain read-modify-write
// (mode 1: the wave owns the row in this launch).  The scan is quadratic in the batch (n^2 * 8 B of L2 reads: 2 MB for the
// reference's 2 x 256 slots), which is what a validation mode can afford; slots == NULL clears the named rows instead.
constexpr int kReduceWaves = 4;

__global__ __launch_bounds__(kWave *kReduceWaves) void reduce_slots_kernel(
    const int64_t *__restrict__ idx_a, int n_a, int64_t off_a, const int64_t *__restrict__ idx_b, int n_b, int64_t off_b,
    int n_rows, const float *__restrict__ slots, int ld_slots, float scale, float *out, int mode)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int k = blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    const int n = n_a + n_b;
    if (k >= n) return;
    const long long r = batch_row(idx_a, n_a, off_a, idx_b, off_b, k);
    if (r < 0 || r >= n_rows) return;
    if (!slots) {                                              // clear form: every slot zeroes its row (idempotent)
        out[(size_t)r * kWave + lane] = 0.0f;
        return;
    }
    for (int base = 0; base < k; base += kWave) {              // a lower-numbered slot with this row owns it
        const int kk = base + lane;
        const bool match = kk < k && batch_row(idx_a, n_a, off_a, idx_b, off_b, kk) == r;
        if (__ballot(match)) return;
    }
    float acc = slots[(size_t)k * ld_slots + lane];
    for (int base = k & ~(kWave - 1); base < n; base += kWave) {
        const int kk = base + lane;
        const bool match = kk > k && kk < n && batch_row(idx_a, n_a, off_a, idx_b, off_b, kk) == r;
        unsigned long long m = __ballot(match);
        while (m) {                                            // ascending slot order
            const int j = (int)__builtin_ctzll(m);
            m &= m - 1;
            acc = acc + slots[(size_t)(base + j) * ld_slots + lane];
        }
    }
    if (scale != 1.0f) acc = acc * scale;
    float *o = out + (size_t)r * kWave + lane;
    *o = mode == 1 ? *o + acc : acc;
}

// reduce_slots_kernel at d = 64 V (V = 2, 4): one wave per slot, every lane owning columns lane, lane + 64, ..; the same scan, the
// same ascending slot order per row, the same clear form.
template <int V>
__global__ __launch_bounds__(kWave *kReduceWaves) void reduce_slots_wide_kernel(
    const int64_t *__restrict__ idx_a, int n_a, int64_t off_a, const int64_t *__restrict__ idx_b, int n_b, int64_t off_b,
    int n_rows, const float *__restrict__ slots, int ld_slots, float scale, float *out, int mode)
{
    constexpr int kRow = kWave * V;
    const int lane = threadIdx.x & (kWave - 1);
    const int k = blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    const int n = n_a + n_b;
    if (k >= n) return;
    const long long r = batch_row(idx_a, n_a, off_a, idx_b, off_b, k);
    if (r < 0 || r >= n_rows) return;
    float *o = out + (size_t)r * kRow + lane;
    if (!slots) {                                              // clear form: every slot zeroes its row (idempotent)
#pragma unroll
        for (int c = 0; c < V; ++c) o[c * kWave] = 0.0f;
        return;
    }
    for (int base = 0; base < k; base += kWave) {              // a lower-numbered slot with this row owns it
        const int kk = base + lane;
        const bool match = kk < k && batch_row(idx_a, n_a, off_a, idx_b, off_b, kk) == r;
        if (__ballot(match)) return;
    }
    float acc[V];
#pragma unroll
    for (int c = 0; c < V; ++c) acc[c] = slots[(size_t)k * ld_slots + c * kWave + lane];
    for (int base = k & ~(kWave - 1); base < n; base += kWave) {
        const int kk = base + lane;
        const bool match = kk > k && kk < n && batch_row(idx_a, n_a, off_a, idx_b, off_b, kk) == r;
        unsigned long long m = __ballot(match);
        while (m) {                                            // ascending slot order
            const int j = (int)__builtin_ctzll(m);
            m &= m - 1;
#pragma unroll
            for (int c = 0; c < V; ++c) acc[c] = acc[c] + slots[(size_t)(base + j) * ld_slots + c * kWave + lane];
        }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const float a = scale != 1.0f ? acc[c] * scale : acc[c];
        o[c * kWave] = mode == 1 ? o[c * kWave] + a : a;
    }
}

// out[0] (+)= x[0] + x[1] + ... + x[n - 1], added in index order by one thread-free wave pattern: lane j sums x[j], x[j + 64], ...
// and the 64 partials are combined by the fixed DPP tree — the same order adam_kernel uses for a step's per-sample losses.
__global__ __launch_bounds__(kWave) void sum_ordered_kernel(const float *__restrict__ x, int n, float scale, float *out, int accumulate)
{
    float t = 0.0f;
    for (int i = threadIdx.x; i < n; i += kWave) t += x[i];
    t = wave_sum_f32(t);
    if (threadIdx.x == 0) *out = accumulate ? *out + t * scale : t * scale;
}

// Sum of n_parts partial blocks of n floats, in part order (deterministic): out[i] (+)= sum_k parts[k][i].
__global__ __launch_bounds__(256) void sum_parts_kernel(const float *__restrict__ parts, int n_parts, int64_t stride, int n, float *out,
                                                        int accumulate)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float g = 0.0f;
    for (int k = 0; k < n_parts; ++k) g += parts[(size_t)k * stride + i];
    out[i] = accumulate ? out[i] + g : g;
}

}  // namespace

extern "C" int spex_reduce_slots_f32(const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b,
                                     int32_t n_rows, const float *slots, int32_t ld_slots, float scale, float *out, int32_t mode,
                                     int32_t d, void *stream)
{
    SPEX_CHECK_ARG(n_a >= 0 && n_b >= 0 && (n_a == 0 || idx_a) && (n_b == 0 || idx_b), "spex_reduce_slots_f32: bad index lists");
    SPEX_CHECK_ARG(out && n_rows >= 0 && (mode == 0 || mode == 1) && (!slots || ld_slots >= d), "spex_reduce_slots_f32: out=%p mode=%d ld=%d",
                   (void *)out, mode, ld_slots);
    if (d != kWave && d != 2 * kWave && d != 4 * kWave) {
        spex::set_error("spex_reduce_slots_f32: d = 64, 128 or 256 only (got %d)", d);
        return SPEX_ERR_UNSUPPORTED;
    }
    const int n = n_a + n_b;
    if (n == 0 || n_rows == 0) return SPEX_OK;
#define SPEX_GO(KERNEL)                                                                                                                \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)((n + kReduceWaves - 1) / kReduceWaves)), dim3(kWave * kReduceWaves), 0, (hipStream_t)stream, \
                       idx_a, n_a, off_a, idx_b, n_b, off_b, n_rows, slots, ld_slots, scale, out, mode)
    if (d == kWave) SPEX_GO(reduce_slots_kernel);
    else if (d == 2 * kWave) SPEX_GO(reduce_slots_wide_kernel<2>);
    else SPEX_GO(reduce_slots_wide_kernel<4>);
#undef SPEX_GO
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

int spex::sum_ordered(const float *x, int32_t n, float scale, float *out, int accumulate, void *stream)
{
    hipLaunchKernelGGL(sum_ordered_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, x, n, scale, out, accumulate);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

int spex::sum_parts(const float *parts, int32_t n_parts, int64_t stride, int32_t n, float *out, int accumulate, void *stream)
{
    if (n <= 0) return SPEX_OK;
    hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, parts, n_parts, stride, n, out,
                       accumulate);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_unique_rows_i32(const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b,
                                    int64_t off_b, int32_t n_rows, int32_t *stamp, int32_t epoch, int32_t *list, int32_t *count,
                                    void *stream)
{
    SPEX_CHECK_ARG(n_a >= 0 && n_b >= 0 && (n_a == 0 || idx_a) && (n_b == 0 || idx_b), "spex_unique_rows_i32: bad index lists");
    SPEX_CHECK_ARG(stamp && list && count && n_rows >= 0 && epoch != 0, "spex_unique_rows_i32: NULL buffer or epoch 0");
    SPEX_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), (hipStream_t)stream));
    if (n_a + n_b == 0) return SPEX_OK;
    hipLaunchKernelGGL(unique_rows_kernel, dim3((unsigned)((n_a + n_b + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx_a, n_a,
                       off_a, idx_b, n_b, off_b, n_rows, stamp, epoch, list, count);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

static int push_rows(const char *who, const spex_graph_t *g, const int32_t *list, const int32_t *count, int32_t max_count, const float *src,
                     int32_t src_indexed, const float *add, int32_t add_indexed, float scale, float add_scale, float *out, int32_t d,
                     void *stream)
{
    SPEX_CHECK_ARG(g && list && count && src && out, "%s: NULL argument", who);
    SPEX_CHECK_ARG(max_count >= 0 && d >= 1, "%s: max_count=%d d=%d", who, max_count, d);
    if (max_count == 0 || g->n_rows == 0) return SPEX_OK;
    const dim3 grid((unsigned)(max_count < kPushRowsMaxWgs ? max_count : kPushRowsMaxWgs));
    if (g->mask_mode != 0)      // the handle's edge-dropout rule per entry: a kernel of its own
        hipLaunchKernelGGL(spmm_push_rows_masked_kernel, grid, dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->val, list, count,
                           g->n_rows, src, src_indexed, add, add_indexed, scale, add_scale, out, d, edge_drop_of(g));
    else
        hipLaunchKernelGGL(spmm_push_rows_kernel, grid, dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->val, list, count,
                           g->n_rows, src, src_indexed, add, add_indexed, scale, add_scale, out, d);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

// spex_unique_rows_i32 without the reset of *count: further index lists of the same epoch appended to the same list.
int spex::unique_rows_more(const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b, int32_t n_b, int64_t off_b, int32_t n_rows,
                           int32_t *stamp, int32_t epoch, int32_t *list, int32_t *count, void *stream)
{
    if (n_a + n_b <= 0) return SPEX_OK;
    hipLaunchKernelGGL(unique_rows_kernel, dim3((unsigned)((n_a + n_b + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx_a, n_a,
                       off_a, idx_b, n_b, off_b, n_rows, stamp, epoch, list, count);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_spmm_push_rows_f32(const spex_graph_t *g, const int32_t *list, const int32_t *count, int32_t max_count,
                                       const float *src, int32_t src_indexed, const float *add, int32_t add_indexed, float scale,
                                       float *out, int32_t d, void *stream)
{
    return push_rows("spex_spmm_push_rows_f32", g, list, count, max_count, src, src_indexed, add, add_indexed, scale, scale, out, d, stream);
}

// spex_spmm_push_rows_f32 with a factor of its own for the `add` term: out += scale * A^T scatter(src) + add_scale * scatter(add) —
// G_(l-1) = g / (L + 1) + A^T G_l over a frontier list is scale = 1, add_scale = 1 / (L + 1).
extern "C" int spex_spmm_push_rows_scaled_f32(const spex_graph_t *g, const int32_t *list, const int32_t *count, int32_t max_count,
                                              const float *src, int32_t src_indexed, const float *add, int32_t add_indexed, float scale,
                                              float add_scale, float *out, int32_t d, void *stream)
{
    return push_rows("spex_spmm_push_rows_scaled_f32", g, list, count, max_count, src, src_indexed, add, add_indexed, scale, add_scale, out, d,
                     stream);
}

// out[col[e], :] += scale * val[e] * src[r, :] for every stored entry e of every row r = list[k], k < min(*count, max_count), in the
// long-list work split (spmm_push_list_kernel); follows the handle's edge-dropout rule as spex_spmm_push_rows_f32 does.
extern "C" int spex_spmm_push_list_f32(const spex_graph_t *g, const int32_t *list, const int32_t *count, int32_t max_count, const float *src,
                                       float scale, float *out, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && list && count && src && out, "spex_spmm_push_list_f32: NULL argument");
    SPEX_CHECK_ARG(max_count >= 0 && src != out, "spex_spmm_push_list_f32: max_count=%d, or src aliases out", max_count);
    if (d != kWave) {
        spex::set_error("spex_spmm_push_list_f32: d == 64 only (got %d)", d);
        return SPEX_ERR_UNSUPPORTED;
    }
    if (max_count == 0 || g->n_rows == 0) return SPEX_OK;
    const int64_t wgs = ((int64_t)max_count + kWgWaves - 1) / kWgWaves;
    const dim3 grid((unsigned)(wgs < kPushListMaxWgs ? wgs : kPushListMaxWgs));
    if (g->mask_mode != 0)      // the handle's edge-dropout rule per entry: a kernel of its own
        hipLaunchKernelGGL(spmm_push_list_masked_kernel, grid, dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->val, list, count,
                           max_count, g->n_rows, src, scale, out, edge_drop_of(g));
    else
        hipLaunchKernelGGL(spmm_push_list_kernel, grid, dim3(kWave * kWgWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->val, list, count,
                           max_count, g->n_rows, src, scale, out);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

static int frontier_rows(const char *who, bool masked, const spex_graph_t *g, int32_t *list, const int32_t *count_b, int32_t max_b, int32_t *stamp,
                         int32_t epoch, int32_t *count_f, void *stream)
{
    SPEX_CHECK_ARG(g && list && count_b && stamp && count_f && count_f != count_b, "%s: NULL buffer, or count_f == count_b", who);
    SPEX_CHECK_ARG(max_b >= 0 && epoch != 0, "%s: max_b=%d epoch=%d", who, max_b, epoch);
    SPEX_CHECK_ARG(g->n_rows == g->n_cols, "%s: the list indexes rows and columns alike: a square graph (%d x %d)", who, g->n_rows, g->n_cols);
    hipLaunchKernelGGL(frontier_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, count_b, count_f);
    SPEX_HIP(hipGetLastError());
    if (max_b == 0 || g->n_rows == 0) return SPEX_OK;
    const int64_t wgs = ((int64_t)max_b + kFrontierWaves - 1) / kFrontierWaves;
    const dim3 grid((unsigned)(wgs < kFrontierMaxWgs ? wgs : kFrontierMaxWgs));
    if (masked && g->mask_mode != 0)
        hipLaunchKernelGGL(frontier_rows_masked_kernel, grid, dim3(kWave * kFrontierWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->n_rows, count_b,
                           max_b, stamp, epoch, list, count_f, edge_drop_of(g));
    else
        hipLaunchKernelGGL(frontier_rows_kernel, grid, dim3(kWave * kFrontierWaves), 0, (hipStream_t)stream, g->rowptr, g->col, g->n_rows, count_b, max_b,
                           stamp, epoch, list, count_f);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_frontier_rows_i32(const spex_graph_t *g, int32_t *list, const int32_t *count_b, int32_t max_b, int32_t *stamp,
                                      int32_t epoch, int32_t *count_f, void *stream)
{
    return frontier_rows("spex_frontier_rows_i32", false, g, list, count_b, max_b, stamp, epoch, count_f, stream);
}

// spex_frontier_rows_i32 under the handle's edge-dropout rule: only columns reached over a kept entry are listed (mask mode 0: the
// same list).  The frontier of a masked step.
extern "C" int spex_frontier_rows_masked_i32(const spex_graph_t *g, int32_t *list, const int32_t *count_b, int32_t max_b, int32_t *stamp,
                                             int32_t epoch, int32_t *count_f, void *stream)
{
    return frontier_rows("spex_frontier_rows_masked_i32", true, g, list, count_b, max_b, stamp, epoch, count_f, stream);
}

extern "C" int spex_spmm_push_batch_f32(const spex_graph_t *g, const int64_t *idx_a, int32_t n_a, int64_t off_a, const int64_t *idx_b,
                                        int32_t n_b, int64_t off_b, const float *src, int32_t ld_src, const float *add, int32_t ld_add,
                                        float scale, float *out, int32_t d, void *stream)
{
    SPEX_CHECK_ARG(g && src && out, "spex_spmm_push_batch_f32: NULL argument");
    SPEX_CHECK_ARG(n_a >= 0 && n_b >= 0 && (n_a == 0 || idx_a) && (n_b == 0 || idx_b), "spex_spmm_push_batch_f32: bad index lists");
    SPEX_CHECK_ARG(g->mask_mode == 0, "spex_spmm_push_batch_f32: edge dropout is not supported in push form");
    if (d != kWave && d != 2 * kWave && d != 4 * kWave) {
        spex::set_error("spex_spmm_push_batch_f32: d = 64, 128 or 256 only (got %d)", d);
        return SPEX_ERR_UNSUPPORTED;
    }
    SPEX_CHECK_ARG(ld_src >= d && (!add || ld_add >= d), "spex_spmm_push_batch_f32: ld_src=%d ld_add=%d", ld_src, ld_add);
    if (n_a + n_b == 0 || g->n_rows == 0) return SPEX_OK;
#define SPEX_GO(KERNEL)                                                                                                                   \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)(n_a + n_b) * kPushParts), dim3(kWave * kPushWaves), 0, (hipStream_t)stream, g->rowptr, g->col, \
                       g->val, g->n_rows, idx_a, n_a, off_a, idx_b, n_b, off_b, src, ld_src, add, ld_add, scale, out)
    if (d == kWave) SPEX_GO(spmm_push_batch_kernel);
    else if (d == 2 * kWave) SPEX_GO(spmm_push_batch_wide_kernel<2>);
    else SPEX_GO(spmm_push_batch_wide_kernel<4>);
#undef SPEX_GO
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

// x[0 : n] = 0 as a kernel launch (hipMemsetAsync costs the host ~10 us a call on this runtime; a launch ~1-2).
namespace {
__global__ __launch_bounds__(256) void zero_kernel(float *__restrict__ x, int64_t n4, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
        reinterpret_cast<float4 *>(x)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (blockIdx.x == 0)
        for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) x[i] = 0.0f;
}
}  // namespace

int spex::zero_f32(float *x, int64_t n, void *stream)
{
    if (n <= 0) return SPEX_OK;
    if ((((uintptr_t)x) & 15) != 0) {
        SPEX_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(float), (hipStream_t)stream));
        return SPEX_OK;
    }
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n4, n);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}
