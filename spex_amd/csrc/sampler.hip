// Negative sampler on the GPU — SURVEY.md 8f "next" #2.
//
// Replaces LightTrainData.ng_sample, LightGCN_SPEX/code/utility1/dataloader.py:250-265: for every positive (u, i) draw
// num_ng items j uniformly from [0, num_item), redrawing while (u, j) is a training interaction.  The reference walks
// 1 M draws in a Python loop against a dok matrix (~27 s per Epinion2 epoch).  Here one thread owns one slot: a
// counter-based draw (philox4x32-10 keyed by the seed, counter = (slot, attempt)) mapped to [0, num_item) by a
// multiply-high, and a binary search in the user's sorted item list (CSR of R).  The distribution is the reference's
// (uniform over the user's non-interacted items); the stream is not NumPy's Mersenne Twister, so for the same seed the
// individual negatives differ — the drop-in Loader keeps its exact-replay host sampler as the default and offers this
// one as `ng_sample(device=...)`.
#include "spex_common.h"

namespace {

__device__ __forceinline__ uint32_t philox2(uint32_t c0_, uint32_t c1_, uint32_t k0, uint32_t k1)
{
    uint32_t c0 = c0_, c1 = c1_, c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

__global__ __launch_bounds__(256) void sample_negatives_kernel(const int32_t *__restrict__ rowptr,
                                                               const int32_t *__restrict__ items,
                                                               const int64_t *__restrict__ pos_user, int64_t n_slots,
                                                               int num_ng, int num_item, int n_user_rows, uint32_t seed_lo,
                                                               uint32_t seed_hi, int64_t *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; slot < n_slots; slot += stride) {
        const int64_t u = pos_user[slot / num_ng];
        int beg = 0, end = 0;
        if (u >= 0 && u < n_user_rows) {
            beg = rowptr[u];
            end = rowptr[u + 1];
        }
        int j = 0;
        bool done = false;
        // Rejection sampling, bounded: a user who has interacted with most of the catalogue would redraw for a long
        // time (for ever, in the reference, if with all of it).  After 16 rejections fall back to drawing the k-th
        // admissible item directly (same uniform law, one more binary search).
        for (uint32_t attempt = 0; attempt < 16u; ++attempt) {
            const uint32_t x = philox2((uint32_t)slot, ((uint32_t)(slot >> 32) << 8) | attempt, seed_lo, seed_hi);
            j = (int)(((uint64_t)x * (uint64_t)(uint32_t)num_item) >> 32);
            int lo = beg, hi = end;  // binary search for j in items[beg, end)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (items[mid] < j) lo = mid + 1;
                else hi = mid;
            }
            if (!(lo < end && items[lo] == j)) {
                done = true;
                break;
            }
        }
        if (!done) {
            const int deg = end - beg, admissible = num_item - deg;
            if (admissible > 0) {
                const uint32_t x = philox2((uint32_t)slot, ((uint32_t)(slot >> 32) << 8) | 255u, seed_lo, seed_hi);
                const int k = (int)(((uint64_t)x * (uint64_t)(uint32_t)admissible) >> 32);   // k-th admissible item
                int lo = 0, hi = deg;  // first position m with items[beg+m] - m > k  (admissible items below it)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (items[beg + mid] - mid > k) hi = mid;
                    else lo = mid + 1;
                }
                j = k + lo;
            } else {
                j = 0;  // the user has every item: no valid negative exists (the reference would not terminate)
            }
        }
        out[slot] = j;
    }
}

// ---- BPR triples (include/spex_hip.h: spex_sample_bpr_triples states the stream word by word; tests restate it from there)
struct Philox4 {
    uint32_t w[4];
};

// Standard Philox4x32-10: counter (c0, c1, c2, c3), key (k0, k1); all four output words.
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// A uniform word onto [0, m), m >= 1, by multiply-high.
__device__ __forceinline__ int to_range(uint32_t w, int m)
{
    return (int)(((uint64_t)w * (uint64_t)(uint32_t)m) >> 32);
}

// j is among the ascending items[beg, end)
__device__ __forceinline__ bool row_has(const int32_t *__restrict__ items, int beg, int end, int j)
{
    int lo = beg, hi = end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (items[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && items[lo] == j;
}

__global__ __launch_bounds__(256) void sample_bpr_triples_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ items,
                                                                 int n_user_rows, const int32_t *__restrict__ active, int n_active,
                                                                 int num_item, int64_t n, int mode, uint32_t seed_lo, uint32_t seed_hi,
                                                                 uint32_t epoch, int64_t *__restrict__ users, int64_t *__restrict__ pos,
                                                                 int64_t *__restrict__ neg)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int nnz = rowptr[n_user_rows];
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; slot < n; slot += stride) {
        const uint32_t s_lo = (uint32_t)slot, s_hi = (uint32_t)(slot >> 32);
        const Philox4 r0 = philox4x32_10(s_lo, s_hi, epoch, 0u, seed_lo, seed_hi);
        int u = 0, beg = 0, end = 0, p = 0;
        if (mode == 0) {
            u = active[to_range(r0.w[0], n_active)];
            if (u >= 0 && u < n_user_rows) {
                beg = rowptr[u];
                end = rowptr[u + 1];
            }
            if (end > beg) p = items[beg + to_range(r0.w[1], end - beg)];
        } else if (nnz > 0 && n_user_rows > 0) {
            const int e = to_range(r0.w[0], nnz);
            int lo = 0, hi = n_user_rows;          // first row index with rowptr[.] > e, over rowptr[1 .. n_user_rows]: the row that holds e
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (rowptr[mid + 1] > e) hi = mid;
                else lo = mid + 1;
            }
            u = lo;
            beg = rowptr[u];
            end = rowptr[u + 1];
            p = items[e];
        }
        // the negative: bounded rejection (candidates 0 .. 5), then the direct draw of the k-th admissible item — the same uniform
        // law, and it terminates for a user who holds most of the catalogue
        int j = to_range(r0.w[2], num_item);
        bool done = !row_has(items, beg, end, j);
        if (!done) {
            j = to_range(r0.w[3], num_item);
            done = !row_has(items, beg, end, j);
        }
        if (!done) {
            const Philox4 r1 = philox4x32_10(s_lo, s_hi, epoch, 1u, seed_lo, seed_hi);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (!done) {
                    j = to_range(r1.w[a], num_item);
                    done = !row_has(items, beg, end, j);
                }
            }
        }
        if (!done) {
            const int deg = end - beg, admissible = num_item - deg;
            if (admissible > 0) {
                const Philox4 r2 = philox4x32_10(s_lo, s_hi, epoch, 2u, seed_lo, seed_hi);
                const int k = to_range(r2.w[0], admissible);
                int lo = 0, hi = deg;  // first position m with items[beg+m] - m > k  (admissible items below it)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (items[beg + mid] - mid > k) hi = mid;
                    else lo = mid + 1;
                }
                j = k + lo;
            } else {
                j = 0;  // the user has every item: no valid negative exists
            }
        }
        users[slot] = u;
        pos[slot] = p;
        neg[slot] = j;
    }
}

// ---- BCE epochs (include/spex_hip.h: spex_sample_bce_epoch states the stream word by word; tests restate it from there)
// MurmurHash3's 32-bit finaliser
__device__ __forceinline__ uint32_t fmix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// The shuffle's six round keys: uniform per launch, drawn once on the host by the entry point (kernel arguments: no registers).
struct BceRoundKeys {
    uint32_t k[6];
};

// One thread per OUTPUT slot: the keyed bijection perm (a balanced Feistel network on 2 h bits, cycle-walked back into [0, n)) names
// the source sample the slot holds, so the epoch is written already shuffled — no sort, no second pass.  Sources [0, P) are the
// positives in the caller's order, source P + k is negative k % num_ng of positive k / num_ng (ng_sample's order), its draw keyed by k.
__global__ __launch_bounds__(256) void sample_bce_epoch_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ items,
                                                               int n_user_rows, const int32_t *__restrict__ pos_user,
                                                               const int32_t *__restrict__ pos_item, uint32_t n_pos, uint32_t num_ng,
                                                               int num_item, uint32_t n, uint32_t h, BceRoundKeys keys, uint32_t seed_lo,
                                                               uint32_t seed_hi, uint32_t epoch, int64_t *__restrict__ users,
                                                               int64_t *__restrict__ items_out, float *__restrict__ labels)
{
    const uint32_t stride = gridDim.x * blockDim.x, mask = (1u << h) - 1u;      // (h <= 16; n < 2^31: slot + stride cannot wrap)
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < n; slot += stride) {
        uint32_t x = slot;
        do {                       // a permutation of [0, 2^(2 h)) walked from inside [0, n) comes back inside: no cap needed
            uint32_t l = x >> h, r = x & mask;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const uint32_t f = l ^ (fmix32(r ^ keys.k[q]) & mask);
                l = r;
                r = f;
            }
            x = (l << h) | r;
        } while (x >= n);
        if (x < n_pos) {
            users[slot] = pos_user[x];
            items_out[slot] = pos_item[x];
            labels[slot] = 1.0f;
            continue;
        }
        const uint32_t k = x - n_pos;
        const int u = pos_user[k / num_ng];
        int beg = 0, end = 0;
        if (u >= 0 && u < n_user_rows) {
            beg = rowptr[u];
            end = rowptr[u + 1];
        }
        // bounded rejection (candidates 0 .. 7), then the direct draw of the k-th admissible item — the same uniform law, and it
        // terminates for a user who holds most of the catalogue
        int j = 0;
        bool done = false;
        for (uint32_t stage = 0; stage < 2u && !done; ++stage) {
            const Philox4 c = philox4x32_10(k, 0u, epoch, stage, seed_lo, seed_hi);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (!done) {
                    j = to_range(c.w[a], num_item);
                    done = !row_has(items, beg, end, j);
                }
            }
        }
        if (!done) {
            const int deg = end - beg, admissible = num_item - deg;
            if (admissible > 0) {
                const Philox4 r2 = philox4x32_10(k, 0u, epoch, 2u, seed_lo, seed_hi);
                const int kth = to_range(r2.w[0], admissible);
                int lo = 0, hi = deg;  // first position m with items[beg+m] - m > kth  (admissible items below it)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (items[beg + mid] - mid > kth) hi = mid;
                    else lo = mid + 1;
                }
                j = kth + lo;
            } else {
                j = 0;  // the user has every item: no valid negative exists
            }
        }
        users[slot] = u;
        items_out[slot] = j;
        labels[slot] = 0.0f;
    }
}

// ---- NGCF epochs (include/spex_hip.h: spex_sample_ngcf_epoch states the law word by word; tests restate it from there)
// h = max(1, ceil(bits / 2)), bits the bit length of m - 1: the Feistel halves of the domain [0, m), m >= 1
__device__ __forceinline__ uint32_t feistel_half_bits(uint32_t m)
{
    const uint32_t bits = m <= 1u ? 0u : 32u - (uint32_t)__clz((int)(m - 1u));
    return bits <= 2u ? 1u : (bits + 1u) / 2u;
}

// One thread per OUTPUT slot, as in sample_bce_epoch_kernel: perm names the source sample the slot holds.  The sources are grouped by
// user — user q owns [6 pos_off[q], 6 pos_off[q + 1]), its 5 c_q negatives first — so a thread finds its user by a binary search over
// pos_off with the source's positive index x / 6 (every block starts at a multiple of 6), ~12 dependent reads of a table that stays
// in L2.  A negative is the image of its index under the user's own keyed bijection of [0, n_q): the first 5 c_q images are distinct,
// which is random.sample's law with no state shared between the threads of one user.
__global__ __launch_bounds__(256) void sample_ngcf_epoch_kernel(const int32_t *__restrict__ pop, int n_pop, const int32_t *__restrict__ user,
                                                                int n_users, const int32_t *__restrict__ pos_off,
                                                                const int32_t *__restrict__ pos_item, uint32_t n_pos,
                                                                const int32_t *__restrict__ row_off, const int32_t *__restrict__ row_rank,
                                                                uint32_t n, uint32_t h, BceRoundKeys keys, uint32_t seed_lo, uint32_t seed_hi,
                                                                uint32_t epoch, int64_t *__restrict__ users, int64_t *__restrict__ items_out,
                                                                float *__restrict__ labels)
{
    const uint32_t stride = gridDim.x * blockDim.x, mask = (1u << h) - 1u;      // (h <= 16; n < 2^31: slot + stride cannot wrap)
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < n; slot += stride) {
        uint32_t x = slot;
        do {
            uint32_t l = x >> h, r = x & mask;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const uint32_t f = l ^ (fmix32(r ^ keys.k[a]) & mask);
                l = r;
                r = f;
            }
            x = (l << h) | r;
        } while (x >= n);
        const int p = (int)(x / 6u);                      // p < n_pos: the first q with pos_off[q + 1] > p owns the source
        int lo = 0, hi = n_users - 1;                     // (pos_off[n_users] = n_pos > p: q = n_users - 1 at the latest)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pos_off[mid + 1] > p) hi = mid;
            else lo = mid + 1;
        }
        const int q = lo, beg = pos_off[q];
        const int c = pos_off[q + 1] - beg;
        const uint32_t i = x - 6u * (uint32_t)beg, k = 5u * (uint32_t)(c > 0 ? c : 0);     // (offsets that keep their promises: i < 6 c)
        int64_t item = 0;
        if (i >= k) {
            const uint32_t at = (uint32_t)beg + (i - k);
            if (at < n_pos) item = pos_item[at];
            users[slot] = user[q];
            items_out[slot] = item;
            labels[slot] = 1.0f;
            continue;
        }
        const int rbeg = row_off[q];
        int m = row_off[q + 1] - rbeg;
        if (m < 0) m = 0;
        const int n_q = n_pop - m;
        if (n_q > 0 && i < (uint32_t)n_q) {
            const Philox4 ka = philox4x32_10((uint32_t)q, 0u, epoch, 5u, seed_lo, seed_hi), kb = philox4x32_10((uint32_t)q, 1u, epoch, 5u, seed_lo, seed_hi);
            const uint32_t key[6] = {ka.w[0], ka.w[1], ka.w[2], ka.w[3], kb.w[0], kb.w[1]};
            const uint32_t hq = feistel_half_bits((uint32_t)n_q), mq = (1u << hq) - 1u;
            uint32_t r_ = i;
            do {
                uint32_t l = r_ >> hq, r = r_ & mq;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const uint32_t f = l ^ (fmix32(r ^ key[a]) & mq);
                    l = r;
                    r = f;
                }
                r_ = (l << hq) | r;
            } while (r_ >= (uint32_t)n_q);
            const int rr = (int)r_;
            int blo = 0, bhi = m;                          // first t with row_rank[rbeg + t] - t > rr: the positives' ranks at or below
            while (blo < bhi) {
                const int mid = (blo + bhi) >> 1;
                if (row_rank[rbeg + mid] - mid > rr) bhi = mid;
                else blo = mid + 1;
            }
            item = pop[rr + blo];                          // rr < n_pop - m and blo <= m: inside the population
        }
        users[slot] = user[q];
        items_out[slot] = item;
        labels[slot] = 0.0f;
    }
}

// ---- dual-task trust paths (include/spex_hip.h: spex_sample_dual_task_paths states the law word by word; tests restate it from there)
// One 256-thread workgroup per batch.  LDS at capacity CAP (the largest batch the instance serves): the batch's users as int32
// (-1: outside the tables), an open-addressing table of 2 CAP sample positions, the per-sample candidate counts (then their
// exclusive prefix sums), 256 cells for the block scan (then the chosen paths of 256 slots) and the total.
template <int CAP>
struct DualPathsLds {
    int32_t user[CAP];
    int32_t table[2 * CAP];
    uint32_t off[CAP];
    uint32_t part[256];
    uint32_t total;
};

// first(j) by an open-addressing table keyed by the user of the position a cell holds: a cell, once taken, only ever holds positions
// of ONE user (atomicMin among them), so the minimum position per user — all the law reads — does not depend on arrival order.
// Only users with at least one path are entered; 2 CAP cells for at most CAP keys: a probe always meets the key or an empty cell.
template <int CAP>
__global__ __launch_bounds__(256) void sample_dual_paths_kernel(const int64_t *__restrict__ users, int64_t n, int B,
                                                                const int32_t *__restrict__ path_rowptr, int n_user_rows,
                                                                const int32_t *__restrict__ path_idx, int n_paths,
                                                                const int64_t *__restrict__ paths, int path_len,
                                                                const int64_t *__restrict__ path_l, const int64_t *__restrict__ path_tgt,
                                                                int cap, uint32_t seed_lo, uint32_t seed_hi, uint32_t epoch,
                                                                int64_t *__restrict__ seq, int64_t *__restrict__ seq_l,
                                                                int64_t *__restrict__ targets, int32_t *__restrict__ count)
{
    __shared__ DualPathsLds<CAP> s;
    constexpr uint32_t kCells = 2u * CAP;
    const int tid = threadIdx.x;
    const uint32_t k = blockIdx.x;
    const int64_t b0 = (int64_t)k * B;
    if (cap == 0) {                                       // (uniform) nothing to choose: the count alone
        if (tid == 0) count[k] = 0;
        return;
    }
    const int nb = (int)(n - b0 < (int64_t)B ? n - b0 : (int64_t)B);          // 1 <= nb <= B <= CAP
    for (uint32_t c = tid; c < kCells; c += 256) s.table[c] = -1;
    for (int j = tid; j < nb; j += 256) {
        const int64_t u = users[b0 + j];
        int cnt = 0;
        if (u >= 0 && u < n_user_rows) {
            cnt = path_rowptr[u + 1] - path_rowptr[u];
            if (cnt < 0) cnt = 0;
        }
        s.user[j] = cnt > 0 ? (int)u : -1;                 // a user without paths takes no part
        s.off[j] = (uint32_t)cnt;
    }
    __syncthreads();
    for (int j = tid; j < nb; j += 256) {
        const int u = s.user[j];
        if (u < 0) continue;
        uint32_t c = fmix32((uint32_t)u) & (kCells - 1u);
        for (;;) {
            const int prev = atomicCAS(&s.table[c], -1, j);
            if (prev == -1) break;                         // the cell is this user's now
            if (s.user[prev] == u) {
                atomicMin(&s.table[c], j);
                break;
            }
            c = (c + 1u) & (kCells - 1u);
        }
    }
    __syncthreads();
    for (int j = tid; j < nb; j += 256) {
        const int u = s.user[j];
        if (u < 0) continue;
        uint32_t c = fmix32((uint32_t)u) & (kCells - 1u);
        int at = s.table[c];
        while (at != -1 && s.user[at] != u) {
            c = (c + 1u) & (kCells - 1u);
            at = s.table[c];
        }
        if (at != j) s.off[j] = 0u;                        // an earlier sample holds the same user
    }
    __syncthreads();
    // exclusive prefix sums of the counts in order of j: a thread's run of `per` consecutive entries, the 256 run sums scanned in LDS
    const int per = (nb + 255) >> 8;
    const int j0 = tid * per, j1 = j0 + per < nb ? j0 + per : nb;
    uint32_t run = 0u;
    for (int j = j0; j < j1; ++j) run += s.off[j];
    s.part[tid] = run;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t add = tid >= d ? s.part[tid - d] : 0u;
        __syncthreads();
        s.part[tid] += add;
        __syncthreads();
    }
    uint32_t before = s.part[tid] - run;
    if (tid == 255) s.total = s.part[255];
    for (int j = j0; j < j1; ++j) {
        const uint32_t c = s.off[j];
        s.off[j] = before;
        before += c;
    }
    __syncthreads();
    const uint32_t total = s.total;
    const uint32_t T = total < (uint32_t)cap ? total : (uint32_t)cap;
    if (tid == 0) count[k] = (int32_t)T;
    if (T == 0u) return;
    // total > cap: slot t holds candidate perm_k(t) — the BCE sampler's Feistel network on [0, total), keyed by the batch
    const bool cut = total > (uint32_t)cap;
    uint32_t h = 1u, key[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (cut) {
        const uint32_t bits = 32u - (uint32_t)__clz((int)(total - 1u));        // (total >= 2 here)
        h = bits <= 2u ? 1u : (bits + 1u) / 2u;
        const Philox4 a = philox4x32_10(k, 0u, epoch, 4u, seed_lo, seed_hi), b = philox4x32_10(k, 1u, epoch, 4u, seed_lo, seed_hi);
        key[0] = a.w[0]; key[1] = a.w[1]; key[2] = a.w[2]; key[3] = a.w[3]; key[4] = b.w[0]; key[5] = b.w[1];
    }
    const uint32_t mask = (1u << h) - 1u;
    const int64_t row0 = (int64_t)k * cap;
    for (uint32_t base = 0u; base < T; base += 256u) {         // (uniform bounds: the barriers inside are met by every thread)
        const uint32_t t = base + (uint32_t)tid;
        int p = -1;
        if (t < T) {
            uint32_t q = t;
            if (cut) {
                do {
                    uint32_t l = q >> h, r = q & mask;
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        const uint32_t f = l ^ (fmix32(r ^ key[i]) & mask);
                        l = r;
                        r = f;
                    }
                    q = (l << h) | r;
                } while (q >= total);
            }
            int lo = 0, hi = nb;                             // the last j with off[j] <= q: first j with off[j] > q, minus one
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s.off[mid] <= q) lo = mid + 1;
                else hi = mid;
            }
            const int j = lo - 1;                            // off[0] = 0 <= q: j >= 0, and its count is positive
            const int64_t at = (int64_t)path_rowptr[s.user[j]] + (int64_t)(q - s.off[j]);
            if (at >= 0 && at < n_paths) {
                p = path_idx[at];
                if (p < 0 || p >= n_paths) p = -1;
            }
            if (p >= 0) {
                seq_l[row0 + t] = path_l[p];
                targets[row0 + t] = path_tgt[p];
            }
        }
        s.part[tid] = (uint32_t)p;
        __syncthreads();
        const uint32_t slots = T - base < 256u ? T - base : 256u;
        for (uint32_t e = tid; e < slots * (uint32_t)path_len; e += 256u) {
            const uint32_t slot = e / (uint32_t)path_len, col = e - slot * (uint32_t)path_len;
            const int pp = (int)s.part[slot];
            if (pp >= 0) seq[(row0 + base + slot) * path_len + col] = paths[(int64_t)pp * path_len + col];
        }
        __syncthreads();
    }
}

}  // namespace

// Standard Philox4x32-10 on the host: the entry point draws the shuffle's round keys with it.
static void philox4x32_10_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

extern "C" int spex_sample_bce_epoch(const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows, const int32_t *d_pos_user,
                                     const int32_t *d_pos_item, int64_t n_pos, int32_t num_ng, int32_t num_item, uint64_t seed, uint32_t epoch,
                                     int64_t *d_users, int64_t *d_items_out, float *d_labels, void *stream)
{
    SPEX_CHECK_ARG(d_rowptr && d_items && d_pos_user && d_pos_item && d_users && d_items_out && d_labels, "spex_sample_bce_epoch: NULL pointer");
    SPEX_CHECK_ARG(n_pos >= 0 && num_ng >= 1 && num_item >= 1 && n_user_rows >= 0,
                   "spex_sample_bce_epoch: n_pos=%lld num_ng=%d num_item=%d n_user_rows=%d (needs n_pos >= 0, num_ng >= 1, num_item >= 1)",
                   (long long)n_pos, num_ng, num_item, n_user_rows);
    SPEX_CHECK_ARG(n_pos < ((int64_t)1 << 31) && n_pos * ((int64_t)num_ng + 1) < ((int64_t)1 << 31),
                   "spex_sample_bce_epoch: n_pos=%lld x (1 + num_ng=%d) samples: the shuffle needs fewer than 2^31", (long long)n_pos, num_ng);
    if (n_pos == 0) return SPEX_OK;
    const uint32_t n = (uint32_t)(n_pos * ((int64_t)num_ng + 1));
    uint32_t bits = 0;                                   // bit length of n - 1
    while (bits < 32 && ((n - 1) >> bits) != 0) ++bits;
    const uint32_t h = bits <= 2 ? 1u : (bits + 1) / 2;   // max(1, ceil(bits / 2)): the Feistel halves
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t a[4], b[4];
    philox4x32_10_host(0u, 0u, epoch, 3u, k0, k1, a);
    philox4x32_10_host(1u, 0u, epoch, 3u, k0, k1, b);
    const BceRoundKeys keys{{a[0], a[1], a[2], a[3], b[0], b[1]}};
    int64_t blocks = ((int64_t)n + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(sample_bce_epoch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_rowptr, d_items, n_user_rows,
                       d_pos_user, d_pos_item, (uint32_t)n_pos, (uint32_t)num_ng, num_item, n, h, keys, k0, k1, epoch, d_users, d_items_out,
                       d_labels);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_sample_ngcf_epoch(const int32_t *d_pop, int32_t n_pop, const int32_t *d_user, int32_t n_users, const int32_t *d_pos_off,
                                      const int32_t *d_pos_item, int64_t n_pos, const int32_t *d_row_off, const int32_t *d_row_rank,
                                      uint64_t seed, uint32_t epoch, int64_t *d_users, int64_t *d_items_out, float *d_labels, void *stream)
{
    SPEX_CHECK_ARG(d_pop && d_user && d_pos_off && d_pos_item && d_row_off && d_row_rank && d_users && d_items_out && d_labels,
                   "spex_sample_ngcf_epoch: NULL pointer");
    SPEX_CHECK_ARG(n_pop >= 1 && n_users >= 0 && n_pos >= 0 && (n_pos == 0 || n_users >= 1),
                   "spex_sample_ngcf_epoch: n_pop=%d n_users=%d n_pos=%lld (needs n_pop >= 1, n_users >= 0, n_pos >= 0, and a user for any positive)",
                   n_pop, n_users, (long long)n_pos);
    SPEX_CHECK_ARG(n_pos < ((int64_t)1 << 31) / 6 + 1 && 6 * n_pos < ((int64_t)1 << 31),
                   "spex_sample_ngcf_epoch: 6 x n_pos=%lld samples: the shuffle needs fewer than 2^31", (long long)n_pos);
    if (n_pos == 0) return SPEX_OK;
    const uint32_t n = (uint32_t)(6 * n_pos);
    uint32_t bits = 0;                                   // bit length of n - 1
    while (bits < 32 && ((n - 1) >> bits) != 0) ++bits;
    const uint32_t h = bits <= 2 ? 1u : (bits + 1) / 2;   // max(1, ceil(bits / 2)): the Feistel halves
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t a[4], b[4];
    philox4x32_10_host(0u, 0u, epoch, 6u, k0, k1, a);
    philox4x32_10_host(1u, 0u, epoch, 6u, k0, k1, b);
    const BceRoundKeys keys{{a[0], a[1], a[2], a[3], b[0], b[1]}};
    int64_t blocks = ((int64_t)n + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(sample_ngcf_epoch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_pop, n_pop, d_user, n_users,
                       d_pos_off, d_pos_item, (uint32_t)n_pos, d_row_off, d_row_rank, n, h, keys, k0, k1, epoch, d_users, d_items_out, d_labels);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_sample_dual_task_paths(const int64_t *d_users, int64_t n, int32_t B, int64_t max_steps, const int32_t *d_path_rowptr,
                                           int32_t n_user_rows, const int32_t *d_path_idx, int32_t n_paths, const int64_t *d_paths,
                                           int32_t path_len, const int64_t *d_path_l, const int64_t *d_path_tgt, int32_t cap, uint64_t seed,
                                           uint32_t epoch, int64_t *d_seq, int64_t *d_seq_l, int64_t *d_targets, int32_t *d_count, void *stream)
{
    SPEX_CHECK_ARG(d_users && d_path_rowptr && d_path_idx && d_paths && d_path_l && d_path_tgt && d_seq && d_seq_l && d_targets && d_count,
                   "spex_sample_dual_task_paths: NULL pointer");
    SPEX_CHECK_ARG(B >= 1 && B <= 4096, "spex_sample_dual_task_paths: B=%d (needs 1 <= B <= 4096: a batch's users are held in LDS)", B);
    SPEX_CHECK_ARG(n >= 0 && cap >= 0 && path_len >= 1 && n_user_rows >= 0 && n_paths >= 0,
                   "spex_sample_dual_task_paths: n=%lld cap=%d path_len=%d n_user_rows=%d n_paths=%d (needs n >= 0, cap >= 0, path_len >= 1)",
                   (long long)n, cap, path_len, n_user_rows, n_paths);
    int64_t n_batches = (n + B - 1) / B;
    if (max_steps >= 0 && max_steps < n_batches) n_batches = max_steps;
    SPEX_CHECK_ARG(n_batches < ((int64_t)1 << 31), "spex_sample_dual_task_paths: %lld batches: the batch index keys a 32-bit counter word",
                   (long long)n_batches);
    if (n_batches == 0) return SPEX_OK;
    const dim3 grid((unsigned)n_batches), block(256);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#define SPEX_DUAL_PATHS_LAUNCH(CAP)                                                                                                          \
    hipLaunchKernelGGL(sample_dual_paths_kernel<CAP>, grid, block, 0, (hipStream_t)stream, d_users, n, B, d_path_rowptr, n_user_rows, d_path_idx, \
                       n_paths, d_paths, path_len, d_path_l, d_path_tgt, cap, k0, k1, epoch, d_seq, d_seq_l, d_targets, d_count)
    if (B <= 256) SPEX_DUAL_PATHS_LAUNCH(256);
    else if (B <= 1024) SPEX_DUAL_PATHS_LAUNCH(1024);
    else SPEX_DUAL_PATHS_LAUNCH(4096);
#undef SPEX_DUAL_PATHS_LAUNCH
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_sample_bpr_triples(const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows, const int32_t *d_active,
                                       int32_t n_active, int32_t num_item, int64_t n, int32_t mode, uint64_t seed, uint32_t epoch,
                                       int64_t *d_users, int64_t *d_pos, int64_t *d_neg, void *stream)
{
    SPEX_CHECK_ARG(d_rowptr && d_items && d_active && d_users && d_pos && d_neg, "spex_sample_bpr_triples: NULL pointer");
    SPEX_CHECK_ARG(n >= 0 && n_user_rows >= 0 && num_item >= 1, "spex_sample_bpr_triples: n=%lld n_user_rows=%d num_item=%d (needs n >= 0, num_item >= 1)",
                   (long long)n, n_user_rows, num_item);
    SPEX_CHECK_ARG(n == 0 || n_active >= 1, "spex_sample_bpr_triples: n_active=%d: no user has a positive to draw", n_active);
    SPEX_CHECK_ARG(mode == 0 || mode == 1, "spex_sample_bpr_triples: mode %d (0: by user, 1: by interaction)", mode);
    if (n == 0) return SPEX_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(sample_bpr_triples_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_rowptr, d_items, n_user_rows,
                       d_active, n_active, num_item, n, mode, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, d_users, d_pos, d_neg);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}

extern "C" int spex_sample_negatives(const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                     const int64_t *d_pos_user, int64_t n_pos, int32_t num_ng, int32_t num_item,
                                     uint64_t seed, int64_t *d_out, void *stream)
{
    SPEX_CHECK_ARG(d_rowptr && d_pos_user && d_out, "spex_sample_negatives: NULL pointer");
    SPEX_CHECK_ARG(n_pos >= 0 && num_ng >= 1 && num_item >= 1 && n_user_rows >= 0, "spex_sample_negatives: bad sizes");
    const int64_t n_slots = n_pos * num_ng;
    if (n_slots == 0) return SPEX_OK;
    int64_t blocks = (n_slots + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(sample_negatives_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_rowptr, d_items,
                       d_pos_user, n_slots, num_ng, num_item, n_user_rows, (uint32_t)seed, (uint32_t)(seed >> 32), d_out);
    SPEX_HIP(hipGetLastError());
    return SPEX_OK;
}
