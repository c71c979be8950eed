// Whole training steps as ONE library call: the fixed launch sequence of a step issued from native code.
//
// Issued launch by launch from Python through ctypes, the exact training step costs the host ~9 us per launch (argument
// marshalling, stream lookup, tensor version bumps) — 12 launches = 110 us of host time for ~75 us of GPU time: the step
// became host-bound once the row-sparse backward had shortened the kernels.  These entry points take the step's buffers
// in a plain-C descriptor and issue the same launches back to back (~1 us each), so the loop is GPU-bound again.
// Nothing here computes: every launch is one of the library's own entry points.
//
// The BCE and the exact BPR LightGCN steps are ONE schedule, lightgcn_step, built from named pieces: step_check, the optional
// sparse-Adam clear and frontier lists, step_forward, the kind's batch launch (step_batch), the backward behind it
// (bf16_backward_push, frontier_backward [+ frontier_backward_bf16], step_backward_pulls) and one closing Adam launch.  What the kinds do NOT share, and the
// schedule keeps: BCE at L == 1 scores through spex_spmm_rowlist_f32 + spex_score_bce_slots_f32 and one pull product, BPR at L == 1
// runs the push form with the push target as the gradient; the deterministic BCE step reduces its slots in one call, the BPR step in
// two; only BPR has the dense form (from kBprStepDenseMinTriples* triples, never under SPEX_STEP_FRONTIER) and the L2 count tables;
// the dense d loss / d light_out is not formed at L == 3 (both kinds) and at BPR's L == 1.  The dual-task step's rec branch calls
// forward_layers and step_backward_pulls too.  Every native epoch is epoch_loop around its step.
#include <mutex>

#include "spex_common.h"

using namespace spex;

#define SPEX_TRY(call)           \
    do {                         \
        int rc_ = (call);        \
        if (rc_ != SPEX_OK) return rc_; \
    } while (0)

// ---- SPEX_STEP_BF16_GATHER (d == 64, L = 2 or 3): the whole-graph launches of the LightGCN steps gather from bf16
//      tables.  Everything a flagged descriptor must satisfy, checked before anything touches the device.
static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return b != nullptr && a0 < b0 + (b_bytes ? b_bytes : 1) && b0 < a0 + a_bytes;
}

static int bf16_step_check(const spex_lightgcn_step_t *s, const char *who)
{
    SPEX_CHECK_ARG((s->flags & SPEX_STEP_WIDE) == 0, "%s: SPEX_STEP_BF16_GATHER does not combine with SPEX_STEP_WIDE (bf16 gather tables are d == 64 only)", who);
    if (s->d != 64 || (s->L != 2 && s->L != 3)) {
        spex::set_error("%s: SPEX_STEP_BF16_GATHER takes d == 64 and L = 2 or 3 (got d = %d, L = %d): L = 1 has no whole-graph forward launch, "
                        "L >= 4 runs the fused running-sum schedule — run those without the flag", who, s->d, s->L);
        return SPEX_ERR_UNSUPPORTED;
    }
    const spex_graph *g = s->graph, *gt = s->graph_t;
    if (g->n_rows > 0 && (g->task == nullptr || gt->task == nullptr)) {
        spex::set_error("%s: SPEX_STEP_BF16_GATHER: the handle has no chunked task table (its source table exceeds a 32-bit offset): run without the flag", who);
        return SPEX_ERR_UNSUPPORTED;
    }
    SPEX_CHECK_ARG(s->E0_16 && s->ws16, "%s: SPEX_STEP_BF16_GATHER needs E0_16 ([N, 64] bf16) and ws16 ([2, N, 64] bf16): NULL %s", who,
                   s->E0_16 ? "ws16" : "E0_16");
    SPEX_CHECK_ARG((((uintptr_t)s->E0_16) & 15) == 0, "%s: E0_16 must be 16-byte aligned", who);
    SPEX_CHECK_ARG((((uintptr_t)s->ws16) & 15) == 0, "%s: ws16 must be 16-byte aligned", who);
    const size_t sz = (size_t)g->n_rows * 64, f = sizeof(float), h = sizeof(uint16_t);
    struct { const void *p; size_t bytes; } other[] = {
        {s->E0, sz * f}, {s->m, sz * f}, {s->v, sz * f}, {s->light_out, sz * f}, {s->ws_fwd, 2 * sz * f}, {s->lo_batch, 0}, {s->g_out, sz * f},
        {s->ws_bwd, 3 * sz * f}, {s->grad_E0, sz * f}, {s->grad_slots, (size_t)s->slot_capacity * 64 * f}, {s->row_counts, 2 * (size_t)g->n_rows * sizeof(int32_t)}};
    for (const auto &o : other) {
        SPEX_CHECK_ARG(!ranges_overlap(s->E0_16, sz * h, o.p, o.bytes), "%s: E0_16 aliases another buffer of the descriptor", who);
        SPEX_CHECK_ARG(!ranges_overlap(s->ws16, 2 * sz * h, o.p, o.bytes), "%s: ws16 aliases another buffer of the descriptor", who);
    }
    SPEX_CHECK_ARG(!ranges_overlap(s->ws16, 2 * sz * h, s->E0_16, sz * h), "%s: ws16 aliases E0_16", who);
    return SPEX_OK;
}

// The step's L - 1 whole-graph forward launches from the shadow: y_l in fp32 into ws_fwd[l - 1] and bf16(y_l) into ws16[l - 1] from
// the same register.  *last16 = bf16(y_(L-1)), the batch kernel's gather source.
static int bf16_forward(const spex_lightgcn_step_t *s, size_t sz, const uint16_t **last16, void *stream)
{
    const uint16_t *cur = s->E0_16;
    for (int32_t l = 0; l + 1 < s->L; ++l) {
        uint16_t *nxt = s->ws16 + (size_t)l * sz;
        SPEX_TRY(spex_spmm_bf16_f32(s->graph, cur, s->ws_fwd + (size_t)l * sz, nxt, nullptr, 1.0f, nullptr, nullptr, 1.0f, 64, stream));
        cur = nxt;
    }
    *last16 = cur;
    return SPEX_OK;
}

// The push form's pull products from P = (g + A^T g) / (L + 1) (fp32, the push target): one cast makes it a gather source (the
// forward's bf16 tables are dead: ws16 is reused); L == 3: G16 = bf16(A^T bf16(P)), bf16 output only, then grad_E0 = A^T G16; L == 2:
// grad_E0 = A^T bf16(P).  All plain: the Adam pass adds P (L == 3) or g_out / (L + 1) (L == 2) exactly as in the fp32 step.
static int bf16_backward_push(const spex_lightgcn_step_t *s, size_t sz, const float *P, void *stream)
{
    SPEX_TRY(spex_cast_bf16_f32(P, s->ws16, (int64_t)sz, stream));
    const uint16_t *src = s->ws16;
    if (s->L == 3) {
        SPEX_TRY(spex_spmm_bf16_f32(s->graph_t, src, nullptr, s->ws16 + sz, nullptr, 1.0f, nullptr, nullptr, 1.0f, 64, stream));
        src = s->ws16 + sz;
    }
    return spex_spmm_bf16_f32(s->graph_t, src, s->grad_E0, nullptr, nullptr, 1.0f, nullptr, nullptr, 1.0f, 64, stream);
}

// ---- SPEX_STEP_FRONTIER (d == 64, L >= 2; with SPEX_STEP_BF16_GATHER: L = 2 or 3, bf16_step_check's rules on top; include/spex_hip.h):
//      forward layer L - 1 and the backward product behind the batch kernel's push run over the batch's frontier F1.  Everything a
//      flagged descriptor must satisfy, checked before anything touches the device.
static int frontier_step_check(const spex_lightgcn_step_t *s, const char *who)
{
    if (s->d != 64 || (s->flags & SPEX_STEP_WIDE) != 0) {
        spex::set_error("%s: SPEX_STEP_FRONTIER takes d == 64 only (got d = %d%s): run other widths without the flag", who, s->d,
                        (s->flags & SPEX_STEP_WIDE) != 0 ? ", SPEX_STEP_WIDE" : "");
        return SPEX_ERR_UNSUPPORTED;
    }
    SPEX_CHECK_ARG(s->L >= 2, "%s: SPEX_STEP_FRONTIER needs L >= 2 (got %d): at L = 1 the step has no whole-graph launch to replace", who, s->L);
    SPEX_CHECK_ARG((s->flags & SPEX_STEP_DETERMINISTIC) == 0,
                   "%s: SPEX_STEP_FRONTIER does not combine with SPEX_STEP_DETERMINISTIC (the frontier push uses float atomics)", who);
    SPEX_CHECK_ARG((s->flags & SPEX_STEP_BPR_DENSE) == 0,
                   "%s: SPEX_STEP_FRONTIER does not combine with SPEX_STEP_BPR_DENSE (a frontier step takes the push form at any T)", who);
    // (edge dropout, fp32 tables: the lists hold the columns reached over kept entries and the three list-driven launches follow the
    //  handle's mask — DESIGN.md 4.27; step_check's rule asks for the transposed handle.  The bf16 list SpMM has no masked form.)
    SPEX_CHECK_ARG((s->flags & SPEX_STEP_BF16_GATHER) == 0 || (s->graph->mask_mode == 0 && s->graph_t->mask_mode == 0),
                   "%s: SPEX_STEP_FRONTIER | SPEX_STEP_BF16_GATHER does not combine with edge dropout", who);
    SPEX_CHECK_ARG(s->frontier_list && s->frontier_stamp && s->frontier_counts,
                   "%s: SPEX_STEP_FRONTIER needs frontier_list ([N] int32), frontier_stamp ([N] int32, zeroed once) and frontier_counts ([2] int32; [4] with SPEX_STEP_SPARSE_ADAM or SPEX_STEP_FRONTIER_DEEP)", who);
    return SPEX_OK;
}

// ---- SPEX_STEP_SPARSE_ADAM (with SPEX_STEP_FRONTIER, L == 2, d == 64; include/spex_hip.h): Adam, the clears and the loss sum over the
//      rows of F2 = F1 U the stored columns of F1's rows — the rows the frontier push can write — instead of the whole table.  Checked
//      in front of frontier_step_check, like it before anything touches the device.
static int sparse_adam_check(const spex_lightgcn_step_t *s, const char *who)
{
    SPEX_CHECK_ARG((s->flags & SPEX_STEP_BF16_GATHER) == 0,
                   "%s: SPEX_STEP_SPARSE_ADAM does not combine with SPEX_STEP_BF16_GATHER (the row-sparse Adam pass keeps no bf16 shadow of E0)", who);
    SPEX_CHECK_ARG((s->flags & SPEX_STEP_FRONTIER) != 0, "%s: SPEX_STEP_SPARSE_ADAM needs SPEX_STEP_FRONTIER (the row list is the frontier's)", who);
    SPEX_CHECK_ARG(s->L == 2 || (s->L == 3 && (s->flags & SPEX_STEP_FRONTIER_DEEP) != 0),
                   "%s: SPEX_STEP_SPARSE_ADAM needs L == 2, or L == 3 with SPEX_STEP_FRONTIER_DEEP (got L = %d): behind a whole-graph pull the gradient is dense",
                   who, s->L);
    return SPEX_OK;
}

// ---- SPEX_STEP_FRONTIER_DEEP (with SPEX_STEP_FRONTIER, L == 3, d == 64, fp32 tables; include/spex_hip.h): every launch
//      of the step runs over a device list — y_1 at F2, y_2 at F1, W = A^T P over F1, grad_E0 = A^T W over F2 — and, with
//      SPEX_STEP_SPARSE_ADAM, Adam over F3.  Checked in front of the two other checks, like them before anything touches the device.
static int deep_step_check(const spex_lightgcn_step_t *s, const char *who)
{
    if (s->d != 64 || (s->flags & SPEX_STEP_WIDE) != 0) {
        spex::set_error("%s: SPEX_STEP_FRONTIER_DEEP takes d == 64 only (got d = %d%s): run other widths without the flag", who, s->d,
                        (s->flags & SPEX_STEP_WIDE) != 0 ? ", SPEX_STEP_WIDE" : "");
        return SPEX_ERR_UNSUPPORTED;
    }
    SPEX_CHECK_ARG((s->flags & SPEX_STEP_FRONTIER) != 0, "%s: SPEX_STEP_FRONTIER_DEEP needs SPEX_STEP_FRONTIER (it takes that form one level further)", who);
    SPEX_CHECK_ARG(s->L == 3, "%s: SPEX_STEP_FRONTIER_DEEP needs L == 3 (got %d): at L == 2 SPEX_STEP_FRONTIER leaves no whole-graph launch, L >= 4 is not built",
                   who, s->L);
    SPEX_CHECK_ARG((s->flags & SPEX_STEP_BF16_GATHER) == 0,
                   "%s: SPEX_STEP_FRONTIER_DEEP does not combine with SPEX_STEP_BF16_GATHER (fp32 tables only)", who);
    return SPEX_OK;       // (SPEX_STEP_DETERMINISTIC, SPEX_STEP_BPR_DENSE, NULL list fields: frontier_step_check's refusals)
}

// The first launch of a flagged step: grad_E0, the frontier push's target, all-zero again — through the list the previous flagged step
// left (SPEX_STEP_GRAD_ROWS_LISTED: nothing else wrote the table since) or, without the bit, over the whole table once.  The deep
// step (L == 3) pushes into two tables: with the bit, W is all-zero as well (the flagged step before has cleared it below |F2|).
static int sparse_adam_begin(spex_lightgcn_step_t *s, size_t sz, void *stream)
{
    const bool listed = (s->flags & SPEX_STEP_GRAD_ROWS_LISTED) != 0;
    s->flags &= ~SPEX_STEP_GRAD_ROWS_LISTED;        // (set again once every launch of the step is queued)
    // (the cell of the step that set the bit: a flagged L == 3 step is a SPEX_STEP_FRONTIER_DEEP step and lists F3, an L == 2 step F2)
    if (listed) return spex_zero_rows_f32(s->grad_E0, s->frontier_list, s->frontier_counts + s->L, s->graph->n_rows, s->graph->n_rows, s->d, stream);
    // L == 3: W = ws_bwd[1], the F1 push's target, too — the flagged step before this one has cleared it by list, any other step has not
    if (s->L == 3) SPEX_TRY(spex::zero_f32(s->ws_bwd + sz, (int64_t)sz, stream));
    return spex::zero_f32(s->grad_E0, (int64_t)sz, stream);
}

// The row-sparse Adam pass of a flagged step over frontier_list[0 .. |F2|): g_out / 3 read and cleared below |Bset|, the batch
// kernel's push target ws_bwd[0] cleared below |F1|, the per-sample losses summed in the dense pass's order.  L == 3: over F3, below.
static int sparse_adam_pass(spex_lightgcn_step_t *s, int32_t t_next, int32_t n_loss, float *loss_sum, const spex::L2Rows *l2, void *stream)
{
    spex::AdamRowList rl;
    const int32_t *count_a = nullptr;
    rl.list = s->frontier_list;
    rl.max_count = rl.n_rows = s->graph->n_rows;
    rl.count_b = s->frontier_counts;
    if (s->L == 3) {
        // SPEX_STEP_FRONTIER_DEEP: over frontier_list[0 .. |F3|); the add term is P (the batch launch's push target, support in F1:
        // read, added and cleared below |F1|), W = ws_bwd[1] is cleared below |F2|; the L2 counts stay keyed to Bset
        rl.count = s->frontier_counts + 3;
        rl.add_g = s->ws_bwd;
        rl.add_div = 1.0f;
        count_a = s->frontier_counts + 1;
        rl.count_z = s->frontier_counts + 2;
        rl.zero_buf = s->ws_bwd + (size_t)s->graph->n_rows * s->d;
    } else {
        rl.count = s->frontier_counts + 2;
        rl.add_g = s->g_out;
        rl.add_div = (float)(s->L + 1);
        rl.count_z = s->frontier_counts + 1;
        rl.zero_buf = s->ws_bwd;
    }
    SPEX_TRY(spex::adam_rows(s->E0, s->grad_E0, s->m, s->v, rl, t_next, s->lr, s->beta1, s->beta2, s->eps, stream, s->grad_slots, n_loss, loss_sum, l2, count_a));
    s->flags |= SPEX_STEP_GRAD_ROWS_LISTED;
    return SPEX_OK;
}

// Bset, then F1 behind it, of a batch of up to three index lists into frontier_list; frontier_counts = { |Bset|, |F1| }.  hops == 2
// (SPEX_STEP_SPARSE_ADAM, SPEX_STEP_FRONTIER_DEEP): F2 behind F1 by a second pass of the same kernel over [0, |F1|); frontier_counts[2] = |F2|.  Under edge
// dropout both hops list the columns reached over KEPT entries only (the handle's mask of this step, set before the call): the masked
// F1 holds every row the batch kernel reads or pushes into, the masked F2 every row the frontier push can write.
static int frontier_lists(spex_lightgcn_step_t *s, const int64_t *a, int32_t n_a, const int64_t *b, int32_t n_b, const int64_t *c, int32_t n_c,
                          void *stream, int hops = 1)
{
    const spex_graph *g = s->graph;
    const int32_t epoch = s->frontier_epoch % 0x7FFFFFFF + 1;      // never 0
    const int64_t n_u = s->n_user_rows;
    SPEX_TRY(spex_unique_rows_i32(a, n_a, 0, b, n_b, n_u, g->n_rows, s->frontier_stamp, epoch, s->frontier_list, s->frontier_counts, stream));
    if (c) SPEX_TRY(spex::unique_rows_more(c, n_c, n_u, nullptr, 0, 0, g->n_rows, s->frontier_stamp, epoch, s->frontier_list, s->frontier_counts, stream));
    s->frontier_epoch = epoch;      // (the stamps are on the device from here on, whatever becomes of the step)
    const int64_t slots = (int64_t)n_a + n_b + (c ? n_c : 0);
    SPEX_TRY(spex_frontier_rows_masked_i32(g, s->frontier_list, s->frontier_counts, (int32_t)(slots < g->n_rows ? slots : g->n_rows), s->frontier_stamp,
                                           epoch, s->frontier_counts + 1, stream));
    // (each further hop walks the rows the hop before appended AND those before them, whose columns are stamped already: one kernel,
    //  one rule.  hops == 3, SPEX_STEP_FRONTIER_DEEP | SPEX_STEP_SPARSE_ADAM: F3 behind F2, the rows the push over F2 can write)
    for (int h = 2; h <= hops; ++h)
        SPEX_TRY(spex_frontier_rows_masked_i32(g, s->frontier_list, s->frontier_counts + h - 1, g->n_rows, s->frontier_stamp, epoch, s->frontier_counts + h, stream));
    return SPEX_OK;
}

// SPEX_STEP_FRONTIER | SPEX_STEP_BF16_GATHER (L = 2 or 3): y_(L-1) at the rows of F1 from the bf16 table of the layer
// before — fp32 into ws_fwd[L - 2], bf16 of the same register into ws16[L - 2], the batch kernel's gather source —, behind y_1 over
// the whole graph from the shadow at L == 3 (the bf16 step's own first launch).  At L == 2 no whole-graph launch is left.
static int frontier_forward_bf16(const spex_lightgcn_step_t *s, size_t sz, const uint16_t **last16, void *stream)
{
    const uint16_t *cur = s->E0_16;
    const size_t l = (size_t)(s->L - 2);
    if (s->L == 3) {
        SPEX_TRY(spex_spmm_bf16_f32(s->graph, cur, s->ws_fwd, s->ws16, nullptr, 1.0f, nullptr, nullptr, 1.0f, 64, stream));
        cur = s->ws16;
    }
    uint16_t *nxt = s->ws16 + l * sz;
    SPEX_TRY(spex_spmm_rowlist_dev_bf16_f32(s->graph, cur, s->frontier_list, s->frontier_counts + 1, s->graph->n_rows, s->ws_fwd + l * sz, nxt, nullptr,
                                            nullptr, 1.0f, 64, stream));
    *last16 = nxt;
    return SPEX_OK;
}

// The frontier step's backward at L == 3 behind W = A^T P (the fp32 frontier push of the fp32 P: exact): one cast makes W a gather
// source (ws16[0]: the forward's y_1 table is dead), then grad_E0 = A^T bf16(W), plain; the Adam pass adds P.  Straight-through with ONE
// rounding, of W, where bf16_backward_push has two (of P and of A^T bf16(P)).  At L == 2 the push target is grad_E0 itself: nothing here.
static int frontier_backward_bf16(const spex_lightgcn_step_t *s, size_t sz, const float *W, void *stream)
{
    SPEX_TRY(spex_cast_bf16_f32(W, s->ws16, (int64_t)sz, stream));
    return spex_spmm_bf16_f32(s->graph_t, s->ws16, s->grad_E0, nullptr, nullptr, 1.0f, nullptr, nullptr, 1.0f, 64, stream);
}

// Forward layer L - 1 at the rows of F1: the table, and for L >= 4 the running sum, at those rows.
static int frontier_forward(const spex_lightgcn_step_t *s, const float *cur, float *nxt, bool plain, void *stream)
{
    return spex_spmm_rowlist_dev_f32(s->graph, cur, s->frontier_list, s->frontier_counts + 1, s->graph->n_rows, nxt, plain ? nullptr : s->light_out,
                                     plain ? nullptr : s->light_out, 1.0f, s->d, stream);
}

// The backward product l = L - 2 from the batch kernel's push target P: W = A^T P (+ g_out / (L + 1) where the whole-graph step's
// launch carries that term: L >= 4) as a push over the F1 list into W, zeroed here.  W = grad_E0 at L == 2, ws_bwd[1] otherwise.
static int frontier_backward(const spex_lightgcn_step_t *s, size_t sz, const float *P, float **W_out, void *stream, bool zeroed = false)
{
    float *W = s->L == 2 ? s->grad_E0 : s->ws_bwd + sz;
    if (!zeroed) SPEX_TRY(spex::zero_f32(W, (int64_t)sz, stream));       // (SPEX_STEP_SPARSE_ADAM: the step's first launch has cleared it)
    if ((s->flags & SPEX_STEP_FRONTIER_DEEP) != 0) {
        // the deep step (L == 3: plain, no add term) takes the long-list kernel here too: on the F1 list it ran 1.04 x (unmasked) and
        // 2.0 x (keep_prob 0.3) the one-workgroup-per-row kernel's rate (profiles/frontier_deep/push_ab.jsonl)
        SPEX_TRY(spex_spmm_push_list_f32(s->graph, s->frontier_list, s->frontier_counts + 1, s->graph->n_rows, P, 1.0f, W, s->d, stream));
        *W_out = W;
        return SPEX_OK;
    }
    SPEX_TRY(spex_spmm_push_rows_scaled_f32(s->graph, s->frontier_list, s->frontier_counts + 1, s->graph->n_rows, P, 1, s->L >= 4 ? s->g_out : nullptr,
                                            1, 1.0f, 1.0f / (float)(s->L + 1), W, s->d, stream));
    *W_out = W;
    return SPEX_OK;
}

// ---- The one LightGCN step schedule.  spex_lightgcn_step_bce_f32 and spex_lightgcn_step_bpr_adam_f32 are lightgcn_step (below, behind
//      the BPR step's own notes) on a StepBatch: what differs between a batch of B labelled samples and a batch of T triples.
struct StepBatch {
    const char *who;                    // the entry point, for messages
    const int64_t *a, *b, *c;           // BCE: users, items, NULL; BPR: users, pos, neg
    const float *labels;                // BCE only
    int32_t n;                          // B samples / T triples
    int32_t rows;                       // table rows per sample: 2 (BCE) or 3 (BPR)
    float *loss_sum;
};

// Everything a descriptor and a batch must satisfy, checked before anything touches the device.  Shared rules in one place; slot
// capacity (2 B / 3 T), row_counts, weight_decay and the width rule — the BPR step takes d = 128 / 256 only from a descriptor that says
// SPEX_STEP_WIDE, the BCE step takes them without the flag — per kind.
static int step_check(const spex_lightgcn_step_t *s, const StepBatch &k)
{
    const char *who = k.who;
    const bool bpr = k.rows == 3;
    SPEX_CHECK_ARG(s && s->graph && s->graph_t && s->E0 && s->m && s->v && s->light_out && s->ws_fwd && s->lo_batch && s->g_out
                       && s->ws_bwd && s->grad_E0 && s->grad_slots && (!bpr || s->row_counts),
                   "%s: NULL field in the step descriptor%s", who, bpr ? " (row_counts included)" : "");
    SPEX_CHECK_ARG(k.a && k.b && (bpr ? k.c != nullptr : k.labels != nullptr) && k.loss_sum && k.n >= 1, "%s: NULL batch pointer or %s < 1", who,
                   bpr ? "T" : "B");
    const spex_graph *g = s->graph, *gt = s->graph_t;
    const int32_t L = s->L, d = s->d, n_u = s->n_user_rows;
    SPEX_CHECK_ARG(g->n_rows == g->n_cols && gt->n_rows == g->n_rows && gt->n_cols == g->n_rows, "%s: square graphs of one size", who);
    if ((s->flags & SPEX_STEP_BF16_GATHER) != 0) SPEX_TRY(bf16_step_check(s, who));
    if ((s->flags & SPEX_STEP_FRONTIER_DEEP) != 0) SPEX_TRY(deep_step_check(s, who));
    if ((s->flags & SPEX_STEP_SPARSE_ADAM) != 0) SPEX_TRY(sparse_adam_check(s, who));
    if ((s->flags & SPEX_STEP_FRONTIER) != 0) SPEX_TRY(frontier_step_check(s, who));
    if (!bpr) {
        SPEX_CHECK_ARG(L >= 1 && (d == 64 || d == 128 || d == 256) && n_u >= 0 && n_u <= g->n_rows,
                       "%s: L=%d d=%d n_user_rows=%d (needs L >= 1 and d = 64, 128 or 256)", who, L, d, n_u);
    } else {
        if ((s->flags & SPEX_STEP_WIDE) != 0) {
            if (d != 128 && d != 256) {
                spex::set_error("%s: SPEX_STEP_WIDE takes d = 128 or 256 (got %d); d == 64 runs without the flag — the widths are 64, 128 and 256", who, d);
                return SPEX_ERR_UNSUPPORTED;
            }
        } else if (d != 64) {
            spex::set_error("%s: d == 64 only (got %d); d = 128 / 256 take the launch-by-launch form", who, d);
            return SPEX_ERR_UNSUPPORTED;
        }
        SPEX_CHECK_ARG(L >= 1 && n_u >= 0 && n_u <= g->n_rows, "%s: L=%d n_user_rows=%d (needs L >= 1)", who, L, n_u);
    }
    SPEX_CHECK_ARG(k.n <= INT32_MAX / k.rows && s->slot_capacity >= k.rows * k.n, "%s: slot capacity %d < %d %s = %lld", who, s->slot_capacity,
                   k.rows, bpr ? "T" : "B", (long long)k.rows * k.n);
    if (bpr) SPEX_CHECK_ARG(s->weight_decay >= 0.0f, "%s: weight_decay %g", who, (double)s->weight_decay);
    // edge dropout (model.py:46-55; set per step on BOTH handles with spex_graph_set_edge_mask — graph_t must then be the transposed
    // handle carrying the edge-id permutation, a masked adjacency is not symmetric): every product of the step uses the handles'
    // mask — the whole-graph launches through spex_spmm_f32, the batch kernel's last layer and push through the same keep rule.
    SPEX_CHECK_ARG(g->mask_mode == gt->mask_mode && (g->mask_mode == 0 || (g->keep_prob == gt->keep_prob && g->seed == gt->seed && g->keep == gt->keep)),
                   "%s: graph and graph_t must carry the same edge-dropout mask", who);
    SPEX_CHECK_ARG(g->mask_mode == 0 || (gt != g && L >= 2),
                   "%s: edge dropout needs L >= 2 and graph_t = the transposed handle (with its edge-id permutation)", who);
    return SPEX_OK;
}

// The first `count` whole-graph forward launches y_(l+1) = A y_l of an L-layer model, into ws_fwd[l & 1]; *cur = the last table written
// (E0 for count == 0).  For L <= 3 the launches run in the PLAIN form (no epilogue operand, one output stream: 12.3 vs 14.8 us on
// Epinion2) and the batch kernel forms the layer sum (E^0 + E^1 (+ E^2)) + y at the batch's rows — the only rows the loss reads — in
// the fused epilogues' order; deeper models keep the running sum fused into the launches (`light`).
static int forward_layers(const spex_graph *g, const float *E0, float *light, float *ws_fwd, int32_t L, int32_t count, int32_t d, void *stream,
                          const float **cur)
{
    const size_t sz = (size_t)g->n_rows * d;
    const bool plain = L >= 2 && L <= 3;
    *cur = E0;
    for (int32_t l = 0; l < count; ++l) {
        float *nxt = ws_fwd + (size_t)(l & 1) * sz;
        if (plain) SPEX_TRY(spex_spmm_f32(g, *cur, nxt, nullptr, 1.0f, nullptr, nullptr, 1.0f, d, stream));
        else SPEX_TRY(spex_spmm_f32(g, *cur, nxt, nullptr, 1.0f, l == 0 ? E0 : light, light, 1.0f, d, stream));
        *cur = nxt;
    }
    return SPEX_OK;
}

struct StepTables {                     // what the forward leaves for the batch launch
    const float *cur = nullptr;         // y_(L-1), its gather source ...
    const uint16_t *cur16 = nullptr;    // ... or, SPEX_STEP_BF16_GATHER, bf16(y_(L-1))
    const float *sum0 = nullptr, *sum1 = nullptr, *sum2 = nullptr;      // the tables whose rows it adds in front of the last layer's
};                                                                      // product: E^0 (+ E^1 + E^2), or the running sum

// Forward layers 0 .. L-2: from the bf16 shadow, or in fp32 over the whole graph — under SPEX_STEP_FRONTIER the last of them at the rows
// of F1 only.  The last layer is left to the batch launch, at the batch's rows.
static int step_forward(const spex_lightgcn_step_t *s, size_t sz, void *stream, StepTables *f)
{
    const int32_t L = s->L;
    const bool plain = L >= 2 && L <= 3, fr = (s->flags & SPEX_STEP_FRONTIER) != 0;
    f->cur = s->E0;
    if ((s->flags & SPEX_STEP_BF16_GATHER) != 0) {
        if (fr) SPEX_TRY(frontier_forward_bf16(s, sz, &f->cur16, stream));
        else SPEX_TRY(bf16_forward(s, sz, &f->cur16, stream));
    } else if ((s->flags & SPEX_STEP_FRONTIER_DEEP) != 0) {
        // y_1 at the rows of F2 from E0, y_2 at the rows of F1 from that table: everything y_2 at F1 reads of y_1 lies in F2.  Both plain.
        SPEX_TRY(spex_spmm_rowlist_dev_f32(s->graph, s->E0, s->frontier_list, s->frontier_counts + 2, s->graph->n_rows, s->ws_fwd, nullptr, nullptr, 1.0f,
                                           s->d, stream));
        SPEX_TRY(frontier_forward(s, s->ws_fwd, s->ws_fwd + sz, true, stream));
        f->cur = s->ws_fwd + sz;
    } else {
        SPEX_TRY(forward_layers(s->graph, s->E0, s->light_out, s->ws_fwd, L, fr ? L - 2 : L - 1, s->d, stream, &f->cur));
        if (fr) {
            float *nxt = s->ws_fwd + (size_t)(L & 1) * sz;
            SPEX_TRY(frontier_forward(s, f->cur, nxt, plain, stream));
            f->cur = nxt;
        }
    }
    f->sum0 = plain || L == 1 ? s->E0 : s->light_out;
    f->sum1 = plain ? s->ws_fwd : nullptr;
    f->sum2 = plain && L == 3 ? s->ws_fwd + sz : nullptr;
    return SPEX_OK;
}

// The pull-form products G_l = g / (L+1) + A^T G_(l+1), l = l_first .. 0, from src = G_(l_first + 1), through ws_bwd[1], [2], [1] ...
// (never the source, never the push target ws_bwd[0]) into grad.  The last one (l = 0) runs in the PLAIN form: its g / (L+1) term is
// added by the Adam pass, which reads g anyway to clear it (one epilogue stream less on a 15 us launch).  L == 3 (the reference's
// depth): BOTH run plain.  With P = G_2 = (g + A^T g) / 4 the gradient is A^T (A^T P + g/4) + g/4 = A^T (A^T P) + (A^T g / 4 + g / 4)
// = A^T (A^T P) + P — and P is the push target, which the Adam pass touches anyway (to clear it): it adds P instead of g / 4.  No
// epilogue operand left in the backward.
static int step_backward_pulls(const spex_graph *gt, const float *src, int32_t l_first, const float *g_dense, float *ws_bwd, float *grad, int32_t L,
                               int32_t d, void *stream)
{
    const size_t sz = (size_t)gt->n_rows * d;
    for (int32_t l = l_first; l >= 0; --l) {
        float *nxt = l == 0 ? grad : ws_bwd + (size_t)(1 + ((L - 2 - l) & 1)) * sz;
        if (l == 0 || L == 3) SPEX_TRY(spex_spmm_f32(gt, src, nxt, nullptr, 1.0f, nullptr, nullptr, 1.0f, d, stream));
        else SPEX_TRY(spex_spmm_f32(gt, src, nxt, g_dense, (float)(L + 1), nullptr, nullptr, 1.0f, d, stream));
        src = nxt;
    }
    return SPEX_OK;
}

// The batch launch of either kind in its forms, from the fp32 or the bf16 table: slots given — per-sample gradient rows, nothing added
// anywhere (SPEX_STEP_DETERMINISTIC); otherwise atomics into `dense` (NULL: not formed) and, G given, the first backward product
// (g + A^T g) * push_scale in push form into G.  counts: the BPR kind's L2 occurrence counts (NULL: no L2 term).
static int step_batch(const spex_lightgcn_step_t *s, const StepBatch &k, const StepTables &f, bool bpr, int32_t *counts, float push_scale,
                      float *loss_rows, float *slots, float *dense, float *G, void *stream)
{
    spex::BatchLaunch b;
    b.bpr = bpr; b.push = slots == nullptr; b.x_bf16 = f.cur16 != nullptr;
    b.g = s->graph; b.X = f.cur16 ? (const void *)f.cur16 : (const void *)f.cur;
    b.acc_in = f.sum0; b.acc2 = f.sum1; b.acc3 = f.sum2; b.acc_div = (float)(s->L + 1);
    b.a = k.a; b.b = k.b; b.c = bpr ? k.c : nullptr; b.labels = bpr ? nullptr : k.labels;
    b.n = k.n; b.n_user_rows = s->n_user_rows; b.grad_scale = 1.0f / (float)k.n;
    if (bpr) {
        b.weight_decay = s->weight_decay; b.E0 = s->E0; b.row_counts = counts;
    }
    b.loss_rows = loss_rows;
    if (slots) {
        b.slots = slots;
    } else {
        b.push_scale = push_scale; b.g_out = dense; b.G = G;
    }
    b.d = s->d; b.stream = stream;
    return spex::batch_launch(b);
}

static int lightgcn_step(spex_lightgcn_step_t *s, const StepBatch &k, void *stream);

extern "C" int spex_lightgcn_step_bce_f32(spex_lightgcn_step_t *s, const int64_t *users, const int64_t *items,
                                          const float *labels, int32_t B, float *loss_sum, void *stream)
{
    const StepBatch k = {"spex_lightgcn_step_bce_f32", users, items, nullptr, labels, B, 2, loss_sum};
    return lightgcn_step(s, k, stream);
}

// The loop of every native epoch: batch k = samples [k B, min((k+1) B, n)) through step(k, b0, nb), at most max_steps (< 0: all) of
// them, stopping at the first error.  keep_prob < 1: the per-step mask is set on both handles (once where gt == g) in front of the
// step, and both are unmasked again on every path.
template <class Step>
static int epoch_loop(const spex_graph *graph, const spex_graph *graph_t, int64_t n, int32_t B, int64_t max_steps, float keep_prob,
                      uint32_t drop_seed, Step step)
{
    spex_graph *g = const_cast<spex_graph *>(graph), *gt = const_cast<spex_graph *>(graph_t);
    const bool drop = keep_prob < 1.0f;
    int rc = SPEX_OK;
    int64_t k = 0;
    for (int64_t b0 = 0; b0 < n && rc == SPEX_OK && (max_steps < 0 || k < max_steps); b0 += B, ++k) {
        const int32_t nb = (int32_t)(n - b0 < B ? n - b0 : B);
        if (drop) {
            const uint64_t seed = ((uint64_t)drop_seed << 32) | (uint64_t)(uint32_t)(k + 1);
            rc = spex_graph_set_edge_mask(g, 2, nullptr, keep_prob, seed);
            if (rc == SPEX_OK && gt != g) rc = spex_graph_set_edge_mask(gt, 2, nullptr, keep_prob, seed);
            if (rc != SPEX_OK) break;
        }
        rc = step(k, b0, nb);
    }
    if (drop) {
        (void)spex_graph_set_edge_mask(g, 0, nullptr, 1.0f, 0);
        if (gt != g) (void)spex_graph_set_edge_mask(gt, 0, nullptr, 1.0f, 0);
    }
    return rc;
}

// Train() of main_rec.py:30-37 over a whole (pre-shuffled, device-resident) epoch as ONE call: batch k = samples [k B, min((k+1) B, n))
// through spex_lightgcn_step_bce_f32 — the host issues ~6 launches per step and nothing else (the Python loop around the one-call
// step cost 7 us per 70 us step: slicing three tensors, building the call).  Loss sums of the full batches -> loss_full, of the ragged
// last batch -> loss_ragged (the caller forms main_rec.py:36's sum of per-batch MEAN losses from the two).
// keep_prob < 1: edge dropout with the in-kernel sampled mask (model.py:46-55), a fresh one per step — seed (drop_seed << 32) | step,
// step counted from 1 — set on both handles as spex_graph_set_edge_mask(.., 2, ..) would; the handles are left unmasked.
extern "C" int spex_lightgcn_epoch_bce_f32(spex_lightgcn_step_t *s, const int64_t *users, const int64_t *items, const float *labels,
                                           int64_t n, int32_t B, int64_t max_steps, float keep_prob, uint32_t drop_seed, float *loss_full,
                                           float *loss_ragged, void *stream)
{
    SPEX_CHECK_ARG(s && s->graph && s->graph_t, "spex_lightgcn_epoch_bce_f32: NULL step descriptor or graph");
    SPEX_CHECK_ARG(users && items && labels && loss_full && loss_ragged && n >= 0 && B >= 1, "spex_lightgcn_epoch_bce_f32: NULL pointer, n < 0 or B < 1");
    SPEX_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f, "spex_lightgcn_epoch_bce_f32: keep_prob %g", keep_prob);
    return epoch_loop(s->graph, s->graph_t, n, B, max_steps, keep_prob, drop_seed, [&](int64_t, int64_t b0, int32_t nb) {
        return spex_lightgcn_step_bce_f32(s, users + b0, items + b0, labels + b0, nb, nb == B ? loss_full : loss_ragged, stream);
    });
}

// The exact BPR training step — BPR differentiated through the propagation, an L2 term on the E0 rows of the batch, Adam: upstream
// LightGCN's training semantics — as ONE call.  The schedule is spex_lightgcn_step_bce_f32's with the triple-shaped batch kernel
// (batch.hip: lightgcn_bpr_batch_kernel, three rows per workgroup; lightgcn_bpr_batch_wide_kernel at d = 128 / 256) in the middle.
// d == 64, or — for a descriptor that carries SPEX_STEP_WIDE: its tables and slots are d wide — d = 128 / 256.
//   fast path:      L - 1 whole-graph launches (plain for L <= 3) -> spex_lightgcn_bpr_batch_f32 (last layer at the 3 T rows, scores,
//                   loss, gradient rows, (g + A^T g) / (L + 1) in push form) -> L - 1 pull products on A^T (all plain at L == 3:
//                   A^T (A^T P) + P) -> Adam, which sums the per-triple losses in order and adds the L2 gradient: 2 L launches
//   deterministic:  slots kernel -> spex_reduce_slots_f32 twice (users over slots [0, T), then (pos, neg) over [T, 3 T) — user rows and
//                   item rows never coincide for valid triples; the second call accumulates, so that the all-zero slots of a skipped
//                   triple whose negative item index lands among the user rows clobber nothing) -> spex_propagate_bwd_f32 -> Adam;
//                   no float atomic
//   L == 1 runs the same schedule (no whole-graph forward launch, the push target is the whole gradient).
// L2 term: loss += weight_decay / 2 * (|E0[u]|^2 + |E0[p]|^2 + |E0[n]|^2) per triple (in the batch kernel); its gradient
// weight_decay / T * E0[r] per occurrence of r is not propagated: the batch kernel counts occurrences in row_counts[t_next & 1] and
// the Adam pass adds count * E0 and clears the other parity's table.  grad_E0 holds the step's whole gradient afterwards.
// From this many triples up the fast path takes the dense form (see below): the push's cost grows with the batch rows' stored
// entries, a third pull product's does not.  Measured on Epinion2, L = 3, us per step push / dense, both forced, alternating
// (tools/bpr_exact_step_time.py --sweep, profiles/bpr_exact/form_sweep.jsonl): T = 256: 71.8 / 80.2, 512: 84.1 / 86.9,
// 768: 95.2 / 92.5, 1 024: 105.9 / 98.8, 1 536: 127.3 / 108.8, 2 048: 150.3 / 120.3, 4 096: 241.0 / 167.6.
// d = 128 / 256, the same sweep (--recdim; profiles/bpr_exact_wide/form_sweep_d128.jsonl, _d256.jsonl; two rounds), the
// smallest swept T from which the dense form wins by more than the windows' spread in both rounds: d = 128: 768: 158.5 / 158.2 and
// 159.1 / 159.8 (no), 1 024: 176.5 / 165.3; d = 256: 256: 214.9 / 224.6 (no), 512: 247.1 / 234.6 and 246.0 / 232.6.
constexpr int32_t kBprStepDenseMinTriples = 768, kBprStepDenseMinTriples128 = 1024, kBprStepDenseMinTriples256 = 512;

// The schedule of both kinds: checks -> [sparse-Adam clear] -> [frontier lists] -> L - 1 forward launches -> the batch launch in one of
// its forms -> the backward behind it -> ONE Adam launch.  s->t advances only once every launch of the step is queued.
//   SPEX_STEP_DETERMINISTIC: every sum that the fast path leaves to float atomics is taken in a fixed order — same forward (same
//                   kernel code for the batch's rows: bit-identical scores), the samples' gradient rows leave as per-sample slots and
//                   are added per table row in ascending slot order (what the reference's CPU index backward does, model.py:115-116),
//                   and the whole backward runs in pull form (each output row one chain in ascending column order, like the
//                   reference's sparse addmm).  Per-sample losses: head of lo_batch, summed in order by the Adam pass.
//   dense (BPR):    the batch launch with the push skipped — the gradient rows go to the dense g_out with atomics — and the whole
//                   backward in pull form (L products: their cost does not grow with T, the push's does)
//   BCE at L == 1:  the last layer at the batch's rows, scoring, then grad = (g + A^T g) / 2 as one pull-form product
//   push:           the batch-sized middle as one launch, the first backward product G_(L-1) = (g + A^T g) / (L+1) in push form over the
//                   rows of A itself: (A^T g)[c] = sum_r A[r, c] g[r] (g_out and the push target ws_bwd[0] are all-zero here: the Adam
//                   pass clears them for the next step; first call: the caller); then the pull products (step_backward_pulls)
static int lightgcn_step(spex_lightgcn_step_t *s, const StepBatch &k, void *stream)
{
    SPEX_TRY(step_check(s, k));
    const spex_graph *g = s->graph, *gt = s->graph_t;
    const int32_t L = s->L, d = s->d, n_u = s->n_user_rows, n = k.n, t_next = s->t + 1;
    const size_t sz = (size_t)g->n_rows * d;
    const bool bpr = k.rows == 3, bf16 = (s->flags & SPEX_STEP_BF16_GATHER) != 0, det = (s->flags & SPEX_STEP_DETERMINISTIC) != 0;
    const bool fr = (s->flags & SPEX_STEP_FRONTIER) != 0, sp = (s->flags & SPEX_STEP_SPARSE_ADAM) != 0, deep = (s->flags & SPEX_STEP_FRONTIER_DEEP) != 0;
    // BPR: the L2 term's count tables by step parity — the batch launch counts into one, the Adam pass clears the other
    spex::L2Rows l2_rows;
    const spex::L2Rows *l2 = nullptr;
    int32_t *counts = nullptr, *counts_other = nullptr;
    if (bpr) {
        counts_other = s->row_counts + (size_t)((t_next + 1) & 1) * g->n_rows;
        if (s->weight_decay > 0.0f) counts = s->row_counts + (size_t)(t_next & 1) * g->n_rows;
        l2_rows.count = counts;
        l2_rows.clear = counts_other;
        l2_rows.scale = s->weight_decay / (float)n;
        l2_rows.g_store = s->grad_E0;
        l2_rows.shift = d == 64 ? 4 : (d == 128 ? 5 : 6);
        l2 = &l2_rows;
    }
    if (sp) {
        // (in front of the lists: the clear may read the previous step's.  The row-sparse pass does not clear the other parity's count
        //  table row by row — the rows that hold counts there are an earlier batch's — so the step clears it whole: 4 N bytes)
        SPEX_TRY(sparse_adam_begin(s, sz, stream));
        if (bpr) SPEX_TRY(spex::zero_f32(reinterpret_cast<float *>(counts_other), (int64_t)g->n_rows, stream));
        l2_rows.clear = nullptr;
    } else {
        s->flags &= ~SPEX_STEP_GRAD_ROWS_LISTED;                       // (this step writes grad_E0 wherever it likes)
    }
    if (fr) SPEX_TRY(frontier_lists(s, k.a, n, k.b, n, k.c, k.c ? n : 0, stream, deep ? (sp ? 3 : 2) : (sp ? 2 : 1)));      // (the first launches: every argument check is above)
    StepTables f;
    SPEX_TRY(step_forward(s, sz, stream, &f));
    auto batch = [&](float push_scale, float *loss_rows, float *slots, float *dense, float *G) -> int {
        return step_batch(s, k, f, bpr, counts, push_scale, loss_rows, slots, dense, G, stream);
    };
    // the whole backward in pull form from the dense d loss / d light_out
    auto backward_dense = [&]() -> int {
        return bf16 ? spex_propagate_bwd_bf16_f32(gt, s->g_out, s->grad_E0, s->ws_bwd, s->ws16, L, d, stream)
                    : spex_propagate_bwd_f32(gt, s->g_out, s->grad_E0, s->ws_bwd, L, d, stream);
    };
    const int32_t dense_min = d == 64 ? kBprStepDenseMinTriples : (d == 128 ? kBprStepDenseMinTriples128 : kBprStepDenseMinTriples256);
    const bool dense = bpr && !fr && ((s->flags & SPEX_STEP_BPR_DENSE) != 0 || ((s->flags & SPEX_STEP_BPR_PUSH) == 0 && n >= dense_min));
    // what the closing Adam launch reads besides the gradient, as the dense-backward forms leave it; the other forms say otherwise
    const float *grad = s->grad_E0, *loss_rows = s->grad_slots, *add = nullptr;
    float *zero1 = s->g_out, *zero2 = s->ws_bwd /* stays the push form's all-zero target */, add_div = 1.0f;
    if (det) {
        SPEX_TRY(batch(0.0f, s->lo_batch, s->grad_slots, nullptr, nullptr));
        if (bpr) {
            // (users over slots [0, T), then (pos, neg) over [T, 3 T) — user rows and item rows never coincide for valid triples; the
            //  second call accumulates, so that the all-zero slots of a skipped triple whose negative item index lands among the user
            //  rows clobber nothing)
            SPEX_TRY(spex_reduce_slots_f32(k.a, n, 0, nullptr, 0, 0, g->n_rows, s->grad_slots, d, 1.0f, s->g_out, 0, d, stream));
            SPEX_TRY(spex_reduce_slots_f32(k.b, n, n_u, k.c, n, n_u, g->n_rows, s->grad_slots + (size_t)n * d, d, 1.0f, s->g_out, 1, d, stream));
        } else {
            SPEX_TRY(spex_reduce_slots_f32(k.a, n, 0, k.b, n, n_u, g->n_rows, s->grad_slots, d, 1.0f, s->g_out, 0, d, stream));
        }
        SPEX_TRY(backward_dense());
        loss_rows = s->lo_batch;
    } else if (dense) {
        SPEX_TRY(batch(0.0f, s->grad_slots, nullptr, s->g_out, nullptr));
        SPEX_TRY(backward_dense());
    } else if (!bpr && L == 1) {
        SPEX_TRY(spex_spmm_rowlist_f32(g, f.cur, k.a, n, 0, k.b, n, n_u, nullptr, s->E0, s->lo_batch, (float)(L + 1), d, stream));
        SPEX_TRY(spex_score_bce_slots_f32(s->lo_batch, s->lo_batch + (size_t)n_u * d, d, d, n_u, g->n_rows - n_u, k.a, k.b, k.labels, n, d,
                                          k.loss_sum, s->g_out, s->g_out + (size_t)n_u * d, 1.0f / (float)n, s->grad_slots, d, stream));
        SPEX_TRY(spex_propagate_bwd_f32(gt, s->g_out, s->grad_E0, s->ws_bwd, L, d, stream));
        loss_rows = nullptr;            // (the scoring launch has added the loss itself, and nothing pushed)
        zero2 = nullptr;
    } else {
        // (BPR at L == 1 runs this form too: no pull product, the push target IS the gradient — read, stored to grad_E0 and cleared by the
        //  Adam pass.  Nothing reads the dense d loss / d light_out there or in the all-plain L == 3 step: it is not formed)
        float *G = s->ws_bwd;
        const bool no_dense = L == 3 || L == 1;
        SPEX_TRY(batch(1.0f / (float)(L + 1), s->grad_slots /* per-sample losses, summed by the Adam pass */, nullptr, no_dense ? nullptr : s->g_out, G));
        const float *src = G;
        if (bf16 && !fr) SPEX_TRY(bf16_backward_push(s, sz, G, stream));      // (the same products from bf16 roundings of their sources)
        float *W = nullptr;
        if (fr) SPEX_TRY(frontier_backward(s, sz, G, &W, stream, sp));     // product l = L - 2 over the frontier (from the fp32 P on either table type)
        if (fr) src = W;
        if (fr && bf16 && L == 3) SPEX_TRY(frontier_backward_bf16(s, sz, W, stream));
        // (none under SPEX_STEP_SPARSE_ADAM, L == 2: the frontier push has left the whole product in grad_E0, non-zero in F2 only)
        if (deep) {
            // grad_E0 = A^T W as a push over the F2 list (W's support), the long-list kernel; complete in F3.  The Adam pass adds P.
            if (!sp) SPEX_TRY(spex::zero_f32(s->grad_E0, (int64_t)sz, stream));      // (SPEX_STEP_SPARSE_ADAM: the step's first launch has cleared it)
            SPEX_TRY(spex_spmm_push_list_f32(g, s->frontier_list, s->frontier_counts + 2, g->n_rows, W, 1.0f, s->grad_E0, d, stream));
        } else if (!bf16)
            SPEX_TRY(step_backward_pulls(gt, src, fr ? L - 3 : L - 2, s->g_out, s->ws_bwd, s->grad_E0, L, d, stream));
        if (L == 1) grad = G;
        if (no_dense) zero1 = nullptr;                                  // (untouched, all-zero)
        add = L == 1 ? nullptr : (L == 3 ? G : s->g_out);
        add_div = L == 3 ? 1.0f : (float)(L + 1);
    }
    // ---- Adam — over the whole table, or over the listed rows — which also sums the per-sample losses in order, adds the L2 gradient
    //      and clears g_out and the push target for the next step
    if (sp)
        SPEX_TRY(sparse_adam_pass(s, t_next, n, k.loss_sum, l2, stream));      // (sets SPEX_STEP_GRAD_ROWS_LISTED again)
    else
        SPEX_TRY(spex::adam_step_z2(s->E0, grad, s->m, s->v, (int64_t)sz, t_next, s->lr, s->beta1, s->beta2, s->eps, zero1, zero2, stream, loss_rows, n,
                                    k.loss_sum, nullptr, add, add_div, l2, bf16 ? s->E0_16 : nullptr));
    s->t = t_next;
    return SPEX_OK;
}

extern "C" int spex_lightgcn_step_bpr_adam_f32(spex_lightgcn_step_t *s, const int64_t *users, const int64_t *pos, const int64_t *neg,
                                               int32_t T, float *loss_sum, void *stream)
{
    const StepBatch k = {"spex_lightgcn_step_bpr_adam_f32", users, pos, neg, nullptr, T, 3, loss_sum};
    return lightgcn_step(s, k, stream);
}

// An epoch of pre-drawn, device-resident triples as ONE call: batch k = triples [k T, min((k+1) T, n)) through
// spex_lightgcn_step_bpr_adam_f32; loss sums, max_steps and the per-step sampled edge mask as in spex_lightgcn_epoch_bce_f32.
extern "C" int spex_lightgcn_epoch_bpr_f32(spex_lightgcn_step_t *s, const int64_t *users, const int64_t *pos, const int64_t *neg, int64_t n,
                                           int32_t T, int64_t max_steps, float keep_prob, uint32_t drop_seed, float *loss_full,
                                           float *loss_ragged, void *stream)
{
    SPEX_CHECK_ARG(s && s->graph && s->graph_t, "spex_lightgcn_epoch_bpr_f32: NULL step descriptor or graph");
    SPEX_CHECK_ARG(users && pos && neg && loss_full && loss_ragged && n >= 0 && T >= 1, "spex_lightgcn_epoch_bpr_f32: NULL pointer, n < 0 or T < 1");
    SPEX_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f, "spex_lightgcn_epoch_bpr_f32: keep_prob %g", keep_prob);
    return epoch_loop(s->graph, s->graph_t, n, T, max_steps, keep_prob, drop_seed, [&](int64_t, int64_t b0, int32_t nb) {
        return spex_lightgcn_step_bpr_adam_f32(s, users + b0, pos + b0, neg + b0, nb, nb == T ? loss_full : loss_ragged, stream);
    });
}

// A sampled epoch: the triples are drawn on the device (sampler.hip: one launch into the caller's index buffers) and consumed by the
// loop above — nothing crosses the host.  Every argument check of both calls comes before the sampler's launch.
extern "C" int spex_lightgcn_epoch_bpr_sampled_f32(spex_lightgcn_step_t *s, const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                                   const int32_t *d_active, int32_t n_active, int32_t num_item, int64_t n, int32_t mode,
                                                   uint64_t seed, uint32_t epoch, int32_t T, int64_t max_steps, float keep_prob,
                                                   uint32_t drop_seed, int64_t *users, int64_t *pos, int64_t *neg, float *loss_full,
                                                   float *loss_ragged, void *stream)
{
    const char *who = "spex_lightgcn_epoch_bpr_sampled_f32";
    SPEX_CHECK_ARG(s && s->graph && s->graph_t, "%s: NULL step descriptor or graph", who);
    SPEX_CHECK_ARG(users && pos && neg && loss_full && loss_ragged && n >= 0 && T >= 1, "%s: NULL pointer, n < 0 or T < 1", who);
    SPEX_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f, "%s: keep_prob %g", who, keep_prob);
    SPEX_TRY(spex_sample_bpr_triples(d_rowptr, d_items, n_user_rows, d_active, n_active, num_item, n, mode, seed, epoch, users, pos, neg, stream));
    return spex_lightgcn_epoch_bpr_f32(s, users, pos, neg, n, T, max_steps, keep_prob, drop_seed, loss_full, loss_ragged, stream);
}

// Epochs epoch0 .. epoch0 + n_epochs - 1 of the call above, back to back on one stream: the host queues epoch after epoch and never
// waits.  One set of index buffers: epoch e + 1's sampler launch is ordered behind epoch e's last step.  Edge dropout: epoch number
// E runs with the mask seed drop_seed + 0x9E3779B9 E (mod 2^32) — the per-epoch calls key their masks by the step WITHIN the epoch,
// so one drop_seed for every epoch would replay one mask sequence.
extern "C" int spex_lightgcn_train_bpr_sampled_f32(spex_lightgcn_step_t *s, const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                                   const int32_t *d_active, int32_t n_active, int32_t num_item, int64_t n, int32_t mode,
                                                   uint64_t seed, uint32_t epoch0, int32_t n_epochs, int32_t T, int64_t max_steps,
                                                   float keep_prob, uint32_t drop_seed, int64_t *users, int64_t *pos, int64_t *neg,
                                                   float *loss_epochs, void *stream)
{
    SPEX_CHECK_ARG(n_epochs >= 0 && loss_epochs, "spex_lightgcn_train_bpr_sampled_f32: n_epochs < 0 or NULL loss_epochs");
    for (int32_t e = 0; e < n_epochs; ++e) {
        const uint32_t epoch = epoch0 + (uint32_t)e;
        SPEX_TRY(spex_lightgcn_epoch_bpr_sampled_f32(s, d_rowptr, d_items, n_user_rows, d_active, n_active, num_item, n, mode, seed, epoch, T,
                                                     max_steps, keep_prob, drop_seed + 0x9E3779B9u * epoch, users, pos, neg,
                                                     loss_epochs + 2 * (size_t)e, loss_epochs + 2 * (size_t)e + 1, stream));
    }
    return SPEX_OK;
}

// A sampled BCE epoch: negatives, labels and the shuffle drawn on the device (sampler.hip: one launch into the caller's buffers) and
// consumed by spex_lightgcn_epoch_bce_f32 — nothing crosses the host.  Every argument check of both calls comes before the sampler's
// launch.
extern "C" int spex_lightgcn_epoch_bce_sampled_f32(spex_lightgcn_step_t *s, const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                                   const int32_t *d_pos_user, const int32_t *d_pos_item, int64_t n_pos, int32_t num_ng,
                                                   int32_t num_item, uint64_t seed, uint32_t epoch, int32_t B, int64_t max_steps,
                                                   float keep_prob, uint32_t drop_seed, int64_t *users, int64_t *items, float *labels,
                                                   float *loss_full, float *loss_ragged, void *stream)
{
    const char *who = "spex_lightgcn_epoch_bce_sampled_f32";
    SPEX_CHECK_ARG(s && s->graph && s->graph_t, "%s: NULL step descriptor or graph", who);
    SPEX_CHECK_ARG(users && items && labels && loss_full && loss_ragged && B >= 1, "%s: NULL pointer or B < 1", who);
    SPEX_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f, "%s: keep_prob %g", who, keep_prob);
    SPEX_TRY(spex_sample_bce_epoch(d_rowptr, d_items, n_user_rows, d_pos_user, d_pos_item, n_pos, num_ng, num_item, seed, epoch, users, items,
                                   labels, stream));
    return spex_lightgcn_epoch_bce_f32(s, users, items, labels, n_pos * ((int64_t)num_ng + 1), B, max_steps, keep_prob, drop_seed, loss_full,
                                       loss_ragged, stream);
}

// Epochs epoch0 .. epoch0 + n_epochs - 1 of the call above, back to back on one stream: the host queues epoch after epoch and never
// waits.  One set of buffers: epoch e + 1's sampler launch is ordered behind epoch e's last step.  Edge dropout: epoch number E runs
// with the mask seed drop_seed + 0x9E3779B9 E (mod 2^32), the BPR call's rule — the per-epoch call keys its masks by the step WITHIN
// the epoch, so one drop_seed for every epoch would replay one mask sequence.
extern "C" int spex_lightgcn_train_bce_sampled_f32(spex_lightgcn_step_t *s, const int32_t *d_rowptr, const int32_t *d_items, int32_t n_user_rows,
                                                   const int32_t *d_pos_user, const int32_t *d_pos_item, int64_t n_pos, int32_t num_ng,
                                                   int32_t num_item, uint64_t seed, uint32_t epoch0, int32_t n_epochs, int32_t B,
                                                   int64_t max_steps, float keep_prob, uint32_t drop_seed, int64_t *users, int64_t *items,
                                                   float *labels, float *loss_epochs, void *stream)
{
    SPEX_CHECK_ARG(n_epochs >= 0 && loss_epochs, "spex_lightgcn_train_bce_sampled_f32: n_epochs < 0 or NULL loss_epochs");
    for (int32_t e = 0; e < n_epochs; ++e) {
        const uint32_t epoch = epoch0 + (uint32_t)e;
        SPEX_TRY(spex_lightgcn_epoch_bce_sampled_f32(s, d_rowptr, d_items, n_user_rows, d_pos_user, d_pos_item, n_pos, num_ng, num_item, seed,
                                                     epoch, B, max_steps, keep_prob, drop_seed + 0x9E3779B9u * epoch, users, items, labels,
                                                     loss_epochs + 2 * (size_t)e, loss_epochs + 2 * (size_t)e + 1, stream));
    }
    return SPEX_OK;
}

// train() of NGCF_SPEX/code/main_rec.py:116-131 over a whole pre-shuffled, device-resident epoch as ONE call: batch k = samples
// [k B, min((k+1) B, n)) through spex_ngcf_step_bce_f32 (the default one-layer model; the step advances its own Adam and dropout
// counters) — the host issues the launches and nothing else.  Loss sums as in spex_lightgcn_epoch_bce_f32.
extern "C" int spex_ngcf_epoch_bce_f32(spex_ngcf_step_t *s, const int64_t *users, const int64_t *items, const float *labels, int64_t n,
                                       int32_t B, int64_t max_steps, float *loss_full, float *loss_ragged, void *stream)
{
    SPEX_CHECK_ARG(s && users && items && labels && loss_full && loss_ragged && n >= 0 && B >= 1,
                   "spex_ngcf_epoch_bce_f32: NULL pointer, n < 0 or B < 1");
    // (no edge dropout in NGCF: keep_prob = 1, the loop touches no handle)
    return epoch_loop(nullptr, nullptr, n, B, max_steps, 1.0f, 0, [&](int64_t, int64_t b0, int32_t nb) {
        return spex_ngcf_step_bce_f32(s, users + b0, items + b0, labels + b0, nb, nb == B ? loss_full : loss_ragged, stream);
    });
}

// A sampled NGCF epoch: negatives (without replacement, per user), labels and the shuffle drawn on the device (sampler.hip: one launch
// into the caller's buffers) and consumed by spex_ngcf_epoch_bce_f32 — nothing crosses the host.  Every argument check of both calls
// comes before the sampler's launch.
extern "C" int spex_ngcf_epoch_bce_sampled_f32(spex_ngcf_step_t *s, const int32_t *d_pop, int32_t n_pop, const int32_t *d_user, int32_t n_users,
                                               const int32_t *d_pos_off, const int32_t *d_pos_item, int64_t n_pos, const int32_t *d_row_off,
                                               const int32_t *d_row_rank, uint64_t seed, uint32_t epoch, int32_t B, int64_t max_steps,
                                               int64_t *users, int64_t *items, float *labels, float *loss_full, float *loss_ragged, void *stream)
{
    SPEX_CHECK_ARG(s && users && items && labels && loss_full && loss_ragged && B >= 1,
                   "spex_ngcf_epoch_bce_sampled_f32: NULL pointer or B < 1");
    SPEX_TRY(spex_sample_ngcf_epoch(d_pop, n_pop, d_user, n_users, d_pos_off, d_pos_item, n_pos, d_row_off, d_row_rank, seed, epoch, users, items,
                                    labels, stream));
    return spex_ngcf_epoch_bce_f32(s, users, items, labels, 6 * n_pos, B, max_steps, loss_full, loss_ragged, stream);
}

// Epochs epoch0 .. epoch0 + n_epochs - 1 of the call above, back to back on one stream: the host queues epoch after epoch and never
// waits.  One set of buffers: epoch e + 1's sampler launch is ordered behind epoch e's last step.  No per-epoch reseed of the message
// dropout: its mask is keyed by the descriptor's dropout_step, which the steps advance across epochs.
extern "C" int spex_ngcf_train_bce_sampled_f32(spex_ngcf_step_t *s, const int32_t *d_pop, int32_t n_pop, const int32_t *d_user, int32_t n_users,
                                               const int32_t *d_pos_off, const int32_t *d_pos_item, int64_t n_pos, const int32_t *d_row_off,
                                               const int32_t *d_row_rank, uint64_t seed, uint32_t epoch0, int32_t n_epochs, int32_t B,
                                               int64_t max_steps, int64_t *users, int64_t *items, float *labels, float *loss_epochs, void *stream)
{
    SPEX_CHECK_ARG(n_epochs >= 0 && loss_epochs, "spex_ngcf_train_bce_sampled_f32: n_epochs < 0 or NULL loss_epochs");
    for (int32_t e = 0; e < n_epochs; ++e)
        SPEX_TRY(spex_ngcf_epoch_bce_sampled_f32(s, d_pop, n_pop, d_user, n_users, d_pos_off, d_pos_item, n_pos, d_row_off, d_row_rank, seed,
                                                 epoch0 + (uint32_t)e, B, max_steps, users, items, labels, loss_epochs + 2 * (size_t)e,
                                                 loss_epochs + 2 * (size_t)e + 1, stream));
    return SPEX_OK;
}

// The north-star step — 3-layer propagation + fused BPR-SGD over a batch of triples — as ONE call.  For L >= 2, on a graph without
// rows beyond 1 024 entries and while 6 T <= N (spmm.hip: step_fuses_last; SPEX_STEP_FUSED_LAST=0 / 1 forces either form), it is L
// launches: L - 1 whole-graph plain launches (the first with the snapshot tail described below) and ONE launch that gathers layer L
// at the batch's <= 3 T slot rows from the layer-(L-1) table — four triples per workgroup, segment-parallel over its 16 waves — and
// runs the BPR update on (((E^0 + E^1) + E^2) + y) / (L + 1), y the gathered row: the whole-graph launch's row bit for bit
// (score.hip: bpr_fused_last_kernel).  The step then traverses (L - 1) nnz entries plus the batch rows' entries; the half of ws
// that used to receive layer L is not written (L = 3: ws[1]; L = 2: ws[0]; on the running-sum fallback L = 2: ws[1], L = 3: none —
// ws[0] keeps E^1).  sum1 is unchanged by this.  Otherwise (L = 1, hub rows, larger T) it is today's schedule:
// ONE call of L + 1 launches with the
// layer mean left to the BPR kernel: EVERY layer in the plain form, the layer-1 launch also setting aside the E^0 rows of the
// batch's <= 3 T slots (a tail of workgroups inside the launch: spex::propagate_plain), and the fused gather + dot + sigmoid + SGD
// kernel forms (((E^0 + E^1) + E^2) + E^3) / (L + 1) at its triples' rows only — the rows of the propagated table the step reads.
// sum1 then holds E^1.  Where that tail would push a one-round launch over 512 workgroups the step keeps layer 1 in the running-sum
// form (sum1 = E^0 + E^1 over the whole table) and the kernel forms ((sum1 + E^2) + E^3) / (L + 1): the same bits.  Same results as spex_propagate_f32 followed by spex_bpr_sgd_step_f32 on its output (the rows are
// bit-identical; the updates land with float atomics in either form).
extern "C" int spex_lightgcn_step_bpr_f32(const spex_graph_t *g, float *E0, float *sum1, float *ws, int32_t n_user_rows, int32_t L,
                                          int32_t d, const int64_t *u, const int64_t *i_pos, const int64_t *i_neg, int64_t T, float lr,
                                          float reg, float *loss_sum, void *stream)
{
    // (an empty batch names no triples: its index pointers may be NULL — an empty device tensor has no storage)
    SPEX_CHECK_ARG(g && E0 && sum1 && ws && T >= 0 && (T == 0 || (u && i_pos && i_neg)), "spex_lightgcn_step_bpr_f32: NULL argument or T < 0");
    SPEX_CHECK_ARG(g->n_rows == g->n_cols && n_user_rows >= 0 && n_user_rows <= g->n_rows, "spex_lightgcn_step_bpr_f32: square graph, 0 <= n_user_rows <= N");
    SPEX_CHECK_ARG(g->mask_mode == 0, "spex_lightgcn_step_bpr_f32: edge dropout is not supported in the one-call step");
    if (d != 64 || L < 1 || L > 3) {
        spex::set_error("spex_lightgcn_step_bpr_f32: d == 64 and 1 <= L <= 3 only (d = %d, L = %d): use spex_propagate_f32 + spex_bpr_sgd_step_f32", d, L);
        return SPEX_ERR_UNSUPPORTED;
    }
    const float *tables[3], *snap = nullptr, *last_src = nullptr;
    SPEX_TRY(spex::propagate_plain(g, E0, sum1, ws, L, d, stream, tables, u, i_pos, i_neg, T, n_user_rows, &snap, &last_src));
    if (last_src)
        return spex::bpr_sgd_fused_last(g, last_src, snap, tables[0], tables[1], (float)(L + 1), E0, n_user_rows, (int64_t)g->n_rows - n_user_rows,
                                        u, i_pos, i_neg, T, lr, reg, loss_sum, stream);
    return spex::bpr_sgd_layers(snap, tables[0], tables[1], tables[2], (float)(L + 1), E0, n_user_rows, (int64_t)g->n_rows - n_user_rows, u,
                                i_pos, i_neg, T, lr, reg, loss_sum, stream);
}

// Fork / join events of the two-stream steps (dual-task, NGCF): one pair PER STEP DESCRIPTOR, created on first use and kept in
// the descriptor's ev_fork / ev_join cells (zero-initialised by the caller, released with spex_step_events_release).  A pair
// shared per device — the first version — could be re-recorded by a second stepper driven from another host thread between
// this stepper's record and its wait, so that a join waited for the wrong stream's work.
static int step_events(void **ev_fork, void **ev_join, hipEvent_t *fork_ev, hipEvent_t *join_ev)
{
    if (!*ev_fork) {
        hipEvent_t e = nullptr;
        SPEX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        *ev_fork = e;
    }
    if (!*ev_join) {
        hipEvent_t e = nullptr;
        SPEX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        *ev_join = e;
    }
    *fork_ev = (hipEvent_t)*ev_fork;
    *join_ev = (hipEvent_t)*ev_join;
    return SPEX_OK;
}

extern "C" int spex_step_events_release(void **ev_fork, void **ev_join)
{
    if (ev_fork && *ev_fork) {
        SPEX_HIP(hipEventDestroy((hipEvent_t)*ev_fork));
        *ev_fork = nullptr;
    }
    if (ev_join && *ev_join) {
        SPEX_HIP(hipEventDestroy((hipEvent_t)*ev_join));
        *ev_join = nullptr;
    }
    return SPEX_OK;
}

extern "C" int spex_ngcf_step_bce_f32(spex_ngcf_step_t *s, const int64_t *users, const int64_t *items, const float *labels,
                                      int32_t B, float *loss_sum, void *stream)
{
    SPEX_CHECK_ARG(s && s->graph && s->E0 && s->mE && s->vE && s->W && s->mW && s->vW && s->side && s->g_slots
                       && s->g_side_c && s->g_ego_c && s->gW_parts && s->grad,
                   "spex_ngcf_step_bce_f32: NULL field in the step descriptor");
    SPEX_CHECK_ARG(users && items && labels && loss_sum && B >= 1, "spex_ngcf_step_bce_f32: NULL batch pointer or B < 1");
    const spex_graph *g = s->graph;
    const int32_t d = 64, n = g->n_rows, n_u = s->n_user_rows;
    SPEX_CHECK_ARG(g->n_rows == g->n_cols && n_u >= 0 && n_u <= n, "spex_ngcf_step_bce_f32: square graph, 0 <= n_user_rows <= N");
    SPEX_CHECK_ARG(s->slot_capacity >= 2 * B, "spex_ngcf_step_bce_f32: slot capacity %d < 2 B = %d", s->slot_capacity, 2 * B);
    SPEX_CHECK_ARG(g->mask_mode == 0, "spex_ngcf_step_bce_f32: edge dropout does not apply to NGCF");
    const float *W_gc = s->W, *b_gc = s->W + d * d, *W_bi = s->W + d * d + d, *b_bi = s->W + 2 * d * d + d;
    const int32_t per = 2 * (d * d + d);
    const uint32_t step = (uint32_t)s->dropout_step;
    // ---- forward, at the batch's rows ONLY: the descriptor is a one-layer model, whose loss reads the concatenated table nowhere
    //      else (main_rec.py:96-104) — side = A ego for the 2B rows (spex_spmm_rowlist_f32: the main kernel's sums, bit for bit, for
    //      rows of <= 1 024 entries) and the layer on 16-slot tiles of those rows, which writes [ego | normalised layer output] into
    //      the dense tables at the rows the scoring reads.  (11.4 + 10.6 us of whole-table launches on Epinion2 became 6 + 4.)
    SPEX_TRY(spex_spmm_rowlist_f32(g, s->E0, users, B, 0, items, B, n_u, s->side, nullptr, nullptr, 1.0f, d, stream));
    // ---- scoring + backward on the batch's 2B slots in one launch (per-sample losses go to the head of g_slots: the table's Adam
    //      pass below adds them to loss_sum in a fixed order), then the push-form A^T product into the (all-zero) table gradient.
    //      Default: the launch also runs the layer's FORWARD at those rows — its tiles hold both rows of 8 samples and score from
    //      the layer output they recompute anyway, so the concatenated table is never formed (spex_ngcf_fwd_score_bwd_rows_f32)
    float *loss_rows = s->g_slots;
    SPEX_TRY(spex_ngcf_fwd_score_bwd_rows_f32(s->E0, s->side, W_gc, b_gc, W_bi, b_bi, labels, 1.0f / (float)B, n, d, s->slope, s->p_drop,
                                              s->seed, step, 0, s->pad_row, users, items, B, n_u, loss_rows, s->g_side_c, s->g_ego_c,
                                              s->gW_parts, per, stream));
    // ---- Adam: the table (its pass clears the gradient again), the layer weights (their pass sums the partial blocks).  The
    //      weights' pass needs only the rows backward: with a second stream it runs beside the push-form product and the table's
    //      pass (a one-workgroup-class launch next to two that fill the chip) and is joined at the end of the step.
    //      t / dropout_step are advanced only after every launch of the step has been queued (a failed call leaves them alone).
    const int32_t t_next = s->t + 1;
    auto weight_adam = [&](void *st) -> int {
        return spex_adam_step_sum_f32(s->W, s->gW_parts, spex_ngcf_layer_bwd_rows_parts(2 * B), per, s->mW, s->vW, per, t_next, s->lr,
                                      s->beta1, s->beta2, s->eps, st);
    };
    const bool det = (s->flags & SPEX_STEP_DETERMINISTIC) != 0;
    if (det)
        SPEX_CHECK_ARG(s->graph_t && s->g_side_dense && s->g_ego_dense && s->graph_t->n_rows == n && s->graph_t->n_cols == n
                           && s->graph_t->mask_mode == 0,
                       "spex_ngcf_step_bce_f32: SPEX_STEP_DETERMINISTIC needs graph_t (A^T) and the two dense [N, 64] gradient buffers");
    const bool two_streams = s->side_stream != nullptr && s->side_stream != stream;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    int rc = SPEX_OK;
    bool forked = false;
    if (two_streams) {
        SPEX_TRY(step_events(&s->ev_fork, &s->ev_join, &fork_ev, &join_ev));
        SPEX_HIP(hipEventRecord(fork_ev, (hipStream_t)stream));
        SPEX_HIP(hipStreamWaitEvent((hipStream_t)s->side_stream, fork_ev, 0));
        forked = true;
        rc = weight_adam(s->side_stream);
        if (hipEventRecord(join_ev, (hipStream_t)s->side_stream) != hipSuccess && rc == SPEX_OK) rc = SPEX_ERR_HIP;
    }
    if (rc == SPEX_OK) {
        if (det) {
            // SPEX_STEP_DETERMINISTIC: the slots' compact rows are added per table row in ascending slot order (dense g_side / g_ego,
            // both all-zero outside the batch's rows), A^T g_side is the pull-form product over the rows of A^T with g_ego added in
            // its epilogue, and the touched rows are cleared again — no float atomics (the weight gradients never had any).
            rc = spex_reduce_slots_f32(users, B, 0, items, B, n_u, n, s->g_side_c, d, 1.0f, s->g_side_dense, 0, d, stream);
            if (rc == SPEX_OK) rc = spex_reduce_slots_f32(users, B, 0, items, B, n_u, n, s->g_ego_c, d, 1.0f, s->g_ego_dense, 0, d, stream);
            if (rc == SPEX_OK) rc = spex_spmm_f32(s->graph_t, s->g_side_dense, s->grad, s->g_ego_dense, 1.0f, nullptr, nullptr, 1.0f, d, stream);
            if (rc == SPEX_OK) rc = spex_reduce_slots_f32(users, B, 0, items, B, n_u, n, nullptr, d, 1.0f, s->g_side_dense, 0, d, stream);
            if (rc == SPEX_OK) rc = spex_reduce_slots_f32(users, B, 0, items, B, n_u, n, nullptr, d, 1.0f, s->g_ego_dense, 0, d, stream);
        } else {
            rc = spex_spmm_push_batch_f32(g, users, B, 0, items, B, n_u, s->g_side_c, d, s->g_ego_c, d, 1.0f, s->grad, d, stream);
        }
    }
    // (one stream: the layer weights' update rides in the table's Adam launch as 33 extra workgroups — a launch of its own cost
    //  the step ~5 us of ramp; parts summed in the same order as spex_adam_step_sum_f32 sums them)
    spex::SmallAdam small;
    if (!two_streams) {
        small.p = s->W; small.m = s->mW; small.v = s->vW; small.parts = s->gW_parts;
        small.n_parts = spex_ngcf_layer_bwd_rows_parts(2 * B); small.stride = per; small.n = per;
    }
    if (rc == SPEX_OK)
        rc = spex::adam_step_z2(s->E0, s->grad, s->mE, s->vE, (int64_t)n * d, t_next, s->lr, s->beta1, s->beta2, s->eps, s->grad, nullptr, stream,
                                loss_rows, B, loss_sum, two_streams ? nullptr : &small);
    if (forked && hipStreamWaitEvent((hipStream_t)stream, join_ev, 0) != hipSuccess && rc == SPEX_OK) rc = SPEX_ERR_HIP;   // joined on every path
    if (rc != SPEX_OK) return rc;
    s->t = t_next;
    if (s->p_drop > 0.0f) s->dropout_step += 1;
    return SPEX_OK;
}

// NGCF with L >= 2 layers: see include/spex_hip.h (spex_ngcf_deep_step_t).  What NGCFStepper.step issued launch by launch from Python
// (~16 launches at ~9 us of host time each) as one native sequence, with the last layer's forward taken at the batch's rows only.
extern "C" int spex_ngcf_deep_step_bce_f32(spex_ngcf_deep_step_t *s, const int64_t *users, const int64_t *items, const float *labels,
                                           int32_t B, float *loss_sum, void *stream)
{
    const char *who = "spex_ngcf_deep_step_bce_f32";
    SPEX_CHECK_ARG(s && s->graph && s->graph_t && s->E0 && s->mE && s->vE && s->W && s->mW && s->vW && s->gW && s->all_emb && s->g_all && s->sides
                       && s->egos && s->g_slots && s->g_side_c && s->g_ego_c && s->gW_parts && s->g_side && s->g_ego && s->g_next && s->p_drop,
                   "%s: NULL field in the step descriptor", who);
    SPEX_CHECK_ARG(users && items && labels && loss_sum && B >= 1, "%s: NULL batch pointer or B < 1", who);
    const spex_graph *g = s->graph, *gt = s->graph_t;
    const int32_t d = 64, n = g->n_rows, n_u = s->n_user_rows, L = s->L, ld = d * (L + 1), per = 2 * (d * d + d);
    SPEX_CHECK_ARG(L >= 2 && L <= 8, "%s: L = %d (two to eight layers; one layer: spex_ngcf_step_bce_f32)", who, L);
    SPEX_CHECK_ARG(g->n_rows == g->n_cols && gt->n_rows == n && gt->n_cols == n && n_u >= 0 && n_u <= n, "%s: square graphs of one size, 0 <= n_user_rows <= N", who);
    SPEX_CHECK_ARG(s->slot_capacity >= 2 * B, "%s: slot capacity %d < 2 B = %d", who, s->slot_capacity, 2 * B);
    SPEX_CHECK_ARG(g->mask_mode == 0 && gt->mask_mode == 0, "%s: edge dropout does not apply to NGCF", who);
    const size_t sz = (size_t)n * d;
    const uint32_t step = (uint32_t)s->dropout_step;
    bool any_drop = false;
    for (int32_t l = 0; l < L; ++l) {
        SPEX_CHECK_ARG(s->p_drop[l] >= 0.0f && s->p_drop[l] < 1.0f, "%s: p_drop[%d] = %f", who, l, (double)s->p_drop[l]);
        any_drop = any_drop || s->p_drop[l] > 0.0f;
    }
    auto Wl = [&](int32_t l, const float *&W_gc, const float *&b_gc, const float *&W_bi, const float *&b_bi) {
        const float *w = s->W + (size_t)l * per;
        W_gc = w; b_gc = w + d * d; W_bi = w + d * d + d; b_bi = w + 2 * d * d + d;
    };
    auto ego_of = [&](int32_t l) -> float * { return l == 0 ? s->E0 : s->egos + (size_t)(l - 1) * sz; };
    const float *W_gc, *b_gc, *W_bi, *b_bi;
    // ---- forward: whole-table layers 0 .. L-2 (each writes [ego |] its normalised output into the concatenated table and its
    //      un-normalised output = the next layer's input), then the last layer at the batch's rows only
    for (int32_t l = 0; l + 1 < L; ++l) {
        float *side = s->sides + (size_t)l * sz;
        SPEX_TRY(spex_spmm_f32(g, ego_of(l), side, nullptr, 1.0f, nullptr, nullptr, 1.0f, d, stream));
        Wl(l, W_gc, b_gc, W_bi, b_bi);
        SPEX_TRY(spex_ngcf_layer_fwd_f32(ego_of(l), side, W_gc, b_gc, W_bi, b_bi, s->all_emb + (size_t)d * l, ld, l == 0 ? 1 : 0, ego_of(l + 1), n, d,
                                         s->slope, s->p_drop[l], s->seed, step, (uint32_t)l, s->pad_row, stream));
    }
    {
        const int32_t l = L - 1;
        float *side = s->sides + (size_t)l * sz;
        SPEX_TRY(spex_spmm_rowlist_f32(g, ego_of(l), users, B, 0, items, B, n_u, side, nullptr, nullptr, 1.0f, d, stream));
        Wl(l, W_gc, b_gc, W_bi, b_bi);
        SPEX_TRY(spex_ngcf_layer_fwd_rows_f32(ego_of(l), side, W_gc, b_gc, W_bi, b_bi, s->all_emb + (size_t)d * l, ld, 0, n, d, s->slope, s->p_drop[l],
                                              s->seed, step, (uint32_t)l, s->pad_row, users, B, 0, items, B, n_u, stream));
    }
    // ---- scoring on the concatenated rows: per-sample gradient rows (the last layer's backward) + the table form (earlier layers)
    SPEX_TRY(spex_score_bce_slots_f32(s->all_emb, s->all_emb + (size_t)n_u * ld, ld, ld, n_u, n - n_u, users, items, labels, B, ld, loss_sum,
                                      s->g_all, s->g_all + (size_t)n_u * ld, 1.0f / (float)B, s->g_slots, ld, stream));
    // ---- backward: the last layer on the batch's slots, A^T g_side in push form, then the dense layers
    float *g_next = s->g_next + (size_t)((L - 1) & 1) * sz;
    {
        const int32_t l = L - 1;
        Wl(l, W_gc, b_gc, W_bi, b_bi);
        SPEX_TRY(spex_ngcf_layer_bwd_rows_f32(ego_of(l), s->sides + (size_t)l * sz, W_gc, b_gc, W_bi, b_bi, s->g_slots + (size_t)d * (l + 1), ld, nullptr,
                                              nullptr, ld, n, d, s->slope, s->p_drop[l], s->seed, step, (uint32_t)l, s->pad_row, users, B, 0, items, B,
                                              n_u, s->g_side_c, s->g_ego_c, s->gW_parts, per, stream));
        SPEX_TRY(spex::zero_f32(g_next, (int64_t)sz, stream));
        SPEX_TRY(spex_spmm_push_batch_f32(g, users, B, 0, items, B, n_u, s->g_side_c, d, s->g_ego_c, d, 1.0f, g_next, d, stream));
    }
    for (int32_t l = L - 2; l >= 0; --l) {
        Wl(l, W_gc, b_gc, W_bi, b_bi);
        float *gw = s->gW + (size_t)l * per;
        SPEX_TRY(spex_ngcf_layer_bwd_f32(ego_of(l), s->sides + (size_t)l * sz, W_gc, b_gc, W_bi, b_bi, s->g_all + (size_t)d * (l + 1), ld, g_next,
                                         l == 0 ? s->g_all : nullptr, ld, n, d, s->slope, s->p_drop[l], s->seed, step, (uint32_t)l, s->pad_row,
                                         s->g_side, s->g_ego, gw, gw + d * d, gw + d * d + d, gw + 2 * d * d + d, stream));
        float *out = s->g_next + (size_t)(l & 1) * sz;
        SPEX_TRY(spex_spmm_f32(gt, s->g_side, out, s->g_ego, 1.0f, nullptr, nullptr, 1.0f, d, stream));
        g_next = out;
    }
    // ---- Adam: the table, the last layer's weights (from their partial blocks), the other layers' (their pass clears gW); the table
    //      form of the scoring gradient is cleared for the next step
    const int32_t t_next = s->t + 1;
    SPEX_TRY(spex::adam_step_z2(s->E0, g_next, s->mE, s->vE, (int64_t)sz, t_next, s->lr, s->beta1, s->beta2, s->eps, nullptr, nullptr, stream));
    const size_t lo = (size_t)(L - 1) * per;
    SPEX_TRY(spex_adam_step_sum_f32(s->W + lo, s->gW_parts, spex_ngcf_layer_bwd_rows_parts(2 * B), per, s->mW + lo, s->vW + lo, per, t_next, s->lr,
                                    s->beta1, s->beta2, s->eps, stream));
    SPEX_TRY(spex::adam_step_z2(s->W, s->gW, s->mW, s->vW, (int64_t)lo, t_next, s->lr, s->beta1, s->beta2, s->eps, s->gW, nullptr, stream));
    SPEX_TRY(spex::zero_f32(s->g_all, (int64_t)n * ld, stream));
    s->t = t_next;
    if (any_drop) s->dropout_step += 1;
    return SPEX_OK;
}

extern "C" int spex_dual_task_step_join(spex_dual_task_step_t *s, void *stream)
{
    SPEX_CHECK_ARG(s, "spex_dual_task_step_join: NULL descriptor");
    if (s->side_pending && s->ev_join) SPEX_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)s->ev_join, 0));
    s->side_pending = 0;
    return SPEX_OK;
}

extern "C" int spex_dual_task_step_f32(spex_dual_task_step_t *s, const int64_t *users, const int64_t *items, const float *labels,
                                       int32_t B, const int64_t *seq, const int64_t *seq_l, const int64_t *targets, int32_t T,
                                       void *stream)
{
    SPEX_CHECK_ARG(s && s->graph && s->graph_t && s->params && s->m && s->v && s->light && s->ws_fwd && s->lo_batch && s->g_prop
                       && s->g_raw && s->g_E0 && s->ws_bwd && s->mixed_slots && s->grad_slots && s->g_prop_slots && s->arange && s->g_user
                       && s->g_small && s->a2 && s->trust_ws && s->dscore && s->loss_b && s->loss && s->loss_acc && s->precision,
                   "spex_dual_task_step_f32: NULL field in the step descriptor");
    SPEX_CHECK_ARG(users && items && labels && B >= 1, "spex_dual_task_step_f32: NULL batch pointer or B < 1");
    SPEX_CHECK_ARG(T >= 0 && T <= s->path_capacity && (T == 0 || (seq && seq_l && targets)),
                   "spex_dual_task_step_f32: T=%d paths (capacity %d) or NULL path pointer", T, s->path_capacity);
    SPEX_CHECK_ARG(s->slot_capacity >= 2 * B, "spex_dual_task_step_f32: slot capacity %d < 2 B = %d", s->slot_capacity, 2 * B);
    const spex_graph *g = s->graph, *gt = s->graph_t;
    const int32_t d = 64, N = g->n_rows, n_u = s->n_user_rows, L = s->L, H = s->n_heads;
    SPEX_CHECK_ARG(g->n_rows == g->n_cols && gt->n_rows == N && gt->n_cols == N, "spex_dual_task_step_f32: square graphs of one size");
    SPEX_CHECK_ARG(s->d == 64 && L >= 1 && n_u >= 2 && n_u <= N, "spex_dual_task_step_f32: d=%d L=%d n_user_rows=%d (needs d == 64)", s->d, L, n_u);
    // edge dropout on the rec branch (model_expert_s.py:104-109; the trust branch reads the raw user table): as in the LightGCN step —
    // the same mask on both handles, graph_t the transposed handle with the edge-id permutation, L >= 2
    SPEX_CHECK_ARG(g->mask_mode == gt->mask_mode && (g->mask_mode == 0 || (g->keep_prob == gt->keep_prob && g->seed == gt->seed && g->keep == gt->keep)),
                   "spex_dual_task_step_f32: graph and graph_t must carry the same edge-dropout mask");
    SPEX_CHECK_ARG(g->mask_mode == 0 || (gt != g && L >= 2),
                   "spex_dual_task_step_f32: edge dropout needs L >= 2 and graph_t = the transposed handle (with its edge-id permutation)");
    const int64_t n_trust = spex_trust_param_count(d, H);
    SPEX_CHECK_ARG(n_trust > 0, "spex_dual_task_step_f32: unsupported number of heads %d", H);
    const bool det = (s->flags & SPEX_STEP_DETERMINISTIC) != 0;
    if (det)
        SPEX_CHECK_ARG(s->g_raw_slots && s->att_parts && s->loss_rows,
                       "spex_dual_task_step_f32: SPEX_STEP_DETERMINISTIC needs g_raw_slots, att_parts and loss_rows");
    const size_t sz = (size_t)N * d, off_u = (size_t)n_u * d;
    float *E0 = s->params, *trust_p = E0 + sz, *att1 = trust_p + n_trust, *att2 = att1 + 4 * d;
    float *g_att1 = s->g_small + n_trust, *g_att2 = g_att1 + 4 * d;
    // ---- trust branch (:170-192) on the raw user table, forward + backward.  It shares nothing with the rec branch but the
    //      (read-only) parameters, so with a second stream it is issued FIRST, behind the previous step's Adam pass, and its
    //      <= path_capacity workgroups run beside the rec branch's launches; the Adam pass waits for both.
    //      (Beside the rec branch the head keeps to ONE workgroup per path: the rec branch's whole-graph launches bound the step and
    //      want every CU; alone on the caller's stream it splits each path's sweep over up to eight — except in the deterministic
    //      step, whose results must not depend on how the streams are arranged: the fold over shares rounds differently.)
    auto trust_branch = [&](void *st) -> int {
        return spex::trust_head_train(E0, n_u, trust_p, seq, seq_l, targets, T, s->path_len, d, H, s->hybrid, 1.0f, nullptr, s->a2, s->dscore,
                                      s->loss_b, s->trust_ws, s->loss + 1, 0, s->g_small, s->g_user, st == stream && !det ? 8 : 1, st);
    };
    // SPEX_STEP_PIPELINED: the trust branch and the update of what it reads (user rows, trust block, task weights) live on
    // side_stream from one step to the next; `stream` and side_stream exchange two events per step, neither on the trust
    // branch's cycle.  side_pending: side_stream holds work `stream` has not been ordered behind yet.
    const bool pipelined = (s->flags & SPEX_STEP_PIPELINED) != 0 && s->side_stream != nullptr && s->side_stream != stream;
    if (s->side_pending && !pipelined) SPEX_TRY(spex_dual_task_step_join(s, stream));      // (the flags changed between two steps)
    const bool two_streams = !pipelined && s->side_stream != nullptr && s->side_stream != stream && T > 0;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    int rc_trust = SPEX_OK;
    bool forked = false;
    if (pipelined) {
        SPEX_TRY(step_events(&s->ev_fork, &s->ev_join, &fork_ev, &join_ev));
        if (!s->side_pending) {            // first step after a join: side_stream starts behind everything queued on `stream`
            SPEX_HIP(hipEventRecord(fork_ev, (hipStream_t)stream));
            SPEX_HIP(hipStreamWaitEvent((hipStream_t)s->side_stream, fork_ev, 0));
        } else {                           // the previous step's side update (user rows!) in front of this step's rec branch
            SPEX_HIP(hipStreamWaitEvent((hipStream_t)stream, join_ev, 0));
        }
        s->side_pending = 1;
        if (T > 0) rc_trust = trust_branch(s->side_stream);
    }
    if (two_streams) {
        SPEX_TRY(step_events(&s->ev_fork, &s->ev_join, &fork_ev, &join_ev));
        SPEX_HIP(hipEventRecord(fork_ev, (hipStream_t)stream));
        SPEX_HIP(hipStreamWaitEvent((hipStream_t)s->side_stream, fork_ev, 0));
        forked = true;
        rc_trust = trust_branch(s->side_stream);
        if (hipEventRecord(join_ev, (hipStream_t)s->side_stream) != hipSuccess && rc_trust == SPEX_OK) rc_trust = SPEX_ERR_HIP;
    }
    // the fused batch kernel's copies of the two gate gradients live in grad_slots (per-sample rows on the other paths): up to 64
    // copies of 512 floats, summed and cleared by the Adam pass — which clears the area after the other paths too, so that a
    // descriptor may change its flags between steps
    const int32_t att_copies_max = s->slot_capacity / 8 < 64 ? s->slot_capacity / 8 : 64;
    int32_t att_copies_used = 0;
    bool fused_middle_used = false;
    bool plain_last = false;          // the rec branch left the g_prop / (L+1) share of its last backward product to the Adam pass
    auto rec_branch = [&]() -> int {
        // ---- rec branch forward (model_expert_s.py:95-126,154-168): layers 1 .. L-1 over the whole graph, the last layer, the gate and
        //      the scores only at the batch's rows
        //      (whole-graph launches in the plain form for L <= 3, the layer sum formed at the batch's rows: see the LightGCN step)
        const bool plain = L >= 2 && L <= 3;
        const float *cur = nullptr;
        SPEX_TRY(forward_layers(g, E0, s->light, s->ws_fwd, L, L - 1, d, stream, &cur));
        if (!det && L >= 2) {
            // (fast path: last layer at the batch's rows + layer mean + gate + scores + the gate's backward + the first backward
            //  product in push form — ONE launch, batch.hip: gated_batch_push_kernel; then the L-1 pull-form launches on A^T, the
            //  last one plain: the Adam pass adds its g_prop / (L+1) share, see the LightGCN step)
            float *G = s->ws_bwd;                     // all-zero here (cleared by the previous step's Adam pass)
            SPEX_TRY(spex::gated_batch_push_layers(g, cur, plain ? E0 : s->light, plain ? s->ws_fwd : nullptr,
                                                   plain && L == 3 ? s->ws_fwd + sz : nullptr, (float)(L + 1), E0, att1, att2, users, items,
                                                   labels, B, n_u, 1.0f / (float)B, 1.0f / (float)(L + 1), s->loss,
                                                   L == 3 ? nullptr : s->g_prop /* L == 3: nothing reads it (all-plain backward) */, G, s->g_raw,
                                                   att_copies_max >= 1 ? s->grad_slots : g_att1, att_copies_max >= 1 ? att_copies_max : 1,
                                                   d, stream));
            att_copies_used = att_copies_max;
            fused_middle_used = true;
            // (L == 3: both products plain, the Adam pass adds the push target P instead of g_prop / 4 — see step_backward_pulls)
            SPEX_TRY(step_backward_pulls(gt, G, L - 2, s->g_prop, s->ws_bwd, s->g_E0, L, d, stream));
            plain_last = true;
            return SPEX_OK;
        }
        // (L == 1 and the deterministic step: last layer at the batch's rows + layer mean + gate + scores + per-sample gradient
        //  rows in one launch, the gate's backward and the propagation's after it)
        SPEX_TRY(spex::gated_batch_fwd_layers(g, cur, plain || L == 1 ? E0 : s->light, plain ? s->ws_fwd : nullptr,
                                              plain && L == 3 ? s->ws_fwd + sz : nullptr, (float)(L + 1), E0, att1, att2, users, items,
                                              labels, B, n_u, 1.0f / (float)B, s->loss, det ? s->loss_rows : nullptr, s->lo_batch,
                                              s->grad_slots, d, stream));
        if (det) {
            // ---- SPEX_STEP_DETERMINISTIC: every sum the fast path leaves to float atomics is taken in a fixed order — the loss in
            //      sample order, the gate's backward into per-slot rows + per-workgroup blocks of the two gate gradients (added in
            //      block order), the slots per table row in ascending slot order, the propagation's backward in pull form.
            SPEX_TRY(spex::sum_ordered(s->loss_rows, B, 1.0f, s->loss, 1, stream));
            SPEX_TRY(spex_expert_gate_rows_bwd_det_f32(E0, s->lo_batch, att1, att2, users, B, 0, items, B, n_u, n_u, N, d, s->grad_slots, d,
                                                       s->g_prop_slots, s->g_raw_slots, s->att_parts, stream));
            const int32_t n_parts = spex_expert_gate_rows_bwd_parts(2 * B);
            SPEX_TRY(spex::sum_parts(s->att_parts, n_parts, 512, 256, g_att1, 1, stream));
            SPEX_TRY(spex::sum_parts(s->att_parts + 256, n_parts, 512, 256, g_att2, 1, stream));
            SPEX_TRY(spex_reduce_slots_f32(users, B, 0, items, B, n_u, N, s->g_prop_slots, d, 1.0f, s->g_prop, 0, d, stream));
            SPEX_TRY(spex_reduce_slots_f32(users, B, 0, items, B, n_u, N, s->g_raw_slots, d, 1.0f, s->g_raw, 0, d, stream));
            SPEX_TRY(spex_propagate_bwd_f32(gt, s->g_prop, s->g_E0, s->ws_bwd, L, d, stream));
            return SPEX_OK;
        }
        // ---- L == 1: rec branch backward (gradients of the UNWEIGHTED loss1; the precisions are applied in the Adam pass): the gate slot
        //      by slot (dense d loss / d light and d loss / d E0 rows added with atomics), then the one pull-form product
        SPEX_TRY(spex_expert_gate_rows_bwd_f32(E0, s->lo_batch, att1, att2, users, B, 0, items, B, n_u, n_u, N, d, s->grad_slots, d,
                                               s->g_prop_slots, s->g_prop, s->g_raw, g_att1, g_att2, stream));
        SPEX_TRY(spex_propagate_bwd_f32(gt, s->g_prop, s->g_E0, s->ws_bwd, L, d, stream));
        return SPEX_OK;
    };
    int rc = rec_branch();
    if (forked && hipStreamWaitEvent((hipStream_t)stream, join_ev, 0) != hipSuccess && rc == SPEX_OK) rc = SPEX_ERR_HIP;   // joined on every path
    if (rc == SPEX_OK) rc = rc_trust;
    // what the Adam pass adds to the last (plain) backward product: g_prop / (L+1), or — L == 3, both products plain — the push
    // target itself (prop_div < 0)
    const float prop_div = !plain_last ? 0.0f : (L == 3 ? -1.0f : (float)(L + 1));
    const int32_t clear_prop = fused_middle_used && L == 3 ? 0 : 1;      // (the fused middle of the L == 3 step never wrote g_prop)
    if (pipelined) {
        // the rec branch's gradients -> side_stream; Adam part 2 (user rows, trust block, task weights, loss cells) there, part 1
        // (item rows, gate matrices) here.  The join event is recorded on every path so that a later join never waits in vain.
        if (hipEventRecord(fork_ev, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent((hipStream_t)s->side_stream, fork_ev, 0) != hipSuccess)
            rc = rc == SPEX_OK ? SPEX_ERR_HIP : rc;
        for (int32_t part = 2; part >= 1 && rc == SPEX_OK; --part)
            rc = spex::dual_task_adam(s->params, s->m, s->v, s->g_E0, s->g_raw, s->g_user, s->g_small, s->g_prop, L >= 2 ? s->ws_bwd : nullptr,
                                      s->loss, s->loss_acc, s->precision, (int64_t)sz, (int64_t)off_u, n_trust, B, T, s->n_rec, s->t + 1, s->lr,
                                      s->beta1, s->beta2, s->eps, (s->flags & SPEX_STEP_FIXED_TASK_WEIGHTS) != 0,
                                      part == 2 ? s->side_stream : stream, prop_div, s->grad_slots, att_copies_used,
                                      att_copies_max * 512, part, clear_prop);
        if (hipEventRecord(join_ev, (hipStream_t)s->side_stream) != hipSuccess && rc == SPEX_OK) rc = SPEX_ERR_HIP;
        if (rc != SPEX_OK) {
            (void)spex_dual_task_step_join(s, stream);
            return rc;
        }
        s->t += 1;
        return SPEX_OK;
    }
    if (rc == SPEX_OK && T > 0 && !two_streams) rc = trust_branch(stream);                // one-stream order
    if (rc != SPEX_OK) return rc;
    // ---- uncertainty-weighted sum of both losses (main_auto_expert_s.py:78-82; SPEX_STEP_FIXED_TASK_WEIGHTS: loss1 + loss2,
    //      main_11.py:69) + Adam over every parameter (:89); t is advanced once the whole step is queued
    SPEX_TRY(spex::dual_task_adam(s->params, s->m, s->v, s->g_E0, s->g_raw, s->g_user, s->g_small, s->g_prop, L >= 2 ? s->ws_bwd : nullptr,
                                  s->loss, s->loss_acc, s->precision, (int64_t)sz, (int64_t)off_u, n_trust, B, T, s->n_rec, s->t + 1, s->lr,
                                  s->beta1, s->beta2, s->eps, (s->flags & SPEX_STEP_FIXED_TASK_WEIGHTS) != 0, stream,
                                  prop_div, s->grad_slots, att_copies_used, att_copies_max * 512, 0, clear_prop));
    s->t += 1;
    return SPEX_OK;
}

// Train() of main_auto_expert_s.py:60-91 over a whole pre-shuffled, device-resident epoch as ONE call: batch k = samples [k B, (k+1) B)
// with the paths [path_off[k], path_off[k+1]) of the epoch's staged path arrays (seq [*, path_len], seq_l, targets: the reference's
// per-batch selection, made up front by the host) through spex_dual_task_step_f32.  Both losses accumulate in the descriptor's
// loss_acc.  keep_prob < 1: the rec branch's sampled edge mask, a fresh one per step (as spex_lightgcn_epoch_bce_f32).
extern "C" int spex_dual_task_epoch_f32(spex_dual_task_step_t *s, const int64_t *users, const int64_t *items, const float *labels, int64_t n,
                                        int32_t B, int64_t max_steps, const int64_t *seq, const int64_t *seq_l, const int64_t *targets,
                                        const int64_t *path_off, float keep_prob, uint32_t drop_seed, void *stream)
{
    SPEX_CHECK_ARG(s && s->graph && s->graph_t && users && items && labels && path_off && n >= 0 && B >= 1,
                   "spex_dual_task_epoch_f32: NULL pointer, n < 0 or B < 1");
    SPEX_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f, "spex_dual_task_epoch_f32: keep_prob %g", keep_prob);
    return epoch_loop(s->graph, s->graph_t, n, B, max_steps, keep_prob, drop_seed, [&](int64_t k, int64_t b0, int32_t nb) {
        const int64_t p0 = path_off[k], T = path_off[k + 1] - p0;
        if (T < 0 || (T > 0 && !(seq && seq_l && targets))) {          // (in front of the batch's first launch)
            spex::set_error("spex_dual_task_epoch_f32: batch %lld has %lld paths (offsets must ascend; path arrays must be given)", (long long)k,
                            (long long)T);
            return (int)SPEX_ERR_INVALID;
        }
        return spex_dual_task_step_f32(s, users + b0, items + b0, labels + b0, nb, T ? seq + p0 * s->path_len : nullptr, T ? seq_l + p0 : nullptr,
                                       T ? targets + p0 : nullptr, (int32_t)T, stream);
    });
}

// spex_dual_task_epoch_f32 over paths staged with a fixed stride: batch k's paths are the first h_count[k] rows from row
// k * path_stride of seq / seq_l / targets — the layout spex_sample_dual_task_paths writes (stride = its cap) — and h_count is a HOST
// array (the step needs T there: the trust launch's grid and the T * task_weights[1] term).  Every count is checked before the first
// launch.  Edge-dropout keys, loss_acc and max_steps as in spex_dual_task_epoch_f32.
extern "C" int spex_dual_task_epoch_strided_f32(spex_dual_task_step_t *s, const int64_t *users, const int64_t *items, const float *labels,
                                                int64_t n, int32_t B, int64_t max_steps, const int64_t *seq, const int64_t *seq_l,
                                                const int64_t *targets, int64_t path_stride, const int32_t *h_count, float keep_prob,
                                                uint32_t drop_seed, void *stream)
{
    SPEX_CHECK_ARG(s && s->graph && s->graph_t && users && items && labels && h_count && n >= 0 && B >= 1 && path_stride >= 0,
                   "spex_dual_task_epoch_strided_f32: NULL pointer, n < 0, B < 1 or path_stride < 0");
    SPEX_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f, "spex_dual_task_epoch_strided_f32: keep_prob %g", keep_prob);
    int64_t n_batches = (n + B - 1) / B;
    if (max_steps >= 0 && max_steps < n_batches) n_batches = max_steps;
    for (int64_t k = 0; k < n_batches; ++k) {
        const int64_t T = h_count[k];
        SPEX_CHECK_ARG(T >= 0 && T <= path_stride && T <= s->path_capacity && (T == 0 || (seq && seq_l && targets)),
                       "spex_dual_task_epoch_strided_f32: batch %lld has %lld paths (stride %lld, capacity %d; path arrays must be given)",
                       (long long)k, (long long)T, (long long)path_stride, s->path_capacity);
    }
    return epoch_loop(s->graph, s->graph_t, n, B, max_steps, keep_prob, drop_seed, [&](int64_t k, int64_t b0, int32_t nb) {
        const int64_t p0 = k * path_stride;
        const int32_t T = h_count[k];
        return spex_dual_task_step_f32(s, users + b0, items + b0, labels + b0, nb, T ? seq + p0 * s->path_len : nullptr, T ? seq_l + p0 : nullptr,
                                       T ? targets + p0 : nullptr, T, stream);
    });
}
