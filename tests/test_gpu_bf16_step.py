"""bf16 gather tables in the one-call LightGCN steps and epochs (SPEX_STEP_BF16_GATHER; d = 64, L = 2 or 3).

Inputs: the Epinion2 fixture and the hub graph of tests/test_gpu_bpr_exact_step.py (whose helpers and fp64 truth are imported, so a
truth computed there is computed once).  The yardstick throughout is the launch-by-launch step of a gather_dtype=torch.bfloat16
stepper: SpexGraph.propagate / propagate_bwd with gather_dtype=torch.bfloat16 around the fp32 scoring kernels — kernels merged before
this mode existed.  Every test prints the figures it asserts on."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_bpr_exact_step import DEV, N_I, N_U, epi, epi_truth, hub_graph, rel_err, t, triples, truth_steps
from test_gpu_wide_step import training_batches

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
_cache = {}


@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


def _stepper(G, epinion2, L=3, deterministic=False, transposed=False, weight_decay=0.0, bf16=True, E0=None):
    from spex_amd.graph import csr_transpose
    from spex_amd.trainer import LightGCNStepper
    csr, E0_np = epi(epinion2)
    gt = None
    if transposed:
        t_rowptr, t_col, t_val, eid = csr_transpose(*csr, len(E0_np))
        gt = G(t_rowptr, t_col, t_val, edge_id=eid)
    return LightGCNStepper(G(*csr), t(E0_np.copy()) if E0 is None else E0, N_U, n_layers=L, lr=1e-3, graph_t=gt,
                           deterministic=deterministic, weight_decay=weight_decay, gather_dtype=BF16 if bf16 else None)


def bits(x16):
    return x16.view(torch.int16)


def shadow_is_current(st):
    return torch.equal(bits(st.E0_16), bits(st.E0.to(BF16)))


def state(st):
    return st.E0.clone(), st.m.clone(), st.v.clone(), st.E0_16.clone() if st.E0_16 is not None else None


def states_equal(a, b):
    return all(torch.equal(x, y) if x.dtype != BF16 else torch.equal(bits(x), bits(y)) for x, y in zip(a, b) if x is not None)


def truth_steps_bce(csr, E0, n_u, L, batches, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """truth_steps (test_gpu_bpr_exact_step.py) with the BCE loss of the reference's step: per step (mean loss, E0, m, v) in fp64."""
    rowptr, col, val = csr
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, col.astype(np.int64)])), torch.from_numpy(val.astype(np.float64)), (n, n)).coalesce()
    W = torch.from_numpy(E0.astype(np.float64))
    m, v = torch.zeros_like(W), torch.zeros_like(W)
    out = []
    for s, (u, i, y) in enumerate(batches):
        u, i = (torch.from_numpy(np.asarray(a, np.int64)) for a in (u, i))
        y = torch.from_numpy(np.asarray(y, np.float64))
        Wr = W.clone().requires_grad_(True)
        cur, acc = Wr, Wr
        for _ in range(L):
            cur = torch.sparse.mm(A, cur)
            acc = acc + cur
        light = acc / (L + 1)
        x = (light[u] * light[n_u + i]).sum(1)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x, y)
        loss.backward()
        g = Wr.grad
        step = s + 1
        m = m + (1 - beta1) * (g - m)
        v = beta2 * v + (1 - beta2) * g * g
        denom = v.sqrt() / np.sqrt(1 - beta2 ** step) + eps
        W = W - (lr / (1 - beta1 ** step)) * (m / denom)
        out.append((float(loss.detach()), W.numpy().copy(), m.numpy().copy(), v.numpy().copy()))
    return out


# ------------------------------------------------------------------------------------------ 1. kernel against its fp32 sibling
def _hub_inputs(G, mode):
    """The hub graph's handle under `mode` ("none", "injected": keep mask, keep_prob 0.6, "sampled": the in-kernel mask), a bf16
    table, its widening, a running-sum table and an E0 table."""
    csr, n_u = hub_graph()
    n = len(csr[0]) - 1
    rng = np.random.default_rng(77)
    g = G(*csr)
    if mode == "injected":
        g.set_edge_mask(1, t((rng.random(len(csr[1])) < 0.6).astype(np.uint8)), 0.6, 0)
    elif mode == "sampled":
        g.set_edge_mask(2, None, 0.6, (9 << 32) | 4)
    X16 = t((rng.normal(size=(n, 64)) * 0.3).astype(np.float32)).to(BF16)
    run = t((rng.normal(size=(n, 64)) * 0.3).astype(np.float32))
    E0 = t((rng.normal(size=(n, 64)) * 0.3).astype(np.float32))
    return csr, n_u, n, g, X16, X16.float().contiguous(), run, E0


def _hub_indices(n, n_u, T, rng):
    """Users / positives / negatives naming a hub row on every side (1 500, 2 600, 1 100 entries), the empty rows 7 and 1 201, the
    64 / 65 boundary rows, a repeated user (T >= 3) and, at T = 17, one index out of range."""
    it = lambda r: r - n_u
    users = np.array(([2, 7, 2, 8, 9, 10] + list(rng.integers(0, n_u, 32)))[:T], np.int64)
    pos = np.array(([it(1500), it(2999), it(1201), it(1200), it(1202), it(1203)] + list(rng.integers(0, n - n_u, 32)))[:T], np.int64)
    neg = np.array(([it(2999), it(1203), it(1500), it(1202), it(1200), it(1201)] + list(rng.integers(0, n - n_u, 32)))[:T], np.int64)
    if T == 17:
        pos[11] = 999999
    return users, pos, neg


@pytest.mark.parametrize("mode", ["none", "injected", "sampled"])
def test_bf16_batch_kernels_equal_their_fp32_siblings_on_the_widened_table(G, mode):
    """On Xw = float(X16) each bf16 kernel returns what its fp32 sibling returns on Xw.  Slots forms (BCE and BPR): loss_per_sample,
    grad_slots and row_counts torch.equal.  Push forms: loss_per_sample equal; g_out within 3e-6 and G within 1e-5, the bounds
    test_bpr_batch_kernel_equals_the_three_launch_sequence (test_gpu_bpr_exact_step.py) gives the fp32 kernel's float atomics."""
    from spex_amd import ops
    csr, n_u, n, g, X16, Xw, run, E0 = _hub_inputs(G, mode)
    L, wd = 3, 1e-2
    rng = np.random.default_rng(3)
    for T in (1, 3, 17):
        users, pos, neg = _hub_indices(n, n_u, T, rng)
        u_d, p_d, n_d = t(users), t(pos), t(neg)
        labels = t((rng.random(T) < 0.5).astype(np.float32))
        # ---- BPR, slots
        out = []
        for fn, X in ((ops.lightgcn_bpr_batch_slots, Xw), (ops.lightgcn_bpr_batch_slots_bf16, X16)):
            slots, per = torch.full((3 * T, 64), 7.0, device=DEV), torch.full((T,), 7.0, device=DEV)
            counts = torch.zeros(n, dtype=torch.int32, device=DEV)
            fn(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, slots, loss_per_sample=per, weight_decay=wd, E0=E0, row_counts=counts)
            out.append((per, slots, counts))
        assert all(torch.equal(a, b) for a, b in zip(*out)), (mode, T, "bpr slots")
        assert out[1][1].abs().max() > 0 and (T < 17 or (out[1][0][11] == 0 and not out[1][1].view(3, T, 64)[:, 11].any()))
        # ---- BPR, push (dense rows and push target), and the dense form alone
        res = []
        for fn, X in ((ops.lightgcn_bpr_batch, Xw), (ops.lightgcn_bpr_batch_bf16, X16)):
            per, g_out, Gp = torch.zeros(T, device=DEV), torch.zeros(n, 64, device=DEV), torch.zeros(n, 64, device=DEV)
            fn(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, 1.0 / (L + 1), None, g_out, Gp, loss_per_sample=per, weight_decay=wd, E0=E0)
            g_only = torch.zeros(n, 64, device=DEV)
            fn(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, 0.0, None, g_only, None, loss_per_sample=torch.zeros(T, device=DEV))
            res.append((per, g_out, Gp, g_only))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[1][0], out[1][0]), (mode, T, "bpr push loss")
        figs = [rel_err(res[1][k].cpu().numpy(), res[0][k].cpu().numpy()) for k in (1, 2, 3)]
        print(f"{mode} T={T} bpr push: g_out {figs[0]:.2e} G {figs[1]:.2e} g_out (dense form) {figs[2]:.2e}")
        assert figs[0] <= 3e-6 and figs[1] <= 1e-5 and figs[2] <= 3e-6
        # ---- BCE, slots and push (items: the positives, one of them out of range at T = 17)
        out = []
        for fn, X in ((ops.lightgcn_batch_slots, Xw), (ops.lightgcn_batch_slots_bf16, X16)):
            slots, per = torch.full((2 * T, 64), 7.0, device=DEV), torch.full((T,), 7.0, device=DEV)
            fn(g, X, run, float(L + 1), u_d, p_d, labels, n_u, 1.0 / T, slots, loss_per_sample=per)
            out.append((per, slots))
        assert all(torch.equal(a, b) for a, b in zip(*out)), (mode, T, "bce slots")
        res = []
        for fn, X in ((ops.lightgcn_batch, Xw), (ops.lightgcn_batch_bf16, X16)):
            per, g_out, Gp = torch.zeros(T, device=DEV), torch.zeros(n, 64, device=DEV), torch.zeros(n, 64, device=DEV)
            fn(g, X, run, float(L + 1), u_d, p_d, labels, n_u, 1.0 / T, 1.0 / (L + 1), None, g_out, Gp, loss_per_sample=per)
            res.append((per, g_out, Gp))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[1][0], out[1][0]), (mode, T, "bce push loss")
        figs = [rel_err(res[1][k].cpu().numpy(), res[0][k].cpu().numpy()) for k in (1, 2)]
        print(f"{mode} T={T} bce push: g_out {figs[0]:.2e} G {figs[1]:.2e}")
        assert figs[0] <= 3e-6 and figs[1] <= 1e-5
    g.set_edge_mask(0)


@pytest.mark.parametrize("mode", ["none", "injected", "sampled"])
def test_bf16_batch_kernel_forward_rows_are_the_bf16_spmm_rows(G, mode):
    """The last-layer rows read back exactly through the slots forms.  BCE kernel: with the item row empty and its running sum zero the
    score is 0, sigmoid(0) = 1/2, and label 0 with grad_scale 2 makes dg exactly 1 — the item-side slot g_i = dg * light_u IS light_u;
    with an all-zero running sum and divisor 1, light_u is the gathered row y.  BPR kernel: an empty user row makes z = 0, dg = 1 with
    grad_scale 2, and with the negative the empty row the user's slot is -light_p.  Rows of at most 1 024 entries must equal
    spex_spmm_bf16_f32's rows bit for bit, under either mask as well."""
    from spex_amd import ops
    csr, n_u, n, g, X16, _, _, _ = _hub_inputs(G, mode)
    deg = np.diff(csr[0])
    EU, EI = 7, 1201 - n_u
    want = g.spmm_bf16(X16)
    zero = torch.zeros(n, 64, device=DEV)
    rng = np.random.default_rng(11)
    for B in (1, 3, 17):
        rows_u = np.array(([9, 10, 8, 2, 7, 9] + list(rng.integers(0, n_u, 32)))[:B], np.int64)
        slots = torch.full((2 * B, 64), 7.0, device=DEV)
        ops.lightgcn_batch_slots_bf16(g, X16, zero, 1.0, t(rows_u), t(np.full(B, EI, np.int64)), torch.zeros(B, device=DEV), n_u, 2.0, slots,
                                      loss_per_sample=torch.zeros(B, device=DEV))
        short = t(deg[rows_u] <= 1024)
        assert torch.equal(slots[B:][short], want[t(rows_u)][short]), (mode, B, "user rows")
        rows_i = np.array(([1202, 1203, 1200, 1201, 2999] + list(rng.integers(n_u, n, 32)))[:B], np.int64)
        slots = torch.full((3 * B, 64), 7.0, device=DEV)
        ops.lightgcn_bpr_batch_slots_bf16(g, X16, zero, 1.0, t(np.full(B, EU, np.int64)), t(rows_i - n_u), t(np.full(B, EI, np.int64)), n_u, 2.0,
                                          slots, loss_per_sample=torch.zeros(B, device=DEV))
        short = t(deg[rows_i] <= 1024)
        assert torch.equal(-slots[:B][short], want[t(rows_i)][short]), (mode, B, "item rows")
        print(f"{mode} B={B}: {int(short.sum())} item rows and the user rows of <= 1024 entries equal spex_spmm_bf16_f32's")
    g.set_edge_mask(0)


# ------------------------------------------------------------------------------------------ 2. the shadow
@pytest.mark.parametrize("form,weight_decay", [("bce", 0.0), ("bce-det", 0.0), ("push", 1e-4), ("push", 0.0), ("dense", 1e-4), ("det", 1e-4)])
def test_shadow_equals_the_cast_of_E0_after_every_step(G, epinion2, form, weight_decay):
    """After each of five one-call steps E0_16, read as int16, equals E0.to(torch.bfloat16): the Adam pass writes both from one
    register, so no cast launch opens the next step."""
    st = _stepper(G, epinion2, deterministic=form.endswith("det"), weight_decay=weight_decay)
    acc = torch.zeros(1, device=DEV)
    if form.startswith("bce"):
        for u, i, y in training_batches(epinion2, 5, seed=41):
            st.step_bce(t(u), t(i), t(y), loss_acc=acc, batch_rows_only=True)
            assert st._shadow_current and shadow_is_current(st)
    else:
        st.bpr_backward = form if form in ("push", "dense") else None
        for u, p, ng in triples(epinion2, 5, seed=41):
            st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True)
            assert st._shadow_current and shadow_is_current(st)
    assert st.t == 5 and not st.g_out.any() and not st.ws_bwd[0].any()      # what the next step accumulates into is left all-zero
    assert not torch.equal(st.E0, t(epi(epinion2)[1]))


# ------------------------------------------------------------------------------------------ 3. the deterministic one-call step
DET_BOUNDS = (2e-5, 2e-5, 2e-5, 4e-5)        # loss sum, E0, m, v: test_one_call_bpr_step_equals_the_launch_by_launch_step's figures


def _twenty(epinion2, kind):
    if kind == "bce":
        return training_batches(epinion2, 18, seed=7) + training_batches(epinion2, 1, B=3, seed=8) + training_batches(epinion2, 1, B=1, seed=9)
    return triples(epinion2, 18, seed=7) + triples(epinion2, 1, T=3, seed=8) + triples(epinion2, 1, T=1, seed=9)


def _step(st, kind, batch, acc, one_call):
    fn = st.step_bce if kind == "bce" else st.step_bpr_exact
    fn(*(t(a) for a in batch), loss_acc=acc, batch_rows_only=one_call)


@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_deterministic_one_call_bf16_step_is_reproducible_and_equals_the_launch_by_launch_step(G, epinion2, kind):
    """20 deterministic steps (256 eighteen times, then 3, then 1): two one-call runs end in bit-identical E0, m, v, E0_16 and equal
    loss sums; against the deterministic launch-by-launch bf16 step the same sequence stays within 2e-5, 2e-5, 2e-5, 4e-5."""
    batches = _twenty(epinion2, kind)
    runs = []
    for one_call in (True, True, False):
        st = _stepper(G, epinion2, deterministic=True, weight_decay=1e-4)
        acc = torch.zeros(1, device=DEV)
        for b in batches:
            _step(st, kind, b, acc, one_call)
        assert st.t == 20
        runs.append((state(st), acc.item()))
    (a, la), (a2, la2), (b, lb) = runs
    assert states_equal(a, a2) and la == la2
    figs = (abs(la - lb) / abs(lb),) + tuple(rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[:3], b[:3]))
    print(f"{kind} det: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert all(f <= bd for f, bd in zip(figs, DET_BOUNDS)), figs


# ------------------------------------------------------------------------------------------ 4. the fast paths against the fp64 truth
# The yardstick's worst figure per quantity (mean loss, E0, m, v) over five steps on Epinion2: the deterministic launch-by-launch step
# of a gather_dtype=torch.bfloat16 stepper against the fp64 truth, as this test prints it.  Figures of the whole-file run on an MI355X
# recorded in DESIGN.md 4.19 (E0 / m / v repeat from run to run; the loss figures sit at fp32's resolution of a mean of 256 losses,
# 6e-8, and that run's are the larger of the two runs made).  The one-call forms may reach twice these.
YARDSTICK = {
    ("bce", 3): (9.742e-08, 3.353e-03, 1.162e-03, 1.241e-03),
    ("bce", 2): (9.618e-08, 8.003e-03, 1.446e-03, 1.121e-03),
    ("bpr", 3): (7.683e-08, 3.720e-03, 1.376e-03, 1.144e-03),
    ("bpr", 2): (1.224e-07, 6.708e-03, 1.326e-03, 9.067e-04),
}


def _truth(epinion2, kind, L):
    key = (kind, L)
    if key not in _cache:
        csr, E0 = epi(epinion2)
        if kind == "bce":
            _cache[key] = truth_steps_bce(csr, E0, N_U, L, training_batches(epinion2, 5, seed=41))
        elif L == 3:
            _cache[key] = epi_truth(epinion2, 1e-4)
        else:
            _cache[key] = truth_steps(csr, E0, N_U, L, triples(epinion2, 5, seed=41), 1e-4)
    return _cache[key]


def _figs(st, acc, n, want):
    loss_o, W, m, v = want
    return (abs(acc.item() / n - loss_o), rel_err(st.E0.cpu().numpy(), W), rel_err(st.m.cpu().numpy(), m), rel_err(st.v.cpu().numpy(), v))


@pytest.mark.parametrize("L", [3, 2])
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_fast_paths_against_the_fp64_truth(G, epinion2, kind, L):
    """Five steps on Epinion2 (BCE at B = 256; BPR at T = 256, weight_decay 1e-4, push and dense forced) against the fp64 truth.  The
    fast paths place the backward's roundings differently from spex_propagate_bwd_bf16_f32, so each quantity may reach twice the
    yardstick's worst figure (at most L differently placed roundings, the atomics' reordering).  Whatever the measurement: the
    deviation of m after step 1 exceeds 1e-6 (the bf16 path ran) and stays below 2 L 2^-8 (no rounding model exceeds it; a wrong
    gather table or a stale shadow lands far outside)."""
    batches = training_batches(epinion2, 5, seed=41) if kind == "bce" else triples(epinion2, 5, seed=41)
    truth = _truth(epinion2, kind, L)
    acc = torch.zeros(1, device=DEV)
    ref = _stepper(G, epinion2, L=L, deterministic=True, weight_decay=1e-4)
    yard = np.zeros(4)
    for s, (b, want) in enumerate(zip(batches, truth)):
        acc.zero_()
        _step(ref, kind, b, acc, False)
        figs = _figs(ref, acc, 256, want)
        yard = np.maximum(yard, figs)
        print(f"yardstick {kind} L={L} step {s + 1}: loss {figs[0]:.3e} E0 {figs[1]:.3e} m {figs[2]:.3e} v {figs[3]:.3e}")
    print(f"yardstick {kind} L={L} worst: " + " ".join(f"{x:.3e}" for x in yard))
    worst_all = {}
    for form in (("fast",) if kind == "bce" else ("push", "dense")):
        st = _stepper(G, epinion2, L=L, weight_decay=1e-4)
        st.bpr_backward = None if kind == "bce" else form
        worst = np.zeros(4)
        for s, (b, want) in enumerate(zip(batches, truth)):
            acc.zero_()
            _step(st, kind, b, acc, True)
            figs = _figs(st, acc, 256, want)
            worst = np.maximum(worst, figs)
            print(f"one-call {kind} {form} L={L} step {s + 1}: loss {figs[0]:.3e} E0 {figs[1]:.3e} m {figs[2]:.3e} v {figs[3]:.3e}")
            if s == 0:
                assert 1e-6 < figs[2] < 2 * L * 2.0 ** -8, (kind, form, L, figs[2])
        print(f"one-call {kind} {form} L={L} worst: " + " ".join(f"{x:.3e}" for x in worst))
        assert st.t == 5 and shadow_is_current(st)
        worst_all[form] = worst
    bound = YARDSTICK[(kind, L)]
    for form, worst in worst_all.items():
        assert all(w <= 2 * y for w, y in zip(worst, bound)), (kind, form, L, worst, bound)


# ------------------------------------------------------------------------------------------ 5. native epochs
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_native_epoch_equals_the_steps_one_by_one(G, epinion2, kind):
    """Deterministic mode, 5 B + 3 samples at B = 256 (a ragged last batch): epoch_bce / epoch_bpr equal the one-call steps issued one
    by one — torch.equal on E0, m, v, E0_16 and on the loss sums."""
    B = 256
    parts = (training_batches(epinion2, 5, seed=21) + training_batches(epinion2, 1, B=3, seed=22)) if kind == "bce" else \
            (triples(epinion2, 5, seed=21) + triples(epinion2, 1, T=3, seed=22))
    cols = [t(np.concatenate([p[k] for p in parts])) for k in range(3)]
    a, b = (_stepper(G, epinion2, deterministic=True, weight_decay=1e-4) for _ in range(2))
    loss_a, loss_b = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
    (a.epoch_bce if kind == "bce" else a.epoch_bpr)(*cols, B, loss_a[0], loss_a[1])
    for k in range(6):
        sl = slice(k * B, min((k + 1) * B, cols[0].numel()))
        fn = b.step_bce if kind == "bce" else b.step_bpr_exact
        fn(*(c[sl].contiguous() for c in cols), loss_acc=loss_b[0 if k < 5 else 1], batch_rows_only=True)
    assert a.t == b.t == 6
    print(f"{kind}: epoch loss sums {loss_a.flatten().tolist()} step by step {loss_b.flatten().tolist()}")
    assert torch.equal(loss_a, loss_b) and states_equal(state(a), state(b))
    assert shadow_is_current(a)


def test_train_bpr_sampled_equals_the_sampled_epochs_one_by_one(G, epinion2):
    """train_bpr_sampled over two epochs with max_steps=3 equals two epoch_bpr_sampled calls (deterministic mode: torch.equal)."""
    from spex_amd.trainer import BprDeviceSampler, bpr_epoch_drop_seed
    T = 256
    s = BprDeviceSampler(epinion2["train"][:, :2], N_U, N_I, DEV, seed=31, by="user", n=4 * T)
    a, b = (_stepper(G, epinion2, deterministic=True, weight_decay=1e-4) for _ in range(2))
    la, lb = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    a.train_bpr_sampled(s, 2, T, la, max_steps=3)
    for e in range(2):
        b.epoch_bpr_sampled(s, e, T, lb[2 * e:2 * e + 1], lb[2 * e + 1:2 * e + 2], max_steps=3, drop_seed=bpr_epoch_drop_seed(0, e))
    assert a.t == b.t == 6
    assert torch.equal(la, lb) and states_equal(state(a), state(b)) and shadow_is_current(a)


# ------------------------------------------------------------------------------------------ 6. mixed sequences on one stepper
def _distinct_triples(rng, T):
    """T triples without a repeated row: the float atomics of step_bpr_sgd and of the launch-by-launch scoring then add once per row."""
    u = rng.choice(N_U, T, replace=False)
    it = rng.choice(N_I, 2 * T, replace=False)
    return u.astype(np.int64), it[:T].astype(np.int64), it[T:].astype(np.int64)


def test_mixed_step_kinds_keep_the_shadow_current(G, epinion2):
    """Deterministic mode: a bf16 one-call step, a launch-by-launch step, step_bpr_sgd, a one-call step again.  The stepper re-casts
    the shadow by itself wherever another path wrote E0: the run is torch.equal to the same sequence with refresh_gather_table() called
    before each one-call step.  A stepper without gather_dtype run beside it is unaffected."""
    rng = np.random.default_rng(6)
    one_a, one_b = triples(epinion2, 2, seed=33)
    lbl, sgd = _distinct_triples(rng, 8), _distinct_triples(rng, 8)
    runs = []
    for explicit in (False, True):
        st = _stepper(G, epinion2, deterministic=True, weight_decay=1e-4)
        beside = _stepper(G, epinion2, deterministic=True, weight_decay=1e-4, bf16=False) if not explicit else None
        acc = torch.zeros(1, device=DEV)
        for k, (kind, b) in enumerate((("one", one_a), ("lbl", lbl), ("sgd", sgd), ("one", one_b))):
            for s in (st, beside):
                if s is None:
                    continue
                if kind == "one":
                    if explicit:
                        s.refresh_gather_table()
                    s.step_bpr_exact(*(t(a) for a in b), loss_acc=acc, batch_rows_only=True)
                elif kind == "lbl":
                    s.step_bpr_exact(*(t(a) for a in b), loss_acc=acc, batch_rows_only=False)
                else:
                    s.step_bpr_sgd(*(t(a) for a in b), lr=0.05)
            assert st._shadow_current == (kind == "one")
        assert shadow_is_current(st)
        runs.append((state(st), None if beside is None else state(beside)))
    assert states_equal(runs[0][0], runs[1][0])
    alone = _stepper(G, epinion2, deterministic=True, weight_decay=1e-4, bf16=False)
    acc = torch.zeros(1, device=DEV)
    alone.step_bpr_exact(*(t(a) for a in one_a), loss_acc=acc, batch_rows_only=True)
    alone.step_bpr_exact(*(t(a) for a in lbl), loss_acc=acc, batch_rows_only=False)
    alone.step_bpr_sgd(*(t(a) for a in sgd), lr=0.05)
    alone.step_bpr_exact(*(t(a) for a in one_b), loss_acc=acc, batch_rows_only=True)
    assert states_equal(runs[0][1], state(alone))
    assert not torch.equal(runs[0][0][0], runs[0][1][0])                   # (the two modes do differ)


# ------------------------------------------------------------------------------------------ 7. edge dropout
def test_one_call_bf16_step_under_edge_dropout(G, epinion2):
    """Three deterministic one-call steps under a fresh sampled mask per step against the launch-by-launch bf16 steps under the same
    masks: loss, E0, m, v within 2e-5, 2e-5, 2e-5, 4e-5; the tables differ from the unmasked run's by more than 1e-4 relative; and
    epoch_bce(keep_prob=0.3) leaves both handles unmasked."""
    from spex_amd.trainer import edge_dropout_mask
    batches = training_batches(epinion2, 3, seed=13)
    out = []
    for one_call, masked in ((True, True), (False, True), (True, False)):
        st = _stepper(G, epinion2, deterministic=True, transposed=True)
        acc = torch.zeros(1, device=DEV)
        for k, b in enumerate(batches):
            if masked:
                st.set_edge_dropout(edge_dropout_mask(st.graph, 0.3, "philox", 5, k + 1))
            _step(st, "bce", b, acc, one_call)
        st.set_edge_dropout(None)
        assert not one_call or shadow_is_current(st)
        out.append((state(st), acc.item(), st))
    (a, la, st_a), (b, lb, _), (c, _, _) = out
    figs = (abs(la - lb) / abs(lb),) + tuple(rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[:3], b[:3]))
    moved = tuple(rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[:2], c[:2]))
    print(f"dropout: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}; against the unmasked run E0 {moved[0]:.2e} m {moved[1]:.2e}")
    assert all(f <= bd for f, bd in zip(figs, DET_BOUNDS)), figs
    assert moved[0] > 1e-4 and moved[1] > 1e-4
    # the native epoch under dropout leaves the handles unmasked: a product on each handle is what it was before the epoch
    before = [h.spmm_bf16(st_a.E0_16).clone() for h in (st_a.graph, st_a.graph_t)]
    X16 = st_a.E0_16.clone()
    u, i, y = (t(np.concatenate([bb[k] for bb in batches])) for k in range(3))
    loss = torch.zeros(2, 1, device=DEV)
    st_a.epoch_bce(u, i, y, 256, loss[0], loss[1], keep_prob=0.3, drop_seed=3)
    assert st_a.t == 6 and shadow_is_current(st_a) and loss[0].item() > 0
    for h, want in zip((st_a.graph, st_a.graph_t), before):
        assert torch.equal(h.spmm_bf16(X16), want)


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_state_untouched(G, epinion2):
    """Every refused descriptor returns its code before anything touches the device, names the cause in spex_last_error(), and leaves
    t, E0 and the loss cell as they were."""
    from spex_amd import _lib
    from spex_amd.trainer import LightGCNStepper
    lib = _lib.load()
    st = _stepper(G, epinion2, weight_decay=1e-4)
    T = 17
    d = st._prepare_desc(T, 3)
    u, p, ng = (t(a) for a in triples(epinion2, 1, T=T, seed=3)[0])
    y = torch.ones(T, device=DEV)
    E0_before = st.E0.clone()
    acc = torch.zeros(1, device=DEV)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    good = {k: getattr(d, k) for k in ("d", "L", "E0_16", "ws16", "flags")}
    INVALID, UNSUPPORTED = -1, -4
    cases = [
        (dict(d=128), UNSUPPORTED, "d == 64"), (dict(L=1), UNSUPPORTED, "L = 2 or 3"), (dict(L=4), UNSUPPORTED, "L = 2 or 3"),
        (dict(E0_16=None), INVALID, "NULL E0_16"), (dict(E0_16=good["E0_16"] + 2), INVALID, "E0_16 must be 16-byte aligned"),
        (dict(E0_16=st.E0.data_ptr()), INVALID, "E0_16 aliases"), (dict(E0_16=st.grad_E0.data_ptr() + 64), INVALID, "E0_16 aliases"),
        (dict(ws16=None), INVALID, "NULL ws16"), (dict(ws16=good["ws16"] + 2), INVALID, "ws16 must be 16-byte aligned"),
        (dict(ws16=st.m.data_ptr()), INVALID, "ws16 aliases"), (dict(ws16=good["E0_16"]), INVALID, "ws16 aliases E0_16"),
        (dict(flags=good["flags"] | _lib.STEP_WIDE), INVALID, "SPEX_STEP_WIDE"),
    ]
    for change, code, text in cases:
        for entry in ("bpr", "bce"):
            for k, v in good.items():
                setattr(d, k, v)
            for k, v in change.items():
                setattr(d, k, v)
            if entry == "bpr":
                rc = lib.spex_lightgcn_step_bpr_adam_f32(ctypes.byref(d), vp(u), vp(p), vp(ng), T, vp(acc), None)
            else:
                rc = lib.spex_lightgcn_step_bce_f32(ctypes.byref(d), vp(u), vp(p), vp(y), T, vp(acc), None)
            msg = lib.spex_last_error().decode()
            assert rc == code and text in msg, (change, entry, rc, msg)
            assert d.t == 0
    for k, v in good.items():
        setattr(d, k, v)
    torch.cuda.synchronize()
    assert torch.equal(st.E0, E0_before) and acc.item() == 0.0 and shadow_is_current(st)
    # the restored descriptor still steps
    st.step_bpr_exact(u, p, ng, loss_acc=acc, batch_rows_only=True)
    assert st.t == 1 and acc.item() > 0 and shadow_is_current(st)
    csr, E0 = epi(epinion2)
    with pytest.raises(ValueError, match="width of 64"):
        LightGCNStepper(G(*csr), torch.zeros(len(E0), 128, device=DEV), N_U, gather_dtype=BF16)
    with pytest.raises(ValueError, match="n_layers 2 or 3"):
        LightGCNStepper(G(*csr), t(E0.copy()), N_U, n_layers=1, gather_dtype=BF16)
