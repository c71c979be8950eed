"""Exact BPR training at embedding widths 128 and 256: the wide triple-shaped batch kernel (lightgcn_bpr_batch_wide_kernel<PUSH, V>),
the one-call step spex_lightgcn_step_bpr_adam_f32 under SPEX_STEP_WIDE, the Adam pass's L2 form on rows of 128 / 256, and the
native epochs.  The d == 64 twin of every test is in tests/test_gpu_bpr_exact_step.py; the inputs (the hub graph generator, the
Epinion2 fixture with the Xavier-uniform tables of default_rng(2020), the triple draws), the fp64 truth and the bounds are that
file's, restated here.  Every test prints the figures it asserts on."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_U, N_I = 3186, 12407
LN2 = float(np.log(2.0))
WIDTHS = (128, 256)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def random_csr(rng, n_rows, n_cols, degrees):
    rowptr = np.zeros(n_rows + 1, np.int64)
    cols = []
    for r in range(n_rows):
        k = min(int(degrees[r]), n_cols)
        cols.append(np.sort(rng.choice(n_cols, k, replace=False)))
        rowptr[r + 1] = rowptr[r] + k
    col = np.concatenate(cols).astype(np.int32)
    val = rng.normal(size=len(col)).astype(np.float32)
    return rowptr.astype(np.int32), col, val


_cache = {}


def hub_graph():
    """A non-symmetric square matrix, 3 000 rows (1 000 user rows), with rows of 0, 1, 64, 65, 1 100, 1 500 and 2 600 entries (the
    generator of tests/test_gpu_wide_step.py and tests/test_gpu_bpr_exact_step.py)."""
    if "hub" not in _cache:
        rng = np.random.default_rng(5)
        n, n_u = 3000, 1000
        deg = rng.integers(1, 50, n)
        deg[[2, 1500, 2999]] = [1500, 2600, 1100]
        deg[[7, 8, 9, 10]] = [0, 1, 64, 65]
        deg[[1200, 1201, 1202, 1203]] = [1, 0, 65, 64]
        rowptr, col, val = random_csr(rng, n, n, deg)
        _cache["hub"] = ((rowptr, col, val * np.float32(0.05)), n_u)
    return _cache["hub"]


def epi(epinion2, d):
    """(csr, E0) of Epinion2 at width d: the LightGCN adjacency, E0 ~ U(-b, b) from default_rng(2020)."""
    if "csr" not in _cache:
        from spex_amd.graph import lightgcn_norm_adj
        tr = epinion2["train"]
        _cache["csr"] = lightgcn_norm_adj(tr[:, 0], tr[:, 1], N_U - 1, N_I)
    if ("E0", d) not in _cache:
        from spex_amd.datasets import epinion2_tables
        _cache["E0", d] = np.concatenate(epinion2_tables(N_U, N_I, dim=d))
    return _cache["csr"], _cache["E0", d]


def triples(epinion2, n_steps, T=256, seed=5):
    """n_steps batches of T triples out of one bpr_epoch_triples draw (upstream's uniform sampling); in every batch of more than one
    triple the last triple repeats the first one's user and positive."""
    from spex_amd.trainer import bpr_epoch_triples
    key = ("triples", seed)
    if key not in _cache:
        _cache[key] = bpr_epoch_triples(epinion2["train"][:, :2], N_U, N_I, np.random.default_rng(seed))
    u, p, n = _cache[key]
    assert n_steps * T <= len(u)
    out = []
    for k in range(n_steps):
        s = slice(k * T, (k + 1) * T)
        bu, bp, bn = u[s].copy(), p[s].copy(), n[s].copy()
        if T > 1:
            bu[-1], bp[-1] = bu[0], bp[0]
        out.append((bu, bp, bn))
    return out


@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


def _handles(G, epinion2, d, transposed):
    """One pair of graph handles per (transposed) for the whole module: creating a handle costs more than a step."""
    key = ("handles", transposed)
    if key not in _cache:
        from spex_amd.graph import csr_transpose
        csr, E0 = epi(epinion2, d)
        gt = None
        if transposed:
            t_rowptr, t_col, t_val, eid = csr_transpose(*csr, len(E0))
            gt = G(t_rowptr, t_col, t_val, edge_id=eid)
        _cache[key] = (G(*csr), gt)
    return _cache[key]


def _stepper(G, epinion2, d, L=3, deterministic=False, transposed=False, weight_decay=0.0, E0=None):
    from spex_amd.trainer import LightGCNStepper
    _, E0_np = epi(epinion2, d)
    g, gt = _handles(G, epinion2, d, transposed)
    return LightGCNStepper(g, t(E0_np.copy()) if E0 is None else E0, N_U, n_layers=L, lr=1e-3, graph_t=gt, deterministic=deterministic,
                           weight_decay=weight_decay)


# ------------------------------------------------------------------------------------------ the fp64 truth
def truth_steps(csr, E0, n_u, L, batches, weight_decay, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """Per step (mean loss, E0, m, v) of exact BPR + L2 + Adam in fp64 on the CPU (torch autograd through torch.sparse.mm)."""
    rowptr, col, val = csr
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, col.astype(np.int64)])), torch.from_numpy(val.astype(np.float64)), (n, n)).coalesce()
    W = torch.from_numpy(E0.astype(np.float64))
    m, v = torch.zeros_like(W), torch.zeros_like(W)
    out = []
    for s, (u, p, ng) in enumerate(batches):
        u, p, ng = (torch.from_numpy(np.asarray(a, np.int64)) for a in (u, p, ng))
        T = len(u)
        Wr = W.clone().requires_grad_(True)
        cur, acc = Wr, Wr
        for _ in range(L):
            cur = torch.sparse.mm(A, cur)
            acc = acc + cur
        light = acc / (L + 1)
        lu, lp, ln = light[u], light[n_u + p], light[n_u + ng]
        z = (lu * ln).sum(1) - (lu * lp).sum(1)
        norms = Wr[u].pow(2).sum() + Wr[n_u + p].pow(2).sum() + Wr[n_u + ng].pow(2).sum()
        loss = torch.nn.functional.softplus(z).mean() + weight_decay * 0.5 * norms / T
        loss.backward()
        g = Wr.grad
        step = s + 1
        m = m + (1 - beta1) * (g - m)
        v = beta2 * v + (1 - beta2) * g * g
        denom = v.sqrt() / np.sqrt(1 - beta2 ** step) + eps
        W = W - (lr / (1 - beta1 ** step)) * (m / denom)
        out.append((float(loss.detach()), W.numpy().copy(), m.numpy().copy(), v.numpy().copy()))
    return out


def epi_truth(epinion2, d, weight_decay, L=3, T=256, n_steps=3, seed=41):
    key = ("truth", d, weight_decay, L, T, n_steps, seed)
    if key not in _cache:
        csr, E0 = epi(epinion2, d)
        _cache[key] = truth_steps(csr, E0, N_U, L, triples(epinion2, n_steps, T=T, seed=seed), weight_decay)
    return _cache[key]


# Bounds of the d == 64 test (the BCE step's: mean loss 2e-6, E0 5e-6, m 1e-5, v 2e-5).  The launch-by-launch step_bpr_exact — the code
# before the wide kernel — is the yardstick: measured against the same truth over 3 steps it gives at most
#   d = 128: loss 5.5e-8, E0 7.4e-7, m 3.3e-7, v 1.30e-5        d = 256: loss 8.4e-8, E0 9.3e-7, m 3.6e-7, v 1.29e-5
# (printed by test_one_call_bpr_step_against_the_fp64_truth), inside every bound at both widths: the bounds stay as they are.
TRUTH_BOUNDS = (2e-6, 5e-6, 1e-5, 2e-5)


def _truth_figs(st, acc, T, want):
    loss_o, W, m, v = want
    return (abs(acc.item() / T - loss_o), rel_err(st.E0.cpu().numpy(), W), rel_err(st.m.cpu().numpy(), m), rel_err(st.v.cpu().numpy(), v))


# ------------------------------------------------------------------------------------------ 1. the batch kernel's forward rows
@pytest.mark.parametrize("T", [1, 3, 17])
@pytest.mark.parametrize("d", WIDTHS)
def test_wide_bpr_batch_kernel_forward_rows_are_the_spmm_rows(G, oracle, d, T):
    """The three propagated rows of a triple, read back EXACTLY through ops.lightgcn_bpr_batch_slots_wide (see the d == 64 twin: with
    both partner rows empty and their running sums zero z = 0, sigmoid = 1/2, grad_scale 2 makes dg exactly 1, and a slot IS the
    light row, up to sign).  The master triple list is the d == 64 test's: hub rows (1 500 / 2 600 / 1 100 entries), empty rows,
    one-entry rows and the 64 / 65 boundary rows on each of the three sides, a repeated user, pos == neg, one index out of range.
    Rows of <= 1 024 entries equal spex_spmm_f32's rows at this width (layer mean fused) bit for bit; hub rows are within 3e-6 of
    the oracle; the out-of-range triple has loss 0 and all-zero slots in every column block; every other loss is log 2 to 2e-6."""
    from spex_amd import ops
    csr, n_u = hub_graph()
    n = len(csr[0]) - 1
    deg = np.diff(csr[0])
    EU, EI = 7, 1201 - n_u                                   # the empty user row, the empty item row
    assert deg[EU] == 0 and deg[n_u + EI] == 0
    it = lambda r: r - n_u
    master = [
        (2, EI, EI, 0), (EU, it(1202), EI, 1), (EU, EI, it(2999), 2),
        (9, EI, EI, 0), (10, EI, EI, 0), (8, EI, EI, 0),
        (EU, it(1500), EI, 1), (EU, it(1203), EI, 1), (EU, EI, it(1202), 2), (EU, EI, it(1203), 2),
        (EU, EI, EI, 0),
        (EU, it(1200), it(1200), None),
        (2, EI, EI, 0),
        (EU, it(2999), EI, 1),
        (2, 999999, EI, None),
        (EU, EI, it(1500), 2), (EU, it(1200), EI, 1),
    ]
    tr = master[:T]
    u, p, ng = (np.array([x[k] for x in tr], np.int64) for k in range(3))
    rng = np.random.default_rng(100 + T)
    E0 = (np.random.default_rng(64).normal(size=(n, d)) * 0.3).astype(np.float32)
    run = (rng.normal(size=(n, d)) * 0.05).astype(np.float32)
    run[EU] = 0.0
    run[n_u + EI] = 0.0
    g = G(*csr)
    X, run_d = t(E0), t(run)
    div = 4.0
    slots = torch.full((3 * T, d), 7.0, device=DEV)
    per = torch.full((T,), 7.0, device=DEV)
    ops.lightgcn_bpr_batch_slots_wide(g, X, run_d, div, t(u), t(p), t(ng), n_u, 2.0, slots, loss_per_sample=per)
    sl = slots.cpu().numpy().reshape(3, T, d)
    full_acc = torch.empty_like(X)
    g.spmm(X, Y=torch.empty_like(X), acc_in=run_d, acc_out=full_acc, acc_div=div)
    want_all = full_acc.cpu().numpy()
    got, rows = [], []
    for k, (a, b, c, side) in enumerate(tr):
        if side == 0:
            got.append(sl[2, k]); rows.append(a)                  # g_n = light_u
            assert np.array_equal(sl[1, k], -sl[2, k]) and not sl[0, k].any()
        elif side == 1:
            got.append(-sl[0, k]); rows.append(n_u + b)           # g_u = -light_p
        elif side == 2:
            got.append(sl[0, k]); rows.append(n_u + c)            # g_u = light_n
    got, rows = np.stack(got), np.array(rows)
    short = deg[rows] <= 1024
    n_hub = {1: 1, 3: 2, 17: 6}[T]
    print(f"d={d} T={T}: {len(rows)} rows read back, {int(short.sum())} of <= 1024 entries, {int((~short).sum())} hub rows")
    assert len(rows) == {1: 1, 3: 3, 17: 15}[T] and int((~short).sum()) == n_hub and int(short.sum()) == len(rows) - n_hub
    assert np.array_equal(got[short], want_all[rows][short])
    truth = (run + oracle.spmm(*csr, E0)) / np.float32(div)
    for r, row in zip(rows[~short], got[~short]):
        e = rel_err(row, truth[r])
        print(f"hub row {r} ({deg[r]} entries) d={d} T={T}: rel err vs oracle {e:.2e}")
        assert e <= 3e-6
    loss = per.cpu().numpy()
    for k, (a, b, c, side) in enumerate(tr):
        if a == 2 and b == 999999:                                 # the out-of-range triple: zero slots in all V blocks, loss 0
            assert loss[k] == 0.0 and not sl[:, k].any()
        else:
            assert abs(loss[k] - LN2) <= 2e-6
            if side is None:
                assert not sl[:, k].any()


# ------------------------------------------------------------------------------------------ 2. one launch = three launches
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_wide_bpr_batch_kernel_equals_the_three_launch_sequence(G, d, masked):
    """ops.lightgcn_bpr_batch_wide on the hub graph (unmasked, and with an injected keep mask, mode 1, keep_prob 0.6, on the handle and
    on its transposed handle): the push form with g_out, the push form without, and the dense-only form against whole-graph product ->
    ops.bpr_loss_grad -> pull-form product on the transpose.  T = 1, 3, 17, and every triple with pos == neg.  Bounds of the d == 64
    test: loss 1e-5, g_out 3e-6, G 1e-5."""
    from spex_amd import ops
    from spex_amd.graph import csr_transpose
    csr, n_u = hub_graph()
    n, L, keep_prob = len(csr[0]) - 1, 3, 0.6
    rng = np.random.default_rng(31 + masked)
    g = G(*csr)
    t_rowptr, t_col, t_val, eid = csr_transpose(*csr, n)
    gt = G(t_rowptr, t_col, t_val, edge_id=eid)
    if masked:
        keep = t((rng.random(len(csr[1])) < keep_prob).astype(np.uint8))
        g.set_edge_mask(1, keep, keep_prob, 0)
        gt.set_edge_mask(1, keep, keep_prob, 0)
    X = t((rng.normal(size=(n, d)) * 0.3).astype(np.float32))
    run = t((rng.normal(size=(n, d)) * 0.3).astype(np.float32))
    lo = torch.empty_like(X)
    g.spmm(X, Y=torch.empty_like(X), acc_in=run, acc_out=lo, acc_div=float(L + 1))
    it = lambda r: r - n_u
    z = lambda: torch.zeros(n, d, device=DEV)
    for T in (1, 3, 17):
        users = np.array(([2, 7, 2, 8, 9, 10] + list(rng.integers(0, n_u, 32)))[:T], np.int64)
        pos = np.array(([it(1500), it(2999), it(1201), it(1200), it(1202), it(1203)] + list(rng.integers(0, n - n_u, 32)))[:T], np.int64)
        neg = np.array(([it(2999), it(1203), it(1500), it(1202), it(1200), it(1201)] + list(rng.integers(0, n - n_u, 32)))[:T], np.int64)
        if T == 17:
            neg[10] = pos[10]
        for same in (False, True):
            ng = pos if same else neg
            u_d, p_d, n_d = t(users), t(pos), t(ng)
            g_out_a = z()
            loss_a = ops.bpr_loss_grad(lo[:n_u], lo[n_u:], u_d, p_d, n_d, g_out_a[:n_u], g_out_a[n_u:], 1.0 / T)
            G_a = (g_out_a + gt.spmm(g_out_a)) / (L + 1)
            loss_b, g_out_b, G_b = torch.zeros(1, device=DEV), z(), z()
            ops.lightgcn_bpr_batch_wide(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, 1.0 / (L + 1), loss_b, g_out_b, G_b)
            G_c = z()                                                 # no dense g_out wanted: the same push target
            per = torch.zeros(T, device=DEV)
            ops.lightgcn_bpr_batch_wide(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, 1.0 / (L + 1), None, None, G_c, loss_per_sample=per)
            g_out_d, loss_d = z(), torch.zeros(1, device=DEV)         # no push: the dense rows alone
            ops.lightgcn_bpr_batch_wide(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, 0.0, loss_d, g_out_d, None)
            la, lb = loss_a.item(), loss_b.item()
            assert abs(loss_d.item() - lb) <= 1e-5 * abs(lb)
            if same:
                scale = (0.5 / T) * float(lo.abs().max())
                e_g = float(g_out_b.abs().max()) / scale
                e_G = float(G_b.abs().max()) / (scale / (L + 1))
                print(f"d={d} masked={masked} T={T} pos==neg: loss {lb:.7f} (T log 2 = {T * LN2:.7f}) g_out residue {e_g:.2e} G residue {e_G:.2e}")
                assert abs(lb - T * LN2) <= 1e-6 * T * LN2
                assert e_g <= 3e-6 and e_G <= 1e-5
                assert float(g_out_a.abs().max()) / scale <= 3e-6
                continue
            figs = (abs(la - lb) / abs(la), rel_err(g_out_b.cpu().numpy(), g_out_a.cpu().numpy()), rel_err(G_b.cpu().numpy(), G_a.cpu().numpy()),
                    rel_err(G_c.cpu().numpy(), G_a.cpu().numpy()), abs(per.sum().item() - la) / abs(la))
            print(f"d={d} masked={masked} T={T}: loss {figs[0]:.2e} g_out {figs[1]:.2e} G {figs[2]:.2e} G (no g_out) {figs[3]:.2e} per-triple loss {figs[4]:.2e}")
            assert figs[0] <= 1e-5 and figs[4] <= 1e-5 and figs[1] <= 3e-6 and figs[2] <= 1e-5 and figs[3] <= 1e-5
            assert rel_err(g_out_d.cpu().numpy(), g_out_a.cpu().numpy()) <= 3e-6
    g.set_edge_mask(0)
    gt.set_edge_mask(0)


# ------------------------------------------------------------------------------------------ 3. the one-call step vs the fp64 truth
@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_one_call_bpr_step_against_the_fp64_truth(G, epinion2, d, weight_decay, deterministic):
    """Three consecutive one-call steps on Epinion2, L = 3, T = 256, against the fp64 truth: per step the mean loss, E0, m and v within
    TRUTH_BOUNDS = (2e-6, 5e-6, 1e-5, 2e-5).  The launch-by-launch step_bpr_exact (a fast stepper, weight_decay 0: the code before
    the wide kernel) runs against the same truth first and its figures are printed: it is the yardstick, and it lies inside every
    bound at both widths (figures at TRUTH_BOUNDS above), so no bound is widened.  The stepper must take the one-call form."""
    T = 256
    batches = triples(epinion2, 3, T=T, seed=41)
    acc = torch.zeros(1, device=DEV)
    ref = _stepper(G, epinion2, d)
    for s, ((u, p, ng), want) in enumerate(zip(batches, epi_truth(epinion2, d, 0.0))):
        loss = ref.step_bpr_exact(t(u), t(p), t(ng))
        acc.fill_(loss.item() * T)
        figs = _truth_figs(ref, acc, T, want)
        print(f"d={d} launch-by-launch wd=0 step {s + 1}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    st = _stepper(G, epinion2, d, deterministic=deterministic, weight_decay=weight_decay)
    assert st._one_call_bpr_ok(*(t(a) for a in batches[0]))
    worst = np.zeros(4)
    for s, ((u, p, ng), want) in enumerate(zip(batches, epi_truth(epinion2, d, weight_decay))):
        acc.zero_()
        assert st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True) is None
        figs = _truth_figs(st, acc, T, want)
        worst = np.maximum(worst, figs)
        print(f"d={d} one-call wd={weight_decay} det={deterministic} step {s + 1}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert st.t == 3
    assert all(w <= b for w, b in zip(worst, TRUTH_BOUNDS)), (worst, TRUTH_BOUNDS)


# ------------------------------------------------------------------------------------------ 4. both forced forms, T = 256 and 2 048
@pytest.mark.parametrize("d", WIDTHS)
def test_both_forms_of_the_fast_path_against_the_truth_and_each_other(G, epinion2, d):
    """stepper.bpr_backward = "push" / "dense" at T = 256, weight_decay 1e-4, three steps against the fp64 truth (TRUTH_BOUNDS); both
    leave g_out and the push target all-zero.  Then one batch of T = 2 048 — across the step's per-width threshold — through the
    step's own choice and both forced forms against the launch-by-launch step: loss, E0, m within 2e-5, v within 4e-5 (the d == 64
    test's bounds)."""
    T = 256
    for form in ("push", "dense"):
        st = _stepper(G, epinion2, d, weight_decay=1e-4)
        st.bpr_backward = form
        acc = torch.zeros(1, device=DEV)
        assert st._one_call_bpr_ok(*(t(a) for a in triples(epinion2, 1, T=T, seed=41)[0]))
        for s, ((u, p, ng), want) in enumerate(zip(triples(epinion2, 3, T=T, seed=41), epi_truth(epinion2, d, 1e-4))):
            acc.zero_()
            st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True)
            figs = _truth_figs(st, acc, T, want)
            print(f"d={d} {form} step {s + 1}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
            assert all(f <= b for f, b in zip(figs, TRUTH_BOUNDS)), (form, s, figs)
        assert not st.g_out.any() and not st.ws_bwd[0].any()
    batch = triples(epinion2, 1, T=2048, seed=19)[0]
    runs = {}
    for form in ("launch by launch", None, "push", "dense"):
        s2 = _stepper(G, epinion2, d, weight_decay=1e-4)
        s2.bpr_backward = None if form == "launch by launch" else form
        a2 = torch.zeros(1, device=DEV)
        assert s2._one_call_bpr_ok(*(t(a) for a in batch))
        s2.step_bpr_exact(*(t(a) for a in batch), loss_acc=a2, batch_rows_only=form != "launch by launch")
        runs[form] = (a2.item(), s2.E0.cpu().numpy(), s2.m.cpu().numpy(), s2.v.cpu().numpy())
    b = runs["launch by launch"]
    for form in (None, "push", "dense"):
        a = runs[form]
        figs = (abs(a[0] - b[0]) / abs(b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2]), rel_err(a[3], b[3]))
        print(f"d={d} T=2048 form={form}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
        assert figs[0] <= 2e-5 and figs[1] <= 2e-5 and figs[2] <= 2e-5 and figs[3] <= 4e-5


# ------------------------------------------------------------------------------------------ 5. other depths
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_one_call_bpr_step_at_other_depths(G, epinion2, d, deterministic):
    """One step each at L = 1, 2, 4 with T = 17 (weight_decay 1e-4) against the fp64 truth: the other schedules of the step."""
    csr, E0 = epi(epinion2, d)
    acc = torch.zeros(1, device=DEV)
    for L in (1, 2, 4):
        batch = triples(epinion2, 1, T=17, seed=60 + L)
        if ("depth", d, L) not in _cache:                          # (shared by the fast and the deterministic case)
            _cache["depth", d, L] = truth_steps(csr, E0, N_U, L, batch, 1e-4)[0]
        want = _cache["depth", d, L]
        st = _stepper(G, epinion2, d, L=L, deterministic=deterministic, weight_decay=1e-4)
        assert st._one_call_bpr_ok(*(t(a) for a in batch[0]))
        acc.zero_()
        st.step_bpr_exact(*(t(a) for a in batch[0]), loss_acc=acc, batch_rows_only=True)
        figs = _truth_figs(st, acc, 17, want)
        print(f"d={d} L={L} det={deterministic}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
        assert all(f <= b for f, b in zip(figs, TRUTH_BOUNDS)), (L, figs)
        assert st.t == 1


# ------------------------------------------------------------------------------------------ 6. deterministic mode repeats
@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_deterministic_one_call_steps_repeat_bit_for_bit(G, epinion2, d, dropout):
    """Two fresh deterministic steppers, five one-call steps each (weight_decay 1e-4; T = 256 four times, then T = 3), without and with
    a fresh in-kernel sampled edge mask per step (keep_prob 0.3): E0, m, v and the loss accumulator are BIT-IDENTICAL."""
    from spex_amd.trainer import edge_dropout_mask
    batches = triples(epinion2, 4, seed=7) + triples(epinion2, 1, T=3, seed=8)
    runs = []
    for _ in range(2):
        st = _stepper(G, epinion2, d, deterministic=True, transposed=dropout, weight_decay=1e-4)
        acc = torch.zeros(1, device=DEV)
        assert st._one_call_bpr_ok(*(t(a) for a in batches[0]))
        for k, (u, p, ng) in enumerate(batches):
            if dropout:
                st.set_edge_dropout(edge_dropout_mask(st.graph, 0.3, "philox", 5, k + 1))
            st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True)
        if dropout:
            st.set_edge_dropout(None)
        assert st.t == 5
        runs.append((st.E0.clone(), st.m.clone(), st.v.clone(), acc.item()))
    a, b = runs
    same = [torch.equal(x, y) for x, y in zip(a[:3], b[:3])] + [a[3] == b[3]]
    print(f"d={d} dropout={dropout}: E0 / m / v / loss identical: {same}; loss sum {a[3]:.6f}")
    assert all(same)
    _, E0 = epi(epinion2, d)
    assert np.abs(a[0].cpu().numpy() - E0).max() > 1e-4


# ------------------------------------------------------------------------------------------ 7. the L2 term alone
@pytest.mark.parametrize("d", WIDTHS)
def test_l2_term_reaches_the_gradient_on_the_batch_rows_only_and_leaves_no_residue(G, epinion2, d):
    """The d == 64 test at rows of 128 / 256 (what a wrong row shift in the Adam pass's L2 form breaks): two deterministic steppers,
    weight_decay 0 against 1e-2.  grad_E0 is bit-identical off the batch's rows; on them it differs by weight_decay / T * count[row]
    * E0[row] within 1e-6 of that term's maximum.  The next step with weight_decay 0 and the one after with the term back on equal
    a fresh stepper's grad_E0 bit for bit (no residue of the counts), and both count tables are all-zero two steps later with the
    term off."""
    _, E0 = epi(epinion2, d)
    (u, p, ng), (u2, p2, n2), (u3, p3, n3), (u4, p4, n4), (u5, p5, n5) = triples(epinion2, 5, seed=77)
    T, wd = 256, 1e-2
    acc = torch.zeros(1, device=DEV)
    a = _stepper(G, epinion2, d, deterministic=True, weight_decay=0.0)
    b = _stepper(G, epinion2, d, deterministic=True, weight_decay=wd)
    assert b._one_call_bpr_ok(t(u), t(p), t(ng))
    a.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True)
    b.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True)
    ga, gb = a.grad_E0.cpu().numpy(), b.grad_E0.cpu().numpy()
    rows = np.concatenate([u, N_U + p, N_U + ng])
    count = np.bincount(rows, minlength=len(E0))
    assert count.max() >= 2
    assert np.array_equal(ga[count == 0], gb[count == 0])
    term = (wd / T) * count[:, None].astype(np.float64) * E0.astype(np.float64)
    e = np.abs((gb.astype(np.float64) - ga.astype(np.float64)) - term).max() / np.abs(term).max()
    print(f"d={d} L2 term: max {np.abs(term).max():.3e}, max |g| on the batch's rows {np.abs(ga[count > 0]).max():.3e}, error {e:.2e} of the term's maximum")
    assert e <= 1e-6
    assert b.row_counts.cpu().numpy().sum() == 3 * T               # the step's own table holds the counts, the other one is clear
    for k, (wd_k, (uu, pp, nn)) in enumerate(((0.0, (u2, p2, n2)), (wd, (u3, p3, n3)))):
        fresh = _stepper(G, epinion2, d, deterministic=True, weight_decay=wd_k, E0=b.E0.clone())
        b.weight_decay = wd_k
        b.step_bpr_exact(t(uu), t(pp), t(nn), loss_acc=acc, batch_rows_only=True)
        fresh.step_bpr_exact(t(uu), t(pp), t(nn), loss_acc=acc, batch_rows_only=True)
        same = torch.equal(b.grad_E0, fresh.grad_E0)
        print(f"d={d} step {k + 2} (weight_decay {wd_k}): grad_E0 equals a fresh stepper's: {same}")
        assert same
    b.weight_decay = 0.0                                           # two steps that count nothing: each clears the other parity's table
    b.step_bpr_exact(t(u4), t(p4), t(n4), loss_acc=acc, batch_rows_only=True)
    b.step_bpr_exact(t(u5), t(p5), t(n5), loss_acc=acc, batch_rows_only=True)
    assert not b.row_counts.any()


# ------------------------------------------------------------------------------------------ 8. edge dropout
@pytest.mark.parametrize("mode", ["philox", "injected"])
@pytest.mark.parametrize("d", WIDTHS)
def test_one_call_bpr_step_under_edge_dropout_equals_the_launch_by_launch_step(G, epinion2, d, mode):
    """Four steps with a fresh edge-dropout mask per step on both handles (the in-kernel sampled mask, and an injected keep mask),
    keep_prob 0.3, through the one-call step (push form and dense form) and the launch-by-launch step: per-step losses and the table
    within 2e-5 (the d == 64 test's bound).  The table did move."""
    from spex_amd.trainer import edge_dropout_mask
    batches = triples(epinion2, 4, seed=13)
    rng = np.random.default_rng(17)
    csr, E0 = epi(epinion2, d)
    masks = [t((rng.random(len(csr[1])) < 0.3).astype(np.uint8)) for _ in batches]
    out = []
    for one_call, form in ((False, None), (True, "push"), (True, "dense")):
        st = _stepper(G, epinion2, d, transposed=True, weight_decay=1e-4)
        st.bpr_backward = form
        acc = torch.zeros(1, device=DEV)
        per_step = []
        for k, (u, p, ng) in enumerate(batches):
            st.set_edge_dropout(edge_dropout_mask(st.graph, 0.3, "philox", 5, k + 1) if mode == "philox" else (1, masks[k], 0.3, 0))
            assert st._one_call_bpr_ok(t(u), t(p), t(ng))
            before = acc.item()
            st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=one_call)
            per_step.append(acc.item() - before)
        st.set_edge_dropout(None)
        out.append((np.asarray(per_step), st.E0.cpu().numpy()))
    l_b, E_b = out[0]
    for (l_a, E_a), form in zip(out[1:], ("push", "dense")):
        print(f"d={d} {mode} {form} form: loss {np.abs(l_a - l_b).max() / np.abs(l_b).max():.2e} E0 {rel_err(E_a, E_b):.2e}")
        assert np.abs(l_a - l_b).max() <= 2e-5 * np.abs(l_b).max()
        assert rel_err(E_a, E_b) <= 2e-5
        assert np.abs(E_a - E0).max() > 1e-4


# ------------------------------------------------------------------------------------------ 9. the native epochs
def _state_figs(total, want, a, b):
    return (abs(total - want) / abs(want), rel_err(a.E0.cpu().numpy(), b.E0.cpu().numpy()), rel_err(a.m.cpu().numpy(), b.m.cpu().numpy()),
            rel_err(a.v.cpu().numpy(), b.v.cpu().numpy()))


def _assert_states(name, figs, a, b, deterministic):
    print(f"{name}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert figs[0] <= 2e-6 and figs[1] <= 2e-5 and figs[2] <= 2e-5 and figs[3] <= 4e-5
    if deterministic:
        assert torch.equal(a.E0, b.E0) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_native_bpr_epochs_equal_the_steps_issued_one_by_one(G, epinion2, d, deterministic):
    """At widths 128 / 256 the epoch calls take the native branch and equal the one-call steps issued one by one — loss 2e-6, table and
    m 2e-5, v 4e-5 (the d == 64 tests' bounds), torch.equal in deterministic mode:
      * train_epoch_bpr over five full batches of T = 256 plus a ragged one of 77 calls epoch_bpr once;
      * epoch_bpr_sampled(sampler, epoch) against epoch_bpr(*sampler.draw(epoch));
      * train_epochs_bpr(stepper, BprDeviceSampler, 2, max_steps=4) against two train_epoch_bpr calls on the same sampler."""
    from spex_amd.trainer import BprDeviceSampler, train_epoch_bpr, train_epochs_bpr
    T = 256
    new = lambda: _stepper(G, epinion2, d, deterministic=deterministic, weight_decay=1e-4)
    arr = tuple(np.concatenate(x)[:5 * T + 77] for x in zip(*triples(epinion2, 6, seed=23)))
    n = len(arr[0])
    st = new()
    calls = []
    inner = st.epoch_bpr
    st.epoch_bpr = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    total = train_epoch_bpr(st, arr, batch_size=T).item()
    assert calls == [1] and st.t == 6
    ref = new()
    want = 0.0
    for k in range(6):
        s, e = k * T, min((k + 1) * T, n)
        acc = torch.zeros(1, device=DEV)
        ref.step_bpr_exact(t(arr[0][s:e]), t(arr[1][s:e]), t(arr[2][s:e]), loss_acc=acc, batch_rows_only=True)
        want += acc.item() / (e - s)
    _assert_states(f"d={d} det={deterministic} epoch_bpr, 5 full batches + 77", _state_figs(total, want, st, ref), st, ref, deterministic)
    # the device sampler's epoch
    smp = BprDeviceSampler(epinion2["train"][:, :2], N_U, N_I, DEV, seed=11, n=4 * T + 50)
    a, b = new(), new()
    acc_a, acc_b = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
    a.epoch_bpr_sampled(smp, 3, T, acc_a[0], acc_a[1])
    b.epoch_bpr(*smp.draw(3), T, acc_b[0], acc_b[1])
    assert a.t == b.t == 5
    figs = _state_figs(acc_a[0].item() / T + acc_a[1].item() / 50, acc_b[0].item() / T + acc_b[1].item() / 50, a, b)
    _assert_states(f"d={d} det={deterministic} epoch_bpr_sampled", figs, a, b, deterministic)
    # the whole-run call
    c, e2 = new(), new()
    calls = []
    inner_c = c.train_bpr_sampled
    c.train_bpr_sampled = lambda *a_, **k: (calls.append(1), inner_c(*a_, **k))[1]
    totals = train_epochs_bpr(c, smp, 2, batch_size=T, max_steps=4)
    want2 = [float(train_epoch_bpr(e2, smp, batch_size=T, max_steps=4, epoch=ep)) for ep in range(2)]
    assert calls == [1] and c.t == e2.t == 8 and len(totals) == 2
    _assert_states(f"d={d} det={deterministic} train_epochs_bpr", _state_figs(sum(totals), sum(want2), c, e2), c, e2, deterministic)
    assert all(abs(x - y) <= 2e-6 * abs(y) for x, y in zip(totals, want2))


# ------------------------------------------------------------------------------------------ 10. the C ABI
def test_wide_bpr_step_and_kernel_argument_checks(G, epinion2):
    """spex_lightgcn_step_bpr_adam_f32 rejects, before any launch (t, the table and the accumulator unchanged): a 128-wide stepper's
    descriptor with SPEX_STEP_WIDE cleared (the 64-only message), and one with the flag and d = 192 (a message listing the widths).
    spex_lightgcn_bpr_batch_wide_f32 rejects d = 64 and d = 192 naming 128 and 256; ops.lightgcn_bpr_batch_wide raises on 64-wide
    tensors.  A deterministic stepper at width 128 refuses the launch-by-launch step_bpr_exact instead of handing out atomics."""
    from spex_amd import _lib, ops
    lib = _lib.load()
    d = 128
    st = _stepper(G, epinion2, d, transposed=True, weight_decay=1e-4)
    u, p, ng = (t(a) for a in triples(epinion2, 1, T=17, seed=3)[0])
    acc = torch.zeros(1, device=DEV)
    E0 = st.E0.clone()
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(desc):
        rc = lib.spex_lightgcn_step_bpr_adam_f32(ctypes.byref(desc), vp(u), vp(p), vp(ng), 17, vp(acc), None)
        msg = lib.spex_last_error().decode()
        torch.cuda.synchronize()
        assert desc.t == 0 and torch.equal(st.E0, E0) and acc.item() == 0.0 and not st.m.any()
        return rc, msg

    desc = st._prepare_desc(17, 3)
    assert desc.flags & _lib.STEP_WIDE and desc.d == 128
    desc.flags &= ~_lib.STEP_WIDE
    rc, msg = call(desc)
    assert rc < 0 and "64" in msg and "128" in msg, (rc, msg)
    desc.flags |= _lib.STEP_WIDE
    desc.d = 192
    rc, msg = call(desc)
    assert rc < 0 and "192" in msg and "128" in msg and "256" in msg, (rc, msg)
    desc.d = 64                                                      # the flag promises wide tables: 64 is not one of them
    rc, msg = call(desc)
    assert rc < 0 and "128" in msg and "256" in msg, (rc, msg)
    desc.d = 128
    for bad in (64, 192):
        rc = lib.spex_lightgcn_bpr_batch_wide_f32(st.graph._h, vp(E0), vp(E0), 4.0, vp(u), vp(p), vp(ng), 17, N_U, 1.0, 0.25, 0.0, None, None,
                                                  vp(acc), None, None, vp(st.ws_bwd), bad, None)
        msg = lib.spex_last_error().decode()
        torch.cuda.synchronize()
        assert rc < 0 and "128" in msg and "256" in msg and "64" in msg, (bad, rc, msg)
        rc = lib.spex_lightgcn_bpr_batch_slots_wide_f32(st.graph._h, vp(E0), vp(E0), 4.0, vp(u), vp(p), vp(ng), 17, N_U, 1.0, 0.0, None, None,
                                                        vp(acc), None, vp(st.ws_bwd), bad, None)
        assert rc < 0 and "128" in lib.spex_last_error().decode()
        torch.cuda.synchronize()
        assert acc.item() == 0.0 and not st.ws_bwd.any()
    z = torch.zeros(len(E0), 64, device=DEV)
    with pytest.raises(ValueError, match="128"):
        ops.lightgcn_bpr_batch_wide(st.graph, z, z, 4.0, u, p, ng, N_U, 1.0, 0.25, acc, None, z.clone())
    with pytest.raises(ValueError, match="128"):
        ops.lightgcn_bpr_batch_slots_wide(st.graph, z, z, 4.0, u, p, ng, N_U, 1.0, torch.zeros(51, 64, device=DEV), loss_sum=acc)
    # the step still runs after all that
    st.step_bpr_exact(u, p, ng, loss_acc=acc, batch_rows_only=True)
    assert st.t == 1 and acc.item() > 0.0
    det = _stepper(G, epinion2, d, deterministic=True)
    with pytest.raises(ValueError, match="atomics"):
        det.step_bpr_exact(u, p, ng)
    with pytest.raises(ValueError, match="atomics"):
        det.step_bpr_exact(u, p, ng, loss_acc=acc, batch_rows_only=False)
    assert det.t == 0
