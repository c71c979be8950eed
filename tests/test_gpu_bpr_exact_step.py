"""Exact BPR training (BPR differentiated through the propagation, L2 on the batch's E0 rows, Adam — upstream LightGCN's training
semantics): the triple-shaped batch kernel, the one-call step spex_lightgcn_step_bpr_adam_f32 and the native epoch.

Inputs: the Epinion2 fixture with the Xavier-uniform tables of numpy.random.default_rng(2020) at d = 64, and one synthetic non-symmetric
graph with rows beyond 1 024 entries, empty rows, a one-entry row and rows at the 64 / 65 segment boundary.
The CPU truth is an fp64 restatement in this file: a sparse fp64 adjacency, L torch.sparse.mm layers and the layer mean, the gather at
the triples, softplus(xn - xp).mean() + weight_decay * 0.5 * norms / T, autograd, Adam in fp64 with torch's formula.

Tolerances are those of the same quantities of the BCE step (tests/test_gpu_wide_step.py); each assertion names its source.  Every
test prints the figures it asserts on."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_U, N_I = 3186, 12407
LN2 = float(np.log(2.0))


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
    generator of tests/test_gpu_wide_step.py::hub_graph)."""
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


def epi(epinion2):
    """(csr, E0) of Epinion2 at d = 64: the LightGCN adjacency, E0 ~ U(-b, b) from default_rng(2020)."""
    if "csr" not in _cache:
        from spex_amd.datasets import epinion2_tables
        from spex_amd.graph import lightgcn_norm_adj
        tr = epinion2["train"]
        _cache["csr"] = lightgcn_norm_adj(tr[:, 0], tr[:, 1], N_U - 1, N_I)
        _cache["E0"] = np.concatenate(epinion2_tables(N_U, N_I, dim=64))
    return _cache["csr"], _cache["E0"]


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


def _stepper(G, epinion2, L=3, deterministic=False, transposed=False, weight_decay=0.0, E0=None):
    from spex_amd.graph import csr_transpose
    from spex_amd.trainer import LightGCNStepper
    csr, E0_np = epi(epinion2)
    gt = None
    if transposed:
        t_rowptr, t_col, t_val, eid = csr_transpose(*csr, len(E0_np))
        gt = G(t_rowptr, t_col, t_val, edge_id=eid)
    return LightGCNStepper(G(*csr), t(E0_np.copy()) if E0 is None else E0, N_U, n_layers=L, lr=1e-3, graph_t=gt,
                           deterministic=deterministic, weight_decay=weight_decay)


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


def epi_truth(epinion2, weight_decay, L=3, T=256, n_steps=5, seed=41):
    key = ("truth", weight_decay, L, T, n_steps, seed)
    if key not in _cache:
        csr, E0 = epi(epinion2)
        _cache[key] = truth_steps(csr, E0, N_U, L, triples(epinion2, n_steps, T=T, seed=seed), weight_decay)
    return _cache[key]


# ------------------------------------------------------------------------------------------ 1. the batch kernel's forward rows
@pytest.mark.parametrize("T", [1, 3, 17])
def test_bpr_batch_kernel_forward_rows_are_the_spmm_rows(G, oracle, T):
    """The three propagated rows of a triple, read back EXACTLY through the slots form.  With both item rows empty and their running
    sums zero, xp = xn = 0, z = 0, sigmoid(0) = 1/2, and grad_scale 2 makes dg exactly 1: the negative's slot g_n = dg * light_u IS
    light_u.  With the user row empty (light_u = 0) again z = 0, and the user's slot g_u = light_n - light_p is light_n when the
    positive is the empty row and -light_p when the negative is.  Triples name the hub rows (1 500 / 2 600 / 1 100 entries), the empty
    rows, the one-entry rows and the 64 / 65 boundary rows on each of the three sides; a user repeats, one triple has pos == neg on a
    non-empty row, one has an index out of range (T = 17).  Rows of <= 1 024 entries equal spex_spmm_f32's rows bit for bit; longer
    rows are within 3e-6 of the oracle (test_gpu_wide_step.py: test_batch_kernel_forward_rows_are_the_spmm_rows)."""
    from spex_amd import ops
    csr, n_u = hub_graph()
    n = len(csr[0]) - 1
    deg = np.diff(csr[0])
    EU, EI = 7, 1201 - n_u                                   # the empty user row, the empty item row
    assert deg[EU] == 0 and deg[n_u + EI] == 0
    it = lambda r: r - n_u
    # (user, pos, neg, side whose row is read back: 0 user / 1 pos / 2 neg / None)
    master = [
        (2, EI, EI, 0), (EU, it(1202), EI, 1), (EU, EI, it(2999), 2),          # a hub user, 65 entries as positive, a hub negative
        (9, EI, EI, 0), (10, EI, EI, 0), (8, EI, EI, 0),                        # user side: 64, 65, 1 entries
        (EU, it(1500), EI, 1), (EU, it(1203), EI, 1), (EU, EI, it(1202), 2), (EU, EI, it(1203), 2),   # a hub positive; 64 / 65 / 64
        (EU, EI, EI, 0),                                                         # all three rows empty
        (EU, it(1200), it(1200), None),                                          # pos == neg on a one-entry row: every slot zero
        (2, EI, EI, 0),                                                          # the hub user again
        (EU, it(2999), EI, 1),                                                   # 1 100 entries on the positive side
        (2, 999999, EI, None),                                                   # out of range: skipped whole
        (EU, EI, it(1500), 2), (EU, it(1200), EI, 1),
    ]
    tr = master[:T]
    u, p, ng = (np.array([x[k] for x in tr], np.int64) for k in range(3))
    rng = np.random.default_rng(100 + T)
    E0 = (np.random.default_rng(64).normal(size=(n, 64)) * 0.3).astype(np.float32)
    run = (rng.normal(size=(n, 64)) * 0.05).astype(np.float32)
    run[EU] = 0.0
    run[n_u + EI] = 0.0
    g = G(*csr)
    X, run_d = t(E0), t(run)
    div = 4.0
    slots = torch.full((3 * T, 64), 7.0, device=DEV)
    per = torch.full((T,), 7.0, device=DEV)
    ops.lightgcn_bpr_batch_slots(g, X, run_d, div, t(u), t(p), t(ng), n_u, 2.0, slots, loss_per_sample=per)
    sl = slots.cpu().numpy().reshape(3, T, 64)
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
    print(f"T={T}: {len(rows)} rows read back, {int(short.sum())} of <= 1024 entries, {int((~short).sum())} hub rows")
    assert len(rows) == {1: 1, 3: 3, 17: 15}[T] and int((~short).sum()) == n_hub and int(short.sum()) == len(rows) - n_hub
    assert np.array_equal(got[short], want_all[rows][short])
    truth = (run + oracle.spmm(*csr, E0)) / np.float32(div)
    for r, row in zip(rows[~short], got[~short]):
        e = rel_err(row, truth[r])
        print(f"hub row {r} ({deg[r]} entries) T={T}: rel err vs oracle {e:.2e}")
        assert e <= 3e-6
    loss = per.cpu().numpy()
    for k, (a, b, c, side) in enumerate(tr):
        if a == 2 and b == 999999:                                 # the out-of-range triple: zero slots, loss 0
            assert loss[k] == 0.0 and not sl[:, k].any()
        else:
            assert abs(loss[k] - LN2) <= 2e-6
            if side is None:                                       # pos == neg with an empty user row: z = 0, every gradient row 0
                assert not sl[:, k].any()


# ------------------------------------------------------------------------------------------ 2. one launch = three launches
@pytest.mark.parametrize("masked", [False, True])
def test_bpr_batch_kernel_equals_the_three_launch_sequence(G, masked):
    """spex_lightgcn_bpr_batch_f32 on the hub graph (non-symmetric; unmasked, and with an injected keep mask, mode 1, keep_prob 0.6, on
    the handle and on its transposed handle) against whole-graph product -> ops.bpr_loss_grad -> pull-form product on the transpose:
    loss 1e-5, g_out 3e-6, G 1e-5 (test_gpu_wide_step.py: test_batch_kernel_under_an_injected_edge_mask_on_a_non_symmetric_matrix).
    With pos == neg for every triple the item rows' g_out contributions cancel to within the g_out bound (relative to the user-side
    scale dg * |light|) and the loss is T log 2 to 1e-6 relative."""
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
    X = t((rng.normal(size=(n, 64)) * 0.3).astype(np.float32))
    run = t((rng.normal(size=(n, 64)) * 0.3).astype(np.float32))
    lo = torch.empty_like(X)
    g.spmm(X, Y=torch.empty_like(X), acc_in=run, acc_out=lo, acc_div=float(L + 1))
    it = lambda r: r - n_u
    for T in (1, 3, 17):
        users = np.array(([2, 7, 2, 8, 9, 10] + list(rng.integers(0, n_u, 32)))[:T], np.int64)
        pos = np.array(([it(1500), it(2999), it(1201), it(1200), it(1202), it(1203)] + list(rng.integers(0, n - n_u, 32)))[:T], np.int64)
        neg = np.array(([it(2999), it(1203), it(1500), it(1202), it(1200), it(1201)] + list(rng.integers(0, n - n_u, 32)))[:T], np.int64)
        if T == 17:
            neg[10] = pos[10]
        for same in (False, True):
            ng = pos if same else neg
            u_d, p_d, n_d = t(users), t(pos), t(ng)
            g_out_a = torch.zeros(n, 64, device=DEV)
            loss_a = ops.bpr_loss_grad(lo[:n_u], lo[n_u:], u_d, p_d, n_d, g_out_a[:n_u], g_out_a[n_u:], 1.0 / T)
            G_a = (g_out_a + gt.spmm(g_out_a)) / (L + 1)
            loss_b, g_out_b, G_b = torch.zeros(1, device=DEV), torch.zeros(n, 64, device=DEV), torch.zeros(n, 64, device=DEV)
            ops.lightgcn_bpr_batch(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, 1.0 / (L + 1), loss_b, g_out_b, G_b)
            G_c = torch.zeros(n, 64, device=DEV)                      # no dense g_out wanted: the same push target
            per = torch.zeros(T, device=DEV)
            ops.lightgcn_bpr_batch(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, 1.0 / (L + 1), None, None, G_c, loss_per_sample=per)
            g_out_d, loss_d = torch.zeros(n, 64, device=DEV), torch.zeros(1, device=DEV)     # no push: the dense rows alone
            ops.lightgcn_bpr_batch(g, X, run, float(L + 1), u_d, p_d, n_d, n_u, 1.0 / T, 0.0, loss_d, g_out_d, None)
            la, lb = loss_a.item(), loss_b.item()
            assert abs(loss_d.item() - lb) <= 1e-5 * abs(lb)
            if same:
                scale = (0.5 / T) * float(lo.abs().max())               # dg * |light|: what the cancelling item-side rows are made of
                e_g = float(g_out_b.abs().max()) / scale
                e_G = float(G_b.abs().max()) / (scale / (L + 1))
                print(f"masked={masked} T={T} pos==neg: loss {lb:.7f} (T log 2 = {T * LN2:.7f}) g_out residue {e_g:.2e} G residue {e_G:.2e}")
                assert abs(lb - T * LN2) <= 1e-6 * T * LN2
                assert e_g <= 3e-6 and e_G <= 1e-5
                assert float(g_out_a.abs().max()) / scale <= 3e-6
                continue
            figs = (abs(la - lb) / abs(la), rel_err(g_out_b.cpu().numpy(), g_out_a.cpu().numpy()), rel_err(G_b.cpu().numpy(), G_a.cpu().numpy()),
                    rel_err(G_c.cpu().numpy(), G_a.cpu().numpy()), abs(per.sum().item() - la) / abs(la))
            print(f"masked={masked} T={T}: loss {figs[0]:.2e} g_out {figs[1]:.2e} G {figs[2]:.2e} G (no g_out) {figs[3]:.2e} per-triple loss {figs[4]:.2e}")
            assert figs[0] <= 1e-5 and figs[4] <= 1e-5 and figs[1] <= 3e-6 and figs[2] <= 1e-5 and figs[3] <= 1e-5
            assert rel_err(g_out_d.cpu().numpy(), g_out_a.cpu().numpy()) <= 3e-6
    g.set_edge_mask(0)
    gt.set_edge_mask(0)


# ------------------------------------------------------------------------------------------ 3. the one-call step vs the fp64 truth
# Bounds of the BCE step (test_gpu_wide_step.py: test_one_call_step_against_the_oracle): mean loss 2e-6, E0 5e-6, m 1e-5, v 2e-5.
TRUTH_BOUNDS = (2e-6, 5e-6, 1e-5, 2e-5)


def _truth_figs(st, acc, T, want):
    loss_o, W, m, v = want
    return (abs(acc.item() / T - loss_o), rel_err(st.E0.cpu().numpy(), W), rel_err(st.m.cpu().numpy(), m), rel_err(st.v.cpu().numpy(), v))


@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
@pytest.mark.parametrize("deterministic", [False, True])
def test_one_call_bpr_step_against_the_fp64_truth(G, epinion2, weight_decay, deterministic):
    """Five consecutive one-call steps (step_bpr_exact(.., loss_acc=.., batch_rows_only=True)) on Epinion2, L = 3, T = 256, triples from
    bpr_epoch_triples with a repeated user, against the fp64 truth: per step the mean loss, E0, m and v within the BCE step's bounds
    (2e-6, 5e-6, 1e-5, 2e-5).  The launch-by-launch step_bpr_exact at weight_decay 0 runs against the same truth first and its figures
    are printed: it is the yardstick for whether a bound fits this loss at all."""
    T = 256
    batches = triples(epinion2, 5, T=T, seed=41)
    acc = torch.zeros(1, device=DEV)
    ref = _stepper(G, epinion2)
    for s, ((u, p, ng), want) in enumerate(zip(batches, epi_truth(epinion2, 0.0))):
        loss = ref.step_bpr_exact(t(u), t(p), t(ng))
        acc.fill_(loss.item() * T)
        figs = _truth_figs(ref, acc, T, want)
        print(f"launch-by-launch wd=0 step {s + 1}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    st = _stepper(G, epinion2, deterministic=deterministic, weight_decay=weight_decay)
    assert st._one_call_bpr_ok(*(t(a) for a in batches[0]))
    worst = np.zeros(4)
    for s, ((u, p, ng), want) in enumerate(zip(batches, epi_truth(epinion2, weight_decay))):
        acc.zero_()
        assert st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True) is None
        figs = _truth_figs(st, acc, T, want)
        worst = np.maximum(worst, figs)
        print(f"one-call wd={weight_decay} det={deterministic} step {s + 1}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert st.t == 5
    assert all(w <= b for w, b in zip(worst, TRUTH_BOUNDS)), (worst, TRUTH_BOUNDS)


@pytest.mark.parametrize("form", ["push", "dense"])
def test_both_forms_of_the_fast_path_against_the_fp64_truth(G, epinion2, form):
    """The fast path picks its backward by T (push form below the step's threshold, dense form from it up); forced either way
    (stepper.bpr_backward) at T = 256, weight_decay 1e-4, five steps against the fp64 truth: the same bounds."""
    T = 256
    st = _stepper(G, epinion2, weight_decay=1e-4)
    st.bpr_backward = form
    acc = torch.zeros(1, device=DEV)
    for s, ((u, p, ng), want) in enumerate(zip(triples(epinion2, 5, T=T, seed=41), epi_truth(epinion2, 1e-4))):
        acc.zero_()
        st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True)
        figs = _truth_figs(st, acc, T, want)
        print(f"{form} step {s + 1}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
        assert all(f <= b for f, b in zip(figs, TRUTH_BOUNDS)), (form, s, figs)
    assert not st.g_out.any() and not st.ws_bwd[0].any()          # both forms leave what the next step accumulates into all-zero


@pytest.mark.parametrize("deterministic", [False, True])
def test_one_call_bpr_step_at_other_depths(G, epinion2, deterministic):
    """One step each at L = 1, 2, 4 with T = 17 (weight_decay 1e-4) against the fp64 truth: the other schedules of the step (no
    whole-graph forward launch; one plain pull product; the running-sum forward with the dense gradient rows).  Same bounds."""
    csr, E0 = epi(epinion2)
    acc = torch.zeros(1, device=DEV)
    for L in (1, 2, 4):
        batch = triples(epinion2, 1, T=17, seed=60 + L)
        want = truth_steps(csr, E0, N_U, L, batch, 1e-4)[0]
        st = _stepper(G, epinion2, L=L, deterministic=deterministic, weight_decay=1e-4)
        acc.zero_()
        st.step_bpr_exact(*(t(a) for a in batch[0]), loss_acc=acc, batch_rows_only=True)
        figs = _truth_figs(st, acc, 17, want)
        print(f"L={L} det={deterministic}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
        assert all(f <= b for f, b in zip(figs, TRUTH_BOUNDS)), (L, figs)
        assert st.t == 1


# ------------------------------------------------------------------------------------------ 4. one call vs launch by launch
@pytest.mark.parametrize("deterministic", [False, True])
def test_one_call_bpr_step_equals_the_launch_by_launch_step(G, epinion2, deterministic):
    """20 steps from one state through the one-call step and through the launch-by-launch step_bpr_exact, weight_decay 1e-4: T = 256
    eighteen times, then T = 3, then T = 1.  Loss sum, E0 and m within 2e-5, v within 4e-5
    (test_gpu_wide_step.py: test_one_call_step_equals_the_launch_by_launch_step).  Deterministic mode: two one-call runs end in
    BIT-IDENTICAL E0 / m / v and equal loss sums."""
    batches = triples(epinion2, 18, seed=7) + triples(epinion2, 1, T=3, seed=8) + triples(epinion2, 1, T=1, seed=9)
    runs = []
    for one_call in (True, True, False):
        st = _stepper(G, epinion2, deterministic=deterministic, weight_decay=1e-4)
        acc = torch.zeros(1, device=DEV)
        for u, p, ng in batches:
            st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=one_call)
        assert st.t == 20
        runs.append((st.E0.cpu().numpy(), st.m.cpu().numpy(), st.v.cpu().numpy(), acc.item()))
    a, a2, b = runs
    if deterministic:
        for x, y in zip(a[:3], a2[:3]):
            assert np.array_equal(x, y)
        assert a[3] == a2[3]
    figs = (abs(a[3] - b[3]) / abs(b[3]), rel_err(a[0], b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2]))
    print(f"det={deterministic}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert figs[0] <= 2e-5 and figs[1] <= 2e-5 and figs[2] <= 2e-5 and figs[3] <= 4e-5


# ------------------------------------------------------------------------------------------ 5. the L2 term alone
def test_l2_term_reaches_the_gradient_on_the_batch_rows_only_and_leaves_no_residue(G, epinion2):
    """Two deterministic steppers from one state, one step each on identical triples, weight_decay 0 against 1e-2.  grad_E0 (the step's
    whole gradient) is bit-identical off the batch's rows; on them it differs by weight_decay / T * count[row] * E0[row] within 1e-6
    relative to that term's maximum (one fp32 rounding of the sum g + term against the term: half an ulp of g, ~1e-7 of the term
    here).  A second step with weight_decay 0 on the stepper that had the term shows no residue of the counts — its grad_E0 equals a
    fresh stepper's from the same table bit for bit — and so does a third step with the term back on (the count tables alternate by
    step parity: the third step counts into the table the first one used)."""
    _, E0 = epi(epinion2)
    (u, p, ng), (u2, p2, n2), (u3, p3, n3) = triples(epinion2, 3, seed=77)
    T, wd = 256, 1e-2
    acc = torch.zeros(1, device=DEV)
    a = _stepper(G, epinion2, deterministic=True, weight_decay=0.0)
    b = _stepper(G, epinion2, deterministic=True, weight_decay=wd)
    a.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True)
    b.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=True)
    ga, gb = a.grad_E0.cpu().numpy(), b.grad_E0.cpu().numpy()
    rows = np.concatenate([u, N_U + p, N_U + ng])
    count = np.bincount(rows, minlength=len(E0))
    assert count.max() >= 2
    assert np.array_equal(ga[count == 0], gb[count == 0])
    term = (wd / T) * count[:, None].astype(np.float64) * E0.astype(np.float64)
    e = np.abs((gb.astype(np.float64) - ga.astype(np.float64)) - term).max() / np.abs(term).max()
    print(f"L2 term: max {np.abs(term).max():.3e}, max |g| on the batch's rows {np.abs(ga[count > 0]).max():.3e}, error {e:.2e} of the term's maximum")
    assert e <= 1e-6
    # no residue: the next steps on `b` against fresh steppers from b's table
    for k, (wd_k, (uu, pp, nn)) in enumerate(((0.0, (u2, p2, n2)), (wd, (u3, p3, n3)))):
        fresh = _stepper(G, epinion2, deterministic=True, weight_decay=wd_k, E0=b.E0.clone())
        b.weight_decay = wd_k
        b.step_bpr_exact(t(uu), t(pp), t(nn), loss_acc=acc, batch_rows_only=True)
        fresh.step_bpr_exact(t(uu), t(pp), t(nn), loss_acc=acc, batch_rows_only=True)
        same = torch.equal(b.grad_E0, fresh.grad_E0)
        print(f"step {k + 2} (weight_decay {wd_k}): grad_E0 equals a fresh stepper's: {same}")
        assert same


# ------------------------------------------------------------------------------------------ 6. edge dropout
@pytest.mark.parametrize("mode", ["philox", "injected"])
def test_one_call_bpr_step_under_edge_dropout_equals_the_launch_by_launch_step(G, epinion2, mode):
    """Six steps with a fresh edge-dropout mask per step on both handles (the in-kernel sampled mask, and an injected keep mask),
    keep_prob 0.3, through the one-call step (its push form and its dense form) and the launch-by-launch step: per-step losses and the table within 2e-5
    (test_gpu_wide_step.py: test_one_call_step_under_edge_dropout_equals_the_launch_by_launch_step).  The table did move."""
    from spex_amd.trainer import edge_dropout_mask
    batches = triples(epinion2, 6, seed=13)
    rng = np.random.default_rng(17)
    csr, E0 = epi(epinion2)
    masks = [t((rng.random(len(csr[1])) < 0.3).astype(np.uint8)) for _ in batches]
    out = []
    for one_call, form in ((False, None), (True, None), (True, "dense")):
        st = _stepper(G, epinion2, transposed=True, weight_decay=1e-4)
        st.bpr_backward = form
        acc = torch.zeros(1, device=DEV)
        per_step = []
        for k, (u, p, ng) in enumerate(batches):
            st.set_edge_dropout(edge_dropout_mask(st.graph, 0.3, "philox", 5, k + 1) if mode == "philox" else (1, masks[k], 0.3, 0))
            before = acc.item()
            st.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc, batch_rows_only=one_call)
            per_step.append(acc.item() - before)
        st.set_edge_dropout(None)
        out.append((np.asarray(per_step), st.E0.cpu().numpy()))
    l_b, E_b = out[0]
    for (l_a, E_a), form in zip(out[1:], ("push", "dense")):
        print(f"{mode} {form} form: loss {np.abs(l_a - l_b).max() / np.abs(l_b).max():.2e} E0 {rel_err(E_a, E_b):.2e}")
        assert np.abs(l_a - l_b).max() <= 2e-5 * np.abs(l_b).max()
        assert rel_err(E_a, E_b) <= 2e-5
        assert np.abs(E_a - E0).max() > 1e-4


# ------------------------------------------------------------------------------------------ 7. the native epoch
@pytest.mark.parametrize("deterministic", [False, True])
def test_native_bpr_epoch_equals_the_steps_issued_one_by_one(G, epinion2, deterministic):
    """train_epoch_bpr over 40 steps of T = 256, and over three full batches plus a ragged one of 77, takes the native branch
    (epoch_bpr is called once: ONE library call for the epoch) and equals the same one-call steps issued one by one: loss 2e-6, table
    2e-5, m 2e-5, v 4e-5 (test_gpu_wide_step.py: test_native_epoch_at_wide_widths); torch.equal in the deterministic mode."""
    from spex_amd.trainer import train_epoch_bpr
    T = 256
    arrays = tuple(np.concatenate(x) for x in zip(*triples(epinion2, 45, seed=23)))
    for n, max_steps, steps in ((len(arrays[0]), 40, 40), (3 * T + 77, None, 4)):
        arr = tuple(a[:n] for a in arrays)
        st = _stepper(G, epinion2, deterministic=deterministic, weight_decay=1e-4)
        calls = []
        inner = st.epoch_bpr
        st.epoch_bpr = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
        total = train_epoch_bpr(st, arr, batch_size=T, max_steps=max_steps).item()
        assert calls == [1] and st.t == steps
        ref = _stepper(G, epinion2, deterministic=deterministic, weight_decay=1e-4)
        want = 0.0
        for k in range(steps):
            s, e = k * T, min((k + 1) * T, n)
            acc = torch.zeros(1, device=DEV)
            ref.step_bpr_exact(t(arr[0][s:e]), t(arr[1][s:e]), t(arr[2][s:e]), loss_acc=acc, batch_rows_only=True)
            want += acc.item() / (e - s)
        figs = (abs(total - want) / abs(want), rel_err(st.E0.cpu().numpy(), ref.E0.cpu().numpy()), rel_err(st.m.cpu().numpy(), ref.m.cpu().numpy()),
                rel_err(st.v.cpu().numpy(), ref.v.cpu().numpy()))
        print(f"det={deterministic} steps={steps}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
        assert figs[0] <= 2e-6 and figs[1] <= 2e-5 and figs[2] <= 2e-5 and figs[3] <= 4e-5
        if deterministic:
            assert torch.equal(st.E0, ref.E0) and torch.equal(st.m, ref.m) and torch.equal(st.v, ref.v)


def test_native_bpr_epoch_under_sampled_edge_dropout(G, epinion2):
    """train_epoch_bpr(edge_dropout=(0.3, "philox", 5)): the native epoch keys a fresh sampled mask per step ((seed << 32) | (k + 1))
    and agrees with the one-call steps issued one by one under edge_dropout_mask's masks to 2e-5 (loss, table); the handles are left
    unmasked."""
    from spex_amd.trainer import edge_dropout_mask, train_epoch_bpr
    T, steps = 256, 6
    csr, E0 = epi(epinion2)
    arr = tuple(np.concatenate(x) for x in zip(*triples(epinion2, steps, seed=29)))
    st = _stepper(G, epinion2, transposed=True, weight_decay=1e-4)
    total = train_epoch_bpr(st, arr, batch_size=T, edge_dropout=(0.3, "philox", 5)).item()
    ref = _stepper(G, epinion2, transposed=True, weight_decay=1e-4)
    want = 0.0
    for k in range(steps):
        acc = torch.zeros(1, device=DEV)
        ref.set_edge_dropout(edge_dropout_mask(ref.graph, 0.3, "philox", 5, k + 1))
        ref.step_bpr_exact(*(t(a[k * T:(k + 1) * T]) for a in arr), loss_acc=acc, batch_rows_only=True)
        want += acc.item() / T
    ref.set_edge_dropout(None)
    figs = (abs(total - want) / abs(want), rel_err(st.E0.cpu().numpy(), ref.E0.cpu().numpy()))
    print(f"epoch under dropout: loss {figs[0]:.2e} E0 {figs[1]:.2e}")
    assert st.t == steps and figs[0] <= 2e-5 and figs[1] <= 2e-5
    X = t(E0)
    plain = _stepper(G, epinion2, transposed=True)
    assert torch.equal(st.graph.spmm(X), plain.graph.spmm(X)) and torch.equal(st.graph_t.spmm(X), plain.graph_t.spmm(X))
    # and the masked steps differ from unmasked ones (the mask was in force)
    un = _stepper(G, epinion2, transposed=True, weight_decay=1e-4)
    train_epoch_bpr(un, arr, batch_size=T)
    assert rel_err(un.E0.cpu().numpy(), st.E0.cpu().numpy()) > 1e-4


# ------------------------------------------------------------------------------------------ 8. the C ABI
def test_bpr_step_argument_checks_and_a_batch_of_2048(G, epinion2):
    """spex_lightgcn_step_bpr_adam_f32 returns a negative status before any launch, with a message naming the cause, for d = 128 in
    the descriptor (the message names 64), slot_capacity < 3 T, and a mask on one handle only.  T = 2 048 runs: one step against the
    launch-by-launch form within 2e-5 (loss, E0, m) and 4e-5 (v), the bounds of the 20-step comparison above."""
    from spex_amd import _lib
    lib = _lib.load()
    st = _stepper(G, epinion2, transposed=True, weight_decay=1e-4)
    u, p, ng = (t(a) for a in triples(epinion2, 1, T=17, seed=3)[0])
    acc = torch.zeros(1, device=DEV)
    E0 = st.E0.clone()
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(desc):
        rc = lib.spex_lightgcn_step_bpr_adam_f32(ctypes.byref(desc), vp(u), vp(p), vp(ng), 17, vp(acc), None)
        msg = lib.spex_last_error().decode()
        torch.cuda.synchronize()
        assert desc.t == 0 and torch.equal(st.E0, E0) and acc.item() == 0.0
        return rc, msg

    desc = st._prepare_desc(17, 3)
    desc.d = 128
    rc, msg = call(desc)
    assert rc < 0 and "64" in msg and "128" in msg, (rc, msg)
    desc.d = 64
    desc.slot_capacity = 3 * 17 - 1
    rc, msg = call(desc)
    assert rc < 0 and "slot capacity" in msg, (rc, msg)
    desc.slot_capacity = st.grad_slots.shape[0]
    st.graph.set_edge_mask(2, None, 0.5, 9)
    rc, msg = call(desc)
    assert rc < 0 and "same edge-dropout mask" in msg, (rc, msg)
    st.graph.set_edge_mask(0)
    # the batch kernels' own entry points name 64 too
    with pytest.raises(ValueError, match="64"):
        from spex_amd import ops
        z = torch.zeros(len(E0), 128, device=DEV)
        ops.lightgcn_bpr_batch(st.graph, z, z, 4.0, u, p, ng, N_U, 1.0, 0.25, acc, None, z.clone())
    rc = lib.spex_lightgcn_bpr_batch_f32(st.graph._h, vp(E0), vp(E0), 4.0, vp(u), vp(p), vp(ng), 17, N_U, 1.0, 0.25, 0.0, None, None, vp(acc),
                                         None, None, vp(st.ws_bwd), 128, None)
    assert rc < 0 and "64" in lib.spex_last_error().decode()
    # T = 2 048: the step's own choice (the dense form at this size) and both forms forced — both sides of the threshold
    batch = triples(epinion2, 1, T=2048, seed=19)[0]
    runs = {}
    for form in ("launch by launch", None, "push", "dense"):
        s2 = _stepper(G, epinion2, weight_decay=1e-4)
        s2.bpr_backward = None if form == "launch by launch" else form
        a2 = torch.zeros(1, device=DEV)
        s2.step_bpr_exact(*(t(a) for a in batch), loss_acc=a2, batch_rows_only=form != "launch by launch")
        runs[form] = (a2.item(), s2.E0.cpu().numpy(), s2.m.cpu().numpy(), s2.v.cpu().numpy())
    b = runs["launch by launch"]
    for form in (None, "push", "dense"):
        a = runs[form]
        figs = (abs(a[0] - b[0]) / abs(b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2]), rel_err(a[3], b[3]))
        print(f"T=2048 form={form}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
        assert figs[0] <= 2e-5 and figs[1] <= 2e-5 and figs[2] <= 2e-5 and figs[3] <= 4e-5
