"""LightGCNStepper as a state machine: the FORM of the step changes from step to step on one stepper, on the hub graph.

Every other module drives one form, or compares two forms from one fresh state, and runs its whole steps on Epinion2 (symmetric, no
empty row).  Here one stepper takes BCE and exact BPR steps, one call and launch by launch, push / dense / deterministic, with edge
dropout switched on and off, through the native epochs and around a step_bpr_sgd, on a non-symmetric graph of 3 000 rows (1 000 user
rows) with rows of 0, 1, 64, 65, 1 100, 1 500 and 2 600 entries — the generator and seed of test_gpu_bpr_exact_step.py::hub_graph,
restated here; graph_t is csr_transpose's handle with its edge-id permutation.  E0 = 0.1 * default_rng(7).normal((3000, d)), lr 1e-3,
weight_decay 1e-2.  Every batch names the hub user (row 2), the empty user (7), the 1 / 64 / 65-entry users (8, 9, 10), the hub items
(graph rows 1 500, 2 999), the 1 / 0 / 65 / 64-entry items (1 200 .. 1 203), a repeated (user, positive) pair and, for BPR, a triple
with pos == neg.

The truth is an fp64 restatement of the SEQUENCE on the CPU (`restate`): one Adam state and one t shared by its steps, each step
torch autograd through L torch.sparse.mm layers and the layer mean — BPR: softplus(xn - xp).mean() + weight_decay / 2 * norms / T;
BCE: binary_cross_entropy_with_logits of <light[u], light[n_u + i]>, mean; under an injected edge mask the masked, 1 / keep_prob-
scaled matrix for that step — then Adam by torch's formula; step_bpr_sgd by the closed form of oracle/spex_oracle.c (scores from the
propagated table, the update on E0).

Compared per step: the mean loss, E0, m, v, and after BPR steps grad_E0 (the step's whole gradient).  After every step, directly: g_out
all-zero; ws_bwd[0] all-zero after a one-call step; the row_counts table of the next step's parity all-zero.

BOUNDS are not taken from the kernels.  The yardstick is the same sequence restated in fp32 on the CPU (`restate(.., torch.float32)`)
against the fp64 truth; each bound is the larger of the project's bound for the quantity (test_gpu_bpr_exact_step.py: loss 2e-6,
E0 5e-6, m 1e-5, v 2e-5; grad_E0 1e-5) and 4 x the fp32 restatement's own figure at that step — 4 for the other summation order
(64-entry segments and float atomics against torch's row-sequential sums).  A stale or missing term or a wrong row is >= 1e-3.
The restatement on BPR, BCE, BPR, BCE, BCE, BPR at L = 3 (CPU, worst step; loss absolute, the rest relative to the truth's maximum):
    d = 64,  T = 17:   loss <= 8e-8, m <= 1.7e-6, v <= 9e-7, grad <= 1.3e-6, E0 6.1e-6
    d = 64,  T = 768:  loss <= 8e-8, E0 7e-7
    d = 256, T = 17:   m <= 8.1e-6, v <= 2.6e-6, grad <= 5.3e-6, E0 1.4e-5
    d = 256, T = 768:  E0 7e-7
E0 at T = 17 is large because this graph is dense at three hops: all 3 000 rows receive a gradient, many of them comparable to
Adam's eps, where g / (|g| + eps) is ill-conditioned — the fp32 restatement alone breaks the project's 5e-6 there.  That is why the
E0 bound is derived per step, and why m, v and grad_E0 carry these tests.
The kernels on an MI355X, worst step over every test of this module (the restatement's worst over the same steps in brackets):
    loss 8.2e-8 (1.2e-7), E0 1.2e-5 (3.7e-5; L = 1, d = 256, T = 17), m 8.8e-7 (2.0e-6), v 1.34e-5 (3.1e-6), grad_E0 4.5e-7 (2.3e-6);
    no figure above 0.67 of its bound (v), the others below 0.3.
v sits at 1.2e-5 .. 1.34e-5 at EVERY step of every form, under the project's 2e-5, not the derived bound: the kernels form 1 - beta2
in fp32 (1 - 0.999f = 0.99998713e-3, 1.29e-5 off), which the project's v bound was sized for; the restatement computes in the
table's type with Python doubles for the scalars.
Once by hand, with the BCE paths' clearing of row_counts taken out: sequence 2 fails at its third step with grad_E0 off by 0.16
(d = 64, T = 17) to 0.41 (d = 64, T = 768) of the truth's maximum, m by 0.10 to 0.24 — the stale L2 gradient of step 1's counts.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, N_U = 3000, 1000
LR, WD, KEEP_PROB, SGD_LR = 1e-3, 1e-2, 0.6, 0.05
# test_gpu_bpr_exact_step.py: TRUTH_BOUNDS (mean loss, E0, m, v) and the 1e-5 of the gradient tables (G, grad_E0) there
PROJECT_BOUNDS = {"loss": 2e-6, "E0": 5e-6, "m": 1e-5, "v": 2e-5, "grad": 1e-5}
QUANTITIES = ("loss", "E0", "m", "v", "grad")
DENSE_MIN = {64: 768, 128: 1024, 256: 512}        # steps.hip: kBprStepDenseMinTriples, ..128, ..256
USERS = [2, 7, 8, 9, 10]                           # 1 500, 0, 1, 64, 65 entries
ITEMS = [1500 - N_U, 2999 - N_U, 1200 - N_U, 1201 - N_U, 1202 - N_U, 1203 - N_U]      # 2 600, 1 100, 1, 0, 65, 64 entries


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------ inputs
_cache = {}


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


def hub_graph():
    """The generator and seed of tests/test_gpu_bpr_exact_step.py::hub_graph."""
    if "hub" not in _cache:
        rng = np.random.default_rng(5)
        deg = rng.integers(1, 50, N)
        deg[[2, 1500, 2999]] = [1500, 2600, 1100]
        deg[[7, 8, 9, 10]] = [0, 1, 64, 65]
        deg[[1200, 1201, 1202, 1203]] = [1, 0, 65, 64]
        rowptr, col, val = random_csr(rng, N, N, deg)
        _cache["hub"] = (rowptr, col, val * np.float32(0.05))
        got = np.diff(rowptr)
        assert list(got[[2, 7, 8, 9, 10, 1200, 1201, 1202, 1203, 1500, 2999]]) == [1500, 0, 1, 64, 65, 1, 0, 65, 64, 2600, 1100]
    return _cache["hub"]


def table(d):
    return (0.1 * np.random.default_rng(7).normal(size=(N, d))).astype(np.float32)


def bpr_batch(seed, T):
    """('bpr', (users, pos, neg)): the special rows on every side, triple 6 with pos == neg, the last triple repeating the first
    one's (user, positive)."""
    rng = np.random.default_rng(seed)
    u, p, ng = rng.integers(0, N_U, T), rng.integers(0, N - N_U, T), rng.integers(0, N - N_U, T)
    u[:5], p[:6], ng[:6] = USERS, ITEMS, ITEMS[3:] + ITEMS[:3]
    ng[6] = p[6]
    u[-1], p[-1] = u[0], p[0]
    return "bpr", (u.astype(np.int64), p.astype(np.int64), ng.astype(np.int64))


def bce_batch(seed, T):
    """('bce', (users, items, labels)): the special rows on both sides, the last sample repeating the first one's pair with the
    other label."""
    rng = np.random.default_rng(seed)
    u, i, y = rng.integers(0, N_U, T), rng.integers(0, N - N_U, T), rng.integers(0, 2, T).astype(np.float32)
    u[:5], i[:6] = USERS, ITEMS
    u[-1], i[-1], y[-1] = u[0], i[0], 1.0 - y[0]
    return "bce", (u.astype(np.int64), i.astype(np.int64), y)


def sgd_batch(seed, T):
    """('sgd', (users, pos, neg)) with no row named twice (the SGD kernel's update order then does not enter); the special rows on
    the user and the positive side."""
    rng = np.random.default_rng(seed)
    u = np.array(USERS + [x for x in rng.permutation(N_U) if x not in USERS][:T - 5], np.int64)
    rest = [x for x in rng.permutation(N - N_U) if x not in ITEMS]
    p = np.array(ITEMS + rest[:T - 6], np.int64)
    ng = np.array(rest[T - 6:2 * T - 6], np.int64)
    assert len(set(u)) == T and len(set(p) | set(ng)) == 2 * T
    return "sgd", (u, p, ng)


def keep_mask(seed):
    return (np.random.default_rng(seed).random(len(hub_graph()[1])) < KEEP_PROB).astype(np.uint8)


# ------------------------------------------------------------------------------------------ the truth, and its fp32 restatement
def restate(seq, d, L, weight_decay, dtype, lr=LR, beta1=0.9, beta2=0.999, eps=1e-8):
    """The sequence `seq` of (kind, arrays, keep mask or None) from E0 = table(d) in `dtype` on the CPU: per step a dict of the mean
    loss, E0, m, v after the step and the step's gradient (None after an SGD step, which leaves m, v and t alone)."""
    rowptr, col, val = hub_graph()
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    idx = torch.from_numpy(np.stack([rows, col.astype(np.int64)]))
    W = torch.from_numpy(table(d)).to(dtype)
    m, v = torch.zeros_like(W), torch.zeros_like(W)
    step, out = 0, []
    for kind, arrs, keep in seq:
        vals = val.astype(np.float64)
        if keep is not None:
            vals = vals * keep / KEEP_PROB
        A = torch.sparse_coo_tensor(idx, torch.from_numpy(vals).to(dtype), (N, N)).coalesce()
        a, b, c = (torch.from_numpy(np.asarray(x)) for x in arrs)
        T = len(a)
        Wr = W.clone().requires_grad_(kind != "sgd")
        cur, acc = Wr, Wr
        for _ in range(L):
            cur = torch.sparse.mm(A, cur)
            acc = acc + cur
        light = acc / (L + 1)
        if kind == "sgd":                      # oracle/spex_oracle.c: spex_oracle_bpr_sgd_f64 with reg = 0
            lu, lp, ln = light[a], light[N_U + b], light[N_U + c]
            x = (lu * (ln - lp)).sum(1)
            s = (torch.sigmoid(x) / T).unsqueeze(1)
            W = W.clone()
            W[a] -= SGD_LR * s * (ln - lp)
            W[N_U + b] -= SGD_LR * -s * lu
            W[N_U + c] -= SGD_LR * s * lu
            out.append({"loss": float(torch.nn.functional.softplus(x).mean()), "E0": W.numpy().copy(), "m": m.numpy().copy(),
                        "v": v.numpy().copy(), "grad": None})
            continue
        if kind == "bpr":
            lu, lp, ln = light[a], light[N_U + b], light[N_U + c]
            z = (lu * ln).sum(1) - (lu * lp).sum(1)
            norms = Wr[a].pow(2).sum() + Wr[N_U + b].pow(2).sum() + Wr[N_U + c].pow(2).sum()
            loss = torch.nn.functional.softplus(z).mean() + weight_decay * 0.5 * norms / T
        else:
            loss = torch.nn.functional.binary_cross_entropy_with_logits((light[a] * light[N_U + b]).sum(1), c.to(dtype))
        loss.backward()
        g = Wr.grad
        step += 1
        m = m + (1 - beta1) * (g - m)
        v = beta2 * v + (1 - beta2) * g * g
        denom = v.sqrt() / np.sqrt(1 - beta2 ** step) + eps
        W = W - (lr / (1 - beta1 ** step)) * (m / denom)
        out.append({"loss": float(loss.detach()), "E0": W.numpy().copy(), "m": m.numpy().copy(), "v": v.numpy().copy(),
                    "grad": g.numpy().copy()})
    return out


def figures(got, want):
    """(loss, E0, m, v, grad) of `got` against the truth `want`: the loss absolute, the tables relative to the truth's maximum."""
    out = {"loss": abs(got["loss"] - want["loss"])}
    for q in QUANTITIES[1:]:
        out[q] = None if got[q] is None or want[q] is None else rel_err(got[q], want[q])
    return out


_truth = {}           # key -> (fp64 truth per step, the fp32 restatement's figures per step); the last few sequences only


def truth_of(key, seq, d, L, weight_decay=WD):
    """The fp64 truth of a sequence and the fp32 restatement's figures against it, computed once per key."""
    if key not in _truth:
        while len(_truth) >= 4:
            _truth.pop(next(iter(_truth)))
        want = restate(seq, d, L, weight_decay, torch.float64)
        f32 = restate(seq, d, L, weight_decay, torch.float32)
        _truth[key] = (want, [figures(a, b) for a, b in zip(f32, want)])
    return _truth[key]


def bounds_of(fig32):
    return {q: max(PROJECT_BOUNDS[q], 4.0 * (fig32[q] or 0.0)) for q in QUANTITIES}


# ------------------------------------------------------------------------------------------ the stepper and its steps
@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


def handles(G):
    from spex_amd.graph import csr_transpose
    csr = hub_graph()
    t_rowptr, t_col, t_val, eid = csr_transpose(*csr, N)
    return G(*csr), G(t_rowptr, t_col, t_val, edge_id=eid)


def stepper(G, d, L=3, deterministic=False, weight_decay=WD):
    from spex_amd.trainer import LightGCNStepper
    g, gt = handles(G)
    return LightGCNStepper(g, t(table(d)), N_U, n_layers=L, lr=LR, graph_t=gt, deterministic=deterministic, weight_decay=weight_decay)


def take(st, el, form):
    """One step of the sequence on the stepper, in the form asked for ('one call' / 'launches'); its mean loss."""
    kind, arrs, keep = el
    st.set_edge_dropout(None if keep is None else (1, t(keep), KEEP_PROB, 0))
    a, b, c = (t(x) for x in arrs)
    T = a.numel()
    if kind == "sgd":
        st.loss_acc.zero_()
        return st.step_bpr_sgd(a, b, c, lr=SGD_LR).item() / T
    acc = torch.zeros(1, device=DEV)
    t0 = st.t
    if kind == "bpr":
        assert st._one_call_bpr_ok(a, b, c)
        assert st.step_bpr_exact(a, b, c, loss_acc=acc, batch_rows_only=form == "one call") is None
    else:
        assert st._one_call_ok(a, b, c)
        assert st.step_bce(a, b, c, loss_acc=acc, batch_rows_only=form == "one call") is None
    assert st.t == t0 + 1
    return acc.item() / T


def state(st, loss, with_grad):
    return {"loss": loss, "E0": st.E0.cpu().numpy(), "m": st.m.cpu().numpy(), "v": st.v.cpu().numpy(),
            "grad": st.grad_E0.cpu().numpy() if with_grad else None}


def check_invariants(st, one_call, label):
    """What every step leaves behind for the next one, whatever form that takes."""
    assert not st.g_out.any(), f"{label}: g_out is not all-zero"
    if one_call:
        assert not st.ws_bwd[0].any(), f"{label}: ws_bwd[0] is not all-zero after a one-call step"
    if st.row_counts is not None:
        assert not st.row_counts[(st.t + 1) & 1].any(), f"{label}: the count table of the next step's parity is not all-zero"


def check(label, got, want, fig32, bounds=None):
    """Print the kernel's figure, the restatement's figure and the bound in force per quantity, then assert."""
    figs, bounds = figures(got, want), bounds or bounds_of(fig32)
    shown = [q for q in QUANTITIES if figs[q] is not None]
    print(f"{label}: " + "  ".join(f"{q} {figs[q]:.2e} (fp32 {fig32[q] or 0.0:.2e}, bound {bounds[q]:.2e})" for q in shown))
    bad = {q: (figs[q], bounds[q]) for q in shown if not figs[q] <= bounds[q]}
    assert not bad, f"{label}: {bad}"


def run(st, seq, forms, truth, label, first=0):
    """Steps `seq` on `st` in `forms`, each compared with truth[first + k] and followed by the invariants."""
    want, f32 = truth
    for k, (el, form) in enumerate(zip(seq, forms)):
        loss = take(st, el, form)
        tag = f"{label} step {first + k + 1} ({el[0]}, {form}, T={len(el[1][0])})"
        check_invariants(st, form == "one call" and el[0] != "sgd", tag)
        check(tag, state(st, loss, el[0] == "bpr"), want[first + k], f32[first + k])


def end_state(st):
    return st.E0.clone(), st.m.clone(), st.v.clone()


# ------------------------------------------------------------------------------------------ 1. whole one-call steps on the hub graph
@pytest.mark.parametrize("d,kind,deterministic", [(d, kind, det) for d in (64, 128, 256) for kind in ("bce", "bpr") for det in (False, True)])
def test_whole_one_call_steps_on_the_hub_graph(G, d, kind, deterministic):
    """Three one-call steps at L = 3 on one stepper, then one step each at L = 1, 2 and 4 on fresh steppers, T = 17: every schedule
    of the one-call step (no whole-graph forward launch; one plain pull product; all plain; the running-sum forward) through rows of
    0 to 2 600 entries and a real transpose."""
    batch = bce_batch if kind == "bce" else bpr_batch
    seq = [batch(100 + k, 17) + (None,) for k in range(3)]
    st = stepper(G, d, deterministic=deterministic)
    run(st, seq, ["one call"] * 3, truth_of(("whole", d, kind, 3), seq, d, 3), f"d={d} det={deterministic} L=3")
    assert st.t == 3
    for L in (1, 2, 4):
        seq = [batch(110 + L, 17) + (None,)]
        st = stepper(G, d, L=L, deterministic=deterministic)
        run(st, seq, ["one call"], truth_of(("whole", d, kind, L), seq, d, L), f"d={d} det={deterministic} L={L}")


# ------------------------------------------------------------------------------------------ 2. BPR / BCE interleaving
def interleaved(T):
    return [(bpr_batch if kind == "bpr" else bce_batch)(200 + k, T) + (None,) for k, kind in enumerate(("bpr", "bce", "bpr", "bce", "bce", "bpr"))]


@pytest.mark.parametrize("d,T,bce_form,deterministic", [(d, T, form, det) for d in (64, 256) for T in (17, 768)
                                                        for form in ("one call", "launches") for det in (False, True)])
def test_bpr_and_bce_steps_interleaved_on_one_stepper(G, d, T, bce_form, deterministic):
    """BPR, BCE, BPR, BCE, BCE, BPR at weight_decay 1e-2, L = 3: the BPR steps one call, the BCE steps one call or launch by launch.
    The one-call BPR step counts the batch's rows into the table of its t's parity and clears the other one; a BCE step advances t
    past a table: the third step must not find the first one's counts (grad_E0 and m at step 3 decide), nor the sixth the third's."""
    seq = interleaved(T)
    forms = ["one call" if el[0] == "bpr" else bce_form for el in seq]
    st = stepper(G, d, deterministic=deterministic)
    run(st, seq, forms, truth_of(("interleaved", d, T), seq, d, 3), f"d={d} T={T} det={deterministic}")
    assert st.t == 6


def test_bpr_and_bce_native_epochs_interleaved_on_one_stepper(G):
    """epoch_bpr of one step, epoch_bce of one step, epoch_bpr of one step on one stepper (d = 64, T = 17): the first three steps of
    the sequence above through the native epochs."""
    d, T = 64, 17
    seq = interleaved(T)
    want, f32 = truth_of(("interleaved", d, T), seq, d, 3)
    st = stepper(G, d)
    for k, (kind, arrs, _) in enumerate(seq[:3]):
        full, ragged = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        (st.epoch_bpr if kind == "bpr" else st.epoch_bce)(*(t(x) for x in arrs), T, full, ragged)
        assert st.t == k + 1 and ragged.item() == 0.0
        tag = f"native epochs step {k + 1} ({kind})"
        check_invariants(st, True, tag)
        check(tag, state(st, full.item() / T, kind == "bpr"), want[k], f32[k])


# ------------------------------------------------------------------------------------------ 3. push / dense by the step's own choice
def alternating(d):
    thr = DENSE_MIN[d]
    return [bpr_batch(300 + k, T) + (None,) for k, T in enumerate((thr - 1, thr, thr - 1, thr, thr, thr, 77))]


def run_alternating(G, d, L, deterministic, truth=None):
    """T = threshold - 1, threshold, threshold - 1, threshold as single steps (push, dense, push, dense by the step's own choice; the
    slot buffer regrown at the second), then ONE native epoch_bpr of n = 2 threshold + 77, batch_size = threshold: two dense steps
    and a ragged push step.  Returns the stepper and the two loss sums."""
    thr, seq = DENSE_MIN[d], alternating(d)
    st = stepper(G, d, L=L, deterministic=deterministic)
    assert st.bpr_backward is None
    label = f"d={d} L={L} det={deterministic}"
    if truth is None:
        for el in seq[:4]:
            take(st, el, "one call")
            check_invariants(st, True, label)
    else:
        run(st, seq[:4], ["one call"] * 4, truth, label)
    assert st.grad_slots.shape[0] == 3 * thr
    full, ragged = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    st.epoch_bpr(*(t(np.concatenate([el[1][k] for el in seq[4:]])) for k in range(3)), thr, full, ragged)
    assert st.t == 7
    check_invariants(st, True, label + " epoch")
    return st, full, ragged


@pytest.mark.parametrize("d,L", [(64, 3), (64, 2), (128, 3), (256, 3)])
def test_push_and_dense_forms_alternate_by_the_steps_own_choice(G, d, L):
    """Nothing forced: T straddles the width's dense threshold from step to step (L = 2: the push form writes g_out too), then the
    native epoch takes two dense steps and a ragged push step in one call; against the truth of the same seven steps.  loss_full
    holds the two full batches' sums, loss_ragged the ragged batch's."""
    thr, seq = DENSE_MIN[d], alternating(d)
    truth = truth_of(("alternating", d, L), seq, d, L)
    want, f32 = truth
    st, full, ragged = run_alternating(G, d, L, False, truth)
    check(f"d={d} L={L} epoch end", state(st, ragged.item() / 77, True), want[6], f32[6])
    got, exp = full.item() / thr, want[4]["loss"] + want[5]["loss"]
    bound = bounds_of(f32[4])["loss"] + bounds_of(f32[5])["loss"]
    print(f"d={d} L={L} epoch: loss_full / T {got:.7f}, the two full steps' mean losses {exp:.7f}: {abs(got - exp):.2e} (bound {bound:.2e})")
    assert abs(got - exp) <= bound


# ------------------------------------------------------------------------------------------ 4. one call / launch by launch alternation
@pytest.mark.parametrize("kind", ["bpr", "bce"])
def test_one_call_and_launch_by_launch_steps_alternate(G, kind):
    """One call, launch by launch, one call, one call, launch by launch, one call (d = 64, T = 17, weight_decay 1e-2): the
    launch-by-launch forms use ws_bwd[0] as a workspace (_ws0_clean) and, for BPR, advance t without the count tables."""
    batch = bce_batch if kind == "bce" else bpr_batch
    seq = [batch(400 + k, 17) + (None,) for k in range(6)]
    forms = ["one call", "launches", "one call", "one call", "launches", "one call"]
    st = stepper(G, 64)
    run(st, seq, forms, truth_of(("forms", kind), seq, 64, 3), kind)
    assert st.t == 6


# ------------------------------------------------------------------------------------------ 5. edge dropout switched during a run
@pytest.mark.parametrize("d,form", [(d, form) for d in (64, 128) for form in (None, "dense")])
def test_edge_dropout_switched_from_step_to_step(G, d, form):
    """Injected keep mask (mode 1, keep_prob 0.6, another mask per step), none, mask, mask, none on one stepper: one-call BPR at T = 17,
    L = 3, in the push form (the step's choice at this T) and with the dense form forced, against the truth with the same masks.
    Afterwards both handles are unmasked: their products equal fresh handles' bit for bit."""
    seq = [bpr_batch(500 + k, 17) + (keep_mask(510 + k) if on else None,) for k, on in enumerate((True, False, True, True, False))]
    st = stepper(G, d)
    st.bpr_backward = form
    run(st, seq, ["one call"] * 5, truth_of(("dropout", d), seq, d, 3), f"d={d} form={form or 'push'}")
    assert st.t == 5 and st.graph.mask_mode == 0 and st.graph_t.mask_mode == 0
    X = t(table(d))
    g, gt = handles(G)
    assert torch.equal(st.graph.spmm(X), g.spmm(X)) and torch.equal(st.graph_t.spmm(X), gt.spmm(X))


# ------------------------------------------------------------------------------------------ 6. step_bpr_sgd between exact steps
@pytest.mark.parametrize("L", [3, 4])
def test_bpr_sgd_step_between_exact_steps(G, L):
    """Exact BPR (one call), step_bpr_sgd, exact BPR at d = 64 (L = 3: the one-call SGD step; L = 4: propagate + the SGD kernel).
    step_bpr_sgd shares light_out and ws_fwd with the exact steps and advances neither t nor Adam's moments; it runs with lr 0.05,
    so that its update (~1e-4 of the table's maximum) is far above the E0 bound: a lost SGD step would fail."""
    seq = [bpr_batch(600, 17) + (None,), sgd_batch(601, 17) + (None,), bpr_batch(602, 17) + (None,)]
    truth = truth_of(("sgd", L), seq, 64, L)
    moved = rel_err(truth[0][1]["E0"], truth[0][0]["E0"])
    print(f"L={L}: the SGD step moves the table by {moved:.2e} of its maximum")
    assert moved >= 1e-4
    st = stepper(G, 64, L=L)
    run(st, seq, ["one call"] * 3, truth, f"L={L}")
    assert st.t == 2


# ------------------------------------------------------------------------------------------ 7. deterministic mode across the mix
@pytest.mark.parametrize("d,T", [(64, 17), (256, 768)])
def test_deterministic_interleaved_sequence_is_bit_reproducible(G, d, T):
    """Sequence 2 (the BCE steps one call) twice from one state with deterministic=True: E0, m, v and every step's loss sum are
    bit-identical."""
    runs = []
    for _ in range(2):
        st = stepper(G, d, deterministic=True)
        losses = []
        for el in interleaved(T):
            losses.append(take(st, el, "one call"))
            check_invariants(st, True, f"d={d} T={T}")
        runs.append((end_state(st), losses))
    assert all(torch.equal(x, y) for x, y in zip(runs[0][0], runs[1][0])) and runs[0][1] == runs[1][1]


@pytest.mark.parametrize("d,L", [(64, 3), (128, 3)])
def test_deterministic_changing_batch_size_is_bit_reproducible(G, d, L):
    """Sequence 3 twice from one state with deterministic=True (one form at every T: the point is the changing T, the slot regrowth
    and the epoch's ragged step): E0, m, v and the loss sums are bit-identical."""
    runs = []
    for _ in range(2):
        st, full, ragged = run_alternating(G, d, L, True)
        runs.append(end_state(st) + (full, ragged))
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ------------------------------------------------------------------------------------------ 8. five layers: both ping-pongs at length
@pytest.fixture(scope="module")
def hub_handles(G):
    return handles(G)


@pytest.mark.parametrize("kind,form", [(kind, form) for kind in ("bce", "bpr") for form in ("fast", "deterministic", "frontier")])
def test_one_call_steps_at_five_layers_equal_the_launch_by_launch_steps(hub_handles, kind, form):
    """L = 5, d = 64 on the hub graph: the first depth at which the one-call step's forward visits ws_fwd[0], [1], [0], [1] and its
    pull products ws_bwd[1], [2], [1].  Three steps (T = 17; BPR: 17, 768 — the dense form, except on the frontier stepper — , 17) from
    one state through the one-call step and through the launch-by-launch step, fast, deterministic and frontier=True: the loss sum,
    E0, m and v within the bounds of test_gpu_wide_step.py::test_one_call_step_equals_the_launch_by_launch_step (loss sum, E0 and m
    2e-5 relative, v 4e-5).  Deterministic: two one-call runs are bit-identical."""
    from spex_amd.trainer import LightGCNStepper
    g, gt = hub_handles
    batch = bce_batch if kind == "bce" else bpr_batch
    seq = [batch(800 + k, T) for k, T in enumerate((17, 768, 17) if kind == "bpr" else (17, 17, 17))]
    runs = []
    for one_call in (True, True, False) if form == "deterministic" else (True, False):
        st = LightGCNStepper(g, t(table(64)), N_U, n_layers=5, lr=LR, graph_t=gt, deterministic=form == "deterministic", weight_decay=WD,
                             frontier=form == "frontier")
        acc = torch.zeros(1, device=DEV)
        for _, arrs in seq:
            a, b, c = (t(x) for x in arrs)
            assert (st._one_call_bpr_ok if kind == "bpr" else st._one_call_ok)(a, b, c)
            (st.step_bpr_exact if kind == "bpr" else st.step_bce)(a, b, c, loss_acc=acc, batch_rows_only=one_call)
        assert st.t == 3
        runs.append((st.E0.cpu().numpy(), st.m.cpu().numpy(), st.v.cpu().numpy(), acc.item()))
    one, launches = runs[0], runs[-1]
    if form == "deterministic":
        assert all(np.array_equal(x, y) for x, y in zip(one[:3], runs[1][:3])) and one[3] == runs[1][3]
    figs = (abs(one[3] - launches[3]) / abs(launches[3]), rel_err(one[0], launches[0]), rel_err(one[1], launches[1]), rel_err(one[2], launches[2]))
    print(f"L=5 {kind} {form}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert figs[0] <= 2e-5 and figs[1] <= 2e-5 and figs[2] <= 2e-5 and figs[3] <= 4e-5
