"""SPEX_STEP_FRONTIER | SPEX_STEP_BF16_GATHER: the list-driven row-list SpMM on a bf16 table, the frontier steps on
bf16 gather tables (d = 64, L = 2 or 3, BCE and exact BPR, one call and launch by launch, the epochs), and `LightGCNStepper.gather_dtype`
switched between steps on one stepper.

Graphs and helpers are those of tests/test_gpu_frontier.py (graph (b): 20 000 rows, a 1 500-entry hub, 2- to 4-segment rows, empty
rows; heavy_graph(); the tiny golden graph), of tests/test_gpu_bf16_step.py (Epinion2, its fp64 truth and the recorded YARDSTICK of
the parent's deterministic whole-graph bf16 step) and of tests/test_gpu_stepper_sequences.py (`restate`: the fp64 restatement of a
sequence), imported.

The gate of whole steps is the project's rule for "roundings placed differently plus atomics": per quantity (mean loss absolute; E0, m,
v relative to the truth's maximum) the worst figure over the steps may reach 2 x the yardstick's, the yardstick being the deterministic
launch-by-launch whole-graph bf16 stepper — code that predates this mode — against the same fp64 truth: on Epinion2 the recorded
YARDSTICK, on graph (b) computed here on the same batches.  The combined mode rounds once in the backward where that step rounds
twice, so the rule is not loosened.  Every test prints the figures it asserts on.

Figures of this file's run on an MI355X: DESIGN.md 4.24."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_stepper_sequences as seqmod
from test_gpu_bf16_step import BF16, YARDSTICK, _figs, _stepper, _truth, bits, shadow_is_current, truth_steps_bce  # noqa: F401
from test_gpu_bpr_exact_step import N_U, epi, triples
from test_gpu_frontier import (DEV, NB, NB_I, NB_U, batch_b, frontier_sets, graph_b, handle, heavy_graph, listed,
                               restating_on_graph_b, t, table_b, tiny)
from test_gpu_stepper_sequences import restate
from test_gpu_wide_step import training_batches

pytestmark = pytest.mark.gpu

SENT = 7.0                      # exactly representable in bf16
WD = 1e-4
_cache = {}


@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


# ------------------------------------------------------------------------------------------ 1. the kernel against the fp32 kernel
def check_rowlist_bf16(g, csr, X16, rows, dev_count=None, tag=""):
    """One launch over `rows` (as they stand in the list; dev_count: what the device cell says) against the fp32 kernel on the widened
    table, the cast of Y, the sentinels, and the whole-graph bf16 launch on rows of up to 1 024 entries."""
    n = len(csr[0]) - 1
    deg = np.diff(csr[0])
    rows = np.asarray(rows, np.int64)
    Xw = X16.float().contiguous()
    Y, ref = torch.full_like(Xw, SENT), torch.full_like(Xw, SENT)
    Y16 = torch.full_like(X16, SENT)
    g.spmm_rows_dev(None, listed(n, rows, dev_count), X16=X16, Y=Y, Y16=Y16)
    g.spmm_rows_dev(Xw, listed(n, rows, dev_count), Y=ref)
    taken = rows[:min(len(rows) if dev_count is None else dev_count, n)]
    taken = taken[(taken >= 0) & (taken < n)]
    idx = t(taken)
    assert torch.equal(Y[idx], ref[idx]), f"{tag}: Y differs from the fp32 kernel on the widened table"
    assert torch.equal(Y, ref), f"{tag}: Y differs from the fp32 kernel outside the list"
    assert torch.equal(bits(Y16), bits(Y.to(BF16))), f"{tag}: Y16 is not the cast of Y"
    rest = torch.ones(n, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert (Y[rest] == SENT).all() and torch.equal(bits(Y16[rest]), bits(torch.full_like(Y16[rest], SENT))), f"{tag}: an unlisted row was written"
    if len(taken):
        assert not (Y[idx] == SENT).all(), f"{tag}: nothing was written"
    whole, whole16 = torch.empty_like(Xw), torch.empty_like(X16)
    g.spmm_bf16(X16, Y=whole, Y16=whole16)
    upto = t(taken[deg[taken] <= 1024])
    assert torch.equal(Y[upto], whole[upto]) and torch.equal(bits(Y16[upto]), bits(whole16[upto])), f"{tag}: differs from spex_spmm_bf16_f32's rows"
    # separately: each output alone
    Y1, Y2 = torch.full_like(Xw, SENT), torch.full_like(X16, SENT)
    g.spmm_rows_dev(None, listed(n, rows, dev_count), X16=X16, Y=Y1)
    g.spmm_rows_dev(None, listed(n, rows, dev_count), X16=X16, Y16=Y2)
    assert torch.equal(Y1, Y) and torch.equal(bits(Y2), bits(Y16)), f"{tag}: one output alone differs"
    print(f"{tag}: {len(taken)} listed rows ({int((deg[taken] > 64).sum())} beyond 64 entries, {int((deg[taken] > 1024).sum())} beyond 1 024) bit-equal")


def test_bf16_rowlist_kernel_on_graph_b():
    csr = graph_b()
    g = handle(csr)
    X16 = t(table_b()).to(BF16)
    _, (u, i, _) = batch_b("bce", 2, 256)
    assert 0 in u
    _, f1 = frontier_sets(csr, np.concatenate([u, i + NB_U]))
    rng = np.random.default_rng(5)
    check_rowlist_bf16(g, csr, X16, rng.permutation(f1), tag="F1 of a 256-sample batch with the hub")
    head = np.array([0, 1, 2, 3, 4, 5, 10, 11, NB - 1] + list(range(100, 108)), np.int64)     # hub and multi-segment rows first
    assert len(head) == 17
    for count in (0, 1, 16, 17):
        check_rowlist_bf16(g, csr, X16, head[:count], tag=f"count {count}")
    check_rowlist_bf16(g, csr, X16, head, dev_count=5, tag="a device count below the list's length")
    check_rowlist_bf16(g, csr, X16, rng.permutation(NB), dev_count=NB + 1000, tag="a device count above max_count (every row)")
    check_rowlist_bf16(g, csr, X16, np.array([5, -1, 3, NB, 200, 0, NB + 7, 12], np.int64), tag="a list holding -1 and n_rows")
    # the running-sum epilogue in place: acc_out is acc_in
    rows = rng.permutation(f1)
    acc = t((0.3 * np.random.default_rng(3).normal(size=(NB, 64))).astype(np.float32))
    a16, a32 = acc.clone(), acc.clone()
    Y16 = torch.full_like(X16, SENT)
    g.spmm_rows_dev(None, listed(NB, rows), X16=X16, Y16=Y16, acc_in=a16, acc_out=a16, acc_div=3.0)
    Y = torch.full((NB, 64), SENT, device=DEV)
    g.spmm_rows_dev(X16.float().contiguous(), listed(NB, rows), Y=Y, acc_in=a32, acc_out=a32, acc_div=3.0)
    assert torch.equal(a16, a32) and not torch.equal(a16, acc) and torch.equal(bits(Y16), bits(Y.to(BF16)))


@pytest.mark.parametrize("layout", ["heavy rows first", "straddling passes", "shuffled"])
def test_bf16_rowlist_kernel_with_more_long_row_tasks_than_lds_slots(layout):
    csr = heavy_graph()
    g = handle(csr)
    n = 4000
    X16 = t((0.1 * np.random.default_rng(22).normal(size=(n, 64))).astype(np.float32)).to(BF16)
    heavy = np.concatenate([np.arange(200, 206), np.arange(100, 116)])
    rng = np.random.default_rng(24)
    short = rng.permutation(np.setdiff1d(np.arange(n), heavy))[:300]
    if layout == "heavy rows first":
        rows = np.concatenate([heavy, short])
    elif layout == "straddling passes":
        rows = np.concatenate([short[:7], heavy[::-1], short[7:]])
    else:
        rows = np.concatenate([rng.permutation(np.concatenate([heavy, short[:26]])), short[26:]])
    for k in range(2):                                          # (a race between the groups of a pass would not show in every launch)
        check_rowlist_bf16(g, csr, X16, rows, tag=f"heavy graph, {layout}, launch {k + 1}")


def test_bf16_rowlist_kernel_on_the_tiny_graph_and_its_refusals():
    from spex_amd import _lib
    rowptr, col, val, n_u, E0 = tiny()
    csr = (rowptr, col, val)
    g = handle(csr)
    n = len(rowptr) - 1
    X16 = t(E0).to(BF16)
    check_rowlist_bf16(g, csr, X16, np.random.default_rng(0).permutation(n), tag="tiny graph, full list")
    lst = listed(n, np.arange(n))
    X128 = torch.zeros(n, 128, device=DEV, dtype=BF16)
    with pytest.raises(_lib.SpexError, match="d == 64"):
        g.spmm_rows_dev(None, lst, X16=X128, Y=torch.zeros(n, 128, device=DEV))
    with pytest.raises(_lib.SpexError, match="no output"):
        g.spmm_rows_dev(None, lst, X16=X16)
    with pytest.raises(_lib.SpexError, match="must not alias"):
        g.spmm_rows_dev(None, lst, X16=X16, Y16=X16)
    g.set_edge_mask(1, torch.ones(len(col), dtype=torch.uint8, device=DEV), 0.6, 0)
    try:
        with pytest.raises(_lib.SpexError, match="without edge dropout"):
            g.spmm_rows_dev(None, lst, X16=X16, Y=torch.zeros(n, 64, device=DEV))
    finally:
        g.set_edge_mask(0)
    with pytest.raises(ValueError, match="either X"):
        g.spmm_rows_dev(X16.float(), lst, X16=X16, Y=torch.zeros(n, 64, device=DEV))
    with pytest.raises(ValueError, match="Y16 comes with X16"):
        g.spmm_rows_dev(X16.float(), lst, Y16=torch.zeros_like(X16))


# ------------------------------------------------------------------------------------------ steppers on graph (b)
def stepper_b(L, frontier, bf16, weight_decay=WD, deterministic=False):
    """A stepper on graph (b); frontier and bf16 together only through the setter (the constructor refuses the pair)."""
    from spex_amd.trainer import LightGCNStepper
    st = LightGCNStepper(handle(graph_b()), t(table_b().copy()), NB_U, n_layers=L, lr=seqmod.LR, weight_decay=weight_decay, frontier=frontier,
                         deterministic=deterministic)
    if bf16:
        st.gather_dtype = BF16
    return st


def step(st, kind, arrs, one_call):
    """One step, the loss sum into a fresh cell; returns the cell."""
    acc = torch.zeros(1, device=DEV)
    a, b, c = (t(x) for x in arrs)
    t0 = st.t
    fn = st.step_bce if kind == "bce" else st.step_bpr_exact
    assert fn(a, b, c, loss_acc=acc, batch_rows_only=one_call) is None
    assert st.t == t0 + 1
    return acc


def figures(st, acc, n, want):
    """(mean loss absolute; E0, m, v relative to the truth's maximum) against one step of `restate`."""
    f = seqmod.figures(seqmod.state(st, acc.item() / n, False), want)
    return np.array([f["loss"], f["E0"], f["m"], f["v"]])


def truth_b(key, seq, L, weight_decay=WD):
    """The fp64 restatement of a sequence on graph (b), and the yardstick on the same batches: the worst figures of the deterministic
    launch-by-launch whole-graph bf16 stepper (the parent's code) against it.  Once per key."""
    if key not in _cache:
        with restating_on_graph_b():
            want = restate(seq, 64, L, weight_decay, torch.float64)
        ref = stepper_b(L, False, True, weight_decay, deterministic=True)
        yard = np.zeros(4)
        for k, (kind, arrs, _) in enumerate(seq):
            figs = figures(ref, step(ref, kind, arrs, False), len(arrs[0]), want[k])
            yard = np.maximum(yard, figs)
            print(f"yardstick {key} step {k + 1}: loss {figs[0]:.3e} E0 {figs[1]:.3e} m {figs[2]:.3e} v {figs[3]:.3e}")
        print(f"yardstick {key} worst: " + " ".join(f"{x:.3e}" for x in yard))
        _cache[key] = (want, yard)
    return _cache[key]


def gate(tag, worst, yard):
    print(f"{tag} worst: " + " ".join(f"{x:.3e}" for x in worst) + "  (yardstick " + " ".join(f"{x:.3e}" for x in yard) + ")")
    assert all(w <= 2 * y for w, y in zip(worst, yard)), (tag, list(worst), list(yard))


# ------------------------------------------------------------------------------------------ 2. the forward of a step is exact
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_forward_of_the_combined_step_is_exact(kind, L):
    """From one state, with the hub outside F1: the one-call frontier-bf16 step's loss sum equals the one-call whole-graph bf16 step's
    (the parent's code; the rows of F1 are identical), and its forward tables at F1 equal the launch-by-launch frontier-bf16 forward's."""
    _, arrs = batch_b(kind, 50 + L, 256, hub=False)
    a, b, c = stepper_b(L, True, True), stepper_b(L, False, True), stepper_b(L, True, True)
    b.bpr_backward = "push"
    acc_a, acc_b = step(a, kind, arrs, True), step(b, kind, arrs, True)
    print(f"{kind} L={L}: loss sums {acc_a.item()!r} {acc_b.item()!r}")
    assert torch.isfinite(acc_a).all() and acc_a.item() > 0 and torch.equal(acc_a, acc_b)
    rows = np.concatenate([arrs[0], arrs[1] + NB_U] + ([arrs[2] + NB_U] if kind == "bpr" else []))
    _, f1 = frontier_sets(graph_b(), rows)
    assert 0 not in f1 and len(f1) < 0.5 * NB
    u = t(arrs[0])
    items = t(arrs[1]) if kind == "bce" else torch.cat([t(arrs[1]), t(arrs[2])])
    c._frontier_forward(u, items)
    assert c._front.count_f.item() == len(f1)
    f1 = t(f1.astype(np.int64))
    assert torch.equal(a.ws_fwd[L - 2][f1], c.ws_fwd[L - 2][f1]) and a.ws_fwd[L - 2][f1].abs().max() > 0
    assert torch.equal(bits(a.ws16[L - 2][f1]), bits(c.ws16[L - 2][f1]))
    assert torch.equal(bits(a.ws16[L - 2][f1]), bits(a.ws_fwd[L - 2][f1].to(BF16)))


# ------------------------------------------------------------------------------------------ 3. no read outside F1
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_nothing_outside_the_frontier_is_read(kind, L):
    """Four one-call steps, ws_fwd and ws16 all-NaN before the first and the third: a row read outside what the step itself wrote
    would reach the loss or the tables."""
    st = stepper_b(L, True, True)
    for k in range(4):
        _, arrs = batch_b(kind, 60 + 4 * L + k, 256, hub=False)
        if k in (0, 2):
            st.ws_fwd.fill_(float("nan"))
            st.ws16.fill_(float("nan"))
        acc = step(st, kind, arrs, True)
        assert torch.isfinite(acc).all() and acc.item() > 0, (kind, L, k)
        for name in ("E0", "m", "v"):
            assert torch.isfinite(getattr(st, name)).all(), (kind, L, k, name)
        assert not st.g_out.any() and not st.ws_bwd[0].any(), (kind, L, k)
        assert st._shadow_current and shadow_is_current(st), (kind, L, k)
        assert st.t == k + 1
    assert st.m.abs().max() > 0


# ------------------------------------------------------------------------------------------ 4. against the fp64 truth
def stepper_epi(G, epinion2, L):
    from spex_amd.trainer import LightGCNStepper
    csr, E0 = epi(epinion2)
    st = LightGCNStepper(G(*csr), t(E0.copy()), N_U, n_layers=L, lr=1e-3, weight_decay=WD, frontier=True)
    st.gather_dtype = BF16
    return st


@pytest.mark.parametrize("L", [3, 2])
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_combined_steps_against_the_fp64_truth_on_epinion2(G, epinion2, kind, L):
    """Five steps (BCE at B = 256; BPR at T = 256, weight_decay 1e-4), one call and launch by launch: per quantity at most twice
    YARDSTICK[(kind, L)], the recorded figure of the parent's deterministic whole-graph bf16 step.  After step 1 the deviation of m
    exceeds 1e-6 (the bf16 tables were read) and stays below 2 L 2^-8."""
    batches = training_batches(epinion2, 5, seed=41) if kind == "bce" else triples(epinion2, 5, seed=41)
    truth = _truth(epinion2, kind, L)
    for form in ("one call", "launches"):
        st = stepper_epi(G, epinion2, L)
        worst = np.zeros(4)
        for s, (b, want) in enumerate(zip(batches, truth)):
            acc = step(st, kind, b, form == "one call")
            figs = _figs(st, acc, 256, want)
            worst = np.maximum(worst, figs)
            print(f"frontier bf16 {kind} {form} L={L} step {s + 1}: loss {figs[0]:.3e} E0 {figs[1]:.3e} m {figs[2]:.3e} v {figs[3]:.3e}")
            if s == 0:
                assert 1e-6 < figs[2] < 2 * L * 2.0 ** -8, (kind, form, L, figs[2])
        assert st.t == 5 and (form != "one call" or shadow_is_current(st))
        gate(f"frontier bf16 {kind} {form} L={L} (Epinion2)", worst, YARDSTICK[(kind, L)])


@pytest.mark.parametrize("L", [3, 2])
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_combined_steps_against_the_fp64_truth_on_graph_b(kind, L):
    """Four steps on graph (b), where F1 is a few percent of the rows (Epinion2's is nearly everything) and holds the hub: a row
    outside F1 that the step needed would be missed here.  The yardstick is computed on the same batches."""
    seq = [batch_b(kind, 820 + k, 256) + (None,) for k in range(4)]
    want, yard = truth_b(("b", kind, L), seq, L)
    for form in ("one call", "launches"):
        st = stepper_b(L, True, True)
        worst = np.zeros(4)
        for k, (_, arrs, _) in enumerate(seq):
            figs = figures(st, step(st, kind, arrs, form == "one call"), 256, want[k])
            worst = np.maximum(worst, figs)
            print(f"frontier bf16 (b) {kind} {form} L={L} step {k + 1}: loss {figs[0]:.3e} E0 {figs[1]:.3e} m {figs[2]:.3e} v {figs[3]:.3e}")
            seqmod.check_invariants(st, form == "one call", f"(b) {kind} {form} L={L} step {k + 1}")
        gate(f"frontier bf16 (b) {kind} {form} L={L}", worst, yard)


# ------------------------------------------------------------------------------------------ 5. switching on one stepper
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_gather_dtype_and_frontier_switched_on_one_stepper(kind):
    """whole fp32 -> frontier fp32 -> frontier bf16 -> whole bf16 -> launch-by-launch frontier bf16 -> whole fp32 on ONE stepper at
    L = 3 (weight_decay 1e-2 for BPR: a stale count table would show), gated as in test 4 over the whole sequence: one set of moments
    and one t.  The shadow is re-cast when bf16 comes back after fp32 steps."""
    plan = [(False, None, True), (True, None, True), (True, BF16, True), (False, BF16, True), (True, BF16, False), (False, None, True)]
    seq = [batch_b(kind, 900 + k, 256) + (None,) for k in range(len(plan))]
    wd = seqmod.WD
    want, yard = truth_b(("switch", kind), seq, 3, wd)
    st = stepper_b(3, True, False, wd)
    tables = tuple(x.data_ptr() for x in (st.E0, st.m, st.v))
    worst = np.zeros(4)
    for k, ((frontier, dtype, one_call), (_, arrs, _)) in enumerate(zip(plan, seq)):
        st.frontier = frontier
        was = st.gather_dtype
        st.gather_dtype = dtype
        assert st.gather_dtype is dtype and st.frontier is frontier
        if dtype is BF16 and was is None:
            assert not st._shadow_current          # fp32 steps moved E0: the next step must re-cast
        stale = st.E0_16.clone() if st.E0_16 is not None else None
        figs = figures(st, step(st, kind, arrs, one_call), 256, want[k])
        worst = np.maximum(worst, figs)
        tag = f"switch {kind} step {k + 1} (frontier={frontier}, gather_dtype={dtype}, one_call={one_call})"
        print(f"{tag}: loss {figs[0]:.3e} E0 {figs[1]:.3e} m {figs[2]:.3e} v {figs[3]:.3e}")
        seqmod.check_invariants(st, one_call, tag)
        if dtype is BF16 and one_call:
            assert st._shadow_current and shadow_is_current(st), tag
        if dtype is BF16 and not one_call:
            assert not st._shadow_current, tag
        if dtype is None and stale is not None:
            assert torch.equal(bits(st.E0_16), bits(stale)), tag       # switched off: the buffers are kept, not written
        assert st.t == k + 1 and tables == tuple(x.data_ptr() for x in (st.E0, st.m, st.v))
    gate(f"switch {kind}", worst, yard)


# ------------------------------------------------------------------------------------------ 6. epochs
@pytest.mark.parametrize("L", [2, 3])
def test_bce_epoch_with_frontier_and_bf16(L):
    """epoch_bce over 4 x 256 + 3 samples: the state against the fp64 truth of the same five batches (not against the code under
    test), t, the loss split into loss_full / loss_ragged, the shadow.  Loss bounds: loss_full / 256 is a sum of four mean losses, each
    within twice the yardstick's figure, so within 4 x that; loss_ragged / 3 is one."""
    parts = [batch_b("bce", 700 + k, 256) for k in range(4)] + [batch_b("bce", 704, 3)]
    seq = [p + (None,) for p in parts]
    want, yard = truth_b(("epoch bce", L), seq, L)
    st = stepper_b(L, True, True)
    u, i, y = (t(np.concatenate([p[1][k] for p in parts])) for k in range(3))
    loss = torch.zeros(2, 1, device=DEV)
    st.epoch_bce(u, i, y, 256, loss[0], loss[1])
    assert st.t == 5 and st._shadow_current and shadow_is_current(st)
    full, ragged = loss[0].item() / 256, loss[1].item() / 3
    d_full, d_ragged = abs(full - sum(w["loss"] for w in want[:4])), abs(ragged - want[4]["loss"])
    figs = figures(st, loss[1], 3, want[4])
    print(f"epoch_bce L={L}: loss_full {d_full:.3e} loss_ragged {d_ragged:.3e} E0 {figs[1]:.3e} m {figs[2]:.3e} v {figs[3]:.3e}  (yardstick "
          + " ".join(f"{x:.3e}" for x in yard) + ")")
    assert ragged > 0 and d_full <= 4 * 2 * yard[0] and d_ragged <= 2 * yard[0]
    assert all(f <= 2 * b for f, b in zip(figs[1:], yard[1:])), (list(figs), list(yard))
    seqmod.check_invariants(st, True, f"epoch_bce L={L}")


@pytest.mark.parametrize("L", [2, 3])
def test_sampled_bpr_epoch_with_frontier_and_bf16(L):
    """epoch_bpr_sampled, max_steps = 4 at T = 256, through BprDeviceSampler: against the fp64 truth over the triples the sampler
    draws for that epoch."""
    from spex_amd.trainer import BprDeviceSampler
    T, steps = 256, 4
    s = BprDeviceSampler(graph_b()[3], NB_U, NB_I, torch.device(DEV, torch.cuda.current_device()), seed=6, n=steps * T + 100)
    drawn = [x.clone().cpu().numpy() for x in s.draw(2)]
    seq = [("bpr", tuple(x[k * T:(k + 1) * T] for x in drawn), None) for k in range(steps)]
    want, yard = truth_b(("epoch bpr", L), seq, L)
    st = stepper_b(L, True, True)
    loss = torch.zeros(2, 1, device=DEV)
    st.epoch_bpr_sampled(s, 2, T, loss[0], loss[1], max_steps=steps)
    assert st.t == steps and st._shadow_current and shadow_is_current(st)
    d_full = abs(loss[0].item() / T - sum(w["loss"] for w in want))
    figs = figures(st, loss[0], T, want[-1])
    print(f"epoch_bpr_sampled L={L}: loss_full {d_full:.3e} E0 {figs[1]:.3e} m {figs[2]:.3e} v {figs[3]:.3e}  (yardstick "
          + " ".join(f"{x:.3e}" for x in yard) + ")")
    assert loss[1].item() == 0.0 and d_full <= steps * 2 * yard[0]
    assert all(f <= 2 * b for f, b in zip(figs[1:], yard[1:])), (list(figs), list(yard))
    seqmod.check_invariants(st, True, f"epoch_bpr_sampled L={L}")


# ------------------------------------------------------------------------------------------ 7. refusals
def test_native_refusals_of_the_combined_mode():
    from spex_amd import _lib
    from spex_amd.graph import _stream
    lib = _lib.load()
    st = stepper_b(3, True, True)
    g = st.graph
    _, (u, i, y) = batch_b("bce", 1, 7)
    u, i, y = t(u), t(i), t(y)
    acc = torch.zeros(1, device=DEV)
    E0_before = st.E0.clone()
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    F, B16 = _lib.STEP_FRONTIER, _lib.STEP_BF16_GATHER

    def status(flags, bpr=False, L=3, d=64, no_shadow=False):
        desc = st._prepare_desc(7, 3 if bpr else 2)
        desc.flags, desc.L, desc.d = flags, L, d
        saved = desc.E0_16
        if no_shadow:
            desc.E0_16 = None
        name = "spex_lightgcn_step_bpr_adam_f32" if bpr else "spex_lightgcn_step_bce_f32"
        rc = getattr(lib, name)(ctypes.byref(desc), vp(u), vp(i), vp(i) if bpr else vp(y), 7, vp(acc), _stream(None))
        desc.E0_16, desc.L, desc.d = saved, 3, 64
        assert desc.t == 0
        return rc, lib.spex_last_error().decode()

    for bpr in (False, True):
        rc, msg = status(F | B16 | _lib.STEP_SPARSE_ADAM, bpr, L=2)
        assert rc == -1 and "SPEX_STEP_SPARSE_ADAM" in msg and "SPEX_STEP_BF16_GATHER" in msg, (rc, msg)
        rc, msg = status(F | B16 | _lib.STEP_SPARSE_ADAM, bpr)
        assert rc == -1 and "SPEX_STEP_SPARSE_ADAM" in msg, (rc, msg)
        for L, d in ((1, 64), (4, 64), (3, 128)):
            rc, msg = status(F | B16, bpr, L=L, d=d)
            assert rc == -4 and "SPEX_STEP_BF16_GATHER" in msg, (L, d, rc, msg)
        rc, msg = status(F | B16 | _lib.STEP_DETERMINISTIC, bpr)
        assert rc == -1 and "SPEX_STEP_DETERMINISTIC" in msg, (rc, msg)
        rc, msg = status(F | B16, bpr, no_shadow=True)
        assert rc == -1 and "NULL E0_16" in msg, (rc, msg)
    rc, msg = status(F | B16 | _lib.STEP_BPR_DENSE, True)
    assert rc == -1 and "SPEX_STEP_BPR_DENSE" in msg, (rc, msg)
    g.set_edge_mask(1, torch.ones(len(graph_b()[1]), dtype=torch.uint8, device=DEV), 0.6, 0)
    try:
        rc, msg = status(F | B16)
        assert rc == -1 and "edge dropout" in msg, (rc, msg)
    finally:
        g.set_edge_mask(0)
    torch.cuda.synchronize()
    assert st.t == 0 and torch.equal(st.E0, E0_before) and acc.item() == 0.0
    # the stepper still steps
    step(st, "bce", (u.cpu().numpy(), i.cpu().numpy(), y.cpu().numpy()), True)
    assert st.t == 1 and shadow_is_current(st)


def test_python_refusals_of_the_setter():
    from spex_amd.trainer import LightGCNStepper
    g = handle(graph_b())
    E0 = t(table_b().copy())
    with pytest.raises(ValueError, match="not with gather_dtype") as e:
        LightGCNStepper(g, E0, NB_U, n_layers=3, gather_dtype=BF16, frontier=True)
    assert "set `stepper.gather_dtype` after construction" in str(e.value)
    wide = LightGCNStepper(g, torch.zeros(NB, 128, device=DEV), NB_U, n_layers=3)
    with pytest.raises(ValueError, match="width of 64"):
        wide.gather_dtype = BF16
    assert wide.gather_dtype is None and wide.E0_16 is None and wide.ws16 is None
    deep = LightGCNStepper(g, E0, NB_U, n_layers=4, frontier=True)
    with pytest.raises(ValueError, match="n_layers 2 or 3"):
        deep.gather_dtype = BF16
    assert deep.gather_dtype is None and deep.E0_16 is None
    with pytest.raises(ValueError, match="gather_dtype must be"):
        deep.gather_dtype = torch.float16
    sp = LightGCNStepper(g, E0, NB_U, n_layers=2, frontier=True, sparse_adam=True)
    with pytest.raises(ValueError, match="sparse_adam"):
        sp.gather_dtype = BF16
    assert sp.gather_dtype is None and sp.E0_16 is None and sp.sparse_adam is True
    sp.sparse_adam = False
    sp.gather_dtype = BF16
    assert sp.gather_dtype is BF16 and sp.E0_16 is not None and not sp._shadow_current
    with pytest.raises(ValueError, match="gather_dtype"):
        sp.sparse_adam = True
    assert sp.sparse_adam is False and sp.gather_dtype is BF16
    sp.gather_dtype = torch.float32                 # off: the buffers stay
    assert sp.gather_dtype is None and sp.E0_16 is not None
    sp.sparse_adam = True
    assert sp.sparse_adam is True
    # a stepper built without frontier takes the setter too
    plain = LightGCNStepper(g, E0, NB_U, n_layers=3)
    plain.gather_dtype = BF16
    assert plain.gather_dtype is BF16 and plain.E0_16.shape == (NB, 64) and plain.ws16.shape == (2, NB, 64)
    assert sp.t == plain.t == 0
