"""SPEX_STEP_FRONTIER_DEEP: the third hop of the frontier list, the list-driven push for long lists, the list SpMM over
the F2 prefix, and the exact L = 3 LightGCN steps whose every launch runs over a device list — with dense Adam and with row-sparse
Adam over F3, unmasked and under edge dropout.

Graphs: `graph_b()` (20 000 rows, hub user 0 of 1 500 entries, rows of 65 .. 200 entries), `heavy_graph()` and `tiny()` of
tests/test_gpu_frontier.py; the hub graph (3 000 rows, not symmetric) of tests/test_gpu_stepper_sequences.py; the 150 000-row graph of
tests/test_gpu_large_graph.py for the one case past the push kernel's grid.  The set sizes these cases rely on are proved in
tests/test_frontier_deep_host.py and asserted again here on the device lists.

Bounds.  Lists: equal as sets and counts.  List SpMM: bit for bit.  Push: 2e-6 of the result's maximum against an fp64 scatter, the
bound of the project's push tests (tests/test_gpu_frontier_dropout.py), and the same against spex_spmm_push_rows_f32 on the same list.
Whole steps: the fp64 restatement of tests/test_gpu_stepper_sequences.py under that module's gate (`bounds_of`), unchanged.  Epochs:
tests/test_gpu_frontier.py::EPOCH_BOUNDS.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_frontier as fmod
import test_gpu_frontier_dropout as dmod
import test_gpu_stepper_sequences as seqmod
from test_frontier_deep_host import TABLE, keep_03, rows_of, sets3
from test_gpu_frontier import DEV, NB, NB_I, NB_U, batch_b, graph_b, heavy_graph, listed, t, table_b, tiny
from test_gpu_frontier_dropout import philox_keep

pytestmark = pytest.mark.gpu

SENT = 12345.0
PUSH_BOUND = 2e-6
CASES = sorted(TABLE)


@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


def device():
    return torch.device(DEV, torch.cuda.current_device())


def mask_args(mask, nnz, keep1=None):
    """(keep bits in NumPy or None, keep_prob, set_edge_mask arguments) of 'none' / 'mode 1' / 'mode 2' at 0.3."""
    if mask == "none":
        return None, 1.0, (0,)
    if mask == "mode 1":
        keep = keep_03() if keep1 is None else keep1
        return keep, 0.3, (1, t(keep), 0.3, 0)
    seed = (55 << 32) | 9
    return philox_keep(nnz, 0.3, seed), 0.3, (2, None, 0.3, seed)


def batch_ab(kind, arrs):
    """(users, items [+ negatives]) as the two index lists FrontierRows.update takes."""
    return arrs[0], (arrs[1] if kind == "bce" else np.concatenate([arrs[1], arrs[2]]))


def frontier_of(g, n, n_u, kind, arrs, hops=3):
    from spex_amd import ops
    a, b = batch_ab(kind, arrs)
    fr = ops.FrontierRows(n, device()).update(t(a), t(b), 0, n_u).expand(g)
    if hops >= 2:
        fr.expand2(g)
    if hops >= 3:
        fr.expand3(g)
    return fr


# ------------------------------------------------------------------------------------------ 1. the third hop
@pytest.mark.parametrize("mask", ["none", "mode 1", "mode 2"])
def test_third_hop_is_the_numpy_set(mask):
    from spex_amd import ops
    csr = graph_b()[:3]
    keep, _, args = mask_args(mask, len(csr[1]))
    g = fmod.handle(csr)
    g.set_edge_mask(*args)
    fr = ops.FrontierRows(NB, device())
    for rnd in range(2):                                         # the second round: new epochs on the same stamp table
        for case in CASES:
            kind, seed, n = case
            arrs = batch_b(kind, seed, n)[1]
            a, b = batch_ab(kind, arrs)
            fr.update(t(a), t(b), 0, NB_U).expand(g).expand2(g).expand3(g)
            sets = sets3(csr, rows_of(kind, arrs, NB_U), keep)
            counts = tuple(int(x) for x in fr.counts.cpu().numpy())
            assert counts == tuple(len(s) for s in sets), (mask, rnd, case)
            assert fr.count_f3.item() == counts[3]
            if mask == "none":
                assert counts == TABLE[case][0]
            elif mask == "mode 1":
                assert counts[1:] == TABLE[case][1]
            lst = fr.list.cpu().numpy()
            for k in range(4):
                assert np.array_equal(np.sort(lst[:counts[k]]), sets[k]), (mask, rnd, case, k)
            assert counts[3] < NB
    assert fr.epoch == 2 * len(CASES)
    g.set_edge_mask(0)


def test_third_hop_on_the_hub_graph_where_two_hops_cover_everything():
    csr = seqmod.hub_graph()
    g = fmod.handle(csr)
    kind, arrs = seqmod.bce_batch(30, 17)
    for _ in range(2):
        fr = frontier_of(g, seqmod.N, seqmod.N_U, kind, arrs)
        assert tuple(fr.counts.cpu().numpy()[1:]) == (2906, 3000, 3000)
        assert np.array_equal(np.sort(fr.list.cpu().numpy()), np.arange(3000))          # no duplicate


# ------------------------------------------------------------------------------------------ 2. the push-list kernel alone
def scatter64(csr, rows, src, scale, keep=None, kp=1.0):
    """scale * A_m^T scatter(src) over `rows` in fp64 (NumPy): the dense result and the sorted rows that receive anything."""
    rowptr, col, val = csr[:3]
    rows = np.asarray(rows, np.int64)
    lens = (rowptr[rows + 1] - rowptr[rows]).astype(np.int64)
    e = np.repeat(rowptr[rows].astype(np.int64) - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(lens.sum())
    r_of = np.repeat(rows, lens)
    if keep is not None:
        sel = keep[e] != 0
        e, r_of = e[sel], r_of[sel]
    out = np.zeros((len(rowptr) - 1, src.shape[1]))
    if len(e) == 0:
        return out, np.zeros(0, np.int64)
    contrib = (scale * val[e].astype(np.float64) / kp)[:, None] * src[r_of].astype(np.float64)
    order = np.argsort(col[e], kind="stable")
    cols, starts = np.unique(col[e][order], return_index=True)
    out[cols] = np.add.reduceat(contrib[order], starts, axis=0)
    return out, cols.astype(np.int64)


def check_push(tag, g, csr, rows_obj, count, rows, src, keep=None, kp=1.0, against_rows_kernel=True):
    """spmm_push_list over rows_obj[0 : count) — `rows` in NumPy — against the fp64 scatter and spmm_push_rows; a sentinel-filled
    table keeps its bits outside the reached rows."""
    from spex_amd import ops
    n = len(csr[0]) - 1
    want, touched = scatter64(csr, rows, src, 0.5, keep, kp)
    out = torch.zeros(n, 64, device=DEV)
    ops.spmm_push_list(g, rows_obj, t(src), out, scale=0.5, count=count)
    got = out.cpu().numpy()
    fig = seqmod.rel_err(got, want)
    fig2 = 0.0
    if against_rows_kernel:
        out2 = torch.zeros(n, 64, device=DEV)
        ops.spmm_push_rows(g, rows_obj, t(src), out2, True, scale=0.5, count=count)
        fig2 = seqmod.rel_err(got, out2.cpu().numpy())
    print(f"push list ({tag}) over {len(rows)} rows, {len(touched)} reached: {fig:.2e} vs fp64, {fig2:.2e} vs spmm_push_rows")
    assert fig <= PUSH_BOUND and fig2 <= PUSH_BOUND
    rest = np.ones(n, bool)
    rest[touched] = False
    assert not got[rest].any()                                  # a dropped entry issues no atomic: unreached rows are exactly zero
    filled = torch.full((n, 64), SENT, device=DEV)
    ops.spmm_push_list(g, rows_obj, t(src), filled, scale=0.5, count=count)
    assert rest.any() and (filled[t(np.flatnonzero(rest))] == SENT).all()
    return got


@pytest.mark.parametrize("mask", ["none", "mode 1", "mode 2"])
def test_push_list_over_the_f1_and_f2_lists_of_graph_b(mask):
    csr = graph_b()[:3]
    keep, kp, args = mask_args(mask, len(csr[1]))
    g = fmod.handle(csr)
    g.set_edge_mask(*args)
    src = np.random.default_rng(71).standard_normal((NB, 64), dtype=np.float32)
    rowptr = csr[0]
    for case in CASES:
        kind, seed, n = case
        arrs = batch_b(kind, seed, n)[1]
        fr = frontier_of(g, NB, NB_U, kind, arrs, hops=2)
        lst = fr.list.cpu().numpy()
        sets = sets3(csr, rows_of(kind, arrs, NB_U), keep)
        for name, cell, k in (("F1", fr.count_f, 1), ("F2", fr.count_f2, 2)):
            cnt = cell.item()
            assert cnt == len(sets[k])
            rows = lst[:cnt]
            if keep is not None:                                # a listed row with every entry dropped adds nothing
                assert any(rowptr[r + 1] > rowptr[r] and not keep[rowptr[r]:rowptr[r + 1]].any() for r in rows)
            if name == "F2" and mask == "none":
                assert 0 in rows and all(r in rows for r in range(1, 6))         # the hub and the rows of 65 - 200 entries
            check_push(f"{mask}, {case}, {name}", g, csr, fr, cell, rows, src, keep, kp)
    g.set_edge_mask(0)


@pytest.mark.parametrize("mask", ["none", "mode 1"])
def test_push_list_with_more_long_row_tasks_than_a_pass_has_waves(mask):
    csr = heavy_graph()
    n = 4000
    deg = np.diff(csr[0])
    keep = None if mask == "none" else (np.random.default_rng(102).random(len(csr[1])) < 0.3).astype(np.uint8)
    g = fmod.handle(csr)
    if keep is not None:
        g.set_edge_mask(1, t(keep), 0.3, 0)
    heavy = np.concatenate([np.arange(200, 206), np.arange(100, 116)])
    short = np.random.default_rng(24).permutation(np.setdiff1d(np.arange(n), heavy))[:300]
    rows = np.concatenate([short[:7], heavy[::-1], short[7:]])
    tasks = [sum((d + 63) // 64 for d in deg[rows[k:k + 16]] if d > 64) for k in range(0, len(rows), 16)]
    assert max(tasks) > 3 * 16, tasks                            # one pass deals several rounds of long-row tasks to its 16 waves
    src = np.random.default_rng(72).standard_normal((n, 64), dtype=np.float32)
    for _ in range(2):                                           # (a race between the passes' task counts would not show in every launch)
        check_push(f"heavy graph, {mask}", g, csr, listed(n, rows), None, rows, src, keep, 0.3 if keep is not None else 1.0)
    # list lengths around one pass of 16 slots
    for k in (1, 15, 16, 17):
        check_push(f"heavy graph, {mask}, {k} rows", g, csr, listed(n, rows[5:5 + k]), None, rows[5:5 + k], src, keep,
                   0.3 if keep is not None else 1.0)


def test_push_list_skips_invalid_rows_reads_its_count_on_the_device_and_refuses_other_widths():
    from spex_amd import _lib, ops
    rowptr, col, val, n_u, E0 = tiny()
    csr = (rowptr, col, val)
    n = len(rowptr) - 1
    g = fmod.handle(csr)
    src = np.random.default_rng(73).standard_normal((n, 64), dtype=np.float32)
    rows = np.random.default_rng(0).permutation(n)[:40]
    lst = np.insert(rows, [0, 7, 40], [-1, n, n + 5])
    want, _ = scatter64(csr, rows, src, 1.0)
    out = torch.zeros(n, 64, device=DEV)
    ops.spmm_push_list(g, listed(n, lst), t(src), out)
    assert seqmod.rel_err(out.cpu().numpy(), want) <= PUSH_BOUND
    # a count cell of 0 writes nothing
    out = torch.full((n, 64), SENT, device=DEV)
    ops.spmm_push_list(g, listed(n, rows, dev_count=0), t(src), out)
    assert (out == SENT).all()
    # a count above max_count is clipped at max_count
    ur = listed(n, rows, dev_count=10 ** 6)
    ur.capacity = 9
    want9, _ = scatter64(csr, rows[:9], src, 1.0)
    out = torch.zeros(n, 64, device=DEV)
    ops.spmm_push_list(g, ur, t(src), out)
    assert seqmod.rel_err(out.cpu().numpy(), want9) <= PUSH_BOUND and not np.allclose(want9, want)
    # other widths
    with pytest.raises(_lib.SpexError, match="d == 64"):
        ops.spmm_push_list(g, listed(n, rows), torch.zeros(n, 128, device=DEV), torch.zeros(n, 128, device=DEV))
    with pytest.raises(ValueError, match="other than out"):
        ops.spmm_push_list(g, listed(n, rows), out, out)


def test_push_list_past_its_grid_on_the_150_000_row_graph():
    """A list of 70 004 entries (three of them out of range): a grid of at most 2 048 workgroups x 16 slots takes a third pass."""
    import test_gpu_large_graph as lgmod
    from test_large_graph_host import NE, graph_e
    csr = graph_e()
    g = fmod.handle(csr)
    lst, rows = lgmod.big_list()
    assert len(lst) > 2 * 2048 * 16
    src = np.random.default_rng(74).standard_normal((NE, 64), dtype=np.float32)
    check_push("graph (e)", g, csr, listed(NE, lst), None, rows, src)


# ------------------------------------------------------------------------------------------ 3. the list SpMM over the F2 prefix
@pytest.mark.parametrize("mask", ["none", "mode 1", "mode 2"])
def test_rowlist_dev_over_the_f2_prefix_equals_the_whole_graph_launch(mask):
    """count=fr.count_f2: the rows of F2, each bit for bit the whole-graph launch's row (rows of up to 1 024 entries) or the row-list
    kernel's (the hub: the list-driven launch adds a longer row's segments in the row-list kernel's order, as documented)."""
    csr = graph_b()[:3]
    deg = np.diff(csr[0])
    keep, kp, args = mask_args(mask, len(csr[1]))
    g = fmod.handle(csr)
    g.set_edge_mask(*args)
    X = t(table_b())
    want = g.spmm(X)
    ref = g if keep is None else dmod.premasked(csr, keep, kp)
    case = ("bce", 2, 256)
    arrs = batch_b(*case)[1]
    fr = frontier_of(g, NB, NB_U, case[0], arrs)
    f2 = sets3(csr, rows_of(case[0], arrs, NB_U), keep)[2]
    assert fr.count_f2.item() == len(f2) and 0 in f2 and fr.count_f3.item() > len(f2)
    Y = torch.full_like(X, SENT)
    g.spmm_rows_dev(X, fr, Y=Y, count=fr.count_f2)
    short = t(f2[deg[f2] <= 1024].astype(np.int64))
    assert torch.equal(Y[short], want[short])
    hub = t(np.array([0], np.int64))
    if keep is None:
        ref_y = torch.zeros_like(X)
        g.spmm_rows(X, hub, Y=ref_y)
    else:
        ref_y = ref.spmm_rows(X, hub, Y=torch.zeros_like(X))
    assert torch.equal(Y[0], ref_y[0])
    # ... and the hub against fp64: 24 chains of at most 64 fmafs, then 23 adds, on values rounded once more under a mask — a worst case
    # of 90 roundings of 2^-24 on the sum of the terms' magnitudes, per column
    e = np.arange(csr[0][0], csr[0][1])
    if keep is not None:
        e = e[keep[e] != 0]
    terms = (csr[2][e].astype(np.float64) / kp)[:, None] * table_b()[csr[1][e]].astype(np.float64)
    err = np.abs(Y[0].cpu().numpy().astype(np.float64) - terms.sum(0))
    assert len(e) > 400 and (err <= 90 * 2.0 ** -24 * np.abs(terms).sum(0)).all(), err.max()
    rest = torch.ones(NB, dtype=torch.bool, device=DEV)
    rest[t(f2.astype(np.int64))] = False
    assert rest.any() and (Y[rest] == SENT).all()
    g.set_edge_mask(0)


# ------------------------------------------------------------------------------------------ steppers and truths
def deep_b(sparse_adam=False, depth=2):
    from spex_amd.trainer import LightGCNStepper
    g, gt = dmod.handles_of(graph_b()[:3])
    return LightGCNStepper(g, t(table_b().copy()), NB_U, n_layers=3, lr=seqmod.LR, graph_t=gt, weight_decay=seqmod.WD, frontier=True,
                           frontier_depth=depth, sparse_adam=sparse_adam)


def deep_hub(G, sparse_adam=False):
    from spex_amd.trainer import LightGCNStepper
    g, gt = seqmod.handles(G)
    return LightGCNStepper(g, t(seqmod.table(64)), seqmod.N_U, n_layers=3, lr=seqmod.LR, graph_t=gt, weight_decay=seqmod.WD, frontier=True,
                           frontier_depth=2, sparse_adam=sparse_adam)


@contextlib.contextmanager
def keep_prob_of(p):
    """seqmod.restate divides a kept value by the module's KEEP_PROB, and seqmod.take hands it to the handles: p for the duration."""
    saved, seqmod.KEEP_PROB = seqmod.KEEP_PROB, p
    try:
        yield
    finally:
        seqmod.KEEP_PROB = saved


def take_mode2(st, el, seed, form):
    """seqmod.take with the in-kernel sampled mask (mode 2, keep_prob 0.3, `seed`) on the handles."""
    kind, arrs, _ = el
    st.set_edge_dropout((2, None, 0.3, seed))
    a, b, c = (t(x) for x in arrs)
    acc = torch.zeros(1, device=DEV)
    (st.step_bpr_exact if kind == "bpr" else st.step_bce)(a, b, c, loss_acc=acc, batch_rows_only=form == "one call")
    return acc.item() / a.numel()


# ------------------------------------------------------------------------------------------ 4. whole steps against the fp64 truth
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_deep_steps_against_the_fp64_truth_on_graph_b(kind):
    """Four steps, one call and launch by launch; then the same four on ONE stepper that switches frontier_depth and frontier."""
    seq = [batch_b(kind, 2000 + k, 256 if k != 2 else 7) + (None,) for k in range(4)]
    with fmod.restating_on_graph_b():
        truth = seqmod.truth_of(("deep b", kind), seq, 64, 3)
    for form in ("one call", "launches"):
        st = deep_b()
        seqmod.run(st, seq, [form] * 4, truth, f"deep (b) {kind} {form}")
        assert st.t == 4
    want, f32 = truth
    st = deep_b(depth=1)
    plan = [(2, True, "one call"), (1, True, "one call"), (2, True, "launches"), (2, False, "one call")]
    for k, ((depth, frontier, form), el) in enumerate(zip(plan, seq)):
        st.frontier_depth, st.frontier = depth, frontier
        loss = seqmod.take(st, el, form)
        tag = f"deep mix (b) {kind} step {k + 1} (depth {depth}, frontier={frontier}, {form})"
        seqmod.check_invariants(st, form == "one call", tag)
        seqmod.check(tag, seqmod.state(st, loss, kind == "bpr"), want[k], f32[k])


def test_deep_steps_on_the_hub_graph_masked_and_unmasked_switching_forms(G):
    """BCE and exact BPR (weight_decay > 0) with another injected mask per step, masks switched off and on (mode 1, seqmod.keep_mask):
    all deep, one call and launch by launch; then one stepper switching depth 1 <-> 2 and the frontier form off and on."""
    seq = dmod.hub_sequence()
    truth = seqmod.truth_of(("deep hub dropout",), seq, 64, 3)
    for form in ("one call", "launches"):
        st = deep_hub(G)
        seqmod.run(st, seq, [form] * len(seq), truth, f"deep hub {form}")
        assert st.t == len(seq)
    want, f32 = truth
    st = deep_hub(G)
    plan = [(2, True, "one call"), (1, True, "one call"), (2, True, "one call"), (2, False, "launches"), (2, True, "launches"),
            (1, True, "launches"), (2, True, "one call")]
    for k, ((depth, frontier, form), el) in enumerate(zip(plan, seq)):
        st.frontier_depth, st.frontier = depth, frontier
        loss = seqmod.take(st, el, form)
        tag = f"deep hub mix step {k + 1} ({el[0]}, depth {depth}, frontier={frontier}, {form}, masked={el[2] is not None})"
        seqmod.check_invariants(st, form == "one call", tag)
        seqmod.check(tag, seqmod.state(st, loss, el[0] == "bpr"), want[k], f32[k])


@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_deep_steps_under_the_sampled_mask_at_03_on_graph_b(kind):
    """Mode 2 at keep_prob 0.3, a fresh seed per step, restated in NumPy (philox_keep) and handed to the truth."""
    nnz = len(graph_b()[1])
    seeds = [(91 << 32) | (k + 1) for k in range(3)]
    seq = [batch_b(kind, 2100 + k, 256) + (philox_keep(nnz, 0.3, seeds[k]),) for k in range(3)]
    with fmod.restating_on_graph_b(), keep_prob_of(0.3):
        want, f32 = seqmod.truth_of(("deep b mode 2", kind), seq, 64, 3)
    for form in ("one call", "launches"):
        st = deep_b()
        for k, el in enumerate(seq):
            loss = take_mode2(st, el, seeds[k], form)
            tag = f"deep (b) mode 2 {kind} {form} step {k + 1}"
            seqmod.check_invariants(st, form == "one call", tag)
            seqmod.check(tag, seqmod.state(st, loss, kind == "bpr"), want[k], f32[k])
        assert st.t == 3


# ------------------------------------------------------------------------------------------ 5. nothing outside the lists is read
@pytest.mark.parametrize("kind,sparse", [("bce", False), ("bpr", False), ("bce", True)])
def test_nothing_outside_the_lists_is_read(kind, sparse):
    csr = graph_b()[:3]
    el = batch_b(kind, 2 if kind == "bce" else 3, 256)
    f2 = sets3(csr, rows_of(kind, el[1], NB_U))[2]
    out = torch.ones(NB, dtype=torch.bool, device=DEV)
    out[t(f2.astype(np.int64))] = False
    assert out.any()
    a, b = deep_b(sparse), deep_b(sparse)
    nan = float("nan")
    a.ws_fwd[0][out], a.ws_fwd[1][out], a.ws_bwd[1][out], a.ws_bwd[2][out], a.light_out[out] = nan, nan, nan, nan, nan
    acc_a, acc_b = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    args = [t(x) for x in el[1]]
    for st, acc in ((a, acc_a), (b, acc_b)):
        (st.step_bce if kind == "bce" else st.step_bpr_exact)(*args, loss_acc=acc, batch_rows_only=True)
    assert torch.isfinite(acc_a).all() and torch.equal(acc_a, acc_b)              # (the forward has no atomics: the loss sum, bit for bit)
    for name, bound in (("E0", 5e-6), ("m", 1e-5), ("v", 2e-5), ("grad_E0", 1e-5)):        # seqmod.PROJECT_BOUNDS: the float atomics' bounds
        x, y = getattr(a, name), getattr(b, name)
        assert torch.isfinite(x).all(), name
        fig = seqmod.rel_err(x.cpu().numpy(), y.cpu().numpy())
        print(f"NaN outside F2, {kind}, sparse_adam={sparse}: {name} {fig:.2e}")
        assert fig <= bound, (name, fig)


# ------------------------------------------------------------------------------------------ 6. row-sparse Adam at depth 2
def sparse_law(seq, sparse, inside_of, dtype, np_dtype):
    """The sequence on graph (b) under the sparse law in `dtype` on the CPU: per step seqmod.restate's single step from the law's own
    table; where sparse[k], Adam with the global t moves the rows of inside_of[k] (the step's F3) only."""
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, seqmod.LR
    W = table_b().astype(np_dtype)
    m, v = np.zeros_like(W), np.zeros_like(W)
    out = []
    for k, el in enumerate(seq):
        with fmod.restating_on_graph_b():
            saved, seqmod.table = seqmod.table, (lambda d, W=W: W)
            try:
                one = seqmod.restate([el], 64, 3, seqmod.WD, dtype)[0]
            finally:
                seqmod.table = saved
        g = one["grad"]
        assert not g[~inside_of[k]].any(), "the restated gradient leaves F3"
        step = k + 1
        m_new, v_new = m + (1 - b1) * (g - m), b2 * v + (1 - b2) * g * g
        W_new = W - (lr / (1 - b1 ** step)) * (m_new / (np.sqrt(v_new) / np.sqrt(1 - b2 ** step) + eps))
        move = inside_of[k][:, None] if sparse[k] else np.ones((NB, 1), bool)
        W, m, v = (np.where(move, new, old).astype(np_dtype) for new, old in ((W_new, W), (m_new, m), (v_new, v)))
        out.append({"loss": one["loss"], "E0": W, "m": m, "v": v, "grad": g})
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", ["one call", "launches"])
def test_sparse_adam_at_depth_two_moves_f3_only(form, masked):
    """BCE, BPR, BCE, BPR on graph (b) with sparse_adam on, on, OFF, on (masked: another mode-1 mask per step at seqmod.KEEP_PROB, the
    second step unmasked).  Rows outside a sparse step's F3: E0, m, v bit-identical before and after, grad_E0 zero — also behind the
    dense step, which leaves grad_E0 full.  Inside: the fp64 truth of the same law under seqmod's gate."""
    csr = graph_b()[:3]
    kp = seqmod.KEEP_PROB
    masks = [None] * 4
    if masked:
        masks = [dmod.keep_b(kp), None, (np.random.default_rng(104).random(len(csr[1])) < kp).astype(np.uint8), dmod.keep_b(kp)]
    plan = (("bce", 256), ("bpr", 256), ("bce", 7), ("bpr", 256))
    sparse = [True, True, False, True]
    seq = [batch_b(kind, 2200 + k, n, hub=k != 1) + (masks[k],) for k, (kind, n) in enumerate(plan)]
    inside_of = []
    for kind, arrs, keep in seq:
        inside = np.zeros(NB, bool)
        inside[sets3(csr, rows_of(kind, arrs, NB_U), keep)[3]] = True
        assert 0 < inside.sum() < NB
        inside_of.append(inside)
    want = sparse_law(seq, sparse, inside_of, torch.float64, np.float64)
    f32 = [seqmod.figures(a, b) for a, b in zip(sparse_law(seq, sparse, inside_of, torch.float32, np.float32), want)]
    st = deep_b(sparse_adam=True)
    for k, el in enumerate(seq):
        st.sparse_adam = sparse[k]
        before = [x.clone() for x in (st.E0, st.m, st.v)]
        loss = seqmod.take(st, el, form)
        tag = f"deep sparse Adam {form} masked={masked} step {k + 1} ({el[0]}, sparse_adam={sparse[k]})"
        if sparse[k]:
            out = t(np.flatnonzero(~inside_of[k]))
            for name, x, x0 in zip(("E0", "m", "v"), (st.E0, st.m, st.v), before):
                assert torch.equal(x[out], x0[out]), f"{tag}: {name} moved outside F3"
            assert not st.grad_E0[out].any(), f"{tag}: grad_E0 is not zero outside F3"
        seqmod.check(tag, seqmod.state(st, loss, el[0] == "bpr"), want[k], f32[k])
        seqmod.check_invariants(st, form == "one call", tag)
        if form == "one call" and sparse[k]:
            assert not st.ws_bwd[1].any(), f"{tag}: W is not all-zero after a sparse deep step"
    assert st.t == 4


@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_first_sparse_step_from_zero_moments_equals_the_dense_deep_step(kind):
    el = batch_b(kind, 2300, 256) + (None,)
    with fmod.restating_on_graph_b():
        _, f32 = seqmod.truth_of(("deep first", kind), [el], 64, 3)
    a, b = deep_b(sparse_adam=True), deep_b()
    la, lb = seqmod.take(a, el, "one call"), seqmod.take(b, el, "one call")
    assert la == lb                                              # one addend each, the same fixed order
    fig = seqmod.rel_err(a.E0.cpu().numpy(), b.E0.cpu().numpy())
    print(f"first sparse deep step vs dense deep step ({kind}): E0 {fig:.2e}")
    assert fig <= seqmod.bounds_of(f32[0])["E0"]


# ------------------------------------------------------------------------------------------ 7. epochs
@pytest.mark.parametrize("kind,sparse", [("bce", False), ("bpr", False), ("bce", True), ("bpr", True)])
def test_deep_epochs_at_keep_prob_03_equal_the_single_steps(kind, sparse):
    B, steps, drop_seed = 256, 3, 77
    els = [batch_b(kind, 2400 + k, B) for k in range(steps)]
    arrs = [t(np.concatenate([el[1][j] for el in els])) for j in range(3)]
    a, c = deep_b(sparse), deep_b(sparse)
    acc_a, acc_c = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
    (a.epoch_bce if kind == "bce" else a.epoch_bpr)(*arrs, B, acc_a[0], acc_a[1], keep_prob=0.3, drop_seed=drop_seed)
    assert a.graph.mask_mode == 0 and a.graph_t.mask_mode == 0
    for k, el in enumerate(els):
        c.set_edge_dropout((2, None, 0.3, (drop_seed << 32) | (k + 1)))
        (c.step_bce if kind == "bce" else c.step_bpr_exact)(*(t(x) for x in el[1]), loss_acc=acc_c[0], batch_rows_only=True)
    assert a.t == c.t == steps and acc_a[1].item() == 0.0
    fmod.compare(f"deep epoch {kind} sparse_adam={sparse} keep_prob 0.3", acc_a[0].cpu().numpy(), acc_c[0].cpu().numpy(), a, c)


def test_a_sampled_epoch_runs_on_a_deep_stepper():
    from spex_amd.trainer import BceDeviceSampler
    pairs = graph_b()[3]
    s = BceDeviceSampler(pairs, NB_U, NB_I, num_ng=1, seed=5, device=DEV)
    st = deep_b(sparse_adam=True)
    acc = torch.zeros(2, 1, device=DEV)
    st.epoch_bce_sampled(s, 1, 256, acc[0], acc[1], max_steps=2, keep_prob=0.3, drop_seed=3)
    assert st.t == 2 and acc[0].item() > 0 and torch.isfinite(st.E0).all()


# ------------------------------------------------------------------------------------------ 8. refusals
def test_python_refusals():
    from spex_amd.trainer import LightGCNStepper
    g, gt = dmod.handles_of(graph_b()[:3])
    E0 = t(table_b().copy())
    mk = lambda **kw: LightGCNStepper(g, E0, NB_U, lr=seqmod.LR, graph_t=gt, **kw)
    with pytest.raises(ValueError, match="built with frontier=True"):
        mk(n_layers=3, frontier_depth=2)
    with pytest.raises(ValueError, match="n_layers == 3"):
        mk(n_layers=2, frontier=True, frontier_depth=2)
    with pytest.raises(ValueError, match="width of 64"):
        LightGCNStepper(g, torch.zeros(NB, 128, device=DEV), NB_U, n_layers=3, graph_t=gt, frontier=True, frontier_depth=2)
    with pytest.raises(ValueError, match="deterministic=True"):
        mk(n_layers=3, frontier=True, frontier_depth=2, deterministic=True)
    with pytest.raises(ValueError, match="1 or 2"):
        mk(n_layers=3, frontier=True, frontier_depth=3)
    with pytest.raises(ValueError, match="only with frontier=True and n_layers == 2"):
        mk(n_layers=3, frontier=True, sparse_adam=True)          # sparse Adam at three layers comes with depth 2 only
    plain = mk(n_layers=3)
    with pytest.raises(ValueError, match="built with frontier=True"):
        plain.frontier_depth = 2
    assert plain.frontier_depth == 1
    st = mk(n_layers=3, frontier=True, frontier_depth=2)
    with pytest.raises(ValueError, match="frontier_depth is 2"):
        st.gather_dtype = torch.bfloat16
    st.frontier_depth = 1
    st.gather_dtype = torch.bfloat16
    with pytest.raises(ValueError, match="gather_dtype is torch.bfloat16"):
        st.frontier_depth = 2
    st.gather_dtype = None
    st.frontier_depth = 2
    st.sparse_adam = True
    with pytest.raises(ValueError, match="not while sparse_adam is on"):
        st.frontier_depth = 1
    assert st.frontier_depth == 2 and st.sparse_adam is True
    st.sparse_adam = False
    st.frontier_depth = 1
    with pytest.raises(ValueError, match="built with frontier=True and n_layers == 2"):
        st.sparse_adam = True
    st.frontier_depth = 2
    # a mask on a stepper whose graph_t is graph
    sym = LightGCNStepper(g, E0, NB_U, n_layers=3, lr=seqmod.LR, frontier=True, frontier_depth=2)
    _, (u, i, y) = batch_b("bce", 1, 7)
    acc = torch.zeros(2, 1, device=DEV)
    with pytest.raises(ValueError, match="does not combine with edge dropout"):
        sym.set_edge_dropout((2, None, 0.3, 5))
    with pytest.raises(ValueError, match="does not combine with edge dropout"):
        sym.epoch_bce(t(u), t(i), t(y), 7, acc[0], acc[1], keep_prob=0.3)
    for x in (st, sym):
        assert x.t == 0 and torch.equal(x.E0, t(table_b()))
    # a stepper with the transposed handle takes both, and both still step
    st.epoch_bce(t(u), t(i), t(y), 7, acc[0], acc[1], keep_prob=0.3)
    sym.step_bce(t(u), t(i), t(y), loss_acc=acc[0], batch_rows_only=True)
    assert st.t == 1 and sym.t == 1 and torch.isfinite(st.E0).all() and torch.isfinite(sym.E0).all()


def test_native_refusals():
    from spex_amd import _lib
    from spex_amd.graph import _stream
    from spex_amd.trainer import LightGCNStepper
    lib = _lib.load()
    g = fmod.handle(graph_b())
    _, (u, i, y) = batch_b("bce", 1, 7)
    u, i, y = t(u), t(i), t(y)
    acc = torch.zeros(1, device=DEV)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    st = LightGCNStepper(g, t(table_b().copy()), NB_U, n_layers=3, frontier=True, frontier_depth=2)
    st16 = LightGCNStepper(g, t(table_b().copy()), NB_U, n_layers=3, frontier=True)
    st16.gather_dtype = torch.bfloat16

    def status(flags, bpr=False, L=3, d=64, st=st):
        desc = st._prepare_desc(7, 3 if bpr else 2)
        desc.flags, desc.L, desc.d = flags, L, d
        name = "spex_lightgcn_step_bpr_adam_f32" if bpr else "spex_lightgcn_step_bce_f32"
        rc = getattr(lib, name)(ctypes.byref(desc), vp(u), vp(i), vp(i) if bpr else vp(y), 7, vp(acc), _stream(None))
        t_after = desc.t
        desc.L, desc.d = 3, 64
        assert t_after == 0
        return rc, lib.spex_last_error().decode()

    F, S, D = _lib.STEP_FRONTIER, _lib.STEP_SPARSE_ADAM, _lib.STEP_FRONTIER_DEEP
    for bpr in (False, True):
        rc, msg = status(D, bpr)
        assert rc == -1 and "needs SPEX_STEP_FRONTIER" in msg
        for L in (2, 4):
            rc, msg = status(F | D, bpr, L=L)
            assert rc == -1 and "L == 3" in msg
        rc, msg = status(F | D, bpr, d=128)
        assert rc == -4 and "d == 64" in msg
        rc, msg = status(F | D | _lib.STEP_BF16_GATHER, bpr)     # (E0_16 is NULL here: the bf16 check itself speaks first)
        assert rc == -1 and "E0_16" in msg
        # ... and on a descriptor that satisfies the bf16 check — a frontier stepper with bf16 tables — the deep check refuses the pair
        rc, msg = status(F | D | _lib.STEP_BF16_GATHER, bpr, st=st16)
        assert rc == -1 and "SPEX_STEP_FRONTIER_DEEP" in msg and "SPEX_STEP_BF16_GATHER" in msg, msg
        assert status(F | _lib.STEP_BF16_GATHER, bpr, L=1, st=st16)[0] != 0 and st16.t == 0
        rc, msg = status(F | D | _lib.STEP_DETERMINISTIC, bpr)
        assert rc == -1 and "SPEX_STEP_DETERMINISTIC" in msg
        rc, msg = status(F | S, bpr)                             # three layers without the new flag: still refused
        assert rc == -1 and "L == 2" in msg
        rc, msg = status(F | S | D, bpr, L=2)
        assert rc == -1 and "L == 3" in msg
    rc, msg = status(F | D | _lib.STEP_BPR_DENSE, True)
    assert rc == -1 and "SPEX_STEP_BPR_DENSE" in msg
    rc, msg = status(F | D | _lib.STEP_WIDE, True)
    assert rc == -4 and "d == 64" in msg
    g.set_edge_mask(2, None, 0.3, 5)                             # a mask on a stepper whose graph_t == graph
    try:
        for flags in (F | D, F | D | S):
            rc, msg = status(flags)
            assert rc == -1 and "edge dropout" in msg
    finally:
        g.set_edge_mask(0)
    assert st.t == 0 and torch.equal(st.E0, t(table_b()))
    assert st16.t == 0 and torch.equal(st16.E0, t(table_b()))
    st16.step_bce(u, i, y, loss_acc=acc, batch_rows_only=True)          # (frontier x bf16 at depth 1: still steps)
    assert st16.t == 1 and torch.isfinite(st16.E0).all()
    acc.zero_()
    st.step_bce(u, i, y, loss_acc=acc, batch_rows_only=True)
    assert st.t == 1 and torch.isfinite(st.E0).all() and acc.item() > 0
