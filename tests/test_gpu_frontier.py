"""SPEX_STEP_FRONTIER: the frontier list kernel, the list-driven row-list SpMM, and the exact LightGCN steps that run forward layer
L - 1 and the second backward product over the batch's frontier F1 = Bset U { stored columns of Bset's rows }.

Graphs.  (a) the tiny golden graph (111 rows; its frontier is almost everything).  (b) `graph_b()`: a seeded symmetric bipartite
graph of 20 000 rows (8 000 user rows), ~3 entries per row, LightGCN's 1 / sqrt(deg deg) values, with user 0 a hub of 1 500 entries
(> 1 024: the row-list kernels' chained segments), users 1 .. 5 of 65, 100, 128, 129 and 200 entries (2 to 4 segments), users
10 .. 19 and the last ten items empty; a 256-sample batch's F1 is a few percent of its rows.  (c) the hub graph of
tests/test_gpu_stepper_sequences.py (3 000 rows, not symmetric, a real transpose) with that module's batches.  (d) `heavy_graph()`:
22 rows of 300 .. 2 600 entries among short ones, for list passes whose long rows need more wave tasks than the kernel has LDS slots.

Whole steps are compared with the fp64 restatement of tests/test_gpu_stepper_sequences.py (`restate`, imported, on (c) as it stands
and on (b) with the module's graph swapped for the call) under that module's gate, unchanged: per quantity the larger of the
project's bound and 4 x the figure of the same sequence restated in fp32 on the CPU.  Batches repeat users and items.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_stepper_sequences as seqmod
from conftest import REPO

pytestmark = pytest.mark.gpu

DEV = "cuda"
NB, NB_U = 20000, 8000
NB_I = NB - NB_U
LONG_USERS = {0: 1500, 1: 65, 2: 100, 3: 128, 4: 129, 5: 200}
EPOCH_BOUNDS = (2e-6, 2e-5, 2e-5, 4e-5)          # loss, E0, m, v: tests/test_gpu_bce_device_sampler.py::EPOCH_BOUNDS
_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------ graphs
def graph_b():
    """(rowptr, col, val, train pairs) of graph (b)."""
    if "b" not in _cache:
        rng = np.random.default_rng(11)
        u = rng.integers(20, NB_U, 28000)
        i = rng.integers(0, NB_I - 10, 28000)
        for user, deg in LONG_USERS.items():
            u = np.concatenate([u, np.full(deg, user)])
            i = np.concatenate([i, rng.choice(NB_I - 10, deg, replace=False)])
        pairs = np.unique(np.stack([u, i], 1), axis=0).astype(np.int64)
        rows = np.concatenate([pairs[:, 0], pairs[:, 1] + NB_U])
        cols = np.concatenate([pairs[:, 1] + NB_U, pairs[:, 0]])
        order = np.lexsort((cols, rows))
        rows, cols = rows[order], cols[order]
        deg = np.bincount(rows, minlength=NB)
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        val = (1.0 / np.sqrt(deg[rows].astype(np.float64) * deg[cols])).astype(np.float32)
        assert deg[0] == 1500 and list(deg[1:6]) == [65, 100, 128, 129, 200] and not deg[10:20].any() and not deg[-10:].any()
        assert 2.5 <= deg.mean() <= 3.5
        _cache["b"] = (rowptr, cols.astype(np.int32), val, pairs)
    return _cache["b"]


def tiny():
    if "tiny" not in _cache:
        g = np.load(f"{REPO}/tests/golden/lightgcn_tiny.npz")
        _cache["tiny"] = (g["rowptr"], g["col"], g["val"], int(g["n_user"]) + 1, g["E0"])
    return _cache["tiny"]


def table_b():
    if "E0b" not in _cache:
        _cache["E0b"] = (0.1 * np.random.default_rng(7).normal(size=(NB, 64))).astype(np.float32)
    return _cache["E0b"]


def handle(csr):
    from spex_amd.graph import SpexGraph
    return SpexGraph(*csr[:3])


def batch_b(kind, seed, n, hub=True):
    """A batch on graph (b) with repeated users and items; from 7 samples up it names the hub, a two-segment user and an empty user.
    hub=False: neither the hub nor an item of the hub's row, so that the hub is not in F1 (a four-segment user in its place)."""
    rng = np.random.default_rng(seed)
    u, a, b = rng.integers(0, NB_U, n), rng.integers(0, NB_I, n), rng.integers(0, NB_I, n)
    if not hub:
        rowptr, col = graph_b()[:2]
        free = np.setdiff1d(np.arange(NB_I), col[rowptr[0]:rowptr[1]] - NB_U)
        u, a, b = rng.integers(1, NB_U, n), rng.choice(free, n), rng.choice(free, n)
    if n >= 7:
        u[:3] = [0 if hub else 5, 4, 12]
        a[0] = NB_I - 3
    u[-1], a[-1] = u[1], a[1]
    if kind == "bce":
        return "bce", (u.astype(np.int64), a.astype(np.int64), rng.integers(0, 2, n).astype(np.float32))
    return "bpr", (u.astype(np.int64), a.astype(np.int64), b.astype(np.int64))


def frontier_sets(csr, rows):
    """(Bset, F1) as sorted arrays, in NumPy."""
    rowptr, col = csr[0], csr[1]
    n = len(rowptr) - 1
    bset = np.unique(rows[(rows >= 0) & (rows < n)])
    cols = np.concatenate([col[rowptr[r]:rowptr[r + 1]] for r in bset] + [np.zeros(0, np.int32)])
    return bset, np.union1d(bset, cols)


# ------------------------------------------------------------------------------------------ 1. the frontier list
@pytest.mark.parametrize("which", ["tiny", "b"])
def test_frontier_list_is_the_numpy_set(which):
    from spex_amd import ops
    if which == "tiny":
        rowptr, col, val, n_u, _ = tiny()
        csr, n = (rowptr, col, val), len(rowptr) - 1
        batches = [(np.array([0, 3, 3, 7, 49], np.int64), np.array([1, 1, 5, 20, 59], np.int64))]
        batches.append((np.arange(0, n_u, dtype=np.int64), np.arange(0, n - n_u, dtype=np.int64)))
    else:
        csr, n, n_u = graph_b()[:3], NB, NB_U
        batches = [batch_b("bce", s, k)[1][:2] for s, k in ((1, 7), (2, 256))]
        batches.append((np.array([0, 0, 12, 9000, -4], np.int64), np.array([5, NB_I - 1, 5, NB_I + 3, 7], np.int64)))   # hub, empty, invalid
        assert 0 in batches[1][0]
    g = handle(csr)
    fr = ops.FrontierRows(n, torch.device(DEV, torch.cuda.current_device()))
    for k, (a, b) in enumerate(batches * 2):                    # the second round: new epochs on the same stamp table, no clearing
        fr.update(t(a), t(b), 0, n_u).expand(g)
        bset, f1 = frontier_sets(csr, np.concatenate([a, b + n_u]))
        cb, cf = fr.count.item(), fr.count_f.item()
        lst = fr.list.cpu().numpy()
        assert (cb, cf) == (len(bset), len(f1)), (which, k)
        assert np.array_equal(np.sort(lst[:cb]), bset) and np.array_equal(np.sort(lst[:cf]), f1), (which, k)
        if which == "b":
            assert cf < 0.25 * n                       # a small share of the rows
    assert fr.epoch == 2 * len(batches)


# ------------------------------------------------------------------------------------------ 2. the list-driven row-list SpMM
def listed(n, rows, dev_count=None):
    """A UniqueRows-shaped list object over `rows` (distinct) for SpexGraph.spmm_rows_dev."""
    from spex_amd import ops
    ur = ops.UniqueRows(n, n, torch.device(DEV, torch.cuda.current_device()))
    ur.list[:len(rows)] = t(np.asarray(rows, np.int32))
    ur.count.fill_(len(rows) if dev_count is None else dev_count)
    return ur


def test_rowlist_dev_equals_the_whole_graph_launch_and_the_rowlist_kernel():
    csr = graph_b()
    g = handle(csr)
    X = t(table_b())
    acc = t((0.3 * np.random.default_rng(3).normal(size=(NB, 64))).astype(np.float32))
    want_y, want_acc = torch.empty_like(X), torch.empty_like(X)
    g.spmm(X, Y=want_y, acc_in=acc, acc_out=want_acc, acc_div=3.0)
    deg = np.diff(csr[0])
    # a frontier-like list: the hub, the multi-segment users, empty rows, and a random tenth of the rest, in random order
    rng = np.random.default_rng(4)
    rows = np.unique(np.concatenate([[0, 1, 2, 3, 4, 5, 10, 11, NB - 1], rng.choice(NB, 2000, replace=False)]))
    rows = rng.permutation(rows)
    SENT = 12345.0
    Y, A = torch.full_like(X, SENT), torch.full_like(X, SENT)
    g.spmm_rows_dev(X, listed(NB, rows), Y=Y, acc_in=acc, acc_out=A, acc_div=3.0)
    short = t(rows[deg[rows] <= 1024].astype(np.int64))
    assert torch.equal(Y[short], want_y[short]) and torch.equal(A[short], want_acc[short])
    hub = t(np.array([0], np.int64))
    ref_y, ref_acc = torch.zeros_like(X), torch.zeros_like(X)
    g.spmm_rows(X, hub, Y=ref_y, acc_in=acc, acc_out=ref_acc, acc_div=3.0)
    assert deg[0] > 1024 and torch.equal(Y[0], ref_y[0]) and torch.equal(A[0], ref_acc[0])
    rest = torch.ones(NB, dtype=torch.bool, device=DEV)
    rest[t(rows.astype(np.int64))] = False
    assert (Y[rest] == SENT).all() and (A[rest] == SENT).all()
    # the running sum in place: acc_out is acc_in
    acc2 = acc.clone()
    g.spmm_rows_dev(X, listed(NB, rows), acc_in=acc2, acc_out=acc2, acc_div=3.0)
    assert torch.equal(acc2[short], want_acc[short]) and torch.equal(acc2[0], ref_acc[0]) and torch.equal(acc2[rest], acc[rest])
    # count = 0 writes nothing; a device count beyond the capacity is cut at the capacity
    Y0 = torch.full_like(X, SENT)
    g.spmm_rows_dev(X, listed(NB, rows, dev_count=0), Y=Y0)
    assert (Y0 == SENT).all()
    # every row, in a random order: 1 250 passes of 16 slots over a grid of at most 1 024 workgroups
    every = rng.permutation(NB)
    Ya = torch.full_like(X, SENT)
    g.spmm_rows_dev(X, listed(NB, every), Y=Ya)
    ok = t(np.flatnonzero(deg <= 1024).astype(np.int64))
    assert torch.equal(Ya[ok], want_y[ok]) and torch.equal(Ya[0], ref_y[0])


def heavy_graph():
    """4 000 x 4 000, rows of 1 .. 49 entries, with rows 100 .. 115 of 300 .. 1 100 entries (5 .. 16 wave tasks each) and rows
    200 .. 205 beyond 1 024 entries (16 tasks each, chained segments): 16 adjacent list slots of them need far more than the kernel's
    64 LDS task slots, so part 2 of a pass runs several groups."""
    if "heavy" not in _cache:
        rng = np.random.default_rng(21)
        deg = rng.integers(1, 50, 4000)
        deg[100:116] = np.linspace(300, 1100, 16).astype(np.int64)
        deg[200:206] = [1100, 1300, 1500, 2000, 2600, 1025]
        rowptr, col, val = seqmod.random_csr(rng, 4000, 4000, deg)
        _cache["heavy"] = (rowptr, col, val * np.float32(0.05))
    return _cache["heavy"]


def groups_of_pass(deg16):
    """How many part-2 groups a pass over 16 slots of these degrees takes (64 task slots, rows packed in order)."""
    tasks = [min((d + 63) // 64, 16) if d > 64 else 0 for d in deg16]
    groups, total = 0, 0
    for k in tasks:
        if total + k > 64:
            groups, total = groups + 1, 0
        total += k
    return groups + (1 if total else 0)


@pytest.mark.parametrize("layout", ["heavy rows first", "straddling passes", "shuffled"])
def test_rowlist_dev_with_more_long_row_tasks_than_lds_slots_in_one_pass(layout):
    """16 adjacent list slots holding more than 64 wave tasks: part 2 of the pass runs several groups over the same LDS slots.  Bit
    for bit spex_spmm_rowlist_f32 on every row, and spex_spmm_f32 on the rows of up to 1 024 entries."""
    csr = heavy_graph()
    g = handle(csr)
    n = 4000
    deg = np.diff(csr[0])
    X = t((0.1 * np.random.default_rng(22).normal(size=(n, 64))).astype(np.float32))
    acc = t((0.3 * np.random.default_rng(23).normal(size=(n, 64))).astype(np.float32))
    heavy = np.concatenate([np.arange(200, 206), np.arange(100, 116)])
    rng = np.random.default_rng(24)
    short = rng.permutation(np.setdiff1d(np.arange(n), heavy))[:300]
    if layout == "heavy rows first":
        rows = np.concatenate([heavy, short])
    elif layout == "straddling passes":
        rows = np.concatenate([short[:7], heavy[::-1], short[7:]])
    else:
        rows = rng.permutation(np.concatenate([heavy, short[:26]]))        # 48 slots, 22 of them heavy
        rows = np.concatenate([rows, short[26:]])
    worst = max(groups_of_pass(deg[rows[k:k + 16]]) for k in range(0, len(rows), 16))
    assert worst >= (3 if layout != "shuffled" else 2), worst
    idx = t(rows.astype(np.int64))
    want_y, want_acc = torch.zeros_like(X), torch.zeros_like(X)
    g.spmm_rows(X, idx, Y=want_y, acc_in=acc, acc_out=want_acc, acc_div=4.0)
    full_y, full_acc = torch.empty_like(X), torch.empty_like(X)
    g.spmm(X, Y=full_y, acc_in=acc, acc_out=full_acc, acc_div=4.0)
    SENT = 777.0
    for _ in range(3):                                          # (a race between groups would not show in every launch)
        Y, A = torch.full_like(X, SENT), torch.full_like(X, SENT)
        g.spmm_rows_dev(X, listed(n, rows), Y=Y, acc_in=acc, acc_out=A, acc_div=4.0)
        assert torch.equal(Y[idx], want_y[idx]) and torch.equal(A[idx], want_acc[idx])
        upto = t(rows[deg[rows] <= 1024].astype(np.int64))
        assert torch.equal(Y[upto], full_y[upto]) and torch.equal(A[upto], full_acc[upto])
        rest = torch.ones(n, dtype=torch.bool, device=DEV)
        rest[idx] = False
        assert (Y[rest] == SENT).all() and (A[rest] == SENT).all()


def test_rowlist_dev_on_the_tiny_graph_and_its_refusals():
    from spex_amd import _lib
    rowptr, col, val, n_u, E0 = tiny()
    g = handle((rowptr, col, val))
    n = len(rowptr) - 1
    X = t(E0)
    want = g.spmm(X)
    rows = np.random.default_rng(0).permutation(n)[:70]
    Y = torch.zeros_like(X)
    g.spmm_rows_dev(X, listed(n, rows), Y=Y)
    assert torch.equal(Y[t(rows.astype(np.int64))], want[t(rows.astype(np.int64))])
    X128 = torch.zeros(n, 128, device=DEV)
    with pytest.raises(_lib.SpexError, match="d == 64"):
        g.spmm_rows_dev(X128, listed(n, rows), Y=torch.zeros_like(X128))


# ------------------------------------------------------------------------------------------ steppers
def stepper_b(L, frontier, weight_decay=seqmod.WD):
    from spex_amd.trainer import LightGCNStepper
    return LightGCNStepper(handle(graph_b()), t(table_b().copy()), NB_U, n_layers=L, lr=seqmod.LR, weight_decay=weight_decay, frontier=frontier)


def stepper_hub(G, L, frontier=True):
    from spex_amd.trainer import LightGCNStepper
    g, gt = seqmod.handles(G)
    return LightGCNStepper(g, t(seqmod.table(64)), seqmod.N_U, n_layers=L, lr=seqmod.LR, graph_t=gt, weight_decay=seqmod.WD, frontier=frontier)


@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


@contextlib.contextmanager
def restating_on_graph_b():
    """seqmod.restate reads the module's graph, N and N_U: hand it graph (b) and table_b for the duration (the file itself is untouched)."""
    saved = (seqmod._cache.get("hub"), seqmod.N, seqmod.N_U, seqmod.table)
    seqmod._cache["hub"], seqmod.N, seqmod.N_U, seqmod.table = graph_b()[:3], NB, NB_U, lambda d: table_b()
    try:
        yield
    finally:
        seqmod._cache["hub"], seqmod.N, seqmod.N_U, seqmod.table = saved
        if saved[0] is None:
            del seqmod._cache["hub"]


# ------------------------------------------------------------------------------------------ 3. nothing is read outside F1
@pytest.mark.parametrize("L", [2, 3, 4])
def test_nothing_outside_the_frontier_is_read(L):
    # (batches that keep the hub out of F1: on a row beyond 1 024 entries the list-driven launch and the whole-graph launch add the
    #  segments in different orders, as documented, and everything gathered from that row would differ in the last bit)
    kind, (u, i, y) = batch_b("bce", 30 + L, 256, hub=False)
    u, i, y = t(u), t(i), t(y)
    rows = torch.cat([u, i + NB_U])
    nan = float("nan")
    # launch by launch: lo_batch at the batch's rows, bit for bit
    a, b = stepper_b(L, True), stepper_b(L, False)
    a.lo_batch = torch.full_like(a.light_out, nan)
    a.ws_fwd.fill_(nan)
    a.light_out.fill_(nan)
    loss_a = a.step_bce(u, i, y, batch_rows_only=True)
    loss_b = b.step_bce(u, i, y, batch_rows_only=True)
    assert torch.isfinite(a.lo_batch[rows]).all() and torch.equal(a.lo_batch[rows], b.lo_batch[rows])
    assert torch.isfinite(loss_a) and abs(loss_a.item() - loss_b.item()) <= 1e-6 * abs(loss_b.item())     # (score_bce adds the losses with atomics)
    assert torch.isfinite(a.E0).all()
    # one call: the loss sum (per-sample losses added in order by the Adam pass), bit for bit
    a, b = stepper_b(L, True), stepper_b(L, False)
    a.ws_fwd.fill_(nan)
    a.light_out.fill_(nan)
    acc_a, acc_b = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    a.step_bce(u, i, y, loss_acc=acc_a, batch_rows_only=True)
    b.step_bce(u, i, y, loss_acc=acc_b, batch_rows_only=True)
    assert torch.isfinite(acc_a).all() and torch.equal(acc_a, acc_b) and torch.isfinite(a.E0).all()
    # exact BPR, one call
    kind, (u, p, ng) = batch_b("bpr", 40 + L, 300, hub=False)
    a, b = stepper_b(L, True), stepper_b(L, False)
    a.ws_fwd.fill_(nan)
    a.light_out.fill_(nan)
    b.bpr_backward = "push"
    acc_a, acc_b = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    a.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc_a, batch_rows_only=True)
    b.step_bpr_exact(t(u), t(p), t(ng), loss_acc=acc_b, batch_rows_only=True)
    assert torch.isfinite(acc_a).all() and torch.equal(acc_a, acc_b) and torch.isfinite(a.E0).all()


# ------------------------------------------------------------------------------------------ 4. step equivalence
SIZES = {"bce": (7, 256), "bpr": (5, 300)}


def hub_batch(kind, seed, n):
    """seqmod's batch of n samples; its BPR generator needs 7 triples for its special rows: T = 5 is the head of such a batch, the
    last triple again repeating the first one's (user, positive)."""
    if kind == "bce":
        return seqmod.bce_batch(seed, n)
    if n >= 7:
        return seqmod.bpr_batch(seed, n)
    _, (u, p, ng) = seqmod.bpr_batch(seed, 7)
    u, p, ng = u[:n].copy(), p[:n].copy(), ng[:n].copy()
    u[-1], p[-1] = u[0], p[0]
    return "bpr", (u, p, ng)


@pytest.mark.parametrize("kind,L,big", [(k, L, big) for k in ("bce", "bpr") for L in (2, 3, 4) for big in (0, 1)])
def test_frontier_steps_against_the_fp64_truth_on_the_hub_graph(G, kind, L, big):
    """Five steps, one call and launch by launch, each step against the truth under seqmod's gate."""
    n = SIZES[kind][big]
    seq = [hub_batch(kind, 700 + k, n) + (None,) for k in range(5)]
    truth = seqmod.truth_of(("frontier", kind, L, n), seq, 64, L)
    for form in ("one call", "launches"):
        st = stepper_hub(G, L)
        seqmod.run(st, seq, [form] * 5, truth, f"frontier {kind} L={L} n={n} {form}")
        assert st.t == 5


@pytest.mark.parametrize("kind,L,n", [("bce", 2, 256), ("bpr", 3, 300), ("bce", 4, 7), ("bpr", 2, 5)])
def test_frontier_steps_against_the_fp64_truth_on_graph_b(kind, L, n):
    """The same on graph (b), where F1 is a small share of the rows: a row outside F1 that the step needed would be missed here."""
    seq = [batch_b(kind, 800 + k, n) + (None,) for k in range(5)]
    with restating_on_graph_b():
        truth = seqmod.truth_of(("frontier b", kind, L, n), seq, 64, L)
    for form in ("one call", "launches"):
        st = stepper_b(L, True)
        seqmod.run(st, seq, [form] * 5, truth, f"frontier (b) {kind} L={L} n={n} {form}")


# ------------------------------------------------------------------------------------------ 5. sequences on one stepper
@pytest.mark.parametrize("L", [2, 3])
def test_frontier_and_whole_graph_steps_alternate_on_one_stepper(G, L):
    """Nine steps on one stepper built with frontier=True, `stepper.frontier` switched from step to step: BPR and BCE, one call and
    launch by launch, a native epoch of one step in between.  A whole-graph step leaves grad_E0 (L = 2: the frontier push's target)
    and ws_bwd[1] full: a push target that was not cleared fails the next frontier step's gradient."""
    plan = [("bpr", "one call", True), ("bce", "one call", False), ("bce", "launches", True), ("bpr", "one call", False),
            ("bce", "epoch", True), ("bpr", "launches", True), ("bce", "one call", True), ("bpr", "one call", True),
            ("bce", "launches", False)]
    seq = [(seqmod.bpr_batch if kind == "bpr" else seqmod.bce_batch)(900 + k, 17) + (None,) for k, (kind, _, _) in enumerate(plan)]
    want, f32 = seqmod.truth_of(("frontier mix", L), seq, 64, L)
    st = stepper_hub(G, L)
    for k, ((kind, form, frontier), el) in enumerate(zip(plan, seq)):
        st.frontier = frontier
        tag = f"mix L={L} step {k + 1} ({kind}, {form}, frontier={frontier})"
        if form == "epoch":
            full, ragged = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
            st.epoch_bce(*(t(x) for x in el[1]), 17, full, ragged)
            loss = full.item() / 17
        else:
            loss = seqmod.take(st, el, form)
        assert st.t == k + 1
        seqmod.check_invariants(st, form != "launches", tag)
        seqmod.check(tag, seqmod.state(st, loss, kind == "bpr"), want[k], f32[k])


# ------------------------------------------------------------------------------------------ 6. epochs
def state(st):
    return st.E0.cpu().numpy(), st.m.cpu().numpy(), st.v.cpu().numpy()


def compare(tag, loss_a, loss_b, st_a, st_b):
    loss_a, loss_b = np.asarray(loss_a, np.float64).ravel(), np.asarray(loss_b, np.float64).ravel()
    assert loss_a.shape == loss_b.shape and np.all(loss_b != 0)
    figs = (float((np.abs(loss_a - loss_b) / np.abs(loss_b)).max()),) + tuple(seqmod.rel_err(x, y) for x, y in zip(state(st_a), state(st_b)))
    print(f"{tag}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert st_a.t == st_b.t
    assert all(f <= b for f, b in zip(figs, EPOCH_BOUNDS)), (tag, figs, EPOCH_BOUNDS)


@pytest.mark.parametrize("L", [2, 3])
def test_frontier_epochs_equal_the_looped_one_call_steps(L):
    from spex_amd.trainer import BceDeviceSampler, BprDeviceSampler
    pairs = graph_b()[3]
    B, steps = 256, 5
    # BCE: the sampled epoch, the native epoch over the same draw, the looped one-call steps
    s = BceDeviceSampler(pairs, NB_U, NB_I, num_ng=1, seed=5, device=DEV)
    a, b, c = stepper_b(L, True), stepper_b(L, True), stepper_b(L, True)
    acc_a, acc_b, acc_c = (torch.zeros(2, 1, device=DEV) for _ in range(3))
    a.epoch_bce_sampled(s, 3, B, acc_a[0], acc_a[1], max_steps=steps)
    u, i, y = (x.clone() for x in s.draw(3))
    b.epoch_bce(u, i, y, B, acc_b[0], acc_b[1], max_steps=steps)
    for k in range(steps):
        c.step_bce(u[k * B:(k + 1) * B], i[k * B:(k + 1) * B], y[k * B:(k + 1) * B], loss_acc=acc_c[0], batch_rows_only=True)
    assert a.t == b.t == c.t == steps
    compare(f"sampled BCE epoch L={L}", acc_a[0].cpu().numpy(), acc_c[0].cpu().numpy(), a, c)
    compare(f"native BCE epoch L={L}", acc_b[0].cpu().numpy(), acc_c[0].cpu().numpy(), b, c)
    # exact BPR: the sampled epoch against the looped one-call steps; n = 700 triples = two full batches of 300 and a ragged one
    s = BprDeviceSampler(pairs, NB_U, NB_I, torch.device(DEV, torch.cuda.current_device()), seed=6, n=700)
    a, c = stepper_b(L, True), stepper_b(L, True)
    acc_a, acc_c = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
    a.epoch_bpr_sampled(s, 2, 300, acc_a[0], acc_a[1])
    u, p, ng = (x.clone() for x in s.draw(2))
    for k in range(3):
        sl = slice(k * 300, min((k + 1) * 300, 700))
        c.step_bpr_exact(u[sl], p[sl], ng[sl], loss_acc=acc_c[0 if k < 2 else 1], batch_rows_only=True)
    assert a.t == c.t == 3
    compare(f"sampled BPR epoch L={L}", acc_a.cpu().numpy(), acc_c.cpu().numpy(), a, c)
    b = stepper_b(L, True)
    acc_b = torch.zeros(2, 1, device=DEV)
    b.epoch_bpr(u, p, ng, 300, acc_b[0], acc_b[1])
    assert b.t == 3
    compare(f"native BPR epoch L={L}", acc_b.cpu().numpy(), acc_c.cpu().numpy(), b, c)


def test_train_epoch_drivers_take_a_frontier_stepper_as_they_are():
    """train_epoch / train_epochs (BCE sampler) and train_epoch_bpr (BPR sampler) on a frontier=True stepper, no new arguments: the
    state of the explicit sampled-epoch calls on a second frontier stepper, under the epoch criteria."""
    from spex_amd.trainer import BceDeviceSampler, BprDeviceSampler, train_epoch, train_epoch_bpr, train_epochs
    pairs = graph_b()[3]
    B, steps = 256, 4
    s = BceDeviceSampler(pairs, NB_U, NB_I, num_ng=1, seed=9, device=DEV)
    a, c = stepper_b(2, True), stepper_b(2, True)
    got = [train_epoch(a, s, batch_size=B, epoch=0, max_steps=steps).item()] + train_epochs(a, s, 2, batch_size=B, max_steps=steps, first_epoch=1)
    acc = torch.zeros(3, 2, device=DEV)
    for e in range(3):
        c.epoch_bce_sampled(s, e, B, acc[e, 0:1], acc[e, 1:2], max_steps=steps)
    assert a.t == c.t == 3 * steps
    compare("train_epoch(s) BCE", np.array(got) * B, acc[:, 0].cpu().numpy(), a, c)
    s = BprDeviceSampler(pairs, NB_U, NB_I, torch.device(DEV, torch.cuda.current_device()), seed=10, n=600)
    a, c = stepper_b(3, True), stepper_b(3, True)
    got = float(train_epoch_bpr(a, s, batch_size=300, epoch=1))
    acc = torch.zeros(2, 1, device=DEV)
    c.epoch_bpr_sampled(s, 1, 300, acc[0], acc[1])
    compare("train_epoch_bpr", [got * 300], acc[0].cpu().numpy(), a, c)

# ------------------------------------------------------------------------------------------ 7. refusals
def test_python_refusals():
    from spex_amd.trainer import LightGCNStepper
    g = handle(graph_b())
    E0 = t(table_b().copy())
    with pytest.raises(ValueError, match="not with deterministic=True"):
        LightGCNStepper(g, E0, NB_U, n_layers=3, deterministic=True, frontier=True)
    with pytest.raises(ValueError, match="not with gather_dtype"):
        LightGCNStepper(g, E0, NB_U, n_layers=3, gather_dtype=torch.bfloat16, frontier=True)
    with pytest.raises(ValueError, match="width of 64 and n_layers >= 2"):
        LightGCNStepper(g, torch.zeros(NB, 128, device=DEV), NB_U, n_layers=3, frontier=True)
    with pytest.raises(ValueError, match="width of 64 and n_layers >= 2"):
        LightGCNStepper(g, E0, NB_U, n_layers=1, frontier=True)
    plain = LightGCNStepper(g, E0, NB_U, n_layers=3)
    with pytest.raises(ValueError, match="only on a stepper built with frontier=True"):
        plain.frontier = True
    plain.frontier = False
    assert plain.frontier is False
    st = LightGCNStepper(g, E0, NB_U, n_layers=3, frontier=True)
    st.frontier = False
    st.frontier = True
    assert st.frontier is True
    with pytest.raises(ValueError, match="does not combine with edge dropout"):
        st.set_edge_dropout((1, torch.ones(len(graph_b()[1]), dtype=torch.uint8, device=DEV), 0.6, 0))
    _, (u, i, y) = batch_b("bce", 1, 7)
    acc = torch.zeros(2, 1, device=DEV)
    with pytest.raises(ValueError, match="does not combine with edge dropout"):
        st.epoch_bce(t(u), t(i), t(y), 7, acc[0], acc[1], keep_prob=0.6)
    with pytest.raises(ValueError, match="does not combine with edge dropout"):
        st.epoch_bpr(t(u), t(i), t(i), 7, acc[0], acc[1], keep_prob=0.6)
    st.bpr_backward = "dense"
    with pytest.raises(ValueError, match="SPEX_STEP_BPR_DENSE"):
        st.step_bpr_exact(t(u), t(i), t(i), loss_acc=acc[0], batch_rows_only=True)
    assert st.t == 0


def test_native_refusals():
    from spex_amd import _lib
    from spex_amd.graph import _stream
    from spex_amd.trainer import LightGCNStepper
    lib = _lib.load()
    g = handle(graph_b())
    _, (u, i, y) = batch_b("bce", 1, 7)
    u, i, y = t(u), t(i), t(y)
    acc = torch.zeros(1, device=DEV)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def status(st, flags, bpr=False, L=None, d=None, drop_list=False):
        desc = st._prepare_desc(7, 3 if bpr else 2)
        desc.flags = flags
        desc.L = st.L if L is None else L
        desc.d = 64 if d is None else d
        saved = desc.frontier_list
        if drop_list:
            desc.frontier_list = None
        name = "spex_lightgcn_step_bpr_adam_f32" if bpr else "spex_lightgcn_step_bce_f32"
        rc = getattr(lib, name)(ctypes.byref(desc), vp(u), vp(i), vp(i) if bpr else vp(y), 7, vp(acc), _stream(None))
        desc.frontier_list, desc.L, desc.d = saved, st.L, 64
        return rc, lib.spex_last_error().decode()

    st = LightGCNStepper(g, t(table_b().copy()), NB_U, n_layers=3, frontier=True)
    F = _lib.STEP_FRONTIER
    for bpr in (False, True):
        assert status(st, F | _lib.STEP_DETERMINISTIC, bpr)[0] == -1 and "SPEX_STEP_DETERMINISTIC" in lib.spex_last_error().decode()
        rc, msg = status(st, F | _lib.STEP_BF16_GATHER, bpr)
        assert rc in (-1, -4) and rc != 0                    # (the bf16 check itself may speak first: E0_16 is NULL here)
        rc, msg = status(st, F, bpr, L=1)
        assert rc == -1 and "L >= 2" in msg
        rc, msg = status(st, F, bpr, d=128)
        assert rc in (-1, -4) and ("d == 64" in msg or "d=128" in msg or "d = 128" in msg), msg
        rc, msg = status(st, F, bpr, drop_list=True)
        assert rc == -1 and "frontier_list" in msg
    rc, msg = status(st, F | _lib.STEP_BPR_DENSE, True)
    assert rc == -1 and "SPEX_STEP_BPR_DENSE" in msg
    rc, msg = status(st, F | _lib.STEP_WIDE, True)
    assert rc == -4 and "d == 64" in msg
    # edge dropout on the handles
    keep = torch.ones(len(graph_b()[1]), dtype=torch.uint8, device=DEV)
    g.set_edge_mask(1, keep, 0.6, 0)
    try:
        rc, msg = status(st, F)
        assert rc == -1 and "edge dropout" in msg
    finally:
        g.set_edge_mask(0)
    assert st.t == 0 and not st.E0.isnan().any() and torch.equal(st.E0, t(table_b()))
