"""The one-call BPR step (spex_lightgcn_step_bpr_f32) with its LAST layer inside the BPR launch (bpr_fused_last_kernel): L - 1
whole-graph plain launches, then one launch that gathers layer L at the triples' <= 3 T slot rows — 4 consecutive triples per
16-wave workgroup, one 64-entry segment per wave task, segment sums combined through LDS in segment order — and runs the BPR update;
the loss of 16 consecutive triples (four workgroups) meets in one cell of the handle and is added to the accumulator once.

Reference form in every test, as in test_gpu_bpr_step_snapshot.py: SpexGraph.propagate followed by ops.bpr_sgd_step(...,
grouped=False) on a copy of the table.  The rows the fused launch forms are the whole-graph launch's bit for bit, so the updated
table is torch.equal wherever every element receives at most one atomic (a batch of distinct rows) and agrees to that file's
tolerances otherwise: loss 1e-6 relative, table rel_err <= 2e-6.

Which form ran is read from the stepper's workspace: it is filled with a sentinel before the step, and on the snapshot schedule
(every test here runs on it: light_out == E^1 is asserted where it matters) the half that receives the last layer — ws_fwd[1] for
L = 3, ws_fwd[0] for L = 2 — stays the sentinel exactly when the fused form ran."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = 0.05
SENTINEL = -12345.0


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


@pytest.fixture(scope="module")
def epi(G, golden, epinion2):
    """Epinion2: one handle, the initial table, the user-row count and E^1, shared by the tests of this module (never modified)."""
    from spex_amd.datasets import epinion2_tables
    from spex_amd.graph import lightgcn_norm_adj
    tr = epinion2["train"]
    csr = lightgcn_norm_adj(tr[:, 0], tr[:, 1], 3185, 12407)
    uw, iw = epinion2_tables(3186, 12407)
    g, E0 = G(*csr), t(np.concatenate([uw, iw]))
    return g, E0, 3186, g.spmm(E0).clone()


def reference_step(g, E, n_u, L, u, p, n):
    """propagate, then the atomic BPR-SGD kernel on a copy of E: (updated table, loss sum)."""
    from spex_amd import ops
    lo = g.propagate(E, L)
    W = E.clone()
    loss = ops.bpr_sgd_step(lo[:n_u], lo[n_u:], W[:n_u], W[n_u:], u, p, n, LR, 0.0, grouped=False).item()
    return W, loss


def stepper(g, E, n_u, L):
    from spex_amd.trainer import LightGCNStepper
    return LightGCNStepper(g, E.clone(), n_u, n_layers=L, lr=LR)


def one_step(st, u, p, n):
    """One step of the stepper behind a sentinel-filled workspace: (its loss sum, whether the fused form ran — None for L = 1,
    whose schedules write neither half, and for an empty batch)."""
    st.ws_fwd.fill_(SENTINEL)
    before = st.loss_acc.item()
    loss = st.step_bpr_sgd(u, p, n).item() - before
    if u.numel() == 0:                       # (an empty batch names no rows: always the whole-graph launches)
        return loss, None
    if st.L == 1:
        assert bool((st.ws_fwd == SENTINEL).all())
        return loss, None
    half = st.ws_fwd[1 if st.L == 3 else 0] == SENTINEL
    assert bool(half.all()) or not bool(half.any()), "the last layer's half of ws is partly written"
    return loss, bool(half.all())


def distinct_batch(perm_u, perm_i, T, u0=0, i0=0):
    """T triples whose users are all distinct and whose 2 T items are all distinct: every table element gets <= 1 atomic."""
    u = perm_u[u0:u0 + T]
    it = perm_i[i0:i0 + 2 * T]
    assert len(set(u)) == T and len(set(it)) == 2 * T
    return t(u), t(it[:T]), t(it[T:])


@pytest.mark.parametrize("L", [2, 3])
def test_distinct_rows_bit_equal_on_epinion2(epi, L, monkeypatch):
    """T = 200 triples of distinct rows, three consecutive batches on one stepper that overlap from step to step (as in
    test_snapshot_is_fresh_every_step): after every step the fused form's table is torch.equal to the reference form's and to the
    whole-graph form's (SPEX_STEP_FUSED_LAST=0) continued from the same table; light_out holds E^1 of the step's input table."""
    g, E0, n_u, _ = epi
    rng = np.random.default_rng(60 + L)
    pu, pi = rng.permutation(3185), rng.permutation(12407)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    st = stepper(g, E0, n_u, L)
    W = E0
    for k in range(3):
        u, p, n = distinct_batch(pu, pi, 200, u0=150 * k, i0=300 * k)
        monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "0")
        old = stepper(g, W, n_u, L)
        loss_old, fused_old = one_step(old, u, p, n)
        monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
        loss_new, fused_new = one_step(st, u, p, n)
        E1 = g.spmm(W).clone()
        W, loss_ref = reference_step(g, W, n_u, L, u, p, n)
        print("L", L, "step", k, "loss", loss_new, loss_old, loss_ref, "table equal", torch.equal(st.E0, W), torch.equal(st.E0, old.E0))
        assert fused_new is True and fused_old is False
        assert torch.equal(st.E0, W), k
        assert torch.equal(st.E0, old.E0), k
        assert torch.equal(st.light_out, E1), k
        assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)
    assert not torch.equal(W, E0)


EDGE_DEGREES = [0, 1, 16, 17, 63, 64, 65, 128, 1000, 1024, 1010, 970, 1024, 990]
EDGE_ITEMS = 1100


@pytest.fixture(scope="module")
def edges(G):
    """14 users with exactly EDGE_DEGREES stored entries (distinct items each), 1 100 items of which the last has none."""
    from spex_amd.graph import lightgcn_norm_adj
    rng = np.random.default_rng(17)
    uu, ii = [], []
    for k, deg in enumerate(EDGE_DEGREES):
        uu += [k] * deg
        ii += list(rng.choice(EDGE_ITEMS - 1, deg, replace=False))
    n_users = len(EDGE_DEGREES)
    csr = lightgcn_norm_adj(np.array(uu), np.array(ii), n_users - 1, EDGE_ITEMS)
    assert list(np.diff(csr[0])[:n_users]) == EDGE_DEGREES and np.diff(csr[0])[n_users + EDGE_ITEMS - 1] == 0
    return G(*csr), t((0.1 * rng.normal(size=(n_users + EDGE_ITEMS, 64))).astype(np.float32)), n_users


@pytest.mark.parametrize("L", [2, 3])
def test_row_length_edges_bit_equal(edges, L, monkeypatch):
    """User rows of 0, 1, 16, 17, 63, 64, 65, 128, 1 000 and 1 024 entries and an item row of 0, every one named once by a batch of
    distinct rows.  The first workgroup's four triples name the users of 1 024, 1 010, 1 024 and 990 entries: 64 user segments and
    8 item segments meet behind its 16 waves (five passes).  Bit-equal to the reference form and to the whole-graph form."""
    g, E0, n_u = edges
    order = [9, 10, 12, 13, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11]
    items = np.random.default_rng(18).permutation(EDGE_ITEMS - 1)[:2 * len(order) - 1]
    items = np.concatenate([items[:9], [EDGE_ITEMS - 1], items[9:]])           # the item without entries: triple 9's positive
    u, p, n = t(np.array(order)), t(items[:len(order)]), t(items[len(order):])
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    new = stepper(g, E0, n_u, L)
    loss_new, fused_new = one_step(new, u, p, n)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "0")
    old = stepper(g, E0, n_u, L)
    loss_old, fused_old = one_step(old, u, p, n)
    W, loss_ref = reference_step(g, E0, n_u, L, u, p, n)
    print("L", L, "loss", loss_new, loss_old, loss_ref, "table equal", torch.equal(new.E0, W), torch.equal(new.E0, old.E0))
    assert fused_new is True and fused_old is False
    assert torch.equal(new.E0, W) and torch.equal(new.E0, old.E0)
    assert not torch.equal(W, E0)
    assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)


@pytest.fixture(scope="module")
def tiny(G):
    """~100 nodes (41 user rows, 60 item rows): the graph of test_gpu_bpr_step_snapshot.py."""
    from spex_amd.datasets import synthetic_interactions
    from spex_amd.graph import lightgcn_norm_adj
    u, i = synthetic_interactions(40, 60, 400, seed=3)
    csr = lightgcn_norm_adj(u.numpy(), i.numpy(), 40, 60)
    rng = np.random.default_rng(3)
    return G(*csr), t((0.1 * rng.normal(size=(101, 64))).astype(np.float32)), 41


@pytest.mark.parametrize("T", [0, 1, 3, 4, 5, 341])
def test_group_edges_on_the_tiny_graph(tiny, T, monkeypatch):
    """T on both sides of one workgroup's four triples and a last workgroup of one (341 = 85 * 4 + 1); duplicate rows and a hot
    user.  T = 341 carries six triples with an out-of-range index, all four kinds (a user below / above the range, an item below /
    above it): triples 4..7 fill one workgroup, 201 and 203 share theirs with two valid ones.  They are skipped and the rows only
    they name stay bit-unchanged.  Tolerances of test_gpu_bpr_step_snapshot.py."""
    g, E0, n_u = tiny
    rng = np.random.default_rng(200 + T)
    # rows 38, 39 (users) and 58, 59 (items) are named by the out-of-range triples only
    u, p, n = rng.integers(0, 38, max(T, 1)), rng.integers(0, 58, max(T, 1)), rng.integers(0, 58, max(T, 1))
    u[:64] = u[0]
    if T == 341:
        u[4], p[4], n[4] = 38, 58, 10 ** 12
        u[5], p[5], n[5] = -1, 59, 58
        u[6], p[6], n[6] = 39, 60, 59
        u[7], p[7], n[7] = n_u, 58, 59
        u[201], p[201], n[201] = 38, 59, -5
        u[203], p[203], n[203] = 39, -1, 58
    ud, pd_, nd = t(u)[:T], t(p)[:T], t(n)[:T]                              # (T = 0: empty views of live buffers)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    st = stepper(g, E0, n_u, 3)
    loss_new, fused = one_step(st, ud, pd_, nd)
    W, loss_ref = reference_step(g, E0, n_u, 3, ud, pd_, nd)
    err = rel_err(st.E0.cpu().numpy(), W.cpu().numpy())
    print("T", T, "loss", loss_new, loss_ref, "rel_err", err)
    assert fused is (None if T == 0 else True)
    assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)
    assert err <= 2e-6
    if T == 0:
        assert torch.equal(st.E0, E0) and loss_new == 0.0
    else:
        assert not torch.equal(st.E0, E0)
    if T == 341:
        rows = [38, 39, n_u + 58, n_u + 59]
        assert torch.equal(st.E0[rows], E0[rows])


def test_one_layer_keeps_the_whole_graph_schedule(epi, monkeypatch):
    """L = 1: the last layer gathers from E^0, which the BPR launch updates, so SPEX_STEP_FUSED_LAST=1 changes nothing.  (Neither
    schedule of L = 1 writes ws — the sentinel cannot tell them apart; the bits can: a batch of distinct rows, torch.equal.)"""
    g, E0, n_u, E1 = epi
    rng = np.random.default_rng(71)
    u, p, n = distinct_batch(rng.permutation(3185), rng.permutation(12407), 200)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    st = stepper(g, E0, n_u, 1)
    loss_new, fused = one_step(st, u, p, n)
    W, loss_ref = reference_step(g, E0, n_u, 1, u, p, n)
    assert fused is None
    assert torch.equal(st.E0, W) and torch.equal(st.light_out, E1)
    assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)


def test_hub_rows_keep_the_whole_graph_schedule(G, monkeypatch):
    """A graph with a row beyond 1 024 entries (the chunk kernel sums it by groups): the whole-graph form even with
    SPEX_STEP_FUSED_LAST=1 — read from the sentinel on the snapshot schedule — and the result within the tolerances."""
    from spex_amd.datasets import synthetic_interactions
    from spex_amd.graph import lightgcn_norm_adj
    n_users, n_items = 3000, 1000
    ui, ii = synthetic_interactions(n_users, n_items, 60000, seed=5)
    csr = lightgcn_norm_adj(ui.numpy(), ii.numpy(), n_users, n_items)
    assert np.diff(csr[0]).max() > 1024
    g, n_u = G(*csr), n_users + 1
    rng = np.random.default_rng(6)
    E0 = t((0.1 * rng.normal(size=(n_u + n_items, 64))).astype(np.float32))
    u, p, n = (t(rng.integers(0, hi, 64)) for hi in (n_users, n_items, n_items))
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", "1")
    st = stepper(g, E0, n_u, 3)
    loss_new, fused = one_step(st, u, p, n)
    W, loss_ref = reference_step(g, E0, n_u, 3, u, p, n)
    err = rel_err(st.E0.cpu().numpy(), W.cpu().numpy())
    print("loss", loss_new, loss_ref, "rel_err", err)
    assert fused is False
    assert torch.equal(st.light_out, g.spmm(E0))
    assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref) and err <= 2e-6


# The rule of step_fuses_last (spex_amd/csrc/spmm.hip): fused while 6 T <= n_rows.  Epinion2 has 15 593 rows: T <= 2 598.
T_BELOW, T_ABOVE = 2048, 3072


@pytest.mark.parametrize("T", [T_BELOW, T_ABOVE])
def test_schedule_rule_and_both_forms_agree(epi, T, monkeypatch):
    """By default T = 2 048 takes the fused form and T = 3 072 the whole-graph form on Epinion2; forced either way, both forms give
    the reference form's table.  The batch is 200 distinct-row triples spread over the batch (every 8th triple up to 1 600), the
    rest skipped triples (user index -1), so the result is decidable bit for bit; the loss within 1e-6 relative."""
    g, E0, n_u, E1 = epi
    rng = np.random.default_rng(80)
    du, dp, dn = distinct_batch(rng.permutation(3185), rng.permutation(12407), 200)
    u = torch.full((T,), -1, dtype=torch.int64, device=DEV)
    p, n = torch.zeros_like(u), torch.zeros_like(u)
    u[0:1600:8], p[0:1600:8], n[0:1600:8] = du, dp, dn
    W, loss_ref = reference_step(g, E0, n_u, 3, u, p, n)
    monkeypatch.delenv("SPEX_STEP_FUSED_LAST", raising=False)
    by_rule = stepper(g, E0, n_u, 3)
    loss_rule, fused_rule = one_step(by_rule, u, p, n)
    assert torch.equal(by_rule.light_out, E1), "not on the snapshot schedule"
    assert fused_rule is (T == T_BELOW)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "0" if fused_rule else "1")
    other = stepper(g, E0, n_u, 3)
    loss_other, fused_other = one_step(other, u, p, n)
    assert fused_other is (not fused_rule)
    print("T", T, "loss", loss_rule, loss_other, loss_ref)
    assert torch.equal(by_rule.E0, W) and torch.equal(other.E0, W)
    assert not torch.equal(W, E0)
    assert abs(loss_rule - loss_ref) <= 1e-6 * abs(loss_ref) and abs(loss_other - loss_ref) <= 1e-6 * abs(loss_ref)
