"""The one-call BPR step (spex_lightgcn_step_bpr_f32) on its snapshot schedule: all L whole-graph launches plain, the layer-1
launch setting aside the E^0 rows of the batch's <= 3 T slots in a tail of extra workgroups, the BPR kernel forming
(((E^0 + E^1) + E^2) + E^3) / (L + 1) from that compact buffer and the three layer tables.

Reference form in every test: SpexGraph.propagate followed by ops.bpr_sgd_step(..., grouped=False) on a copy of the table
(the form of test_one_call_bpr_step_equals_propagate_then_bpr).  The propagated rows are bit-identical in both forms; the
updates land with float atomics, so the updated table is bit-identical wherever every element receives at most one atomic (a
batch of distinct rows) and agrees to the existing test's tolerances otherwise: loss 1e-6 relative, table rel_err <= 2e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = 0.05


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
    """Epinion2: one handle, the initial table and the user-row count, shared by the tests of this module (never modified)."""
    from spex_amd.datasets import epinion2_tables
    from spex_amd.graph import lightgcn_norm_adj
    tr = epinion2["train"]
    csr = lightgcn_norm_adj(tr[:, 0], tr[:, 1], 3185, 12407)
    uw, iw = epinion2_tables(3186, 12407)
    return G(*csr), t(np.concatenate([uw, iw])), 3186


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
    """One step of the stepper; its loss sum (the stepper accumulates)."""
    before = st.loss_acc.item()
    return st.step_bpr_sgd(u, p, n).item() - before


def distinct_batch(perm_u, perm_i, T, u0=0, i0=0):
    """T triples whose users are all distinct and whose 2 T items are all distinct: every table element gets <= 1 atomic."""
    u = perm_u[u0:u0 + T]
    it = perm_i[i0:i0 + 2 * T]
    assert len(set(u)) == T and len(set(it)) == 2 * T
    return t(u), t(it[:T]), t(it[T:])


@pytest.mark.parametrize("L", [1, 2, 3])
def test_distinct_rows_bit_equal_to_propagate_then_bpr(epi, L):
    """Bit equality where it is decidable: T = 200 triples of distinct rows on Epinion2 — the updated table torch.equal to the
    reference form's, the loss sums (per-block partials in both forms) within 1e-6 relative.  sum1 (light_out) holds E^1."""
    g, E0, n_u = epi
    rng = np.random.default_rng(50 + L)
    u, p, n = distinct_batch(rng.permutation(3185), rng.permutation(12407), 200)
    st = stepper(g, E0, n_u, L)
    loss_new = one_step(st, u, p, n)
    W, loss_ref = reference_step(g, E0, n_u, L, u, p, n)
    print("L", L, "loss", loss_new, loss_ref, "table equal", torch.equal(st.E0, W))
    assert torch.equal(st.E0, W)
    assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)
    assert not torch.equal(W, E0)
    assert torch.equal(st.light_out, g.spmm(E0))                         # the documented content of sum1 on this schedule: E^1


def test_snapshot_is_fresh_every_step(epi):
    """Three consecutive steps on one stepper with three different distinct-row batches that overlap from step to step (50 users;
    100 items that were negatives become positives), each against its own reference iteration: bit-equal after every step.  A
    snapshot read from stale rows (the previous step's buffer) or from rows the step already updated fails here."""
    g, E0, n_u = epi
    rng = np.random.default_rng(7)
    pu, pi = rng.permutation(3185), rng.permutation(12407)
    st = stepper(g, E0, n_u, 3)
    W = E0
    for k in range(3):
        u, p, n = distinct_batch(pu, pi, 200, u0=150 * k, i0=300 * k)
        loss_new = one_step(st, u, p, n)
        W, loss_ref = reference_step(g, W, n_u, 3, u, p, n)
        print("step", k, "loss", loss_new, loss_ref, "table equal", torch.equal(st.E0, W))
        assert torch.equal(st.E0, W), k
        assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)


@pytest.fixture(scope="module")
def tiny(G):
    """~100 nodes (41 user rows, 60 item rows): one workgroup of the task table."""
    from spex_amd.datasets import synthetic_interactions
    from spex_amd.graph import lightgcn_norm_adj
    u, i = synthetic_interactions(40, 60, 400, seed=3)
    csr = lightgcn_norm_adj(u.numpy(), i.numpy(), 40, 60)
    rng = np.random.default_rng(3)
    return G(*csr), t((0.1 * rng.normal(size=(101, 64))).astype(np.float32)), 41


@pytest.mark.parametrize("T", [0, 1, 21, 22, 341, 342, 5000])
def test_tail_edges_on_a_one_workgroup_graph(tiny, T):
    """3 T on both sides of 64 (one wave of the tail) and of 1 024 (one workgroup of it), and a tail of 15 workgroups behind a
    table of one; duplicate rows and a hot user (u[:64] = u[0]).  T = 342 carries four triples with an out-of-range index (one
    in each array, below and above the range): they are skipped, their snapshot slots never gather, and the rows only they
    name stay bit-unchanged.  Tolerances of the existing test."""
    g, E0, n_u = tiny
    rng = np.random.default_rng(100 + T)
    # rows 38, 39 (users) and 58, 59 (items) are named by the out-of-range triples only
    u, p, n = rng.integers(0, 38, max(T, 1)), rng.integers(0, 58, max(T, 1)), rng.integers(0, 58, max(T, 1))
    u[:64] = u[0]
    if T == 342:
        u[5], p[5], n[5] = 38, 58, 10 ** 12
        u[70], p[70], n[70] = -1, 59, 58
        u[200], p[200], n[200] = 39, 60, 59
        u[341], p[341], n[341] = n_u, 58, 59
    ud, pd_, nd = t(u)[:T], t(p)[:T], t(n)[:T]                              # (T = 0: empty views of live buffers)
    st = stepper(g, E0, n_u, 3)
    loss_new = one_step(st, ud, pd_, nd)
    W, loss_ref = reference_step(g, E0, n_u, 3, ud, pd_, nd)
    err = rel_err(st.E0.cpu().numpy(), W.cpu().numpy())
    print("T", T, "loss", loss_new, loss_ref, "rel_err", err)
    assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)
    assert err <= 2e-6
    if T == 0:
        assert torch.equal(st.E0, E0) and loss_new == 0.0
    if T == 342:
        rows = [38, 39, n_u + 58, n_u + 59]
        assert torch.equal(st.E0[rows], E0[rows])
        assert not torch.equal(st.E0[:38], E0[:38])


def test_hub_rows_five_steps_on_one_handle(G):
    """A graph with rows beyond 1 024 entries (hub segments lead the task table and fold through tickets that count arrivals per
    launch): five steps on one handle, every step against the reference form.  Guards the ticket counters and every use of the
    grid size in a launch that is longer than its task table."""
    from spex_amd.datasets import synthetic_interactions
    from spex_amd.graph import lightgcn_norm_adj
    n_users, n_items = 3000, 1000
    ui, ii = synthetic_interactions(n_users, n_items, 60000, seed=5)
    csr = lightgcn_norm_adj(ui.numpy(), ii.numpy(), n_users, n_items)
    assert np.diff(csr[0]).max() > 1024
    g = G(*csr)
    n_u = n_users + 1
    rng = np.random.default_rng(5)
    W = t((0.1 * rng.normal(size=(n_u + n_items, 64))).astype(np.float32))
    st = stepper(g, W, n_u, 3)
    for k in range(5):
        u, p, n = (t(rng.integers(0, hi, 512)) for hi in (n_users, n_items, n_items))
        loss_new = one_step(st, u, p, n)
        W, loss_ref = reference_step(g, W, n_u, 3, u, p, n)
        err = rel_err(st.E0.cpu().numpy(), W.cpu().numpy())
        print("step", k, "loss", loss_new, loss_ref, "rel_err", err)
        assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref), k
        assert err <= 2e-6, k
        # (both forms continue from the reference table, so that a step's error is its own)
        st.E0.copy_(W)


def test_fallback_schedule_gives_the_same_table(epi, monkeypatch):
    """The rule: the snapshot tail adds ceil(3 T / 1024) workgroups to the layer-1 launch; if the task table's launch fits one
    dispatch round (<= 512 workgroups) and would not fit it with the tail, the step keeps the old schedule (layer 1 in the
    running-sum form, sum1 = E^0 + E^1, three tables).  Epinion2's table is 496 workgroups, so T = 6 000 (18 tail workgroups)
    falls back.  The batch is 200 distinct-row triples followed by 5 800 the BPR kernel skips (user index -1), so the result is
    decidable bit for bit: the same table as the reference form, and as the snapshot schedule forced on the same batch
    (SPEX_STEP_SNAPSHOT=1; =0 forces the old schedule at any T).  Which schedule ran is read from sum1."""
    g, E0, n_u = epi
    rng = np.random.default_rng(9)
    u, p, n = distinct_batch(rng.permutation(3185), rng.permutation(12407), 200)
    pad = torch.full((5800,), -1, dtype=torch.int64, device=DEV)
    zero = torch.zeros(5800, dtype=torch.int64, device=DEV)
    u6, p6, n6 = torch.cat([u, pad]), torch.cat([p, zero]), torch.cat([n, zero])
    E1 = g.spmm(E0).clone()
    W, loss_ref = reference_step(g, E0, n_u, 3, u6, p6, n6)

    old = stepper(g, E0, n_u, 3)
    loss_old = one_step(old, u6, p6, n6)
    assert torch.equal(old.light_out, E0 + E1), "T = 6000 on Epinion2 did not take the fallback schedule"
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", "1")
    new = stepper(g, E0, n_u, 3)
    loss_new = one_step(new, u6, p6, n6)
    assert torch.equal(new.light_out, E1), "SPEX_STEP_SNAPSHOT=1 did not take the snapshot schedule"
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", "0")
    forced = stepper(g, E0, n_u, 3)
    one_step(forced, u, p, n)
    assert torch.equal(forced.light_out, E0 + E1), "SPEX_STEP_SNAPSHOT=0 did not take the fallback schedule"
    monkeypatch.delenv("SPEX_STEP_SNAPSHOT")
    print("loss", loss_old, loss_new, loss_ref)
    assert torch.equal(old.E0, W) and torch.equal(new.E0, W) and torch.equal(old.E0, new.E0)
    assert not torch.equal(W, E0)
    assert abs(loss_old - loss_ref) <= 1e-6 * abs(loss_ref) and abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)
