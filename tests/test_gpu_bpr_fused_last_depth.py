"""Phase A of bpr_fused_last_kernel (score.hip) as a software pipeline: a triple's three indices in one round trip, an item's (col, val)
requested one item ahead, and however many 16-entry chunks of row gathers the kernel keeps in flight.  Only the position of the loads
and waits may differ from the plain loop, so every row the launch forms is still the whole-graph launch's row bit for bit.  The
cases are chosen by what such a pipeline can get wrong, without knowing its depth:

  * every remainder of a row length against any in-flight depth (degrees 0 ... 130);
  * waves that take 1, 2, 3 and 4 items (S = 15 ... 49 segments behind a workgroup's 16 waves), consecutive items of one wave shaped
    (64 entries, 1 entry) and (1 entry, 64 entries) — what a prefetched item must not inherit from its predecessor —, an empty row
    between two long ones;
  * a last workgroup of one valid triple beside out-of-range ones, on the two-pass path;
  * duplicate rows (the atomics' order is free: tolerances of test_gpu_bpr_step_snapshot.py);
  * three consecutive steps of the bench's own 2 048 triples on Epinion2.

Every case runs L = 2 and 3 on both schedules of the step (SPEX_STEP_SNAPSHOT=0 / 1: the two instantiations of the kernel) and
compares the fused form (SPEX_STEP_FUSED_LAST=1) with the forced whole-graph form (=0) and with the reference form (SpexGraph.propagate,
then ops.bpr_sgd_step(..., grouped=False) on a copy of the table).  On batches of distinct rows every table element receives at most
one atomic: the tables are torch.equal; the loss agrees within 1e-6 relative.  With duplicates: table 2e-6 relative, loss 1e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = 0.05
SENTINEL = -12345.0
FORMS = [(L, snap) for L in (2, 3) for snap in ("0", "1")]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def reference_step(g, E, n_u, L, u, p, n):
    """propagate, then the atomic BPR-SGD kernel on a copy of E: (updated table, loss sum)."""
    from spex_amd import ops
    lo = g.propagate(E, L)
    W = E.clone()
    loss = ops.bpr_sgd_step(lo[:n_u], lo[n_u:], W[:n_u], W[n_u:], u, p, n, LR, 0.0, grouped=False).item()
    return W, loss


def forced_step(monkeypatch, g, E, n_u, L, snap, fused, u, p, n):
    """One step of a fresh stepper on a copy of E with both switches forced: (updated table, loss sum).  On the snapshot schedule the
    half of the workspace that would receive the last layer tells which form ran (test_gpu_bpr_step_fused_last.py): it is checked."""
    from spex_amd.trainer import LightGCNStepper
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", snap)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1" if fused else "0")
    st = LightGCNStepper(g, E.clone(), n_u, n_layers=L, lr=LR)
    st.ws_fwd.fill_(SENTINEL)
    before = st.loss_acc.item()
    loss = st.step_bpr_sgd(u, p, n).item() - before
    if snap == "1":
        half = st.ws_fwd[1 if L == 3 else 0] == SENTINEL
        assert bool(half.all()) if fused else not bool(half.any()), "the other form ran"
    return st.E0, loss


def check_three_forms(monkeypatch, g, E0, n_u, L, snap, u, p, n, exact, unchanged_rows=()):
    new, loss_new = forced_step(monkeypatch, g, E0, n_u, L, snap, True, u, p, n)
    old, loss_old = forced_step(monkeypatch, g, E0, n_u, L, snap, False, u, p, n)
    W, loss_ref = reference_step(g, E0, n_u, L, u, p, n)
    e_old, e_ref = rel_err(new.cpu().numpy(), old.cpu().numpy()), rel_err(new.cpu().numpy(), W.cpu().numpy())
    print("L", L, "snapshot", snap, "loss", loss_new, loss_old, loss_ref, "rel_err vs whole-graph", e_old, "vs reference", e_ref,
          "equal", torch.equal(new, old), torch.equal(new, W))
    assert not torch.equal(W, E0)
    if exact:
        assert torch.equal(new, old) and torch.equal(new, W)
    else:
        assert e_old <= 2e-6 and e_ref <= 2e-6
    assert abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref) and abs(loss_new - loss_old) <= 1e-6 * abs(loss_old)
    for r in unchanged_rows:
        assert torch.equal(new[r], E0[r])


# ---- every chunk remainder -------------------------------------------------------------------------------------------------------

REM_USERS, REM_ITEMS = 131, 300


@pytest.fixture(scope="module")
def remainders():
    """User k has exactly k stored entries (k = 0 ... 130, distinct items each) over 300 items."""
    from spex_amd.graph import SpexGraph, lightgcn_norm_adj
    rng = np.random.default_rng(31)
    uu, ii = [], []
    for k in range(REM_USERS):
        uu += [k] * k
        ii += list(rng.choice(REM_ITEMS, k, replace=False))
    csr = lightgcn_norm_adj(np.array(uu), np.array(ii), REM_USERS - 1, REM_ITEMS)
    assert list(np.diff(csr[0])[:REM_USERS]) == list(range(REM_USERS))
    return SpexGraph(*csr), t((0.1 * rng.normal(size=(REM_USERS + REM_ITEMS, 64))).astype(np.float32)), REM_USERS


@pytest.mark.parametrize("L,snap", FORMS)
def test_every_row_length_to_130(remainders, L, snap, monkeypatch):
    """Users of 0, 1, ..., 130 entries named in order by one batch of distinct rows (131 triples, 262 distinct items): each remainder
    of a row length modulo any number of 16-entry chunks in flight, one- and two- and three-segment rows side by side."""
    g, E0, n_u = remainders
    items = np.random.default_rng(32).permutation(REM_ITEMS)[:2 * REM_USERS]
    u, p, n = t(np.arange(REM_USERS)), t(items[:REM_USERS]), t(items[REM_USERS:])
    check_three_forms(monkeypatch, g, E0, n_u, L, snap, u, p, n, exact=True)


# ---- items per wave --------------------------------------------------------------------------------------------------------------

COMMON, N_ITEMS = 1500, 1600         # items 0 .. 1499 are drawn by the users' rows; 1500 .. 1599 get entries only where a user is given one
S_TARGETS = [15, 16, 17, 31, 32, 33, 47, 48, 49]
REMS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
N_FILL = 130                         # users of one entry, all on item LONG_ITEM: an item row of three segments
LONG_ITEM, ONE_A, ONE_B = 1500, 1501, 1502     # ONE_*: items of exactly one entry;  1510 .. 1599: items without entries


class Waves:
    """The graph of the items-per-wave cases.  Workgroup specs are lists of four (user degree, positive, negative) with the items given as
    'c' (a fresh item of 1 .. 64 entries: one segment), 'e' (a fresh item without entries) or an item index."""

    def __init__(self):
        from spex_amd.graph import SpexGraph, lightgcn_norm_adj
        rng = np.random.default_rng(41)
        specs = []
        for k, S in enumerate(S_TARGETS):                # eight one-segment items + four users of S - 8 segments in all
            left, segs = S - 8, []
            for j in range(4):
                segs.append(min(16, left - (3 - j)))
                left -= segs[-1]
            specs.append([(64 * (s - 1) + REMS[(4 * k + j) % len(REMS)], "c", "c") for j, s in enumerate(segs)])
        # (64 entries, 1 entry): segments 0 .. 15 are the 1 024-entry user's, segment 16 the one-entry item's: wave 0 takes both
        specs.append([(1024, ONE_A, "c"), (65, "c", "c"), (1, "c", "c"), (40, "c", "c")])
        # (1 entry, 64 entries): segment 0 is the one-entry user's, 1 and 2 the items', 3 .. 18 the 1 024-entry user's
        specs.append([(1, "c", "c"), (1024, "c", ONE_B), (130, "c", "c"), (64, "c", "c")])
        # an empty row between two long ones: 1 000 entries, none, 130; then empty rows at both ends
        specs.append([(1000, "e", LONG_ITEM), (0, "c", "e"), (700, "e", "e"), (17, "c", "c")])
        self.specs = specs
        degs = [d for wg in specs for d, _, _ in wg]
        uu, ii = [], []
        for k, d in enumerate(degs):
            extra = [x for x in specs[k // 4][k % 4][1:] if x in (ONE_A, ONE_B)]
            uu += [k] * d
            ii += extra + list(rng.choice(COMMON, d - len(extra), replace=False))
        n_users = len(degs) + N_FILL
        uu += list(range(len(degs), n_users))
        ii += [LONG_ITEM] * N_FILL
        csr = lightgcn_norm_adj(np.array(uu), np.array(ii), n_users - 1, N_ITEMS)
        self.deg = np.diff(csr[0])
        assert list(self.deg[:len(degs)]) == degs and self.deg.max() <= 1024
        item_deg = self.deg[n_users:]
        assert item_deg[ONE_A] == 1 and item_deg[ONE_B] == 1 and item_deg[LONG_ITEM] == N_FILL and not item_deg[1510:].any()
        fresh_c = iter(rng.permutation(np.flatnonzero((item_deg[:COMMON] >= 1) & (item_deg[:COMMON] <= 64))))
        fresh_e = iter(range(1510, N_ITEMS))
        pick = lambda x: int(next(fresh_c)) if x == "c" else int(next(fresh_e)) if x == "e" else x
        self.u = np.arange(len(degs))
        self.p = np.array([pick(x) for wg in specs for _, x, _ in wg])
        self.n = np.array([pick(x) for wg in specs for _, _, x in wg])
        self.n_u = n_users
        self.g = SpexGraph(*csr)
        self.E0 = t((0.1 * rng.normal(size=(n_users + N_ITEMS, 64))).astype(np.float32))

    def segments(self, u, p, n):
        """segments behind each 4-triple workgroup, rows cut the way the kernel cuts them"""
        d = np.stack([self.deg[u], self.deg[self.n_u + p], self.deg[self.n_u + n]], 1)
        return list(((d + 63) // 64).reshape(-1, 12).sum(1))


@pytest.fixture(scope="module")
def waves():
    return Waves()


@pytest.mark.parametrize("L,snap", FORMS)
def test_one_to_four_items_per_wave(waves, L, snap, monkeypatch):
    """Twelve workgroups of distinct rows: S = 15, 16, 17 (wave 0: one, one, two items), 31, 32, 33 (two, two, three), 47, 48, 49 (three,
    three, four: one more than a pipeline of depth two holds), then the shaped pairs and the empty rows of Waves."""
    w = waves
    S = w.segments(w.u, w.p, w.n)
    assert S[:len(S_TARGETS)] == S_TARGETS and S[len(S_TARGETS)] > 16 and S[len(S_TARGETS) + 1] > 16, S
    assert len(set(w.u)) == len(w.u) and len(set(w.p) | set(w.n)) == 2 * len(w.u)
    check_three_forms(monkeypatch, w.g, w.E0, w.n_u, L, snap, t(w.u), t(w.p), t(w.n), exact=True)


@pytest.mark.parametrize("L,snap", FORMS)
def test_last_workgroup_of_one_valid_triple_on_two_passes(waves, L, snap, monkeypatch):
    """Workgroup 0: four valid triples; workgroup 1: a user below the range, ONE valid triple of 18 segments (a 1 024-entry user: its
    waves 0 and 1 take two items), a positive item above the range and a negative item far above it.  The skipped triples' other rows
    are named by nothing else and stay bit-unchanged."""
    w = waves
    k = 4 * len(S_TARGETS)                               # the (64, 1) workgroup's first triple: the 1 024-entry user
    u = np.concatenate([w.u[:4], [-1, w.u[k], w.u[k + 1], w.u[k + 2]]])
    p = np.concatenate([w.p[:4], [w.p[k + 1], w.p[k], N_ITEMS, w.p[k + 2]]])
    n = np.concatenate([w.n[:4], [w.n[k + 1], w.n[k], w.n[k + 2], 10 ** 12]])
    assert sum((int(w.deg[r]) + 63) // 64 for r in (w.u[k], w.n_u + w.p[k], w.n_u + w.n[k])) == 18
    untouched = [int(w.u[k + 1]), int(w.u[k + 2]), w.n_u + int(w.p[k + 1]), w.n_u + int(w.p[k + 2]), w.n_u + int(w.n[k + 1]), w.n_u + int(w.n[k + 2])]
    check_three_forms(monkeypatch, w.g, w.E0, w.n_u, L, snap, t(u), t(p), t(n), exact=True, unchanged_rows=untouched)


@pytest.mark.parametrize("L,snap", FORMS)
def test_hot_user_in_and_across_workgroups(waves, L, snap, monkeypatch):
    """One 1 024-entry user in all four triples of workgroup 0 (72 segments: five passes) and in triples of workgroups 1 to 3, items
    repeated as well: the atomics' order is free, so tolerances instead of bits."""
    w = waves
    rng = np.random.default_rng(43)
    hot = int(w.u[4 * len(S_TARGETS)])
    u = rng.choice(w.u[:4 * len(S_TARGETS)], 16)
    u[[0, 1, 2, 3, 4, 9, 15]] = hot
    items = rng.choice(np.concatenate([w.p, w.n]), 10)
    p, n = rng.choice(items, 16), rng.choice(items, 16)
    assert w.segments(u, p, n)[0] >= 64
    check_three_forms(monkeypatch, w.g, w.E0, w.n_u, L, snap, t(u), t(p), t(n), exact=False)


# ---- the bench's batch -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def epi(epinion2):
    from spex_amd.datasets import epinion2_tables
    from spex_amd.graph import SpexGraph, lightgcn_norm_adj
    tr = epinion2["train"]
    uw, iw = epinion2_tables(3186, 12407)
    trng = np.random.default_rng(2021)                   # bench.py's triples
    triples = tuple(t(trng.integers(0, hi, 2048)) for hi in (3185, 12407, 12407))
    return SpexGraph(*lightgcn_norm_adj(tr[:, 0], tr[:, 1], 3185, 12407)), t(np.concatenate([uw, iw])), 3186, triples


@pytest.mark.parametrize("L,snap", FORMS)
def test_three_steps_of_the_bench_batch_on_epinion2(epi, L, snap, monkeypatch):
    """Three consecutive steps of the bench's 2 048 triples on one fused stepper; before each, a whole-graph stepper starts from the
    fused one's table: after the step the tables agree to 2e-6 relative and the step's loss to 1e-6."""
    from spex_amd.trainer import LightGCNStepper
    g, E0, n_u, (u, p, n) = epi
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", snap)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    st = LightGCNStepper(g, E0.clone(), n_u, n_layers=L, lr=LR)
    for k in range(3):
        W = st.E0.clone()
        old, loss_old = forced_step(monkeypatch, g, W, n_u, L, snap, False, u, p, n)
        monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
        st.loss_acc.zero_()                              # (a difference of running sums would add their rounding to the step's)
        loss_new = st.step_bpr_sgd(u, p, n).item()
        err = rel_err(st.E0.cpu().numpy(), old.cpu().numpy())
        print("L", L, "snapshot", snap, "step", k, "loss", loss_new, loss_old, "rel_err", err)
        assert not torch.equal(st.E0, W)
        assert err <= 2e-6
        assert abs(loss_new - loss_old) <= 1e-6 * abs(loss_old)
