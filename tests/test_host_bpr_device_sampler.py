"""Host side of the device BPR sampler (no GPU): the tables it draws from, a NumPy Philox4x32-10 against the Random123 known
answers, and the law checker — validated here on the host sampler, used on the device sampler by test_gpu_bpr_device_sampler.py.

The law checker's bound is the binomial law's own: a cell of probability p holds Binomial(n, p) draws, standard deviation
sqrt(n p (1 - p)); every cell must lie within 6 of them.  P(|z| > 6) = 2e-9 per cell (the normal approximation holds: the smallest
expected count is in the thousands), so over the ~300 cells of the graph below a correct sampler fails with probability < 1e-6."""
import numpy as np
import pytest

from spex_amd.trainer import bpr_epoch_triples, bpr_sampler_tables

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ Philox4x32-10 in NumPy
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Standard Philox4x32-10 on arrays (or scalars) of 32-bit words held in uint64: returns the four output words."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_numpy_philox_reproduces_the_random123_known_answers(ctr, key, want):
    got = tuple(int(w[0]) for w in philox4x32_10(*ctr, *key))
    assert got == want, [hex(g) for g in got]


def test_numpy_philox_is_elementwise():
    ctr = np.array([[0, 0, 0, 0], [0xffffffff] * 4, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], np.uint64)
    a = philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], 0xa4093822, 0x299f31d0)
    for r in range(3):
        b = philox4x32_10(*ctr[r], 0xa4093822, 0x299f31d0)
        assert [int(w[r]) for w in a] == [int(w[0]) for w in b]


# ------------------------------------------------------------------------------------------ the tables
def test_sampler_tables_are_the_host_samplers_key_set():
    rng = np.random.default_rng(3)
    n_users, n_items = 40, 23
    pairs = np.stack([rng.integers(0, n_users, 300), rng.integers(0, n_items, 300)], 1)
    pairs = pairs[(pairs[:, 0] != 7) & (pairs[:, 0] != 39)]                  # users 7 and 39 (the last row) have no positive
    pairs = np.concatenate([pairs, pairs[:50], pairs[10:20]])                 # duplicates, some of them three times
    rng.shuffle(pairs)
    rowptr, items, active = bpr_sampler_tables(pairs, n_users, n_items)
    assert rowptr.dtype == items.dtype == active.dtype == np.int32
    keys = np.unique(pairs[:, 0] * n_items + pairs[:, 1])                     # bpr_epoch_triples' key set
    assert rowptr.shape == (n_users + 1,) and rowptr[0] == 0 and rowptr[-1] == len(keys) == len(items)
    assert len(keys) < len(pairs)
    rows = np.repeat(np.arange(n_users), np.diff(rowptr))
    assert np.array_equal(rows * n_items + items, keys)                      # same pairs, sorted by (user, item): rows ascending, no duplicate
    for u in range(n_users):
        row = items[rowptr[u]:rowptr[u + 1]]
        assert np.all(np.diff(row) > 0)
    assert 7 not in active and 39 not in active
    assert np.array_equal(active, np.unique(pairs[:, 0]))
    assert rowptr[8] == rowptr[7]
    # a list of pairs, and an empty one
    r2, i2, a2 = bpr_sampler_tables([(1, 2), (1, 2), (0, 3)], 3, 5)
    assert r2.tolist() == [0, 1, 2, 2] and i2.tolist() == [3, 2] and a2.tolist() == [0, 1]
    r3, i3, a3 = bpr_sampler_tables(np.empty((0, 2), np.int64), 3, 5)
    assert r3.tolist() == [0, 0, 0, 0] and len(i3) == 0 and len(a3) == 0


@pytest.mark.parametrize("fn", [lambda p, nu, ni: bpr_sampler_tables(p, nu, ni),
                                lambda p, nu, ni: bpr_epoch_triples(p, nu, ni, np.random.default_rng(0))])
def test_sampler_tables_raise_what_the_host_sampler_raises(fn):
    ok = [(0, 0), (1, 2)]
    for bad in ([(3, 0)], [(-1, 0)], [(0, 4)], [(0, -1)]):
        with pytest.raises(ValueError, match="out of range"):
            fn(np.array(ok + bad), 3, 4)
    with pytest.raises(ValueError, match="every item"):
        fn(np.array([(2, 0), (2, 1), (2, 2), (2, 3), (2, 3), (0, 1)]), 3, 4)
    fn(np.array([(2, 0), (2, 1), (2, 2), (2, 2), (0, 1)]), 3, 4)               # all but one item: fine


# ------------------------------------------------------------------------------------------ the law checker
N_LAW = 1 << 20


def law_graph():
    """8 users x 16 items: user 0 has no positive, user 1 holds items 0 - 14 (only item 15 is a valid negative), user 2 holds one item,
    users 3 - 7 hold 3 .. 8 random items (one of them exactly 8).  Returns (pairs [nnz, 2], n_users, n_items)."""
    rng = np.random.default_rng(11)
    rows = {1: np.arange(15), 2: np.array([9])}
    for u, deg in zip(range(3, 8), (3, 8, 5, 6, 4)):
        rows[u] = np.sort(rng.choice(16, deg, replace=False))
    pairs = np.array([(u, i) for u, row in rows.items() for i in row], np.int64)
    return pairs, 8, 16


def check_law(users, pos, neg, pairs, n_users, n_items, by="user"):
    """Every joint cell (user, pos, neg) of the sampling law against its binomial bound: a cell of probability p > 0 holds within
    6 sqrt(n p (1 - p)) of n p draws, a cell of probability 0 none.  by "user": P(user) = 1 / #active; "interaction": degree / nnz.
    Returns (largest deviation in standard deviations, smallest expected count, number of cells with p > 0)."""
    users, pos, neg = (np.asarray(a, np.int64) for a in (users, pos, neg))
    n = len(users)
    assert len(pos) == n and len(neg) == n
    for a, hi in ((users, n_users), (pos, n_items), (neg, n_items)):
        assert a.min() >= 0 and a.max() < hi
    has = np.zeros((n_users, n_items), bool)
    has[pairs[:, 0], pairs[:, 1]] = True
    deg = has.sum(1)
    p_user = (deg > 0) / (deg > 0).sum() if by == "user" else deg / deg.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        p_cell = p_user / deg / (n_items - deg)                               # per (pos in row, neg not in row)
    p = np.where(has[:, :, None] & ~has[:, None, :], p_cell[:, None, None], 0.0)
    assert abs(p.sum() - 1.0) < 1e-12
    count = np.bincount((users * n_items + pos) * n_items + neg, minlength=p.size).reshape(p.shape)
    assert count[p == 0].sum() == 0, "a draw landed in a cell of probability zero"
    live = p > 0
    sigma = np.sqrt(n * p[live] * (1 - p[live]))
    z = np.abs(count[live] - n * p[live]) / sigma
    worst = float(z.max())
    assert worst <= 6.0, f"a cell is {worst:.2f} standard deviations from its expectation"
    return worst, float((n * p[live]).min()), int(live.sum())


def test_law_checker_accepts_the_host_sampler_and_rejects_wrong_laws():
    pairs, n_users, n_items = law_graph()
    tiled = np.tile(pairs, (-(-N_LAW // len(pairs)), 1))[:N_LAW]              # bpr_epoch_triples draws one triple per pair given
    u, p, ng = bpr_epoch_triples(tiled, n_users, n_items, np.random.default_rng(1))
    assert len(u) == N_LAW
    worst, smallest, cells = check_law(u, p, ng, pairs, n_users, n_items, by="user")
    print(f"host sampler: {cells} cells, largest deviation {worst:.2f} sigma, smallest expected count {smallest:.0f}")
    assert 250 <= cells <= 350 and smallest > 2000
    assert np.all(ng[u == 1] == 15)
    # the checker is not vacuous: the by-user stream is not the by-interaction law, a positive as negative is caught, and so is a
    # user marginal that is off by a few percent
    with pytest.raises(AssertionError):
        check_law(u, p, ng, pairs, n_users, n_items, by="interaction")
    bad = ng.copy()
    bad[0] = p[0]
    with pytest.raises(AssertionError, match="probability zero"):
        check_law(u, p, bad, pairs, n_users, n_items, by="user")
    keep = np.ones(N_LAW, bool)
    keep[np.flatnonzero(u == 2)[::10]] = False                                # user 2 under-drawn by 10 %: ~10 sigma in each of its cells
    with pytest.raises(AssertionError, match="standard deviations"):
        check_law(u[keep], p[keep], ng[keep], pairs, n_users, n_items, by="user")
