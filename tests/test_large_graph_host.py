"""Graph (e) and its batches, in NumPy alone: the inputs of tests/test_gpu_large_graph.py, and the proof that they cross every grid
cap and table switch of DESIGN.md 4.25 — so that a later edit of the generator cannot silently move those tests back under a cap.

Graph (e): a seeded symmetric bipartite graph of 150 000 rows (40 000 user rows, 110 000 item rows) with LightGCN's
1 / sqrt(deg deg) values, built the way graph (b) of tests/test_gpu_frontier.py is: ~3 entries per row; user 0 a hub of 1 500 entries;
users 1 .. 5 of 65, 100, 128, 129 and 200 entries; users 10 .. 19 and items 109 980 .. 109 989 empty; the last row non-empty; users
100 .. 179 "wide", exactly 1 000 entries each over the pairwise disjoint item blocks [1 000 k, 1 000 (k + 1)).  No row is longer than
2 600 entries, the longest row the suite already runs.

Batches repeat users and items.  `heavy` names all 80 wide users, the hub, an empty user and the last row: its F1 holds the 80 000
items of the wide blocks.  `light` draws from a pool of 300 users and 300 items that holds no wide user: its lists are small.
"""
import numpy as np

NE, NE_U = 150000, 40000
NE_I = NE - NE_U
LONG_USERS = {0: 1500, 1: 65, 2: 100, 3: 128, 4: 129, 5: 200}
EMPTY_USERS = np.arange(10, 20)
EMPTY_ITEMS = np.arange(NE_I - 20, NE_I - 10)
WIDE_USERS = np.arange(100, 180)
WIDE = 1000
SIZES = {"bce": (256, 2048), "bpr": (256, 2048)}          # BPR: the push form and the dense form (>= kBprStepDenseMinTriples = 768)
# the bounds of DESIGN.md 4.25, read from the kernels (d = 64)
DENSE_PASS_ROWS = 2048 * 256 * 4 // 64                    # adam_kernel / adam_shadow_kernel / zero_kernel / zero_rows_kernel: 32 768 rows
LIST_PASS_ROWS = 65536                                    # adam_rows (2 048 x 32), frontier_rows (2^14 x 4), push_rows (2^16), cast_bf16
ADJACENT_ROWS_FROM = (16 << 20) // 256 + 1                # the packer's adjacent-row layout: a source table beyond 16 MiB
_cache = {}


def csr_of_pairs(pairs):
    """(rowptr, col, val) of the symmetric bipartite graph over NE rows of distinct (user, item) pairs, 1 / sqrt(deg deg) values."""
    rows = np.concatenate([pairs[:, 0], pairs[:, 1] + NE_U])
    cols = np.concatenate([pairs[:, 1] + NE_U, pairs[:, 0]])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    deg = np.bincount(rows, minlength=NE)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    val = (1.0 / np.sqrt(deg[rows].astype(np.float64) * deg[cols])).astype(np.float32)
    return rowptr, cols.astype(np.int32), val


def graph_e():
    """(rowptr, col, val, train pairs) of graph (e)."""
    if "e" not in _cache:
        rng = np.random.default_rng(13)
        n_pairs = 140000
        u = rng.integers(200, NE_U, n_pairs)
        i = rng.integers(0, NE_I - 20, n_pairs)
        for user, deg in LONG_USERS.items():
            u = np.concatenate([u, np.full(deg, user)])
            i = np.concatenate([i, rng.choice(NE_I - 20, deg, replace=False)])
        for k, user in enumerate(WIDE_USERS):
            u = np.concatenate([u, np.full(WIDE, user)])
            i = np.concatenate([i, np.arange(WIDE * k, WIDE * (k + 1))])
        u, i = np.concatenate([u, [200]]), np.concatenate([i, [NE_I - 1]])          # the last row is not empty
        pairs = np.unique(np.stack([u, i], 1), axis=0).astype(np.int64)
        _cache["e"] = csr_of_pairs(pairs) + (pairs,)
    return _cache["e"]


def table_e(d=64):
    if ("E0", d) not in _cache:
        _cache["E0", d] = (0.1 * np.random.default_rng(7).normal(size=(NE, d))).astype(np.float32)
    return _cache["E0", d]


def light_pool():
    """(users, items) the light batches draw from: 300 + 300 rows, the multi-segment users 1 .. 5 and an empty user among them, no
    wide user and no item of a wide block."""
    rng = np.random.default_rng(17)
    users = np.concatenate([[1, 2, 3, 4, 5, 12], rng.choice(np.arange(200, NE_U), 294, replace=False)])
    items = rng.choice(np.arange(WIDE * len(WIDE_USERS), NE_I - 20), 300, replace=False)
    return users, items


def batch_e(kind, which, seed, n):
    """(kind, (users, items, labels)) or (kind, (users, positives, negatives)) of n samples on graph (e); which: 'heavy' / 'light'."""
    rng = np.random.default_rng(seed)
    if which == "heavy":
        u, a, b = rng.integers(0, NE_U, n), rng.integers(0, NE_I, n), rng.integers(0, NE_I, n)
        u[:82] = np.concatenate([WIDE_USERS, [0, 12]])
        a[0], b[1] = NE_I - 1, NE_I - 1                   # the last row, on either item side
    else:
        users, items = light_pool()
        u, a, b = rng.choice(users, n), rng.choice(items, n), rng.choice(items, n)
        u[:6] = users[:6]
    u[-1], a[-1] = u[1], a[1]                             # a repeated (user, item) pair
    if kind == "bce":
        return "bce", (u.astype(np.int64), a.astype(np.int64), rng.integers(0, 2, n).astype(np.float32))
    return "bpr", (u.astype(np.int64), a.astype(np.int64), b.astype(np.int64))


def batch_rows(el):
    kind, arrs = el[0], el[1]
    return np.concatenate([arrs[0]] + [x + NE_U for x in arrs[1:(2 if kind == "bce" else 3)]])


def frontier_sets(csr, rows):
    """(Bset, F1) as sorted arrays: tests/test_gpu_frontier.py::frontier_sets, vectorised (that one loops over the rows in Python,
    which is slow over 80 000 of them; test_sets_agree_with_the_frontier_modules_rule holds the two together)."""
    rowptr, col = csr[0], csr[1]
    n = len(rowptr) - 1
    bset = np.unique(rows[(rows >= 0) & (rows < n)])
    lens = (rowptr[bset + 1] - rowptr[bset]).astype(np.int64)
    starts = np.repeat(rowptr[bset].astype(np.int64) - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return bset, np.union1d(bset, col[starts + np.arange(lens.sum())])


def sets_e(el):
    """(Bset, F1, F2) of a batch on graph (e), once per batch."""
    key = ("sets", el[0], el[1][0].tobytes(), el[1][1].tobytes(), el[1][2].tobytes() if el[0] == "bpr" else b"")
    if key not in _cache:
        csr = graph_e()
        bset, f1 = frontier_sets(csr, batch_rows(el))
        _cache[key] = (bset, f1, frontier_sets(csr, f1)[1])
    return _cache[key]


CASES = [(kind, which, n) for kind in ("bce", "bpr") for which in ("heavy", "light") for n in SIZES[kind]]


# ------------------------------------------------------------------------------------------ the properties
def test_graph_e_has_the_rows_it_claims():
    rowptr, col, val, pairs = graph_e()
    deg = np.diff(rowptr)
    assert len(deg) == NE and NE > LIST_PASS_ROWS and NE >= ADJACENT_ROWS_FROM
    assert NE * 64 > 2 * 2048 * 256 * 4 and NE > 2 * DENSE_PASS_ROWS            # a dense pass makes more than two trips (4.6)
    assert deg.max() <= 2600
    assert deg[0] == 1500 and list(deg[1:6]) == [65, 100, 128, 129, 200]
    assert not deg[EMPTY_USERS].any() and not deg[NE_U + EMPTY_ITEMS].any() and deg[-1] >= 1
    assert (deg[WIDE_USERS] == WIDE).all()
    blocks = [col[rowptr[u]:rowptr[u + 1]] for u in WIDE_USERS]
    assert len(np.unique(np.concatenate(blocks))) == WIDE * len(WIDE_USERS)     # pairwise disjoint
    assert 2.5 <= deg.mean() <= 3.5
    # symmetric, LightGCN values
    rows = np.repeat(np.arange(NE), deg)
    fwd = rows.astype(np.int64) * NE + col
    bwd = col.astype(np.int64) * NE + rows
    assert np.array_equal(np.sort(fwd), np.sort(bwd)) and len(np.unique(fwd)) == len(fwd)
    assert np.array_equal(val, (1.0 / np.sqrt(deg[rows].astype(np.float64) * deg[col])).astype(np.float32))
    assert ((rows < NE_U) != (col < NE_U)).all()                                # bipartite
    assert table_e().shape == (NE, 64) and table_e(128).shape == (NE, 128)


def test_sets_agree_with_the_frontier_modules_rule():
    """The vectorised frontier_sets is tests/test_gpu_frontier.py's, on a light batch of graph (e) and on graph (b)."""
    import test_gpu_frontier as frmod
    el = batch_e("bpr", "light", 3, 256)
    for csr, rows in ((graph_e(), batch_rows(el)), (frmod.graph_b(), np.array([0, 0, 12, 9000, -4, 8005, 19999 + 3, 8007], np.int64))):
        want, got = frmod.frontier_sets(csr, rows), frontier_sets(csr, rows)
        assert all(np.array_equal(a, b) for a, b in zip(want, got))
        want2, got2 = frmod.frontier_sets(csr, want[1]), frontier_sets(csr, got[1])
        assert np.array_equal(want2[1], got2[1])


def test_batches_cross_or_stay_under_the_list_caps():
    for kind, which, n in CASES:
        for seed in (1, 2):
            el = batch_e(kind, which, seed, n)
            u = el[1][0]
            assert len(u) == n and all(len(x) == n for x in el[1])
            assert len(np.unique(u)) < n                                        # users repeat
            bset, f1, f2 = sets_e(el)
            if which == "heavy":
                assert np.isin(WIDE_USERS, u).all() and 0 in u and 12 in u and NE - 1 in bset
                assert len(f1) >= 80000 and len(np.union1d(bset, f1)) > LIST_PASS_ROWS, (kind, n, len(f1))
                assert len(f2) > len(f1) and len(f2) > LIST_PASS_ROWS, (kind, n, len(f2))
                assert len(f2) < NE                                             # rows stay outside: the sparse pass has something to leave alone
            else:
                assert not np.isin(WIDE_USERS, f1).any()
                assert len(f2) < DENSE_PASS_ROWS, (kind, n, len(f2))
                assert 12 in bset and len(bset) > 100


def test_dense_form_threshold_is_crossed_by_the_large_bpr_batch():
    assert SIZES["bpr"][0] < 768 <= SIZES["bpr"][1]                             # steps.hip: kBprStepDenseMinTriples
