"""Inputs that put the scoring, BPR, owner-exchange, trust-head, dual-task, NGCF and headline BPR-SGD launches past every grid cap of
DESIGN.md 4.29, in NumPy alone, and the proof that they cross those caps — so that a later edit of a generator cannot silently move
a GPU case that uses them back under a cap.  Graph (e), its batches and the dense-pass cap are
those of tests/test_large_graph_host.py; new here:

  graph (e')      graph (e) with every row cut to at most 1 024 entries (user 0 keeps the first 1 024 of its 1 500 pairs), still
                  symmetric with LightGCN's values: no hub row, so the headline BPR-SGD step may fuse its last layer
  NGCF adjacency  D^-1 (A + I) of graph (e)'s pairs (spex_amd.graph.ngcf_norm_adj): non-symmetric, user 0's row of 1 501 entries
  trust paths     T paths of up to L positions over n_users users, padded with the pad row n_users: every length 1 .. L, user 0,
                  users above 32 768, the last user, a user repeated inside a path; targets 0 and n_users - 1 among them
  scoring inputs  B = 2 x 32 768 + 17 samples on 300 x 700 tables (three trips of score_bce_kernel's 32 768 waves), duplicated
                  users, one out-of-range index per trip
  owned rows      K = 70 001 positions over 20 000, the window [5 000, 15 000) owning about half, its four edges planted
  BPR triples     T = 524 288 + 12 345 on 300 x 500 tables in sampler order (five negatives per positive, positives sorted by user)
                  and shuffled, out-of-range triples in the last 12 345 (the second pass of 32 768 waves x 16 triples)
  headline sizes  T = 256, 2 048, 25 000 (6 T <= N: fused last layer), 25 001 (falls back), 40 000 (> 32 768 waves)
"""
import numpy as np

from test_large_graph_host import DENSE_PASS_ROWS, NE, NE_I, NE_U, WIDE_USERS, batch_e, csr_of_pairs, graph_e

# the bounds of DESIGN.md 4.29, read from the kernels
SCORE_PASS_WAVES = 2048 * 16                  # score.hip grid_for: 2 048 blocks of 16 waves, one wave per sample / triple / position
BPR_PER_WAVE = 16                             # score.hip bpr_per_wave: consecutive triples per wave from T = 16 x 16 384
BPR_PASS_TRIPLES = SCORE_PASS_WAVES * BPR_PER_WAVE
DUAL_ADAM_PASS_ROWS = DENSE_PASS_ROWS         # optim.hip dual_task_adam_kernel / adam_step_z2: 2 048 blocks x 256 float4 = 32 768 rows
TRUST_REDUCE_PASS_USERS = 1024 * 4            # trust.hip trust_reduce_kernel: 1 024 user blocks of 4 rows
TRUST_SWEEP_BATCH_ROWS, TRUST_MAX_SPLIT, CUS = 512, 8, 256
ROW_IDS_MAX_COLS = 65536                      # a handle of more columns has no row ids: adjacent rows, no row heads, xcd_contig off
ROW_MAX_FUSED = 1024                          # rows above this are hub rows (n_hub > 0): the headline step never fuses its last layer

SCORE_U, SCORE_I, SCORE_B = 300, 700, 2 * SCORE_PASS_WAVES + 17
SCORE_BAD = (60, SCORE_PASS_WAVES + 11, 2 * SCORE_PASS_WAVES + 3)          # one out-of-range sample in each trip
OWNED_K, OWNED_TOTAL, OWNED_LO, OWNED_LOCAL = 70001, 20000, 5000, 10000
BPR_U, BPR_I, BPR_T, BPR_TAIL = 300, 500, 524288 + 12345, 12345
TRUST_USERS = 40000
TRUST_SHAPES = [(15, 6, 3), (129, 6, 3), (15, 16, 4)]                      # (paths, positions, input heads)
SGD_FUSED_T, SGD_FALLBACK_T, SGD_HUB_T = (256, 2048, 25000), 25001, (2048, 40000)
_cache = {}


def graph_e_prime():
    """(rowptr, col, val, pairs) of graph (e'): of every user's and then of every item's pairs (sorted) only the first 1 024 stay."""
    if "e'" not in _cache:
        pairs = graph_e()[3]
        for side in (0, 1):
            order = np.lexsort((pairs[:, 1 - side], pairs[:, side]))
            pairs = pairs[order]
            first = np.flatnonzero(np.r_[True, pairs[1:, side] != pairs[:-1, side]])
            rank = np.arange(len(pairs)) - np.repeat(first, np.diff(np.r_[first, len(pairs)]))
            pairs = pairs[rank < ROW_MAX_FUSED]
        pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
        _cache["e'"] = csr_of_pairs(pairs) + (pairs,)
    return _cache["e'"]


def ngcf_adj_e():
    """D^-1 (A + I) over graph (e)'s pairs as (rowptr, col, val)."""
    if "ngcf" not in _cache:
        from spex_amd.graph import ngcf_norm_adj
        pairs = graph_e()[3]
        _cache["ngcf"] = ngcf_norm_adj(pairs[:, 0], pairs[:, 1], NE_U, NE_I)
    return _cache["ngcf"]


def trust_paths(n_users, T, L, seed):
    """(seq [T, L] padded with the pad row n_users, lengths [T], targets [T]) as int64."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, L + 1, T)
    lens[:min(L, T)] = np.arange(1, L + 1)[:T]                          # every length where T allows
    lens[-1] = L                                                         # the full width: no padded position
    seq = np.full((T, L), n_users, np.int64)
    for k in range(T):
        seq[k, :lens[k]] = rng.integers(0, n_users, lens[k])
    seq[1, 0], seq[2, 1], seq[3, 0] = 0, n_users - 1, n_users - 2        # user 0, the last user, one more above 32 768
    seq[4, :3] = seq[4, 0]                                               # the same user at several positions
    seq[5, 0], seq[5, 2] = 32768, 32769                                  # either side of the Adam pass's first trip
    tgt = rng.integers(0, n_users, T)
    tgt[0], tgt[1], tgt[2] = 0, n_users - 1, tgt[3]                      # a repeated target
    return seq, lens.astype(np.int64), tgt.astype(np.int64)


def score_inputs(d):
    """(users table, items table, u, i, labels) of the scoring case at width d; the samples at SCORE_BAD are out of range."""
    rng = np.random.default_rng(300 + d)
    users = (0.3 * rng.standard_normal((SCORE_U, d))).astype(np.float32)
    items = (0.3 * rng.standard_normal((SCORE_I, d))).astype(np.float32)
    u, i = rng.integers(0, SCORE_U, SCORE_B), rng.integers(0, SCORE_I, SCORE_B)
    u[:50] = 7
    u[-10:] = 7                                                          # the same user in the first and in the third trip
    u[SCORE_BAD[0]], i[SCORE_BAD[1]], u[SCORE_BAD[2]] = SCORE_U + 5, -1, SCORE_U
    y = (rng.random(SCORE_B) < 0.2).astype(np.float32)
    return users, items, u.astype(np.int64), i.astype(np.int64), y


def owned_positions():
    """K positions in [0, OWNED_TOTAL) with repeats; the window's edges lo - 1, lo, lo + n_local - 1, lo + n_local planted in the
    first and in the third trip."""
    rng = np.random.default_rng(41)
    pos = rng.integers(0, OWNED_TOTAL, OWNED_K)
    edges = [OWNED_LO - 1, OWNED_LO, OWNED_LO + OWNED_LOCAL - 1, OWNED_LO + OWNED_LOCAL]
    pos[:4], pos[-4:] = edges, edges
    pos[100:110] = OWNED_LO + 77                                         # one owned row ten times
    return pos.astype(np.int64)


def bpr_triples(shuffled):
    """(u, pos, neg) of BPR_T triples; out-of-range ones (user too large, negative positive, negative == table size) in the tail."""
    rng = np.random.default_rng(43)
    P = -(-BPR_T // 5)
    pu, pi = np.sort(rng.integers(0, BPR_U, P)), rng.integers(0, BPR_I, P)
    u, p = np.repeat(pu, 5)[:BPR_T], np.repeat(pi, 5)[:BPR_T]
    n = rng.integers(0, BPR_I, BPR_T)
    if shuffled:
        order = rng.permutation(BPR_T)
        u, p, n = u[order], p[order], n[order]
    u, p, n = u.copy(), p.copy(), n.copy()
    first = BPR_T - BPR_TAIL
    u[[first, first + 100]] = BPR_U + 5, -3
    p[first + 7000] = -1
    n[[first + 9999, BPR_T - 1]] = BPR_I, BPR_I + 1
    return u.astype(np.int64), p.astype(np.int64), n.astype(np.int64)


def bpr_in_range(u, p, n):
    return (u >= 0) & (u < BPR_U) & (p >= 0) & (p < BPR_I) & (n >= 0) & (n < BPR_I)


def sgd_triples(which, T):
    """(users, positives, negatives) of a headline BPR-SGD batch: batch_e's heavy BPR batch, seed 300 + T % 97."""
    return batch_e("bpr", which, 300 + T % 97, T)[1]


def trips(n, per_pass):
    return -(-n // per_pass)


# ------------------------------------------------------------------------------------------ the properties
def test_graph_e_has_hub_rows_and_no_row_ids():
    deg = np.diff(graph_e()[0])
    assert (deg > ROW_MAX_FUSED).sum() >= 1 and deg[0] == 1500                  # n_hub > 0: never fused
    assert NE > ROW_IDS_MAX_COLS                                                # adjacent-row layout: no row heads, xcd_contig off
    assert NE > DUAL_ADAM_PASS_ROWS and trips(NE, DUAL_ADAM_PASS_ROWS) == 5     # dual_task_adam parts 0 / 1, adam_step_z2's main grid
    assert NE_U > DUAL_ADAM_PASS_ROWS                                           # part 2 (the user rows) takes a second trip too
    assert NE_U - 1 > 2 * TRUST_REDUCE_PASS_USERS                               # the dual step's trust table: 39 999 users + the pad row


def test_graph_e_prime_is_graph_e_without_hub_rows():
    rowptr, col, val, pairs = graph_e_prime()
    deg, deg_e = np.diff(rowptr), np.diff(graph_e()[0])
    assert len(deg) == NE and deg.max() == ROW_MAX_FUSED and deg[0] == ROW_MAX_FUSED
    assert (deg <= deg_e).all() and (deg[WIDE_USERS] == 1000).all()
    changed = np.flatnonzero(deg != deg_e)
    assert changed[0] == 0 and len(changed) == 1 + (1500 - ROW_MAX_FUSED) and (changed[1:] >= NE_U).all()
    assert len(pairs) == len(graph_e()[3]) - (1500 - ROW_MAX_FUSED)
    rows = np.repeat(np.arange(NE), deg)
    fwd, bwd = rows.astype(np.int64) * NE + col, col.astype(np.int64) * NE + rows
    assert np.array_equal(np.sort(fwd), np.sort(bwd)) and len(np.unique(fwd)) == len(fwd)      # symmetric, no repeated entry
    assert np.array_equal(val, (1.0 / np.sqrt(deg[rows].astype(np.float64) * deg[col])).astype(np.float32))
    assert deg[-1] >= 1 and NE > ROW_IDS_MAX_COLS


def test_ngcf_adjacency_is_not_symmetric_and_has_hub_rows():
    rowptr, col, val = ngcf_adj_e()
    deg = np.diff(rowptr)
    assert len(deg) == NE and deg[0] == 1501 and (deg > ROW_MAX_FUSED).sum() >= 1
    assert deg.min() == 1                                                       # the self loop of an otherwise empty row
    rows = np.repeat(np.arange(NE), deg)
    assert np.allclose(np.bincount(rows, weights=val.astype(np.float64), minlength=NE), 1.0, atol=1e-5)     # D^-1 (A + I): rows sum to 1
    first_item = NE_U + graph_e()[3][0, 1]
    a = val[rowptr[0]:rowptr[1]][col[rowptr[0]:rowptr[1]] == first_item]
    b = val[rowptr[first_item]:rowptr[first_item + 1]][col[rowptr[first_item]:rowptr[first_item + 1]] == 0]
    assert len(a) == 1 and len(b) == 1 and a[0] != b[0]                         # A[0, i] != A[i, 0]
    assert NE > DUAL_ADAM_PASS_ROWS                                             # adam_step_z2's main grid takes a second trip


def test_scoring_inputs_cross_the_wave_cap_with_one_bad_index_per_trip():
    assert trips(SCORE_B, SCORE_PASS_WAVES) == 3
    for d in (64, 100):
        users, items, u, i, y = score_inputs(d)
        assert users.shape == (SCORE_U, d) and items.shape == (SCORE_I, d) and len(u) == len(i) == len(y) == SCORE_B
        bad = np.flatnonzero((u < 0) | (u >= SCORE_U) | (i < 0) | (i >= SCORE_I))
        assert tuple(bad) == SCORE_BAD and [b // SCORE_PASS_WAVES for b in bad] == [0, 1, 2]
        assert (u[:50] == 7).all() and (u[-10:] == 7).all() and 0 < y.mean() < 0.5


def test_owned_positions_cross_the_wave_cap_and_straddle_the_window():
    pos = owned_positions()
    assert len(pos) == OWNED_K and trips(OWNED_K, SCORE_PASS_WAVES) == 3
    own = (pos >= OWNED_LO) & (pos < OWNED_LO + OWNED_LOCAL)
    assert 0.45 <= own.mean() <= 0.55 and len(np.unique(pos)) < OWNED_K
    assert list(own[:4]) == [False, True, True, False] and list(own[-4:]) == [False, True, True, False]
    assert own[:SCORE_PASS_WAVES].any() and own[2 * SCORE_PASS_WAVES:].any() and (~own[2 * SCORE_PASS_WAVES:]).any()


def test_bpr_triples_cross_the_sixteen_per_wave_cap():
    assert min(BPR_T // (256 * 64), 16) == BPR_PER_WAVE and BPR_T > BPR_PASS_TRIPLES and BPR_T - BPR_TAIL == BPR_PASS_TRIPLES
    for shuffled in (False, True):
        u, p, n = bpr_triples(shuffled)
        ok = bpr_in_range(u, p, n)
        assert len(u) == BPR_T and (~ok).sum() == 5 and ok[:BPR_PASS_TRIPLES].all() and not ok[-1]
        if not shuffled:
            assert (np.diff(u[ok]) >= 0).all() and (u[:5] == u[0]).all() and (p[:5] == p[0]).all()
        else:
            assert (np.diff(u[ok]) < 0).any()
        assert len(np.unique(u[ok])) == BPR_U and len(np.unique(n[ok])) == BPR_I


def test_trust_paths_cross_the_reduce_cap_and_take_both_sweep_forms():
    n_users = TRUST_USERS
    assert trips(n_users, TRUST_REDUCE_PASS_USERS) >= 3 and min((n_users + 3) // 4, 1024) == 1024
    n_batches = trips(n_users, TRUST_SWEEP_BATCH_ROWS)
    for T, L, H in TRUST_SHAPES:
        split = min(TRUST_MAX_SPLIT, CUS // ((T + 7) & ~7), n_batches)          # trust.hip: spex::trust_head_train
        assert split == (TRUST_MAX_SPLIT if T == 15 else 1), (T, split)
        seq, lens, tgt = trust_paths(n_users, T, L, 70 + T + L)
        assert seq.shape == (T, L) and set(lens) >= (set(range(1, L + 1)) if T >= L else {1, L}) and lens.max() == L
        named = seq[np.arange(L)[None, :] < lens[:, None]]
        assert 0 in named and n_users - 1 in named and (named > 32768).any() and named.max() < n_users
        assert (seq[np.arange(L)[None, :] >= lens[:, None]] == n_users).all()
        assert tgt[0] == 0 and tgt[1] == n_users - 1 and tgt[2] == tgt[3]
        assert len(np.setdiff1d(np.arange(n_users), named)) > 0


def test_headline_sizes_sit_on_either_side_of_the_fused_rule():
    assert all(6 * T <= NE for T in SGD_FUSED_T) and 6 * SGD_FUSED_T[-1] == NE and 6 * SGD_FALLBACK_T > NE
    assert SGD_HUB_T[1] > SCORE_PASS_WAVES and 3 * SGD_HUB_T[1] == 120000 and SGD_HUB_T[0] <= SCORE_PASS_WAVES
    for T in SGD_FUSED_T + (SGD_FALLBACK_T,) + SGD_HUB_T:
        u, p, n = sgd_triples("heavy", T)
        assert len(u) == T and u.max() < NE_U and max(p.max(), n.max()) < NE_I and len(np.unique(u)) < T
        named = np.unique(np.concatenate([u, p + NE_U, n + NE_U]))
        assert len(named) < NE                                                  # some row is named by no triple
