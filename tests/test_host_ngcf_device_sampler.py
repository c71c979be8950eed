"""Host side of the device NGCF epoch sampler (no GPU): trainer.ngcf_sampler_tables, and a NumPy restatement of the law that
include/spex_hip.h writes down at spex_sample_ngcf_epoch (reference_epoch — test_gpu_ngcf_device_sampler.py holds the kernel to it bit
for bit).  The restatement is written from the header's text alone: F(x; m, K), the per-user keys of stage 5, the shuffle's of stage 6.

Exact properties (any size): a user's negatives are pairwise distinct, never one of its positives, always in the population; every
occurrence of a positive appears once; the epoch is a permutation of the unshuffled sources.
Marginal law: check_negative_law's shape does not fit (it takes the whole catalogue as the population and a with-replacement law), its
ACCEPTANCE does: a cell that a correct sampler fills with probability p in each of E independent keys holds Binomial(E, p), and must
lie within 6 sqrt(E p (1 - p)) of E p.  P(|z| > 6) = 2e-9 per cell; the cells checked below number under 10 000, so a correct sampler
fails with probability < 2e-5 — and the keys are fixed, so the test either holds or does not."""
import types

import numpy as np
import pytest
import torch

from test_host_bce_device_sampler import check_shuffle_grid, fmix32, half_bits
from test_host_bpr_device_sampler import philox4x32_10

from spex_amd.trainer import NgcfDeviceSampler, ngcf_sampler_tables

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ the documented law, in NumPy
def half_bits_many(m):
    """h = max(1, ceil(bits / 2)), bits the bit length of m - 1 (0 for m = 1), elementwise."""
    m = np.asarray(m, np.int64)
    bits = np.zeros(m.shape, np.int64)
    for b in range(32):
        bits += ((m - 1) >> b) != 0
    return np.maximum(1, (bits + 1) // 2)


def feistel(x, m, K):
    """F(x; m, K) elementwise: x, m arrays of one length (0 <= x < m), K uint64 [6, len].  Six rounds of
    (L, R) <- (R, L ^ (fmix32(R ^ K[r]) & mask)) on x = (L << h) | R, repeated while x >= m."""
    x = np.asarray(x, np.uint64).copy()
    m = np.asarray(m, np.uint64)
    h = half_bits_many(m).astype(np.uint64)
    mask = (np.uint64(1) << h) - np.uint64(1)
    todo = np.arange(len(x))
    while len(todo):
        hh, mm = h[todo], mask[todo]
        L, R = x[todo] >> hh, x[todo] & mm
        for r in range(6):
            L, R = R, L ^ (fmix32(R ^ K[r][todo]) & mm)
        x[todo] = (L << hh) | R
        todo = todo[x[todo] >= m[todo]]
    return x.astype(np.int64)


def stage_keys(c0_pair, epoch, stage, seed):
    """K[0 .. 3] = w0 .. w3 of counter (a0, a1, epoch, stage), K[4], K[5] = w0, w1 of counter (b0, b1, epoch, stage); c0_pair =
    ((a0, a1), (b0, b1)).  uint64 [6, len]."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    (a0, a1), (b0, b1) = c0_pair
    a = philox4x32_10(a0, a1, epoch, stage, k0, k1)
    b = philox4x32_10(b0, b1, epoch, stage, k0, k1)
    return np.stack([a[0], a[1], a[2], a[3], b[0], b[1]])


def negative_items(tables, q, i, seed, epoch):
    """Negative i of user q (arrays of one length; epoch a scalar or an array of that length): r = F(i; n_q, K_q), the r-th member of
    the population that is not one of the user's positives; item 0 where n_q <= 0 or i >= n_q."""
    pop, _, _, _, row_off, row_rank = (np.asarray(a, np.int64) for a in tables)
    q, i = np.asarray(q, np.int64), np.asarray(i, np.int64)
    m_q = np.diff(row_off)
    n_q = len(pop) - m_q
    out = np.zeros(len(q), np.int64)
    ok = np.flatnonzero((n_q[q] > 0) & (i < n_q[q]))
    if not len(ok):
        return out
    qq, ii = q[ok], i[ok]
    ep = np.broadcast_to(np.asarray(epoch, np.uint64), q.shape)[ok]
    K = stage_keys(((qq, 0), (qq, 1)), ep, 5, seed)
    r = feistel(ii, n_q[qq], K)
    # #{t : row_rank[row_off[q] + t] - t <= r}: the adjusted ranks ascend within a user; one composite key orders all users' segments
    owner = np.repeat(np.arange(len(m_q)), m_q)
    adj = row_rank - (np.arange(len(row_rank)) - row_off[owner])
    big = len(pop) + 1
    count = np.searchsorted(owner * big + adj, qq * big + r, side="right") - row_off[qq]
    out[ok] = pop[r + count]
    return out


def unshuffled_epoch(tables, seed, epoch):
    """The n = 6 n_pos source samples: (users, items, labels, the owning user's position q per source)."""
    pop, user, pos_off, pos_item, row_off, row_rank = (np.asarray(a, np.int64) for a in tables)
    c = np.diff(pos_off)
    q = np.repeat(np.arange(len(user)), 6 * c)
    i = np.arange(6 * len(pos_item)) - 6 * pos_off[q]
    k = 5 * c[q]
    neg = i < k
    items = np.empty(len(q), np.int64)
    items[~neg] = pos_item[(pos_off[q] + i - k)[~neg]]
    items[neg] = negative_items(tables, q[neg], i[neg], seed, epoch)
    return user[q], items, (~neg).astype(np.float32), q


def shuffle_perm(n, seed, epoch):
    """perm(s) = F(s; n, K), K from the counters (0, 0, epoch, 6) and (1, 0, epoch, 6)."""
    K = stage_keys(((0, 0), (1, 0)), epoch, 6, seed)
    return feistel(np.arange(n), np.full(n, n), np.repeat(K, n, axis=1))


def reference_epoch(tables, seed, epoch):
    """spex_sample_ngcf_epoch as include/spex_hip.h words it: (users, items, labels, source index per slot)."""
    u, v, y, _ = unshuffled_epoch(tables, seed, epoch)
    src = shuffle_perm(len(u), seed, epoch) if len(u) else np.zeros(0, np.int64)
    return u[src], v[src], y[src], src


# ------------------------------------------------------------------------------------------ graphs
def gap_graph():
    """A population of 18 items with id gaps (every id = 3 rank + 2 except the last, 99).  Users, in this order: 40 holds nothing
    (an empty user first), 7 holds three distinct items — 5 c = 15 = 18 - 3 = n_q exactly —, 12 holds [8, 5, 8] (a duplicated positive:
    c = 3, m = 2, n_q = 16), 3 holds nothing (an empty user in the middle), 9 holds one item, 21 holds nothing (an empty user last)."""
    all_items = {3 * r + 2 for r in range(17)} | {99}
    train_items = {40: [], 7: [50, 2, 99], 12: [8, 5, 8], 3: [], 9: [29], 21: []}
    return train_items, all_items, [40, 7, 12, 3, 9, 21]


def law_data():
    """A catalogue of 70 seen items out of ids 0 .. 139 (every second id, shifted: gaps everywhere), 6 users of 1 .. 9 positives: user 0
    has c = 3, n_q = 67; user 4 has a duplicated positive."""
    rng = np.random.default_rng(17)
    all_items = set((2 * np.arange(70) + 1).tolist())
    pop = np.array(sorted(all_items))
    train_items = {u: rng.choice(pop, c, replace=False).tolist() for u, c in enumerate((3, 9, 1, 6, 4, 2))}
    train_items[4][3] = train_items[4][0]
    return train_items, all_items, list(train_items.keys())


def epinion2_tables(epinion2):
    """Epinion2 as the NGCF drop-in's Data reads it: users ascending (file order), whole blocks of 256 users (3 072 of 3 185), the
    population = the items seen in training.  Returns (tables, data) — data stands in for the drop-in's Data object."""
    pairs = epinion2["train"][:, :2]
    order = np.argsort(pairs[:, 0], kind="stable")
    pairs = pairs[order]
    users, start = np.unique(pairs[:, 0], return_index=True)
    bounds = np.append(start, len(pairs))
    train_items = {int(u): pairs[bounds[k]:bounds[k + 1], 1].tolist() for k, u in enumerate(users)}
    data = types.SimpleNamespace(train_items=train_items, all_items=set(pairs[:, 1].tolist()), batch_size=256)
    epoch_users = list(train_items.keys())[: len(train_items) // 256 * 256]
    return ngcf_sampler_tables(train_items, data.all_items, epoch_users), data


# ------------------------------------------------------------------------------------------ 1. the tables
def test_tables_on_a_population_with_gaps():
    train_items, all_items, users = gap_graph()
    pop, user, pos_off, pos_item, row_off, row_rank = ngcf_sampler_tables(train_items, all_items, users)
    assert all(a.dtype == np.int32 for a in (pop, user, pos_off, pos_item, row_off, row_rank))
    assert pop.tolist() == sorted(all_items) and len(pop) == 18 and pop[-1] == 99 and pop[1] - pop[0] == 3
    assert user.tolist() == users
    assert pos_off.tolist() == [0, 0, 3, 6, 6, 7, 7]
    assert pos_item.tolist() == [50, 2, 99, 8, 5, 8, 29]                       # file order, the duplicate kept
    assert row_off.tolist() == [0, 0, 3, 5, 5, 6, 6]
    assert row_rank.tolist() == [0, 16, 17, 1, 2, 9]                           # ranks of {2, 50, 99}, {5, 8}, {29}, ascending per user
    n_q = len(pop) - np.diff(row_off)
    assert n_q.tolist() == [18, 15, 16, 18, 17, 18]
    assert 5 * 3 == n_q[1]                                                      # user 7: the sample is the whole complement
    for q in range(len(users)):
        seg = row_rank[row_off[q]:row_off[q + 1]]
        assert pop[seg].tolist() == sorted(set(train_items[users[q]]))
    # a user the dictionary does not know has no positives either
    t2 = ngcf_sampler_tables(train_items, all_items, [7, 1000])
    assert t2[2].tolist() == [0, 3, 3] and t2[4].tolist() == [0, 3, 3]
    empty = ngcf_sampler_tables(train_items, all_items, [])
    assert empty[2].tolist() == [0] and len(empty[3]) == 0 and len(empty[5]) == 0 and empty[1].dtype == np.int32


def test_tables_raise_the_references_error():
    train_items, all_items, users = gap_graph()
    train_items[9] = [29, 32, 35, 38]                                          # c = 4 distinct: 20 > 18 - 4
    with pytest.raises(ValueError, match="Sample larger than population or is negative"):
        ngcf_sampler_tables(train_items, all_items, users)
    train_items[9] = [29, 29, 29, 29]                                          # c = 4, m = 1: 20 > 17
    with pytest.raises(ValueError, match="Sample larger than population"):
        ngcf_sampler_tables(train_items, all_items, users)
    train_items[9] = [29, 29, 29]                                              # c = 3, m = 1: 15 <= 17
    assert ngcf_sampler_tables(train_items, all_items, users)[2][-1] == 9
    train_items[9] = [4]                                                       # an id in a gap of the population
    with pytest.raises(ValueError, match="outside the population"):
        ngcf_sampler_tables(train_items, all_items, users)
    with pytest.raises(ValueError, match="at least one item"):
        ngcf_sampler_tables({}, set(), [])


def test_sampler_object_holds_the_tables_of_whole_user_blocks():
    rng = np.random.default_rng(2)
    all_items = set(range(0, 400, 2))
    train_items = {u: rng.choice(np.arange(0, 400, 2), 1 + u % 4, replace=False).tolist() for u in range(600, 0, -1)}   # file order: descending ids
    data = types.SimpleNamespace(train_items=train_items, all_items=all_items, batch_size=128)
    s = NgcfDeviceSampler(data, seed=9, device="cpu")
    assert s.user.tolist() == list(range(600, 88, -1)) and s.user.numel() == 512         # two whole blocks of 256, the tail of 88 dropped
    assert s.n_pos == sum(len(train_items[u]) for u in range(600, 88, -1)) and s.n == 6 * s.n_pos
    assert (s.seed, s.batch_size) == (9, 128) and s.pop.dtype == torch.int32 and s.pop.numel() == 200
    assert not callable(s) and not hasattr(s, "sample_epoch")
    bufs = s.epoch_buffers()
    assert [b.dtype for b in bufs] == [torch.int64, torch.int64, torch.float32] and all(b.shape == (s.n,) for b in bufs)
    assert s.epoch_buffers()[0] is bufs[0]


# ------------------------------------------------------------------------------------------ 2. exact properties of the restated law
def check_epoch_is_valid(tables, u, v, y, src, seed, epoch):
    pop, user, pos_off, pos_item, row_off, row_rank = (np.asarray(a, np.int64) for a in tables)
    n = 6 * len(pos_item)
    assert len(u) == len(v) == len(y) == len(src) == n
    assert np.array_equal(np.sort(src), np.arange(n)), "the epoch is not a permutation of the unshuffled sources"
    su, sv, sy, sq = unshuffled_epoch(tables, seed, epoch)
    assert np.array_equal(u, su[src]) and np.array_equal(v, sv[src]) and np.array_equal(y, sy[src])
    q_of_slot = sq[src]
    assert np.isin(y, (0, 1)).all()
    for q in range(len(user)):
        mine = q_of_slot == q
        pos = pos_item[pos_off[q]:pos_off[q + 1]]
        assert np.all(u[mine] == user[q])
        neg = v[mine & (y == 0)]
        assert len(neg) == 5 * len(pos)
        assert len(np.unique(neg)) == len(neg), f"user at {q}: a negative is drawn twice"
        assert not np.isin(neg, pos).any(), f"user at {q}: a negative is one of its positives"
        assert np.isin(neg, pop).all(), f"user at {q}: a negative is outside the population"
        assert np.array_equal(np.sort(v[mine & (y == 1)]), np.sort(pos)), f"user at {q}: the positives do not appear once per occurrence"
        if 5 * len(pos) == len(pop) - len(np.unique(pos)):
            assert np.array_equal(np.sort(neg), np.setdiff1d(pop, pos)), f"user at {q}: the whole complement, once each"


@pytest.mark.parametrize("seed, epoch", [(0, 0), (0x123456789ABCDEF, 1), (77, 0x80000005), (0xFEDCBA9876543210, 2)])
def test_restated_law_is_exact_on_the_gap_graph_and_the_law_graph(seed, epoch):
    for train_items, all_items, users in (gap_graph(), law_data()):
        tables = ngcf_sampler_tables(train_items, all_items, users)
        u, v, y, src = reference_epoch(tables, seed, epoch)
        check_epoch_is_valid(tables, u, v, y, src, seed, epoch)
    # the unshuffled order is the reference's: per user the negatives, then the positives in file order
    tables = ngcf_sampler_tables(*gap_graph())
    su, sv, sy, _ = unshuffled_epoch(tables, seed, epoch)
    assert su.tolist() == [7] * 18 + [12] * 18 + [9] * 6
    assert sy.tolist() == ([0.0] * 15 + [1.0] * 3) * 2 + [0.0] * 5 + [1.0]
    assert sv[15:18].tolist() == [50, 2, 99] and sv[33:36].tolist() == [8, 5, 8] and sv[41] == 29


def test_draws_differ_between_keys_and_users_do_not_share_a_permutation():
    tables = ngcf_sampler_tables(*law_data())
    a, b, c = (unshuffled_epoch(tables, s, e)[1] for s, e in ((5, 0), (5, 1), (6, 0)))
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    # two users with the same row and the same n_q draw different negatives: the key is the user's position
    train_items = {0: [1, 3, 5], 1: [1, 3, 5]}
    t2 = ngcf_sampler_tables(train_items, set(range(1, 141, 2)), [0, 1])
    v = unshuffled_epoch(t2, 5, 0)[1]
    assert not np.array_equal(v[:15], v[18:33])


# ------------------------------------------------------------------------------------------ 3. the marginal law
def test_negatives_are_uniform_over_the_complement():
    """law_data()'s users over E = 4 096 keys (seeds 0 .. 63 x epochs 0 .. 63).  For every user (n_q = 61 .. 69 >= 32) and every member
    j of its complement: (a) negative 0 is j in Binomial(E, 1 / n_q) of the keys — the bijection's image of one point is uniform;
    (b) j is among the user's k = 5 c negatives in Binomial(E, k / n_q) of the keys — the inclusion probability of a sample without
    replacement.  Every cell within 6 sqrt(E p (1 - p)) of E p, cells outside the complement empty.  The smallest expectation is
    E / n_q = 59 (the normal approximation behind 6 sigma wants > 30).  The keys are fixed, so the figures are too: the restatement's
    largest deviations are 3.33 sigma (first draw) and 3.04 sigma (inclusion) over the 396 cells of each kind — what the largest of
    396 standard normal values is expected to be, 2.7 sigma short of the bound."""
    train_items, all_items, users = law_data()
    tables = ngcf_sampler_tables(train_items, all_items, users)
    pop, _, pos_off, pos_item, row_off, _ = (np.asarray(a, np.int64) for a in tables)
    seeds, epochs = np.meshgrid(np.arange(64), np.arange(64))
    E = seeds.size
    worst = [0.0, 0.0]
    for q in range(len(users)):
        pos = pos_item[pos_off[q]:pos_off[q + 1]]
        k = 5 * len(pos)
        comp = np.setdiff1d(pop, pos)
        n_q = len(comp)
        assert n_q == len(pop) - (row_off[q + 1] - row_off[q]) >= 32 and E / n_q > 30
        draws = np.empty((E, k), np.int64)
        for s in range(64):                                        # (the seed is a scalar of the restatement; the epochs vectorise)
            ep = np.repeat(np.arange(64), k)
            got = negative_items(tables, np.full(64 * k, q), np.tile(np.arange(k), 64), int(s), ep)
            draws[s * 64:(s + 1) * 64] = got.reshape(64, k)
        assert np.isin(draws, comp).all()
        assert all(len(set(row)) == k for row in draws.tolist())
        rank = np.searchsorted(comp, draws)
        for which, (cells, p) in enumerate(((np.bincount(rank[:, 0], minlength=n_q), 1.0 / n_q),
                                            (np.bincount(rank.ravel(), minlength=n_q), k / n_q))):
            if p >= 1.0:
                assert np.all(cells == E)
                continue
            z = np.abs(cells - E * p) / np.sqrt(E * p * (1 - p))
            worst[which] = max(worst[which], float(z.max()))
            assert cells.min() > 0
            assert z.max() <= 6.0, f"user at {q}: a complement item is {z.max():.2f} standard deviations from its expectation ({('first draw', 'inclusion')[which]})"
    print(f"{E} keys: first-draw cells worst {worst[0]:.2f} sigma, inclusion cells worst {worst[1]:.2f} sigma")


# ------------------------------------------------------------------------------------------ 4. the shuffle
def test_shuffle_grid_on_one_epinion2_sized_epoch(epinion2):
    tables, _ = epinion2_tables(epinion2)
    n = 6 * len(tables[3])
    assert len(tables[1]) == 3072 and 1_200_000 < n < 1_260_000
    src = shuffle_perm(n, 2020, 0)
    worst = check_shuffle_grid(src, grid=16)
    print(f"n = {n}: 16 x 16 (slot bucket, source bucket) grid, largest deviation {worst:.2f} sigma")
    assert not np.array_equal(src, shuffle_perm(n, 2020, 1))
    assert half_bits(n) == 11


def test_feistel_restatement_agrees_with_the_bce_modules_on_equal_keys():
    """F is spex_sample_bce_epoch's network: with that sampler's round keys (stage 3) it is that module's perm."""
    from test_host_bce_device_sampler import perm, round_keys
    for n in (1, 2, 6, 7, 96, 4097):
        K = round_keys(77, 5)
        assert np.array_equal(feistel(np.arange(n), np.full(n, n), np.repeat(K, n, axis=1)), perm(n, 77, 5)[0])
        assert int(half_bits_many(np.array([n]))[0]) == half_bits(n)
