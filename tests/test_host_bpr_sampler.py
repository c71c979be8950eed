"""trainer.bpr_epoch_triples: the host sampler of the exact BPR epochs (upstream LightGCN's uniform sampling — a user uniform over the
users with a positive, one of that user's positives uniformly, a negative uniform over the items that is none of them)."""
import numpy as np

from spex_amd.trainer import bpr_epoch_triples


def _pairs(rng, n_users, n_items, n, idle=()):
    u = rng.integers(0, n_users, n)
    u = u[~np.isin(u, idle)]
    return np.stack([u, rng.integers(0, n_items, len(u))], axis=1)


def test_negatives_are_never_positives_and_positives_always_are():
    rng = np.random.default_rng(1)
    n_users, n_items = 40, 25                      # dense: most first draws of a negative hit a positive and are redrawn
    pairs = _pairs(rng, n_users, n_items, 600, idle=(3, 17))
    pos_of = {u: set(pairs[pairs[:, 0] == u, 1]) for u in range(n_users)}
    u, p, n = bpr_epoch_triples(pairs, n_users, n_items, np.random.default_rng(2))
    assert u.dtype == p.dtype == n.dtype == np.int64 and len(u) == len(p) == len(n) == len(pairs)
    assert all(int(b) in pos_of[int(a)] for a, b in zip(u, p))
    assert not any(int(c) in pos_of[int(a)] for a, c in zip(u, n))
    assert n.min() >= 0 and n.max() < n_items
    assert not np.isin(u, (3, 17)).any()           # users without a positive are never drawn
    assert set(u) <= set(pairs[:, 0])


def test_same_seed_same_triples_and_only_its_own_generator():
    rng = np.random.default_rng(3)
    pairs = _pairs(rng, 30, 50, 400)
    state = np.random.get_state()[1].copy()
    a = bpr_epoch_triples(pairs, 30, 50, np.random.default_rng(7))
    b = bpr_epoch_triples(pairs, 30, 50, np.random.default_rng(7))
    c = bpr_epoch_triples(pairs, 30, 50, np.random.default_rng(8))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not all(np.array_equal(x, y) for x, y in zip(a, c))
    assert np.array_equal(np.random.get_state()[1], state)       # NumPy's global stream is untouched


def test_three_user_toy_set_draws_users_uniformly():
    """Users 0 / 1 / 2 hold 1 / 5 / 30 positives: upstream draws the USER uniformly, not the interaction.  36 000 draws, each user's
    count is Binomial(n, 1/3): within 5 sigma of n / 3.  User 1's five positives are uniform too (Binomial(n_1, 1/5), 5 sigma)."""
    pairs = np.array([[0, 4]] + [[1, i] for i in range(5)] + [[2, i] for i in range(10, 40)])
    pairs = np.tile(pairs, (1000, 1))              # duplicates do not weigh: 36 000 interactions -> 36 000 draws
    u, p, n = bpr_epoch_triples(pairs, 3, 50, np.random.default_rng(11))
    draws = len(u)
    assert draws == 36000
    sigma = np.sqrt(draws * (1 / 3) * (2 / 3))
    counts = np.bincount(u, minlength=3)
    print("per-user draws", counts, "expected", draws / 3, "5 sigma", 5 * sigma)
    assert np.abs(counts - draws / 3).max() <= 5 * sigma
    n1 = counts[1]
    c1 = np.bincount(p[u == 1], minlength=5)[:5]
    print("user 1 positives", c1)
    assert c1.sum() == n1 and np.abs(c1 - n1 / 5).max() <= 5 * np.sqrt(n1 * 0.2 * 0.8)
    assert (p[u == 0] == 4).all() and not np.isin(n[u == 2], np.arange(10, 40)).any()


def test_empty_and_invalid_inputs():
    import pytest
    u, p, n = bpr_epoch_triples(np.empty((0, 2), np.int64), 3, 5, np.random.default_rng(0))
    assert len(u) == len(p) == len(n) == 0
    with pytest.raises(ValueError, match="out of range"):
        bpr_epoch_triples(np.array([[0, 9]]), 3, 5, np.random.default_rng(0))
    with pytest.raises(ValueError, match="no negative"):
        bpr_epoch_triples(np.array([[0, 0], [0, 1]]), 1, 2, np.random.default_rng(0))
