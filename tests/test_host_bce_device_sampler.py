"""Host side of the device BCE epoch sampler (no GPU): a NumPy restatement of the stream include/spex_hip.h writes down at
spex_sample_bce_epoch (reference_epoch, perm — test_gpu_bce_device_sampler.py holds the kernel to it bit for bit), the shuffle as a
bijection, and the statistical checkers — validated here on the host path (LightTrainData.ng_sample() followed by
dataloader_epoch_order), shown to reject wrong laws, then used on the device sampler by the GPU tests.

Bounds are the binomial law's own: a cell of probability p over n trials has standard deviation sqrt(n p (1 - p)); every cell must
lie within 6 of them.  P(|z| > 6) = 2e-9 per cell, so over the few thousand cells checked below a correct sampler fails with
probability < 1e-5.  (The shuffle's cells are hypergeometric — a permutation places every source exactly once — whose variance is
smaller than the binomial's, so the binomial bound holds a fortiori.)"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_host_bpr_device_sampler import law_graph, philox4x32_10

from spex_amd.trainer import BceDeviceSampler, bpr_sampler_tables, dataloader_epoch_order

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ the documented stream, in NumPy
def to_range(w, m):
    """floor(w * m / 2^32) for 32-bit words w held in uint64."""
    return ((w * np.asarray(m, np.uint64)) >> np.uint64(32)).astype(np.int64)


def fmix32(x):
    """MurmurHash3's 32-bit finaliser on 32-bit words held in uint64."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def round_keys(seed, epochs):
    """K[0 .. 3] = the four words of counter (0, 0, epoch, 3), K[4 .. 5] = words 0 and 1 of counter (1, 0, epoch, 3); key = seed.
    For an array of epochs: uint64 [6, len(epochs)]."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    epochs = np.atleast_1d(np.asarray(epochs, np.uint64))
    a = philox4x32_10(0, 0, epochs, 3, k0, k1)
    b = philox4x32_10(1, 0, epochs, 3, k0, k1)
    return np.stack([a[0], a[1], a[2], a[3], b[0], b[1]])


def half_bits(n):
    """h = max(1, ceil(bits / 2)), bits the bit length of n - 1."""
    return max(1, -(-int(n - 1).bit_length() // 2))


def perm_many(n, seed, epochs):
    """perm(i) for every i in [0, n) and every epoch of `epochs` ([E, n]), with the number of Feistel passes every slot took: six
    rounds of (L, R) <- (R, L ^ (fmix32(R ^ K[r]) & mask)) on x = (L << h) | R, repeated while x >= n."""
    h = np.uint64(half_bits(n))
    mask = (np.uint64(1) << h) - np.uint64(1)
    K = round_keys(seed, epochs)                                   # [6, E]
    E = K.shape[1]
    x = np.tile(np.arange(n, dtype=np.uint64), E)
    row = np.repeat(np.arange(E), n)                               # the epoch of every flattened slot
    walks = np.zeros(E * n, np.int64)
    todo = np.arange(E * n)
    while len(todo):
        L, R = x[todo] >> h, x[todo] & mask
        for r in range(6):
            L, R = R, L ^ (fmix32(R ^ K[r][row[todo]]) & mask)
        x[todo] = (L << h) | R
        walks[todo] += 1
        todo = todo[x[todo] >= np.uint64(n)]
    return x.astype(np.int64).reshape(E, n), walks.reshape(E, n)


def perm(n, seed, epoch):
    src, walks = perm_many(n, seed, [epoch])
    return src[0], walks[0]


def reference_epoch(rowptr, items, pos_user, pos_item, num_ng, num_item, seed, epoch):
    """spex_sample_bce_epoch as include/spex_hip.h words it.  Returns (users, items, labels, source index per slot, number of
    negatives that took the direct draw)."""
    rowptr, items, pos_user, pos_item = (np.asarray(a, np.int64) for a in (rowptr, items, pos_user, pos_item))
    P = len(pos_user)
    n = P * (1 + num_ng)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    # the unshuffled epoch: positives, then the negatives of positive 0, of positive 1, ...
    k = np.arange(P * num_ng, dtype=np.uint64)
    k_lo, k_hi = k & M32, k >> np.uint64(32)
    users = pos_user[np.arange(P * num_ng) // num_ng]
    n_rows = len(rowptr) - 1
    inside = (users >= 0) & (users < n_rows)
    safe = np.where(inside, users, 0)
    beg, end = np.where(inside, rowptr[safe], 0), np.where(inside, rowptr[safe + 1], 0)
    keys = np.repeat(np.arange(n_rows), np.diff(rowptr)) * num_item + items      # ascending

    def stored(at, j):
        q = users[at] * num_item + j
        pos = np.searchsorted(keys, q)
        return inside[at] & (pos < len(keys)) & (keys[np.minimum(pos, max(len(keys) - 1, 0))] == q) if len(keys) else np.zeros(len(at), bool)

    neg = np.zeros(P * num_ng, np.int64)
    todo = np.arange(P * num_ng)
    for stage in (0, 1):
        if not len(todo):
            break
        w = philox4x32_10(k_lo[todo], k_hi[todo], epoch, stage, k0, k1)
        left = np.arange(len(todo))
        for a in range(4):
            cand = to_range(w[a][left], num_item)
            neg[todo[left]] = cand
            left = left[stored(todo[left], cand)]
        todo = todo[left]
    n_direct = len(todo)
    if n_direct:
        w2 = philox4x32_10(k_lo[todo], k_hi[todo], epoch, 2, k0, k1)
        for x, i in enumerate(todo):
            row = items[beg[i]:end[i]]
            if num_item - len(row) <= 0:
                neg[i] = 0
                continue
            t = int(to_range(w2[0][x], num_item - len(row)))
            neg[i] = t + np.searchsorted(row - np.arange(len(row)), t, side="right")     # first m with row[m] - m > t
    src_users = np.concatenate([pos_user, users])
    src_items = np.concatenate([pos_item, neg])
    src_labels = np.concatenate([np.ones(P, np.float32), np.zeros(P * num_ng, np.float32)])
    src, _ = perm(n, seed, epoch) if n else (np.zeros(0, np.int64), None)
    return src_users[src], src_items[src], src_labels[src], src, n_direct


# ------------------------------------------------------------------------------------------ the checkers
def check_validity(users, items, labels, positives, table_pairs, n_users, n_items, num_ng):
    """Exact: outputs in range, the label-1 samples are `positives` as a multiset, every user has num_ng x (its positives) label-0
    samples, and no label-0 item is in its user's row."""
    users, items, labels = np.asarray(users, np.int64), np.asarray(items, np.int64), np.asarray(labels)
    positives = np.asarray(positives, np.int64).reshape(-1, 2)
    assert len(users) == len(items) == len(labels) == len(positives) * (1 + num_ng)
    assert users.min() >= 0 and users.max() < n_users and items.min() >= 0 and items.max() < n_items
    assert np.isin(labels, (0, 1)).all()
    one = labels == 1
    assert np.array_equal(np.sort(users[one] * n_items + items[one]), np.sort(positives[:, 0] * n_items + positives[:, 1])), \
        "the label-1 samples are not the positives"
    assert np.array_equal(np.bincount(users[~one], minlength=n_users), num_ng * np.bincount(positives[:, 0], minlength=n_users)), \
        "a user does not have num_ng negatives per positive"
    table_pairs = np.asarray(table_pairs, np.int64).reshape(-1, 2)
    keys = np.unique(table_pairs[:, 0] * n_items + table_pairs[:, 1])
    assert not np.isin(users[~one] * n_items + items[~one], keys).any(), "a label-0 item is in its user's row"


def check_negative_law(users, items, labels, positives, table_pairs, n_users, n_items, num_ng):
    """Every (user, negative) cell against its binomial bound over the n slots: a slot is the negative j of user u with probability
    p = num_ng P_u / n / (n_items - deg_u) for j outside u's row (P_u: u's positives), 0 inside: within 6 sqrt(n p (1 - p)) of n p, and
    a probability-zero cell holds nothing.  Returns (largest deviation in sigma, smallest expected count, cells with p > 0)."""
    users, items, labels = np.asarray(users, np.int64), np.asarray(items, np.int64), np.asarray(labels)
    positives = np.asarray(positives, np.int64).reshape(-1, 2)
    table_pairs = np.asarray(table_pairs, np.int64).reshape(-1, 2)
    n = len(users)
    has = np.zeros((n_users, n_items), bool)
    has[table_pairs[:, 0], table_pairs[:, 1]] = True
    P_u = np.bincount(positives[:, 0], minlength=n_users)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_cell = num_ng * P_u / n / (n_items - has.sum(1))
    p = np.where(~has & (P_u > 0)[:, None], per_cell[:, None], 0.0)
    assert abs(p.sum() - num_ng / (1 + num_ng)) < 1e-12
    zero = labels == 0
    count = np.bincount(users[zero] * n_items + items[zero], minlength=p.size).reshape(p.shape)
    assert count[p == 0].sum() == 0, "a negative landed in a cell of probability zero"
    live = p > 0
    z = np.abs(count[live] - n * p[live]) / np.sqrt(n * p[live] * (1 - p[live]))
    worst = float(z.max())
    assert worst <= 6.0, f"a (user, negative) cell is {worst:.2f} standard deviations from its expectation"
    return worst, float((n * p[live]).min()), int(live.sum())


def check_shuffle_grid(src, grid=16):
    """slot i holds source src[i]: on a grid x grid partition of (slot bucket, source bucket), bucket = floor(index grid / n), every
    cell lies within 6 sqrt(n p (1 - p)) of n p, p = (slots in the bucket / n) (sources in the bucket / n).  Returns the largest
    deviation in sigma."""
    src = np.asarray(src, np.int64)
    n = len(src)
    assert np.array_equal(np.sort(src), np.arange(n)), "the shuffle is not a bijection"
    bucket = np.arange(n) * grid // n
    size = np.bincount(bucket, minlength=grid).astype(np.float64)
    count = np.bincount(bucket * grid + src * grid // n, minlength=grid * grid).reshape(grid, grid)
    p = np.outer(size, size) / float(n) ** 2
    z = np.abs(count - n * p) / np.sqrt(n * p * (1 - p))
    worst = float(z.max())
    assert worst <= 6.0, f"a (slot bucket, source bucket) cell is {worst:.2f} standard deviations from its expectation"
    return worst


def check_positives_per_batch(labels, num_ng, batch=256):
    """The label-1 samples per full batch of `batch`: Binomial(batch, q), q = 1 / (1 + num_ng), for a uniform shuffle — their mean
    within 6 standard errors of batch q, every batch within 6 sigma.  Returns (mean deviation in standard errors, largest batch
    deviation in sigma, variance over the binomial variance)."""
    labels = np.asarray(labels)
    nb = len(labels) // batch
    assert nb >= 1
    per = (labels[:nb * batch].reshape(nb, batch) == 1).sum(1)
    q = 1.0 / (1 + num_ng)
    sigma = np.sqrt(batch * q * (1 - q))
    z_mean = abs(per.mean() - batch * q) / (sigma / np.sqrt(nb))
    z_max = float(np.abs(per - batch * q).max() / sigma)
    assert z_mean <= 6.0, f"positives per batch: mean {per.mean():.3f}, {z_mean:.2f} standard errors from {batch * q:.3f}"
    assert z_max <= 6.0, f"positives per batch: a batch is {z_max:.2f} standard deviations from {batch * q:.3f}"
    return float(z_mean), z_max, float(per.var() / sigma ** 2)


# ------------------------------------------------------------------------------------------ graphs
def tiny_graph():
    """12 users x 23 items: user 7 holds nothing, the others 2 .. 8 random items.  Returns (pairs, n_users, n_items)."""
    rng = np.random.default_rng(3)
    n_users, n_items = 12, 23
    pairs = [(u, i) for u in range(n_users) if u != 7 for i in np.sort(rng.choice(n_items, 2 + u % 7, replace=False))]
    return np.array(pairs, np.int64), n_users, n_items


def host_epoch(pairs, n_users, n_items, repeat):
    """The host path on `pairs` repeated `repeat` times: LightTrainData.ng_sample() then dataloader_epoch_order.  Returns (users, items,
    labels, order, positives)."""
    import utility1.dataloader as dl
    positives = np.tile(pairs, (repeat, 1))
    mat = sp.csr_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n_users, n_items))
    td = dl.LightTrainData(positives.tolist(), n_items, mat.todok())
    td.ng_sample()
    order = dataloader_epoch_order(len(td.users_fill)).numpy()
    return td.users_fill[order], td.items_fill[order], np.asarray(td.labels_fill_np)[order], order, positives


# ------------------------------------------------------------------------------------------ 1. the shuffle is a bijection
@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 65, 96, 257, 4096, 4097])
def test_perm_is_a_bijection(n):
    assert half_bits(1) == 1 and half_bits(2) == 1 and half_bits(4) == 1 and half_bits(5) == 2 and half_bits(16) == 2
    assert half_bits(17) == 3 and half_bits(64) == 3 and half_bits(65) == 4 and half_bits(4096) == 6 and half_bits(4097) == 7
    assert n <= 1 << (2 * half_bits(n)) and (n <= 4 or 1 << (2 * half_bits(n)) < 4 * n)
    seen = set()
    for seed, epoch in ((0, 0), (0x123456789ABCDEF, 1), (77, 0x80000005), (0xFEDCBA9876543210, 2)):
        src, walks = perm(n, seed, epoch)
        assert np.array_equal(np.sort(src), np.arange(n)), (n, seed, epoch)
        assert walks.min() >= 1
        seen.add(tuple(src))
    if n >= 7:                                   # (n = 7: 5 040 orders; four keys coinciding would be a bug, not chance)
        assert len(seen) == 4


def test_round_keys_and_finaliser_are_the_documented_ones():
    # MurmurHash3 fmix32 known values: fmix32(0) = 0; fmix32(1) = 0x514E28B7 (the finaliser of the published reference code)
    assert int(fmix32(np.uint64(0))) == 0 and int(fmix32(np.uint64(1))) == 0x514E28B7
    K = round_keys(5, 9)
    a = philox4x32_10(0, 0, 9, 3, 5, 0)
    b = philox4x32_10(1, 0, 9, 3, 5, 0)
    assert K[:, 0].tolist() == [int(a[0][0]), int(a[1][0]), int(a[2][0]), int(a[3][0]), int(b[0][0]), int(b[1][0])]
    assert len(set(K[:, 0].tolist())) == 6
    assert not np.array_equal(round_keys(5, 10), K) and not np.array_equal(round_keys(5 + (1 << 32), 9), K)
    many = round_keys(5, [8, 9, 10])
    assert many.shape == (6, 3) and np.array_equal(many[:, 1:2], K)


# ------------------------------------------------------------------------------------------ 2. the checkers, on the host path
def test_checkers_accept_the_host_path_and_reject_wrong_laws():
    np.random.seed(5)
    torch.manual_seed(5)
    for name, (pairs, n_users, n_items), repeat in (("tiny", tiny_graph(), 100), ("law", law_graph(), 100)):
        users, items, labels, order, positives = host_epoch(pairs, n_users, n_items, repeat)
        check_validity(users, items, labels, positives, pairs, n_users, n_items, 5)
        worst, smallest, cells = check_negative_law(users, items, labels, positives, pairs, n_users, n_items, 5)
        grid = check_shuffle_grid(order)
        z_mean, z_max, ratio = check_positives_per_batch(labels, 5)
        print(f"host path, {name} graph: n {len(users)}, {cells} negative cells, worst {worst:.2f} sigma (smallest expectation {smallest:.0f}); "
              f"grid {grid:.2f} sigma; positives per batch: mean {z_mean:.2f} s.e., worst batch {z_max:.2f} sigma, variance ratio {ratio:.3f}")
        assert smallest > 30                 # (the normal approximation behind the 6 sigma bound: a Poisson-like cell of mean 30 passes
                                             # 30 + 6 sqrt(30) with probability ~1e-7, and cannot fall 6 sigma below)
    # (the law graph's last run stays in hand) — the checkers are not vacuous:
    n = len(users)
    ident = np.arange(n)                                                     # an identity shuffle: ng_sample's own order
    with pytest.raises(AssertionError, match="slot bucket"):
        check_shuffle_grid(ident)
    unshuffled = np.concatenate([np.ones(n // 6), np.zeros(n - n // 6)])
    with pytest.raises(AssertionError, match="positives per batch"):
        check_positives_per_batch(unshuffled, 5)
    with pytest.raises(AssertionError, match="bijection"):
        check_shuffle_grid(np.where(ident == 5, 6, ident))
    # negatives allowed inside the row: uniform over the whole catalogue
    rng = np.random.default_rng(0)
    bad = items.copy()
    zero = labels == 0
    bad[zero] = rng.integers(0, n_items, int(zero.sum()))
    with pytest.raises(AssertionError, match="probability zero"):
        check_negative_law(users, bad, labels, positives, pairs, n_users, n_items, 5)
    with pytest.raises(AssertionError, match="in its user's row"):
        check_validity(users, bad, labels, positives, pairs, n_users, n_items, 5)
    # a skewed negative law: user 4 (eight stored items, 500 draws expected per admissible item) never draws its first admissible item:
    # those draws are moved to its second
    adm = np.setdiff1d(np.arange(n_items), pairs[pairs[:, 0] == 4, 1])
    skew = items.copy()
    skew[zero & (users == 4) & (items == adm[0])] = adm[1]
    with pytest.raises(AssertionError, match="standard deviations"):
        check_negative_law(users, skew, labels, positives, pairs, n_users, n_items, 5)
    # a positive dropped for a negative
    lab = labels.copy()
    lab[np.flatnonzero(labels == 1)[0]] = 0
    with pytest.raises(AssertionError):
        check_validity(users, items, lab, positives, pairs, n_users, n_items, 5)


def test_restated_stream_has_the_reference_law_on_the_law_graph():
    """The NumPy restatement itself (the GPU tests hold the kernel to it bit for bit) through the same checkers; user 1 holds 15 of 16
    items, so most of its negatives take the direct draw."""
    pairs, n_users, n_items = law_graph()
    rowptr, items, _ = bpr_sampler_tables(pairs, n_users, n_items)
    positives = np.tile(pairs, (100, 1))
    u, i, y, src, n_direct = reference_epoch(rowptr, items, positives[:, 0], positives[:, 1], 5, n_items, 77, 3)
    check_validity(u, i, y, positives, pairs, n_users, n_items, 5)
    worst, smallest, cells = check_negative_law(u, i, y, positives, pairs, n_users, n_items, 5)
    grid = check_shuffle_grid(src)
    z_mean, z_max, ratio = check_positives_per_batch(y, 5)
    n_user1 = int(((u == 1) & (y == 0)).sum())
    print(f"restated stream: n {len(u)}, {cells} cells, worst {worst:.2f} sigma; grid {grid:.2f}; batches {z_mean:.2f} s.e. / {z_max:.2f} sigma / "
          f"ratio {ratio:.3f}; {n_direct} direct draws, user 1 has {n_user1} negatives")
    assert np.all(i[(u == 1) & (y == 0)] == 15)
    assert n_direct > 0.5 * n_user1                                         # (15/16)^8 = 0.60 of user 1's negatives


# ------------------------------------------------------------------------------------------ 3. small-n cells
@pytest.mark.parametrize("n", [7, 96])
def test_small_n_every_slot_source_cell_is_visited_uniformly(n):
    """Over E = 4 096 epochs (seed 77) slot i holds source j in Binomial(E, 1 / n) of them: every (slot, source) cell within
    6 sqrt(E p (1 - p)) of E p, none empty."""
    E, p = 4096, 1.0 / n
    src, _ = perm_many(n, 77, np.arange(E))
    count = np.bincount((np.tile(np.arange(n), E) * n + src.ravel()), minlength=n * n).reshape(n, n)
    assert count.sum(0).tolist() == [E] * n and count.sum(1).tolist() == [E] * n
    z = np.abs(count - E * p) / np.sqrt(E * p * (1 - p))
    print(f"n = {n}: {E} epochs, cells {count.min()} .. {count.max()} around {E * p:.1f}, largest deviation {z.max():.2f} sigma")
    assert count.min() > 0
    assert z.max() <= 6.0


# ------------------------------------------------------------------------------------------ 4. the sampler object's host side
def test_sampler_refuses_what_the_tables_refuse():
    ok = [(0, 0), (1, 2)]
    for bad in ([(3, 0)], [(-1, 0)], [(0, 4)], [(0, -1)]):
        with pytest.raises(ValueError, match="out of range"):
            BceDeviceSampler(np.array(ok + bad), 3, 4, device="cpu")
    with pytest.raises(ValueError, match="every item"):
        BceDeviceSampler(np.array([(2, 0), (2, 1), (2, 2), (2, 3), (2, 3), (0, 1)]), 3, 4, device="cpu")
    with pytest.raises(ValueError, match="num_ng"):
        BceDeviceSampler(np.array(ok), 3, 4, num_ng=0, device="cpu")
    s = BceDeviceSampler(np.array(ok + [(1, 2)]), 3, 4, num_ng=2, seed=9, device="cpu")      # duplicates are kept as samples
    assert (s.n_pos, s.num_ng, s.n, s.n_items, s.seed) == (3, 2, 9, 4, 9)
    assert s.pos_user.tolist() == [0, 1, 1] and s.pos_item.tolist() == [0, 2, 2] and s.pos_user.dtype == torch.int32
    assert s.rowptr.tolist() == [0, 1, 2, 2] and s.items.tolist() == [0, 2]
    assert not callable(s) and not hasattr(s, "ng_sample")
    bufs = s.epoch_buffers()
    assert [b.dtype for b in bufs] == [torch.int64, torch.int64, torch.float32] and all(b.shape == (9,) for b in bufs)
    assert s.epoch_buffers()[0] is bufs[0]


def test_sampler_from_train_data_keeps_the_positives_in_order():
    import utility1.dataloader as dl
    pairs, n_users, n_items = tiny_graph()
    td = dl.LightTrainData(pairs.tolist(), n_items, None)
    s = BceDeviceSampler.from_train_data(td, n_users=n_users, seed=4, device="cpu")
    assert s.num_ng == 5 and s.n_items == n_items and s.n == 6 * len(pairs) and s.seed == 4
    assert np.array_equal(s.pos_user.numpy(), pairs[:, 0]) and np.array_equal(s.pos_item.numpy(), pairs[:, 1])
    assert s.rowptr.numel() == n_users + 1
    assert BceDeviceSampler.from_train_data(td, device="cpu").rowptr.numel() == int(pairs[:, 0].max()) + 2
