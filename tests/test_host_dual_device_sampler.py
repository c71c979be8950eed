"""Host side of the device dual-task path sampler (no GPU): a NumPy restatement of the law include/spex_hip.h writes down at
spex_sample_dual_task_paths (reference_paths — test_gpu_dual_device_sampler.py holds the kernel to it bit for bit), the path tables
against the driver's index, the selection's exact properties, and the inclusion law of the cut — validated on the reference's own
random.sample (trainer.dual_task_epoch_paths) and shown to reject wrong laws.

Bounds are the binomial law's own: over K batch keys a candidate of a batch with `total` candidates is among the cap chosen in
Binomial(K, cap / total) of them, and in the first slot in Binomial(K, 1 / total); every such count must lie within 5 standard
deviations of its mean."""
import importlib.util
import os
import random
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_host_bce_device_sampler import fmix32, half_bits
from test_host_bpr_device_sampler import philox4x32_10

from spex_amd.trainer import DualDeviceSampler, dual_sampler_tables, dual_task_epoch_paths

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ the documented law, in NumPy
def batch_round_keys(seed, epoch, ks):
    """K[0 .. 3] = the four words of counter (k, 0, epoch, 4), K[4 .. 5] = words 0 and 1 of counter (k, 1, epoch, 4); key = seed.
    For an array of batch indices: uint64 [6, len(ks)]."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    ks = np.atleast_1d(np.asarray(ks, np.uint64))
    a = philox4x32_10(ks, 0, epoch, 4, k0, k1)
    b = philox4x32_10(ks, 1, epoch, 4, k0, k1)
    return np.stack([a[0], a[1], a[2], a[3], b[0], b[1]])


def perm_slots(total, n_slots, seed, epoch, ks):
    """perm_k(t) for t in [0, n_slots) and every batch index of `ks` ([len(ks), n_slots]) on the domain [0, total): six rounds of
    (L, R) <- (R, L ^ (fmix32(R ^ K[r]) & mask)) on x = (L << h) | R, repeated while x >= total."""
    h = np.uint64(half_bits(total))
    mask = (np.uint64(1) << h) - np.uint64(1)
    K = batch_round_keys(seed, epoch, ks)                             # [6, E]
    E = K.shape[1]
    x = np.tile(np.arange(n_slots, dtype=np.uint64), E)
    row = np.repeat(np.arange(E), n_slots)
    todo = np.arange(E * n_slots)
    while len(todo):
        L, R = x[todo] >> h, x[todo] & mask
        for r in range(6):
            L, R = R, L ^ (fmix32(R ^ K[r][row[todo]]) & mask)
        x[todo] = (L << h) | R
        todo = todo[x[todo] >= np.uint64(total)]
    return x.astype(np.int64).reshape(E, n_slots)


def batch_candidates(users, rowptr, idx):
    """(c, off, total) of one batch and its candidate list in order of q."""
    users = np.asarray(users, np.int64)
    rowptr = np.asarray(rowptr, np.int64)
    n_rows = len(rowptr) - 1
    first = np.zeros(len(users), bool)
    first[np.unique(users, return_index=True)[1]] = True
    inside = (users >= 0) & (users < n_rows)
    safe = np.where(inside, users, 0)
    c = np.where(first & inside, rowptr[safe + 1] - rowptr[safe], 0)
    off = np.cumsum(c) - c
    return c, off, int(c.sum()), safe


def reference_paths(users, B, rowptr, idx, cap, seed, epoch, max_steps=None):
    """spex_sample_dual_task_paths as include/spex_hip.h words it: the chosen path ids of every batch, slot by slot (a list of int64
    arrays) and the counts (int32)."""
    users, idx = np.asarray(users, np.int64), np.asarray(idx, np.int64)
    rowptr = np.asarray(rowptr, np.int64)
    n = len(users)
    n_batches = -(-n // B)
    if max_steps is not None and max_steps >= 0:
        n_batches = min(n_batches, max_steps)
    chosen, count = [], np.zeros(n_batches, np.int32)
    for k in range(n_batches):
        u = users[k * B:(k + 1) * B]
        c, off, total, safe = batch_candidates(u, rowptr, idx)
        T = min(total, cap)
        count[k] = T
        if T == 0:
            chosen.append(np.zeros(0, np.int64))
            continue
        q = np.arange(T) if total <= cap else perm_slots(total, T, seed, epoch, [k])[0]
        j = np.searchsorted(off, q, side="right") - 1                 # the last j with off_j <= q: its count is positive
        assert np.all(c[j] > 0) and np.all(q < off[j] + c[j])
        chosen.append(idx[rowptr[safe[j]] + q - off[j]])
    return chosen, count


# ------------------------------------------------------------------------------------------ fixtures
def epinion2_paths(golden):
    t = golden("trust_epinion2_paths")
    return [r[:l].tolist() for r, l in zip(t["train_paths"].astype(np.int64), t["train_len"])], t["train_targets"].astype(np.int64).tolist()


def driver_index():
    """paths_by_first_user of tests/drivers/dual_driver.py (the module parses its command line on import)."""
    argv = sys.argv
    sys.argv = ["dual_driver"]
    try:
        spec = importlib.util.spec_from_file_location("_dual_driver_for_tables", os.path.join(REPO, "tests", "drivers", "dual_driver.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod.paths_by_first_user


class FakeTrust:
    """The three fields of utility2.utils.Data the sampler reads."""

    def __init__(self, paths, targets, pad, width=None):
        width = width or max([len(p) for p in paths] + [1])
        self.inputs = np.full((len(paths), width), pad, np.int64)
        self.mask = np.zeros((len(paths), width), np.int64)
        for r, p in enumerate(paths):
            self.inputs[r, :len(p)] = p
            self.mask[r, :len(p)] = 1
        self.targets = np.asarray(targets, np.int64)


# ------------------------------------------------------------------------------------------ 1. the tables
def test_tables_equal_the_drivers_index(golden):
    by_first = driver_index()
    paths, _ = epinion2_paths(golden)
    cases = [(paths, 3186), (paths, None),
             ([[4, 1], [0, 2, 3], [4, 0], [0, 9], [6, 6, 6]], 9),          # users 1, 2, 3, 5, 7, 8 hold no path
             ([], 3), ([], None)]
    for ps, rows in cases:
        rowptr, idx = dual_sampler_tables(ps, rows)
        want = by_first(ps)
        n_rows = len(rowptr) - 1
        assert rowptr.dtype == np.int32 and idx.dtype == np.int32 and rowptr[0] == 0 and rowptr[-1] == len(ps) == len(idx)
        assert n_rows == (rows if rows is not None else (max(p[0] for p in ps) + 1 if ps else 0))
        for u in range(n_rows):
            assert idx[rowptr[u]:rowptr[u + 1]].tolist() == list(want.get(u, [])), u
        assert sum(len(v) for v in want.values()) == len(idx)
    # a padded array reads the same as the lists
    ft = FakeTrust(cases[2][0], [0] * 5, pad=9)
    assert all(np.array_equal(a, b) for a, b in zip(dual_sampler_tables(ft.inputs, 9), dual_sampler_tables(cases[2][0], 9)))
    with pytest.raises(ValueError, match="out of range"):
        dual_sampler_tables([[3, 1]], 3)
    with pytest.raises(ValueError, match="out of range"):
        dual_sampler_tables([[-1, 1]], 3)


# ------------------------------------------------------------------------------------------ 2. the selection's exact properties
def test_restated_selection_is_distinct_and_starts_at_the_batchs_users(golden):
    paths, _ = epinion2_paths(golden)
    rowptr, idx = dual_sampler_tables(paths, 3186)
    first = np.array([p[0] for p in paths])
    rng = np.random.default_rng(1)
    for B, cap in ((256, 15), (7, 3), (300, 1)):
        users = rng.integers(0, 3186, 40 * B + 5)
        chosen, count = reference_paths(users, B, rowptr, idx, cap, seed=2020, epoch=3)
        assert len(chosen) == 41 and count.dtype == np.int32
        cut = 0
        for k, (ch, T) in enumerate(zip(chosen, count)):
            u = users[k * B:(k + 1) * B]
            every = np.flatnonzero(np.isin(first, u))                     # the reference's candidates (main_auto_expert_s.py:64-69)
            assert T == len(ch) == min(len(every), cap)
            assert len(set(ch.tolist())) == len(ch) and np.isin(ch, every).all()
            if len(every) <= cap:                                         # not cut: all of them, grouped by first occurrence of the user
                assert sorted(ch.tolist()) == every.tolist()
            cut += len(every) > cap
        assert cut > 20
    # a bounded draw is a prefix of the full one; seed and epoch change the cut, not the counts
    users = rng.integers(0, 3186, 20 * 256)
    full = reference_paths(users, 256, rowptr, idx, 15, 7, 0)
    head = reference_paths(users, 256, rowptr, idx, 15, 7, 0, max_steps=6)
    assert len(head[0]) == 6 and all(np.array_equal(a, b) for a, b in zip(head[0], full[0])) and np.array_equal(head[1], full[1][:6])
    for other in (reference_paths(users, 256, rowptr, idx, 15, 8, 0), reference_paths(users, 256, rowptr, idx, 15, 7, 1)):
        assert np.array_equal(other[1], full[1]) and not all(np.array_equal(a, b) for a, b in zip(other[0], full[0]))


def test_restatement_on_crafted_batches():
    """Duplicates count once (at their first position), users without paths and users outside the table count nothing, and the three
    sides of the cap: total == 0, total == cap, total == cap + 1."""
    rowptr, idx = dual_sampler_tables([[0, 1], [2, 1], [0, 3], [2, 9], [2, 4], [5, 5]], 6)          # user 0: {0, 2}; 2: {1, 3, 4}; 5: {5}
    ref = lambda u, cap: reference_paths(u, len(u), rowptr, idx, cap, 1, 0)
    ch, cnt = ref([2, 2, 0, 2, 0], 5)
    assert cnt.tolist() == [5] and ch[0].tolist() == [1, 3, 4, 0, 2]                                # total == cap: in candidate order
    ch, cnt = ref([1, 3, 4, -1, 6, 99], 5)
    assert cnt.tolist() == [0] and len(ch[0]) == 0                                                   # total == 0
    ch, cnt = ref([5, 7, 2, 5, 0, 2], 5)
    assert cnt.tolist() == [5] and len(set(ch[0].tolist())) == 5 and set(ch[0].tolist()) <= {5, 1, 3, 4, 0, 2}    # total == cap + 1: cut
    ch, cnt = ref([5, 7, 2, 5, 0, 2], 0)
    assert cnt.tolist() == [0]


# ------------------------------------------------------------------------------------------ 3. the inclusion law of the cut
TOTALS, CAP, KEYS = (16, 17, 40, 257), 15, 8000


def check_inclusion(sel, total, cap=CAP):
    """sel [K, cap]: the candidates chosen for K batch keys out of [0, total).  Every row distinct; every candidate's inclusion count
    within 5 sqrt(K p (1 - p)) of K p, p = cap / total; likewise its first-slot count with p = 1 / total.  Returns the two largest
    deviations in sigma."""
    sel = np.asarray(sel, np.int64)
    K = len(sel)
    assert sel.shape == (K, cap) and sel.min() >= 0 and sel.max() < total
    assert (np.diff(np.sort(sel, axis=1), axis=1) > 0).all(), "a batch's chosen candidates are not distinct"
    worst = []
    for name, counts, p in (("inclusion", np.bincount(sel.ravel(), minlength=total), cap / total),
                            ("first slot", np.bincount(sel[:, 0], minlength=total), 1.0 / total)):
        z = np.abs(counts - K * p) / np.sqrt(K * p * (1 - p))
        worst.append(float(z.max()))
        assert worst[-1] <= 5.0, f"total {total}: a candidate's {name} count is {worst[-1]:.2f} standard deviations from its expectation"
    return tuple(worst)


def test_inclusion_law_of_the_keyed_cut_and_of_random_sample():
    """total in {16, 17, 40, 257}, cap 15, 8 000 batch keys each.  Observed with the batch keys (seed 2020, epoch 0, batch k = the
    key index), largest |z| (inclusion / first slot) per total: 16: 2.26 / 1.85, 17: 1.94 / 1.83, 40: 2.31 / 2.01, 257: 3.62 / 2.85 —
    3.62 and 2.85 over all; the reference's random.sample under random.seed(5): 3.39 / 3.08 (both at total 257)."""
    figs = {}
    for total in TOTALS:
        sel = perm_slots(total, CAP, 2020, 0, np.arange(KEYS))
        figs[total] = check_inclusion(sel, total)
    print("keyed cut, |z| max (inclusion, first slot) per total:", {k: tuple(round(x, 2) for x in v) for k, v in figs.items()})
    # the same checker takes the reference's law: trainer.dual_task_epoch_paths (random.sample) on one user holding `total` paths
    state = random.getstate()
    random.seed(5)
    try:
        ref = {}
        for total in TOTALS:
            chosen = dual_task_epoch_paths([np.array([0])] * KEYS, {0: list(range(total))}, CAP)
            ref[total] = check_inclusion(np.array(chosen), total)
    finally:
        random.setstate(state)
    print("random.sample, |z| max (inclusion, first slot) per total:", {k: tuple(round(x, 2) for x in v) for k, v in ref.items()})
    # ... and rejects two wrong laws
    rng = np.random.default_rng(0)
    for total in TOTALS:
        with pytest.raises(AssertionError, match="inclusion count"):
            check_inclusion(np.tile(np.arange(CAP), (KEYS, 1)), total)                     # always the first cap candidates
        with pytest.raises(AssertionError, match="not distinct"):
            check_inclusion(rng.integers(0, total, (KEYS, CAP)), total)                    # sampling with replacement


def test_batch_keys_are_the_documented_ones():
    K = batch_round_keys(5, 9, [7])
    a, b = philox4x32_10(7, 0, 9, 4, 5, 0), philox4x32_10(7, 1, 9, 4, 5, 0)
    assert K[:, 0].tolist() == [int(a[0][0]), int(a[1][0]), int(a[2][0]), int(a[3][0]), int(b[0][0]), int(b[1][0])]
    assert not np.array_equal(batch_round_keys(5, 9, [8]), K) and not np.array_equal(batch_round_keys(5, 10, [7]), K)
    assert not np.array_equal(batch_round_keys(5 + (1 << 32), 9, [7]), K)
    many = batch_round_keys(5, 9, [6, 7, 8])
    assert many.shape == (6, 3) and np.array_equal(many[:, 1:2], K)
    for total in (2, 3, 16, 17, 300):                                   # a bijection of [0, total) for every batch key
        full = perm_slots(total, total, 5, 9, [0, 1, 2])
        assert all(np.array_equal(np.sort(r), np.arange(total)) for r in full)


# ------------------------------------------------------------------------------------------ 4. the sampler object's host side
def test_sampler_refuses_what_the_bce_sampler_refuses():
    ok = [(0, 0), (1, 2)]
    trust = FakeTrust([[1, 0], [0, 2, 1], [1, 2]], [2, 1, 0], pad=2, width=4)
    for bad in ([(3, 0)], [(-1, 0)], [(0, 4)], [(0, -1)]):
        with pytest.raises(ValueError, match="out of range"):
            DualDeviceSampler(np.array(ok + bad), 3, 4, trust, 15, 256, device="cpu")
    with pytest.raises(ValueError, match="every item"):
        DualDeviceSampler(np.array([(2, 0), (2, 1), (2, 2), (2, 3), (2, 3), (0, 1)]), 3, 4, trust, 15, 256, device="cpu")
    with pytest.raises(ValueError, match="num_ng"):
        DualDeviceSampler(np.array(ok), 3, 4, trust, 15, 256, num_ng=0, device="cpu")
    for cap, B in ((-1, 256), (15, 0), (15, 4097)):
        with pytest.raises(ValueError, match="cap"):
            DualDeviceSampler(np.array(ok), 3, 4, trust, cap, B, device="cpu")
    with pytest.raises(ValueError, match="first node is out of range"):
        DualDeviceSampler(np.array(ok), 3, 4, FakeTrust([[3, 0]], [1], pad=2), 15, 256, device="cpu")
    s = DualDeviceSampler(np.array(ok + [(1, 2)]), 3, 4, trust, 15, 4, num_ng=2, seed=9, device="cpu")
    assert (s.n, s.cap, s.batch_size, s.n_batches, s.seed, s.n_paths, s.path_len) == (9, 15, 4, 3, 9, 3, 4)
    assert (s.bce.n_pos, s.bce.num_ng, s.bce.seed) == (3, 2, 9) and s.bce.pos_user.tolist() == [0, 1, 1]
    assert s.path_rowptr.tolist() == [0, 1, 3, 3] and s.path_idx.tolist() == [1, 0, 2] and s.path_rowptr.dtype == torch.int32
    assert s.paths.tolist() == [[1, 0, 2, 2], [0, 2, 1, 2], [1, 2, 2, 2]] and s.path_l.tolist() == [2, 3, 2] and s.path_tgt.tolist() == [2, 1, 0]
    assert s.paths.dtype == s.path_l.dtype == s.path_tgt.dtype == torch.int64
    assert not callable(s) and not hasattr(s, "ng_sample")
    with pytest.raises(ValueError, match="GPU only"):
        s.draw(0)


def test_sampler_from_train_data_and_a_trust_data(golden):
    import utility1.dataloader as dl
    from utility2.utils import Data
    rng = np.random.default_rng(3)
    n_users, n_items = 12, 23
    pairs = np.array([(u, i) for u in range(n_users) if u != 7 for i in np.sort(rng.choice(n_items, 2 + u % 7, replace=False))], np.int64)
    td = dl.LightTrainData(pairs.tolist(), n_items, None)
    raw = ([[3, 1, 4], [0, 5], [3, 2], [11, 0, 1, 2]], [5, 6, 7, 8])
    trust = Data(raw, n_users, shuffle=False)
    s = DualDeviceSampler.from_train_data(td, trust, 15, 256, n_users=n_users + 1, seed=4, device="cpu")
    assert s.bce.num_ng == 5 and s.bce.n_items == n_items and s.n == 6 * len(pairs) and s.seed == 4 and s.path_len == trust.len_max == 4
    assert np.array_equal(s.bce.pos_user.numpy(), pairs[:, 0]) and s.path_rowptr.numel() == n_users + 2
    assert s.paths.numpy().tolist() == np.asarray(trust.inputs).tolist() and s.path_l.tolist() == [3, 2, 2, 4] and s.path_tgt.tolist() == [5, 6, 7, 8]
    assert s.paths[1].tolist() == [0, 5, n_users, n_users]                  # padded with the pad row
    assert s.path_idx.tolist() == [1, 0, 2, 3]
    assert DualDeviceSampler.from_train_data(td, trust, 15, 256, device="cpu").path_rowptr.numel() == 13
