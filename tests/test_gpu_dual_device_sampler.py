"""Dual-task epochs drawn on the device: the per-batch trust-path selection (spex_sample_dual_task_paths), the strided epoch call
(spex_dual_task_epoch_strided_f32) and what trainer builds on them (DualDeviceSampler, train_epoch_dual / train_epochs_dual with a
sampler).

The law is restated in NumPy from the text of include/spex_hip.h (test_host_dual_device_sampler.reference_paths) and the kernel must
reproduce it bit for bit: counts, rows, and a sentinel left in every slot past a batch's count.  The training comparisons use the
DETERMINISTIC step and issue the same launches on both sides, so parameters, moments and both loss sums are compared with
torch.equal."""
import ctypes
import random
import threading

import numpy as np
import pytest
import torch

from test_host_bce_device_sampler import reference_epoch
from test_host_dual_device_sampler import FakeTrust, batch_candidates, epinion2_paths, reference_paths

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
N_U, N_I = 3186, 12407
SENTINEL = -7

_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    from spex_amd.datasets import materialise_epinion2
    return materialise_epinion2(str(tmp_path_factory.mktemp("data")))


# ------------------------------------------------------------------------------------------ synthetic tables, no model
N_ROWS = 1100
U_ONE, U_CAP, U_CAP1, U_TWO = 1, 2, 3, 4          # users holding exactly 1, 15, 16 and 2 paths


def synthetic(path_len):
    """1 100 user rows, most of them without a path: user 1 holds 1 path, user 2 15, user 3 16, user 4 2, every seventh user from 7 on
    1 .. 5.  Paths of 1 .. path_len nodes padded with N_ROWS - 1; ids are dealt in a shuffled order, so a user's ids are not a run."""
    key = ("syn", path_len)
    if key not in _cache:
        from spex_amd.trainer import dual_sampler_tables
        rng = np.random.default_rng(path_len)
        firsts = [U_ONE] + [U_CAP] * 15 + [U_CAP1] * 16 + [U_TWO] * 2 + [u for u in range(7, N_ROWS - 1, 7) for _ in range(1 + u % 5)]
        firsts = np.array(firsts)[rng.permutation(len(firsts))]
        paths = [[int(f)] + rng.integers(0, N_ROWS - 1, int(rng.integers(0, path_len))).tolist() for f in firsts]
        trust = FakeTrust(paths, rng.integers(0, N_ROWS - 1, len(paths)), pad=N_ROWS - 1, width=path_len)
        rowptr, idx = dual_sampler_tables(trust.inputs, N_ROWS)
        assert [rowptr[u + 1] - rowptr[u] for u in (U_ONE, U_CAP, U_CAP1, U_TWO, 5, 7)] == [1, 15, 16, 2, 0, 3]
        _cache[key] = (trust, rowptr, idx)
    return _cache[key]


def device_tables(path_len):
    key = ("syn-dev", path_len)
    if key not in _cache:
        trust, rowptr, idx = synthetic(path_len)
        _cache[key] = (t(rowptr), t(idx), t(trust.inputs), t(trust.mask.sum(1)), t(trust.targets))
    return _cache[key]


def crafted_users(B):
    """Whole batches of B: all samples one user (total 15 == cap, 16 == cap + 1, 1, 2: the three sides of cap 1 and cap 15), all
    distinct users, users without paths only (total == 0), indices outside [0, N_ROWS) only, a mix of everything; then random batches
    and a ragged tail (n is no multiple of B for B > 1)."""
    rng = np.random.default_rng(B)
    outside = np.array([-1, N_ROWS, N_ROWS + 5, 1 << 40, -(1 << 35)])
    no_path = np.array([0, 5, 6, 8, 9, 10, 1099])
    mix = np.concatenate([outside, no_path, [U_ONE, U_CAP, U_TWO, U_CAP, 14, 21, 14]])
    batches = [np.full(B, U_CAP), np.full(B, U_CAP1), np.full(B, U_ONE), np.full(B, U_TWO), np.arange(B), np.arange(B)[::-1] + 3,
               no_path[rng.integers(0, len(no_path), B)], outside[rng.integers(0, len(outside), B)], mix[rng.integers(0, len(mix), B)],
               rng.integers(-3, N_ROWS + 3, B), rng.integers(0, 40, B), rng.integers(0, N_ROWS, B)]
    tail = rng.integers(0, N_ROWS, max(1, B // 2) if B > 1 else 1)
    return np.concatenate(batches + [tail]).astype(np.int64)


def run_kernel(users, B, tables, cap, path_len, seed, epoch, max_steps=None, n_out=None):
    """ops.sample_dual_task_paths into sentinel-filled outputs of n_out batches (default: as many as are drawn)."""
    from spex_amd import ops
    n_batches = -(-len(users) // B)
    n_out = n_out if n_out is not None else (n_batches if max_steps is None else min(n_batches, max_steps))
    full = lambda *shape, dt=torch.int64: torch.full(shape, SENTINEL, dtype=dt, device=DEV)
    out = (full(n_out * cap, path_len), full(n_out * cap), full(n_out * cap), full(n_out, dt=torch.int32))
    ops.sample_dual_task_paths(t(users), B, *tables, cap, seed, epoch, max_steps=max_steps, out=out)
    return tuple(x.cpu().numpy() for x in out)


def check_against_restatement(got, users, B, trust, rowptr, idx, cap, seed, epoch, max_steps=None):
    seq, seq_l, tgt, count = got
    chosen, want_count = reference_paths(users, B, rowptr, idx, cap, seed, epoch, max_steps)
    assert np.array_equal(count[:len(want_count)], want_count), (count[:len(want_count)].tolist(), want_count.tolist())
    lengths = trust.mask.sum(1)
    for k, ch in enumerate(chosen):
        rows = slice(k * cap, k * cap + len(ch))
        assert np.array_equal(seq[rows], trust.inputs[ch]) and np.array_equal(seq_l[rows], lengths[ch]) and np.array_equal(tgt[rows], trust.targets[ch]), k
        rest = slice(k * cap + len(ch), (k + 1) * cap)
        assert (seq[rest] == SENTINEL).all() and (seq_l[rest] == SENTINEL).all() and (tgt[rest] == SENTINEL).all(), k
    done = len(chosen)
    assert (count[done:] == SENTINEL).all() and (seq[done * cap:] == SENTINEL).all() and (seq_l[done * cap:] == SENTINEL).all()
    return chosen, want_count


# ------------------------------------------------------------------------------------------ 1. bit-exactness
@pytest.mark.parametrize("path_len", [1, 5, 16])
@pytest.mark.parametrize("cap", [1, 15])
@pytest.mark.parametrize("B", [1, 3, 64, 65, 256, 300, 1024])
def test_kernel_reproduces_the_documented_law(B, cap, path_len):
    (trust, rowptr, idx), tables = synthetic(path_len), device_tables(path_len)
    users = crafted_users(B)
    assert B == 1 or len(users) % B != 0
    seed, epoch = 0xFEDCBA9876543210, 0x80000005                      # both key words and the epoch word's top bit in use
    got = run_kernel(users, B, tables, cap, path_len, seed, epoch)
    chosen, count = check_against_restatement(got, users, B, trust, rowptr, idx, cap, seed, epoch)
    totals = [batch_candidates(users[k * B:(k + 1) * B], rowptr, idx)[2] for k in range(len(count))]
    assert totals[:4] == [15, 16, 1, 2] and totals[6] == 0 and totals[7] == 0               # the crafted batches are what they claim
    assert count.tolist() == [min(x, cap) for x in totals]
    assert {cap, cap + 1} <= set(totals) and 0 in totals                                   # total == cap, == cap + 1, == 0
    if B >= 64:
        assert totals[4] > 2 * cap                                                         # all-distinct users: a deep cut
    for ch in chosen:
        assert len(set(ch.tolist())) == len(ch)


def test_a_batch_at_the_largest_supported_size():
    """B = 4 096 (the third instance of the kernel: 65 KB of LDS), 1 100 distinct users at most: every sample a duplicate many times over."""
    (trust, rowptr, idx), tables = synthetic(5), device_tables(5)
    rng = np.random.default_rng(0)
    users = np.concatenate([rng.integers(-2, N_ROWS + 2, 4096), np.arange(4096) % N_ROWS, rng.integers(0, N_ROWS, 1000)]).astype(np.int64)
    for B in (4096, 1025):
        got = run_kernel(users, B, tables, 15, 5, 11, 2)
        _, count = check_against_restatement(got, users, B, trust, rowptr, idx, 15, 11, 2)
        assert (count == 15).all()


# ------------------------------------------------------------------------------------------ 2. stream and argument properties
def test_max_steps_prefix_and_seed_and_epoch():
    (trust, rowptr, idx), tables = synthetic(5), device_tables(5)
    users = np.random.default_rng(4).integers(0, N_ROWS, 64 * 20 + 9).astype(np.int64)
    full = run_kernel(users, 64, tables, 15, 5, 7, 0)
    assert (full[3][:19] == 15).all() and full[3][19:].tolist() == [8, 0]           # 19 batches are cut, one is not, the ragged one is empty
    head = run_kernel(users, 64, tables, 15, 5, 7, 0, max_steps=6, n_out=21)
    check_against_restatement(head, users, 64, trust, rowptr, idx, 15, 7, 0, max_steps=6)
    assert all(np.array_equal(head[i][:6 * 15], full[i][:6 * 15]) for i in range(3)) and np.array_equal(head[3][:6], full[3][:6])
    again = run_kernel(users, 64, tables, 15, 5, 7, 0)
    other_seed, other_epoch = run_kernel(users, 64, tables, 15, 5, 8, 0), run_kernel(users, 64, tables, 15, 5, 7, 1)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    for other in (other_seed, other_epoch):
        assert np.array_equal(other[3], full[3]) and not np.array_equal(other[0], full[0])
        assert (other[0].reshape(21, -1) != full[0].reshape(21, -1)).any(1)[:19].all()      # every cut batch is cut otherwise
        assert np.array_equal(other[0][19 * 15:], full[0][19 * 15:])                        # ... and the uncut one is the same
    assert run_kernel(users, 64, tables, 15, 5, 7 + (1 << 32), 0)[0].tolist() != full[0].tolist()      # the key's high word counts
    # max_steps = 0 and cap = 0
    none = run_kernel(users, 64, tables, 15, 5, 7, 0, max_steps=0, n_out=2)
    assert all((x == SENTINEL).all() for x in none)
    zero = run_kernel(users, 64, tables, 0, 5, 7, 0)
    assert zero[3].tolist() == [0] * 21 and zero[0].size == 0


def test_rejected_arguments_return_a_negative_status_and_touch_nothing():
    from spex_amd import _lib
    lib = _lib.load()
    (trust, rowptr, idx), tables = synthetic(5), device_tables(5)
    users = t(np.arange(200, dtype=np.int64))
    out = (torch.full((4 * 15, 5), SENTINEL, dtype=torch.int64, device=DEV), torch.full((60,), SENTINEL, dtype=torch.int64, device=DEV),
           torch.full((60,), SENTINEL, dtype=torch.int64, device=DEV), torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV))
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    good = dict(users=vp(users), n=200, B=64, max_steps=-1, rowptr=vp(tables[0]), n_rows=N_ROWS, idx=vp(tables[1]), n_paths=tables[1].numel(),
                paths=vp(tables[2]), path_len=5, path_l=vp(tables[3]), path_tgt=vp(tables[4]), cap=15, seq=vp(out[0]), seq_l=vp(out[1]),
                targets=vp(out[2]), count=vp(out[3]))

    def call(**kw):
        k = dict(good, **kw)
        rc = lib.spex_sample_dual_task_paths(k["users"], k["n"], k["B"], k["max_steps"], k["rowptr"], k["n_rows"], k["idx"], k["n_paths"], k["paths"],
                                             k["path_len"], k["path_l"], k["path_tgt"], k["cap"], 5, 0, k["seq"], k["seq_l"], k["targets"], k["count"],
                                             None)
        return rc, lib.spex_last_error().decode()

    cases = [dict(users=None), dict(rowptr=None), dict(idx=None), dict(paths=None), dict(path_l=None), dict(path_tgt=None), dict(seq=None),
             dict(seq_l=None), dict(targets=None), dict(count=None), dict(B=0), dict(B=-1), dict(B=4097), dict(n=-1), dict(cap=-1),
             dict(path_len=0), dict(n_rows=-1), dict(n_paths=-1)]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "spex_sample_dual_task_paths" in msg, (kw, rc, msg)
    assert "NULL" in call(count=None)[1] and "4096" in call(B=4097)[1] and "cap" in call(cap=-1)[1]
    torch.cuda.synchronize()
    assert all(bool((x == SENTINEL).all()) for x in out)
    for kw in (dict(n=0), dict(max_steps=0)):                         # nothing to draw: OK, nothing launched
        assert call(**kw)[0] == 0
    torch.cuda.synchronize()
    assert all(bool((x == SENTINEL).all()) for x in out)
    assert call(cap=0)[0] == 0                                        # only the counts
    torch.cuda.synchronize()
    assert out[3].tolist() == [0] * 4 and all(bool((x == SENTINEL).all()) for x in out[:3])
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert (out[3] >= 0).all() and out[3].max().item() == 15


# ------------------------------------------------------------------------------------------ 3. Epinion2, B = 256, cap = 15
def epi_trust(golden):
    if "trust" not in _cache:
        from utility2.utils import Data
        _cache["trust"] = Data(epinion2_paths(golden), N_U - 1, shuffle=False)
    return _cache["trust"]


def test_epinion2_epoch_every_batch_takes_fifteen_distinct_paths_of_its_users(epinion2, golden):
    from spex_amd.trainer import DualDeviceSampler
    trust = epi_trust(golden)
    s = DualDeviceSampler(epinion2["train"][:, :2], N_U, N_I, trust, 15, 256, seed=2020, device=DEV)
    assert s.n == 1255824 and s.n_batches == 4906 and s.n_paths == 27004
    users, items, labels, seq, seq_l, tgt, count = (x.cpu().numpy() for x in s.draw(0))
    again = s.draw(0)
    assert torch.equal(again[3], t(seq)) and torch.equal(again[6], t(count))
    bce = s.bce.draw(0)
    assert np.array_equal(bce[0].cpu().numpy(), users) and np.array_equal(bce[1].cpu().numpy(), items)       # one seed serves both samplers
    assert count.shape == (4906,) and (count == 15).all()
    rowptr, idx = s.path_rowptr.cpu().numpy(), s.path_idx.cpu().numpy()
    chosen, want_count = reference_paths(users, 256, rowptr, idx, 15, 2020, 0)
    first = np.asarray(trust.inputs)[:, 0]
    every = np.bincount(first, minlength=N_U)
    assert (want_count == 15).all()
    ids = np.stack(chosen)
    assert np.array_equal(seq, np.asarray(trust.inputs)[ids.ravel()])
    assert np.array_equal(seq_l, np.asarray(trust.mask).sum(1)[ids.ravel()]) and np.array_equal(tgt, np.asarray(trust.targets)[ids.ravel()])
    assert (np.diff(np.sort(ids, axis=1), axis=1) > 0).all()                                                 # distinct within a batch
    for k in range(4906):
        u = users[k * 256:(k + 1) * 256]
        assert np.isin(seq[k * 15:(k + 1) * 15, 0], u).all(), k                                              # each starts at a user of its batch
        assert min(int(every[np.unique(u)].sum()), 15) == 15                                                 # the reference's law on the host
    # a bounded draw is a prefix; another epoch is another epoch
    head = s.draw(0, max_steps=7)
    assert head[3].shape == (7 * 15, s.path_len) and torch.equal(head[3], t(seq[:7 * 15])) and torch.equal(head[0], t(users))
    assert not torch.equal(s.draw(1)[3], t(seq))


# ------------------------------------------------------------------------------------------ 4. epoch level
CAP_SMALL, STEPS = 10, 40


def small_setup(epinion2, golden):
    """A reduced pair and path set: pairs = train[::51][:4096] (24 576 samples: 96 batches of 256), paths = those of the first 32 users
    holding 1 .. 6 paths that occur in the pairs, cap 10.  Asserted on the restatement, before the GPU is used: among the first 40
    batches of epochs 0 and 1 there is a batch without paths, one with fewer than cap and one that is cut."""
    if "small" not in _cache:
        from spex_amd.trainer import bpr_sampler_tables, dual_sampler_tables
        from utility2.utils import Data
        pairs = epinion2["train"][::51][:4096, :2]
        paths, targets = epinion2_paths(golden)
        first = np.array([p[0] for p in paths])
        held = np.bincount(first, minlength=N_U)
        keep = [u for u in np.unique(pairs[:, 0]) if 1 <= held[u] <= 6][:32]
        sel = np.flatnonzero(np.isin(first, keep))
        raw = ([paths[k] for k in sel], [targets[k] for k in sel])
        assert len(keep) == 32 and len(sel) == 74
        rowptr, items, _ = bpr_sampler_tables(pairs, N_U, N_I)
        p_rowptr, p_idx = dual_sampler_tables(raw[0], N_U)
        for epoch in (0, 1):
            users = reference_epoch(rowptr, items, pairs[:, 0], pairs[:, 1], 5, N_I, 2020, epoch)[0]
            totals = np.array([batch_candidates(users[k * 256:(k + 1) * 256], p_rowptr, p_idx)[2] for k in range(STEPS)])
            assert (totals == 0).any() and ((totals > 0) & (totals < CAP_SMALL)).any() and (totals > CAP_SMALL).any(), totals
        _cache["small"] = (pairs, Data(raw, N_U - 1, shuffle=False))
    return _cache["small"]


def small_sampler(epinion2, golden):
    from spex_amd.trainer import DualDeviceSampler
    pairs, trust = small_setup(epinion2, golden)
    return DualDeviceSampler(pairs, N_U, N_I, trust, CAP_SMALL, 256, seed=2020, device=DEV)


def dual_stepper(data_root, path_len, dropout=False, cap=CAP_SMALL):
    """A fresh Epinion2 dual-task model (seeded: every call builds the same one) and its deterministic stepper."""
    import lg_parser
    import utility1.dataloader as dataloader
    import utility1.model_expert_s as mex
    import utility1.utils as utils
    from spex_amd.trainer import DualTaskStepper
    extra = ("--dropout", "1", "--keepprob", "0.3") if dropout else ()
    args = lg_parser.parse_args_r(["--dataset", "epinion2", "--data_path", data_root, *extra])
    if ("loader", dropout) not in _cache:
        _cache[("loader", dropout)] = dataloader.Loader(args)
    utils.set_seed(args.seed)                                         # (after the loader: every model starts from the same generator state)
    net = mex.LightGCN(args, _cache[("loader", dropout)]).to(DEV)
    return DualTaskStepper(net, path_capacity=cap, path_len=path_len, lr=args.lr, deterministic=True)


def same_state(a, b):
    return torch.equal(a.arena, b.arena) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and a.t == b.t


def compacted(out, n_batches, cap):
    """draw()'s strided paths in the path_off form of DualTaskStepper.epoch, compacted on the host."""
    seq, seq_l, tgt, count = (x.cpu() for x in out[3:])
    rows = torch.cat([k * cap + torch.arange(int(count[k])) for k in range(n_batches)])
    path_off = np.zeros(n_batches + 1, np.int64)
    np.cumsum(count[:n_batches].numpy(), out=path_off[1:])
    return seq[rows].contiguous().to(DEV), seq_l[rows].contiguous().to(DEV), tgt[rows].contiguous().to(DEV), path_off


@pytest.mark.parametrize("dropout", [None, (0.3, "philox", 5)])
def test_sampled_epoch_equals_draw_compaction_and_the_existing_epoch(epinion2, golden, data_root, dropout):
    from spex_amd.trainer import train_epoch_dual
    s = small_sampler(epinion2, golden)
    a, b = dual_stepper(data_root, s.path_len, bool(dropout)), dual_stepper(data_root, s.path_len, bool(dropout))
    assert same_state(a, b)
    n_paths = []
    got = train_epoch_dual(a, s, epoch=1, max_steps=STEPS, edge_dropout=dropout, n_paths_out=n_paths)
    out = s.draw(1, max_steps=STEPS)
    count = out[6].cpu().numpy()
    assert n_paths == count.tolist() and 0 in n_paths and max(n_paths) == CAP_SMALL and any(0 < c < CAP_SMALL for c in n_paths)
    seq, seq_l, tgt, path_off = compacted(out, STEPS, CAP_SMALL)
    b.loss_acc.zero_()
    b.epoch(out[0], out[1], out[2], 256, seq, seq_l, tgt, path_off, max_steps=STEPS, keep_prob=dropout[0] if dropout else 1.0,
            drop_seed=dropout[2] if dropout else 0)
    b.join()
    assert a.t == STEPS and same_state(a, b)
    assert torch.equal(got, b.loss_acc) and got[0].item() > 0 and got[1].item() > 0
    assert getattr(a.model.Graph, "mask_mode", 0) == 0


@pytest.mark.parametrize("dropout", [None, (0.3, "philox", 5)])
def test_two_sampled_epochs_equal_two_per_epoch_calls_without_side_effects(epinion2, golden, data_root, dropout, monkeypatch):
    from spex_amd.trainer import bpr_epoch_drop_seed, train_epoch_dual, train_epochs_dual
    s = small_sampler(epinion2, golden)
    a, b = dual_stepper(data_root, s.path_len, bool(dropout)), dual_stepper(data_root, s.path_len, bool(dropout))
    started = []
    inner_start = threading.Thread.start
    monkeypatch.setattr(threading.Thread, "start", lambda self, *x, **k: (started.append(self), inner_start(self, *x, **k))[1])
    n_threads = threading.active_count()
    states = random.getstate(), np.random.get_state(), torch.get_rng_state()
    fired = []
    totals = train_epochs_dual(a, s, 2, edge_dropout=dropout, max_steps=STEPS, after_epoch=lambda e, x: fired.append((e, a.t)))
    assert started == [] and threading.active_count() == n_threads
    assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[2])
    now = np.random.get_state()
    assert now[0] == states[1][0] and np.array_equal(now[1], states[1][1]) and now[2:] == states[1][2:]
    assert fired == [(0, STEPS), (1, 2 * STEPS)] and len(totals) == 2 and totals[0].shape == (2,)
    want = []
    for e in range(2):
        drop = None if dropout is None else (dropout[0], dropout[1], bpr_epoch_drop_seed(dropout[2], e))
        want.append(train_epoch_dual(b, s, epoch=e, max_steps=STEPS, edge_dropout=drop).cpu().numpy())
    assert a.t == 2 * STEPS and same_state(a, b)
    assert np.array_equal(np.stack(totals), np.stack(want)) and not np.array_equal(totals[0], totals[1])
    if dropout is not None:
        assert bpr_epoch_drop_seed(5, 0) == 5 and bpr_epoch_drop_seed(5, 1) != 5
    # first_epoch: epochs 1 .. 2 start where a run of epoch 1 alone starts
    c, d = dual_stepper(data_root, s.path_len, bool(dropout)), dual_stepper(data_root, s.path_len, bool(dropout))
    first = train_epochs_dual(c, s, 1, edge_dropout=dropout, max_steps=STEPS, first_epoch=1)[0]
    drop = None if dropout is None else (dropout[0], dropout[1], bpr_epoch_drop_seed(dropout[2], 1))
    assert np.array_equal(first, train_epoch_dual(d, s, epoch=1, max_steps=STEPS, edge_dropout=drop).cpu().numpy()) and same_state(c, d)


def test_python_loop_form_on_the_samplers_arrays_equals_the_native_form(epinion2, golden, data_root):
    from spex_amd.trainer import train_epoch_dual
    s = small_sampler(epinion2, golden)
    a, b = dual_stepper(data_root, s.path_len), dual_stepper(data_root, s.path_len)
    cum = []
    got = train_epoch_dual(a, s, epoch=0, max_steps=STEPS, cum_every=10, cum_out=cum)
    want = train_epoch_dual(b, s, epoch=0, max_steps=STEPS)
    assert len(cum) == 4 and torch.equal(cum[-1], got) and torch.equal(got, want) and same_state(a, b)
    # the arguments a sampler makes redundant are refused, and so is another batch size
    with pytest.raises(ValueError, match="the sampler holds"):
        train_epoch_dual(a, s, epi_trust(golden), {}, 15)
    with pytest.raises(ValueError, match="is not the sampler's"):
        train_epoch_dual(a, s, batch_size=128)
    assert a.t == STEPS


# ------------------------------------------------------------------------------------------ 5. the strided epoch call
def test_strided_epoch_call_rejects_bad_counts_before_any_launch(epinion2, golden, data_root):
    from spex_amd import _lib
    lib = _lib.load()
    s = small_sampler(epinion2, golden)
    st = dual_stepper(data_root, s.path_len)
    out = s.draw(0, max_steps=4)
    before = st.arena.clone()
    acc = st.loss_acc.clone()
    d = st._prepare_desc(256)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(counts, stride=CAP_SMALL, **kw):
        h = np.asarray(counts, np.int32)
        rc = lib.spex_dual_task_epoch_strided_f32(ctypes.byref(d), vp(out[0]), vp(out[1]), vp(out[2]), 1024, 256, kw.get("max_steps", -1),
                                                  vp(out[3]), vp(out[4]), vp(out[5]), stride, h.ctypes.data_as(ctypes.c_void_p),
                                                  kw.get("keep_prob", 1.0), 0, None)
        return rc, lib.spex_last_error().decode()

    assert st.path_capacity == CAP_SMALL
    for counts, stride, where in (([1, 2, 3, 11], 16, "batch 3"), ([1, 2, 3, 9], 8, "batch 3"), ([1, -1, 0, 0], 10, "batch 1"),
                                  ([0, 0, 0, 11], 10, "batch 3")):      # above the capacity, above the stride, negative, above both
        rc, msg = call(counts, stride)
        assert rc < 0 and "spex_dual_task_epoch_strided_f32" in msg and where in msg, (counts, rc, msg)
    assert call([1, 1, 1, 1], keep_prob=0.0)[0] < 0
    torch.cuda.synchronize()
    assert d.t == 0 and st.t == 0 and torch.equal(st.arena, before) and torch.equal(st.loss_acc, acc)
    assert call([1, 2, 3, 11], 16, max_steps=3)[0] == 0                  # the bad count lies past the bound: three steps run
    torch.cuda.synchronize()
    assert d.t == 3 and not torch.equal(st.arena, before)
    st.t = d.t
    with pytest.raises(ValueError, match="int32"):
        st.epoch_strided(out[0], out[1], out[2], 256, out[3], out[4], out[5], CAP_SMALL, np.zeros(96, np.int64))
    with pytest.raises(_lib.SpexError, match="batch 0 has 11 paths"):
        st.epoch_strided(out[0], out[1], out[2], 256, out[3], out[4], out[5], 11, np.full(96, 11, np.int32), max_steps=3)
    assert st.t == 3
