"""NGCF epochs drawn on the device (spex_sample_ngcf_epoch: per user 5 x |positives| negatives WITHOUT replacement, the positives, and
the shuffle in one launch) and the sampled epochs built on them (spex_ngcf_epoch_bce_sampled_f32, spex_ngcf_train_bce_sampled_f32;
trainer.NgcfDeviceSampler, train_epoch_ngcf / train_epochs_ngcf with a sampler).

The law is restated in NumPy from the text of include/spex_hip.h (test_host_ngcf_device_sampler.reference_epoch, whose exact
properties and marginal law are checked there on the CPU) and the kernel must reproduce it bit for bit.  The training comparisons
issue the same launches on both sides in the DETERMINISTIC step, where a run is a pure function of its inputs: torch.equal.  The one
exception is the 2-layer stepper, which has no deterministic mode (NGCFStepper(deterministic=True) refuses L >= 2: the deep step's
scoring tables and push use float atomics): there the steps' INPUTS are held to draw()'s slices bit for bit, and the results to the
bounds test_gpu_ngcf.py::test_deep_one_call_step_equals_the_launch_by_launch_step sets for two runs of the same four launches.

The training graph is the 300-user golden (tests/golden/ngcf_small_epochs.npz): 256 users per epoch, n = 14 934 samples = 58 batches
of 256 and one of 86."""
import ctypes
import os
import random
import threading

import numpy as np
import pytest
import torch

from conftest import REPO
from test_host_ngcf_device_sampler import epinion2_tables, gap_graph, reference_epoch

pytestmark = pytest.mark.gpu

DEV = "cuda"
_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_tables(pop, users, lists):
    """The six tables without ngcf_sampler_tables' checks (a test may break the caller's promise 5 c <= n_q on purpose)."""
    pop = np.asarray(sorted(pop), np.int64)
    pos_off, row_off, ranks = [0], [0], []
    for pos in lists:
        r = np.searchsorted(pop, np.unique(np.asarray(pos, np.int64)))
        ranks.append(r)
        pos_off.append(pos_off[-1] + len(pos))
        row_off.append(row_off[-1] + len(r))
    cat = lambda parts: np.concatenate([np.asarray(p, np.int64).reshape(-1) for p in parts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return (pop.astype(np.int32), np.asarray(users, np.int32), np.asarray(pos_off, np.int32), cat(lists), np.asarray(row_off, np.int32), cat(ranks))


def draw(tables, seed, epoch, out=None):
    from spex_amd import ops
    return ops.sample_ngcf_epoch(*(t(a) for a in tables), seed, epoch, out=out)


# ------------------------------------------------------------------------------------------ 1. bit-exactness
def small_case(U, n_pop):
    """U users over a population of n_pop items — ids with gaps at n_pop = 64 (every third id) — with c_q from (0, 1, 3, 43) where
    5 c <= n_pop - c allows it (1 otherwise): U = 1: c = 1; U = 2: an empty user first; U = 7: empty users first, in the middle and
    last, and the user at position 5 lists its first positive twice when it has three."""
    from spex_amd.trainer import ngcf_sampler_tables
    rng = np.random.default_rng(100 * U + n_pop)
    pop = (3 * np.arange(n_pop) + 2) if n_pop == 64 else np.arange(n_pop)
    want = {1: [1], 2: [0, 3], 7: [0, 3, 1, 0, 43, 3, 0]}[U]
    cs = [c if 5 * c <= n_pop - c else 1 for c in want]
    train_items = {}
    for q, c in enumerate(cs):
        pos = rng.choice(pop, c, replace=False).tolist()
        if q == 5 and c == 3:
            pos[2] = pos[0]
        train_items[1000 - 7 * q] = pos                                    # user ids unrelated to the position q that keys the draw
    return ngcf_sampler_tables(train_items, set(pop.tolist()), list(train_items.keys())), cs


@pytest.mark.parametrize("n_pop", [6, 64, 683])
@pytest.mark.parametrize("U", [1, 2, 7])
def test_kernel_reproduces_the_documented_law_on_small_epochs(U, n_pop):
    """n = 6 (one user, c = 1 over a population of 6: h = 2 for the shuffle, n_q = 5 = 5 c: the whole complement) up to n = 300
    (U = 7 at n_pop = 683, one user with c = 43), both key words and the epoch word's top bit in use."""
    tables, cs = small_case(U, n_pop)
    n = 6 * sum(cs)
    for seed, epoch in ((0xFEDCBA9876543210, 0x80000005), (5, 0)):
        got = draw(tables, seed, epoch)
        want = reference_epoch(tables, seed, epoch)
        assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.float32 and all(x.shape == (n,) for x in got)
        for g, w, name in zip(got, want, ("users", "items", "labels")):
            assert np.array_equal(g.cpu().numpy(), w), f"U = {U}, n_pop = {n_pop}, n = {n}: {name}"
    if U == 1 and n_pop == 6:
        v, y = got[1].cpu().numpy(), got[2].cpu().numpy()
        pos = tables[3]
        assert n == 6 and sorted(v[y == 0].tolist()) == sorted(set(range(6)) - set(pos.tolist()))      # every non-positive exactly once


def test_kernel_reproduces_the_law_on_the_gap_graph_and_on_tiny_complements():
    """The host test's gap graph (a user with 5 c = n_q exactly, a duplicated positive, empty users first / middle / last), and tables
    that BREAK the caller's promise so that the domains of one and two elements (h = 1) and the guards run: n_q = 2 (negatives 0 and 1
    are the two complement members, negatives 2 .. 4 write item 0), n_q = 1, n_q = 0 (every negative writes item 0) — nothing is read
    out of bounds, and the restatement says the same."""
    from spex_amd.trainer import ngcf_sampler_tables
    cases = [ngcf_sampler_tables(*gap_graph()),
             raw_tables([4, 9, 11], [5], [[9]]),                            # n_pop = 3, m = 1: n_q = 2
             raw_tables([4, 9], [5, 6], [[9], [4]]),                        # n_q = 1, twice
             raw_tables([7], [0], [[7]]),                                   # n_q = 0
             raw_tables([4, 9, 11], [5, 8, 6], [[], [9, 9, 9, 9], []])]     # c = 4, m = 1: n_q = 2 < 20
    for k, tables in enumerate(cases):
        for seed, epoch in ((3, 1), (0x123456789ABCDEF, 7)):
            got = draw(tables, seed, epoch)
            want = reference_epoch(tables, seed, epoch)
            for g, w, name in zip(got, want, ("users", "items", "labels")):
                assert np.array_equal(g.cpu().numpy(), w), f"case {k}: {name}"
    v, y = got[1].cpu().numpy(), got[2].cpu().numpy()                       # the last case: 20 negatives, two of them real
    assert sorted(v[y == 0].tolist()) == [0] * 18 + [4, 11]


def epi_epoch(epinion2):
    """The shared Epinion2 epoch (seed 2020, epoch 0): (sampler, tables, the kernel's three arrays on the host)."""
    if "epoch" not in _cache:
        from spex_amd.trainer import NgcfDeviceSampler
        tables, data = epinion2_tables(epinion2)
        s = NgcfDeviceSampler(data, seed=2020, device=DEV)
        out = s.draw(0)
        assert all(x.is_cuda and x.shape == (s.n,) for x in out)
        _cache["epoch"] = (s, tables, tuple(x.cpu().numpy() for x in out))
    return _cache["epoch"]


def test_kernel_reproduces_the_law_on_one_epinion2_epoch(epinion2):
    s, tables, got = epi_epoch(epinion2)
    assert s.user.numel() == 3072 and s.n == 6 * len(tables[3]) == 1217538
    for a, b in zip((s.pop, s.user, s.pos_off, s.pos_item, s.row_off, s.row_rank), tables):
        assert np.array_equal(a.cpu().numpy(), b)
    want = reference_epoch(tables, 2020, 0)
    for g, w, name in zip(got, want, ("users", "items", "labels")):
        assert np.array_equal(g, w), f"Epinion2, {name}"
    # the exact properties once more on the kernel's own output: per user 5 c distinct negatives outside its row
    u, v, y = got
    neg = y == 0
    pairs = epinion2["train"][:, :2]
    assert neg.sum() == 5 * (~neg).sum()
    keys = u[neg] * 12407 + v[neg]
    assert len(np.unique(keys)) == len(keys), "a user drew a negative twice"
    assert not np.isin(keys, pairs[:, 0] * 12407 + pairs[:, 1]).any(), "a negative is one of its user's positives"
    assert np.isin(v[neg], tables[0]).all()


# ------------------------------------------------------------------------------------------ 2. a function of (seed, epoch)
def test_draws_are_a_function_of_seed_and_epoch(epinion2):
    from spex_amd import ops
    from spex_amd.trainer import NgcfDeviceSampler
    s, _, got = epi_epoch(epinion2)
    again, other_epoch = s.draw(0), s.draw(1)
    bufs = s.epoch_buffers()
    into = ops.sample_ngcf_epoch(s.pop, s.user, s.pos_off, s.pos_item, s.row_off, s.row_rank, s.seed, 0, out=bufs)
    other_seed = NgcfDeviceSampler(epinion2_tables(epinion2)[1], seed=2021, device=DEV).draw(0)
    for k in range(3):
        assert np.array_equal(again[k].cpu().numpy(), got[k]) and torch.equal(into[k], again[k]) and into[k].data_ptr() == bufs[k].data_ptr()
        assert not torch.equal(again[k], other_epoch[k]) and not torch.equal(again[k], other_seed[k])
    assert (again[0] != other_epoch[0]).float().mean().item() > 0.5 and (again[0] != other_seed[0]).float().mean().item() > 0.5


# ------------------------------------------------------------------------------------------ 3. argument checks
def test_rejected_arguments_return_a_negative_status_and_touch_nothing():
    from spex_amd import _lib
    from spex_amd.trainer import ngcf_sampler_tables
    lib = _lib.load()
    tables = ngcf_sampler_tables(*gap_graph())
    dt = [t(a) for a in tables]
    n = 6 * len(tables[3])
    out = [torch.full((n,), -5, dtype=torch.int64, device=DEV), torch.full((n,), -5, dtype=torch.int64, device=DEV),
           torch.full((n,), -5.0, dtype=torch.float32, device=DEV)]
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    good = dict(pop=vp(dt[0]), n_pop=len(tables[0]), user=vp(dt[1]), U=len(tables[1]), pos_off=vp(dt[2]), pos_item=vp(dt[3]), n_pos=len(tables[3]),
                row_off=vp(dt[4]), row_rank=vp(dt[5]), users=vp(out[0]), items_out=vp(out[1]), labels=vp(out[2]))

    def call(**kw):
        k = dict(good, **kw)
        rc = lib.spex_sample_ngcf_epoch(k["pop"], k["n_pop"], k["user"], k["U"], k["pos_off"], k["pos_item"], k["n_pos"], k["row_off"], k["row_rank"],
                                        5, 0, k["users"], k["items_out"], k["labels"], None)
        return rc, lib.spex_last_error().decode()

    cases = [dict(pop=None), dict(user=None), dict(pos_off=None), dict(pos_item=None), dict(row_off=None), dict(row_rank=None), dict(users=None),
             dict(items_out=None), dict(labels=None), dict(n_pop=0), dict(n_pop=-3), dict(U=-1), dict(U=0), dict(n_pos=-1),
             dict(n_pos=(1 << 31) // 6 + 1), dict(n_pos=1 << 40), dict(n_pos=1 << 62)]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "spex_sample_ngcf_epoch" in msg, (kw, rc, msg)
    assert "2^31" in call(n_pos=(1 << 31) // 6 + 1)[1] and "NULL" in call(labels=None)[1] and "n_pop" in call(n_pop=0)[1]
    torch.cuda.synchronize()
    assert all(bool((x == -5).all()) for x in out)
    rc, _ = call(n_pos=0, U=0)                                          # nothing to draw: OK, nothing launched
    assert rc == 0
    torch.cuda.synchronize()
    assert all(bool((x == -5).all()) for x in out)
    rc, _ = call()
    torch.cuda.synchronize()
    assert rc == 0 and all(bool((x != -5).all()) for x in out)          # (users 7 / 12 / 9, items of the population, labels 0 / 1)


# ------------------------------------------------------------------------------------------ the training graph
@pytest.fixture(scope="module")
def small_root(tmp_path_factory):
    from test_gpu_ngcf import _materialise
    root = str(tmp_path_factory.mktemp("ngcf_sampler_data"))
    g = np.load(os.path.join(REPO, "tests", "golden", "ngcf_small_epochs.npz"))
    _materialise(root, "small", g["train_pairs"], list(enumerate(g["test_pos"])), list(enumerate(g["test_neg"])))
    return os.path.join(root, "")


def make(small_root, p_drop=0.1, layers="[64]", deterministic=True, seed=11):
    """(data, model, stepper) on the 300-user graph from fixed seeds: every call gives the same initial state."""
    from test_gpu_ngcf import ngcf_args
    from spex_amd.dropin.ngcf.utility.load_data import Data
    from spex_amd.ngcf import NGCF
    from spex_amd.trainer import NGCFStepper
    torch.manual_seed(seed); random.seed(seed); np.random.seed(seed)
    data = Data(path=small_root + "small", batch_size=256)
    _, norm, _ = data.get_adj_mat()
    L = layers.count("64")
    model = NGCF({"n_users": data.n_users, "n_items": data.n_items, "norm_adj": norm}, DEV,
                 ngcf_args(mess_dropout=str([p_drop] * L), layer_size=layers)).to(DEV)
    model.message_dropout_seed = 4242
    model.train()
    return data, model, NGCFStepper(model, lr=1e-3, deterministic=deterministic)


def state(st):
    return [p.detach().clone() for p in st.model.parameters()] + [x.clone() for x in (st.mE, st.vE, st.mW, st.vW)]


def same_state(a, b):
    return a.t == b.t and a.model.dropout_step == b.model.dropout_step and all(torch.equal(x, y) for x, y in zip(state(a), state(b)))


def sampler_of(data, seed=31):
    from spex_amd.trainer import NgcfDeviceSampler
    return NgcfDeviceSampler(data, seed=seed, device=DEV)


def test_sampled_epoch_checks_its_arguments_before_the_sampler_runs(small_root):
    from spex_amd import _lib
    lib = _lib.load()
    data, model, st = make(small_root)
    s = sampler_of(data)
    assert s.n == 14934 and s.user.numel() == 256 and s.batch_size == 256
    bufs = s.epoch_buffers()
    for b in bufs:
        b.fill_(7)
    acc = torch.zeros(2, 1, device=DEV)
    d = st._prepare_desc(256)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(batch=256, loss=vp(acc[0]), labels=vp(bufs[2]), n_pos=s.n_pos, n_pop=s.pop.numel(), U=256, row_rank=vp(s.row_rank), step=ctypes.byref(d)):
        rc = lib.spex_ngcf_epoch_bce_sampled_f32(step, vp(s.pop), n_pop, vp(s.user), U, vp(s.pos_off), vp(s.pos_item), n_pos, vp(s.row_off), row_rank,
                                                 1, 0, batch, -1, vp(bufs[0]), vp(bufs[1]), labels, loss, vp(acc[1]), None)
        return rc, lib.spex_last_error().decode()

    for kw in (dict(batch=0), dict(loss=None), dict(labels=None), dict(n_pos=1 << 31), dict(n_pop=0), dict(U=0), dict(row_rank=None), dict(step=None)):
        rc, msg = call(**kw)
        assert rc < 0 and msg, (kw, rc, msg)
    rc, msg = lib.spex_ngcf_train_bce_sampled_f32(ctypes.byref(d), vp(s.pop), s.pop.numel(), vp(s.user), 256, vp(s.pos_off), vp(s.pos_item), s.n_pos,
                                                  vp(s.row_off), vp(s.row_rank), 1, 0, 2, 256, -1, vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), None,
                                                  None), lib.spex_last_error()
    assert rc < 0 and b"loss_epochs" in msg
    torch.cuda.synchronize()
    assert d.t == 0 and d.dropout_step == 0 and all(bool((b == 7).all()) for b in bufs) and not acc.any()
    # the Python layer: a sampler on another device than the stepper, a multi-layer stepper, a short loss buffer
    from spex_amd.trainer import NgcfDeviceSampler, train_epoch_ngcf
    cpu = NgcfDeviceSampler(data, device="cpu")
    with pytest.raises(ValueError, match="the sampler's tables live on cpu"):
        st.epoch_sampled(cpu, 0, 256, acc[0], acc[1])
    with pytest.raises(ValueError, match="the sampler's tables live on cpu"):
        train_epoch_ngcf(st, cpu, step_losses=[])
    with pytest.raises(ValueError, match="loss_epochs"):
        st.train_sampled(s, 3, 256, torch.zeros(4, device=DEV))
    _, _, deep = make(small_root, layers="[64,64]", deterministic=False)
    with pytest.raises(ValueError, match="single-layer"):
        deep.epoch_sampled(s, 0, 256, acc[0], acc[1])
    assert st.t == 0 and model.dropout_step == 0


# ------------------------------------------------------------------------------------------ 4. the sampled epoch
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("B, max_steps, steps", [(256, 40, 40), (384, None, 39)])
def test_sampled_epoch_equals_draw_followed_by_the_native_epoch(small_root, p_drop, B, max_steps, steps):
    """B = 256: the first 40 batches; B = 384: the whole epoch, 38 full batches and a ragged one of 342.  Deterministic step: the
    parameters, the Adam moments and both loss cells are bit-equal."""
    (da, ma, a), (db, mb, b) = make(small_root, p_drop), make(small_root, p_drop)
    s = sampler_of(da)
    acc_a, acc_b = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
    a.epoch_sampled(s, 4, B, acc_a[0], acc_a[1], max_steps=max_steps)
    u, i, y = s.draw(4)
    assert all(torch.equal(x, z) for x, z in zip(s.epoch_buffers(), (u, i, y)))
    b.epoch(u, i, y, B, acc_b[0], acc_b[1], max_steps=max_steps)
    assert a.t == steps and ma.dropout_step == (steps if p_drop > 0 else 0)
    assert (acc_a[1].item() != 0.0) == (max_steps is None) and acc_a[0].item() != 0.0
    assert torch.equal(acc_a, acc_b) and same_state(a, b)
    assert not torch.equal(state(a)[0], state(make(small_root, p_drop)[2])[0])          # (it trained)


# ------------------------------------------------------------------------------------------ 5. several epochs in one call
def test_three_epochs_in_one_call_equal_three_per_epoch_calls(small_root):
    (da, ma, a), (db, mb, b) = make(small_root), make(small_root)
    s = sampler_of(da, seed=13)
    acc_a = torch.zeros(3, 2, device=DEV)
    a.train_sampled(s, 3, 384, acc_a, first_epoch=5)
    acc_b = torch.zeros(3, 2, device=DEV)
    for e in range(3):
        b.epoch_sampled(s, 5 + e, 384, acc_b[e, 0:1], acc_b[e, 1:2])
    assert a.t == 117 and ma.dropout_step == 117 and a._desc.t == 117 and a._desc.dropout_step == 117
    got = acc_a.cpu().numpy()
    assert np.all(got != 0) and len(set(got[:, 0].tolist())) == 3     # [2 e]: full batches, [2 e + 1]: the ragged one, per epoch
    assert np.all(got[:, 0] > 10 * got[:, 1])                         # 38 x 384 samples against 342
    assert torch.equal(acc_a, acc_b) and same_state(a, b)


# ------------------------------------------------------------------------------------------ 6. dispatch
def test_train_epoch_and_train_epochs_take_a_sampler(small_root):
    """Single-layer stepper: train_epoch_ngcf takes epoch_sampled (once), train_epochs_ngcf takes train_sampled (once) — or one
    epoch_sampled per epoch with after_epoch — and no thread is started; with
    step_losses the epoch is drawn by draw() and trained step by step.  Deterministic step: all of them equal the explicit calls."""
    from spex_amd.trainer import train_epoch_ngcf, train_epochs_ngcf
    B = 384
    data, _, ref = make(small_root)
    s = sampler_of(data, seed=5)
    n_threads = threading.active_count()
    seen = []

    def spy(st, name):
        inner = getattr(st, name)
        setattr(st, name, lambda *x, **k: (seen.append((name, threading.active_count())), inner(*x, **k))[1])

    def total(acc):                                                   # main_rec.py:129's sum of per-batch mean losses
        return acc[0].item() / B + acc[1].item() / (s.n % B)

    acc = torch.zeros(2, 1, device=DEV)
    ref.epoch(*s.draw(2), B, acc[0], acc[1])
    want = total(acc)
    _, _, a = make(small_root)
    _, _, b = make(small_root)
    spy(a, "epoch_sampled")
    got_a = train_epoch_ngcf(a, s, batch_size=B, epoch=2).item()
    assert seen == [("epoch_sampled", n_threads)]
    spy(b, "epoch_sampled")
    draws = []
    inner_draw = s.draw
    s.draw = lambda e: (draws.append(e), inner_draw(e))[1]
    losses = []
    got_b = train_epoch_ngcf(b, s, batch_size=B, epoch=2, step_losses=losses).item()
    del s.draw
    assert draws == [2] and len(seen) == 1 and len(losses) == 39 and all(0.1 < x < 2.0 for x in losses)
    for st, got in ((a, got_a), (b, got_b)):
        assert same_state(st, ref) and abs(got - want) <= 2e-6 * abs(want)
    # three epochs
    _, _, ref3 = make(small_root)
    acc3 = torch.zeros(3, 2, device=DEV)
    for e in range(3):
        ref3.epoch_sampled(s, 1 + e, B, acc3[e, 0:1], acc3[e, 1:2])
    want3 = [total(acc3[e]) for e in range(3)]
    seen.clear()
    _, _, c = make(small_root)
    spy(c, "train_sampled")
    totals = train_epochs_ngcf(c, s, 3, batch_size=B, first_epoch=1)
    assert seen == [("train_sampled", n_threads)] and len(totals) == 3 and all(isinstance(x, float) for x in totals)
    seen.clear()
    _, _, e_ = make(small_root)
    spy(e_, "train_sampled")
    spy(e_, "epoch_sampled")
    fired = []
    totals_e = train_epochs_ngcf(e_, s, 3, batch_size=B, first_epoch=1, after_epoch=lambda ep, x: fired.append((ep, float(x), e_.t)))
    assert seen == [("epoch_sampled", n_threads)] * 3
    assert [f[0] for f in fired] == [0, 1, 2] and [f[2] for f in fired] == [39, 78, 117] and [f[1] for f in fired] == totals_e
    for st, got in ((c, totals), (e_, totals_e)):
        assert same_state(st, ref3) and np.abs(np.array(got) - np.array(want3)).max() <= 2e-6 * np.abs(want3).max()
    assert threading.active_count() == n_threads
    # the sampler's own batch size is the default
    _, _, f = make(small_root)
    _, _, h = make(small_root)
    tf = train_epoch_ngcf(f, s, epoch=0, max_steps=3).item()
    acc = torch.zeros(2, 1, device=DEV)
    h.epoch(*s.draw(0), 256, acc[0], acc[1], max_steps=3)
    assert same_state(f, h) and abs(tf - acc[0].item() / 256) <= 2e-6 * tf


def test_global_generators_do_not_move_under_the_sampler(small_root):
    from spex_amd.trainer import train_epoch_ngcf, train_epochs_ngcf
    data, _, st = make(small_root)
    s = sampler_of(data)
    py_state, np_state, torch_state = random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state()
    train_epoch_ngcf(st, s, epoch=0, max_steps=5)
    train_epoch_ngcf(st, s, epoch=1, max_steps=5, step_losses=[])
    train_epoch_ngcf(st, s, epoch=2, max_steps=5, callbacks={2: lambda: None})
    train_epochs_ngcf(st, s, 2, max_steps=5)
    train_epochs_ngcf(st, s, 2, max_steps=5, after_epoch=lambda ep, x: None)
    assert st.t == 35
    assert random.getstate() == py_state and np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


def test_two_layer_stepper_with_the_sampler_runs_the_python_loop_over_the_drawn_tensors(small_root):
    """L = 2: no native epoch — train_epoch_ngcf draws once and calls NGCFStepper.step per batch.  The batches handed to step() are
    draw()'s slices, bit for bit; the result against step() called by hand on those slices within the bounds two runs of the deep step
    are held to (float atomics: see the module docstring)."""
    from spex_amd.trainer import train_epoch_ngcf
    data, ma, a = make(small_root, layers="[64,64]", deterministic=False)
    _, mb, b = make(small_root, layers="[64,64]", deterministic=False)
    s = sampler_of(data, seed=3)
    u, i, y = s.draw(6)
    handed = []
    inner = a.step
    a.step = lambda uu, ii, yy, loss_acc=None: (handed.append((uu.clone(), ii.clone(), yy.clone())), inner(uu, ii, yy, loss_acc=loss_acc))[1]
    py_state, torch_state = random.getstate(), torch.get_rng_state()
    got = train_epoch_ngcf(a, s, epoch=6, max_steps=4).item()
    assert random.getstate() == py_state and torch.equal(torch.get_rng_state(), torch_state)
    assert len(handed) == 4 and a._deep_desc is not None and a._desc is None
    acc = torch.zeros(1, device=DEV)
    for k, (uu, ii, yy) in enumerate(handed):
        sl = slice(256 * k, 256 * (k + 1))
        assert torch.equal(uu, u[sl]) and torch.equal(ii, i[sl]) and torch.equal(yy, y[sl])
        b.step(u[sl], i[sl], y[sl], loss_acc=acc)
    assert a.t == b.t == 4 and ma.dropout_step == mb.dropout_step == 4
    want = acc.item() / 256
    print(f"2-layer, 4 steps: loss sum {got:.6f} vs {want:.6f}")
    assert abs(got - want) * 256 <= 4 * 2e-3                              # that test's 2e-3 per step's loss sum, four steps
    for (n, p), q in zip(ma.named_parameters(), mb.parameters()):
        dv = (p.detach() - q.detach()).abs()
        assert float(dv.mean()) <= 2e-6 and float(dv.max()) <= 1e-3 + 1e-7, (n, float(dv.mean()), float(dv.max()))


def test_passing_data_keeps_the_host_path(small_root):
    """train_epochs_ngcf / train_epoch_ngcf with a Data: the run of the code before the sampler existed — epoch_arrays_ngcf (the `random`
    stream, then the DataLoader's shuffle from torch's generator), the upload, NGCFStepper.epoch — repeated here by hand from the same
    seeds: bit-equal parameters, equal totals, and the generators left where that run leaves them."""
    from spex_amd.trainer import _sum_of_batch_means, _upload, epoch_arrays_ngcf, train_epoch_ngcf, train_epochs_ngcf
    data_a, _, a = make(small_root)
    totals = train_epochs_ngcf(a, data_a, 2)
    total3 = train_epoch_ngcf(a, data_a).item()
    end_py, end_torch = random.getstate(), torch.get_rng_state()
    data_b, _, b = make(small_root)
    want = []
    for _ in range(3):
        u, i, y = _upload(b.E0.device, *epoch_arrays_ngcf(data_b))
        acc = torch.zeros(2, 1, device=DEV)
        b.epoch(u, i, y, 256, acc[0], acc[1])
        want.append(float(_sum_of_batch_means(acc, u.numel(), 256)))
    assert same_state(a, b) and a.t == 3 * 59
    assert totals + [total3] == want
    assert random.getstate() == end_py and torch.equal(torch.get_rng_state(), end_torch)
