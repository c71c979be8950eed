"""BPR triples drawn on the device (spex_sample_bpr_triples) and the sampled epochs built on them
(spex_lightgcn_epoch_bpr_sampled_f32, spex_lightgcn_train_bpr_sampled_f32; trainer.BprDeviceSampler).

The stream is restated below in NumPy from the text of include/spex_hip.h (reference_triples) and the kernel must reproduce it bit
for bit; the sampling law is checked cell by cell with the binomial bound of test_host_bpr_device_sampler.py (validated there on the
host sampler).  The training comparisons issue the same launches on both sides, so the deterministic mode is compared with
torch.equal and the fast mode within the bounds of tests/test_gpu_bpr_exact_step.py (float-atomic order only)."""
import ctypes

import numpy as np
import pytest
import torch

from test_host_bpr_device_sampler import N_LAW, check_law, law_graph, philox4x32_10

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_U, N_I = 3186, 12407
T = 256
# test_gpu_bpr_exact_step.py: test_native_bpr_epoch_equals_the_steps_issued_one_by_one
EPOCH_BOUNDS = (2e-6, 2e-5, 2e-5, 4e-5)          # loss, E0, m, v

_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------ the documented stream, in NumPy
def to_range(w, m):
    """floor(w * m / 2^32) for 32-bit words w held in uint64."""
    return ((w * np.asarray(m, np.uint64)) >> np.uint64(32)).astype(np.int64)


def reference_triples(rowptr, items, active, num_item, n, mode, seed, epoch):
    """spex_sample_bpr_triples as include/spex_hip.h words it: key = the seed's two halves, counter = (slot low, slot high, epoch,
    stage); stage 0: w0 -> user position / entry, w1 -> positive position, w2 w3 -> candidates 0 1; stage 1: candidates 2 .. 5;
    stage 2: w0 -> k, the k-th item in ascending order that is not in the row."""
    rowptr, items, active = (np.asarray(a, np.int64) for a in (rowptr, items, active))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    slot = np.arange(n, dtype=np.uint64)
    s_lo, s_hi = slot & np.uint64(0xFFFFFFFF), slot >> np.uint64(32)
    w = philox4x32_10(s_lo, s_hi, epoch, 0, k0, k1)
    nnz = int(rowptr[-1])
    if mode == 0:
        users = active[to_range(w[0], len(active))]
        beg, end = rowptr[users], rowptr[users + 1]
        pos = items[beg + to_range(w[1], end - beg)]
    else:
        e = to_range(w[0], nnz)
        users = np.searchsorted(rowptr, e, side="right") - 1          # the last u with rowptr[u] <= e
        beg, end = rowptr[users], rowptr[users + 1]
        pos = items[e]
    keys = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)) * num_item + items      # ascending: rows ascending within ascending users

    def stored(u, j):
        q = u * num_item + j
        at = np.searchsorted(keys, q)
        return (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == q)

    neg = to_range(w[2], num_item)
    todo = np.flatnonzero(stored(users, neg))
    cand = to_range(w[3][todo], num_item)
    neg[todo] = cand
    todo = todo[stored(users[todo], cand)]
    if len(todo):
        w1 = philox4x32_10(s_lo[todo], s_hi[todo], epoch, 1, k0, k1)
        left = np.arange(len(todo))                                   # positions in todo still without a negative
        for a in range(4):
            cand = to_range(w1[a][left], num_item)
            neg[todo[left]] = cand
            left = left[stored(users[todo[left]], cand)]
        todo = todo[left]
    n_fallback = len(todo)
    if n_fallback:
        w2 = philox4x32_10(s_lo[todo], s_hi[todo], epoch, 2, k0, k1)
        for x, i in enumerate(todo):
            row = items[beg[i]:end[i]]
            k = int(to_range(w2[0][x], num_item - len(row)))
            neg[i] = k + np.searchsorted(row - np.arange(len(row)), k, side="right")     # first m with row[m] - m > k
    return users, pos, neg, n_fallback


# ------------------------------------------------------------------------------------------ fixtures
def law_tables():
    if "law" not in _cache:
        from spex_amd.trainer import bpr_sampler_tables
        pairs, n_users, n_items = law_graph()
        _cache["law"] = (pairs, n_users, n_items, bpr_sampler_tables(pairs, n_users, n_items))
    return _cache["law"]


def epi_tables(epinion2):
    if "epi_tables" not in _cache:
        from spex_amd.trainer import bpr_sampler_tables
        _cache["epi_tables"] = bpr_sampler_tables(epinion2["train"][:, :2], N_U, N_I)
    return _cache["epi_tables"]


def epi_sampler(epinion2, seed=2020, by="user", n=None):
    from spex_amd.trainer import BprDeviceSampler
    return BprDeviceSampler(epinion2["train"][:, :2], N_U, N_I, DEV, seed=seed, by=by, n=n)


def epi(epinion2):
    """(csr, E0) of Epinion2 at d = 64: the LightGCN adjacency, E0 ~ U(-b, b) from default_rng(2020) (test_gpu_bpr_exact_step.py)."""
    if "csr" not in _cache:
        from spex_amd.datasets import epinion2_tables
        from spex_amd.graph import lightgcn_norm_adj
        tr = epinion2["train"]
        _cache["csr"] = lightgcn_norm_adj(tr[:, 0], tr[:, 1], N_U - 1, N_I)
        _cache["E0"] = np.concatenate(epinion2_tables(N_U, N_I, dim=64))
    return _cache["csr"], _cache["E0"]


def stepper(epinion2, deterministic=False, transposed=False):
    from spex_amd.graph import SpexGraph, csr_transpose
    from spex_amd.trainer import LightGCNStepper
    csr, E0 = epi(epinion2)
    gt = None
    if transposed:
        if "csr_t" not in _cache:
            _cache["csr_t"] = csr_transpose(*csr, len(E0))
        t_rowptr, t_col, t_val, eid = _cache["csr_t"]
        gt = SpexGraph(t_rowptr, t_col, t_val, edge_id=eid)
    return LightGCNStepper(SpexGraph(*csr), t(E0.copy()), N_U, n_layers=3, lr=1e-3, graph_t=gt, deterministic=deterministic,
                           weight_decay=1e-4)


def state(st):
    return st.E0.cpu().numpy(), st.m.cpu().numpy(), st.v.cpu().numpy()


def compare(tag, loss_a, loss_b, st_a, st_b, deterministic, bounds=EPOCH_BOUNDS):
    loss_a, loss_b = np.asarray(loss_a, np.float64), np.asarray(loss_b, np.float64)
    assert np.all(loss_b != 0)
    figs = (float((np.abs(loss_a - loss_b) / np.abs(loss_b)).max()),) + tuple(rel_err(x, y) for x, y in zip(state(st_a), state(st_b)))
    print(f"{tag} det={deterministic}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert st_a.t == st_b.t
    assert all(f <= b for f, b in zip(figs, bounds)), (tag, figs, bounds)
    if deterministic:
        assert torch.equal(st_a.E0, st_b.E0) and torch.equal(st_a.m, st_b.m) and torch.equal(st_a.v, st_b.v)
        assert np.array_equal(loss_a, loss_b)


# ------------------------------------------------------------------------------------------ 1. validity
@pytest.mark.parametrize("by", ["user", "interaction"])
def test_every_triple_is_valid_on_epinion2(epinion2, by):
    rowptr, items, active = epi_tables(epinion2)
    s = epi_sampler(epinion2, by=by)
    assert s.n == len(epinion2["train"]) == 209304
    out = s.draw(0)
    assert all(x.dtype == torch.int64 and x.is_cuda and x.shape == (s.n,) for x in out)
    u, p, ng = (x.cpu().numpy() for x in out)
    assert u.min() >= 0 and u.max() < N_U and p.min() >= 0 and p.max() < N_I and ng.min() >= 0 and ng.max() < N_I
    assert np.isin(u, active).all()
    keys = np.repeat(np.arange(N_U), np.diff(rowptr)).astype(np.int64) * N_I + items
    assert np.isin(u * N_I + p, keys).all(), "a positive is not one of its user's items"
    assert not np.isin(u * N_I + ng, keys).any(), "a negative is one of its user's items"
    print(f"by={by}: {len(np.unique(u))} distinct users of {len(active)} active, {len(np.unique(ng))} distinct negatives")
    if by == "user":                                                  # 66 draws per user on average: nobody is left out
        assert len(np.unique(u)) == len(active)


# ------------------------------------------------------------------------------------------ 2. the law
@pytest.mark.parametrize("by", ["user", "interaction"])
def test_sampling_law_on_the_8_by_16_graph(by):
    from spex_amd import ops
    pairs, n_users, n_items, (rowptr, items, active) = law_tables()
    u, p, ng = (x.cpu().numpy() for x in ops.sample_bpr_triples(t(rowptr), t(items), t(active), n_items, N_LAW, seed=77, epoch=3, by=by))
    worst, smallest, cells = check_law(u, p, ng, pairs, n_users, n_items, by=by)
    print(f"by={by}: {cells} cells, largest deviation {worst:.2f} sigma, smallest expected count {smallest:.0f}")
    deg = np.diff(rowptr)
    marg = np.bincount(u, minlength=n_users) / N_LAW
    want = (deg > 0) / (deg > 0).sum() if by == "user" else deg / deg.sum()
    print("user marginal", np.round(marg, 4), "expected", np.round(want, 4))
    assert marg[0] == 0
    assert np.all(np.abs(marg - want) <= 6 * np.sqrt(want * (1 - want) / N_LAW))
    # user 1 holds 15 of 16 items: six rejections fail with probability (15/16)^6 = 0.68, so most of its slots take the direct draw of
    # the k-th admissible item, and every one of its negatives is item 15
    assert (u == 1).sum() > 1000 and np.all(ng[u == 1] == 15)
    _, _, _, n_fallback = reference_triples(rowptr, items, active, n_items, 4096, 0 if by == "user" else 1, 77, 3)
    n_user1 = int((u[:4096] == 1).sum())
    print(f"user 1 in the first 4096 slots: {n_user1} slots, {n_fallback} direct draws over all users")
    assert n_fallback > 0.5 * n_user1


# ------------------------------------------------------------------------------------------ 3. bit-exactness
@pytest.mark.parametrize("by", ["user", "interaction"])
def test_kernel_reproduces_the_documented_stream_bit_for_bit(epinion2, by):
    from spex_amd import ops
    mode = 0 if by == "user" else 1
    _, _, n_items, (rowptr, items, active) = law_tables()
    seed, epoch = 0xFEDCBA9876543210, 0x80000005                      # both key words and the epoch word's top bit in use
    got = ops.sample_bpr_triples(t(rowptr), t(items), t(active), n_items, 4096, seed=seed, epoch=epoch, by=by)
    want = reference_triples(rowptr, items, active, n_items, 4096, mode, seed, epoch)
    assert want[3] > 100                                              # the direct draw is exercised
    for g, w, name in zip(got, want, ("users", "pos", "neg")):
        assert np.array_equal(g.cpu().numpy(), w), f"8 x 16 graph, {name}"
    rowptr, items, active = epi_tables(epinion2)
    s = epi_sampler(epinion2, seed=2020, by=by)
    got = s.draw(7)
    want = reference_triples(rowptr, items, active, N_I, s.n, mode, 2020, 7)
    print(f"by={by}: Epinion2, {s.n} slots, {want[3]} direct draws")
    for g, w, name in zip(got, want, ("users", "pos", "neg")):
        assert np.array_equal(g.cpu().numpy(), w), f"Epinion2, {name}"


# ------------------------------------------------------------------------------------------ 4. prefix, determinism
@pytest.mark.parametrize("by", ["user", "interaction"])
def test_draws_are_a_function_of_seed_epoch_and_slot(epinion2, by):
    s = epi_sampler(epinion2, seed=9, by=by)
    assert not callable(s)
    full = s.draw(0)
    again = s.draw(0)
    short = epi_sampler(epinion2, seed=9, by=by, n=1000).draw(0)
    other_epoch = s.draw(1)
    other_seed = epi_sampler(epinion2, seed=10, by=by).draw(0)
    for k in range(3):
        assert torch.equal(full[k], again[k])
        assert short[k].shape == (1000,) and torch.equal(short[k], full[k][:1000])
        assert not torch.equal(full[k], other_epoch[k]) and not torch.equal(full[k], other_seed[k])
        assert (full[k] != other_epoch[k]).float().mean().item() > 0.5


# ------------------------------------------------------------------------------------------ 5. argument checks
def test_rejected_arguments_return_a_negative_status_and_touch_nothing():
    from spex_amd import _lib
    lib = _lib.load()
    _, _, n_items, (rowptr, items, active) = law_tables()
    r, i, a = t(rowptr), t(items), t(active)
    out = [torch.full((64,), 7, dtype=torch.int64, device=DEV) for _ in range(3)]
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    good = dict(rowptr=vp(r), items=vp(i), n_rows=len(rowptr) - 1, active=vp(a), n_active=len(active), num_item=n_items, n=64, mode=0,
                users=vp(out[0]), pos=vp(out[1]), neg=vp(out[2]))

    def call(**kw):
        k = dict(good, **kw)
        rc = lib.spex_sample_bpr_triples(k["rowptr"], k["items"], k["n_rows"], k["active"], k["n_active"], k["num_item"], k["n"], k["mode"], 5, 0,
                                         k["users"], k["pos"], k["neg"], None)
        return rc, lib.spex_last_error().decode()

    cases = [dict(rowptr=None), dict(items=None), dict(active=None), dict(users=None), dict(pos=None), dict(neg=None), dict(n=-1),
             dict(n_active=0), dict(num_item=0), dict(mode=2), dict(mode=-1)]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "spex_sample_bpr_triples" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all(bool((x == 7).all()) for x in out)
    rc, _ = call(n=0, n_active=0)                                     # nothing to draw: OK, nothing launched
    assert rc == 0
    torch.cuda.synchronize()
    assert all(bool((x == 7).all()) for x in out)
    rc, _ = call()
    torch.cuda.synchronize()
    assert rc == 0 and all(bool((x != 7).any()) for x in out[:1])


def test_sampled_epoch_checks_its_arguments_before_the_sampler_runs(epinion2):
    from spex_amd import _lib
    lib = _lib.load()
    st = stepper(epinion2)
    s = epi_sampler(epinion2, n=3 * T)
    bufs = s.epoch_buffers()
    for b in bufs:
        b.fill_(7)
    acc = torch.zeros(2, 1, device=DEV)
    d = st._prepare_desc(T, 3)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(mode=0, keep_prob=1.0, n_active=s.active.numel(), loss=vp(acc[0])):
        rc = lib.spex_lightgcn_epoch_bpr_sampled_f32(ctypes.byref(d), vp(s.rowptr), vp(s.items), N_U, vp(s.active), n_active, N_I, s.n, mode, 1, 0,
                                                     T, -1, keep_prob, 0, vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), loss, vp(acc[1]), None)
        return rc, lib.spex_last_error().decode()

    for kw in (dict(mode=3), dict(keep_prob=0.0), dict(n_active=0), dict(loss=None)):
        rc, msg = call(**kw)
        assert rc < 0 and msg, (kw, rc, msg)
    rc, msg = lib.spex_lightgcn_train_bpr_sampled_f32(ctypes.byref(d), vp(s.rowptr), vp(s.items), N_U, vp(s.active), s.active.numel(), N_I, s.n, 0, 1,
                                                      0, 2, T, -1, 1.0, 0, vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), None, None), lib.spex_last_error()
    assert rc < 0 and b"loss_epochs" in msg
    torch.cuda.synchronize()
    assert d.t == 0 and all(bool((b == 7).all()) for b in bufs) and not acc.any()
    with pytest.raises(ValueError, match="n >= 1"):
        st.epoch_bpr_sampled(epi_sampler(epinion2, n=0), 0, T, acc[0], acc[1])


# ------------------------------------------------------------------------------------------ 6. the sampled epoch
@pytest.mark.parametrize("deterministic", [False, True])
def test_sampled_epoch_equals_draw_followed_by_the_native_epoch(epinion2, deterministic):
    for n, max_steps, steps in ((None, 10, 10), (3 * T + 77, None, 4)):
        s = epi_sampler(epinion2, seed=31, n=n)
        a, b = stepper(epinion2, deterministic), stepper(epinion2, deterministic)
        acc_a, acc_b = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
        a.epoch_bpr_sampled(s, 4, T, acc_a[0], acc_a[1], max_steps=max_steps)
        u, p, ng = s.draw(4)
        assert all(torch.equal(x, y) for x, y in zip(s.epoch_buffers(), (u, p, ng)))
        b.epoch_bpr(u, p, ng, T, acc_b[0], acc_b[1], max_steps=max_steps)
        assert a.t == steps
        k = 1 if n is None else 2                                     # (no ragged batch in the first run: its accumulator stays 0)
        assert not acc_a[1].any() if n is None else acc_a[1].item() != 0.0
        compare(f"sampled epoch, {steps} steps", acc_a.cpu().numpy().ravel()[:k], acc_b.cpu().numpy().ravel()[:k], a, b, deterministic)


def test_train_epoch_bpr_takes_a_sampler_and_device_triples(epinion2):
    """train_epoch_bpr with a BprDeviceSampler takes epoch_bpr_sampled (once); with step_losses it draws and loops; a tuple of device
    tensors is trained on where it is.  All three agree with draw() + epoch_bpr in the deterministic mode, bit for bit."""
    from spex_amd.trainer import train_epoch_bpr
    s = epi_sampler(epinion2, seed=5)
    ref = stepper(epinion2, True)
    acc = torch.zeros(2, 1, device=DEV)
    ref.epoch_bpr(*s.draw(2), T, acc[0], acc[1], max_steps=4)
    want = acc[0].item() / T
    a = stepper(epinion2, True)
    calls = []
    inner = a.epoch_bpr_sampled
    a.epoch_bpr_sampled = lambda *x, **k: (calls.append(1), inner(*x, **k))[1]
    got_a = train_epoch_bpr(a, s, batch_size=T, max_steps=4, epoch=2).item()
    assert calls == [1]
    b = stepper(epinion2, True)
    losses = []
    got_b = train_epoch_bpr(b, s, batch_size=T, max_steps=4, epoch=2, step_losses=losses).item()
    c = stepper(epinion2, True)
    got_c = train_epoch_bpr(c, s.draw(2), batch_size=T, max_steps=4).item()
    assert len(losses) == 4
    for st, got in ((a, got_a), (b, got_b), (c, got_c)):
        assert st.t == 4 and torch.equal(st.E0, ref.E0) and torch.equal(st.m, ref.m) and torch.equal(st.v, ref.v)
        assert abs(got - want) <= 2e-6 * abs(want)
    assert got_a == want and got_c == want


# ------------------------------------------------------------------------------------------ 7. the multi-epoch driver
@pytest.mark.parametrize("deterministic", [False, True])
def test_train_epochs_bpr_with_a_device_sampler(epinion2, deterministic):
    from spex_amd.trainer import train_epochs_bpr
    s = epi_sampler(epinion2, seed=13)
    runs = []
    for _ in range(2 if deterministic else 1):
        a = stepper(epinion2, deterministic)
        calls = []
        inner = a.train_bpr_sampled
        a.train_bpr_sampled = lambda *x, **k: (calls.append(1), inner(*x, **k))[1]
        totals = train_epochs_bpr(a, s, 3, batch_size=T, max_steps=5)
        assert calls == [1] and a.t == 15 and len(totals) == 3 and all(isinstance(x, float) for x in totals)
        runs.append((a, totals))
    a, totals = runs[0]
    if deterministic:
        a2, totals2 = runs[1]
        assert totals == totals2 and torch.equal(a.E0, a2.E0) and torch.equal(a.m, a2.m) and torch.equal(a.v, a2.v)
    # the epoch-by-epoch loop over draw(e)
    b = stepper(epinion2, deterministic)
    want = []
    for e in range(3):
        acc = torch.zeros(2, 1, device=DEV)
        b.epoch_bpr(*s.draw(e), T, acc[0], acc[1], max_steps=5)
        want.append(acc[0].item() / T)
    compare("train_epochs_bpr, one call", totals, want, a, b, deterministic)
    assert len(set(totals)) == 3
    # with after_epoch: one native call per epoch, the callback between them, the same run
    c = stepper(epinion2, deterministic)
    seen = []
    inner_c = c.train_bpr_sampled
    c.train_bpr_sampled = lambda *x, **k: (seen.append("train"), inner_c(*x, **k))[1]
    totals_c = train_epochs_bpr(c, s, 3, batch_size=T, max_steps=5, after_epoch=lambda e, total: seen.append((e, float(total), c.t)))
    assert [x[0] for x in seen] == [0, 1, 2] and [x[2] for x in seen] == [5, 10, 15]
    assert [x[1] for x in seen] == totals_c
    compare("train_epochs_bpr, after_epoch", totals_c, want, c, b, deterministic)


# ------------------------------------------------------------------------------------------ 8. edge dropout
def test_sampled_epochs_under_edge_dropout_wear_a_fresh_mask_sequence_per_epoch(epinion2):
    from spex_amd.trainer import bpr_epoch_drop_seed, edge_dropout_mask, train_epochs_bpr
    s = epi_sampler(epinion2, seed=17)
    a = stepper(epinion2, transposed=True)
    totals = train_epochs_bpr(a, s, 2, batch_size=T, max_steps=3, edge_dropout=(0.3, "philox", 5))
    assert a.t == 6
    seeds = [bpr_epoch_drop_seed(5, e) for e in range(2)]
    assert seeds == [5, (5 + 0x9E3779B9) & 0xFFFFFFFF]                # the documented function; epoch 0 keeps the seed
    b = stepper(epinion2, transposed=True)
    want = []
    for e in range(2):
        u, p, ng = s.draw(e)
        total = 0.0
        for k in range(3):
            acc = torch.zeros(1, device=DEV)
            b.set_edge_dropout(edge_dropout_mask(b.graph, 0.3, "philox", seeds[e], k + 1))
            b.step_bpr_exact(u[k * T:(k + 1) * T], p[k * T:(k + 1) * T], ng[k * T:(k + 1) * T], loss_acc=acc, batch_rows_only=True)
            total += acc.item() / T
        want.append(total)
    b.set_edge_dropout(None)
    figs = (float(np.abs(np.array(totals) - np.array(want)).max() / np.abs(want).max()), rel_err(a.E0.cpu().numpy(), b.E0.cpu().numpy()))
    print(f"sampled epochs under dropout: loss {figs[0]:.2e} E0 {figs[1]:.2e}")
    assert figs[0] <= 2e-5 and figs[1] <= 2e-5
    # epoch 1's masks are not epoch 0's: the masked operator of step 1 differs between the two epochs
    X = t(epi(epinion2)[1])
    prods = []
    for e in range(2):
        b.set_edge_dropout(edge_dropout_mask(b.graph, 0.3, "philox", seeds[e], 1))
        prods.append(b.graph.spmm(X).clone())
    b.set_edge_dropout(None)
    assert not torch.equal(prods[0], prods[1])
    # ... and a run that replays epoch 0's sequence in epoch 1 (what one drop_seed for every epoch gives) ends elsewhere
    c = stepper(epinion2, transposed=True)
    for e in range(2):
        acc = torch.zeros(2, 1, device=DEV)
        c.epoch_bpr(*s.draw(e), T, acc[0], acc[1], max_steps=3, keep_prob=0.3, drop_seed=5)
    assert rel_err(c.E0.cpu().numpy(), a.E0.cpu().numpy()) > 1e-4
    # the handles are left unmasked
    plain = stepper(epinion2, transposed=True)
    assert torch.equal(a.graph.spmm(X), plain.graph.spmm(X)) and torch.equal(a.graph_t.spmm(X), plain.graph_t.spmm(X))
    # the epoch-by-epoch form (after_epoch) wears the same masks
    d = stepper(epinion2, transposed=True)
    fired = []
    totals_d = train_epochs_bpr(d, s, 2, batch_size=T, max_steps=3, edge_dropout=(0.3, "philox", 5), after_epoch=lambda e, x: fired.append(e))
    assert fired == [0, 1]
    assert np.abs(np.array(totals_d) - np.array(totals)).max() <= 2e-5 * np.abs(totals).max()
    assert rel_err(d.E0.cpu().numpy(), a.E0.cpu().numpy()) <= 2e-5
