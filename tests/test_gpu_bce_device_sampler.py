"""BCE epochs drawn on the device (spex_sample_bce_epoch: negatives, labels and the shuffle in one launch) and the sampled epochs built
on them (spex_lightgcn_epoch_bce_sampled_f32, spex_lightgcn_train_bce_sampled_f32; trainer.BceDeviceSampler, train_epoch / train_epochs
with a sampler).

The stream is restated in NumPy from the text of include/spex_hip.h (test_host_bce_device_sampler.reference_epoch) and the kernel must
reproduce it bit for bit; validity is exact; the negative law, the shuffle's grid and the positives per batch are held to the binomial
6 sigma bounds of test_host_bce_device_sampler.py (validated there on the host path).  The training comparisons issue the same launches
on both sides: the deterministic mode is compared with torch.equal, the fast mode within the native-epoch bounds of
test_gpu_wide_step.py::test_native_epoch_at_wide_widths (loss 2e-6, E0 and m 2e-5, v 4e-5: float-atomic order only).

One full Epinion2 epoch (seed 2020, epoch 0: n = 1 255 824) is drawn once, restated once, and shared by the tests that read it."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from test_host_bce_device_sampler import (check_negative_law, check_positives_per_batch, check_shuffle_grid, check_validity, half_bits, perm,
                                          reference_epoch)
from test_host_bpr_device_sampler import law_graph

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_U, N_I = 3186, 12407
B = 256
EPOCH_BOUNDS = (2e-6, 2e-5, 2e-5, 4e-5)          # loss, E0, m, v: test_gpu_wide_step.py::test_native_epoch_at_wide_widths

_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------ fixtures
def law_tables():
    if "law" not in _cache:
        from spex_amd.trainer import bpr_sampler_tables
        pairs, n_users, n_items = law_graph()
        _cache["law"] = (pairs, n_users, n_items, bpr_sampler_tables(pairs, n_users, n_items))
    return _cache["law"]


def epi_sampler(epinion2, seed=2020, prefix=None, num_ng=5, device=DEV):
    from spex_amd.trainer import BceDeviceSampler
    return BceDeviceSampler(epinion2["train"][:prefix, :2], N_U, N_I, num_ng=num_ng, seed=seed, device=device)


def epi_epoch(epinion2):
    """The shared Epinion2 epoch: (sampler, the kernel's (users, items, labels) as host arrays)."""
    if "epoch" not in _cache:
        s = epi_sampler(epinion2)
        out = s.draw(0)
        assert out[0].dtype == out[1].dtype == torch.int64 and out[2].dtype == torch.float32
        assert all(x.is_cuda and x.shape == (s.n,) for x in out)
        _cache["epoch"] = (s, tuple(x.cpu().numpy() for x in out))
    return _cache["epoch"]


def epi_reference(epinion2):
    """The NumPy restatement of the shared epoch: (users, items, labels, source per slot, direct draws)."""
    if "reference" not in _cache:
        s, _ = epi_epoch(epinion2)
        pairs = epinion2["train"][:, :2]
        _cache["reference"] = reference_epoch(s.rowptr.cpu().numpy(), s.items.cpu().numpy(), pairs[:, 0], pairs[:, 1], 5, N_I, 2020, 0)
    return _cache["reference"]


def epi(epinion2, d):
    """(csr, E0) of Epinion2 at width d: the LightGCN adjacency, E0 ~ U(-b, b) from default_rng(2020) (test_gpu_wide_step.py)."""
    if "csr" not in _cache:
        from spex_amd.graph import lightgcn_norm_adj
        tr = epinion2["train"]
        _cache["csr"] = lightgcn_norm_adj(tr[:, 0], tr[:, 1], N_U - 1, N_I)
    if d not in _cache:
        from spex_amd.datasets import epinion2_tables
        _cache[d] = np.concatenate(epinion2_tables(N_U, N_I, dim=d))
    return _cache["csr"], _cache[d]


def stepper(epinion2, d=64, deterministic=False, transposed=False):
    from spex_amd.graph import SpexGraph, csr_transpose
    from spex_amd.trainer import LightGCNStepper
    csr, E0 = epi(epinion2, d)
    gt = None
    if transposed:
        if "csr_t" not in _cache:
            _cache["csr_t"] = csr_transpose(*csr, len(E0))
        t_rowptr, t_col, t_val, eid = _cache["csr_t"]
        gt = SpexGraph(t_rowptr, t_col, t_val, edge_id=eid)
    return LightGCNStepper(SpexGraph(*csr), t(E0.copy()), N_U, n_layers=3, lr=1e-3, graph_t=gt, deterministic=deterministic)


def state(st):
    return st.E0.cpu().numpy(), st.m.cpu().numpy(), st.v.cpu().numpy()


def compare(tag, loss_a, loss_b, st_a, st_b, deterministic, bounds=EPOCH_BOUNDS):
    loss_a, loss_b = np.asarray(loss_a, np.float64).ravel(), np.asarray(loss_b, np.float64).ravel()
    assert loss_a.shape == loss_b.shape and np.all(loss_b != 0)
    figs = (float((np.abs(loss_a - loss_b) / np.abs(loss_b)).max()),) + tuple(rel_err(x, y) for x, y in zip(state(st_a), state(st_b)))
    print(f"{tag} det={deterministic}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert st_a.t == st_b.t
    assert all(f <= b for f, b in zip(figs, bounds)), (tag, figs, bounds)
    if deterministic:
        assert torch.equal(st_a.E0, st_b.E0) and torch.equal(st_a.m, st_b.m) and torch.equal(st_a.v, st_b.v)
        assert np.array_equal(loss_a, loss_b)


# ------------------------------------------------------------------------------------------ 1. validity
def test_every_sample_is_valid_on_epinion2(epinion2):
    s, (u, i, y) = epi_epoch(epinion2)
    pairs = epinion2["train"][:, :2]
    assert s.n_pos == len(pairs) == 209304 and s.n == 1255824
    check_validity(u, i, y, pairs, pairs, N_U, N_I, 5)


# ------------------------------------------------------------------------------------------ 2. the negative law
def test_negative_law_on_the_8_by_16_graph():
    """2^20 slots: 2^18 positives (the graph's pairs repeated) with 3 negatives each.  User 0 has no positive, user 1 holds 15 of 16
    items (every negative is item 15; eight rejections fail with probability (15/16)^8 = 0.60: the direct draw), user 2 holds one."""
    from spex_amd import ops
    pairs, n_users, n_items, (rowptr, items, _) = law_tables()
    P, num_ng = 1 << 18, 3
    positives = np.tile(pairs, (-(-P // len(pairs)), 1))[:P]
    u, i, y = (x.cpu().numpy() for x in ops.sample_bce_epoch(t(rowptr), t(items), t(positives[:, 0].astype(np.int32)),
                                                             t(positives[:, 1].astype(np.int32)), num_ng, n_items, seed=77, epoch=3))
    assert len(u) == 1 << 20
    check_validity(u, i, y, positives, pairs, n_users, n_items, num_ng)
    worst, smallest, cells = check_negative_law(u, i, y, positives, pairs, n_users, n_items, num_ng)
    print(f"{cells} (user, negative) cells, largest deviation {worst:.2f} sigma, smallest expected count {smallest:.0f}")
    assert smallest > 1000
    assert (u == 0).sum() == 0
    neg1 = (u == 1) & (y == 0)
    assert neg1.sum() == 3 * (positives[:, 0] == 1).sum() > 100000 and np.all(i[neg1] == 15)
    # the direct draw is what serves user 1: in the restated stream of a 4 096-positive prefix most of its negatives take it
    ref = reference_epoch(rowptr, items, positives[:4096, 0], positives[:4096, 1], num_ng, n_items, 77, 3)
    n_user1 = int(((ref[0] == 1) & (ref[2] == 0)).sum())
    print(f"4 096-positive prefix: user 1 has {n_user1} negatives, {ref[4]} direct draws over all users")
    assert ref[4] > 0.5 * n_user1


# ------------------------------------------------------------------------------------------ 3. the shuffle law
def test_shuffle_law_on_one_epinion2_epoch(epinion2):
    """The positives per batch are counted on the kernel's own labels.  The grid needs every slot's source index, which the outputs
    do not carry: it is the restated perm's — after the kernel's users and labels are shown to be that perm's, slot by slot (the
    bit-exactness test holds the items to it as well)."""
    s, (u, i, y) = epi_epoch(epinion2)
    z_mean, z_max, ratio = check_positives_per_batch(y, 5, batch=B)
    print(f"positives per batch of {B}: {len(y) // B} full batches, mean {z_mean:.2f} standard errors from {B / 6:.3f}, worst batch "
          f"{z_max:.2f} sigma, variance {ratio:.3f} x binomial")
    ref_u, _, ref_y, src, _ = epi_reference(epinion2)
    assert np.array_equal(u, ref_u) and np.array_equal(y, ref_y)
    worst = check_shuffle_grid(src, grid=16)
    print(f"16 x 16 (slot bucket, source bucket) grid: largest deviation {worst:.2f} sigma")


# ------------------------------------------------------------------------------------------ 4. bit-exactness
@pytest.mark.parametrize("num_ng", [1, 4, 5])
@pytest.mark.parametrize("P", [1, 2, 43, 683])
def test_kernel_reproduces_the_documented_stream_on_small_epochs(P, num_ng):
    """n = 2 .. 4 098: both sides of a Feistel domain boundary (n = 4 096 / 4 098 at P = 683, n = 258 at P = 43, num_ng = 5) and domains
    up to four times n, where a slot walks the cycle many times."""
    from spex_amd import ops
    pairs, _, n_items, (rowptr, items, _) = law_tables()
    positives = np.tile(pairs, (-(-(P + 3) // len(pairs)), 1))[3:3 + P]          # (from user 1's row on: P = 1 is a direct draw)
    seed, epoch = 0xFEDCBA9876543210, 0x80000005                      # both key words and the epoch word's top bit in use
    n = P * (1 + num_ng)
    got = ops.sample_bce_epoch(t(rowptr), t(items), t(positives[:, 0].astype(np.int32)), t(positives[:, 1].astype(np.int32)), num_ng, n_items,
                               seed=seed, epoch=epoch)
    want = reference_epoch(rowptr, items, positives[:, 0], positives[:, 1], num_ng, n_items, seed, epoch)
    walks = perm(n, seed, epoch)[1]
    print(f"P={P} num_ng={num_ng}: n {n}, domain {1 << (2 * half_bits(n))}, walks mean {walks.mean():.2f} max {walks.max()}, {want[4]} direct draws")
    for g, w, name in zip(got, want, ("users", "items", "labels")):
        assert np.array_equal(g.cpu().numpy(), w), f"n = {n}, {name}"
    assert got[2].dtype == torch.float32
    if n == 4098:
        assert 1 << (2 * half_bits(n)) == 16384 and walks.max() >= 8    # a cycle-walk of many steps


def test_kernel_reproduces_the_documented_stream_on_epinion2_and_the_law_graph(epinion2):
    from spex_amd import ops
    _, got = epi_epoch(epinion2)
    want = epi_reference(epinion2)
    walks = perm(len(got[0]), 2020, 0)[1]
    print(f"Epinion2: {len(got[0])} slots, walks mean {walks.mean():.2f} max {walks.max()}, {want[4]} direct draws")
    for g, w, name in zip(got, want, ("users", "items", "labels")):
        assert np.array_equal(g, w), f"Epinion2, {name}"
    pairs, _, n_items, (rowptr, items, _) = law_tables()
    positives = np.tile(pairs, (100, 1))
    got = ops.sample_bce_epoch(t(rowptr), t(items), t(positives[:, 0].astype(np.int32)), t(positives[:, 1].astype(np.int32)), 5, n_items,
                               seed=0x123456789ABCDEF, epoch=2)
    want = reference_epoch(rowptr, items, positives[:, 0], positives[:, 1], 5, n_items, 0x123456789ABCDEF, 2)
    assert want[4] > 1000                                             # the direct draw is exercised
    for g, w, name in zip(got, want, ("users", "items", "labels")):
        assert np.array_equal(g.cpu().numpy(), w), f"8 x 16 graph, {name}"


# ------------------------------------------------------------------------------------------ 5. a function of (seed, epoch, slot)
def test_draws_are_a_function_of_seed_and_epoch(epinion2):
    s = epi_sampler(epinion2, seed=9, prefix=20000)
    assert not callable(s) and not hasattr(s, "ng_sample")
    full, again, other_epoch = s.draw(0), s.draw(0), s.draw(1)
    other_seed = epi_sampler(epinion2, seed=10, prefix=20000).draw(0)
    bufs = s.epoch_buffers()
    from spex_amd import ops
    into = ops.sample_bce_epoch(s.rowptr, s.items, s.pos_user, s.pos_item, s.num_ng, s.n_items, s.seed, 0, out=bufs)
    for k in range(3):
        assert torch.equal(full[k], again[k]) and torch.equal(full[k], into[k]) and into[k].data_ptr() == bufs[k].data_ptr()
        assert not torch.equal(full[k], other_epoch[k]) and not torch.equal(full[k], other_seed[k])
    assert (full[0] != other_epoch[0]).float().mean().item() > 0.5 and (full[0] != other_seed[0]).float().mean().item() > 0.5


# ------------------------------------------------------------------------------------------ 6. argument checks
def test_rejected_arguments_return_a_negative_status_and_touch_nothing():
    from spex_amd import _lib
    lib = _lib.load()
    pairs, _, n_items, (rowptr, items, _) = law_tables()
    r, i, pu, pi = t(rowptr), t(items), t(pairs[:, 0].astype(np.int32)), t(pairs[:, 1].astype(np.int32))
    n = len(pairs) * 6
    out = [torch.full((n,), 99, dtype=torch.int64, device=DEV), torch.full((n,), 99, dtype=torch.int64, device=DEV),
           torch.full((n,), 99.0, dtype=torch.float32, device=DEV)]
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    good = dict(rowptr=vp(r), items=vp(i), n_rows=len(rowptr) - 1, pos_user=vp(pu), pos_item=vp(pi), n_pos=len(pairs), num_ng=5, num_item=n_items,
                users=vp(out[0]), items_out=vp(out[1]), labels=vp(out[2]))

    def call(**kw):
        k = dict(good, **kw)
        rc = lib.spex_sample_bce_epoch(k["rowptr"], k["items"], k["n_rows"], k["pos_user"], k["pos_item"], k["n_pos"], k["num_ng"], k["num_item"],
                                       5, 0, k["users"], k["items_out"], k["labels"], None)
        return rc, lib.spex_last_error().decode()

    cases = [dict(rowptr=None), dict(items=None), dict(pos_user=None), dict(pos_item=None), dict(users=None), dict(items_out=None),
             dict(labels=None), dict(num_ng=0), dict(num_ng=-1), dict(n_pos=-1), dict(num_item=0), dict(n_rows=-1),
             dict(n_pos=(1 << 31) // 6 + 1), dict(n_pos=1 << 30, num_ng=1), dict(n_pos=1 << 40), dict(n_pos=1 << 62, num_ng=7)]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "spex_sample_bce_epoch" in msg, (kw, rc, msg)
    assert "2^31" in call(n_pos=(1 << 31) // 6 + 1)[1] and "NULL" in call(labels=None)[1] and "num_ng" in call(num_ng=0)[1]
    torch.cuda.synchronize()
    assert all(bool((x == 99).all()) for x in out)
    rc, _ = call(n_pos=0)                                             # nothing to draw: OK, nothing launched
    assert rc == 0
    torch.cuda.synchronize()
    assert all(bool((x == 99).all()) for x in out)
    rc, _ = call()
    torch.cuda.synchronize()
    assert rc == 0 and all(bool((x != 99).all()) for x in out)        # (users < 8, items < 16, labels 0 / 1)


def test_sampled_epoch_checks_its_arguments_before_the_sampler_runs(epinion2):
    from spex_amd import _lib
    lib = _lib.load()
    st = stepper(epinion2)
    s = epi_sampler(epinion2, prefix=1000)
    bufs = s.epoch_buffers()
    for b in bufs:
        b.fill_(7)
    acc = torch.zeros(2, 1, device=DEV)
    d = st._prepare_desc(B)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(num_ng=5, keep_prob=1.0, batch=B, loss=vp(acc[0]), n_pos=s.n_pos, labels=vp(bufs[2])):
        rc = lib.spex_lightgcn_epoch_bce_sampled_f32(ctypes.byref(d), vp(s.rowptr), vp(s.items), N_U, vp(s.pos_user), vp(s.pos_item), n_pos, num_ng,
                                                     N_I, 1, 0, batch, -1, keep_prob, 0, vp(bufs[0]), vp(bufs[1]), labels, loss, vp(acc[1]), None)
        return rc, lib.spex_last_error().decode()

    for kw in (dict(num_ng=0), dict(keep_prob=0.0), dict(batch=0), dict(loss=None), dict(labels=None), dict(n_pos=1 << 31)):
        rc, msg = call(**kw)
        assert rc < 0 and msg, (kw, rc, msg)
    rc, msg = lib.spex_lightgcn_train_bce_sampled_f32(ctypes.byref(d), vp(s.rowptr), vp(s.items), N_U, vp(s.pos_user), vp(s.pos_item), s.n_pos, 5, N_I,
                                                      1, 0, 2, B, -1, 1.0, 0, vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), None, None), lib.spex_last_error()
    assert rc < 0 and b"loss_epochs" in msg
    torch.cuda.synchronize()
    assert d.t == 0 and all(bool((b == 7).all()) for b in bufs) and not acc.any()
    # the Python layer: a sampler on another device than the stepper, an empty sampler
    with pytest.raises(ValueError, match="the sampler's tables live on cpu"):
        st.epoch_bce_sampled(epi_sampler(epinion2, prefix=1000, device="cpu"), 0, B, acc[0], acc[1])
    with pytest.raises(ValueError, match="the sampler's tables live on cpu"):
        st.train_bce_sampled(epi_sampler(epinion2, prefix=1000, device="cpu"), 2, B, torch.zeros(4, device=DEV))
    from spex_amd.trainer import train_epoch
    with pytest.raises(ValueError, match="the sampler's tables live on cpu"):
        train_epoch(st, epi_sampler(epinion2, prefix=1000, device="cpu"), step_losses=[])
    with pytest.raises(ValueError, match="n >= 1"):
        st.epoch_bce_sampled(epi_sampler(epinion2, prefix=0), 0, B, acc[0], acc[1])
    with pytest.raises(ValueError, match="loss_epochs"):
        st.train_bce_sampled(s, 3, B, torch.zeros(4, device=DEV))
    assert st.t == 0


# ------------------------------------------------------------------------------------------ 7. the sampled epoch
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("deterministic", [False, True])
def test_sampled_epoch_equals_draw_followed_by_the_native_epoch(epinion2, d, deterministic):
    """A 1 000-pair prefix of Epinion2: n = 6 000 = 23 full batches of 256 and a ragged one of 112."""
    s = epi_sampler(epinion2, seed=31, prefix=1000)
    assert s.n == 6000
    a, b = stepper(epinion2, d, deterministic), stepper(epinion2, d, deterministic)
    acc_a, acc_b = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
    a.epoch_bce_sampled(s, 4, B, acc_a[0], acc_a[1])
    u, i, y = s.draw(4)
    assert all(torch.equal(x, z) for x, z in zip(s.epoch_buffers(), (u, i, y)))
    b.epoch_bce(u, i, y, B, acc_b[0], acc_b[1])
    assert a.t == 24 and acc_a[1].item() != 0.0
    compare(f"sampled epoch d={d}", acc_a.cpu().numpy(), acc_b.cpu().numpy(), a, b, deterministic)


# ------------------------------------------------------------------------------------------ 8. several epochs in one call
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("deterministic", [False, True])
def test_three_epochs_in_one_call_equal_three_per_epoch_calls(epinion2, d, deterministic):
    s = epi_sampler(epinion2, seed=13, prefix=1000)
    a, b = stepper(epinion2, d, deterministic), stepper(epinion2, d, deterministic)
    acc_a = torch.zeros(3, 2, device=DEV)
    a.train_bce_sampled(s, 3, B, acc_a, first_epoch=5)
    acc_b = torch.zeros(3, 2, device=DEV)
    for e in range(3):
        b.epoch_bce_sampled(s, 5 + e, B, acc_b[e, 0:1], acc_b[e, 1:2])
    assert a.t == 72
    got, want = acc_a.cpu().numpy(), acc_b.cpu().numpy()
    assert np.all(got != 0) and len(set(got[:, 0].tolist())) == 3     # [2 e]: full batches, [2 e + 1]: the ragged one, per epoch
    assert np.all(got[:, 0] > 10 * got[:, 1])                         # 23 x 256 samples against 112
    compare(f"three epochs d={d}", got, want, a, b, deterministic)


def test_sampled_epochs_under_edge_dropout_wear_a_fresh_mask_sequence_per_epoch(epinion2):
    from spex_amd.trainer import bpr_epoch_drop_seed, edge_dropout_mask
    s = epi_sampler(epinion2, seed=17, prefix=1000)
    a = stepper(epinion2, transposed=True)
    acc_a = torch.zeros(3, 2, device=DEV)
    a.train_bce_sampled(s, 3, B, acc_a, max_steps=3, keep_prob=0.5, drop_seed=5)
    assert a.t == 9 and not acc_a[:, 1].any()
    seeds = [bpr_epoch_drop_seed(5, e) for e in range(3)]
    assert seeds == [5, (5 + 0x9E3779B9) & 0xFFFFFFFF, (5 + 2 * 0x9E3779B9) & 0xFFFFFFFF]      # the documented rule; epoch 0 keeps the seed
    # the same steps one by one under edge_dropout_mask(.., "philox", bpr_epoch_drop_seed(seed, e), k + 1)
    b = stepper(epinion2, transposed=True)
    want = np.zeros(3)
    for e in range(3):
        u, i, y = s.draw(e)
        for k in range(3):
            acc = torch.zeros(1, device=DEV)
            b.set_edge_dropout(edge_dropout_mask(b.graph, 0.5, "philox", seeds[e], k + 1))
            b.step_bce(u[k * B:(k + 1) * B], i[k * B:(k + 1) * B], y[k * B:(k + 1) * B], loss_acc=acc, batch_rows_only=True)
            want[e] += acc.item()
    b.set_edge_dropout(None)
    compare("sampled epochs under dropout", acc_a[:, 0].cpu().numpy(), want, a, b, False)
    # the epochs' first-step masks differ from one another
    X = t(epi(epinion2, 64)[1])
    prods = []
    for e in range(3):
        b.set_edge_dropout(edge_dropout_mask(b.graph, 0.5, "philox", seeds[e], 1))
        prods.append(b.graph.spmm(X).clone())
    b.set_edge_dropout(None)
    assert not torch.equal(prods[0], prods[1]) and not torch.equal(prods[1], prods[2]) and not torch.equal(prods[0], prods[2])
    # ... and a run that replays epoch 0's sequence in every epoch (one drop_seed for all) ends elsewhere
    c = stepper(epinion2, transposed=True)
    for e in range(3):
        acc = torch.zeros(2, 1, device=DEV)
        c.epoch_bce_sampled(s, e, B, acc[0], acc[1], max_steps=3, keep_prob=0.5, drop_seed=5)
    assert rel_err(c.E0.cpu().numpy(), a.E0.cpu().numpy()) > 1e-4
    # the handles are left unmasked
    plain = stepper(epinion2, transposed=True)
    assert torch.equal(a.graph.spmm(X), plain.graph.spmm(X)) and torch.equal(a.graph_t.spmm(X), plain.graph_t.spmm(X))


# ------------------------------------------------------------------------------------------ 9. dispatch
def test_train_epoch_and_train_epochs_take_a_sampler(epinion2):
    """train_epoch with a BceDeviceSampler takes epoch_bce_sampled (once), train_epochs takes train_bce_sampled (once) — or one
    epoch_bce_sampled per epoch with after_epoch — and no thread is started; with step_losses the epoch is drawn by draw() and trained
    step by step.  Deterministic mode: all of them equal the explicit calls bit for bit."""
    from spex_amd.trainer import train_epoch, train_epochs
    s = epi_sampler(epinion2, seed=5, prefix=1000)
    n_threads = threading.active_count()
    seen = []

    def spy(st, name):
        inner = getattr(st, name)
        setattr(st, name, lambda *x, **k: (seen.append((name, threading.active_count())), inner(*x, **k))[1])

    def total(acc):                                                   # main_rec.py:36's sum of per-batch mean losses
        return acc[0].item() / B + acc[1].item() / (s.n % B)

    # one epoch
    ref = stepper(epinion2, deterministic=True)
    acc = torch.zeros(2, 1, device=DEV)
    ref.epoch_bce(*s.draw(2), B, acc[0], acc[1])
    want = total(acc)
    a = stepper(epinion2, deterministic=True)
    spy(a, "epoch_bce_sampled")
    got_a = train_epoch(a, s, batch_size=B, epoch=2).item()
    assert seen == [("epoch_bce_sampled", n_threads)]
    b = stepper(epinion2, deterministic=True)
    spy(b, "epoch_bce_sampled")
    draws = []
    inner_draw = s.draw
    s.draw = lambda e: (draws.append(e), inner_draw(e))[1]
    losses = []
    got_b = train_epoch(b, s, batch_size=B, epoch=2, step_losses=losses).item()
    del s.draw
    assert draws == [2] and len(seen) == 1 and len(losses) == 24 and all(0.1 < x < 2.0 for x in losses)
    for st, got in ((a, got_a), (b, got_b)):
        assert st.t == 24 and torch.equal(st.E0, ref.E0) and torch.equal(st.m, ref.m) and torch.equal(st.v, ref.v)
        assert abs(got - want) <= 2e-6 * abs(want)
    # three epochs
    ref = stepper(epinion2, deterministic=True)
    acc3 = torch.zeros(3, 2, device=DEV)
    ref.train_bce_sampled(s, 3, B, acc3)
    want3 = [total(acc3[e]) for e in range(3)]
    seen.clear()
    c = stepper(epinion2, deterministic=True)
    spy(c, "train_bce_sampled")
    totals = train_epochs(c, s, 3, batch_size=B)
    assert seen == [("train_bce_sampled", n_threads)] and len(totals) == 3 and all(isinstance(x, float) for x in totals)
    seen.clear()
    e_ = stepper(epinion2, deterministic=True)
    spy(e_, "train_bce_sampled")
    spy(e_, "epoch_bce_sampled")
    fired = []
    totals_e = train_epochs(e_, s, 3, batch_size=B, after_epoch=lambda ep, x: fired.append((ep, float(x), e_.t)))
    assert seen == [("epoch_bce_sampled", n_threads)] * 3
    assert [f[0] for f in fired] == [0, 1, 2] and [f[2] for f in fired] == [24, 48, 72] and [f[1] for f in fired] == totals_e
    for st, got in ((c, totals), (e_, totals_e)):
        assert st.t == 72 and torch.equal(st.E0, ref.E0) and torch.equal(st.m, ref.m) and torch.equal(st.v, ref.v)
        assert np.abs(np.array(got) - np.array(want3)).max() <= 2e-6 * np.abs(want3).max()
    assert threading.active_count() == n_threads
