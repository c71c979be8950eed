"""Wide embeddings (d = 128 / 256) on the batch-sized kernels, the one-call LightGCN step and the native epoch.

Inputs: the Epinion2 fixture with the Xavier-uniform tables of numpy.random.default_rng(2020) at the width under test, one synthetic
non-symmetric graph with rows beyond 1 024 entries and empty rows, batches of 1 / 3 / 17 / 256 samples with repeated users.
The CPU truth is oracle.lightgcn_loss_and_grad + oracle.adam_step (width-generic, pinned to the reference at d = 64).

Tolerances are those of the d == 64 tests of the same quantities (tests/test_gpu_kernels.py, test_gpu_dropin.py,
test_gpu_deterministic.py); each assertion names its source.  The Adam moments have no d == 64 test of their own: m is linear in the
gradient (the gradient's tolerance), v quadratic (twice that) — from the same state; over a few steps the bound of the table after
the same steps applies to m, twice it to v.  Every test prints the figures it asserts on."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDE = [128, 256]
N_U, N_I = 3186, 12407


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def random_csr(rng, n_rows, n_cols, degrees):
    rowptr = np.zeros(n_rows + 1, np.int64)
    cols = []
    for r in range(n_rows):
        k = min(int(degrees[r]), n_cols)
        cols.append(np.sort(rng.choice(n_cols, k, replace=False)))
        rowptr[r + 1] = rowptr[r] + k
    col = np.concatenate(cols).astype(np.int32)
    val = rng.normal(size=len(col)).astype(np.float32)
    return rowptr.astype(np.int32), col, val


_cache = {}


def epi(epinion2, d):
    """(csr, E0) of Epinion2 at width d: the LightGCN adjacency, E0 ~ U(-b, b) from default_rng(2020)."""
    if "csr" not in _cache:
        from spex_amd.graph import lightgcn_norm_adj
        tr = epinion2["train"]
        _cache["csr"] = lightgcn_norm_adj(tr[:, 0], tr[:, 1], N_U - 1, N_I)
    if d not in _cache:
        from spex_amd.datasets import epinion2_tables
        _cache[d] = np.concatenate(epinion2_tables(N_U, N_I, dim=d))
    return _cache["csr"], _cache[d]


def hub_graph():
    """A non-symmetric square matrix with rows beyond 1 024 entries, empty rows, a one-entry row and rows at the 64 / 65 segment
    boundary (the generator of the d == 64 hub-row tests)."""
    if "hub" not in _cache:
        rng = np.random.default_rng(5)
        n, n_u = 3000, 1000
        deg = rng.integers(1, 50, n)
        deg[[2, 1500, 2999]] = [1500, 2600, 1100]
        deg[[7, 8, 9, 10]] = [0, 1, 64, 65]
        deg[[1200, 1201, 1202, 1203]] = [1, 0, 65, 64]
        rowptr, col, val = random_csr(rng, n, n, deg)
        _cache["hub"] = ((rowptr, col, val * np.float32(0.05)), n_u)
    return _cache["hub"]


def training_batches(epinion2, n_steps, B=256, seed=5):
    """Batches shaped like the reference's (a random observed pair or one of its same-user negatives): users repeat inside a batch."""
    rng = np.random.default_rng(seed)
    train = epinion2["train"]
    out = []
    for _ in range(n_steps):
        k = rng.integers(0, len(train), B)
        u, i = train[k, 0].copy(), train[k, 1].copy()
        if B > 1:
            u[-1] = u[0]                                  # a repeated user in every batch, however small
        neg = rng.random(B) < 5 / 6
        i[neg] = rng.integers(0, N_I, int(neg.sum()))
        out.append((u.astype(np.int64), i.astype(np.int64), (~neg).astype(np.float32)))
    return out


@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


# ------------------------------------------------------------------------------------------ 1. the batch kernel's forward rows
@pytest.mark.parametrize("d", WIDE)
@pytest.mark.parametrize("B", [1, 3, 17, 256])
def test_batch_kernel_forward_rows_are_the_spmm_rows(G, oracle, epinion2, d, B):
    """The propagated rows the batch kernel forms, read back EXACTLY through the slots form: a sample that pairs row r with an empty
    row whose running sum is zero has x = 0, sigmoid(x) = 1/2, and with label 0 and grad_scale 2 its dg is exactly 1 — the sample's
    gradient slot on the empty row's side IS light_r.  Those rows equal the rows of graph.spmm with the layer mean fused, at the same
    width: bit for bit for rows of <= 1 024 entries, within the d == 64 hub-row tolerance (3e-6 against the oracle:
    test_spmm_rowlist_is_the_full_product_at_the_listed_rows, test_gpu_kernels.py) beyond.  spex_spmm_rowlist_f32 gives the same rows."""
    from spex_amd import ops
    for name in ("epinion2", "hubs"):
        if name == "epinion2":
            csr, E0 = epi(epinion2, d)
            n_u, empty_u, empty_i = N_U, N_U - 1, 1324
        else:
            csr, n_u = hub_graph()
            E0 = (np.random.default_rng(d).normal(size=(len(csr[0]) - 1, d)) * 0.3).astype(np.float32)
            empty_u, empty_i = 7, 1201 - n_u
        n = len(csr[0]) - 1
        deg = np.diff(csr[0])
        assert deg[empty_u] == 0 and deg[n_u + empty_i] == 0
        rng = np.random.default_rng(100 * d + B)
        run = (rng.normal(size=(n, d)) * 0.05).astype(np.float32)
        run[empty_u] = 0.0
        run[n_u + empty_i] = 0.0
        half = (B + 1) // 2
        # first `half` samples read an item row (user side empty), the others a user row (item side empty); the heaviest rows first
        items = np.r_[np.argsort(-deg[n_u:])[:4], rng.integers(0, n - n_u, 256)][:half]
        users = np.r_[np.argsort(-deg[:n_u])[:4], rng.integers(0, n_u, 256)][:B - half]
        if len(items) > 2:
            items[-1] = items[0]                                            # repeats
        bu = np.r_[np.full(half, empty_u), users].astype(np.int64)
        bi = np.r_[items, np.full(B - half, empty_i)].astype(np.int64)
        g = G(*csr)
        X, run_d = t(E0), t(run)
        div = 4.0
        slots = torch.full((2 * B, d), 7.0, device=DEV)
        per = torch.full((B,), 7.0, device=DEV)
        ops.lightgcn_batch_slots(g, X, run_d, div, t(bu), t(bi), torch.zeros(B, device=DEV), n_u, 2.0, slots, loss_per_sample=per)
        got_rows = np.r_[bi[:half] + n_u, bu[half:]]
        got = torch.cat([slots[:half], slots[B + half:2 * B]]).cpu().numpy()
        full_acc = torch.empty_like(X)
        g.spmm(X, Y=torch.empty_like(X), acc_in=run_d, acc_out=full_acc, acc_div=div)
        want = full_acc.cpu().numpy()[got_rows]
        short = deg[got_rows] <= 1024
        assert np.array_equal(got[short], want[short]), (name, d, B)
        lo = torch.zeros_like(X)
        g.spmm_rows(X, t(bu), t(bi), 0, n_u, acc_in=run_d, acc_out=lo, acc_div=div)
        assert np.array_equal(lo.cpu().numpy()[got_rows][short], want[short]), (name, d, B)
        if (~short).any():
            truth = (run + oracle.spmm(*csr, E0)) / np.float32(div)
            for r, row in zip(got_rows[~short], got[~short]):
                e = rel_err(row, truth[r])
                print(f"hub row {r} ({deg[r]} entries) d={d} B={B}: rel err vs oracle {e:.2e}")
                assert e <= 3e-6
            assert rel_err(lo.cpu().numpy()[got_rows][~short], truth[got_rows[~short]]) <= 3e-6
        assert name != "hubs" or B < 3 or (~short).any()
        assert np.abs(per.cpu().numpy() - np.log(2.0)).max() <= 2e-6


# ------------------------------------------------------------------------------------------ 2. one launch = three launches
def _three_launches(ops, g, X, run, L, u_d, i_d, y_d, n_u):
    n, d, B = X.shape[0], X.shape[1], u_d.numel()
    lo = run.clone()
    g.spmm_rows(X, u_d, i_d, 0, n_u, acc_in=run, acc_out=lo, acc_div=float(L + 1))
    slots, loss = torch.zeros(2 * B, d, device=DEV), torch.zeros(1, device=DEV)
    g_out, G_ = torch.zeros(n, d, device=DEV), torch.zeros(n, d, device=DEV)
    ops.score_bce(lo[:n_u], lo[n_u:], u_d, i_d, y_d, loss_sum=loss, grad_users=g_out[:n_u], grad_items=g_out[n_u:], grad_scale=1.0 / B,
                  grad_slots=slots)
    ops.spmm_push_batch(g, u_d, i_d, n_u, slots, G_, add=slots, scale=1.0 / (L + 1))
    return loss, g_out, G_, slots


@pytest.mark.parametrize("d", WIDE)
def test_batch_kernel_equals_the_three_launch_sequence(G, oracle, epinion2, d):
    """spex_lightgcn_batch_f32 / spex_lightgcn_batch_slots_f32 at d = 128 / 256 against spmm_rows -> score_bce (slots) ->
    spmm_push_batch at the same width, L = 1 .. 4 on Epinion2 (B = 256, the heaviest rows, repeats) and B = 1 / 3 / 17 on the graph with
    hub, empty and boundary rows; the three-launch push target against the oracle's pull-form product.  Tolerances:
    test_lightgcn_batch_kernel_equals_the_three_launch_sequence (loss 1e-5, g_out / G 2e-6, G vs the oracle 1e-5) and
    test_batch_kernels_small_batches_and_degenerate_rows / ..hub_rows_and_a_non_symmetric_matrix (3e-6), test_gpu_kernels.py."""
    from spex_amd import ops
    csr, E0 = epi(epinion2, d)
    g = G(*csr)
    n, n_u, B = len(E0), N_U, 256
    rng = np.random.default_rng(12)
    X, run = t(E0), t((rng.normal(size=E0.shape) * 0.05).astype(np.float32))
    deg = np.diff(csr[0])
    users, items = rng.integers(0, N_U - 1, B), rng.integers(0, N_I, B)
    users[:4] = np.argsort(-deg[:n_u])[:4]
    items[:4] = np.argsort(-deg[n_u:])[:4]
    users[10:14] = users[0]
    items[20:30] = items[1]
    labels = (rng.random(B) < 1 / 6).astype(np.float32)
    u_d, i_d, y_d = t(users), t(items), t(labels)
    for L in (1, 2, 3, 4):
        loss_a, g_out_a, G_a, slots_a = _three_launches(ops, g, X, run, L, u_d, i_d, y_d, n_u)
        loss_b, g_out_b, G_b = torch.zeros(1, device=DEV), torch.zeros(n, d, device=DEV), torch.zeros(n, d, device=DEV)
        ops.lightgcn_batch(g, X, run, float(L + 1), u_d, i_d, y_d, n_u, 1.0 / B, 1.0 / (L + 1), loss_b, g_out_b, G_b)
        slots_b, loss_c = torch.full((2 * B, d), 7.0, device=DEV), torch.zeros(1, device=DEV)
        ops.lightgcn_batch_slots(g, X, run, float(L + 1), u_d, i_d, y_d, n_u, 1.0 / B, slots_b, loss_sum=loss_c)
        figs = (abs(loss_a.item() - loss_b.item()) / abs(loss_a.item()), rel_err(g_out_b.cpu().numpy(), g_out_a.cpu().numpy()),
                rel_err(G_b.cpu().numpy(), G_a.cpu().numpy()), rel_err(slots_b.cpu().numpy(), slots_a.cpu().numpy()))
        print(f"d={d} L={L}: loss {figs[0]:.2e} g_out {figs[1]:.2e} G {figs[2]:.2e} slots {figs[3]:.2e}")
        assert figs[0] <= 1e-5 and abs(loss_a.item() - loss_c.item()) <= 1e-5 * abs(loss_a.item())
        assert figs[1] <= 2e-6 and figs[2] <= 2e-6 and figs[3] <= 2e-6
        if L == 3:      # the push target of both forms against the oracle's pull form (A is symmetric here)
            gd = g_out_a.cpu().numpy()
            want_G = (gd.astype(np.float64) + oracle.spmm(*csr, gd).astype(np.float64)) / (L + 1)
            assert rel_err(G_a.cpu().numpy(), want_G) <= 1e-5 and rel_err(G_b.cpu().numpy(), want_G) <= 1e-5
    # small batches on hub / empty / one-entry / boundary rows of a non-symmetric matrix
    csr, n_u = hub_graph()
    n, L = len(csr[0]) - 1, 3
    t_csr = oracle.csr_transpose(*csr, n)
    g = G(*csr)
    X = t((rng.normal(size=(n, d)) * 0.3).astype(np.float32))
    run = t((rng.normal(size=(n, d)) * 0.3).astype(np.float32))
    for B in (1, 3, 17):
        users = np.array(([2, 7, 2, 8, 9, 10] + list(rng.integers(0, n_u, 32)))[:B])
        items = np.array(([1500 - n_u, 2999 - n_u, 1201 - n_u, 1200 - n_u, 1202 - n_u, 1203 - n_u] + list(rng.integers(0, n - n_u, 32)))[:B])
        labels = (rng.random(B) < 0.4).astype(np.float32)
        u_d, i_d, y_d = t(users), t(items), t(labels)
        loss_a, g_out_a, G_a, slots_a = _three_launches(ops, g, X, run, L, u_d, i_d, y_d, n_u)
        loss_b, g_out_b, G_b = torch.zeros(1, device=DEV), torch.zeros(n, d, device=DEV), torch.zeros(n, d, device=DEV)
        ops.lightgcn_batch(g, X, run, float(L + 1), u_d, i_d, y_d, n_u, 1.0 / B, 1.0 / (L + 1), loss_b, g_out_b, G_b)
        figs = (abs(loss_a.item() - loss_b.item()), rel_err(g_out_b.cpu().numpy(), g_out_a.cpu().numpy()),
                rel_err(G_b.cpu().numpy(), G_a.cpu().numpy()))
        print(f"hubs d={d} B={B}: loss {figs[0]:.2e} g_out {figs[1]:.2e} G {figs[2]:.2e}")
        assert figs[0] <= 1e-5 * abs(loss_a.item()) + 1e-7 and figs[1] <= 3e-6 and figs[2] <= 3e-6
        gd = g_out_b.cpu().numpy()
        want_G = (gd.astype(np.float64) + oracle.spmm(*t_csr[:3], gd).astype(np.float64)) / (L + 1)     # A^T g: pull form on the transpose
        assert rel_err(G_b.cpu().numpy(), want_G) <= 1e-5


@pytest.mark.parametrize("d", WIDE)
def test_batch_kernel_under_an_injected_edge_mask_on_a_non_symmetric_matrix(G, oracle, d):
    """The same launch with an injected keep mask on the handle (mode 1), on the non-symmetric graph with hub rows: the forward rows
    are the masked spex_spmm_f32's (bit for bit up to 1 024 entries, read back exactly as in the first test), and loss, dense
    gradient and push target equal masked whole-graph product -> score_bce -> pull-form product on the TRANSPOSED handle carrying
    the edge-id permutation and the same mask (tolerances: 1e-5 loss, 3e-6 g_out, 1e-5 against a pull-form product — test_gpu_kernels.py,
    test_lightgcn_batch_kernel_hub_rows_and_a_non_symmetric_matrix)."""
    from spex_amd import ops
    from spex_amd.graph import csr_transpose
    csr, n_u = hub_graph()
    n, L, B, keep_prob = len(csr[0]) - 1, 2, 17, 0.6
    rng = np.random.default_rng(31 + d)
    keep = t((rng.random(len(csr[1])) < keep_prob).astype(np.uint8))
    g = G(*csr)
    t_rowptr, t_col, t_val, eid = csr_transpose(*csr, n)
    gt = G(t_rowptr, t_col, t_val, edge_id=eid)
    g.set_edge_mask(1, keep, keep_prob, 0)
    gt.set_edge_mask(1, keep, keep_prob, 0)
    X = t((rng.normal(size=(n, d)) * 0.3).astype(np.float32))
    run = t((rng.normal(size=(n, d)) * 0.3).astype(np.float32))
    users = np.array(([2, 7, 2, 8, 9, 10] + list(rng.integers(0, n_u, 32)))[:B])
    items = np.array(([1500 - n_u, 2999 - n_u, 1201 - n_u, 1200 - n_u, 1202 - n_u, 1203 - n_u] + list(rng.integers(0, n - n_u, 32)))[:B])
    labels = (rng.random(B) < 0.4).astype(np.float32)
    u_d, i_d, y_d = t(users), t(items), t(labels)
    lo = torch.empty_like(X)
    g.spmm(X, Y=torch.empty_like(X), acc_in=run, acc_out=lo, acc_div=float(L + 1))
    loss_a, g_out_a = torch.zeros(1, device=DEV), torch.zeros(n, d, device=DEV)
    ops.score_bce(lo[:n_u], lo[n_u:], u_d, i_d, y_d, loss_sum=loss_a, grad_users=g_out_a[:n_u], grad_items=g_out_a[n_u:], grad_scale=1.0 / B)
    G_a = (g_out_a + gt.spmm(g_out_a)) / (L + 1)
    loss_b, g_out_b, G_b = torch.zeros(1, device=DEV), torch.zeros(n, d, device=DEV), torch.zeros(n, d, device=DEV)
    ops.lightgcn_batch(g, X, run, float(L + 1), u_d, i_d, y_d, n_u, 1.0 / B, 1.0 / (L + 1), loss_b, g_out_b, G_b)
    figs = (abs(loss_a.item() - loss_b.item()) / abs(loss_a.item()), rel_err(g_out_b.cpu().numpy(), g_out_a.cpu().numpy()),
            rel_err(G_b.cpu().numpy(), G_a.cpu().numpy()))
    print(f"masked d={d}: loss {figs[0]:.2e} g_out {figs[1]:.2e} G {figs[2]:.2e}")
    assert figs[0] <= 1e-5 and figs[1] <= 3e-6 and figs[2] <= 1e-5
    # the masked forward rows, exactly: item rows paired with the empty user row 7, user rows with the empty item row 1201
    run0 = run.clone()
    run0[7] = 0.0
    run0[1201] = 0.0
    g.spmm(X, Y=torch.empty_like(X), acc_in=run0, acc_out=lo, acc_div=float(L + 1))
    bu = np.array([7, 7, 7, 2, 8, 9, 10], np.int64)
    bi = np.array([1500 - n_u, 1202 - n_u, 1203 - n_u, 1201 - n_u, 1201 - n_u, 1201 - n_u, 1201 - n_u], np.int64)
    slots = torch.zeros(14, d, device=DEV)
    ops.lightgcn_batch_slots(g, X, run0, float(L + 1), t(bu), t(bi), torch.zeros(7, device=DEV), n_u, 2.0, slots, loss_per_sample=torch.zeros(7, device=DEV))
    rows = np.r_[bi[:3] + n_u, bu[3:]]
    got, want = torch.cat([slots[:3], slots[7 + 3:]]).cpu().numpy(), lo.cpu().numpy()[rows]
    short = np.diff(csr[0])[rows] <= 1024
    assert short.sum() == 5 and np.array_equal(got[short], want[short])
    keep_np = keep.cpu().numpy()
    truth = (run0.cpu().numpy() + oracle.spmm_masked(*csr, keep_np, keep_prob, X.cpu().numpy())) / np.float32(L + 1)
    assert rel_err(got[~short], truth[rows[~short]]) <= 3e-6
    g.set_edge_mask(0)
    gt.set_edge_mask(0)


# ------------------------------------------------------------------------------------------ 3. reduce_slots
@pytest.mark.parametrize("d", WIDE)
def test_reduce_slots_wide_adds_in_ascending_slot_order(d):
    """spex_reduce_slots_f32 at d = 128 / 256 against sequential fp32 adds in slot order (np.add.at; index_add_ on the CPU walks the
    same order): bit-identical — heavy repetition, an out-of-range slot, the accumulate form, the clear form, a strided slot array."""
    from spex_amd import ops
    rng = np.random.default_rng(3 + d)
    n_rows, n_u = 5000, 2000
    ua, ub = rng.integers(0, n_u, 300), rng.integers(0, n_rows - n_u, 300)
    ua[:200] = np.where(rng.random(200) < 0.7, 17, ua[:200])
    ub[5:40] = 123
    ub[77] = 999999                                                    # out of range: skipped
    slots = (rng.normal(size=(600, d)) * np.exp(rng.normal(size=(600, 1)) * 3)).astype(np.float32)
    rows = np.concatenate([ua, ub + n_u])
    ok = (rows >= 0) & (rows < n_rows)
    want = np.zeros((n_rows, d), np.float32)
    np.add.at(want, rows[ok], slots[ok])
    ref = torch.zeros(n_rows, d).index_add_(0, torch.from_numpy(rows[ok]), torch.from_numpy(slots[ok])).numpy()
    assert np.array_equal(ref, want)
    out = torch.full((n_rows, d), 7.0, device=DEV)
    ops.reduce_slots(t(ua), t(ub), n_u, n_rows, t(slots), out)
    got = out.cpu().numpy()
    touched = np.zeros(n_rows, bool); touched[rows[ok]] = True
    assert np.array_equal(got[touched], want[touched])
    assert (got[~touched] == 7.0).all()
    base = rng.normal(size=(n_rows, d)).astype(np.float32)
    out2 = t(base.copy())
    ops.reduce_slots(t(ua), t(ub), n_u, n_rows, t(slots), out2, scale=0.25, accumulate=True)
    want2 = base.copy()
    want2[touched] = base[touched] + want[touched] * np.float32(0.25)
    assert np.array_equal(out2.cpu().numpy(), want2)
    ops.reduce_slots(t(ua), t(ub), n_u, n_rows, None, out)             # clear form
    got = out.cpu().numpy()
    assert (got[touched] == 0.0).all() and (got[~touched] == 7.0).all()
    strided = np.zeros((600, d + 64), np.float32); strided[:, :d] = slots
    out3 = torch.zeros(n_rows, d, device=DEV)
    ops.reduce_slots(t(ua), t(ub), n_u, n_rows, t(strided), out3)
    assert np.array_equal(out3.cpu().numpy()[touched], want[touched])


# ------------------------------------------------------------------------------------------ 4. the one-call step vs the oracle
def _stepper(G, epinion2, d, L=3, deterministic=False, transposed=False):
    from spex_amd.graph import csr_transpose
    from spex_amd.trainer import LightGCNStepper
    csr, E0 = epi(epinion2, d)
    gt = None
    if transposed:
        t_rowptr, t_col, t_val, eid = csr_transpose(*csr, len(E0))
        gt = G(t_rowptr, t_col, t_val, edge_id=eid)
    return LightGCNStepper(G(*csr), t(E0.copy()), N_U, n_layers=L, lr=1e-3, graph_t=gt, deterministic=deterministic)


@pytest.mark.parametrize("d", WIDE)
def test_one_call_step_against_the_oracle(G, oracle, epinion2, d):
    """Five consecutive one-call steps (step_bce(.., loss_acc=.., batch_rows_only=True)) on Epinion2, L = 3, B = 256 with repeated
    users, against oracle.lightgcn_loss_and_grad + oracle.adam_step: per-step mean loss within 2e-6 and E0 within 5e-6 relative
    (test_g3_g4_training_steps_vs_reference), m within 1e-5 (that test's gradient tolerance: m is linear in the gradients) and v within
    2e-5 (quadratic).  A batch of 17 with L = 1, 2 and 4 covers the other step forms for one step each."""
    csr, E0 = epi(epinion2, d)
    t_csr = oracle.csr_transpose(*csr, len(E0))
    st = _stepper(G, epinion2, d)
    assert st._one_call_ok(*(t(a) for a in training_batches(epinion2, 1)[0]))
    W, m, v = E0.copy(), np.zeros_like(E0), np.zeros_like(E0)
    acc = torch.zeros(1, device=DEV)
    for s, (u, i, y) in enumerate(training_batches(epinion2, 5, seed=41)):
        acc.zero_()
        st.step_bce(t(u), t(i), t(y), loss_acc=acc, batch_rows_only=True)
        _, loss_o, Gd = oracle.lightgcn_loss_and_grad(*csr, W, N_U, 3, u, i, y, t_csr=t_csr)
        oracle.adam_step(W, Gd, m, v, s + 1)
        figs = (abs(acc.item() / 256 - float(loss_o)), rel_err(st.E0.cpu().numpy(), W), rel_err(st.m.cpu().numpy(), m), rel_err(st.v.cpu().numpy(), v))
        print(f"d={d} step {s + 1}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
        assert figs[0] <= 2e-6 and figs[1] <= 5e-6 and figs[2] <= 1e-5 and figs[3] <= 2e-5
    assert st.t == 5
    for L in (1, 2, 4):
        st = _stepper(G, epinion2, d, L=L)
        u, i, y = training_batches(epinion2, 1, B=17, seed=L)[0]
        acc.zero_()
        st.step_bce(t(u), t(i), t(y), loss_acc=acc, batch_rows_only=True)
        _, loss_o, Gd = oracle.lightgcn_loss_and_grad(*csr, E0, N_U, L, u, i, y, t_csr=t_csr)
        W, m, v = E0.copy(), np.zeros_like(E0), np.zeros_like(E0)
        oracle.adam_step(W, Gd, m, v, 1)
        assert abs(acc.item() / 17 - float(loss_o)) <= 2e-6 and rel_err(st.E0.cpu().numpy(), W) <= 5e-6, L
        assert rel_err(st.m.cpu().numpy(), m) <= 1e-5 and rel_err(st.v.cpu().numpy(), v) <= 2e-5, L


# ------------------------------------------------------------------------------------------ 5. one call vs launch by launch
@pytest.mark.parametrize("d", WIDE)
@pytest.mark.parametrize("deterministic", [False, True])
def test_one_call_step_equals_the_launch_by_launch_step(G, epinion2, d, deterministic):
    """20 steps from the same state through the one-call step and through the launch-by-launch step (batch_rows_only=False), fast and
    deterministic mode, B = 256 and a batch of 3 and of 1 at the end: loss sums within 2e-5, E0 within 2e-5 relative (the d == 64
    bounds of test_one_call_step_under_edge_dropout_equals_the_launch_by_launch_step, test_gpu_dropin.py), m within the same 2e-5, v
    within twice that.  Deterministic mode: two one-call runs end in BIT-IDENTICAL E0 / m / v (test_gpu_deterministic.py)."""
    batches = training_batches(epinion2, 18, seed=7) + training_batches(epinion2, 1, B=3, seed=8) + training_batches(epinion2, 1, B=1, seed=9)
    runs = []
    for one_call in (True, True, False):
        st = _stepper(G, epinion2, d, deterministic=deterministic)
        acc = torch.zeros(1, device=DEV)
        for u, i, y in batches:
            st.step_bce(t(u), t(i), t(y), loss_acc=acc, batch_rows_only=one_call)
        assert st.t == 20
        runs.append((st.E0.cpu().numpy(), st.m.cpu().numpy(), st.v.cpu().numpy(), acc.item()))
    a, a2, b = runs
    if deterministic:
        for x, y in zip(a[:3], a2[:3]):
            assert np.array_equal(x, y)
        assert a[3] == a2[3]
    figs = (abs(a[3] - b[3]) / abs(b[3]), rel_err(a[0], b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2]))
    print(f"d={d} det={deterministic}: loss {figs[0]:.2e} E0 {figs[1]:.2e} m {figs[2]:.2e} v {figs[3]:.2e}")
    assert figs[0] <= 2e-5 and figs[1] <= 2e-5 and figs[2] <= 2e-5 and figs[3] <= 4e-5


def test_deterministic_stepper_refuses_a_width_without_a_fixed_order_form(G, epinion2):
    from spex_amd.trainer import LightGCNStepper
    csr, _ = epi(epinion2, 128)
    E0 = torch.zeros(len(csr[0]) - 1, 96, device=DEV)
    with pytest.raises(ValueError, match="64, 128 or 256"):
        LightGCNStepper(G(*csr), E0, N_U, deterministic=True)
    LightGCNStepper(G(*csr), E0, N_U, deterministic=False)


# ------------------------------------------------------------------------------------------ 6. edge dropout
@pytest.mark.parametrize("d", WIDE)
@pytest.mark.parametrize("mode", ["philox", "injected"])
def test_one_call_step_under_edge_dropout_equals_the_launch_by_launch_step(G, epinion2, d, mode):
    """Six steps with a fresh edge-dropout mask per step on both handles — the in-kernel sampled mask (set_edge_dropout with the
    "philox" stream) and an injected keep mask — through the one-call step and the launch-by-launch step: per-step losses and the
    table within 2e-5 (test_one_call_step_under_edge_dropout_equals_the_launch_by_launch_step at d == 64, test_gpu_dropin.py)."""
    from spex_amd.trainer import edge_dropout_mask
    batches = training_batches(epinion2, 6, seed=13)
    rng = np.random.default_rng(17)
    csr, E0 = epi(epinion2, d)
    masks = [t((rng.random(len(csr[1])) < 0.3).astype(np.uint8)) for _ in batches]
    out = []
    for one_call in (True, False):
        st = _stepper(G, epinion2, d, transposed=True)
        acc = torch.zeros(1, device=DEV)
        per_step = []
        for k, (u, i, y) in enumerate(batches):
            st.set_edge_dropout(edge_dropout_mask(st.graph, 0.3, "philox", 5, k + 1) if mode == "philox" else (1, masks[k], 0.3, 0))
            before = acc.item()
            st.step_bce(t(u), t(i), t(y), loss_acc=acc, batch_rows_only=one_call)
            per_step.append(acc.item() - before)
        st.set_edge_dropout(None)
        out.append((np.asarray(per_step), st.E0.cpu().numpy()))
    (l_a, E_a), (l_b, E_b) = out
    print(f"d={d} {mode}: loss {np.abs(l_a - l_b).max() / np.abs(l_b).max():.2e} E0 {rel_err(E_a, E_b):.2e}")
    assert np.abs(l_a - l_b).max() <= 2e-5 * np.abs(l_b).max()
    assert rel_err(E_a, E_b) <= 2e-5
    assert np.abs(E_a - E0).max() > 1e-4                                      # (the steps did move the table)


# ------------------------------------------------------------------------------------------ 7. the native epoch
class _Epoch:
    """The slice of a LightTrainData that train_epoch reads."""

    def __init__(self, batches):
        self.users_fill = np.concatenate([b[0] for b in batches])
        self.items_fill = np.concatenate([b[1] for b in batches])
        self.labels_fill_np = np.concatenate([b[2] for b in batches])

    def ng_sample(self):
        pass

    def __len__(self):
        return len(self.users_fill)


@pytest.mark.parametrize("d", WIDE)
@pytest.mark.parametrize("deterministic", [False, True])
def test_native_epoch_at_wide_widths(G, epinion2, d, deterministic):
    """train_epoch(stepper, data, max_steps=40) at d = 128 / 256 takes the native branch (epoch_bce is called: ONE library call for
    the epoch) and equals 40 step_bce calls over the same arrays — loss sum within 2e-6, table within 2e-5
    (test_native_epoch_loop_equals_the_python_loop, test_gpu_dropin.py), bit for bit in the deterministic mode; so does an epoch of
    three full batches and a ragged one of 77."""
    from spex_amd.trainer import train_epoch
    B = 256
    data = _Epoch(training_batches(epinion2, 45, seed=23))
    arrays = (data.users_fill, data.items_fill, data.labels_fill_np)
    for n, max_steps, steps in ((len(data), 40, 40), (3 * B + 77, None, 4)):
        arr = tuple(a[:n] for a in arrays)
        st = _stepper(G, epinion2, d, deterministic=deterministic)
        calls = []
        inner = st.epoch_bce
        st.epoch_bce = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
        total = train_epoch(st, data, max_steps=max_steps, arrays=arr).item()
        assert calls == [1] and st.t == steps
        ref = _stepper(G, epinion2, d, deterministic=deterministic)
        want = 0.0
        for k in range(steps):
            s, e = k * B, min((k + 1) * B, n)
            acc = torch.zeros(1, device=DEV)
            ref.step_bce(t(arr[0][s:e]), t(arr[1][s:e]), t(arr[2][s:e]), loss_acc=acc, batch_rows_only=True)
            want += acc.item() / (e - s)
        figs = (abs(total - want) / abs(want), rel_err(st.E0.cpu().numpy(), ref.E0.cpu().numpy()))
        print(f"d={d} det={deterministic} steps={steps}: loss {figs[0]:.2e} E0 {figs[1]:.2e}")
        assert figs[0] <= 2e-6 and figs[1] <= 2e-5
        assert rel_err(st.m.cpu().numpy(), ref.m.cpu().numpy()) <= 2e-5 and rel_err(st.v.cpu().numpy(), ref.v.cpu().numpy()) <= 4e-5
        if deterministic:
            assert torch.equal(st.E0, ref.E0) and torch.equal(st.m, ref.m) and torch.equal(st.v, ref.v)


# ------------------------------------------------------------------------------------------ 8. the C ABI
def test_step_rejects_other_widths_and_names_the_three(G, epinion2):
    """spex_lightgcn_step_bce_f32 with d = 96 in the descriptor: a negative status before anything is launched, and a message that
    lists 64 / 128 / 256."""
    from spex_amd import _lib
    st = _stepper(G, epinion2, 128)
    u, i, y = (t(a) for a in training_batches(epinion2, 1, B=17)[0])
    desc = st._prepare_desc(17)
    desc.d = 96
    acc = torch.zeros(1, device=DEV)
    E0 = st.E0.clone()
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = _lib.load().spex_lightgcn_step_bce_f32(ctypes.byref(desc), vp(u), vp(i), vp(y), 17, vp(acc), None)
    msg = _lib.load().spex_last_error().decode()
    torch.cuda.synchronize()
    assert rc < 0 and all(w in msg for w in ("64", "128", "256")), (rc, msg)
    assert desc.t == 0 and torch.equal(st.E0, E0) and acc.item() == 0.0
