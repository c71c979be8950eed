"""Frontier steps under edge dropout: the masked frontier list, the masked list-driven SpMM, the masked push over a
list, and the exact LightGCN steps with SPEX_STEP_FRONTIER [| SPEX_STEP_SPARSE_ADAM] on masked handles.

Graphs: `graph_b()` of tests/test_gpu_frontier.py (20 000 rows, 60 236 entries, hub user 0 of 1 500 entries) with a transposed handle
that carries the edge-id permutation, built as tests/test_gpu_stepper_sequences.py::handles builds its own; that module's hub graph
(c) (3 000 rows, not symmetric, rows of 0, 1, 64, 65, 1 100, 1 500, 2 600 entries); `heavy_graph()` of test_gpu_frontier.py.

Masks.  Mode 1: `default_rng(101).random(nnz) < p`, p = 0.3 and 0.6, indexed by edge id (= the entry index of `graph`); on (c)
seqmod.keep_mask (0.6).  Mode 2: the header's law restated in NumPy — u01 = float32(philox4x32-10(counter (edge id, 0, 0, 0), key =
the seed's two words)[0] >> 8) * 2^-24, kept iff u01 + keep_prob >= 1 in fp32 — with the Philox of tests/test_host_bpr_device_sampler.py.
What holds on these inputs (computed on the CPU, asserted below): at 0.3 the 256-sample batch's |F1| is 1 418 of 3 409 unmasked, |F2|
2 128 of 8 725; 86 columns are reached over both a dropped and a kept entry; 176 of its 506 rows have every entry dropped; the hub
keeps 454 of its 1 500 entries.

Bounds.  List SpMM: bit for bit.  Push: the 2e-6 (relative to the result's maximum) of the project's unmasked push tests
(test_gpu_kernels.py::test_unique_rows_and_push_form_spmm_vs_oracle, test_gpu_large_graph.py) against an fp64 scatter.  Whole steps:
seqmod.restate in fp64 with the same masks under seqmod.bounds_of, unchanged, as tests/test_gpu_frontier.py does.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_frontier as fmod
import test_gpu_stepper_sequences as seqmod
from test_gpu_frontier import DEV, NB, NB_I, NB_U, batch_b, graph_b, heavy_graph, listed, t
from test_host_bpr_device_sampler import philox4x32_10

pytestmark = pytest.mark.gpu

KP = seqmod.KEEP_PROB                    # 0.6: what seqmod.restate divides a kept value by
_cache = {}


# ------------------------------------------------------------------------------------------ masks, sets, handles
def keep_b(p):
    """The seeded injected mask on graph (b)."""
    return (np.random.default_rng(101).random(len(graph_b()[1])) < p).astype(np.uint8)


def philox_keep(nnz, keep_prob, seed):
    """Mode 2 restated from the header's law: one bit per edge id."""
    w = philox4x32_10(np.arange(nnz, dtype=np.uint64), 0, 0, 0, seed & 0xFFFFFFFF, seed >> 32)[0]
    u01 = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return ((u01 + np.float32(keep_prob)) >= np.float32(1.0)).astype(np.uint8)


def hop(csr, rows, keep):
    """rows U the columns of the kept entries of rows (keep None: of every stored entry), sorted."""
    rowptr, col = csr[0], csr[1]
    parts = [np.asarray(rows, np.int64)]
    for r in rows:
        c = col[rowptr[r]:rowptr[r + 1]]
        parts.append(c if keep is None else c[keep[rowptr[r]:rowptr[r + 1]] != 0])
    return np.unique(np.concatenate(parts))


def masked_sets(csr, rows, keep):
    n = len(csr[0]) - 1
    bset = np.unique(rows[(rows >= 0) & (rows < n)])
    f1 = hop(csr, bset, keep)
    return bset, f1, hop(csr, f1, keep)


def handles_of(csr):
    from spex_amd.graph import SpexGraph, csr_transpose
    n = len(csr[0]) - 1
    t_rowptr, t_col, t_val, eid = csr_transpose(*csr[:3], n)
    return SpexGraph(*csr[:3]), SpexGraph(t_rowptr, t_col, t_val, edge_id=eid)


def premasked(csr, keep, keep_prob):
    """An UNMASKED handle over the same pattern whose values are the masked ones, formed in fp32 as the kernels form them (kept:
    val / keep_prob, dropped: 0).  fmaf(0, x, acc) == fmaf(0, 0, acc) for finite x: its row-list kernels give the masked row-list
    arithmetic, bit for bit, hubs included."""
    from spex_amd.graph import SpexGraph
    val = np.where(keep != 0, csr[2] / np.float32(keep_prob), np.float32(0.0)).astype(np.float32)
    return SpexGraph(csr[0], csr[1], val)


def device():
    return torch.device(DEV, torch.cuda.current_device())


# ------------------------------------------------------------------------------------------ 1. the masked list
def test_the_inputs_have_the_properties_the_cases_rely_on():
    csr = graph_b()[:3]
    keep = keep_b(0.3)
    u, i, _ = batch_b("bce", 2, 256)[1]
    rows = np.concatenate([u, i + NB_U])
    bset, f1, f2 = masked_sets(csr, rows, None)
    bm, f1m, f2m = masked_sets(csr, rows, keep)
    assert (len(bset), len(f1), len(f1m), len(f2), len(f2m)) == (506, 3409, 1418, 8725, 2128)
    rowptr, col = csr[0], csr[1]
    e = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in bset])
    assert len(np.intersect1d(col[e][keep[e] != 0], col[e][keep[e] == 0])) == 86          # reached over a dropped AND a kept entry
    assert sum(1 for r in bset if rowptr[r + 1] > rowptr[r] and not keep[rowptr[r]:rowptr[r + 1]].any()) == 176
    assert 0 in f1m and rowptr[1] - rowptr[0] == 1500 and int(keep[rowptr[0]:rowptr[1]].sum()) == 454


@pytest.mark.parametrize("mask", ["mode 1, 0.3", "mode 1, 0.6", "mode 2"])
def test_masked_frontier_list_is_the_numpy_set(mask):
    from spex_amd import ops
    csr = graph_b()[:3]
    nnz = len(csr[1])
    if mask == "mode 2":
        seed = (77 << 32) | 5
        keep, args = philox_keep(nnz, 0.3, seed), (2, None, 0.3, seed)
    else:
        p = float(mask[-3:])
        keep = keep_b(p)
        args = (1, t(keep), p, 0)
    assert 0.2 * nnz < keep.sum() < 0.7 * nnz
    g = fmod.handle(csr)
    fr, plain = ops.FrontierRows(NB, device()), ops.FrontierRows(NB, device())
    batches = [batch_b(kind, s, n)[1] for kind, s, n in (("bce", 1, 7), ("bce", 2, 256), ("bpr", 3, 256))]
    for rnd in range(2):                                         # the second round: new epochs on the same stamp table
        for k, arrs in enumerate(batches):
            a = arrs[0]
            b = arrs[1] if arrs[2].dtype != np.int64 else np.concatenate([arrs[1], arrs[2]])
            rows = np.concatenate([a, b + NB_U])
            # mode 0 on the handle: the new entry writes what the old one writes (as sets and counts; the order is the atomics')
            g.set_edge_mask(0)
            plain.update(t(a), t(b), 0, NB_U).expand(g).expand2(g)
            bset, f1, f2 = masked_sets(csr, rows, None)
            lst = plain.list.cpu().numpy()
            assert (plain.count.item(), plain.count_f.item(), plain.count_f2.item()) == (len(bset), len(f1), len(f2))
            via_new = ops.FrontierRows(NB, device()).update(t(a), t(b), 0, NB_U)
            for cell_in, cap, cell_out in ((via_new.count, via_new.max_b, via_new.count_f), (via_new.count_f, NB, via_new.count_f2)):
                ops._launch(via_new.list.device, "spex_frontier_rows_masked_i32", g._h, ops._ptr(via_new.list), ops._ptr(cell_in), cap,
                            ops._ptr(via_new.stamp), via_new.epoch, ops._ptr(cell_out))
            assert torch.equal(via_new.counts[:3], plain.counts[:3])
            assert np.array_equal(np.sort(via_new.list.cpu().numpy()[:len(f2)]), np.sort(lst[:len(f2)]))
            # the masked handle
            g.set_edge_mask(*args)
            fr.update(t(a), t(b), 0, NB_U).expand(g).expand2(g)
            bm, f1m, f2m = masked_sets(csr, rows, keep)
            lst = fr.list.cpu().numpy()
            cb, cf, cf2 = fr.count.item(), fr.count_f.item(), fr.count_f2.item()
            assert (cb, cf, cf2) == (len(bm), len(f1m), len(f2m)), (mask, rnd, k)
            assert np.array_equal(np.sort(lst[:cb]), bm) and np.array_equal(np.sort(lst[:cf]), f1m) and np.array_equal(np.sort(lst[:cf2]), f2m)
            assert len(f1m) < len(f1) and len(f2m) < len(f2)
            # spex_frontier_rows_i32 itself lists every stored column whatever the mask
            old = ops.FrontierRows(NB, device()).update(t(a), t(b), 0, NB_U)
            ops._launch(old.list.device, "spex_frontier_rows_i32", g._h, ops._ptr(old.list), ops._ptr(old.count), old.max_b, ops._ptr(old.stamp),
                        old.epoch, ops._ptr(old.count_f))
            assert old.count_f.item() == len(f1)
    g.set_edge_mask(0)


def test_masked_frontier_list_on_the_hub_graph():
    from spex_amd import ops
    csr = seqmod.hub_graph()
    g = fmod.handle(csr)
    fr = ops.FrontierRows(seqmod.N, device())
    for k in range(4):
        keep = seqmod.keep_mask(40 + k)
        g.set_edge_mask(1, t(keep), KP, 0)
        _, (a, b, _) = seqmod.bce_batch(30 + k, 17)
        fr.update(t(a), t(b), 0, seqmod.N_U).expand(g).expand2(g)
        bm, f1m, f2m = masked_sets(csr, np.concatenate([a, b + seqmod.N_U]), keep)
        lst = fr.list.cpu().numpy()
        assert (fr.count.item(), fr.count_f.item(), fr.count_f2.item()) == (len(bm), len(f1m), len(f2m))
        assert np.array_equal(np.sort(lst[:len(f1m)]), f1m) and np.array_equal(np.sort(lst[:len(f2m)]), f2m)
        assert 2 in bm and len(f1m) < len(hop(csr, bm, None))


# ------------------------------------------------------------------------------------------ 2. the masked list SpMM
def rows_with_degrees(deg, wanted, keep, rowptr):
    rows = []
    for d in wanted:
        hit = np.flatnonzero(deg == d)
        assert len(hit), f"no row of {d} entries"
        rows.append(int(hit[0]))
    return rows


@pytest.mark.parametrize("which,mode", [("b", 1), ("b", 2), ("hub", 1)])
def test_masked_rowlist_dev_equals_the_masked_whole_graph_launch(which, mode):
    csr = graph_b()[:3] if which == "b" else seqmod.hub_graph()
    n = len(csr[0]) - 1
    rowptr, col = csr[0], csr[1]
    deg = np.diff(rowptr)
    if mode == 2:
        seed = (9 << 32) | 3
        keep, kp = philox_keep(len(col), 0.3, seed), 0.3
        args = (2, None, kp, seed)
    else:
        kp = 0.3 if which == "b" else KP
        keep = keep_b(kp) if which == "b" else seqmod.keep_mask(21)
        args = (1, t(keep), kp, 0)
    g = fmod.handle(csr)
    g.set_edge_mask(*args)
    rng = np.random.default_rng(5)
    X = t((0.1 * rng.normal(size=(n, 64))).astype(np.float32))
    acc = t((0.3 * rng.normal(size=(n, 64))).astype(np.float32))
    want_y, want_acc = torch.empty_like(X), torch.empty_like(X)
    g.spmm(X, Y=want_y, acc_in=acc, acc_out=want_acc, acc_div=3.0)
    wanted = (0, 1, 65, 100, 128, 129, 200, 1500) if which == "b" else (0, 1, 64, 65, 1100, 1500, 2600)
    special = rows_with_degrees(deg, wanted, keep, rowptr)
    all_dropped = [r for r in range(n) if deg[r] > 1 and not keep[rowptr[r]:rowptr[r + 1]].any()][:3]
    assert all_dropped
    rows = np.unique(np.concatenate([special, all_dropped, rng.choice(n, 1500, replace=False)]))
    rows = rng.permutation(rows)
    SENT = 12345.0
    Y, A = torch.full_like(X, SENT), torch.full_like(X, SENT)
    g.spmm_rows_dev(X, listed(n, rows), Y=Y, acc_in=acc, acc_out=A, acc_div=3.0)
    short = t(rows[deg[rows] <= 1024].astype(np.int64))
    assert torch.equal(Y[short], want_y[short]) and torch.equal(A[short], want_acc[short])
    assert not Y[t(np.array(all_dropped, np.int64))].any()                     # every entry dropped: written, as 0
    # every listed row, the rows beyond 1 024 entries included: the row-list arithmetic on the masked values
    ref = premasked(csr, keep, kp)
    idx = t(rows.astype(np.int64))
    ref_y, ref_acc = torch.zeros_like(X), torch.zeros_like(X)
    ref.spmm_rows(X, idx, Y=ref_y, acc_in=acc, acc_out=ref_acc, acc_div=3.0)
    assert (deg[rows] > 1024).any() and torch.equal(Y[idx], ref_y[idx]) and torch.equal(A[idx], ref_acc[idx])
    rest = torch.ones(n, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert (Y[rest] == SENT).all() and (A[rest] == SENT).all()
    # the running sum in place
    acc2 = acc.clone()
    g.spmm_rows_dev(X, listed(n, rows), acc_in=acc2, acc_out=acc2, acc_div=3.0)
    assert torch.equal(acc2[idx], ref_acc[idx]) and torch.equal(acc2[rest], acc[rest])
    # list lengths around one pass of 16 slots
    for k in (1, 15, 16, 17):
        Yk = torch.full_like(X, SENT)
        head = np.array(special + [r for r in rows if r not in special])[:k]
        g.spmm_rows_dev(X, listed(n, head), Y=Yk)
        hk = t(head.astype(np.int64))
        assert torch.equal(Yk[hk], ref.spmm_rows(X, hk, Y=torch.zeros_like(X))[hk]) and (Yk == SENT).sum().item() == (n - k) * 64
    # a source row that the listed rows name over dropped entries only may hold Inf: the dropped entry's gathered value is replaced
    # (a short list of short rows, so that such source rows exist on the hub graph too)
    few = np.array([r for r in rows if 0 < deg[r] <= 200][:48])
    e = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in few])
    only_dropped = np.setdiff1d(col[e][keep[e] == 0], col[e][keep[e] != 0])
    last_of_row = col[rowptr[few + 1] - 1]                                       # (the padding lanes re-read a segment's last column)
    assert len(np.intersect1d(only_dropped, last_of_row)), "no dropped last entry among the listed rows"
    Xi = X.clone()
    Xi[t(only_dropped.astype(np.int64))] = float("inf")
    Yf, Yi = torch.full_like(X, SENT), torch.full_like(X, SENT)
    g.spmm_rows_dev(X, listed(n, few), Y=Yf)
    g.spmm_rows_dev(Xi, listed(n, few), Y=Yi)
    fi = t(few.astype(np.int64))
    assert torch.isfinite(Yi[fi]).all() and torch.equal(Yi[fi], Yf[fi]) and torch.equal(Yf[fi], ref_y[fi])
    g.set_edge_mask(0)


def test_masked_rowlist_dev_with_more_long_row_tasks_than_lds_slots():
    csr = heavy_graph()
    n = 4000
    keep = (np.random.default_rng(102).random(len(csr[1])) < 0.3).astype(np.uint8)
    g, ref = fmod.handle(csr), premasked(csr, keep, 0.3)
    g.set_edge_mask(1, t(keep), 0.3, 0)
    deg = np.diff(csr[0])
    X = t((0.1 * np.random.default_rng(22).normal(size=(n, 64))).astype(np.float32))
    acc = t((0.3 * np.random.default_rng(23).normal(size=(n, 64))).astype(np.float32))
    heavy = np.concatenate([np.arange(200, 206), np.arange(100, 116)])
    short = np.random.default_rng(24).permutation(np.setdiff1d(np.arange(n), heavy))[:300]
    rows = np.concatenate([short[:7], heavy[::-1], short[7:]])
    assert max(fmod.groups_of_pass(deg[rows[k:k + 16]]) for k in range(0, len(rows), 16)) >= 3
    idx = t(rows.astype(np.int64))
    want_y, want_acc = torch.zeros_like(X), torch.zeros_like(X)
    ref.spmm_rows(X, idx, Y=want_y, acc_in=acc, acc_out=want_acc, acc_div=4.0)
    full_y = g.spmm(X)
    Y, A = torch.full_like(X, 777.0), torch.full_like(X, 777.0)
    g.spmm_rows_dev(X, listed(n, rows), Y=Y, acc_in=acc, acc_out=A, acc_div=4.0)
    assert torch.equal(Y[idx], want_y[idx]) and torch.equal(A[idx], want_acc[idx])
    upto = t(rows[deg[rows] <= 1024].astype(np.int64))
    assert torch.equal(Y[upto], full_y[upto])


def test_bf16_list_spmm_still_refuses_a_mask():
    from spex_amd import _lib
    csr = graph_b()[:3]
    g = fmod.handle(csr)
    g.set_edge_mask(1, t(keep_b(0.6)), 0.6, 0)
    X16 = torch.zeros(NB, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.SpexError, match="without edge dropout"):
        g.spmm_rows_dev(None, listed(NB, np.arange(5)), X16=X16, Y=torch.zeros(NB, 64, device=DEV))


# ------------------------------------------------------------------------------------------ 3. the masked push
def scatter_fp64(csr, keep, kp, rows, src, src_indexed, scale, add, add_scale):
    rowptr, col, val = csr
    out = np.zeros((len(rowptr) - 1, src.shape[1]))
    for k, r in enumerate(rows):
        e = np.arange(rowptr[r], rowptr[r + 1])
        e = e[keep[e] != 0]
        s = src[r if src_indexed else k].astype(np.float64)
        np.add.at(out, col[e], scale * (val[e].astype(np.float64) / kp)[:, None] * s[None, :])
        out[r] += add_scale * add[r if src_indexed else k].astype(np.float64)
    return out


@pytest.mark.parametrize("mask", ["mode 1, 0.3", "mode 1, 0.6", "mode 2"])
def test_masked_push_over_a_list_vs_fp64_scatter(mask):
    from spex_amd import ops
    csr = graph_b()[:3]
    if mask == "mode 2":
        seed, kp = (3 << 32) | 8, 0.3
        keep, args = philox_keep(len(csr[1]), kp, seed), (2, None, kp, seed)
    else:
        kp = float(mask[-3:])
        keep = keep_b(kp)
        args = (1, t(keep), kp, 0)
    g = fmod.handle(csr)
    g.set_edge_mask(*args)
    u, i, _ = batch_b("bce", 2, 256)[1]
    fr = ops.FrontierRows(NB, device()).update(t(u), t(i), 0, NB_U).expand(g)
    cf = fr.count_f.item()
    rows = fr.list.cpu().numpy()[:cf]
    assert 0 in rows and cf == len(masked_sets(csr, np.concatenate([u, i + NB_U]), keep)[1])
    rng = np.random.default_rng(62)
    src, add = rng.standard_normal((NB, 64), dtype=np.float32), rng.standard_normal((NB, 64), dtype=np.float32)
    for indexed in (True, False):
        for add_scale in (None, 0.25):
            out = torch.zeros(NB, 64, device=DEV)
            ops.spmm_push_rows(g, fr, t(src), out, indexed, add=t(add), add_indexed=indexed, scale=0.5, add_scale=add_scale, frontier=True)
            want = scatter_fp64(csr, keep, kp, rows, src, indexed, 0.5, add, 0.5 if add_scale is None else add_scale)
            got = out.cpu().numpy()
            fig = seqmod.rel_err(got, want)
            print(f"masked push ({mask}, indexed={indexed}, add_scale={add_scale}) over |F1| = {cf}: {fig:.2e}")
            assert fig <= 2e-6
            assert not got[~want.any(1)].any()                  # a dropped entry issues no atomic: untouched rows are exactly zero
    g.set_edge_mask(0)


# ------------------------------------------------------------------------------------------ 4. whole steps
@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


def stepper_hub(G, L, sparse_adam=False):
    from spex_amd.trainer import LightGCNStepper
    g, gt = seqmod.handles(G)
    return LightGCNStepper(g, t(seqmod.table(64)), seqmod.N_U, n_layers=L, lr=seqmod.LR, graph_t=gt, weight_decay=seqmod.WD, frontier=True,
                           sparse_adam=sparse_adam)


def stepper_b(L, sparse_adam=False, weight_decay=seqmod.WD):
    from spex_amd.trainer import LightGCNStepper
    g, gt = handles_of(graph_b()[:3])
    return LightGCNStepper(g, t(fmod.table_b().copy()), NB_U, n_layers=L, lr=seqmod.LR, graph_t=gt, weight_decay=weight_decay, frontier=True,
                           sparse_adam=sparse_adam)


def hub_sequence():
    """BCE (B = 7, 256) and exact BPR (T = 17, 256), another injected mask per step, masks switched off and on."""
    plan = [("bce", 7, True), ("bpr", 17, True), ("bce", 256, False), ("bpr", 256, True), ("bce", 7, True), ("bpr", 17, False), ("bce", 256, True)]
    return [(seqmod.bce_batch if kind == "bce" else seqmod.bpr_batch)(1100 + k, n) + (seqmod.keep_mask(1200 + k) if on else None,)
            for k, (kind, n, on) in enumerate(plan)]


@pytest.mark.parametrize("L", [2, 3])
def test_masked_frontier_steps_against_the_fp64_truth_on_the_hub_graph(G, L):
    seq = hub_sequence()
    truth = seqmod.truth_of(("frontier dropout", L), seq, 64, L)
    for form in ("one call", "launches"):
        st = stepper_hub(G, L)
        seqmod.run(st, seq, [form] * len(seq), truth, f"masked frontier L={L} {form}")
        assert st.t == len(seq)
    # one stepper switched between the whole-graph masked step and the frontier masked step, one call and launch by launch
    st = stepper_hub(G, L)
    want, f32 = truth
    forms = ["one call", "launches", "one call", "one call", "launches", "one call", "one call"]
    for k, (el, form) in enumerate(zip(seq, forms)):
        st.frontier = k % 2 == 0
        loss = seqmod.take(st, el, form)
        tag = f"masked mix L={L} step {k + 1} ({el[0]}, {form}, frontier={st.frontier}, masked={el[2] is not None})"
        seqmod.check_invariants(st, form == "one call", tag)
        seqmod.check(tag, seqmod.state(st, loss, el[0] == "bpr"), want[k], f32[k])


@pytest.mark.parametrize("kind,L,n", [("bce", 2, 256), ("bpr", 3, 256)])
def test_masked_frontier_steps_against_the_fp64_truth_on_graph_b(kind, L, n):
    """On graph (b) the masked F1 is a few percent of the rows: a row outside it that the step needed would be missed here."""
    seq = [batch_b(kind, 1300 + k, n) + (keep_b(KP) if k != 1 else None,) for k in range(3)]
    seq[2] = seq[2][:2] + ((np.random.default_rng(103).random(len(graph_b()[1])) < KP).astype(np.uint8),)
    with fmod.restating_on_graph_b():
        truth = seqmod.truth_of(("frontier dropout b", kind, L, n), seq, 64, L)
    for form in ("one call", "launches"):
        st = stepper_b(L)
        seqmod.run(st, seq, [form] * 3, truth, f"masked frontier (b) {kind} L={L} {form}")


@pytest.mark.parametrize("kind,L", [("bce", 2), ("bpr", 3), ("bce", 3), ("bpr", 2)])
def test_masked_frontier_native_epochs_against_the_fp64_truth(G, kind, L):
    """epoch_bce / epoch_bpr with keep_prob = 0.6 on a frontier stepper: two steps of 17 under the sampled masks of seeds
    (drop_seed << 32) | step, restated in NumPy and handed to the truth."""
    T, drop_seed = 17, 41
    nnz = len(seqmod.hub_graph()[1])
    batch = seqmod.bce_batch if kind == "bce" else seqmod.bpr_batch
    seq = [batch(1400 + k, T) + (philox_keep(nnz, KP, (drop_seed << 32) | (k + 1)),) for k in range(2)]
    want, f32 = seqmod.truth_of(("frontier dropout epoch", kind, L), seq, 64, L)
    st = stepper_hub(G, L)
    full, ragged = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    arrs = [t(np.concatenate([el[1][j] for el in seq])) for j in range(3)]
    (st.epoch_bce if kind == "bce" else st.epoch_bpr)(*arrs, T, full, ragged, keep_prob=KP, drop_seed=drop_seed)
    assert st.t == 2 and ragged.item() == 0.0 and st.graph.mask_mode == 0 and st.graph_t.mask_mode == 0
    tag = f"masked frontier epoch {kind} L={L}"
    seqmod.check_invariants(st, True, tag)
    state = seqmod.state(st, want[1]["loss"], kind == "bpr")      # (the epoch returns the SUM of its steps' losses: checked below)
    seqmod.check(tag, state, want[1], f32[1])
    got, exp = full.item() / T, want[0]["loss"] + want[1]["loss"]
    bound = seqmod.bounds_of(f32[0])["loss"] + seqmod.bounds_of(f32[1])["loss"]
    print(f"{tag}: loss_full / T {got:.7f}, the two steps' mean losses {exp:.7f}: {abs(got - exp):.2e} (bound {bound:.2e})")
    assert abs(got - exp) <= bound


# ------------------------------------------------------------------------------------------ 5. sparse Adam at L = 2 under a mask
@pytest.mark.parametrize("form", ["one call", "launches"])
def test_masked_sparse_adam_moves_the_masked_two_hop_set_only(form):
    """Three BCE / BPR steps at L = 2 with SPEX_STEP_SPARSE_ADAM on graph (b), another mask per step (the second step unmasked).  Rows
    outside the step's masked F2: E0, m, v bit-identical before and after.  Rows inside: the fp64 truth of the SAME law — the
    gradient of seqmod.restate's step from the truth's own table, Adam with the global t at the rows of F2 only — under seqmod's gate
    (the project's bound or 4 x the figure of the same law restated in fp32 on the CPU).
    grad_E0 is zero outside the list afterwards, whatever list the step before left."""
    csr = graph_b()[:3]
    masks = [keep_b(KP), None, (np.random.default_rng(104).random(len(csr[1])) < KP).astype(np.uint8)]
    seq = [batch_b(kind, 1500 + k, n) + (masks[k],) for k, (kind, n) in enumerate((("bce", 256), ("bpr", 256), ("bce", 7)))]
    st = stepper_b(2, sparse_adam=True)
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, seqmod.LR

    def law(dtype, np_dtype):
        """The sequence under the sparse law in `dtype` on the CPU: per step seqmod.restate's single step from the law's own table."""
        W = fmod.table_b().astype(np_dtype)
        m, v = np.zeros_like(W), np.zeros_like(W)
        out = []
        for k, el in enumerate(seq):
            with fmod.restating_on_graph_b():
                saved, seqmod.table = seqmod.table, (lambda d, W=W: W)
                try:
                    one = seqmod.restate([el], 64, 2, seqmod.WD, dtype)[0]
                finally:
                    seqmod.table = saved
            g = one["grad"]
            assert not g[~inside_of[k]].any(), "the restated gradient leaves the masked F2"
            step = k + 1
            m_new, v_new = m + (1 - b1) * (g - m), b2 * v + (1 - b2) * g * g
            W_new = W - (lr / (1 - b1 ** step)) * (m_new / (np.sqrt(v_new) / np.sqrt(1 - b2 ** step) + eps))
            W, m, v = (np.where(inside_of[k][:, None], new, old).astype(np_dtype) for new, old in ((W_new, W), (m_new, m), (v_new, v)))
            out.append({"loss": one["loss"], "E0": W, "m": m, "v": v, "grad": g})
        return out

    inside_of = []
    for kind, arrs, keep in seq:
        rows = np.concatenate([arrs[0], arrs[1] + NB_U] + ([arrs[2] + NB_U] if kind == "bpr" else []))
        inside = np.zeros(NB, bool)
        inside[masked_sets(csr, rows, keep)[2]] = True
        assert 0 < inside.sum() < 0.8 * NB
        inside_of.append(inside)
    want = law(torch.float64, np.float64)
    f32 = [seqmod.figures(a, b) for a, b in zip(law(torch.float32, np.float32), want)]      # the yardstick, as seqmod.truth_of forms it
    for k, el in enumerate(seq):
        before = [x.clone() for x in (st.E0, st.m, st.v)]
        loss = seqmod.take(st, el, form)
        out = t(np.flatnonzero(~inside_of[k]))
        for name, x, x0 in zip(("E0", "m", "v"), (st.E0, st.m, st.v), before):
            assert torch.equal(x[out], x0[out]), f"step {k + 1}: {name} moved outside the masked F2"
        assert not st.grad_E0[out].any(), f"step {k + 1}: grad_E0 is not zero outside the list"
        seqmod.check(f"masked sparse Adam {form} step {k + 1} ({el[0]})", seqmod.state(st, loss, el[0] == "bpr"), want[k], f32[k])
        seqmod.check_invariants(st, form == "one call", f"step {k + 1}")
    assert st.t == 3


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_stepper_untouched(G):
    from spex_amd import _lib
    from spex_amd.graph import _stream
    from spex_amd.trainer import LightGCNStepper
    keep = t(seqmod.keep_mask(7))
    _, (u, i, y) = seqmod.bce_batch(1, 17)
    u, i, y = t(u), t(i), t(y)
    acc = torch.zeros(2, 1, device=DEV)
    phrase = "does not combine with edge dropout"

    def untouched(st, E0):
        return st.t == 0 and torch.equal(st.E0, E0)

    # a frontier stepper without a transposed handle
    g, gt = seqmod.handles(G)
    st = LightGCNStepper(g, t(seqmod.table(64)), seqmod.N_U, n_layers=2, lr=seqmod.LR, frontier=True)
    E0 = st.E0.clone()
    with pytest.raises(ValueError, match=phrase):
        st.set_edge_dropout((1, keep, KP, 0))
    with pytest.raises(ValueError, match=phrase):
        st.epoch_bce(u, i, y, 17, acc[0], acc[1], keep_prob=KP)
    assert untouched(st, E0) and st.graph.mask_mode == 0
    # bf16 gather tables x frontier x mask: switching the mask on, switching bf16 on under a mask, the epochs, the steps
    st = LightGCNStepper(g, t(seqmod.table(64)), seqmod.N_U, n_layers=2, lr=seqmod.LR, graph_t=gt, frontier=True)
    st.gather_dtype = torch.bfloat16
    with pytest.raises(ValueError, match=phrase):
        st.set_edge_dropout((1, keep, KP, 0))
    with pytest.raises(ValueError, match=phrase):
        st.epoch_bpr(u, i, i, 17, acc[0], acc[1], keep_prob=KP)
    assert untouched(st, E0) and st.graph.mask_mode == 0 and st.graph_t.mask_mode == 0
    st.gather_dtype = None
    st.set_edge_dropout((1, keep, KP, 0))
    with pytest.raises(ValueError, match=phrase):
        st.gather_dtype = torch.bfloat16
    assert st.gather_dtype is None and untouched(st, E0)
    # the C step with SPEX_STEP_FRONTIER | SPEX_STEP_BF16_GATHER on masked two-handle steppers: -1, "edge dropout" in the message
    st.set_edge_dropout(None)
    st.gather_dtype = torch.bfloat16
    desc = st._prepare_desc(17, 2)
    st.graph.set_edge_mask(1, keep, KP, 0)
    st.graph_t.set_edge_mask(1, keep, KP, 0)
    lib = _lib.load()
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    assert desc.flags & _lib.STEP_FRONTIER and desc.flags & _lib.STEP_BF16_GATHER
    rc = lib.spex_lightgcn_step_bce_f32(ctypes.byref(desc), vp(u), vp(i), vp(y), 17, vp(acc), _stream(None))
    assert rc == -1 and "edge dropout" in lib.spex_last_error().decode() and desc.t == 0
    torch.cuda.synchronize()
    assert untouched(st, E0) and not acc.any()
    st.graph.set_edge_mask(0)
    st.graph_t.set_edge_mask(0)
