"""The large-graph regime: the list kernels, the dense and row-sparse Adam passes and whole one-call steps past every
bounded grid's first pass, on a handle in the adjacent-row layout (no row ids, no row heads, no packed words, `xcd_contig` off), and
one gather table that crosses 4 GiB.

Graph (e) and its batches `heavy` / `light` are those of tests/test_large_graph_host.py, which proves in NumPy that they cross every
cap: 150 000 rows (a dense pass of 2 048 x 256 float4 makes 4.6 trips), |F1| of `heavy` >= 80 000 > 65 536, |F2| of `light` < 32 768.

Part A compares kernels alone, bit for bit or as sets.  Part B runs three consecutive one-call steps (`heavy`, `light`, `heavy`) per
form on one Adam state, so that the second and third step read what the pass before cleared and updated past its first trip.  The
truth is the fp64 restatement of tests/test_gpu_stepper_sequences.py (`restate`; for row-sparse Adam `restate_sparse` of
tests/test_gpu_sparse_adam.py) with that module's graph swapped for (e); the gate is that module's, unchanged: per quantity the larger
of PROJECT_BOUNDS and 4 x the fp32 CPU restatement's own figure at that step.  The bf16 forms are gated at the bf16 modules' margin —
the kernels' worst figure over the three steps <= 2 x the yardstick's, per quantity — but the yardstick here is no stepper of this
library (the launch-by-launch bf16 stepper shares the striding Adam pass under test): it is `restate_rounded`, an fp32 CPU restatement
with torch's CPU bf16 rounding at the points DESIGN.md 4.19 / 4.24 name and a straight-through backward.  Part C is one test on a
2 048 x (2^24 + 4 096) handle whose fp32 gather table is 4 GiB + 1 MiB: byte offsets beyond 32 bits.  The d = 64 bf16 table would
need 2^25 rows to cross; it is left out.

The kernels on an MI355X, worst step (the yardstick's worst over the same steps in brackets; loss absolute, the rest relative to
the truth's maximum):
    fp32 forms (whole, deterministic, d = 128, frontier L = 2 / 3, sparse Adam, the switched stepper's fp32 steps; brackets: the fp32
    CPU restatement): loss 3.7e-8 (9.7e-8), E0 8.3e-7 (6.5e-6), m 2.7e-6 (3.5e-6), v 1.32e-5 (5.6e-6), grad_E0 2.5e-6 (3.9e-6);
    no figure above 0.66 of its bound (v: the kernels form 1 - beta2 in fp32, which the project's 2e-5 was sized for), the others
    below 0.28.
    bf16 forms at L = 3, B = T = 256 (brackets: restate_rounded):
        BCE whole     loss 3.33e-7 (3.92e-7)  E0 5.598e-3 (5.598e-3)  m 5.615e-3 (5.615e-3)  v 2.864e-3 (2.855e-3)
        BCE frontier  loss 4.52e-7 (5.11e-7)  E0 5.600e-3 (5.600e-3)  m 5.597e-3 (5.597e-3)  v 2.677e-3 (2.689e-3)
        BPR whole     loss 5.41e-7 (5.41e-7)  E0 5.323e-3 (5.323e-3)  m 2.390e-3 (2.390e-3)  v 2.351e-3 (2.345e-3)
        BPR frontier  loss 5.41e-7 (4.81e-7)  E0 5.323e-3 (5.323e-3)  m 2.459e-3 (2.459e-3)  v 1.738e-3 (1.744e-3)
    the switched stepper's bf16 step (L = 2, frontier + bf16 on `light`), BCE / BPR: loss 2.6e-7 / 4.8e-7 (2.6e-7 / 4.2e-7), E0
    4.3e-4 / 6.9e-4 (the same), m 8.7e-4 / 9.0e-4 (the same), v 7.5e-4 / 1.08e-3 (7.5e-4 / 1.07e-3).
    Part A: the dense Adam pass equals oracle.adam_step exactly at t = 1, 2, 100 000 (bound 1e-6); push over |F1| = 81 214: 9.5e-7,
    scaled form 1.02e-6 (bound 2e-6).  Part C: spmm 2.0e-7, spmm_rowlist_dev 2.4e-7, push 1.8e-7 (bound 2e-6).
The kernels reproduce restate_rounded to three or four digits: the roundings sit where DESIGN.md says.  The fp64 truth of a sequence
and its fp32 restatement cost 3 - 4 s together on the GPU host (computed once per (kind, batch size, L), shared by the forms); the
module runs in 74 s, its slowest case (d = 128, whose truth is twice the size) in 8 - 10 s.  More: DESIGN.md 4.25.
"""
import contextlib

import numpy as np
import pytest
import torch

import test_gpu_sparse_adam as spmod
import test_gpu_stepper_sequences as seqmod
from test_gpu_bf16_step import BF16, bits, shadow_is_current
from test_gpu_frontier import DEV, handle, listed, t
from test_gpu_stepper_sequences import check, check_invariants, figures, rel_err, restate, state
from test_large_graph_host import NE, NE_U, batch_e, graph_e, sets_e, table_e

pytestmark = pytest.mark.gpu

SENT = 12345.0
WD = seqmod.WD
_cache = {}


@pytest.fixture(scope="module")
def g_e():
    g = handle(graph_e())
    assert not g.bin_packed and not g.packed_words                       # the adjacent-row layout of a source table beyond 16 MiB
    return g


def dev_rows(rows):
    return t(np.asarray(rows, np.int64))


def mask_of(rows, n=NE):
    m = torch.zeros(n, dtype=torch.bool, device=DEV)
    m[dev_rows(rows)] = True
    return m


def heavy_f1():
    """(Bset, F1, F2) of the heavy BCE batch of 256 samples."""
    return sets_e(batch_e("bce", "heavy", 100, 256))


def big_list():
    """70 001 distinct rows of the 150 000, shuffled, with three out-of-range entries planted: (the list, the rows in range)."""
    rng = np.random.default_rng(61)
    rows = rng.permutation(NE)[:70001]
    lst = np.insert(rows, [5, 33000, 70000], [-1, NE, NE + 77])
    assert len(lst) == 70004 and len(np.unique(rows)) == 70001
    return lst, rows


# ================================================================================================ Part A: kernels alone
@pytest.mark.parametrize("kind,n", [("bce", 256), ("bpr", 2048)])
def test_frontier_list_is_the_numpy_set_in_three_segments_on_graph_e(g_e, kind, n):
    """spex_frontier_rows_i32 twice (F1, then F2 over 81 000 input rows: more than kFrontierMaxWgs x 4) for `heavy`, then `light`, then
    `heavy` again on one stamp table: the three segments are Bset, F1 minus Bset, F2 minus F1; the stamp table holds the epoch exactly
    on F2."""
    from spex_amd import ops
    fr = ops.FrontierRows(NE, torch.device(DEV, torch.cuda.current_device()))
    for k, which in enumerate(("heavy", "light", "heavy")):
        el = batch_e(kind, which, 100 + k, n)
        bset, f1, f2 = sets_e(el)
        a = t(el[1][0])
        b = t(el[1][1]) if kind == "bce" else t(np.concatenate([el[1][1], el[1][2]]))
        fr.update(a, b, 0, NE_U).expand(g_e).expand2(g_e)
        cb, cf, cf2, _ = fr.counts.cpu().numpy()
        lst = fr.list.cpu().numpy()
        assert (cb, cf, cf2) == (len(bset), len(f1), len(f2)), (which, cb, cf, cf2)
        assert np.array_equal(np.sort(lst[:cb]), bset), which
        assert np.array_equal(np.sort(lst[cb:cf]), np.setdiff1d(f1, bset)), which
        assert np.array_equal(np.sort(lst[cf:cf2]), np.setdiff1d(f2, f1)), which
        assert np.array_equal(np.flatnonzero(fr.stamp.cpu().numpy() == fr.epoch), f2), which
    assert fr.epoch == 3


@pytest.mark.parametrize("step", [1, 7])
def test_adam_rows_equals_the_dense_pass_bit_for_bit_past_its_first_pass(step):
    """spex_adam_rows_f32 over 70 004 list slots (2 048 blocks x 32 slots = 65 536 per pass) against spex_adam_step_f32 over the
    150 000 rows (4.6 passes): equal bit for bit on the listed rows, p, m, v untouched elsewhere."""
    from spex_amd import ops
    lst, rows = big_list()
    gen = torch.Generator(device=DEV).manual_seed(50 + step)
    p0, g, m0, v0 = (torch.randn(NE, 64, device=DEV, generator=gen) for _ in range(4))
    v0 = v0.abs()
    want = [x.clone() for x in (p0, m0, v0)]
    ops.adam_step(want[0], g, want[1], want[2], step, spmod.LR, spmod.B1, spmod.B2, spmod.EPS)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.adam_rows(p, g, m, v, listed(NE, lst), step, spmod.LR, spmod.B1, spmod.B2, spmod.EPS)
    mask = mask_of(rows)
    assert int(mask.sum()) == 70001
    for got, new, old, name in zip((p, m, v), want, (p0, m0, v0), "pmv"):
        assert torch.equal(got[mask], new[mask]), name
        assert torch.equal(got[~mask], old[~mask]), name
        assert not torch.equal(new[mask], old[mask])


def test_dense_adam_pass_vs_oracle_past_its_first_pass(oracle):
    """spex_adam_step_f32 on 150 000 x 64 + 3 floats against oracle.adam_step at t = 1, 2 and 100 000 under the 1e-6 of
    test_adam_kernel_vs_oracle; with zero= the cleared buffer is all zero, its last three floats included."""
    from spex_amd import ops
    rng = np.random.default_rng(6)
    n = NE * 64 + 3
    p, g, m, v = (rng.standard_normal(n, dtype=np.float32) for _ in range(4))
    v = np.abs(v)
    pp, gg, mm, vv = t(p), t(g), t(m), t(v)
    for step in (1, 2, 100000):
        oracle.adam_step(p, g, m, v, step, lr=1e-3)
        ops.adam_step(pp, gg, mm, vv, step, lr=1e-3)
        figs = [rel_err(x.cpu().numpy(), y) for x, y in ((pp, p), (mm, m), (vv, v))]
        print(f"t={step}: p {figs[0]:.2e} m {figs[1]:.2e} v {figs[2]:.2e}")
        assert max(figs) <= 1e-6, (step, figs)
    z = torch.ones(n, device=DEV)
    oracle.adam_step(p, g, m, v, 100001, lr=1e-3)
    ops.adam_step(pp, gg, mm, vv, 100001, lr=1e-3, zero=z)
    assert rel_err(pp.cpu().numpy(), p) <= 1e-6 and torch.count_nonzero(z).item() == 0 and not z[-3:].any()


@pytest.mark.parametrize("d", [64, 256])
def test_zero_rows_past_its_first_pass(d):
    """spex_zero_rows_f32 over the 70 004-slot list (2 048 x 256 float4 per pass: 32 768 rows at d = 64, 8 192 at d = 256): exactly the
    listed rows are zero, every other row keeps the sentinel."""
    from spex_amd import ops
    lst, rows = big_list()
    x = torch.full((NE, d), SENT, device=DEV)
    ops.zero_rows(x, listed(NE, lst))
    mask = mask_of(rows)
    assert not x[mask].any() and (x[~mask] == SENT).all()


def scatter_fp64(csr, rows, src, scale, add=None, add_scale=None):
    """out = scale * A^T scatter(src) + add_scale * scatter(add) over `rows` in fp64 (NumPy), and the rows of `out` that receive
    anything."""
    rowptr, col, val = csr[:3]
    lens = (rowptr[rows + 1] - rowptr[rows]).astype(np.int64)
    e = np.repeat(rowptr[rows].astype(np.int64) - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(lens.sum())
    contrib = val[e].astype(np.float64)[:, None] * src[np.repeat(rows, lens)].astype(np.float64)
    order = np.argsort(col[e], kind="stable")
    cols, starts = np.unique(col[e][order], return_index=True)
    sums = scale * np.add.reduceat(contrib[order], starts, axis=0)
    touched = cols.astype(np.int64)
    if add is not None:
        touched = np.union1d(touched, rows)
    dense = np.zeros((len(touched), src.shape[1]))
    dense[np.searchsorted(touched, cols)] = sums
    if add is not None:
        dense[np.searchsorted(touched, rows)] += add_scale * add[rows].astype(np.float64)
    return touched, dense


def test_push_rows_over_a_list_beyond_its_grid_vs_fp64_scatter(g_e):
    """spex_spmm_push_rows_f32 and the _scaled form over the F1 list of `heavy` (81 000 rows; a grid of at most 65 536 workgroups)
    against an fp64 scatter in NumPy under the 2e-6 of test_unique_rows_and_push_form_spmm_vs_oracle; rows outside the list's column
    set are exactly zero."""
    from spex_amd import ops
    csr = graph_e()
    el = batch_e("bce", "heavy", 100, 256)
    bset, f1, _ = sets_e(el)
    assert len(f1) > 65536
    fr = ops.FrontierRows(NE, torch.device(DEV, torch.cuda.current_device()))
    fr.update(t(el[1][0]), t(el[1][1]), 0, NE_U).expand(g_e)
    assert fr.count_f.item() == len(f1)
    rng = np.random.default_rng(62)
    src = rng.standard_normal((NE, 64), dtype=np.float32)
    add = rng.standard_normal((NE, 64), dtype=np.float32)
    for add_scale in (None, 0.25):
        out = torch.zeros(NE, 64, device=DEV)
        ops.spmm_push_rows(g_e, fr, t(src), out, True, add=t(add), add_indexed=True, scale=0.5, add_scale=add_scale, frontier=True)
        touched, want = scatter_fp64(csr, f1, src, 0.5, add, 0.5 if add_scale is None else add_scale)
        got = out.cpu().numpy()
        fig = rel_err(got[touched], want)
        print(f"push over |F1| = {len(f1)} (add_scale {add_scale}): {fig:.2e}; {len(touched)} rows touched")
        assert fig <= 2e-6
        rest = np.ones(NE, bool)
        rest[touched] = False
        assert rest.any() and not got[rest].any()
        assert np.count_nonzero(np.abs(got[touched]).max(1)) == len(touched)          # every touched row did receive something


def test_rowlist_dev_on_a_handle_without_row_ids_equals_the_whole_graph_launch(g_e):
    """spex_spmm_rowlist_dev_f32 and spex_spmm_rowlist_dev_bf16_f32 over the shuffled F1 list of `heavy` on the adjacent-row handle:
    bit for bit the whole-graph launch on rows of up to 1 024 entries, within the SpMM bound (2e-6 of the row's maximum) on the hub
    row, whose segments the two launches add in different orders; unlisted rows keep their sentinel."""
    csr = graph_e()
    deg = np.diff(csr[0])
    _, f1, _ = heavy_f1()
    rows = np.random.default_rng(63).permutation(f1)
    assert 0 in rows and deg[0] > 1024 and NE - 1 in rows
    X = t(table_e())
    X16 = X.to(BF16)
    upto = dev_rows(rows[deg[rows] <= 1024])
    rest = ~mask_of(rows)
    whole = g_e.spmm(X)
    Y = torch.full_like(X, SENT)
    g_e.spmm_rows_dev(X, listed(NE, rows), Y=Y)
    assert torch.equal(Y[upto], whole[upto]) and (Y[rest] == SENT).all()
    assert rel_err(Y[0].cpu().numpy(), whole[0].cpu().numpy()) <= 2e-6
    whole32, whole16 = torch.empty_like(X), torch.empty_like(X16)
    g_e.spmm_bf16(X16, Y=whole32, Y16=whole16)
    Y, Y16 = torch.full_like(X, SENT), torch.full_like(X16, 7.0)
    g_e.spmm_rows_dev(None, listed(NE, rows), X16=X16, Y=Y, Y16=Y16)
    assert torch.equal(Y[upto], whole32[upto]) and torch.equal(bits(Y16[upto]), bits(whole16[upto]))
    assert (Y[rest] == SENT).all() and (Y16[rest] == 7.0).all()
    assert rel_err(Y[0].cpu().numpy(), whole32[0].cpu().numpy()) <= 2e-6
    assert torch.equal(bits(Y16[~rest]), bits(Y[~rest].to(BF16)))


def test_cast_bf16_past_its_first_pass_equals_torch_bit_for_bit():
    """spex_cast_bf16_f32 on 150 000 x 64 + 3 elements (4 096 x 256 x 4 per pass), 16-byte aligned and offset by one element (the
    scalar kernel), against torch's CPU cast."""
    from spex_amd.graph import cast_bf16
    x = torch.randn(NE * 64 + 4, generator=torch.Generator().manual_seed(3))
    xd = x.to(DEV)
    for lo in (0, 1):
        src = xd[lo:lo + NE * 64 + 3]
        assert src.is_contiguous() and src.data_ptr() % 16 == 4 * lo
        got = cast_bf16(src)
        assert torch.equal(bits(got).cpu(), bits(x[lo:lo + NE * 64 + 3].to(BF16))), lo


# ================================================================================================ Part B: whole one-call steps
@contextlib.contextmanager
def restating_on_graph_e():
    """seqmod.restate reads the module's graph, N, N_U and table: hand it graph (e) for the duration (the pattern of
    tests/test_gpu_frontier.py::restating_on_graph_b)."""
    saved = (seqmod._cache.get("hub"), seqmod.N, seqmod.N_U, seqmod.table)
    seqmod._cache["hub"], seqmod.N, seqmod.N_U, seqmod.table = graph_e()[:3], NE, NE_U, table_e
    try:
        yield
    finally:
        seqmod._cache["hub"], seqmod.N, seqmod.N_U, seqmod.table = saved
        if saved[0] is None:
            del seqmod._cache["hub"]


def seq_e(kind, n, whiches=("heavy", "light", "heavy")):
    return [batch_e(kind, which, 100 + k, n) + (None,) for k, which in enumerate(whiches)]


def truth_e(kind, n, L, d=64, sparse=None, whiches=("heavy", "light", "heavy")):
    """(the sequence, its fp64 truth per step, the fp32 restatement's figures per step), the last two keys kept."""
    key = (kind, n, L, d, sparse, whiches)
    if key not in _cache:
        while len(_cache) >= 2:
            _cache.pop(next(iter(_cache)))
        seq = seq_e(kind, n, whiches)
        with restating_on_graph_e():
            if sparse is None:
                want, f32 = restate(seq, d, L, WD, torch.float64), restate(seq, d, L, WD, torch.float32)
            else:
                want = spmod.restate_sparse(seq, list(sparse), L, WD, torch.float64)
                f32 = spmod.restate_sparse(seq, list(sparse), L, WD, torch.float32)
        _cache[key] = {"seq": seq, "want": want, "f32": [figures(a, b) for a, b in zip(f32, want)]}
    return _cache[key]


def rnd(x):
    return x.to(BF16).float()


def restate_rounded(seq, L, law):
    """The sequence on graph (e) in fp32 on the CPU, one Adam state; law[k] per step: 'fp32', 'sparse' (row-sparse Adam at the
    structural F2), 'bf16 whole' (push form: y1 = A bf16(E0), y_(l+1) = A bf16(y_l), the layer sum with the exact E0;
    backward P = (g + A^T g) / (L + 1) in fp32, L = 3: A^T bf16(A^T bf16(P)) + P, L = 2: A^T bf16(P) + g / 3) or 'bf16 frontier'
    (4.24: the same forward; backward L = 3: A^T bf16(A^T P) + P, L = 2: no rounding).  Straight-through: the gradient is propagated
    as if the roundings of the forward were the identity.  Per step the dict of seqmod.restate."""
    rowptr, col, val = graph_e()[:3]
    rows = np.repeat(np.arange(NE, dtype=np.int64), np.diff(rowptr))
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, col.astype(np.int64)])), torch.from_numpy(val), (NE, NE)).coalesce()
    At = A.t().coalesce()
    W = torch.from_numpy(table_e()).clone()
    m, v = torch.zeros_like(W), torch.zeros_like(W)
    out = []
    for step, (el, how) in enumerate(zip(seq, law), 1):
        kind, arrs = el[0], el[1]
        a, b, c = (torch.from_numpy(np.asarray(x)) for x in arrs)
        T = len(a)
        r16 = rnd if how.startswith("bf16") else (lambda x: x)
        with torch.no_grad():
            cur, acc = W, W
            for _ in range(L):
                cur = torch.sparse.mm(A, r16(cur))
                acc = acc + cur
            light0 = acc / (L + 1)
        lt, Wr = light0.clone().requires_grad_(True), W.clone().requires_grad_(True)
        if kind == "bpr":
            lu, lp, ln = lt[a], lt[NE_U + b], lt[NE_U + c]
            z = (lu * ln).sum(1) - (lu * lp).sum(1)
            norms = Wr[a].pow(2).sum() + Wr[NE_U + b].pow(2).sum() + Wr[NE_U + c].pow(2).sum()
            loss = torch.nn.functional.softplus(z).mean() + WD * 0.5 * norms / T
        else:
            loss = torch.nn.functional.binary_cross_entropy_with_logits((lt[a] * lt[NE_U + b]).sum(1), c.float())
        loss.backward()
        g = lt.grad
        with torch.no_grad():
            if how.startswith("bf16"):
                P = (g + torch.sparse.mm(At, g)) / (L + 1)
                if L == 3:
                    inner = torch.sparse.mm(At, rnd(P)) if how == "bf16 whole" else torch.sparse.mm(At, P)
                    grad = torch.sparse.mm(At, rnd(inner)) + P
                else:
                    grad = torch.sparse.mm(At, rnd(P) if how == "bf16 whole" else P) + g / (L + 1)
            else:
                cur, acc = g, g
                for _ in range(L):
                    cur = torch.sparse.mm(At, cur)
                    acc = acc + cur
                grad = acc / (L + 1)
            if Wr.grad is not None:
                grad = grad + Wr.grad
            m1 = m + (1 - spmod.B1) * (grad - m)
            v1 = spmod.B2 * v + (1 - spmod.B2) * grad * grad
            W1 = W - (seqmod.LR / (1 - spmod.B1 ** step)) * (m1 / (v1.sqrt() / np.sqrt(1 - spmod.B2 ** step) + spmod.EPS))
            if how == "sparse":
                keep = torch.zeros(NE, 1, dtype=torch.bool)
                keep[torch.from_numpy(sets_e(el)[2].astype(np.int64))] = True
                W, m, v = torch.where(keep, W1, W), torch.where(keep, m1, m), torch.where(keep, v1, v)
            else:
                W, m, v = W1, m1, v1
        out.append({"loss": float(loss.detach()), "E0": W.numpy().copy(), "m": m.numpy().copy(), "v": v.numpy().copy(), "grad": grad.numpy().copy()})
    return out


def yardstick_e(entry, L, law):
    """The figures of restate_rounded against the entry's fp64 truth, per step, once per law."""
    key = ("rounded", tuple(law))
    if key not in entry:
        entry[key] = [figures(a, b) for a, b in zip(restate_rounded(entry["seq"], L, law), entry["want"])]
    return entry[key]


def stepper_e(L, d=64, **kw):
    from spex_amd.trainer import LightGCNStepper
    bf16 = kw.pop("bf16", False)
    st = LightGCNStepper(handle(graph_e()), t(table_e(d).copy()), NE_U, n_layers=L, lr=seqmod.LR, weight_decay=WD, **kw)
    if bf16:
        st.gather_dtype = BF16
    return st


def take(st, el):
    return seqmod.take(st, el, "one call")


BF16_Q = ("loss", "E0", "m", "v")


def gate_bf16(tag, worst, yard):
    """The bf16 modules' margin: per quantity the kernels' worst figure <= 2 x the yardstick's worst figure."""
    print(f"{tag} worst: " + "  ".join(f"{q} {worst[q]:.3e} (restatement {yard[q]:.3e})" for q in BF16_Q))
    bad = {q: (worst[q], yard[q]) for q in BF16_Q if not worst[q] <= 2 * yard[q]}
    assert not bad, f"{tag}: {bad}"


def run_form(form, kind, n, L, d=64):
    """Three one-call steps of one form on a fresh stepper against the truth; returns the stepper's end state and loss sums."""
    sparse = (True, True, True) if form == "sparse" else None
    entry = truth_e(kind, n, L, d, sparse)
    seq, want, f32 = entry["seq"], entry["want"], entry["f32"]
    st = stepper_e(L, d, deterministic=True if form == "deterministic" else None, frontier=form in ("frontier", "sparse", "bf16 frontier"),
                   sparse_adam=form == "sparse", bf16=form.startswith("bf16"))
    tag0 = f"(e) {form} {kind} n={n} L={L} d={d}"
    worst = dict.fromkeys(BF16_Q, 0.0)
    losses = []
    for k, el in enumerate(seq):
        before = (st.E0.clone(), st.m.clone(), st.v.clone()) if form == "sparse" else None
        loss = take(st, el)
        losses.append(loss)
        tag = f"{tag0} step {k + 1}"
        check_invariants(st, True, tag)
        got = state(st, loss, kind == "bpr" and not form.startswith("bf16"))
        if form.startswith("bf16"):
            assert st._shadow_current and shadow_is_current(st), tag
            assert torch.equal(bits(st.E0_16).cpu(), bits(st.E0.cpu().to(BF16))), f"{tag}: the shadow is not torch's CPU cast of E0"
            figs = figures(got, want[k])
            print(f"{tag}: " + "  ".join(f"{q} {figs[q]:.3e}" for q in BF16_Q))
            worst = {q: max(worst[q], figs[q]) for q in BF16_Q}
        else:
            check(tag, got, want[k], f32[k])
        if form == "sparse":
            out = ~mask_of(sets_e(el)[2])
            assert out.any() and not st.grad_E0[out].any(), f"{tag}: grad_E0 is not zero outside F2"
            for x, was, name in zip((st.E0, st.m, st.v), before, ("E0", "m", "v")):
                assert torch.equal(x[out], was[out]), f"{tag}: {name} moved outside F2"
    assert st.t == 3
    if form.startswith("bf16"):
        yard = yardstick_e(entry, L, [form] * 3)
        gate_bf16(tag0, worst, {q: max(f[q] for f in yard) for q in BF16_Q})
    return (st.E0.clone(), st.m.clone(), st.v.clone()), losses


L3_CASES = ([("bce", 256, f) for f in ("whole", "deterministic", "frontier", "bf16 whole", "bf16 frontier")]
            + [("bce", 2048, f) for f in ("whole", "frontier")]
            + [("bpr", 256, f) for f in ("whole", "frontier", "bf16 whole", "bf16 frontier")]
            + [("bpr", 2048, f) for f in ("whole", "frontier")])


@pytest.mark.parametrize("kind,n,form", L3_CASES)
def test_one_call_steps_at_three_layers_on_graph_e(kind, n, form):
    """L = 3, d = 64: whole-graph fp32 (BPR at T = 2 048: the dense form), deterministic (twice, bit for bit), frontier, and both
    with bf16 gather tables."""
    end, losses = run_form(form, kind, n, 3)
    if form == "deterministic":
        end2, losses2 = run_form(form, kind, n, 3)
        assert all(torch.equal(x, y) for x, y in zip(end, end2)) and losses == losses2


def test_wide_bpr_steps_on_graph_e():
    """d = 128, L = 3, exact BPR at T = 256: the wide L2 Adam form (rows of 128: shift 5) over 150 000 rows."""
    run_form("whole", "bpr", 256, 3, d=128)


@pytest.mark.parametrize("kind,form", [(k, f) for k in ("bce", "bpr") for f in ("frontier", "sparse")])
def test_frontier_and_sparse_adam_steps_at_two_layers_on_graph_e(kind, form):
    """L = 2: the frontier step (dense Adam) and the row-sparse Adam step, whose list on `heavy` holds |F2| ~ 118 000 rows (65 536
    list slots per pass): rows outside the step's F2 stand still bit for bit and grad_E0 is zero there."""
    run_form(form, kind, 256, 2)


@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_forms_switched_on_one_stepper_on_graph_e(kind):
    """whole -> frontier -> sparse -> frontier + bf16 on ONE stepper (L = 2, one set of moments, one t) over heavy, light, heavy,
    light: the fp32 steps under seqmod's gate against the truth with step 3's row-sparse law, the bf16 step under the bf16 margin
    against restate_rounded of the same four steps."""
    whiches = ("heavy", "light", "heavy", "light")
    law = ("fp32", "fp32", "sparse", "bf16 frontier")
    entry = truth_e(kind, 256, 2, 64, (False, False, True, False), whiches)
    seq, want, f32 = entry["seq"], entry["want"], entry["f32"]
    yard = yardstick_e(entry, 2, law)
    st = stepper_e(2, frontier=True)
    tables = tuple(x.data_ptr() for x in (st.E0, st.m, st.v))
    for k, (el, how) in enumerate(zip(seq, law)):
        st.sparse_adam = False
        st.gather_dtype = BF16 if how == "bf16 frontier" else None
        st.frontier, st.sparse_adam = k > 0, how == "sparse"
        loss = take(st, el)
        tag = f"(e) switch {kind} step {k + 1} ({how}, {whiches[k]})"
        check_invariants(st, True, tag)
        got = state(st, loss, kind == "bpr" and how != "bf16 frontier")
        if how == "bf16 frontier":
            assert st._shadow_current and shadow_is_current(st), tag
            assert torch.equal(bits(st.E0_16).cpu(), bits(st.E0.cpu().to(BF16))), tag
            figs = figures(got, want[k])
            gate_bf16(tag, figs, yard[k])
        else:
            check(tag, got, want[k], f32[k])
        assert st.t == k + 1 and tables == tuple(x.data_ptr() for x in (st.E0, st.m, st.v))


# ================================================================================================ Part C: a table that crosses 4 GiB
def test_gather_table_that_crosses_4_gib(oracle):
    """A 2 048 x (2^24 + 4 096) handle, rows of 1 .. 200 entries and one of 1 100, 40 % of the stored columns at or beyond 2^24 (byte
    offsets of an fp32 [n_cols, 64] table beyond 2^32), column 2^24 - 1 and the last column named: spmm and spmm_rowlist_dev against
    the fp64 product of the named X rows (bit for bit the oracle's fmaf chain on rows of <= 64 entries, 2e-6 elsewhere:
    test_spmm_properties_on_an_hbm_resident_graph), then spex_spmm_push_rows_f32 into a zeroed [n_cols, 64] target: the named rows
    against the fp64 scatter, and as many non-zero elements as the expected rows have — a wrapped address is a stray row below 2^24."""
    from spex_amd import ops
    from spex_amd.graph import SpexGraph
    if torch.cuda.mem_get_info()[0] < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory")
    n, lo, n_cols = 2048, 1 << 24, (1 << 24) + 4096
    rng = np.random.default_rng(71)
    deg = rng.integers(1, 201, n)
    deg[7] = 1100
    cols = []
    for r in range(n):
        k_hi = int(round(0.4 * deg[r]))
        c = np.concatenate([np.unique(rng.integers(0, lo - 1, deg[r] - k_hi)), lo + rng.choice(4096, k_hi, replace=False)])
        if r == 0:
            c = np.union1d(c, [lo - 1, n_cols - 1])
        cols.append(np.sort(c))
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    col = np.concatenate(cols).astype(np.int32)
    val = (0.05 * rng.standard_normal(len(col))).astype(np.float32)
    assert 1 <= np.diff(rowptr).min() and np.diff(rowptr).max() <= 202 + 898 and np.diff(rowptr)[7] > 1024
    assert (col >= lo).mean() >= 1 / 3 and lo - 1 in col and n_cols - 1 in col and int(col.max()) * 256 > 1 << 32
    g = SpexGraph(rowptr, col, val, n_cols=n_cols)
    X = torch.randn(n_cols, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    assert X.numel() * 4 == (4 << 30) + (1 << 20)
    named, inv = np.unique(col, return_inverse=True)
    Xn = X[dev_rows(named)].cpu().numpy()
    ref = oracle.spmm(rowptr, inv.astype(np.int32), val, Xn)
    lens = np.diff(rowptr)
    want = np.add.reduceat(val.astype(np.float64)[:, None] * Xn[inv].astype(np.float64), rowptr[:-1].astype(np.int64), axis=0)
    short = lens <= 64
    Y = g.spmm(X)
    Yl = torch.full((n, 64), SENT, device=DEV)
    g.spmm_rows_dev(X, listed(n, rng.permutation(n)), Y=Yl)
    for name, got in (("spmm", Y.cpu().numpy()), ("spmm_rowlist_dev", Yl.cpu().numpy())):
        fig = rel_err(got, want)
        print(f"{name}: {fig:.2e} against the fp64 product")
        assert np.array_equal(got[short], ref[short]), name
        assert fig <= 2e-6, (name, fig)
    del Y, Yl
    # the push form: out[c] += A[r, c] * src[r] into the 4 GiB + 1 MiB target
    src = rng.standard_normal((n, 64), dtype=np.float32)
    out = torch.zeros(n_cols, 64, device=DEV)
    ops.spmm_push_rows(g, listed(n, np.arange(n)), t(src), out, True)
    touched, expect = scatter_fp64((rowptr, col, val), np.arange(n), src, 1.0)
    assert np.array_equal(touched, named)
    got = out[dev_rows(named)].cpu().numpy()
    fig = rel_err(got, expect)
    print(f"push: {fig:.2e} against the fp64 scatter over {len(named)} rows")
    assert fig <= 2e-6
    assert torch.count_nonzero(out).item() == np.count_nonzero(got)
