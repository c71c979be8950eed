"""SPEX_STEP_SPARSE_ADAM: row-sparse ("lazy") Adam for the L = 2 frontier steps — E0, m, v change at the rows of the batch's two-hop
set F2 = F1 U { stored columns of F1's rows } by dense Adam's own expression with the global step count, and stand still bit for bit
everywhere else.

Graphs, batches and steppers are those of tests/test_gpu_frontier.py (graph (b): 20 000 rows, ~3 entries per row, a 1 500-entry hub;
the tiny golden graph; the non-symmetric hub graph of tests/test_gpu_stepper_sequences.py), imported.  Whole steps are compared with
an fp64 restatement of the SEQUENCE on the CPU (`restate_sparse`, patterned on seqmod.restate: autograd through L sparse layers and
the layer mean, then Adam by torch's formula) in which p, m, v change only at the structural F2 of each sparse step's batch — taken
over the rows of A, not of A^T.  The gate is seqmod's, unchanged: per quantity the larger of the project's bound and 4 x the figure
of the same sequence restated in fp32 on the CPU (`seqmod.figures`, `check`, `bounds_of`).  A row that wrongly coasted on its
momentum moves by ~lr = 1e-3 against a table of maximum ~0.4: 2e-3 relative, far above the E0 bound of 5e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_frontier as frmod
import test_gpu_stepper_sequences as seqmod
from test_gpu_frontier import DEV, NB, NB_I, NB_U, batch_b, graph_b, handle, restating_on_graph_b, stepper_b, stepper_hub, t, table_b, tiny

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def G():
    from spex_amd.graph import SpexGraph
    return SpexGraph


def sets_of(csr, rows):
    """(Bset, F1, F2) as sorted arrays, in NumPy: two applications of the frontier's one-hop rule."""
    bset, f1 = frmod.frontier_sets(csr, rows)
    return bset, f1, frmod.frontier_sets(csr, f1)[1]


def batch_rows(el, n_u):
    kind, arrs = el[0], el[1]
    if kind == "bce":
        return np.concatenate([arrs[0], arrs[1] + n_u])
    return np.concatenate([arrs[0], arrs[1] + n_u, arrs[2] + n_u])


# ------------------------------------------------------------------------------------------ 1. the kernel against the dense pass
def listed(n, rows, capacity=None):
    ur = frmod.listed(n, np.asarray(rows, np.int32))
    if capacity is not None:
        ur.capacity = capacity                      # the host-side bound handed to the kernel as max_count
    return ur


@pytest.mark.parametrize("step", [1, 7])
def test_adam_rows_equals_the_dense_pass_bit_for_bit_on_its_rows(step):
    from spex_amd import ops
    n = 300
    rng = np.random.default_rng(50 + step)
    p0, g, m0, v0 = (t(rng.normal(size=(n, 64)).astype(np.float32)) for _ in range(4))
    v0 = v0.abs()
    want = [x.clone() for x in (p0, m0, v0)]
    ops.adam_step(want[0], g, want[1], want[2], step, LR, B1, B2, EPS)
    cases = [(rng.permutation(n)[:k], None) for k in (0, 1, 3, 5, 257)]
    cases.append((np.array([5, -1, 17, n, 42]), None))                 # values outside [0, n_rows) are skipped
    cases.append((rng.permutation(n)[:9], 6))                          # max_count below the count: the list is cut there
    for rows, cap in cases:
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        ops.adam_rows(p, g, m, v, listed(n, rows, cap), step, LR, B1, B2, EPS)
        live = np.array([r for r in rows[:cap] if 0 <= r < n], np.int64)
        mask = torch.zeros(n, dtype=torch.bool, device=DEV)
        mask[t(live)] = True
        for got, new, old, name in zip((p, m, v), want, (p0, m0, v0), "pmv"):
            assert torch.equal(got[mask], new[mask]), (name, len(rows), cap)
            assert torch.equal(got[~mask], old[~mask]), (name, len(rows), cap)
        x = p0.clone()
        ops.zero_rows(x, listed(n, rows, cap))
        assert not x[mask].any() and torch.equal(x[~mask], p0[~mask]), (len(rows), cap)
    assert not torch.equal(want[0], p0)


# ------------------------------------------------------------------------------------------ 2. the F2 list
@pytest.mark.parametrize("which", ["tiny", "b"])
def test_two_hop_list_is_the_numpy_set_in_three_segments(which):
    from spex_amd import ops
    if which == "tiny":
        rowptr, col, val, n_u, _ = tiny()
        csr, n = (rowptr, col, val), len(rowptr) - 1
        batches = [(np.array([0, 3, 3, 7, 49], np.int64), np.array([1, 1, 5, 20, 59], np.int64)), (np.array([2], np.int64), np.array([4], np.int64))]
    else:
        csr, n, n_u = graph_b()[:3], NB, NB_U
        batches = [batch_b("bce", s, k, hub=hub)[1][:2] for s, k, hub in ((1, 7, True), (2, 256, True), (3, 256, False))]
        batches.append((np.array([0, 0, 12, 9000, -4], np.int64), np.array([5, NB_I - 1, 5, NB_I + 3, 7], np.int64)))   # hub, empty, invalid
        assert 0 in batches[1][0] and 12 in batches[1][0]
    g = handle(csr)
    fr = ops.FrontierRows(n, torch.device(DEV, torch.cuda.current_device()))
    for k, (a, b) in enumerate(batches * 2):                    # the second round: new epochs on the same stamp table, no clearing
        fr.update(t(a), t(b), 0, n_u).expand(g).expand2(g)
        bset, f1, f2 = sets_of(csr, np.concatenate([a, b + n_u]))
        cb, cf, cf2, spare = fr.counts.cpu().numpy()
        lst = fr.list.cpu().numpy()
        assert (cb, cf, cf2) == (len(bset), len(f1), len(f2)), (which, k)
        assert np.array_equal(np.sort(lst[:cb]), bset), (which, k)
        assert np.array_equal(np.sort(lst[cb:cf]), np.setdiff1d(f1, bset)), (which, k)
        assert np.array_equal(np.sort(lst[cf:cf2]), np.setdiff1d(f2, f1)), (which, k)
        assert len(np.unique(lst[:cf2])) == cf2, (which, k)
    assert fr.epoch == 2 * len(batches)


# ------------------------------------------------------------------------------------------ the truth
def restate_sparse(seq, sparse, L, weight_decay, dtype):
    """The sequence `seq` of (kind, arrays, None) on seqmod's current graph and table in `dtype` on the CPU, one Adam state and one t;
    where sparse[k], step k changes E0, m, v only at the structural F2 of its batch (rows of A).  Per step the dict of seqmod.restate."""
    rowptr, col, val = seqmod.hub_graph()
    N, N_U = seqmod.N, seqmod.N_U
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    idx = torch.from_numpy(np.stack([rows, col.astype(np.int64)]))
    A = torch.sparse_coo_tensor(idx, torch.from_numpy(val.astype(np.float64)).to(dtype), (N, N)).coalesce()
    W = torch.from_numpy(seqmod.table(64)).to(dtype)
    m, v = torch.zeros_like(W), torch.zeros_like(W)
    out = []
    for step, (el, sp) in enumerate(zip(seq, sparse), 1):
        kind, arrs = el[0], el[1]
        a, b, c = (torch.from_numpy(np.asarray(x)) for x in arrs)
        T = len(a)
        Wr = W.clone().requires_grad_(True)
        cur, acc = Wr, Wr
        for _ in range(L):
            cur = torch.sparse.mm(A, cur)
            acc = acc + cur
        light = acc / (L + 1)
        if kind == "bpr":
            lu, lp, ln = light[a], light[N_U + b], light[N_U + c]
            z = (lu * ln).sum(1) - (lu * lp).sum(1)
            norms = Wr[a].pow(2).sum() + Wr[N_U + b].pow(2).sum() + Wr[N_U + c].pow(2).sum()
            loss = torch.nn.functional.softplus(z).mean() + weight_decay * 0.5 * norms / T
        else:
            loss = torch.nn.functional.binary_cross_entropy_with_logits((light[a] * light[N_U + b]).sum(1), c.to(dtype))
        loss.backward()
        g = Wr.grad
        m1 = m + (1 - B1) * (g - m)
        v1 = B2 * v + (1 - B2) * g * g
        denom = v1.sqrt() / np.sqrt(1 - B2 ** step) + EPS
        W1 = W - (LR / (1 - B1 ** step)) * (m1 / denom)
        if sp:
            f2 = sets_of((rowptr, col), batch_rows(el, N_U))[2]
            assert not g[np.setdiff1d(np.arange(N), f2)].any()           # the support is structural
            keep = torch.zeros(N, 1, dtype=torch.bool)
            keep[torch.from_numpy(f2.astype(np.int64))] = True
            W, m, v = torch.where(keep, W1, W), torch.where(keep, m1, m), torch.where(keep, v1, v)
        else:
            W, m, v = W1, m1, v1
        out.append({"loss": float(loss.detach()), "E0": W.numpy().copy(), "m": m.numpy().copy(), "v": v.numpy().copy(), "grad": g.numpy().copy()})
    return out


_truth = {}


def truth_of(key, seq, sparse, L=2):
    if key not in _truth:
        while len(_truth) >= 3:
            _truth.pop(next(iter(_truth)))
        want = restate_sparse(seq, sparse, L, seqmod.WD, torch.float64)
        f32 = restate_sparse(seq, sparse, L, seqmod.WD, torch.float32)
        _truth[key] = (want, [seqmod.figures(x, y) for x, y in zip(f32, want)])
    return _truth[key]


def sparse_stepper(which, G=None):
    st = stepper_b(2, True) if which == "b" else stepper_hub(G, 2)
    st.sparse_adam = True
    return st


def outside(csr, el, n_u, n):
    """Boolean device mask of the rows outside the structural F2 of a batch."""
    mask = torch.ones(n, dtype=torch.bool, device=DEV)
    mask[t(sets_of(csr, batch_rows(el, n_u))[2].astype(np.int64))] = False
    return mask


# ------------------------------------------------------------------------------------------ 3. steps against the fp64 truth
@pytest.mark.parametrize("which,kind,n", [(w, k, n) for w in ("b", "hub") for k, n in (("bce", 7), ("bce", 256), ("bpr", 5), ("bpr", 300))])
def test_sparse_adam_steps_against_the_fp64_truth(G, which, kind, n):
    """Six steps, one call and launch by launch; on graph (b) every other batch keeps the hub out of F1, so that most rows lie
    outside F2.  After every step: the invariants every one-call step owes the next, and grad_E0 exactly zero outside F2."""
    if which == "b":
        seq = [batch_b(kind, 1000 + k, n, hub=k % 2 == 1) + (None,) for k in range(6)]
        with restating_on_graph_b():
            want, f32 = truth_of((which, kind, n), seq, [True] * 6)
        csr, n_u, n_rows = graph_b()[:2], NB_U, NB
    else:
        seq = [frmod.hub_batch(kind, 1100 + k, n) + (None,) for k in range(6)]
        want, f32 = truth_of((which, kind, n), seq, [True] * 6)
        csr, n_u, n_rows = seqmod.hub_graph()[:2], seqmod.N_U, seqmod.N
    for form in ("one call", "launches"):
        st = sparse_stepper(which, G)
        for k, el in enumerate(seq):
            loss = seqmod.take(st, el, form)
            tag = f"sparse adam ({which}) {kind} n={n} {form} step {k + 1}"
            seqmod.check_invariants(st, form == "one call", tag)
            out = outside(csr, el, n_u, n_rows)
            assert not st.grad_E0[out].any(), f"{tag}: grad_E0 is not zero outside F2"
            seqmod.check(tag, seqmod.state(st, loss, kind == "bpr"), want[k], f32[k])
        assert st.t == 6


# ------------------------------------------------------------------------------------------ 4. rows outside F2 stand still
@pytest.mark.parametrize("kind,n", [("bce", 256), ("bpr", 300)])
def test_rows_outside_f2_stand_still_bit_for_bit(kind, n):
    csr = graph_b()[:2]
    els = [batch_b(kind, 1200 + k, n, hub=False) for k in range(2)]
    f2 = [sets_of(csr, batch_rows(el, NB_U))[2] for el in els]
    still = np.setdiff1d(f2[0], f2[1])
    never = np.setdiff1d(np.arange(NB), np.union1d(f2[0], f2[1]))
    print(f"|F2| {len(f2[0])}, {len(f2[1])} of {NB} rows; in the first only: {len(still)}; in neither: {len(never)}")
    assert len(still) >= 100 and len(never) >= 100
    rows = t(still.astype(np.int64))
    a, b = stepper_b(2, True), stepper_b(2, True)
    a.sparse_adam = True
    after1 = {}
    for st, name in ((a, "sparse"), (b, "dense")):
        acc = torch.zeros(1, device=DEV)
        args = [t(x) for x in els[0][1]]
        (st.step_bce if kind == "bce" else st.step_bpr_exact)(*args, loss_acc=acc, batch_rows_only=True)
        after1[name] = (acc.clone(), st.E0[rows].clone(), st.m[rows].clone(), st.v[rows].clone())
        args = [t(x) for x in els[1][1]]
        (st.step_bce if kind == "bce" else st.step_bpr_exact)(*args, loss_acc=acc, batch_rows_only=True)
    # the first step's loss sum is the dense-Adam frontier step's bit for bit: one addend, the same fixed order
    assert torch.equal(after1["sparse"][0], after1["dense"][0]) and after1["dense"][0].item() != 0.0
    for x, was in zip((a.E0, a.m, a.v), after1["sparse"][1:]):
        assert torch.equal(x[rows], was)
    for x, was in zip((b.E0, b.m, b.v), after1["dense"][1:]):
        assert not torch.equal(x[rows], was)                  # under dense Adam the same rows coast on their momentum
    # and rows that no batch reached were never touched at all
    never = t(never.astype(np.int64))
    assert torch.equal(a.E0[never], t(table_b())[never]) and not a.m[never].any() and not a.v[never].any()


# ------------------------------------------------------------------------------------------ 5. forms alternate on one stepper
def test_sparse_dense_frontier_and_whole_graph_steps_alternate_on_one_stepper():
    """Nine steps on one stepper, (frontier, sparse_adam) switched from step to step.  A whole-graph or dense-Adam step leaves grad_E0
    full: the next sparse step must clear the whole table, not only the rows of a list that no longer describes it."""
    plan = [("bpr", "one call", True, True), ("bce", "one call", False, True), ("bce", "launches", True, True),
            ("bpr", "one call", True, False), ("bce", "epoch", True, True), ("bpr", "launches", True, True),
            ("bce", "one call", True, True), ("bpr", "one call", True, True), ("bce", "launches", False, False)]
    seq = [batch_b(kind, 1300 + k, 17, hub=k % 3 == 0) + (None,) for k, (kind, _, _, _) in enumerate(plan)]
    law = [fr and sp for _, _, fr, sp in plan]
    with restating_on_graph_b():
        want, f32 = truth_of(("mix",), seq, law)
    csr = graph_b()[:2]
    st = stepper_b(2, True)
    for k, ((kind, form, frontier, sparse), el) in enumerate(zip(plan, seq)):
        st.frontier, st.sparse_adam = frontier, sparse
        tag = f"mix step {k + 1} ({kind}, {form}, frontier={frontier}, sparse_adam={sparse})"
        if form == "epoch":
            full, ragged = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
            st.epoch_bce(*(t(x) for x in el[1]), 17, full, ragged)
            loss = full.item() / 17
        else:
            loss = seqmod.take(st, el, form)
        assert st.t == k + 1
        seqmod.check_invariants(st, form != "launches", tag)
        if law[k]:
            assert not st.grad_E0[outside(csr, el, NB_U, NB)].any(), f"{tag}: grad_E0 is not zero outside F2"
        seqmod.check(tag, seqmod.state(st, loss, kind == "bpr"), want[k], f32[k])


def test_a_write_to_grad_E0_between_sparse_steps_is_noticed():
    """The user fills grad_E0 between two sparse one-call steps: the second clears the whole table, not the listed rows only."""
    els = [batch_b("bce", 1400 + k, 17, hub=False) for k in range(2)]
    st = sparse_stepper("b")
    acc = torch.zeros(1, device=DEV)
    st.step_bce(*(t(x) for x in els[0][1]), loss_acc=acc, batch_rows_only=True)
    st.grad_E0.fill_(3.0)
    st.step_bce(*(t(x) for x in els[1][1]), loss_acc=acc, batch_rows_only=True)
    assert not st.grad_E0[outside(graph_b()[:2], els[1], NB_U, NB)].any() and torch.isfinite(st.E0).all()
    assert st.E0.abs().max().item() < 1.0


# ------------------------------------------------------------------------------------------ 6. epochs
def test_sparse_adam_epochs_equal_the_looped_one_call_steps():
    from spex_amd.trainer import BceDeviceSampler, BprDeviceSampler
    pairs = graph_b()[3]
    B, steps = 256, 5
    s = BceDeviceSampler(pairs, NB_U, NB_I, num_ng=1, seed=5, device=DEV)
    a, b, c = sparse_stepper("b"), sparse_stepper("b"), sparse_stepper("b")
    acc_a, acc_b, acc_c = (torch.zeros(2, 1, device=DEV) for _ in range(3))
    a.epoch_bce_sampled(s, 3, B, acc_a[0], acc_a[1], max_steps=steps)
    u, i, y = (x.clone() for x in s.draw(3))
    b.epoch_bce(u, i, y, B, acc_b[0], acc_b[1], max_steps=steps)
    for k in range(steps):
        c.step_bce(u[k * B:(k + 1) * B], i[k * B:(k + 1) * B], y[k * B:(k + 1) * B], loss_acc=acc_c[0], batch_rows_only=True)
    assert a.t == b.t == c.t == steps
    frmod.compare("sampled BCE epoch, sparse adam", acc_a[0].cpu().numpy(), acc_c[0].cpu().numpy(), a, c)
    frmod.compare("native BCE epoch, sparse adam", acc_b[0].cpu().numpy(), acc_c[0].cpu().numpy(), b, c)
    # exact BPR, weight_decay > 0: 1 100 triples = three full batches of 300 and a ragged one
    s = BprDeviceSampler(pairs, NB_U, NB_I, torch.device(DEV, torch.cuda.current_device()), seed=6, n=1100)
    a, c = sparse_stepper("b"), sparse_stepper("b")
    acc_a, acc_c = torch.zeros(2, 1, device=DEV), torch.zeros(2, 1, device=DEV)
    a.epoch_bpr_sampled(s, 2, 300, acc_a[0], acc_a[1])
    u, p, ng = (x.clone() for x in s.draw(2))
    for k in range(4):
        sl = slice(k * 300, min((k + 1) * 300, 1100))
        c.step_bpr_exact(u[sl], p[sl], ng[sl], loss_acc=acc_c[0 if k < 3 else 1], batch_rows_only=True)
    assert a.t == c.t == 4
    frmod.compare("sampled BPR epoch, sparse adam", acc_a.cpu().numpy(), acc_c.cpu().numpy(), a, c)
    b = sparse_stepper("b")
    acc_b = torch.zeros(2, 1, device=DEV)
    b.epoch_bpr(u, p, ng, 300, acc_b[0], acc_b[1])
    assert b.t == 4
    frmod.compare("native BPR epoch, sparse adam", acc_b.cpu().numpy(), acc_c.cpu().numpy(), b, c)


def test_train_epoch_drivers_take_a_sparse_adam_stepper_as_they_are():
    from spex_amd.trainer import BceDeviceSampler, BprDeviceSampler, train_epoch, train_epoch_bpr
    pairs = graph_b()[3]
    B, steps = 256, 4
    s = BceDeviceSampler(pairs, NB_U, NB_I, num_ng=1, seed=9, device=DEV)
    a, c = sparse_stepper("b"), sparse_stepper("b")
    got = train_epoch(a, s, batch_size=B, epoch=0, max_steps=steps).item()
    acc = torch.zeros(2, 1, device=DEV)
    c.epoch_bce_sampled(s, 0, B, acc[0], acc[1], max_steps=steps)
    assert a.t == c.t == steps
    frmod.compare("train_epoch, sparse adam", [got * B], acc[0].cpu().numpy(), a, c)
    s = BprDeviceSampler(pairs, NB_U, NB_I, torch.device(DEV, torch.cuda.current_device()), seed=10, n=600)
    a, c = sparse_stepper("b"), sparse_stepper("b")
    got = float(train_epoch_bpr(a, s, batch_size=300, epoch=1))
    acc = torch.zeros(2, 1, device=DEV)
    c.epoch_bpr_sampled(s, 1, 300, acc[0], acc[1])
    frmod.compare("train_epoch_bpr, sparse adam", [got * 300], acc[0].cpu().numpy(), a, c)


# ------------------------------------------------------------------------------------------ 7. refusals
def test_python_refusals():
    from spex_amd.trainer import LightGCNStepper
    g = handle(graph_b())
    E0 = t(table_b().copy())
    with pytest.raises(ValueError, match="only with frontier=True and n_layers == 2"):
        LightGCNStepper(g, E0, NB_U, n_layers=2, sparse_adam=True)
    with pytest.raises(ValueError, match="only with frontier=True and n_layers == 2"):
        LightGCNStepper(g, E0, NB_U, n_layers=3, frontier=True, sparse_adam=True)
    plain = LightGCNStepper(g, E0, NB_U, n_layers=2)
    with pytest.raises(ValueError, match="built with frontier=True and n_layers == 2"):
        plain.sparse_adam = True
    deep = LightGCNStepper(g, E0, NB_U, n_layers=3, frontier=True)
    with pytest.raises(ValueError, match="built with frontier=True and n_layers == 2"):
        deep.sparse_adam = True
    st = LightGCNStepper(g, E0, NB_U, n_layers=2, frontier=True, sparse_adam=True)
    assert st.sparse_adam is True
    st.sparse_adam = False
    st.sparse_adam = True
    st.frontier = False                              # ignored while the frontier form is off
    assert st.sparse_adam is True and st.t == 0


def test_native_refusals():
    from spex_amd import _lib
    from spex_amd.graph import _stream
    from spex_amd.trainer import LightGCNStepper
    lib = _lib.load()
    g = handle(graph_b())
    _, (u, i, y) = batch_b("bce", 1, 7)
    u, i, y = t(u), t(i), t(y)
    acc = torch.zeros(1, device=DEV)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def status(st, flags, bpr=False, L=None, d=None, drop_list=False):
        desc = st._prepare_desc(7, 3 if bpr else 2)
        desc.flags = flags
        desc.L = st.L if L is None else L
        desc.d = 64 if d is None else d
        saved = desc.frontier_list
        if drop_list:
            desc.frontier_list = None
        name = "spex_lightgcn_step_bpr_adam_f32" if bpr else "spex_lightgcn_step_bce_f32"
        rc = getattr(lib, name)(ctypes.byref(desc), vp(u), vp(i), vp(i) if bpr else vp(y), 7, vp(acc), _stream(None))
        t_after = desc.t
        desc.frontier_list, desc.L, desc.d = saved, st.L, 64
        assert t_after == 0
        return rc, lib.spex_last_error().decode()

    st = LightGCNStepper(g, t(table_b().copy()), NB_U, n_layers=2, frontier=True, sparse_adam=True)
    F, S = _lib.STEP_FRONTIER, _lib.STEP_SPARSE_ADAM
    for bpr in (False, True):
        rc, msg = status(st, S, bpr)
        assert rc == -1 and "needs SPEX_STEP_FRONTIER" in msg
        rc, msg = status(st, F | S, bpr, L=3)
        assert rc == -1 and "L == 2" in msg
        rc, msg = status(st, F | S, bpr, L=1)
        assert rc == -1
        # everything the frontier form refuses stays refused
        rc, msg = status(st, F | S | _lib.STEP_DETERMINISTIC, bpr)
        assert rc == -1 and "SPEX_STEP_DETERMINISTIC" in msg
        rc, msg = status(st, F | S | _lib.STEP_BF16_GATHER, bpr)
        assert rc in (-1, -4)
        rc, msg = status(st, F | S, bpr, d=128)
        assert rc in (-1, -4) and ("d == 64" in msg or "d=128" in msg or "d = 128" in msg), msg
        rc, msg = status(st, F | S, bpr, drop_list=True)
        assert rc == -1 and "frontier_list" in msg
    rc, msg = status(st, F | S | _lib.STEP_BPR_DENSE, True)
    assert rc == -1 and "SPEX_STEP_BPR_DENSE" in msg
    rc, msg = status(st, F | S | _lib.STEP_WIDE, True)
    assert rc == -4 and "d == 64" in msg
    keep = torch.ones(len(graph_b()[1]), dtype=torch.uint8, device=DEV)
    g.set_edge_mask(1, keep, 0.6, 0)
    try:
        rc, msg = status(st, F | S)
        assert rc == -1 and "edge dropout" in msg
    finally:
        g.set_edge_mask(0)
    assert st.t == 0 and not st.E0.isnan().any() and torch.equal(st.E0, t(table_b()))
