"""Packed words in the chunk table (graph.hip / spmm_chunk.h: a bin-packed table of at most 65 536 rows stores
(output row << 16) | source row in one word per entry and has no row array).  Only where an entry's output row is read from changed,
so every product is what it was, bit for bit: each case below is torch.equal between a handle built normally (packed) and one built
under SPEX_PACK_WORDS=0 (the three-array layout, the kernels' other path), and the plain products are also held to
test_gpu_spmm_implied.py's `documented_order`, the restatement of DESIGN 4.1's summation order.

Fixture: 300 user rows x 900 items, 12 000 drawn interactions through lightgcn_norm_adj, then altered row by row (the matrix need not
stay symmetric: every comparison runs the same matrix through both layouts) so that it holds rows of exactly 1, 16, 17, 63, 64, 65,
68, 69, 76, 77, 200 and 1 024 entries, a hub of 1 100 (the in-kernel fold) — 900 in the hub-free twin the steps run on, so that the
fused BPR launch is taken — and 40 rows without a stored entry (lists of empty rows).  Its transpose carries the edge-id permutation.

The exact steps are compared bit for bit with deterministic=True: the default mode adds gradients with float atomics whose order is
free, so two runs of ONE layout need not agree in the last bit; the fixed-order mode runs the same chunk kernels and must.  The
default mode is compared too, to the tolerances test_gpu_bpr_step_fused_last.py uses where the atomics' order is free.

The 16-bit edge: a 65 536 x 65 536 table (the largest that packs; its fp32 gather table is 16 MB) with entries in row 65 535 and
column 65 535, among them (65 535, 65 535) whose word is 0xFFFFFFFF — the value the dropout path uses as its dropped mark on the
source-row half — against the unpacked handle, plain and under both dropout modes; one node more, or more than 65 536 rows, and the
handle reports the row array and gives the same rows."""
import os

import numpy as np
import pytest
import torch

from test_gpu_bpr_step_fused_last import one_step, rel_err
from test_gpu_spmm_implied import documented_order

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEEP_PROB = 0.8
N_U, N_I = 300, 900
N = N_U + N_I
DEGS = [1, 16, 17, 63, 64, 65, 68, 69, 76, 77, 200, 1024]
HUB_DEG, NO_HUB_DEG = 1100, 900
EMPTY = list(range(250, 270)) + list(range(N_U + 800, N_U + 820))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def special_row(k):
    return 3 * k + 1            # user rows 1, 4, 7, ...: apart, so that first-fit does not pack them together by construction


def fixture_csr(hub):
    from spex_amd.graph import lightgcn_norm_adj
    rng = np.random.default_rng(2024)
    rowptr, col, val = lightgcn_norm_adj(rng.integers(0, N_U - 1, 12000), rng.integers(0, N_I, 12000), N_U - 1, N_I)
    rows = [(col[rowptr[r]:rowptr[r + 1]], val[rowptr[r]:rowptr[r + 1]]) for r in range(N)]
    for k, deg in enumerate(DEGS + [HUB_DEG if hub else NO_HUB_DEG]):
        rows[special_row(k)] = (np.sort(rng.choice(N, deg, replace=False)).astype(np.int32), rng.uniform(0.01, 0.1, deg).astype(np.float32))
    for r in EMPTY:
        rows[r] = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    csr = (np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32), np.concatenate([c for c, _ in rows]).astype(np.int32),
           np.concatenate([v for _, v in rows]).astype(np.float32))
    deg = np.diff(csr[0])
    want = DEGS + [HUB_DEG if hub else NO_HUB_DEG]
    assert [deg[special_row(k)] for k in range(len(want))] == want and int((deg == 0).sum()) >= 40 and (deg > 1024).any() == hub
    return csr


def handle(csr, packed, **kw):
    """A handle of csr, built normally (packed=True) or under SPEX_PACK_WORDS=0; the switch is read at creation."""
    from spex_amd.graph import SpexGraph
    old = os.environ.get("SPEX_PACK_WORDS")
    if packed:
        os.environ.pop("SPEX_PACK_WORDS", None)
    else:
        os.environ["SPEX_PACK_WORDS"] = "0"
    try:
        return SpexGraph(*csr, **kw)
    finally:
        if old is None:
            os.environ.pop("SPEX_PACK_WORDS", None)
        else:
            os.environ["SPEX_PACK_WORDS"] = old


class Side:
    """One matrix as two handles (packed words / row array), input tables and, on demand, the yardstick's product."""

    def __init__(self, csr, rng, edge_id=None, n_cols=None):
        self.csr, self.edge_id = csr, edge_id
        n = len(csr[0]) - 1
        self.new = handle(csr, True, edge_id=edge_id, n_cols=n_cols)
        self.old = handle(csr, False, edge_id=edge_id, n_cols=n_cols)
        assert self.new.bin_packed and self.new.packed_words and self.old.bin_packed and not self.old.packed_words
        self.Xh = (0.1 * rng.normal(size=(self.new.n_cols, 64))).astype(np.float32)
        self.X = t(self.Xh)
        self.Ah = rng.normal(size=(n, 64)).astype(np.float32)       # epilogue operand
        self.A = t(self.Ah)
        self.keep = t((rng.random(len(csr[1])) < KEEP_PROB).astype(np.uint8))
        self._ref = None

    def both(self):
        return (self.new, self.old)

    def ref(self, O):
        if self._ref is None:
            self._ref = documented_order(O, *self.csr, self.Xh)
        return self._ref


class Fixture:
    def __init__(self, hub, seed):
        from spex_amd.graph import csr_transpose
        rng = np.random.default_rng(seed)
        csr = fixture_csr(hub)
        self.fwd = Side(csr, rng)
        tr = csr_transpose(*csr, N)
        self.tr = Side(tr[:3], rng, edge_id=tr[3])


_fixtures = {}


def fixture_of(hub):
    if hub not in _fixtures:
        _fixtures[hub] = Fixture(hub, 5 if hub else 6)
    return _fixtures[hub]


@pytest.fixture(scope="module")
def fx():
    return fixture_of(True)


@pytest.fixture(scope="module")
def fx_flat():
    return fixture_of(False)


@pytest.fixture(params=["fwd", "tr"])
def side(request, fx):
    return getattr(fx, request.param)


# ------------------------------------------------------------------------------------------------ 1. packed against unpacked
def test_plain_product(side, oracle):
    Y = side.new.spmm(side.X)
    assert torch.equal(Y, side.old.spmm(side.X))
    assert torch.equal(Y, t(side.ref(oracle)))


@pytest.mark.parametrize("div", [1.0, 4.0])
def test_running_sum_form_with_every_output(side, oracle, div):
    out = []
    for g in side.both():
        Y, S = torch.empty_like(side.X), torch.empty_like(side.X)
        g.spmm(side.X, Y=Y, acc_in=side.A, acc_out=S, acc_div=div)
        out.append((Y, S))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    ref = side.ref(oracle)
    assert torch.equal(out[0][0], t(ref)) and torch.equal(out[0][1], t((side.Ah + ref) * np.float32(1.0 / div)))


@pytest.mark.parametrize("div", [1.0, 3.0, 4.0])
def test_add_in_form(side, div):
    a, b = (g.spmm(side.X, add_in=side.A, add_div=div) for g in side.both())
    assert torch.equal(a, b)


def masked(g, side, mode):
    if mode == "keep_mask":
        g.set_edge_mask(1, side.keep, KEEP_PROB)
    else:
        g.set_edge_mask(2, None, KEEP_PROB, seed=0x1234ABCD5678)


@pytest.mark.parametrize("mode", ["keep_mask", "philox"])
@pytest.mark.parametrize("form", ["plain", "acc", "add"])
def test_edge_dropout(side, mode, form):
    out = []
    for g in side.both():
        masked(g, side, mode)
        try:
            if form == "plain":
                out.append(g.spmm(side.X))
            elif form == "acc":
                out.append(g.spmm(side.X, acc_in=side.A, acc_out=torch.empty_like(side.X), acc_div=3.0))
            else:
                out.append(g.spmm(side.X, add_in=side.A, add_div=3.0))
        finally:
            g.set_edge_mask(0)
    assert torch.equal(out[0], out[1])
    if form == "plain":
        assert not torch.equal(out[0], side.new.spmm(side.X))          # (the mask did drop something, and is off again)


@pytest.mark.parametrize("form", ["plain", "acc", "add"])
def test_bf16_gather_table(side, form):
    X16 = side.X.to(torch.bfloat16)
    out = []
    for g in side.both():
        Y, Y16 = torch.empty_like(side.X), torch.empty_like(X16)
        if form == "plain":
            g.spmm_bf16(X16, Y=Y, Y16=Y16)
            out.append((Y, Y16))
        elif form == "acc":
            S = torch.empty_like(side.X)
            g.spmm_bf16(X16, Y=Y, Y16=Y16, acc_in=side.A, acc_out=S, acc_div=4.0)
            out.append((Y, Y16, S))
        else:
            g.spmm_bf16(X16, Y=Y, Y16=Y16, add_in=side.A, add_div=4.0)
            out.append((Y, Y16))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    if form == "plain":                 # (rows beyond 1 024 entries are folded differently by the two kernels)
        short = t(np.diff(side.csr[0]) <= 1024)
        assert torch.equal(out[0][0][short], side.new.spmm(X16.float())[short])


@pytest.mark.parametrize("V", [2, 4])
@pytest.mark.parametrize("mode", [None, "keep_mask"])
def test_wide_kernels_read_the_packed_words_too(side, V, mode):
    """d = 128 / 256 (spmm_chunk_wide_kernel) on the same handles: all three forms, without and with edge dropout."""
    rng = np.random.default_rng(40 + V)
    X = t((0.1 * rng.normal(size=(side.new.n_cols, 64 * V))).astype(np.float32))
    A = t(rng.normal(size=(side.new.n_rows, 64 * V)).astype(np.float32))
    out = []
    for g in side.both():
        if mode:
            masked(g, side, mode)
        try:
            Y, S = torch.empty_like(A), torch.empty_like(A)
            g.spmm(X, Y=Y, acc_in=A, acc_out=S, acc_div=3.0)
            out.append((g.spmm(X), Y, S, g.spmm(X, add_in=A, add_div=4.0)))
        finally:
            g.set_edge_mask(0)
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert bool(torch.isfinite(out[0][0]).all())
    if mode is None:
        assert bool((out[0][0][t(np.diff(side.csr[0]) > 0)] != 0).any(dim=1).all())


@pytest.mark.parametrize("L", [2, 3])
def test_propagate_and_its_backward(fx, L):
    fwd = [g.propagate(fx.fwd.X, L).clone() for g in fx.fwd.both()]
    assert torch.equal(fwd[0], fwd[1])
    bwd = [g.propagate_bwd(fx.fwd.A, L).clone() for g in fx.tr.both()]
    assert torch.equal(bwd[0], bwd[1])
    f16 = [g.propagate(fx.fwd.X, L, gather_dtype=torch.bfloat16).clone() for g in fx.fwd.both()]
    b16 = [g.propagate_bwd(fx.fwd.A, L, gather_dtype=torch.bfloat16).clone() for g in fx.tr.both()]
    assert torch.equal(f16[0], f16[1]) and torch.equal(b16[0], b16[1])
    assert not torch.equal(fwd[0], fx.fwd.X) and bool(torch.isfinite(fwd[0]).all()) and bool(torch.isfinite(bwd[0]).all())


# ------------------------------------------------------------------------------------------------ 2. the 16-bit edge
EDGE_N = 65536


def edge_rows(rng, n_cols):
    """row -> sorted columns: row 65 535 and column 65 535 carry entries, (65 535, 65 535) among them; 200 random short rows."""
    top = EDGE_N - 1
    rows = {top: [0, 5, 4096, top], 0: [7, top], 1000: sorted(set(rng.choice(n_cols, 20, replace=False)) | {top}), 65534: [top]}
    for r in rng.choice(np.arange(1, top - 1), 200, replace=False):
        if int(r) not in rows:
            rows[int(r)] = sorted(rng.choice(EDGE_N, int(rng.integers(1, 71)), replace=False))
    rows[40000] = sorted(rng.choice(EDGE_N, 130, replace=False))          # three segments
    return rows


def csr_of(rows, n_rows, rng):
    deg = np.zeros(n_rows, np.int64)
    for r, c in rows.items():
        deg[r] = len(c)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.concatenate([np.asarray(rows[r], np.int32) for r in sorted(rows)])
    return rowptr, col, rng.uniform(0.05, 0.5, len(col)).astype(np.float32)


@pytest.fixture(scope="module")
def edge():
    rng = np.random.default_rng(65535)
    rows = edge_rows(rng, EDGE_N)
    csr = csr_of(rows, EDGE_N, np.random.default_rng(1))
    new, old = handle(csr, True, n_cols=EDGE_N), handle(csr, False, n_cols=EDGE_N)
    X = t((0.1 * rng.normal(size=(EDGE_N, 64))).astype(np.float32))
    assert X.numel() * 4 == 16 << 20
    top_entry = int(csr[0][EDGE_N]) - 1                                  # (65 535, 65 535): the last stored entry
    assert csr[1][top_entry] == EDGE_N - 1 and np.diff(csr[0])[EDGE_N - 1] == 4
    return rows, csr, new, old, X, top_entry


def test_all_ones_word_packed_equals_unpacked(edge):
    rows, csr, new, old, X, top_entry = edge
    assert new.bin_packed and new.packed_words and old.bin_packed and not old.packed_words
    Y = new.spmm(X)
    assert torch.equal(Y, old.spmm(X))
    top = EDGE_N - 1
    want = torch.zeros(64, device=DEV)
    for c, v in zip(csr[1][csr[0][top]:], csr[2][csr[0][top]:]):
        want = torch.addcmul(want, X[int(c)], torch.tensor(float(v), device=DEV))
    assert torch.allclose(Y[top], want, rtol=1e-5, atol=1e-7) and bool((Y[top] != 0).all())
    empty = torch.ones(EDGE_N, dtype=torch.bool, device=DEV)
    empty[t(np.array(sorted(rows), np.int64))] = False
    assert bool((Y[empty] == 0).all()) and bool((Y[~empty] != 0).any(dim=1).all())
    A = t(np.random.default_rng(2).normal(size=(EDGE_N, 64)).astype(np.float32))
    a, b = (g.spmm(X, acc_in=A, acc_out=torch.empty_like(X), acc_div=4.0) for g in (new, old))
    assert torch.equal(a, b)
    a, b = (g.spmm(X, add_in=A, add_div=3.0) for g in (new, old))
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["top_dropped", "top_kept", "philox"])
def test_all_ones_word_under_edge_dropout(edge, case):
    """The entry whose packed word is 0xFFFFFFFF, dropped (its word must not be taken for a kept one, nor a kept one for dropped:
    the mark lives on the 16-bit source row) and kept, and the Philox draw: equal to the unpacked handle."""
    rows, csr, new, old, X, top_entry = edge
    keep = np.random.default_rng(3).random(len(csr[1])) < KEEP_PROB
    keep[top_entry] = case != "top_dropped"
    keep[top_entry - 1] = case == "top_dropped"
    keep_d = t(keep.astype(np.uint8))
    out = []
    for g in (new, old):
        if case == "philox":
            g.set_edge_mask(2, None, KEEP_PROB, seed=0x5EED)
        else:
            g.set_edge_mask(1, keep_d, KEEP_PROB)
        try:
            out.append(g.spmm(X))
        finally:
            g.set_edge_mask(0)
    assert torch.equal(out[0], out[1])
    if case != "philox":                 # row 65 535 against the kept entries, summed in column order
        top = EDGE_N - 1
        want = torch.zeros(64, device=DEV)
        for e in range(csr[0][top], csr[0][top + 1]):
            if keep[e]:
                want = torch.addcmul(want, X[int(csr[1][e])], torch.tensor(float(np.float32(csr[2][e]) / np.float32(KEEP_PROB)), device=DEV))
        assert torch.allclose(out[0][top], want, rtol=1e-5, atol=1e-7)
        assert not torch.equal(out[0][top], new.spmm(X)[top])


def test_one_node_more_is_not_packed_and_gives_the_same_rows(edge):
    rows, csr, new, old, X, top_entry = edge
    n = EDGE_N + 1
    csr1 = (np.concatenate([csr[0], csr[0][-1:]]).astype(np.int32), csr[1], csr[2])
    g = handle(csr1, True, n_cols=n)
    assert not g.packed_words and not g.bin_packed
    X1 = torch.cat([X, torch.ones(1, 64, device=DEV)])
    Y = g.spmm(X1)
    assert torch.equal(Y[:EDGE_N], new.spmm(X)) and bool((Y[EDGE_N] == 0).all())


def test_too_many_rows_or_columns_report_not_packed():
    """n_cols > 65 536 with few rows: no bin-packed table at all.  More than 65 536 rows over few columns: bin-packed, with the row
    array; its row 69 999 repeats row 5's entries and must repeat its product."""
    rng = np.random.default_rng(8)
    wide = csr_of({0: [1, 70000], 7: [65536, 65537, 99999]}, 10, rng)
    g = handle(wide, True, n_cols=100000)
    assert not g.packed_words and not g.bin_packed
    rows = {int(r): sorted(rng.choice(1000, int(rng.integers(1, 80)), replace=False)) for r in rng.choice(69000, 300, replace=False)}
    rows[5] = sorted(rng.choice(1000, 40, replace=False))
    rows[69999] = rows[5]
    tall = csr_of(rows, 70000, rng)
    b5, b9 = tall[0][5], tall[0][69999]
    tall[2][b9:b9 + 40] = tall[2][b5:b5 + 40]
    g = handle(tall, True, n_cols=1000)
    assert g.bin_packed and not g.packed_words
    X = t((0.1 * rng.normal(size=(1000, 64))).astype(np.float32))
    Y = g.spmm(X)
    assert torch.equal(Y[69999], Y[5]) and bool((Y[5] != 0).all())
    short = handle((tall[0][:65537].copy(), tall[1][:tall[0][65536]], tall[2][:tall[0][65536]]), True, n_cols=1000)
    assert short.packed_words
    assert torch.equal(short.spmm(X), Y[:65536])


# ------------------------------------------------------------------------------------------------ 3. steps
def distinct_triples(rng, T, repeat=False):
    ok_u = np.array([r for r in range(N_U - 1) if r not in EMPTY])
    ok_i = np.array([r for r in range(N_I) if N_U + r not in EMPTY])
    u, it = rng.permutation(ok_u)[:T], rng.permutation(ok_i)[:2 * T]
    if repeat:
        u[1::2] = u[0]
        it[T:] = it[T]
    return t(u.astype(np.int64)), t(it[:T].astype(np.int64)), t(it[T:].astype(np.int64))


@pytest.mark.parametrize("repeat", [False, True])
@pytest.mark.parametrize("L", [2, 3])
def test_fused_bpr_sgd_step(fx_flat, L, repeat, monkeypatch):
    """One step_bpr_sgd at T = 8 on the hub-free fixture: the fused form runs (the sentinel) on both layouts.  Distinct rows: table,
    E^1 and loss bit-equal.  Repeated rows (float atomics in free order): loss 1e-6 relative, table 2e-6."""
    from spex_amd.trainer import LightGCNStepper
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", "1")
    u, p, n = distinct_triples(np.random.default_rng(90 + L), 8, repeat)
    res = []
    for g in fx_flat.fwd.both():
        st = LightGCNStepper(g, fx_flat.fwd.X.clone(), N_U, n_layers=L, lr=0.05)
        loss, fused = one_step(st, u, p, n)
        assert fused is True
        res.append((st.E0.clone(), st.light_out.clone(), loss))
    print("L", L, "repeat", repeat, "loss", res[0][2], res[1][2], "table equal", torch.equal(res[0][0], res[1][0]))
    assert not torch.equal(res[0][0], fx_flat.fwd.X) and torch.equal(res[0][1], res[1][1])
    if repeat:
        assert abs(res[0][2] - res[1][2]) <= 1e-6 * abs(res[1][2])
        assert rel_err(res[0][0].cpu().numpy(), res[1][0].cpu().numpy()) <= 2e-6
    else:
        assert torch.equal(res[0][0], res[1][0]) and res[0][2] == res[1][2]


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("kind", ["bce", "bpr"])
def test_exact_steps(fx_flat, kind, deterministic):
    """One exact BCE step at B = 8 and one exact BPR step at T = 8 (one-call forms) on both layouts.  Fixed-order mode: table, Adam
    moments and loss bit-equal.  Default mode: its backward adds with float atomics in free order, so two runs of ONE layout need
    not agree in the last bit; held to test_gpu_bpr_step_fused_last.py's tolerances instead (loss 1e-6 relative, table 2e-6), and
    the figures are printed."""
    from spex_amd.trainer import LightGCNStepper
    u, p, n = distinct_triples(np.random.default_rng(95), 8)
    labels = t(np.array([1, 0, 1, 1, 0, 0, 1, 0], np.float32))
    res = []
    for g, gt in zip(fx_flat.fwd.both(), fx_flat.tr.both()):
        st = LightGCNStepper(g, fx_flat.fwd.X.clone(), N_U, n_layers=3, lr=1e-3, graph_t=gt, deterministic=deterministic, weight_decay=1e-4)
        acc = torch.zeros(1, device=DEV)
        if kind == "bce":
            st.step_bce(u, p, labels, loss_acc=acc, batch_rows_only=True)
        else:
            st.step_bpr_exact(u, p, n, loss_acc=acc, batch_rows_only=True)
        res.append((st.E0.clone(), st.m.clone(), st.v.clone(), acc.clone()))
    assert not torch.equal(res[0][0], fx_flat.fwd.X) and res[0][3].item() > 0
    err = rel_err(res[0][0].cpu().numpy(), res[1][0].cpu().numpy())
    print(kind, "deterministic", deterministic, "loss", res[0][3].item(), res[1][3].item(), "table rel_err", err,
          "equal", [torch.equal(a, b) for a, b in zip(*res)])
    if deterministic:
        assert all(torch.equal(a, b) for a, b in zip(*res))
    else:
        assert abs(res[0][3].item() - res[1][3].item()) <= 1e-6 * abs(res[1][3].item())
        assert err <= 2e-6


# ------------------------------------------------------------------------------------------------ 4. spex_graph_set_values
def test_set_values_on_a_packed_handle(fx):
    """Fresh handles (the module's shared ones keep their values): new values by edge id, then one product — identity numbering
    and the transpose's permutation."""
    for side in (fx.fwd, fx.tr):
        src = t(np.random.default_rng(12).uniform(0.01, 0.2, len(side.csr[1])).astype(np.float32))
        out = []
        for packed in (True, False):
            g = handle(side.csr, packed, edge_id=side.edge_id)
            assert g.packed_words == packed
            g.set_values(src)
            out.append(g.spmm(side.X))
        assert torch.equal(out[0], out[1]) and not torch.equal(out[0], side.new.spmm(side.X))


# ------------------------------------------------------------------------------------------------ 5. last chunks
def test_last_chunks_of_every_fill(fx, oracle):
    """Segments whose last chunk holds 1, 4, 5, 12, 13 and 16 real entries (rows of 65, 68, 69, 76, 77 and 1 024 entries: 64-entry
    segments, so the last one holds deg - 64 * (nseg - 1)), and packs — a row of exactly 64 entries is a pack of its own with a full
    last chunk, rows of 1, 17 and 63 end packs that first fit fills further: their product is the yardstick's, bit for bit."""
    deg = np.diff(fx.fwd.csr[0])
    last = {int(d): (int(d) - 64 * ((int(d) + 63) // 64 - 1) - 1) % 16 + 1 for d in deg if 64 < d <= 1024}
    assert {last[d] for d in (65, 68, 69, 76, 77, 1024)} == {1, 4, 5, 12, 13, 16}
    assert 64 in deg and {int(d) % 16 for d in deg if 0 < d < 64} == set(range(16))       # short rows of every length modulo a chunk
    S = torch.empty_like(fx.fwd.X)
    Y = fx.fwd.new.spmm(fx.fwd.X, Y=torch.empty_like(fx.fwd.X), acc_in=fx.fwd.A, acc_out=S, acc_div=1.0)
    ref = fx.fwd.ref(oracle)
    assert torch.equal(Y, t(ref)) and torch.equal(S, t(fx.fwd.Ah + ref))
    assert torch.equal(fx.fwd.new.spmm(fx.fwd.X), t(ref))


@pytest.mark.parametrize("which", ["fwd", "tr"])
def test_inf_in_row_0_stays_out_of_rows_that_do_not_read_it(fx, which):
    """Row 0 of the gathered table is +Inf: a row of the product is non-finite exactly when it has a stored entry in column 0 — a
    padded slot never stands on a row the sum does not read — on both layouts, every form, and under dropout with the entry kept."""
    side = getattr(fx, which)
    rowptr, col, _ = side.csr
    reads0 = np.zeros(len(rowptr) - 1, bool)
    reads0[np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))[col == 0]] = True
    assert 2 <= reads0.sum() < len(reads0) // 2
    X = side.X.clone()
    X[0] = float("inf")
    bad = t(reads0)
    for g in side.both():
        S = torch.empty_like(X)
        Y = g.spmm(X, Y=torch.empty_like(X), acc_in=side.A, acc_out=S, acc_div=4.0)
        for out in (g.spmm(X), Y, S, g.spmm(X, add_in=side.A, add_div=4.0), g.spmm_bf16(X.to(torch.bfloat16))):
            finite = torch.isfinite(out).all(dim=1)
            assert torch.equal(finite, ~bad)
        g.set_edge_mask(1, torch.ones_like(side.keep), 1.0)
        try:
            assert torch.equal(torch.isfinite(g.spmm(X)).all(dim=1), ~bad)
        finally:
            g.set_edge_mask(0)
