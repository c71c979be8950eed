"""The d = 64 chunk kernel on the chunk table at implied positions (graph.hip: task k's chunks at chunk k * stride; spmm.hip: the
first super-chunk's metadata requested together with the task record).  Only WHERE the metadata sits and WHEN it is requested
changed, so every product is what it was, bit for bit.

Yardstick: `documented_order`, a restatement of the summation order of DESIGN 4.1 — a row is cut into 64-entry segments, each
segment is one sequential fmaf chain from 0 (the C oracle's spex_oracle_spmm_csr_f32 on a CSR whose rows are the segments), a row's
segments are added in order in float32, and a row beyond 1 024 entries adds its segments in groups of 16, then the groups in order.
The same restatement is bit-equal to the library before this layout (recorded in profiles/implied_positions/).  Every form is also
held, torch.equal, to a handle of the same matrix built with SPEX_PACK_IMPLIED=0 (the dense layout, the kernel's old path).

Shapes, the smallest at which the new positions can go wrong:
  rem    131 users x 300 items, user k with k entries (k = 0 ... 130): tasks of 1 to 4 chunks, partly filled packs, rows of 2 and 3
         segments, a list of rows without entries, null tasks;
  hub    test_gpu_bpr_exact_step.py::hub_graph: rows of 0, 1, 64, 65, 1 100, 1 500 and 2 600 entries (hub groups lead the table);
  weibo  bench.py's Weibo-shaped graph: packs raised above 64 entries, stride above 4, tasks with a second super-chunk.
Each with its transpose as a second handle carrying edge ids (what edge dropout is keyed by)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEEP_PROB = 0.8


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def documented_order(O, rowptr, col, val, X):
    """A X in the summation order of DESIGN 4.1 (see the module docstring)."""
    rowptr = np.asarray(rowptr, np.int64)
    n, deg = len(rowptr) - 1, np.diff(rowptr)
    nseg = (deg + 63) // 64
    first = np.concatenate([[0], np.cumsum(nseg)])
    row_of = np.repeat(np.arange(n), nseg)
    beg = rowptr[row_of] + 64 * (np.arange(first[-1]) - first[row_of])
    end = np.minimum(beg + 64, rowptr[row_of + 1])
    seg_rowptr = np.concatenate([[0], np.cumsum(end - beg)])
    assert seg_rowptr[-1] == rowptr[-1] and np.array_equal(seg_rowptr[:-1], beg)       # the segments tile the entries in order
    P = O.spmm(seg_rowptr.astype(np.int32), col, val, X)
    Y = np.zeros((n, X.shape[1]), np.float32)
    one = nseg == 1
    Y[one] = P[first[:-1][one]]

    def in_order(parts):
        y = parts[0].copy()
        for q in parts[1:]:
            y = y + q
        return y

    for r in np.flatnonzero(nseg > 1):
        parts = P[first[r]:first[r + 1]]
        Y[r] = in_order(parts) if deg[r] <= 1024 else in_order([in_order(parts[k:k + 16]) for k in range(0, len(parts), 16)])
    return Y


def handle(csr, implied, **kw):
    from spex_amd.graph import SpexGraph
    old = os.environ.get("SPEX_PACK_IMPLIED")
    os.environ["SPEX_PACK_IMPLIED"] = "1" if implied else "0"
    try:
        return SpexGraph(*csr, **kw)
    finally:
        if old is None:
            del os.environ["SPEX_PACK_IMPLIED"]
        else:
            os.environ["SPEX_PACK_IMPLIED"] = old


class Side:
    """One matrix as two handles (implied positions / dense layout), an input table and, on demand, the yardstick's product."""

    def __init__(self, csr, rng, edge_id=None):
        self.csr, self.edge_id = csr, edge_id
        n = len(csr[0]) - 1
        self.new = handle(csr, True, edge_id=edge_id)
        self.old = handle(csr, False, edge_id=edge_id)
        self.Xh = (0.1 * rng.normal(size=(n, 64))).astype(np.float32)
        self.X = t(self.Xh)
        self.Ah = rng.normal(size=(n, 64)).astype(np.float32)       # epilogue operand
        self.A = t(self.Ah)
        self.keep = t((rng.random(len(csr[1])) < KEEP_PROB).astype(np.uint8))
        self._ref = None

    def ref(self, O):
        if self._ref is None:
            self._ref = documented_order(O, *self.csr, self.Xh)
        return self._ref


class Shape:
    def __init__(self, csr, n_u, T, seed):
        from spex_amd.graph import csr_transpose
        rng = np.random.default_rng(seed)
        n = len(csr[0]) - 1
        self.n_u, self.T = n_u, T
        self.fwd = Side(csr, rng)
        tr = csr_transpose(*csr, n)
        self.tr = Side(tr[:3], rng, edge_id=tr[3])
        pu, pi = rng.permutation(n_u), rng.permutation(n - n_u)
        self.batch = tuple(t(a.astype(np.int64)) for a in (pu[:T], pi[:T], pi[T:2 * T]))       # distinct rows: <= 1 atomic per element


def rem_csr():
    from spex_amd.graph import lightgcn_norm_adj
    rng = np.random.default_rng(31)
    uu, ii = [], []
    for k in range(131):
        uu += [k] * k
        ii += list(rng.choice(300, k, replace=False))
    csr = lightgcn_norm_adj(np.array(uu), np.array(ii), 130, 300)
    assert list(np.diff(csr[0])[:131]) == list(range(131))
    return csr


def weibo_csr():
    from spex_amd.datasets import synthetic_interactions
    from spex_amd.graph import lightgcn_norm_adj
    u, i = synthetic_interactions(6812, 20000, 400000, seed=7, sigma=1.4)
    return lightgcn_norm_adj(u, i, 6811, 20000)


_shapes = {}


@pytest.fixture(scope="module", params=["rem", "hub", "weibo"])
def shape(request):
    name = request.param
    if name not in _shapes:
        if name == "rem":
            _shapes[name] = Shape(rem_csr(), 131, 64, 1)
        elif name == "hub":
            from test_gpu_bpr_exact_step import hub_graph
            csr, n_u = hub_graph()
            assert sorted(set(np.diff(csr[0])) & {0, 1, 64, 65, 1100, 1500, 2600}) == [0, 1, 64, 65, 1100, 1500, 2600]
            _shapes[name] = Shape(csr, n_u, 100, 2)
        else:
            _shapes[name] = Shape(weibo_csr(), 6812, 200, 3)
    return _shapes[name]


@pytest.fixture(params=["fwd", "tr"])
def side(request, shape):
    return getattr(shape, request.param)


def test_plain_product_is_the_documented_order(side, oracle):
    Y = side.new.spmm(side.X)
    assert torch.equal(Y, t(side.ref(oracle)))
    assert torch.equal(Y, side.old.spmm(side.X))


def test_running_sum_form(side, oracle):
    """acc_out = (acc_in + y) / acc_div, Y = y beside it; a power-of-two divisor against the yardstick, 3 against the dense handle."""
    Y, S = torch.empty_like(side.X), torch.empty_like(side.X)
    side.new.spmm(side.X, Y=Y, acc_in=side.A, acc_out=S, acc_div=4.0)
    ref = side.ref(oracle)
    assert torch.equal(Y, t(ref)) and torch.equal(S, t((side.Ah + ref) * np.float32(0.25)))
    for div in (1.0, 3.0):
        a, b = (g.spmm(side.X, acc_in=side.A, acc_out=torch.empty_like(side.X), acc_div=div) for g in (side.new, side.old))
        assert torch.equal(a, b)
    S1 = side.A.clone()                                   # in place, as the propagation runs it
    side.new.spmm(side.X, acc_in=S1, acc_out=S1, acc_div=1.0)
    assert torch.equal(S1, t(side.Ah + ref))


def test_add_in_form(side, oracle):
    """Y = y + add_in / add_div (the backward of the layer mean)."""
    Y = side.new.spmm(side.X, add_in=side.A, add_div=4.0)
    assert torch.equal(Y, t(side.ref(oracle) + side.Ah * np.float32(0.25)))
    for div in (1.0, 3.0):
        assert torch.equal(side.new.spmm(side.X, add_in=side.A, add_div=div), side.old.spmm(side.X, add_in=side.A, add_div=div))


@pytest.mark.parametrize("mode", ["keep_mask", "philox"])
@pytest.mark.parametrize("form", ["plain", "acc", "add"])
def test_edge_dropout_matches_the_dense_handle(side, mode, form):
    out = []
    for g in (side.new, side.old):
        if mode == "keep_mask":
            g.set_edge_mask(1, side.keep, KEEP_PROB)
        else:
            g.set_edge_mask(2, None, KEEP_PROB, seed=0x1234ABCD5678)
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


@pytest.mark.parametrize("L", [2, 3])
def test_snapshot_tail_launch_through_a_step(shape, L, monkeypatch):
    """One BPR step on the snapshot schedule (the layer-1 launch carries the tail) on a batch of distinct rows: the updated table and
    E^1 are torch.equal between the two layouts; the loss agrees within 1e-6 relative."""
    from spex_amd.trainer import LightGCNStepper
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", "1")
    u, p, n = shape.batch
    res = []
    for g in (shape.fwd.new, shape.fwd.old):
        st = LightGCNStepper(g, shape.fwd.X.clone(), shape.n_u, n_layers=L, lr=0.05)
        loss = st.step_bpr_sgd(u, p, n).item()
        res.append((st.E0.clone(), st.light_out.clone(), loss))
    assert not torch.equal(res[0][0], shape.fwd.X)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert abs(res[0][2] - res[1][2]) <= 1e-6 * abs(res[1][2])
