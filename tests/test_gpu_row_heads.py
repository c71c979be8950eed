"""Row heads on the graph handle (graph.hip: head_col / head_val, a fixed-stride copy of every row's first entries) and the fused BPR
launch's static ownership of each slot row's first segment (score.hip: bpr_fused_last_kernel).  With heads, wave j < 12 of a workgroup
requests segment 0 of slot row j at the position the row id implies, in the same round trip as rowptr; the later segments go to waves
12 .. 15, 0, 1, ... round robin.  Only where an entry is read from and which wave sums a segment may differ from the launch without
heads: every segment is still one fmaf chain from 0 in entry order, a row still adds its segments in segment order.

Graph: 230 users x 260 items, random values.  Users 0 .. 11 and items 0 .. 11 have exactly 0, 1, 3, 15, 16, 17, 63, 64, 65, 128, 130 and
200 entries (both sides of the head's 64 entries and of the 16-entry chunk, rows of one to four segments); the other rows are random.
One handle is created with heads, one under SPEX_ROW_HEADS=0 (the switch is read at creation).  Every case runs L = 2 and 3 on both
schedules of the step (SPEX_STEP_SNAPSHOT=0 / 1: the kernel's two instantiations).

  * batches of T = 1, 3, 4, 5, 16, 67 triples whose 3 T rows are distinct (every table element receives one atomic add): E0 after one
    step torch.equal between heads on, heads off and the whole-graph schedule (SPEX_STEP_FUSED_LAST=0); the loss bit for bit between
    the two handles at T <= 16 (one loss cell), within 1e-6 relative beyond that and against the whole-graph schedule;
  * duplicate rows; an out-of-range index; a last workgroup of one valid triple; workgroups of four rows of >= 2 segments each (more
    later segments than waves 12 .. 15) — against the heads-off handle, 2e-6 relative on the table where rows repeat (the atomics'
    order is free; the tolerance of test_gpu_bpr_fused_last_depth.py), torch.equal where they do not, loss 1e-6 relative;
  * after spex_graph_set_values on the handle with heads, the step equals the step on a fresh heads-off handle built from the new
    values (torch.equal): the heads follow the values — on a handle with the identity edge numbering and on one with an edge_id
    permutation (what a transposed copy carries);
  * row 0 of the table the fused launch gathers from set to +Inf: every batch row that does not reference column 0 stays finite, with
    heads, without them and on the whole-graph schedule, and the three agree bit for bit — a padded slot never stands on a row the
    sum does not read."""
import numpy as np
import pytest
import torch

from test_gpu_bpr_fused_last_depth import FORMS, forced_step, rel_err, t
from test_row_heads_host import DEGS, N_ITEMS, N_USERS, make_csr  # noqa: F401

pytestmark = pytest.mark.gpu

N_SPECIAL = len(DEGS)

def handle(monkeypatch, capfd, csr, heads):
    """A SpexGraph created with or without row heads; the packer's own debug line says which it built."""
    import re
    from spex_amd.graph import SpexGraph
    monkeypatch.setenv("SPEX_DEBUG_PACK", "1")
    if heads:
        monkeypatch.delenv("SPEX_ROW_HEADS", raising=False)
    else:
        monkeypatch.setenv("SPEX_ROW_HEADS", "0")
    capfd.readouterr()
    g = SpexGraph(*csr)
    m = re.search(r"row heads (\d+) bytes", capfd.readouterr().err)
    monkeypatch.delenv("SPEX_ROW_HEADS", raising=False)
    monkeypatch.delenv("SPEX_DEBUG_PACK", raising=False)
    assert m and (int(m.group(1)) > 0) == heads, (heads, m and m.group(0))
    return g


class Pair:
    def __init__(self, monkeypatch, capfd):
        self.csr = make_csr()
        self.on = handle(monkeypatch, capfd, self.csr, True)
        self.off = handle(monkeypatch, capfd, self.csr, False)
        self.E0 = t((0.1 * np.random.default_rng(6).normal(size=(N_USERS + N_ITEMS, 64))).astype(np.float32))


_PAIR = []


@pytest.fixture()
def pair(monkeypatch, capfd):
    if not _PAIR:
        _PAIR.append(Pair(monkeypatch, capfd))
    return _PAIR[0]


def distinct(T, seed):
    """T triples of 3 T distinct rows; the special rows come first (rotated by the seed), so every T names some of them."""
    rng = np.random.default_rng(seed)
    users = np.concatenate([np.roll(np.arange(N_SPECIAL), seed), N_SPECIAL + rng.permutation(N_USERS - N_SPECIAL)])[:T]
    items = np.concatenate([np.roll(np.arange(N_SPECIAL), 2 * seed + 1), N_SPECIAL + rng.permutation(N_ITEMS - N_SPECIAL)])[:2 * T]
    return users, items[0::2].copy(), items[1::2].copy()


def both(monkeypatch, pair, L, snap, u, p, n):
    on, loss_on = forced_step(monkeypatch, pair.on, pair.E0, N_USERS, L, snap, True, t(u), t(p), t(n))
    off, loss_off = forced_step(monkeypatch, pair.off, pair.E0, N_USERS, L, snap, True, t(u), t(p), t(n))
    print("L", L, "snapshot", snap, "T", len(u), "loss heads on", loss_on, "off", loss_off, "equal", torch.equal(on, off),
          "rel_err", rel_err(on.cpu().numpy(), off.cpu().numpy()))
    assert not torch.equal(on, pair.E0)
    return on, loss_on, off, loss_off


@pytest.mark.parametrize("L,snap", FORMS)
@pytest.mark.parametrize("T", [1, 3, 4, 5, 16, 67])
def test_heads_on_equals_heads_off_equals_whole_graph(pair, L, snap, T, monkeypatch):
    u, p, n = distinct(T, T)
    assert len(set(u)) == T and len(set(p) | set(n)) == 2 * T
    on, loss_on, off, loss_off = both(monkeypatch, pair, L, snap, u, p, n)
    whole, loss_whole = forced_step(monkeypatch, pair.off, pair.E0, N_USERS, L, snap, False, t(u), t(p), t(n))
    print("loss whole-graph", loss_whole, "equal", torch.equal(on, whole))
    assert torch.equal(on, off) and torch.equal(on, whole) and torch.equal(off, whole)
    if T <= 16:
        assert loss_on == loss_off
    assert abs(loss_on - loss_off) <= 1e-6 * abs(loss_off) and abs(loss_on - loss_whole) <= 1e-6 * abs(loss_whole)


@pytest.mark.parametrize("L,snap", FORMS)
def test_duplicate_rows(pair, L, snap, monkeypatch):
    """The 200- and 130-entry rows in several triples of one workgroup and across workgroups, items repeated as positives and negatives."""
    rng = np.random.default_rng(11)
    u = rng.choice(np.arange(N_SPECIAL), 24)
    u[[0, 1, 2, 3, 7, 20]] = 11
    u[[4, 5]] = 10
    items = np.concatenate([np.arange(N_SPECIAL), rng.choice(np.arange(N_SPECIAL, N_ITEMS), 6)])
    p, n = rng.choice(items, 24), rng.choice(items, 24)
    on, loss_on, off, loss_off = both(monkeypatch, pair, L, snap, u, p, n)
    assert rel_err(on.cpu().numpy(), off.cpu().numpy()) <= 2e-6
    assert abs(loss_on - loss_off) <= 1e-6 * abs(loss_off)


@pytest.mark.parametrize("L,snap", FORMS)
def test_out_of_range_index_and_last_workgroup_of_one_valid_triple(pair, L, snap, monkeypatch):
    """Nine triples of distinct rows: triples 1, 3 and 6 carry a bad user / positive / negative (skipped: their rows stay bit-unchanged
    on both handles, their waves own no head), so workgroups 0 and 1 mix skipped and valid triples; workgroup 2 holds one valid triple."""
    u, p, n = distinct(9, 3)
    good = (u.copy(), p.copy(), n.copy())
    u[1], p[3], n[6] = -1, N_ITEMS, 10 ** 12
    on, loss_on, off, loss_off = both(monkeypatch, pair, L, snap, u, p, n)
    assert torch.equal(on, off)
    assert abs(loss_on - loss_off) <= 1e-6 * abs(loss_off)
    for k in (1, 3, 6):
        for r in (int(good[0][k]), N_USERS + int(good[1][k]), N_USERS + int(good[2][k])):
            assert torch.equal(on[r], pair.E0[r]) and torch.equal(off[r], pair.E0[r])


@pytest.mark.parametrize("L,snap", FORMS)
def test_more_later_segments_than_waves_12_to_15(pair, L, snap, monkeypatch):
    """Two workgroups whose triples name the rows of 65, 128, 130 and 200 entries on both sides (users as users, items as positives) and
    short rows as negatives: 2 + 2 + 3 + 4 segments per side, 14 later segments per workgroup behind the 12 first ones — one each for
    waves 12 .. 15 and, behind their own row's head, waves 0 .. 9.  (Waves that take several later segments: the 1 024-entry rows of
    test_gpu_bpr_fused_last_depth.py, which run with heads as well.)  Workgroup 1 names the same rows in another order: duplicates, so
    the table is compared with the atomics' tolerance."""
    big = np.array([8, 9, 10, 11])
    u = np.concatenate([big, big[::-1]])
    p = np.concatenate([big, np.roll(big, 1)])
    n = np.array([1, 2, 3, 4, 5, 6, 7, 0])
    on, loss_on, off, loss_off = both(monkeypatch, pair, L, snap, u, p, n)
    assert rel_err(on.cpu().numpy(), off.cpu().numpy()) <= 2e-6
    assert abs(loss_on - loss_off) <= 1e-6 * abs(loss_off)
    # the first workgroup alone: distinct rows, bit for bit
    on, loss_on, off, loss_off = both(monkeypatch, pair, L, snap, u[:4], p[:4], n[:4])
    assert torch.equal(on, off) and loss_on == loss_off


@pytest.mark.parametrize("L,snap", FORMS)
def test_heads_follow_a_value_rewrite(L, snap, monkeypatch, capfd):
    """set_values on a handle with heads, then one step: equal to a fresh heads-off handle created from the new values — and not to the
    step with the old ones."""
    rowptr, col, val = make_csr()
    new_val = (val[::-1] * np.float32(0.75)).copy()
    g_on = handle(monkeypatch, capfd, (rowptr, col, val), True)
    g_on.set_values(t(new_val))
    g_off = handle(monkeypatch, capfd, (rowptr, col, new_val), False)
    g_old = handle(monkeypatch, capfd, (rowptr, col, val), False)
    E0 = t((0.1 * np.random.default_rng(8).normal(size=(N_USERS + N_ITEMS, 64))).astype(np.float32))
    u, p, n = (t(a) for a in distinct(16, 2))
    on, loss_on = forced_step(monkeypatch, g_on, E0, N_USERS, L, snap, True, u, p, n)
    off, loss_off = forced_step(monkeypatch, g_off, E0, N_USERS, L, snap, True, u, p, n)
    old, _ = forced_step(monkeypatch, g_old, E0, N_USERS, L, snap, True, u, p, n)
    print("L", L, "snapshot", snap, "loss", loss_on, loss_off, "equal", torch.equal(on, off), "old values equal", torch.equal(on, old))
    assert torch.equal(on, off) and loss_on == loss_off
    assert not torch.equal(on, old)


@pytest.mark.parametrize("L,snap", FORMS)
def test_heads_follow_a_value_rewrite_through_edge_ids(L, snap, monkeypatch, capfd):
    """The same with an edge_id permutation on the handle: entry e takes src[edge_id[e]]."""
    import re
    from spex_amd.graph import SpexGraph
    rowptr, col, val = make_csr()
    perm = np.random.default_rng(9).permutation(len(col)).astype(np.int32)
    src = (np.random.default_rng(10).uniform(0.05, 1.0, len(col))).astype(np.float32)
    monkeypatch.setenv("SPEX_DEBUG_PACK", "1")
    monkeypatch.delenv("SPEX_ROW_HEADS", raising=False)
    capfd.readouterr()
    g_on = SpexGraph(rowptr, col, val, edge_id=perm)
    m = re.search(r"row heads (\d+) bytes", capfd.readouterr().err)
    monkeypatch.delenv("SPEX_DEBUG_PACK", raising=False)
    assert m and int(m.group(1)) > 0
    g_on.set_values(t(src))
    g_off = handle(monkeypatch, capfd, (rowptr, col, src[perm]), False)
    E0 = t((0.1 * np.random.default_rng(8).normal(size=(N_USERS + N_ITEMS, 64))).astype(np.float32))
    u, p, n = (t(a) for a in distinct(16, 2))
    on, loss_on = forced_step(monkeypatch, g_on, E0, N_USERS, L, snap, True, u, p, n)
    off, loss_off = forced_step(monkeypatch, g_off, E0, N_USERS, L, snap, True, u, p, n)
    print("L", L, "snapshot", snap, "loss", loss_on, loss_off, "equal", torch.equal(on, off))
    assert torch.equal(on, off) and loss_on == loss_off


@pytest.mark.parametrize("snap", ["0", "1"])
def test_inf_in_row_0_of_the_gathered_table_stays_out_of_rows_that_do_not_read_it(snap, monkeypatch, capfd):
    """User 0 and item 0 are each other's only neighbour and E0[item 0] = +Inf, so at L = 2 the table the last layer gathers from, E^1,
    holds +Inf in row 0 and nowhere else, and item 0's row is the only one that references column 0.  A batch of 16 distinct rows
    that names neither (users and items of 1, 3, 15, 17, 63, 65, 130, 200 ... entries: last quads with one to three padded slots, with
    and without a tail behind the head) must come out finite on all three forms, and equal."""
    csr = make_csr(link00=True)
    g_on, g_off = handle(monkeypatch, capfd, csr, True), handle(monkeypatch, capfd, csr, False)
    E0h = (0.1 * np.random.default_rng(12).normal(size=(N_USERS + N_ITEMS, 64))).astype(np.float32)
    E0h[N_USERS] = np.inf
    E0 = t(E0h)
    E1 = g_off.spmm(E0)
    assert bool(torch.isinf(E1[0]).all()) and bool(torch.isfinite(E1[1:N_USERS]).all()) and bool(torch.isfinite(E1[N_USERS + 1:]).all())
    u, p, n = distinct(17, 4)
    keep = (u != 0) & (p != 0) & (n != 0)
    u, p, n = u[keep][:16], p[keep][:16], n[keep][:16]
    assert len(u) == 16 and set(range(1, 12)) <= set(u) and len(set(range(1, 12)) & (set(p) | set(n))) >= 9
    rows = torch.cat([t(u), N_USERS + t(p), N_USERS + t(n)])
    out = [forced_step(monkeypatch, g, E0, N_USERS, 2, snap, fused, t(u), t(p), t(n)) for g, fused in ((g_on, True), (g_off, True), (g_off, False))]
    for (W, loss), name in zip(out, ("heads on", "heads off", "whole graph")):
        print(name, "snapshot", snap, "loss", loss, "finite batch rows", bool(torch.isfinite(W[rows]).all()), "nan anywhere", bool(torch.isnan(W).any()))
        assert bool(torch.isfinite(W[rows]).all()) and not bool(torch.isnan(W).any()) and np.isfinite(loss), name
        assert not torch.equal(W[rows], E0[rows])
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][0], out[2][0])
    assert out[0][1] == out[1][1]
