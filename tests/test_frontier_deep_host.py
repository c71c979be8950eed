"""The inputs of tests/test_gpu_frontier_deep.py, proved in NumPy (no GPU): the sizes of Bset, F1, F2 and F3 — each hop the rows before
it and the columns of their stored (under a mask: stored and kept) entries — for the three batches on graph (b) of
tests/test_gpu_frontier.py, unmasked and under `default_rng(101).random(nnz) < 0.3`, and for the degenerate batch on the hub graph of
tests/test_gpu_stepper_sequences.py, where two hops cover every row."""
import numpy as np
import pytest

import test_gpu_frontier as fmod
import test_gpu_stepper_sequences as seqmod
from test_gpu_frontier import NB, NB_U, batch_b, graph_b

# batch -> (|Bset|, |F1|, |F2|, |F3|) unmasked, (|F1|, |F2|, |F3|) at mask 0.3
TABLE = {("bce", 2, 256): ((506, 3409, 8725, 15088), (1418, 2128, 2802)),
         ("bpr", 3, 256): ((758, 4033, 10068, 15877), (1800, 2670, 3340)),
         ("bce", 1, 7): ((12, 1652, 4816, 11184), (512, 880, 1373))}


def keep_03():
    return (np.random.default_rng(101).random(len(graph_b()[1])) < 0.3).astype(np.uint8)


def rows_of(kind, arrs, n_u):
    return np.concatenate([arrs[0], arrs[1] + n_u] + ([arrs[2] + n_u] if kind == "bpr" else []))


def hop(csr, rows, keep=None):
    """rows U the columns of the stored (keep given: and kept) entries of rows, sorted."""
    rowptr, col = csr[0], csr[1]
    parts = [np.asarray(rows, np.int64)]
    for r in rows:
        c = col[rowptr[r]:rowptr[r + 1]]
        parts.append(c if keep is None else c[keep[rowptr[r]:rowptr[r + 1]] != 0])
    return np.unique(np.concatenate(parts))


def sets3(csr, rows, keep=None):
    """(Bset, F1, F2, F3) as sorted arrays."""
    n = len(csr[0]) - 1
    out = [np.unique(rows[(rows >= 0) & (rows < n)])]
    for _ in range(3):
        out.append(hop(csr, out[-1], keep))
    return tuple(out)


@pytest.mark.parametrize("case", sorted(TABLE))
def test_set_sizes_on_graph_b(case):
    kind, seed, n = case
    csr = graph_b()[:3]
    rows = rows_of(kind, batch_b(kind, seed, n)[1], NB_U)
    plain, masked = sets3(csr, rows), sets3(csr, rows, keep_03())
    assert tuple(len(s) for s in plain) == TABLE[case][0]
    assert len(masked[0]) == TABLE[case][0][0] and tuple(len(s) for s in masked[1:]) == TABLE[case][1]
    deg = np.diff(csr[0])
    long_rows = np.flatnonzero(deg >= 65)
    assert deg[0] == 1500 and sorted(deg[long_rows]) == [65, 100, 128, 129, 200, 1500]
    assert np.isin(long_rows, plain[2]).all()                      # the hub and the rows of 65 - 200 entries are in F2
    assert len(plain[3]) < NB and len(masked[3]) < NB              # "rows outside F3" is never empty
    for a, b in zip(plain[:-1], plain[1:]):
        assert np.isin(a, b).all()
    for m, p in zip(masked, plain):
        assert np.isin(m, p).all()


def test_two_hops_cover_the_hub_graph():
    csr = seqmod.hub_graph()
    kind, arrs = seqmod.bce_batch(30, 17)
    sets = sets3(csr, rows_of(kind, arrs, seqmod.N_U))
    assert (len(sets[1]), len(sets[2]), len(sets[3])) == (2906, 3000, 3000) and seqmod.N == 3000


def test_hop_agrees_with_the_frontier_tests_own_sets():
    csr = graph_b()[:3]
    rows = rows_of("bce", batch_b("bce", 2, 256)[1], NB_U)
    bset, f1 = fmod.frontier_sets(csr, rows)
    mine = sets3(csr, rows)
    assert np.array_equal(bset, mine[0]) and np.array_equal(f1, mine[1])
    from spex_amd import _lib, ops
    assert hasattr(ops.FrontierRows, "expand3") and _lib.STEP_FRONTIER_DEEP == 1024      # what the GPU tests drive with these sets
