"""The fused BPR launch (score.hip: bpr_fused_last_kernel) with its last chunks gathered without padding: a 16-entry chunk issues
loads for its real entries only, four at a time (a wave-uniform count picks one of four straight-line bodies).  The terms left out
were fmaf(0, x, acc); the chain over the real entries is the same, so every row the launch forms is the whole-graph launch's row.

Graph: 131 users x 300 items, user k with k entries (k = 0 ... 130) — every remainder of a row against the 16-entry chunk and the
4-entry quad, rows of 0 to 3 segments.  L = 2 and 3 with SPEX_STEP_SNAPSHOT=1 and SPEX_STEP_FUSED_LAST=1, against the forced
whole-graph form and the reference form (propagate, then ops.bpr_sgd_step(grouped=False)):

  * T = 1, 3, 4, 5, 67: the last workgroup (4 triples) and the last wave of the snapshot tail (64 slots) partly filled;
  * indices out of range in each of the three positions beside valid triples: the skipped triples' rows stay bit-unchanged;
  * an empty batch;
  * further steps on the same stepper with a smaller, then a larger T: the handle's per-step buffers are reused, nothing of the
    earlier, larger batch may be read.

Batches name distinct rows (every table element receives at most one atomic): tables torch.equal, loss within 1e-6 relative."""
import numpy as np
import pytest
import torch

from test_gpu_bpr_fused_last_depth import REM_ITEMS, REM_USERS, check_three_forms, forced_step, reference_step, remainders, t  # noqa: F401

pytestmark = pytest.mark.gpu

SNAP = "1"


def distinct(seed, T):
    rng = np.random.default_rng(seed)
    users, items = rng.permutation(REM_USERS)[:T], rng.permutation(REM_ITEMS)[:2 * T]
    return users, items[:T], items[T:]


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("T", [1, 3, 4, 5, 67])
def test_partial_last_workgroup_and_tail_wave(remainders, L, T, monkeypatch):
    g, E0, n_u = remainders
    u, p, n = distinct(100 + T, T)
    check_three_forms(monkeypatch, g, E0, n_u, L, SNAP, t(u), t(p), t(n), exact=True)


@pytest.mark.parametrize("L", [2, 3])
def test_out_of_range_in_each_position(remainders, L, monkeypatch):
    """Nine triples: 1, 3 and 6 carry a bad user / positive / negative (below the range, one past it, far above it); the other six are
    valid, so workgroups 0 and 1 mix skipped and valid triples and workgroup 2 holds one valid triple."""
    g, E0, n_u = remainders
    u, p, n = distinct(7, 9)
    good = (u.copy(), p.copy(), n.copy())
    u[1], p[3], n[6] = -1, REM_ITEMS, 10 ** 12
    untouched = [int(good[0][k]) for k in (1, 3, 6)] + [n_u + int(good[1][k]) for k in (1, 3, 6)] + [n_u + int(good[2][k]) for k in (1, 3, 6)]
    untouched = [r for r in untouched if 0 <= r < n_u + REM_ITEMS]
    check_three_forms(monkeypatch, g, E0, n_u, L, SNAP, t(u), t(p), t(n), exact=True, unchanged_rows=untouched)


@pytest.mark.parametrize("L", [2, 3])
def test_empty_batch(remainders, L, monkeypatch):
    from spex_amd.trainer import LightGCNStepper
    g, E0, n_u = remainders
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", SNAP)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    st = LightGCNStepper(g, E0.clone(), n_u, n_layers=L, lr=0.05)
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    assert st.step_bpr_sgd(e, e, e).item() == 0.0
    assert torch.equal(st.E0, E0)


@pytest.mark.parametrize("L", [2, 3])
def test_further_steps_with_another_T_on_one_stepper(remainders, L, monkeypatch):
    """T = 67, then 5, then 40 on ONE stepper (one handle: its snapshot buffer and loss cells are grown once and still hold the first
    batch's contents).  The 5-triple step's second workgroup has one triple.  Each step is compared with a fresh whole-graph stepper
    and with the reference form started from the same table."""
    from spex_amd.trainer import LightGCNStepper
    g, E0, n_u = remainders
    monkeypatch.setenv("SPEX_STEP_SNAPSHOT", SNAP)
    monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
    st = LightGCNStepper(g, E0.clone(), n_u, n_layers=L, lr=0.05)
    for k, T in enumerate((67, 5, 40)):
        u, p, n = (t(a) for a in distinct(200 + k, T))
        W = st.E0.clone()
        old, loss_old = forced_step(monkeypatch, g, W, n_u, L, SNAP, False, u, p, n)
        ref, loss_ref = reference_step(g, W, n_u, L, u, p, n)
        monkeypatch.setenv("SPEX_STEP_FUSED_LAST", "1")
        st.loss_acc.zero_()
        loss_new = st.step_bpr_sgd(u, p, n).item()
        print("L", L, "T", T, "loss", loss_new, loss_old, loss_ref, "equal", torch.equal(st.E0, old), torch.equal(st.E0, ref))
        assert not torch.equal(st.E0, W)
        assert torch.equal(st.E0, old) and torch.equal(st.E0, ref)
        assert abs(loss_new - loss_old) <= 1e-6 * abs(loss_old) and abs(loss_new - loss_ref) <= 1e-6 * abs(loss_ref)
