"""The scoring, BPR, owner-exchange and trust-head launches past every bounded grid's first pass, each against a
plain fp64 restatement of the same operation.  The inputs are those of tests/test_large_steps_host.py, which proves in NumPy that
they cross the caps: B = 65 553 samples and K = 70 001 positions against grid_for's 32 768 waves (three trips), T = 536 633 triples
against 32 768 waves x 16 triples, 40 000 users against trust_reduce_kernel's 1 024 blocks x 4 rows (ten trips) and the split sweep.

Part A compares kernels alone.  The gates are the project's figures for these kernels (tests/test_gpu_kernels.py: gamma 1e-6, mean
loss 1e-6, gradient and updated tables 1e-5; the trust head: 2e-5, tests/test_gpu_dropin.py), each widened only to 4 x the distance of
the same restatement in fp32 from the fp64 truth where that is larger (`gate`, the rule of tests/test_gpu_stepper_sequences.py::
bounds_of); every figure is printed beside its yardstick and bound before it is asserted.  Bit-for-bit claims (the gather, repeats
on one workspace, untouched rows, sentinels behind every output) use torch.equal.

Measured on an MI355X (the fp32 restatement in brackets): score_bce gamma 9.3e-8 (1.5e-7), mean loss <= 4.5e-7 (1.9e-6), gradient
tables and slots <= 5.9e-7 (5.6e-7); scatter 1.5e-7 (1.4e-7); BPR mean loss <= 1.1e-6 (5e-6 .. 1.5e-5), SGD tables <= 3.3e-6 (4e-8:
the kernel adds each triple into the fp32 table, the restatement adds the summed update once), gradient tables <= 1.4e-6 (1.8e-6);
trust head <= 2.9e-6 (d scores; 3.5e-6), the other quantities <= 1.0e-6.  The module runs in 5.5 s.  More, and the sensitivity runs:
DESIGN.md 4.29.

Not reachable alone: the per-sample-loss form of score_bce_kernel (spex::score_bce_slots_rows) has no entry in the C ABI; it runs
inside the partitioned dual-task steps only.  The dual-task, NGCF and headline BPR-SGD one-call steps on graph (e) are not
tested here: DESIGN.md 4.29 names them as the follow-up; the host module already carries their inputs.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_gpu_stepper_sequences import rel_err, t
from test_large_steps_host import (BPR_I, BPR_T, BPR_U, OWNED_K, OWNED_LO, OWNED_LOCAL, SCORE_B, SCORE_BAD, SCORE_I, SCORE_U,
                                   TRUST_SHAPES, TRUST_USERS, bpr_in_range, bpr_triples, owned_positions, score_inputs, trust_paths)

pytestmark = pytest.mark.gpu

SENT = 12345.0
TAIL = 1000                 # every output is this many elements too long; the tail must come back untouched
torch.set_num_threads(min(16, torch.get_num_threads()))


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def gate(label, fig, project, fig32):
    """Print the kernel's figure beside the fp32 restatement's and the bound in force, then assert."""
    bound = max(project, 4.0 * fig32)
    print(f"{label}: {fig:.2e} (fp32 {fig32:.2e}, bound {bound:.2e})")
    assert fig <= bound, f"{label}: {fig:.3e} > {bound:.3e}"


def padded(n, fill=SENT):
    """(a flat device buffer of n + TAIL elements filled with `fill`, its first n elements)."""
    buf = torch.full((n + TAIL,), fill, dtype=torch.float32, device=dev())
    return buf, buf[:n]


def tail_untouched(buf, n, fill=SENT):
    return bool((buf[n:] == fill).all())


def incidence(idx, n_rows):
    """S [n_rows, len(idx)] with S[idx[k], k] = 1: S @ rows sums the rows per destination (fp64: an exact scatter)."""
    k = len(idx)
    return sp.csr_matrix((np.ones(k), (idx, np.arange(k))), shape=(n_rows, k))


def running_sum(x):
    """The sum of x taken term by term in x's own type, as a plain loop would: in fp32 the yardstick of a loss SUM accumulated in
    fp32 (n partial sums of magnitude up to S carry about sqrt(n) ulp(S) / sqrt(12) of rounding, which a pairwise sum would hide)."""
    return np.cumsum(x, dtype=x.dtype)[-1]


# ================================================================================================ A.1 scoring
def score_closed_form(d, dtype):
    users, items, u, i, y = score_inputs(d)
    ok = (u >= 0) & (u < SCORE_U) & (i >= 0) & (i < SCORE_I)
    U, I, yy = users.astype(dtype), items.astype(dtype), y.astype(dtype)[ok]
    pu, pi = U[u[ok]], I[i[ok]]
    x = (pu * pi).sum(1, dtype=dtype)
    bce = np.maximum(x, 0) - x * yy + np.log1p(np.exp(-np.abs(x)))
    dg = ((1 / (1 + np.exp(-x)) - yy) * dtype(1.0 / SCORE_B))[:, None]
    su, si = dg * pi, dg * pu
    slots = np.zeros((2 * SCORE_B, d), dtype)
    slots[:SCORE_B][ok], slots[SCORE_B:][ok] = su, si
    rows = np.zeros(SCORE_B, dtype)
    rows[ok] = bce
    return {"ok": ok, "gamma": x, "loss": running_sum(bce) / SCORE_B, "loss_rows": rows, "slots": slots,
            "gu": (incidence(u[ok], SCORE_U).astype(dtype) @ su), "gi": (incidence(i[ok], SCORE_I).astype(dtype) @ si)}


@pytest.fixture(scope="module")
def score_truth():
    cache = {}

    def get(d):
        if d not in cache:
            want, f32 = score_closed_form(d, np.float64), score_closed_form(d, np.float32)
            cache[d] = (want, {q: (abs(float(f32[q]) - float(want[q])) if q == "loss" else rel_err(f32[q], want[q]))
                               for q in ("gamma", "loss", "slots", "gu", "gi")})
        return cache[d]
    return get


@pytest.mark.parametrize("d", [64, 100])
def test_score_bce_three_trips_vs_fp64(score_truth, d):
    """spex_score_bce_f32 over B = 2 x 32 768 + 17 samples: gamma, the loss sum and both atomically accumulated gradient tables
    against fp64; gamma is NaN exactly at the three out-of-range samples (one per trip of the grid); every output's tail of 1 000
    sentinels comes back untouched."""
    from spex_amd.graph import _launch, _ptr
    want, f32 = score_truth(d)
    users, items, u, i, y = score_inputs(d)
    ok = want["ok"]
    gamma_buf, gamma = padded(SCORE_B)
    loss_buf, loss = padded(1)
    loss.zero_()
    gu_buf, gu = padded(SCORE_U * d)
    gi_buf, gi = padded(SCORE_I * d)
    gu.zero_(), gi.zero_()
    U, I, ud, idd, yd = t(users), t(items), t(u), t(i), t(y)
    _launch(dev(), "spex_score_bce_f32", _ptr(U), _ptr(I), d, d, SCORE_U, SCORE_I, _ptr(ud), _ptr(idd), _ptr(yd), SCORE_B, d, _ptr(gamma),
            _ptr(loss), _ptr(gu), _ptr(gi), 1.0 / SCORE_B)
    g = gamma.cpu().numpy()
    assert np.isnan(g[list(SCORE_BAD)]).all() and not np.isnan(g[ok]).any() and (~ok).sum() == len(SCORE_BAD)
    tag = f"score_bce d={d}"
    gate(f"{tag} gamma", rel_err(g[ok], want["gamma"]), 1e-6, f32["gamma"])
    gate(f"{tag} mean loss", abs(loss.item() / SCORE_B - want["loss"]), 1e-6, f32["loss"])
    gate(f"{tag} grad_users", rel_err(gu.view(SCORE_U, d).cpu().numpy(), want["gu"]), 1e-5, f32["gu"])
    gate(f"{tag} grad_items", rel_err(gi.view(SCORE_I, d).cpu().numpy(), want["gi"]), 1e-5, f32["gi"])
    for name, buf, n in (("gamma", gamma_buf, SCORE_B), ("loss_sum", loss_buf, 1), ("grad_users", gu_buf, SCORE_U * d), ("grad_items", gi_buf, SCORE_I * d)):
        assert tail_untouched(buf, n), name
    # scores only (no labels): the same gamma bit for bit, NaN at the same places
    gamma2_buf, gamma2 = padded(SCORE_B)
    _launch(dev(), "spex_score_bce_f32", _ptr(U), _ptr(I), d, d, SCORE_U, SCORE_I, _ptr(ud), _ptr(idd), None, SCORE_B, d, _ptr(gamma2),
            None, None, None, 0.0)
    assert torch.equal(gamma2[t(ok)], gamma[t(ok)]) and torch.isnan(gamma2[t(~ok)]).all() and tail_untouched(gamma2_buf, SCORE_B)


@pytest.mark.parametrize("d", [64, 100])
def test_score_bce_slots_three_trips_vs_fp64(score_truth, d):
    """spex_score_bce_slots_f32: both halves of grad_slots (row b: the sample's user-side row, row B + b its item-side row) against
    fp64, the rows of the out-of-range samples exactly zero in both halves, the gradient tables and the loss sum as above, the slot
    buffer's tail untouched."""
    from spex_amd import ops
    want, f32 = score_truth(d)
    users, items, u, i, y = score_inputs(d)
    extra = -(-TAIL // d)
    slots = torch.full((2 * SCORE_B + extra, d), SENT, device=dev())
    gu_buf, gu = padded(SCORE_U * d)
    gi_buf, gi = padded(SCORE_I * d)
    gu.zero_(), gi.zero_()
    loss_buf, loss = padded(1)
    loss.zero_()
    none, out = ops.score_bce(t(users), t(items), t(u), t(i), t(y), gu.view(SCORE_U, d), gi.view(SCORE_I, d), 1.0 / SCORE_B, loss_sum=loss,
                              grad_slots=slots)
    assert none is None and out is loss
    got = slots[:2 * SCORE_B].cpu().numpy()
    tag = f"score_bce_slots d={d}"
    gate(f"{tag} user half", rel_err(got[:SCORE_B], want["slots"][:SCORE_B]), 1e-5, f32["slots"])
    gate(f"{tag} item half", rel_err(got[SCORE_B:], want["slots"][SCORE_B:]), 1e-5, f32["slots"])
    for b in SCORE_BAD:
        assert not got[b].any() and not got[SCORE_B + b].any(), b
    assert np.count_nonzero(np.abs(got).max(1)) == 2 * (SCORE_B - len(SCORE_BAD))            # every other slot row was written
    gate(f"{tag} mean loss", abs(loss.item() / SCORE_B - want["loss"]), 1e-6, f32["loss"])
    gate(f"{tag} grad_users", rel_err(gu.view(SCORE_U, d).cpu().numpy(), want["gu"]), 1e-5, f32["gu"])
    gate(f"{tag} grad_items", rel_err(gi.view(SCORE_I, d).cpu().numpy(), want["gi"]), 1e-5, f32["gi"])
    assert bool((slots[2 * SCORE_B:] == SENT).all())
    assert tail_untouched(gu_buf, SCORE_U * d) and tail_untouched(gi_buf, SCORE_I * d) and tail_untouched(loss_buf, 1)


# ================================================================================================ A.2 owner exchange
@pytest.mark.parametrize("d", [64, 100])
def test_gather_owned_rows_three_trips_bit_for_bit(d):
    """spex_gather_owned_rows_f32 over K = 70 001 positions: out[k] is the table row where the window owns the position and zero
    elsewhere, bit for bit; the tail behind out is untouched."""
    from spex_amd import ops
    pos = owned_positions()
    table = np.random.default_rng(44).standard_normal((OWNED_LOCAL, d), dtype=np.float32)
    own = (pos >= OWNED_LO) & (pos < OWNED_LO + OWNED_LOCAL)
    want = np.zeros((OWNED_K, d), np.float32)
    want[own] = table[pos[own] - OWNED_LO]
    buf, out = padded(OWNED_K * d)
    ops.gather_owned_rows(t(table), t(pos), OWNED_LO, out.view(OWNED_K, d))
    assert torch.equal(out.view(OWNED_K, d).cpu(), torch.from_numpy(want)) and tail_untouched(buf, OWNED_K * d)


@pytest.mark.parametrize("d,clear", [(64, True), (64, False), (100, True), (100, False)])
def test_scatter_add_owned_rows_three_trips_vs_fp64(d, clear):
    """spex_scatter_add_owned_rows_f32: table[pos[k] - lo] += upd[k] against an fp64 scatter, rows no owned position names bit for
    bit as before, guards of 1 000 sentinels on either side of the shard untouched (a position outside the window writes nowhere);
    upd cleared to its last float under clear_upd, else untouched."""
    from spex_amd import ops
    pos = owned_positions()
    rng = np.random.default_rng(45)
    base = rng.standard_normal((OWNED_LOCAL, d), dtype=np.float32)
    upd = rng.standard_normal((OWNED_K, d), dtype=np.float32)
    own = (pos >= OWNED_LO) & (pos < OWNED_LO + OWNED_LOCAL)
    S = incidence(pos[own] - OWNED_LO, OWNED_LOCAL)
    want = base.astype(np.float64) + S @ upd[own].astype(np.float64)
    f32 = rel_err(base + (S.astype(np.float32) @ upd[own]), want)
    n = OWNED_LOCAL * d
    shard_buf = torch.full((TAIL + n + TAIL,), SENT, device=dev())
    shard = shard_buf[TAIL:TAIL + n].view(OWNED_LOCAL, d)
    shard.copy_(t(base))
    upd_buf, upd_d = padded(OWNED_K * d)
    upd_d.copy_(t(upd).reshape(-1))
    ops.scatter_add_owned_rows(upd_d.view(OWNED_K, d), t(pos), OWNED_LO, shard, clear=clear)
    got = shard.cpu().numpy()
    gate(f"scatter_add_owned_rows d={d} clear={clear}", rel_err(got, want), 1e-5, f32)
    unnamed = np.setdiff1d(np.arange(OWNED_LOCAL), pos[own] - OWNED_LO)
    assert len(unnamed) > 100 and np.array_equal(got[unnamed], base[unnamed])
    assert bool((shard_buf[:TAIL] == SENT).all()) and bool((shard_buf[TAIL + n:] == SENT).all())
    if clear:
        assert not upd_d.any()
    else:
        assert torch.equal(upd_d.cpu(), torch.from_numpy(upd).reshape(-1))
    assert tail_untouched(upd_buf, OWNED_K * d)


# ================================================================================================ A.3 BPR, the atomic form
BPR_LR, BPR_REG = 50.0, 1e-3      # lr: the step moves the tables by ~6e-3 of their maximum, so that the second pass's 2.3 % of the
                                   # triples (1.4e-4) stand far above the 1e-5 gate; at lr 0.5 they would move it by 1.4e-6 and hide below it


def bpr_tables():
    rng = np.random.default_rng(46)
    return (0.2 * rng.standard_normal((BPR_U, 64))).astype(np.float32), (0.2 * rng.standard_normal((BPR_I, 64))).astype(np.float32)


def bpr_closed_form(shuffled, dtype):
    """oracle/spex_oracle.c: spex_oracle_bpr_sgd_f64 (batch-synchronous: scores from the tables as read, every update scaled by
    1 / T) over the triples in range, as three incidence-matrix products; and the gradient of the mean loss (reg = 0)."""
    Ut, It = bpr_tables()
    u, p, n = bpr_triples(shuffled)
    ok = bpr_in_range(u, p, n)
    u, p, n = u[ok], p[ok], n[ok]
    U, I = Ut.astype(dtype), It.astype(dtype)
    uu, diff = U[u], I[n] - I[p]
    x = (uu * diff).sum(1, dtype=dtype)
    loss = running_sum(np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))) / BPR_T
    s = ((1 / (1 + np.exp(-x))) / dtype(BPR_T))[:, None]
    Su, Sp, Sn = (incidence(idx, rows).astype(dtype) for idx, rows in ((u, BPR_U), (p, BPR_I), (n, BPR_I)))
    gu, su = Su @ (s * diff), s * uu
    gi = Sn @ su - Sp @ su
    r = dtype(BPR_REG / BPR_T)
    return {"loss": loss, "gu": gu, "gi": gi, "U": U - dtype(BPR_LR) * (gu + r * (Su @ uu)),
            "I": I - dtype(BPR_LR) * (gi + r * (Sp @ I[p] + Sn @ I[n]))}


@pytest.fixture(scope="module")
def bpr_truth():
    cache = {}

    def get(shuffled):
        if shuffled not in cache:
            want, f32 = bpr_closed_form(shuffled, np.float64), bpr_closed_form(shuffled, np.float32)
            cache[shuffled] = (want, {q: (abs(float(f32[q]) - float(want[q])) if q == "loss" else rel_err(f32[q], want[q])) for q in want})
        return cache[shuffled]
    return get


@pytest.mark.parametrize("order", ["sampler", "shuffled"])
def test_bpr_atomic_form_past_sixteen_triples_per_wave_vs_fp64(bpr_truth, order):
    """spex_bpr_sgd_step_f32 and spex_bpr_loss_f32 (the atomic form, forced) over T = 524 288 + 12 345 triples: 33 540 waves of 16
    consecutive triples against a grid of 32 768; the five out-of-range triples sit in the second pass and are skipped.  The loss,
    both updated tables and both gradient tables against the closed form in fp64; the tables' tails untouched."""
    from spex_amd import ops
    want, f32 = bpr_truth(order == "shuffled")
    Ut, It = bpr_tables()
    u, p, n = (t(x) for x in bpr_triples(order == "shuffled"))
    Uw_buf, Uw = padded(BPR_U * 64)
    Iw_buf, Iw = padded(BPR_I * 64)
    Uw.copy_(t(Ut).reshape(-1)), Iw.copy_(t(It).reshape(-1))
    loss = ops.bpr_sgd_step(t(Ut), t(It), Uw.view(BPR_U, 64), Iw.view(BPR_I, 64), u, p, n, lr=BPR_LR, reg=BPR_REG, grouped=False)
    tag = f"bpr {order}"
    gate(f"{tag} sgd mean loss", abs(loss.item() / BPR_T - want["loss"]), 1e-6, f32["loss"])
    gate(f"{tag} sgd users", rel_err(Uw.view(BPR_U, 64).cpu().numpy(), want["U"]), 1e-5, f32["U"])
    gate(f"{tag} sgd items", rel_err(Iw.view(BPR_I, 64).cpu().numpy(), want["I"]), 1e-5, f32["I"])
    moved = rel_err(want["U"], Ut)
    assert moved >= 1e-3, moved                                        # the update is far above the gate: a skipped pass would show
    assert tail_untouched(Uw_buf, BPR_U * 64) and tail_untouched(Iw_buf, BPR_I * 64)
    gu_buf, gu = padded(BPR_U * 64)
    gi_buf, gi = padded(BPR_I * 64)
    gu.zero_(), gi.zero_()
    loss = ops.bpr_loss_grad(t(Ut), t(It), u, p, n, gu.view(BPR_U, 64), gi.view(BPR_I, 64), 1.0 / BPR_T, grouped=False)
    gate(f"{tag} loss_grad mean loss", abs(loss.item() / BPR_T - want["loss"]), 1e-6, f32["loss"])
    gate(f"{tag} grad_users", rel_err(gu.view(BPR_U, 64).cpu().numpy(), want["gu"]), 1e-5, f32["gu"])
    gate(f"{tag} grad_items", rel_err(gi.view(BPR_I, 64).cpu().numpy(), want["gi"]), 1e-5, f32["gi"])
    assert tail_untouched(gu_buf, BPR_U * 64) and tail_untouched(gi_buf, BPR_I * 64)
    # the loss alone (no gradient tables: one triple per wave, 17 passes of the grid)
    loss1 = ops.bpr_loss_grad(t(Ut), t(It), u, p, n)
    gate(f"{tag} loss alone", abs(loss1.item() / BPR_T - want["loss"]), 1e-6, f32["loss"])


# ================================================================================================ A.4 the trust head on 40 000 users
PREFILL = 2.0 ** -12        # grad_table is added into: small against the gradients' rounding, exact to subtract


def trust_inputs(T, L, H):
    from spex_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(100 * T + L)
    table = torch.rand(TRUST_USERS + 1, 64, generator=gen) * 0.6 - 0.3
    params = torch.rand(ops.trust_param_count(H, 64), generator=gen) * 0.4 - 0.2
    return (table, params) + trust_paths(TRUST_USERS, T, L, 70 + T + L)


def trust_head_restated(table, flat, seq, lens, targets, H, dtype):
    """The trust head's part of oracle.trust_oracle.dual_task_losses (its lines after loss1) on the flat parameter block of
    include/spex_hip.h, under autograd in `dtype`: the loss, per-path losses, a2, d loss / d scores and both gradients."""
    from oracle.trust_oracle import path_attention
    F = torch.nn.functional
    d = 64
    tab, par = table.to(dtype).requires_grad_(True), flat.to(dtype).requires_grad_(True)
    at = [0]

    def take(*shape):
        k = int(np.prod(shape))
        x = par[at[0]:at[0] + k].view(*shape)
        at[0] += k
        return x
    a_in = [take(2 * d) for _ in range(H)]
    a_out, w = take(2 * d), take(H * d, d)
    W1, b1, W2, b2, w3, Wt, bt, att_t = take(d, d), take(d), take(d, d), take(d), take(1, d), take(d, 2 * d), take(d), take(2 * d, 2)
    assert at[0] == par.numel()
    seq, lens, targets = torch.from_numpy(seq), torch.from_numpy(lens), torch.from_numpy(targets)
    T, L = seq.shape
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(dtype)
    mul_seq = torch.cat([path_attention(tab, seq, lens, a, True) for a in a_in], dim=2)
    mul_one = F.elu(mul_seq.reshape(-1, H * d) @ w)
    hidden = path_attention(None, mul_one.view(T, L, d), lens, a_out, False)
    ht = hidden[torch.arange(T), lens - 1]
    q1 = (ht @ W1.t() + b1).view(T, 1, -1)
    q2 = hidden @ W2.t() + b2
    alpha = torch.sigmoid(q1 + q2) @ w3.t()
    a = (alpha * hidden * mask.view(T, -1, 1)).sum(1)
    p_a = torch.cat([a, ht], 1) @ Wt.t() + bt
    p_max = (tab[seq] * mask.unsqueeze(2)).max(dim=1)[0]
    att = torch.softmax(torch.cat([p_a, p_max], 1) @ att_t, 1)
    a2 = p_a * att[:, :1] + p_max * att[:, 1:2]
    scores = a2 @ tab[:-1].t()
    scores.retain_grad()
    loss_b = F.cross_entropy(scores, targets, reduction="none")
    loss = loss_b.mean()
    loss.backward()
    return {"loss": np.array([loss.item()]), "path losses": loss_b.detach().numpy(), "a2": a2.detach().numpy(), "dscore": scores.grad.numpy(),
            "grad params": par.grad.numpy(), "grad table": tab.grad.numpy()}


TRUST_Q = ("loss", "path losses", "a2", "dscore", "grad params", "grad table")


@pytest.mark.parametrize("T,L,H", TRUST_SHAPES)
def test_trust_head_train_on_40000_users_vs_fp64(monkeypatch, T, L, H):
    """spex_trust_head_train_f32 on a 40 001-row table (trust_reduce_kernel's user blocks take ten trips; the sweep in the
    library's own split of eight workgroups per path at T = 15, one workgroup per path at T = 129) against the fp64 restatement
    under autograd: loss, path losses, a2, d scores, the parameter gradients and the whole table gradient, which is added into a
    prefilled buffer whose pad row no path or logit touches.  The workspace starts as random bits; two calls on it repeat bit for
    bit."""
    from spex_amd import _lib
    from spex_amd.graph import _launch, _ptr
    monkeypatch.delenv("SPEX_TRUST_SPLIT", raising=False)
    table, params, seq, lens, tgt = trust_inputs(T, L, H)
    want = trust_head_restated(table, params, seq, lens, tgt, H, torch.float64)
    f32 = trust_head_restated(table, params, seq, lens, tgt, H, torch.float32)
    n_users, n_rows = TRUST_USERS, TRUST_USERS + 1
    n_ws = int(_lib.load().spex_trust_workspace_floats(T, L, 64, H, n_rows))
    assert n_ws > 0
    ws_buf = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_ws + TAIL,), dtype=torch.int32, device=dev())
    ws_tail = ws_buf[n_ws:].clone()
    ws = ws_buf.view(torch.float32)[:n_ws]
    tab_d, par_d, seq_d, len_d, tgt_d = table.to(dev()), params.to(dev()), t(seq), t(lens), t(tgt)

    def call():
        bufs = {"a2": padded(T * 64), "dscore": padded(T * n_users), "path losses": padded(T), "loss": padded(1), "grad params": padded(params.numel()),
                "grad table": padded(n_rows * 64, PREFILL)}
        bufs["loss"][1].zero_()
        _launch(dev(), "spex_trust_head_train_f32", _ptr(tab_d), n_rows, _ptr(par_d), _ptr(seq_d), _ptr(len_d), _ptr(tgt_d), T, L, 64, H, 1, 1.0,
                None, _ptr(bufs["a2"][1]), _ptr(bufs["dscore"][1]), _ptr(bufs["path losses"][1]), _ptr(ws), _ptr(bufs["loss"][1]), 0,
                _ptr(bufs["grad params"][1]), _ptr(bufs["grad table"][1]))
        torch.cuda.synchronize()
        return bufs
    first, second = call(), call()
    for q in TRUST_Q:
        assert torch.equal(first[q][0], second[q][0]), f"{q}: the second call on the same workspace differs"
        assert tail_untouched(first[q][0], first[q][1].numel(), PREFILL if q == "grad table" else SENT), q
    assert torch.equal(ws_buf[n_ws:], ws_tail)
    got = {q: first[q][1].cpu().numpy().astype(np.float64) for q in TRUST_Q}
    got["a2"], got["dscore"] = got["a2"].reshape(T, 64), got["dscore"].reshape(T, n_users)
    gt = got["grad table"].reshape(n_rows, 64)
    assert (gt[-1] == PREFILL).all(), "the pad row of grad_table lost its prefill"
    got["grad table"] = gt - PREFILL
    assert not want["grad table"][-1].any() and np.count_nonzero(np.abs(want["grad table"]).max(1)) == n_users
    for q in TRUST_Q:
        gate(f"trust head T={T} L={L} H={H} {q}", rel_err(got[q], want[q]), 2e-5, rel_err(f32[q], want[q]))
