"""The one launcher behind the ten spex_lightgcn_[bpr_]batch_* exports (batch.hip: spex::batch_launch over a spex::BatchLaunch
descriptor): every export, called through the C ABI, against the one-call training step that reaches the same kernel
through steps.hip (step_batch fills the same descriptor).

Input: a random non-symmetric square graph of 1 100 rows (300 user rows) — the smallest size class at which a row can hold more than
1 024 stored entries, since a row's columns are distinct: user row 0 has 1 030 (more than one workgroup's 16 x 64 gather slots and
more than one part's push runs), user row 1 is empty, one item row has 70 (two segments), the rest 1 .. 11.  B = T = 5; samples
0 .. 2 name the hub row (so that its columns receive three or more atomic addends per launch), sample 3 the empty row, sample 4 has
a user index out of range (skipped whole: zero slots, loss 0, no count).  n_layers = 2: the step's forward is one plain launch y1 = A E0
(left in ws_fwd[0]), and the batch kernel adds E0 + y1 at the batch's rows — the exports take that sum as their one running-sum table,
formed here by one fp32 add per element, the kernel's own.

Equivalence (12 cases: BCE / BPR x slots / push x fp32 d = 64, fp32 d = 128, bf16 d = 64): slots, per-sample losses and row_counts
equal the step's bit for bit.  The push tables G and g_out are consumed and cleared inside the step, so they are held against the
launch's own statement instead: the slot rows (bit-equal to the step's, asserted in the same case) pushed by a sequential fp32 sum in
sample order on the host — g_out[r] += g, G[r] += push_scale * g, G[col[e]] += val[e] * (push_scale * g), each product rounded once as
in the kernel.  Such a sum is one of the orders the kernel's float atomics can take, so the launch may differ from it by the
atomic-order spread only.  That spread, measured on this input with the kernels as they were BEFORE they shared their push loop (the
parent commit's build; 16 384 launches per export, largest element-wise max - min over the launches, absolute; values up to 3.7e-3
in G, three times that in g_out, so the figures are one to two units in the last place; no launch was farther than its figure from
the sequential sum; the kernels with the shared loop gave the same twelve figures):
    spex_lightgcn_batch_f32 d = 64            G 2.328306e-10   g_out 4.656613e-10
    spex_lightgcn_batch_f32 d = 128           G 4.656613e-10   g_out 9.313226e-10
    spex_lightgcn_batch_bf16_f32              G 4.656613e-10   g_out 9.313226e-10
    spex_lightgcn_bpr_batch_f32               G 4.656613e-10   g_out 9.313226e-10
    spex_lightgcn_bpr_batch_wide_f32 d = 128  G 4.656613e-10   g_out 9.313226e-10
    spex_lightgcn_bpr_batch_bf16_f32          G 4.656613e-10   g_out 4.656613e-10
The test allows twice the figure of its export (SPREAD below).  Every case prints what it asserts on."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_wide_step import random_csr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
N, N_U, B, L = 1100, 300, 5, 2
USERS = np.array([0, 0, 0, 1, N_U + 5], np.int64)          # hub, hub, hub, the empty row, out of range
ITEMS = np.array([3, 9, 40, 11, 2], np.int64)              # (item 40: the row of 70 entries)
NEG = np.array([9, 14, 20, 3, 5], np.int64)
LABELS = np.array([1, 0, 1, 0, 1], np.float32)
WEIGHT_DECAY = 1e-3
OK, INVALID, UNSUPPORTED = 0, -1, -4

# (export, triples, push form, bf16 table, width)
ENTRIES = [
    ("spex_lightgcn_batch_slots_f32", False, False, False, 64),
    ("spex_lightgcn_batch_slots_f32", False, False, False, 128),
    ("spex_lightgcn_batch_f32", False, True, False, 64),
    ("spex_lightgcn_batch_f32", False, True, False, 128),
    ("spex_lightgcn_bpr_batch_slots_f32", True, False, False, 64),
    ("spex_lightgcn_bpr_batch_slots_wide_f32", True, False, False, 128),
    ("spex_lightgcn_bpr_batch_f32", True, True, False, 64),
    ("spex_lightgcn_bpr_batch_wide_f32", True, True, False, 128),
    ("spex_lightgcn_batch_slots_bf16_f32", False, False, True, 64),
    ("spex_lightgcn_batch_bf16_f32", False, True, True, 64),
    ("spex_lightgcn_bpr_batch_slots_bf16_f32", True, False, True, 64),
    ("spex_lightgcn_bpr_batch_bf16_f32", True, True, True, 64),
]
IDS = [f"{e[0]}-d{e[4]}" for e in ENTRIES]
# atomic-order spread of the parent commit's kernels on this input (the docstring's table): (G, g_out), absolute
SPREAD = {
    "spex_lightgcn_batch_f32-d64": (2.328306e-10, 4.656613e-10),
    "spex_lightgcn_batch_f32-d128": (4.656613e-10, 9.313226e-10),
    "spex_lightgcn_batch_bf16_f32-d64": (4.656613e-10, 9.313226e-10),
    "spex_lightgcn_bpr_batch_f32-d64": (4.656613e-10, 9.313226e-10),
    "spex_lightgcn_bpr_batch_wide_f32-d128": (4.656613e-10, 9.313226e-10),
    "spex_lightgcn_bpr_batch_bf16_f32-d64": (4.656613e-10, 4.656613e-10),
}
_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr():
    if "csr" not in _cache:
        rng = np.random.default_rng(11)
        deg = rng.integers(1, 12, N)
        deg[0], deg[1], deg[N_U + 40] = 1030, 0, 70
        rowptr, col, val = random_csr(rng, N, N, deg)
        _cache["csr"] = (rowptr, col, val * np.float32(0.05))
    return _cache["csr"]


def handles():
    """(A, A^T with the edge-id permutation): the step's graph and graph_t."""
    if "handles" not in _cache:
        from spex_amd.graph import SpexGraph, csr_transpose
        t_rowptr, t_col, t_val, eid = csr_transpose(*csr(), N)
        _cache["handles"] = (SpexGraph(*csr()), SpexGraph(t_rowptr, t_col, t_val, edge_id=eid))
    return _cache["handles"]


def table(d):
    if ("E0", d) not in _cache:
        _cache["E0", d] = np.random.default_rng(2020 + d).uniform(-0.1, 0.1, (N, d)).astype(np.float32)
    return _cache["E0", d]


def batch(bpr):
    key = ("batch", bpr)
    if key not in _cache:
        _cache[key] = (t(USERS), t(ITEMS), t(NEG) if bpr else t(LABELS))
    return _cache[key]


def p(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def call(name, bpr, push, g, X, acc_in, idx, E0, d, out):
    """One export through the C ABI, arguments in the header's order; returns (status, message)."""
    from spex_amd import _lib
    from spex_amd.graph import _stream
    a, b, c = idx
    args = [g._h, p(X), p(acc_in), ctypes.c_float(L + 1), p(a), p(b), p(c), B, N_U, ctypes.c_float(1.0 / B)]
    if push:
        args.append(ctypes.c_float(1.0 / (L + 1)))
    if bpr:
        args += [ctypes.c_float(WEIGHT_DECAY), p(E0), p(out.get("row_counts"))]
    args += [None, p(out.get("loss"))]
    args += [p(out.get("g_out")), p(out.get("G"))] if push else [p(out.get("slots"))]
    args += [d, _stream(DEV)]
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.spex_last_error().decode("utf-8", "replace")


def outputs(bpr, push, d):
    k = 3 if bpr else 2
    out = {"loss": torch.full((B,), float("nan"), device=DEV)}
    if bpr:
        out["row_counts"] = torch.zeros(N, dtype=torch.int32, device=DEV)
    if push:
        out["G"], out["g_out"] = torch.zeros(N, d, device=DEV), torch.zeros(N, d, device=DEV)
    else:
        out["slots"] = torch.full((k * B, d), float("nan"), device=DEV)
    return out


def step_state(bpr, push, bf16, d):
    """One one-call training step of the form that reaches the export's kernel; returns (stepper, E0 before the step)."""
    from spex_amd.trainer import LightGCNStepper
    g, gt = handles()
    E0 = t(table(d))
    st = LightGCNStepper(g, E0.clone(), N_U, n_layers=L, lr=1e-3, graph_t=gt, deterministic=not push,
                         weight_decay=WEIGHT_DECAY if bpr else 0.0, gather_dtype=BF16 if bf16 else None)
    acc = torch.zeros(1, device=DEV)
    a, b, c = batch(bpr)
    if bpr:
        st.step_bpr_exact(a, b, c, loss_acc=acc, batch_rows_only=True)
    else:
        st.step_bce(a, b, c, loss_acc=acc, batch_rows_only=True)
    torch.cuda.synchronize()
    assert st.t == 1, "the one-call step did not run"
    return st, E0


def entry_inputs(st, E0, bf16):
    """What the step's batch launch read: the gather table y1 (ws_fwd[0]; bf16: its rounding, which the forward launch wrote from the
    same register) and the running sum E0 + y1."""
    y1 = st.ws_fwd[0]
    return (y1.to(BF16).contiguous() if bf16 else y1), (E0 + y1).contiguous()


def pushed_by_hand(slots, bpr, d):
    """The launch's statement on the host: the slot rows added into (G, g_out) by a sequential fp32 sum in sample order."""
    rowptr, col, val = csr()
    g = slots.cpu().numpy()
    G, g_out = np.zeros((N, d), np.float32), np.zeros((N, d), np.float32)
    scale = np.float32(1.0) / np.float32(L + 1)
    lists = [USERS, ITEMS + N_U] + ([NEG + N_U] if bpr else [])
    for s in range(B):
        if USERS[s] >= N_U:
            continue
        for k, rows in enumerate(lists):
            r, row_g = int(rows[s]), g[k * B + s]
            g_out[r] += row_g
            gs = scale * row_g                                   # push_scale * g: one rounding, then one per product
            G[r] += gs
            e = slice(rowptr[r], rowptr[r + 1])
            G[col[e]] += val[e][:, None] * gs[None, :]           # (a row's columns are distinct)
    return G, g_out


@pytest.mark.parametrize("entry", ENTRIES, ids=IDS)
def test_export_equals_the_one_call_step(entry):
    name, bpr, push, bf16, d = entry
    g, _ = handles()
    st, E0 = step_state(bpr, push, bf16, d)
    X, acc_in = entry_inputs(st, E0, bf16)
    k = 3 if bpr else 2
    out = outputs(bpr, push, d)
    rc, msg = call(name, bpr, push, g, X, acc_in, batch(bpr), E0, d, out)
    torch.cuda.synchronize()
    assert rc == OK, msg
    # per-sample losses: the deterministic step keeps them at the head of lo_batch, the push step at the head of grad_slots
    step_loss = (st.grad_slots if push else st.lo_batch).reshape(-1)[:B]
    print(f"{name} d={d}: losses {out['loss'].tolist()} (step {step_loss.tolist()})")
    assert torch.equal(out["loss"], step_loss)
    assert out["loss"][B - 1].item() == 0.0 and (out["loss"][:B - 1] > 0).all()       # the skipped sample; the others scored
    if bpr:
        print(f"  row_counts: {int(out['row_counts'].sum())} occurrences (step {int(st.row_counts[1].sum())})")
        assert torch.equal(out["row_counts"], st.row_counts[1]) and int(out["row_counts"].sum()) == 3 * (B - 1)
    if not push:
        same = torch.equal(out["slots"], st.grad_slots[:k * B])
        print(f"  slots bit-equal: {same}; largest |slot| {out['slots'].abs().max().item():.3e}")
        assert same
        assert all(float(out["slots"][j * B + B - 1].abs().max()) == 0.0 for j in range(k))       # the skipped sample's rows
        return
    # the push tables against the launch's statement from the slot rows of the same form
    slot_name = name.replace("batch_", "batch_slots_", 1)
    slots = outputs(bpr, False, d)
    rc, msg = call(slot_name, bpr, False, g, X, acc_in, batch(bpr), E0, d, slots)
    assert rc == OK, msg
    torch.cuda.synchronize()
    G_ref, g_out_ref = pushed_by_hand(slots["slots"], bpr, d)
    for what, got, ref, spread in (("G", out["G"], G_ref, SPREAD[f"{name}-d{d}"][0]), ("g_out", out["g_out"], g_out_ref, SPREAD[f"{name}-d{d}"][1])):
        err = float(np.abs(got.cpu().numpy() - ref).max())
        print(f"  {what}: largest |launch - sequential sum| {err:.3e}, allowed {2 * spread:.3e} (largest |{what}| {np.abs(ref).max():.3e})")
        assert np.abs(ref).max() > 0 and err <= 2 * spread


EXPORTS = [e for k, e in enumerate(ENTRIES) if e[0] not in [f[0] for f in ENTRIES[:k]]]        # each of the ten once


@pytest.mark.parametrize("entry", EXPORTS, ids=[e[0] for e in EXPORTS])
def test_export_refuses_a_wrong_width_and_a_null_table_by_name(entry):
    name, bpr, push, bf16, d = entry
    g, _ = handles()
    E0 = t(table(d))
    X = E0.to(BF16) if bf16 else E0
    bad_d = {"spex_lightgcn_bpr_batch_slots_wide_f32": 64, "spex_lightgcn_bpr_batch_wide_f32": 64}.get(name, 128 if bpr or bf16 else 96)
    out = outputs(bpr, push, d)
    rc, msg = call(name, bpr, push, g, X, E0, batch(bpr), E0, bad_d, out)
    print(f"{name}: d = {bad_d} -> {rc}: {msg}")
    assert rc == UNSUPPORTED and msg.startswith(name + ":") and str(bad_d) in msg
    rc, msg = call(name, bpr, push, g, None, E0, batch(bpr), E0, d, out)
    print(f"{name}: X = NULL -> {rc}: {msg}")
    assert rc == INVALID and msg.startswith(name + ":") and "NULL" in msg
    torch.cuda.synchronize()
    assert torch.isnan(out["loss"]).all()                     # nothing was launched
