"""Which native calls the epoch drivers of trainer.py issue, cell by cell (train_epoch / train_epoch_bpr / train_epoch_ngcf /
train_epoch_dual and their train_epochs* forms): family x source x option against a table written out here, recorded through
trainer._launch — every native call of the steppers goes through it.  The sampler's draw() is recorded beside it ("draw", epoch).

LightGCN: one graph of 24 users x 40 items, 6 entries per user, d = 64, L = 2 (edge dropout needs two layers), graph_t the transposed
handle; 25 positives with 5 negatives each / 150 triples: n = 150, two full batches of 64 and a ragged one of 22.  NGCF: the 300-user
graph and the builders of test_gpu_ngcf_device_sampler.py (the device sampler takes whole blocks of 256 users), batches of 384.  Dual:
the fixture of test_gpu_dual_device_sampler.py::test_python_loop_form_on_the_samplers_arrays_equals_the_native_form.

Beside the calls, the losses: every cell that trains on the same drawn epoch under the same masks must return the same total whichever
form it took — within 2e-6 of the loss, the bound test_gpu_bce_device_sampler.py, test_gpu_bpr_device_sampler.py and
test_gpu_ngcf_device_sampler.py hold a driver's total to against the explicit native call; the deterministic dual steppers bit for bit,
as their neighbour does."""
import numpy as np
import pytest
import torch

from test_gpu_dual_device_sampler import STEPS, compacted, data_root, dual_stepper, small_sampler      # noqa: F401 (data_root: a fixture)
from test_gpu_ngcf_device_sampler import make, sampler_of, small_root                                  # noqa: F401 (small_root: a fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_USERS, N_ITEMS, D, B, EPOCH = 24, 40, 64, 64, 3
LOSS_BOUND = 2e-6

# where the loop bounds sit among a native call's arguments (behind the function's name; negative: from the end)
ARGS = {
    "spex_lightgcn_epoch_bce_f32": {"max_steps": 6}, "spex_lightgcn_epoch_bpr_f32": {"max_steps": 6},
    "spex_lightgcn_epoch_bce_sampled_f32": {"max_steps": -8}, "spex_lightgcn_epoch_bpr_sampled_f32": {"max_steps": -8},
    "spex_lightgcn_train_bce_sampled_f32": {"n_epochs": -9, "max_steps": -7}, "spex_lightgcn_train_bpr_sampled_f32": {"n_epochs": -9, "max_steps": -7},
    "spex_ngcf_epoch_bce_f32": {"max_steps": 6}, "spex_ngcf_epoch_bce_sampled_f32": {"max_steps": -6},
    "spex_ngcf_train_bce_sampled_f32": {"n_epochs": -7, "max_steps": -5},
}
NOT_RECORDED = ("spex_dual_task_step_join",)          # issued only while a pipelined step is pending: not a choice of the drivers


class Recorder:
    """trainer._launch wrapped: the calls in order as (name,) or (name, {bound: value}), forwarded unchanged."""

    def __init__(self, monkeypatch):
        from spex_amd import trainer
        self.calls, inner = [], trainer._launch

        def launch(device, name, *args):
            if name not in NOT_RECORDED:
                self.calls.append((name, {k: args[i] for k, i in ARGS[name].items()}) if name in ARGS else (name,))
            return inner(device, name, *args)
        monkeypatch.setattr(trainer, "_launch", launch)

    def spy_draw(self, sampler, monkeypatch):
        inner = sampler.draw
        monkeypatch.setattr(sampler, "draw", lambda e, *a, **k: (self.calls.append(("draw", e)), inner(e, *a, **k))[1], raising=False)

    def take(self):
        out, self.calls[:] = list(self.calls), []
        return out


def close(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return a.shape == b.shape and np.all(b != 0) and float((np.abs(a - b) / np.abs(b)).max()) <= LOSS_BOUND


# ------------------------------------------------------------------------------------------ LightGCN
_cache = {}


def small_graph():
    if "graph" not in _cache:
        from spex_amd.graph import csr_transpose, lightgcn_norm_adj
        rng = np.random.default_rng(7)
        pairs = np.array([(u, i) for u in range(N_USERS) for i in rng.choice(N_ITEMS, 6, replace=False)], dtype=np.int64)
        pairs = pairs[rng.permutation(len(pairs))]
        csr = lightgcn_norm_adj(pairs[:, 0], pairs[:, 1], N_USERS, N_ITEMS)
        n = N_USERS + 1 + N_ITEMS
        E0 = ((rng.random((n, D), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
        _cache["graph"] = (pairs, csr, csr_transpose(*csr, n), E0)
    return _cache["graph"]


def lightgcn_stepper():
    from spex_amd.graph import SpexGraph
    from spex_amd.trainer import LightGCNStepper
    _, csr, (t_rowptr, t_col, t_val, eid), E0 = small_graph()
    return LightGCNStepper(SpexGraph(*csr), torch.from_numpy(E0.copy()).to(DEV), N_USERS + 1, n_layers=2, lr=1e-3,
                           graph_t=SpexGraph(t_rowptr, t_col, t_val, edge_id=eid), weight_decay=1e-4)


def lightgcn_sampler(family):
    from spex_amd.trainer import BceDeviceSampler, BprDeviceSampler
    pairs = small_graph()[0]
    if family == "bce":
        s = BceDeviceSampler(pairs[:25], N_USERS + 1, N_ITEMS, num_ng=5, seed=11, device=DEV)
    else:
        s = BprDeviceSampler(pairs, N_USERS + 1, N_ITEMS, DEV, seed=11, n=150)
    assert s.n == 150
    return s


NAMES = {"bce": dict(step="spex_lightgcn_step_bce_f32", epoch="spex_lightgcn_epoch_bce_f32", sampled="spex_lightgcn_epoch_bce_sampled_f32",
                     train="spex_lightgcn_train_bce_sampled_f32"),
         "bpr": dict(step="spex_lightgcn_step_bpr_adam_f32", epoch="spex_lightgcn_epoch_bpr_f32", sampled="spex_lightgcn_epoch_bpr_sampled_f32",
                     train="spex_lightgcn_train_bpr_sampled_f32")}
OPTIONS = {"plain": {}, "step_losses": {"step_losses": True}, "philox": {"edge_dropout": (0.7, "philox", 5)},
           "philox_step_losses": {"edge_dropout": (0.7, "philox", 5), "step_losses": True}, "reference": {"edge_dropout": (0.7, "reference")},
           "max_steps": {"max_steps": 2}}


def one_epoch_table(f):
    """(source, option) -> the calls of one train_epoch / train_epoch_bpr.  "host": the drawn epoch as host arrays; "triples" (BPR):
    as a tuple of device tensors; "sampler": the device sampler itself."""
    step3, draw = [(f["step"],)] * 3, [("draw", EPOCH)]
    table = {}
    for src in ("host", "triples", "sampler"):
        pre = draw if src == "sampler" else []
        native = f["sampled"] if src == "sampler" else f["epoch"]
        table[src, "plain"] = [(native, {"max_steps": -1})]
        table[src, "philox"] = [(native, {"max_steps": -1})]
        table[src, "max_steps"] = [(native, {"max_steps": 2})]
        table[src, "step_losses"] = table[src, "philox_step_losses"] = table[src, "reference"] = pre + step3
    return table


@pytest.mark.parametrize("family", ["bce", "bpr"])
def test_lightgcn_one_epoch_cells(family, monkeypatch):
    from spex_amd.trainer import train_epoch, train_epoch_bpr
    rec = Recorder(monkeypatch)
    s = lightgcn_sampler(family)
    drawn = s.draw(EPOCH)
    host = tuple(x.cpu().numpy() for x in drawn)
    rec.spy_draw(s, monkeypatch)
    table = one_epoch_table(NAMES[family])
    totals = {}
    for src in ("host", "sampler") + (("triples",) if family == "bpr" else ()):
        for opt, kw in OPTIONS.items():
            st = lightgcn_stepper()
            kw = dict(kw)
            losses = [] if kw.pop("step_losses", False) else None
            torch.manual_seed(99)                                     # (the reference stream's masks: the same ones in every cell)
            if family == "bce":
                total = train_epoch(st, s if src == "sampler" else None, batch_size=B, arrays=None if src == "sampler" else host, epoch=EPOCH,
                                    step_losses=losses, **kw)
            else:
                total = train_epoch_bpr(st, {"host": host, "triples": drawn, "sampler": s}[src], batch_size=B, epoch=EPOCH, step_losses=losses, **kw)
            assert rec.take() == table[src, opt], (family, src, opt)
            assert torch.is_tensor(total) and total.is_cuda
            assert st.t == (2 if opt == "max_steps" else 3) and getattr(st.graph, "mask_mode", 0) == 0
            if losses is not None:
                assert len(losses) == 3 and abs(losses[0] + losses[1] + losses[2] - total.item()) <= 1e-5 * total.item()
            totals[src, opt] = total.item()
            print(f"{family} {src:8s} {opt:12s} {totals[src, opt]:.7f}")
    # the same epoch under the same masks: one total, whichever form and source
    for (src, opt), got in totals.items():
        same_masks = {"step_losses": "plain", "philox_step_losses": "philox"}.get(opt, opt)        # (the loop's keyed masks are the native epoch's)
        assert close(got, totals["host", same_masks]), (family, src, opt, got, totals["host", same_masks])
    assert not close(totals["host", "philox"], totals["host", "plain"]) and not close(totals["host", "reference"], totals["host", "plain"])


class HostBceData:
    """LightTrainData's surface for train_epochs: ng_sample() draws a fresh 150-sample epoch from NumPy's global generator."""

    def ng_sample(self):
        self.users_fill = np.random.randint(0, N_USERS, 150).astype(np.int64)
        self.items_fill = np.random.randint(0, N_ITEMS, 150).astype(np.int64)
        self.labels_fill_np = (np.random.random(150) < 0.2).astype(np.float32)

    def __len__(self):
        return 150


@pytest.mark.parametrize("family", ["bce", "bpr"])
def test_lightgcn_two_epoch_cells(family, monkeypatch):
    """train_epochs / train_epochs_bpr over 2 epochs from epoch 4: a sampler without after_epoch is ONE native call, with it one sampled
    epoch per epoch (under the philox stream with the per-epoch seed: the same totals); host data is one native epoch per epoch."""
    from spex_amd.trainer import train_epochs, train_epochs_bpr
    f = NAMES[family]
    rec = Recorder(monkeypatch)
    s = lightgcn_sampler(family)
    rec.spy_draw(s, monkeypatch)
    run = train_epochs if family == "bce" else train_epochs_bpr
    for drop in (None, (0.7, "philox", 5)):
        results = []
        for after in (False, True):
            st, fired = lightgcn_stepper(), []
            totals = run(st, s, 2, batch_size=B, edge_dropout=drop, first_epoch=4, after_epoch=(lambda e, x: fired.append((e, float(x)))) if after else None)
            want = [(f["sampled"], {"max_steps": -1})] * 2 if after else [(f["train"], {"n_epochs": 2, "max_steps": -1})]
            assert rec.take() == want, (family, drop, after)
            assert len(totals) == 2 and all(isinstance(x, float) for x in totals) and st.t == 6
            assert fired == ([(0, totals[0]), (1, totals[1])] if after else [])
            results.append(totals)
        print(f"{family} sampler, dropout {drop}: {results}")
        assert close(results[1], results[0])
    st = lightgcn_stepper()
    assert run(st, s, 2, batch_size=B, max_steps=2) and rec.take() == [(f["train"], {"n_epochs": 2, "max_steps": 2})] and st.t == 4
    assert run(st, s, 0, batch_size=B) == [] and rec.take() == []
    # the reference stream bars the whole-run call and the native epochs: drawn and looped, the seed kept
    st = lightgcn_stepper()
    torch.manual_seed(3)
    run(st, s, 2, batch_size=B, edge_dropout=(0.7, "reference"))
    assert rec.take() == ([("draw", 0)] + [(f["step"],)] * 3 + [("draw", 1)] + [(f["step"],)] * 3)
    # host data: the next epoch prepared on a second thread, one native epoch per epoch
    results = []
    for after in (False, True):
        np.random.seed(5); torch.manual_seed(5)
        st = lightgcn_stepper()
        if family == "bce":
            totals = train_epochs(st, HostBceData(), 2, batch_size=B, after_epoch=(lambda e, x: None) if after else None)
        else:
            rng = np.random.default_rng(5)
            totals = train_epochs_bpr(st, lambda: tuple(rng.integers(0, hi, 150) for hi in (N_USERS, N_ITEMS, N_ITEMS)), 2, batch_size=B,
                                      after_epoch=(lambda e, x: None) if after else None)
        assert rec.take() == [(f["epoch"], {"max_steps": -1})] * 2 and st.t == 6
        results.append(totals)
    assert close(results[1], results[0]) and results[0][0] != results[0][1]


# ------------------------------------------------------------------------------------------ NGCF
NB = 384
N_NGCF_STEPS = 39                                      # n = 14 934: 38 full batches of 384 and a ragged one of 342


def test_ngcf_cells(small_root, monkeypatch):
    from spex_amd.trainer import train_epoch_ngcf, train_epochs_ngcf
    rec = Recorder(monkeypatch)
    data, _, _ = make(small_root)
    s = sampler_of(data, seed=5)
    host = tuple(x.cpu().numpy() for x in s.draw(EPOCH))
    rec.spy_draw(s, monkeypatch)
    step, epoch, sampled, train = ("spex_ngcf_step_bce_f32", "spex_ngcf_epoch_bce_f32", "spex_ngcf_epoch_bce_sampled_f32",
                                   "spex_ngcf_train_bce_sampled_f32")
    table = {}
    for src, native, pre in (("host", epoch, []), ("sampler", sampled, [("draw", EPOCH)])):
        table[src, "plain"] = [(native, {"max_steps": -1})]
        table[src, "max_steps"] = [(native, {"max_steps": 2})]
        table[src, "step_losses"] = pre + [(step,)] * N_NGCF_STEPS
        table[src, "callbacks"] = pre + [("cb", 0), (step,), (step,), ("cb", 2)] + [(step,)] * (N_NGCF_STEPS - 2)
    totals = {}
    for src in ("host", "sampler"):
        for opt in ("plain", "max_steps", "step_losses", "callbacks"):
            _, model, st = make(small_root)
            losses = [] if opt == "step_losses" else None
            cbs = {0: lambda: rec.calls.append(("cb", 0)), 2: lambda: rec.calls.append(("cb", 2))} if opt == "callbacks" else None
            total = train_epoch_ngcf(st, s if src == "sampler" else data, batch_size=NB, arrays=None if src == "sampler" else host, epoch=EPOCH,
                                     step_losses=losses, callbacks=cbs, max_steps=2 if opt == "max_steps" else None)
            assert rec.take() == table[src, opt], (src, opt)
            n_steps = 2 if opt == "max_steps" else N_NGCF_STEPS
            assert torch.is_tensor(total) and st.t == n_steps and model.dropout_step == n_steps
            if losses is not None:
                assert len(losses) == N_NGCF_STEPS and abs(sum(losses) - total.item()) <= 1e-5 * total.item()
            totals[src, opt] = total.item()
            print(f"ngcf {src:8s} {opt:12s} {totals[src, opt]:.7f}")
    for (src, opt), got in totals.items():
        assert close(got, totals["host", "max_steps" if opt == "max_steps" else "plain"]), (src, opt)
    # two epochs from epoch 1
    results = []
    for after in (False, True):
        _, _, st = make(small_root)
        fired = []
        got = train_epochs_ngcf(st, s, 2, batch_size=NB, first_epoch=1, max_steps=3, after_epoch=(lambda e, x: fired.append((e, float(x)))) if after else None)
        assert rec.take() == ([(sampled, {"max_steps": 3})] * 2 if after else [(train, {"n_epochs": 2, "max_steps": 3})])
        assert st.t == 6 and fired == ([(0, got[0]), (1, got[1])] if after else []) and all(isinstance(x, float) for x in got)
        results.append(got)
    assert close(results[1], results[0])
    assert train_epochs_ngcf(st, s, 0, batch_size=NB) == [] and rec.take() == []
    # two layers: no native form — drawn and looped through the deep one-call step
    _, _, deep = make(small_root, layers="[64,64]", deterministic=False)
    train_epoch_ngcf(deep, s, batch_size=NB, epoch=EPOCH, max_steps=2)
    assert rec.take() == [("draw", EPOCH)] + [("spex_ngcf_deep_step_bce_f32",)] * 2
    train_epochs_ngcf(deep, s, 2, batch_size=NB, max_steps=1)
    assert rec.take() == [("draw", 0), ("spex_ngcf_deep_step_bce_f32",), ("draw", 1), ("spex_ngcf_deep_step_bce_f32",)]


# ------------------------------------------------------------------------------------------ dual-task
def test_dual_cells(epinion2, golden, data_root, monkeypatch):
    """The sampler's epoch and the same epoch as host arrays (its draw compacted to the path_off form), each native and — cum_every = 1
    forces it — step by step: four deterministic steppers, one state and one (loss1, loss2)."""
    from spex_amd.trainer import train_epoch_dual
    rec = Recorder(monkeypatch)
    s = small_sampler(epinion2, golden)
    out = s.draw(0, max_steps=STEPS)
    count = out[6].cpu().numpy()
    seq, seq_l, tgt, path_off = compacted(out, STEPS, s.cap)
    n = STEPS * 256
    arrays = (out[0][:n].cpu().numpy(), out[1][:n].cpu().numpy(), out[2][:n].cpu().numpy(), seq.cpu().numpy(), seq_l.cpu().numpy(), tgt.cpu().numpy(),
              [list(range(int(c))) for c in count])
    results = []
    for src in ("sampler", "host"):
        for cum_every in (None, 1):
            st, cum, n_paths = dual_stepper(data_root, s.path_len), [], []
            if src == "sampler":
                got = train_epoch_dual(st, s, epoch=0, max_steps=STEPS, cum_every=cum_every, cum_out=cum, n_paths_out=n_paths)
                native = "spex_dual_task_epoch_strided_f32"
            else:
                got = train_epoch_dual(st, None, object(), {}, s.cap, batch_size=256, cum_every=cum_every, cum_out=cum, n_paths_out=n_paths,
                                       arrays=arrays)
                native = "spex_dual_task_epoch_f32"
            assert rec.take() == ([("spex_dual_task_step_f32",)] * STEPS if cum_every else [(native,)]), (src, cum_every)
            assert n_paths == count.tolist() and len(cum) == (STEPS if cum_every else 0) and st.t == STEPS
            assert not cum or torch.equal(cum[-1], got)
            results.append((got, st))
    got0, st0 = results[0]
    assert got0[0].item() > 0 and got0[1].item() > 0
    for got, st in results[1:]:
        assert torch.equal(got, got0) and torch.equal(st.arena, st0.arena) and torch.equal(st.m, st0.m) and torch.equal(st.v, st0.v)
