"""bf16 gather tables against fp32, one process, alternating windows: the d = 64 SpMM launch in its plain and running-sum forms and
the whole 3-layer propagation, on Epinion2 (cache-resident) and on the HBM-resident replicated graph of bench.py's `roofline_hbm`
leg (spex_amd.datasets.scaled_graph), plus what the rounding costs where the project gates accuracy (HR / NDCG of the drop-in
model's test() on Epinion2, deviation of the propagated table).

Timing: HIP events around a window of back-to-back launches; fp32 and bf16 windows ALTERNATE, every figure is the median over the
windows with (min, max) beside it — a difference smaller than that spread is not a difference.  Share of HBM peak is ALGORITHMIC:
nnz (4 + 4 + e d) + N (4 + 4 d) bytes with e = 4 (fp32) or 2 (bf16) per gathered element, over the launch time, over 8 TB/s.

usage: python tools/bf16_gather_time.py [--hbm-log2 24] [--windows 9] [--launches 4000] [--out profiles/bf16_gather/timing.jsonl] [--no-accuracy]"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spex_amd", "dropin")):
    if p not in sys.path:
        sys.path.insert(0, p)
from spex_amd import _lib  # noqa: E402
if os.environ.get("SPEX_LIB"):          # time another build of the library (A/B of a kernel variant)
    _lib.LIB_PATH = os.path.abspath(os.environ["SPEX_LIB"])
from spex_amd.datasets import epinion2_tables, load_epinion2, materialise_epinion2, scaled_graph  # noqa: E402
from spex_amd.graph import SpexGraph, cast_bf16, lightgcn_norm_adj  # noqa: E402

HBM_PEAK_GBS = 8000.0
D, L = 64, 3
BF16 = torch.bfloat16


def algorithmic_bytes(nnz, n, elem):
    return nnz * (4 + 4 + elem * D) + n * (4 + 4 * D)


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(fns, n, windows, warm):
    """{name: (median, min, max)} us per call; one window of each variant per round, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    got = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            got[k].append(window_us(fn, n))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in got.items()}


def raw(name, *args):
    """A library entry bound to its arguments once (ctypes, no Python wrapper per call: at ~10 us per launch the wrappers' argument
    checks would be part of the figure); called once here so that a refused argument fails loudly."""
    fn = getattr(_lib.load(), name)
    args = tuple(ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args)
    _lib.check(fn(*args), name)
    return lambda: fn(*args)


def measure(name, g, X, n_launch, windows, emit):
    n, nnz = g.n_rows, g.nnz
    X16 = cast_bf16(X)
    Y, A, Y16 = torch.empty_like(X), torch.empty_like(X), torch.empty_like(X16)
    ws, ws16 = torch.empty((2,) + X.shape, device=X.device), torch.empty((2,) + X.shape, dtype=BF16, device=X.device)
    h, st = g._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = {
        "plain": {"fp32": raw("spex_spmm_f32", h, X, Y, None, 1.0, None, None, 1.0, D, st),
                  "bf16": raw("spex_spmm_bf16_f32", h, X16, Y, None, None, 1.0, None, None, 1.0, D, st),
                  "bf16_y16": raw("spex_spmm_bf16_f32", h, X16, None, Y16, None, 1.0, None, None, 1.0, D, st)},
        # the propagation's middle layers: next gather table + running sum
        "running_sum": {"fp32": raw("spex_spmm_f32", h, X, Y, None, 1.0, X, A, 1.0, D, st),
                        "bf16": raw("spex_spmm_bf16_f32", h, X16, None, Y16, None, 1.0, X, A, 1.0, D, st)},
        "propagate_L3": {"fp32": raw("spex_propagate_f32", h, X, A, None, ws, L, D, st),
                         "bf16": raw("spex_propagate_bf16_f32", h, X, A, ws16, L, D, st)},     # (includes its cast launch)
        "cast": {"bf16": raw("spex_cast_bf16_f32", X, X16, X.numel(), st)},
    }
    for form, fns in rows.items():
        per_call = L if form == "propagate_L3" else 1
        t = alternate(fns, max(1, n_launch // per_call), windows, warm=3 if n_launch < 50 else 30)
        rec = {"graph": name, "n_rows": n, "nnz": nnz, "form": form, "launches_per_window": max(1, n_launch // per_call), "windows": windows}
        for k, (med, lo, hi) in t.items():
            rec[f"{k}_us"] = {"median": med, "min": lo, "max": hi}
            if form in ("plain", "running_sum"):
                elem = 4 if k == "fp32" else 2
                rec[f"{k}_algorithmic_frac_of_hbm_peak"] = algorithmic_bytes(nnz, n, elem) / (med * 1e-6) / 1e9 / HBM_PEAK_GBS
        if "fp32" in t:
            spread = max(t["fp32"][2] - t["fp32"][1], t["bf16"][2] - t["bf16"][1])
            rec["fp32_minus_bf16_us"] = t["fp32"][0] - t["bf16"][0]
            rec["window_spread_us"] = spread
            rec["bf16_faster_beyond_spread"] = bool(t["fp32"][0] - t["bf16"][0] > spread)
        emit(rec)
    # results must not change with the timing: the bf16 launch is the fp32 launch on the widened table (rows <= 1 024 entries: bit for bit)
    ref, got = g.spmm(X16.float()), g.spmm_bf16(X16)
    emit({"graph": name, "check": "bf16 launch vs fp32 launch on the widened table", "max_abs_diff": float((ref - got).abs().max()),
          "rows_differing": int((ref != got).any(dim=1).sum()), "hub_rows": int((np.diff(g.host[0]) > 1024).sum())})
    m32, m16 = g.propagate(X, L).clone(), g.propagate(X, L, gather_dtype=BF16).clone()
    dev = (m32 - m16).abs()
    emit({"graph": name, "check": "mean_out bf16 vs fp32, L = 3", "max_abs": float(dev.max()), "max_rel_to_largest": float(dev.max() / m32.abs().max()),
          "max_rel_elementwise_over_1e-3_of_largest": float((dev / m32.abs().clamp_min(1e-3 * float(m32.abs().max()))).max())})


def accuracy(emit):
    """test() of the drop-in model on Epinion2 at the fixed E0 of the G5 end-to-end case (epinion2_tables(3186, 12407)) and after its
    five golden training steps, each model training and evaluating in its own gather dtype."""
    import lg_parser
    sys.argv = [sys.argv[0]]
    import utility1.dataloader as dataloader
    import utility1.model as model
    import utility1.utils as utils
    from utility1.batch_test import test
    gold = np.load(os.path.join(ROOT, "tests", "golden", "lightgcn_epinion2.npz"))
    root = materialise_epinion2(tempfile.mkdtemp(prefix="bf16_gather_"))
    args = lg_parser.parse_args_r(["--dataset", "epinion2", "--data_path", root])
    res = {}
    for name in ("fp32", "bf16"):
        os.environ["SPEX_GATHER_DTYPE"] = name
        utils.set_seed(args.seed)
        dataset = dataloader.Loader(args)
        net = model.LightGCN(args, dataset).to("cuda")
        uw, iw = epinion2_tables(3186, 12407)
        with torch.no_grad():
            net.embedding_user.weight.copy_(torch.from_numpy(uw))
            net.embedding_item.weight.copy_(torch.from_numpy(iw))
        res[name] = {}
        for stage in ("at_E0", "after_5_golden_steps"):
            if stage != "at_E0":
                opt = torch.optim.Adam(net.parameters(), lr=args.lr)
                net.train()
                for s in range(5):
                    opt.zero_grad()
                    u, i, y = (torch.from_numpy(gold[k][s]).cuda() for k in ("batch_users", "batch_items", "batch_labels"))
                    net(users=u, items=i, labels=y, flag=0).backward()
                    opt.step()
            net.eval()
            with torch.no_grad():
                ret = test(net, dataset.testRatings, dataset.testNegatives)
            res[name][stage] = {"recall": [float(x) for x in ret["recall"]], "ndcg": [float(x) for x in ret["ndcg"]]}
    os.environ.pop("SPEX_GATHER_DTYPE", None)
    for stage in res["fp32"]:
        d = {k: float(np.abs(np.asarray(res["fp32"][stage][k]) - np.asarray(res["bf16"][stage][k])).max()) for k in ("recall", "ndcg")}
        emit({"check": f"test() HR / NDCG @10,20,50 on Epinion2, {stage}", "fp32": res["fp32"][stage], "bf16": res["bf16"][stage],
              "max_abs_diff": d, "golden_g5_recall": [float(x) for x in gold["g5_recall"]], "golden_g5_ndcg": [float(x) for x in gold["g5_ndcg"]]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hbm-log2", type=int, default=24, help="log2 of the HBM-resident graph's node count (0: skip it)")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=4000, help="launches per window on Epinion2 (a short run under a profiler: fewer)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-accuracy", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bf16_gather_time.py measures on the GPU only")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit({"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hbm_peak_GBs": HBM_PEAK_GBS, "d": D})
    tr = load_epinion2()["train"]
    g = SpexGraph(*lightgcn_norm_adj(tr[:, 0], tr[:, 1], 3185, 12407), device=dev)
    uw, iw = epinion2_tables(3186, 12407)
    X = torch.from_numpy(np.concatenate([uw, iw])).to(dev)
    measure("epinion2", g, X, a.launches, a.windows, emit)
    if not a.no_accuracy:
        accuracy(emit)
    g.close()
    if a.hbm_log2:
        rp, cc, vv, _ = scaled_graph(a.hbm_log2, device=dev)
        g2 = SpexGraph(rp, cc, vv, device=dev)
        del rp, cc, vv
        X2 = torch.rand(g2.n_rows, D, device=dev) - 0.5
        measure(f"epinion2 x {max(1, round((1 << a.hbm_log2) / 15593))} (2^{a.hbm_log2} nodes, HBM-resident)", g2, X2, 6, a.windows, emit)
        g2.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
