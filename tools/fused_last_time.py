"""The one-call BPR step on Epinion2 (d = 64) with its last layer inside the BPR launch (SPEX_STEP_FUSED_LAST=1) against the
whole-graph schedule (=0): us per step by HIP events, both forms forced, over a sweep of batch sizes T — the measurement the
constant of step_fuses_last (spex_amd/csrc/spmm.hip) is fixed from.  One JSON line per (L, T).
usage: python tools/fused_last_time.py [--layers 3] [--T 256 1024 2048 4096 8192] [--steps 400] [--reps 5]
SPEX_LIB=<path> times another build of the library."""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if os.environ.get("SPEX_LIB"):
    from spex_amd import _lib as _l
    _l.LIB_PATH = os.path.abspath(os.environ["SPEX_LIB"])
from spex_amd.datasets import load_epinion2, xavier_uniform_np
from spex_amd.graph import SpexGraph, lightgcn_norm_adj
from spex_amd.trainer import LightGCNStepper
dev = torch.device("cuda:0")


def timed(fn, n, reps):
    """us per call: median and minimum over `reps` timed regions of n calls."""
    for _ in range(30): fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    return float(np.median(out)), float(min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, nargs="+", default=[3])
    ap.add_argument("--T", type=int, nargs="+", default=[256, 1024, 2048, 4096, 8192])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    tr = load_epinion2()["train"]
    n_u, n_i = 3185, 12407
    g = SpexGraph(*lightgcn_norm_adj(tr[:, 0], tr[:, 1], n_u, n_i), device=dev)
    rng = np.random.default_rng(13)
    E0 = torch.from_numpy(np.concatenate([xavier_uniform_np(n_u + 1, 64, rng), xavier_uniform_np(n_i, 64, rng)])).to(dev)
    for L in a.layers:
        for T in a.T:
            tu, tp, tn = (torch.from_numpy(rng.integers(0, hi, T)).to(dev) for hi in (n_u, n_i, n_i))
            row = {"graph": "epinion2", "n_rows": n_u + 1 + n_i, "L": L, "T": T}
            for form in ("0", "1"):
                os.environ["SPEX_STEP_FUSED_LAST"] = form
                st = LightGCNStepper(g, E0.clone(), n_u + 1, n_layers=L, lr=1e-3)
                med, best = timed(lambda: st.step_bpr_sgd(tu, tp, tn), a.steps, a.reps)
                row["fused_us" if form == "1" else "whole_graph_us"] = {"median": round(med, 2), "min": round(best, 2)}
            del os.environ["SPEX_STEP_FUSED_LAST"]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
