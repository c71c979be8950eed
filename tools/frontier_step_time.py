#!/usr/bin/env python3
"""The one-call exact training steps in frontier form (LightGCNStepper(frontier=True), SPEX_STEP_FRONTIER) against the whole-graph
form: one process, a frontier=False and a frontier=True stepper over ONE graph handle, their windows alternating.

Measured: the exact BCE step at B = 256 / 2 048 and the exact BPR step at T = 256 / 2 048 (whole-graph form: push or dense by the
step's own choice; frontier form: push at any T), L = 2 and 3, d = 64, on Epinion2 (cache-resident) or on
spex_amd.datasets.scaled_graph(K) (2^K nodes: HBM-resident from K = 22).  Every time includes every launch of the step, the clears of
the push targets among them.  Timing: HIP events around a window of back-to-back steps; every figure is the median over the windows
with (min, max) — a difference inside that spread is not a difference.  --trace L: no timing; three BCE steps (B = 256) of the
frontier form at depth L for a kernel trace taken around this script in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/frontier_step_time.py --graph 24 --trace 2).

usage: python tools/frontier_step_time.py --graph epinion2|22|24 [--windows 9] [--steps N] [--out profiles/frontier/timing.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spex_amd.datasets import epinion2_tables, load_epinion2, scaled_graph  # noqa: E402
from spex_amd.graph import SpexGraph, lightgcn_norm_adj  # noqa: E402
from spex_amd.trainer import LightGCNStepper  # noqa: E402

D = 64


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
    for fn in fns.values():
        for _ in range(warm):
            fn()
    got = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            got[k].append(window_us(fn, n))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in got.items()}


def build(which, dev):
    if which == "epinion2":
        n_u, n_i = 3186, 12407              # the fixture's user rows (one spare, as the reference counts them) and items
        tr = load_epinion2()["train"]
        csr = lightgcn_norm_adj(tr[:, 0], tr[:, 1], n_u - 1, n_i)
        E0 = torch.from_numpy(np.concatenate(epinion2_tables(n_u, n_i, dim=D))).to(dev)
        return SpexGraph(*csr, device=dev), E0, n_u, csr[0]
    rp, cc, vv, n_u = scaled_graph(int(which), device=dev)
    g = SpexGraph(rp, cc, vv, device=dev)
    return g, (torch.rand(len(rp) - 1, D, device=dev) - 0.5) * 0.1, n_u, rp


def draw(rng, rowptr, n_u, n, k, dev):
    """k (user, positive item, uniform item): the positives degree-weighted, as the samplers draw them."""
    deg = np.diff(rowptr)[n_u:].astype(np.float64)
    pos = rng.choice(n - n_u, k, p=deg / deg.sum())
    dt = lambda x: torch.from_numpy(np.asarray(x, np.int64)).to(dev)
    return dt(rng.integers(0, n_u, k)), dt(pos), dt(rng.integers(0, n - n_u, k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="epinion2")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=0, help="steps per window (0: 400 on Epinion2, 6 on the scaled graphs)")
    ap.add_argument("--layers", default="2,3")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frontier_step_time.py: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    dev = torch.device("cuda:0")
    g, E0, n_u, rowptr = build(a.graph, dev)
    n = g.n_rows
    rng = np.random.default_rng(0)
    batches = {k: draw(rng, rowptr, n_u, n, k, dev) for k in (256, 2048)}
    labels = {k: (torch.rand(k, device=dev) < 1 / 6).float() for k in batches}
    acc = torch.zeros(1, device=dev)
    if a.trace:
        st = LightGCNStepper(g, E0.clone(), n_u, n_layers=a.trace, lr=1e-3, weight_decay=1e-4, frontier=True)
        u, p, _ = batches[256]
        for _ in range(3):
            st.step_bce(u, p, labels[256], loss_acc=acc, batch_rows_only=True)
        torch.cuda.synchronize()
        print("frontier rows |Bset|, |F1|:", st._front.counts.tolist())
        return
    steps = a.steps or (400 if a.graph == "epinion2" else 6)
    rows = []
    for L in (int(x) for x in a.layers.split(",")):
        st = {m: LightGCNStepper(g, E0.clone(), n_u, n_layers=L, lr=1e-3, weight_decay=1e-4, frontier=m == "frontier") for m in ("whole", "frontier")}
        for kind, k in (("bce", 256), ("bce", 2048), ("bpr", 256), ("bpr", 2048)):
            u, p, ng = batches[k]
            if kind == "bce":
                fns = {m: (lambda s=s: s.step_bce(u, p, labels[k], loss_acc=acc, batch_rows_only=True)) for m, s in st.items()}
            else:
                fns = {m: (lambda s=s: s.step_bpr_exact(u, p, ng, loss_acc=acc, batch_rows_only=True)) for m, s in st.items()}
            res = alternate(fns, steps, a.windows, 3)
            f1 = st["frontier"]._front.counts.tolist()
            row = {"graph": a.graph, "n": n, "nnz": g.nnz, "L": L, "step": f"exact {kind.upper()} step, {'B' if kind == 'bce' else 'T'} = {k}",
                   "Bset_rows": f1[0], "F1_rows": f1[1], "windows": a.windows, "steps_per_window": steps, "whole_us": res["whole"],
                   "frontier_us": res["frontier"], "whole_over_frontier": res["whole"][0] / res["frontier"][0]}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del st
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
