#!/usr/bin/env python3
"""The one-call exact training steps with bf16 gather tables (LightGCNStepper(gather_dtype=torch.bfloat16), SPEX_STEP_BF16_GATHER)
against the fp32 steps: one process, an fp32 and a bf16 stepper over ONE pair of graph handles, their windows alternating.

Measured: the one-call exact BCE step at B = 256 (push form) and the exact BPR step at T = 2 048 (dense form), L = 3, d = 64, on
Epinion2 (cache-resident) or on spex_amd.datasets.scaled_graph(K) (2^K nodes: HBM-resident from K = 22).  Timing: HIP events around
a window of back-to-back steps; every figure is the median over the windows with (min, max) — a difference inside that spread is
not a difference.  --trace: no timing; a few steps of ONE mode for a kernel trace taken around this script in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/bf16_step_time.py --graph epinion2 --trace bf16).

usage: python tools/bf16_step_time.py --graph epinion2|22|24 [--windows 9] [--steps N] [--out profiles/bf16_step/timing.jsonl]"""
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

L, D = 3, 64


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
        return SpexGraph(*csr, device=dev), E0, n_u
    rp, cc, vv, n_u = scaled_graph(int(which), device=dev)
    g = SpexGraph(rp, cc, vv, device=dev)
    return g, (torch.rand(len(rp) - 1, D, device=dev) - 0.5) * 0.1, n_u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="epinion2")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=0, help="steps per window (0: 400 on Epinion2, 6 on the scaled graphs)")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", choices=["fp32", "bf16"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bf16_step_time.py: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    dev = torch.device("cuda:0")
    g, E0, n_u = build(a.graph, dev)
    n = g.n_rows
    rng = np.random.default_rng(0)
    dt = lambda x: torch.from_numpy(x.astype(np.int64)).to(dev)
    B, T = 256, 2048
    bce = (dt(rng.integers(0, n_u, B)), dt(rng.integers(0, n - n_u, B)), (torch.rand(B, device=dev) < 1 / 6).float())
    bpr = (dt(rng.integers(0, n_u, T)), dt(rng.integers(0, n - n_u, T)), dt(rng.integers(0, n - n_u, T)))
    acc = torch.zeros(1, device=dev)
    modes = ("fp32", "bf16") if a.trace is None else (a.trace,)
    st = {m: LightGCNStepper(g, E0.clone(), n_u, n_layers=L, lr=1e-3, weight_decay=1e-4,
                             gather_dtype=torch.bfloat16 if m == "bf16" else None) for m in modes}
    step_bce = {m: (lambda s=s: s.step_bce(*bce, loss_acc=acc, batch_rows_only=True)) for m, s in st.items()}
    step_bpr = {m: (lambda s=s: s.step_bpr_exact(*bpr, loss_acc=acc, batch_rows_only=True)) for m, s in st.items()}
    if a.trace is not None:
        for fn in (step_bce[a.trace], step_bpr[a.trace]):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return
    steps = a.steps or (400 if a.graph == "epinion2" else 6)
    rows = []
    for name, fns in (("exact BCE step, B = 256 (push form)", step_bce), ("exact BPR step, T = 2048 (dense form)", step_bpr)):
        res = alternate(fns, steps, a.windows, 3)
        row = {"graph": a.graph, "n": n, "nnz": g.nnz, "step": name, "windows": a.windows, "steps_per_window": steps,
               "fp32_us": res["fp32"], "bf16_us": res["bf16"], "fp32_over_bf16": res["fp32"][0] / res["bf16"][0]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
