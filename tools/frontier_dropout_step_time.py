#!/usr/bin/env python3
"""The exact training steps under edge dropout (keep_prob 0.3, the in-kernel sampled mask, a fresh seed per step as the native epochs
draw it) in frontier form against the whole-graph masked step: one process, ONE stepper built with frontier=True over a graph handle
and its transposed handle (edge-id permutation), its forms switched between windows that alternate:

  whole_masked      the whole-graph masked one-call step (`stepper.frontier = False`): the baseline
  frontier_masked   the frontier masked step
  sparse_masked     L = 2 only: the frontier masked step with row-sparse Adam (SPEX_STEP_SPARSE_ADAM)
  frontier_plain    the unmasked frontier step: what the smaller masked F1 buys is frontier_plain - frontier_masked

A window is ONE native epoch call (epoch_bce / epoch_bpr) over `steps` copies of the batch: the host issues the launches and nothing
else, and under keep_prob < 1 every step runs with its own mask seed.  Measured: the exact BCE step at B = 256 / 2 048 and the exact
BPR step at T = 256 / 2 048, L = 2 and 3, d = 64, on Epinion2 (cache-resident) or spex_amd.datasets.scaled_graph(K) (2^K nodes:
HBM-resident from K = 22).  HIP events around the window; every figure is the median over the windows with (min, max) — a difference
inside that spread is not a difference.  The row counts are those of the window's last step.

usage: python tools/frontier_dropout_step_time.py --graph epinion2|22|24 [--windows 7] [--steps N] [--keep-prob 0.3]
                                                  [--out profiles/frontier_dropout/timing.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from frontier_step_time import D, draw  # noqa: E402
from spex_amd.datasets import epinion2_tables, load_epinion2, scaled_graph  # noqa: E402
from spex_amd.graph import SpexGraph, lightgcn_norm_adj  # noqa: E402
from spex_amd.trainer import LightGCNStepper  # noqa: E402


def transposed_handle(rowptr, col, val, dev):
    """The handle of A^T with the edge-id permutation (graph.csr_transpose's result), formed on the device: a stable sort of the
    entries by (column, row)."""
    rp = torch.as_tensor(np.asarray(rowptr), device=dev).long()
    cc = torch.as_tensor(np.asarray(col), device=dev).long()
    n = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, device=dev), rp[1:] - rp[:-1])
    order = torch.argsort(cc * n + rows, stable=True)
    t_rowptr = torch.zeros(n + 1, dtype=torch.long, device=dev)
    t_rowptr[1:] = torch.cumsum(torch.bincount(cc, minlength=n), 0)
    vv = torch.as_tensor(np.asarray(val), device=dev)[order]
    out = [x.cpu().numpy() for x in (t_rowptr.int(), rows[order].int(), vv, order.int())]
    del rp, cc, rows, order, vv
    return SpexGraph(out[0], out[1], out[2], edge_id=out[3], device=dev)


def load(which, dev):
    """(rowptr, col, val), E0, n_user_rows: tools/frontier_step_time.py's graphs and tables."""
    if which == "epinion2":
        n_u, n_i = 3186, 12407
        tr = load_epinion2()["train"]
        csr = lightgcn_norm_adj(tr[:, 0], tr[:, 1], n_u - 1, n_i)
        return csr, torch.from_numpy(np.concatenate(epinion2_tables(n_u, n_i, dim=D))).to(dev), n_u
    rp, cc, vv, n_u = scaled_graph(int(which), device=dev)
    return (rp, cc, vv), (torch.rand(len(rp) - 1, D, device=dev) - 0.5) * 0.1, n_u


def window_us(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="epinion2")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=0, help="steps per window (0: 200 on Epinion2, 6 on the scaled graphs)")
    ap.add_argument("--layers", default="2,3")
    ap.add_argument("--keep-prob", type=float, default=0.3)
    ap.add_argument("--cells", default="bce:256,bce:2048,bpr:256,bpr:2048")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frontier_dropout_step_time.py: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    dev = torch.device("cuda:0")
    csr, E0, n_u = load(a.graph, dev)
    rowptr = csr[0]
    g = SpexGraph(*csr, device=dev)
    gt = transposed_handle(*csr, dev)
    n = g.n_rows
    rng = np.random.default_rng(0)
    steps = a.steps or (200 if a.graph == "epinion2" else 6)
    cells = [(c.split(":")[0], int(c.split(":")[1])) for c in a.cells.split(",")]
    batches = {k: draw(rng, rowptr, n_u, n, k, dev) for k in sorted({k for _, k in cells})}
    labels = {k: (torch.rand(k, device=dev) < 1 / 6).float() for k in batches}
    acc = torch.zeros(2, 1, device=dev)
    rows = []
    for L in (int(x) for x in a.layers.split(",")):
        st = LightGCNStepper(g, E0.clone(), n_u, n_layers=L, lr=1e-3, weight_decay=1e-4, graph_t=gt, frontier=True)
        forms = {"whole_masked": (False, False, a.keep_prob), "frontier_masked": (True, False, a.keep_prob)}
        if L == 2:
            forms["sparse_masked"] = (True, True, a.keep_prob)
        forms["frontier_plain"] = (True, False, 1.0)
        for kind, k in cells:
            u, p, ng = (x.repeat(steps) for x in batches[k])
            y = labels[k].repeat(steps)
            seed = [0]

            def run(form):
                frontier, sparse, kp = forms[form]
                st.frontier = frontier
                st.sparse_adam = sparse
                seed[0] += 1
                if kind == "bce":
                    st.epoch_bce(u, p, y, k, acc[0], acc[1], keep_prob=kp, drop_seed=seed[0])
                else:
                    st.epoch_bpr(u, p, ng, k, acc[0], acc[1], keep_prob=kp, drop_seed=seed[0])

            got, counts = {f: [] for f in forms}, {}
            for f in forms:
                run(f)                                           # warm-up: allocations, the first touch of every table
            for _ in range(a.windows):
                for f in forms:
                    got[f].append(window_us(lambda f=f: run(f), steps))
                    if forms[f][0]:
                        counts[f] = st._front.counts.tolist()
            res = {f: (float(np.median(v)), float(min(v)), float(max(v))) for f, v in got.items()}
            row = {"graph": a.graph, "n": n, "nnz": g.nnz, "L": L, "keep_prob": a.keep_prob,
                   "step": f"exact {kind.upper()} step, {'B' if kind == 'bce' else 'T'} = {k}", "windows": a.windows, "steps_per_window": steps,
                   "Bset_rows": counts["frontier_plain"][0], "F1_rows": counts["frontier_plain"][1], "F1_rows_masked": counts["frontier_masked"][1]}
            if L == 2:
                row["F2_rows_masked"] = counts["sparse_masked"][2]
            for f, v in res.items():
                row[f + "_us"] = v
            row["whole_over_frontier_masked"] = res["whole_masked"][0] / res["frontier_masked"][0]
            if L == 2:
                row["whole_over_sparse_masked"] = res["whole_masked"][0] / res["sparse_masked"][0]
            row["frontier_plain_over_masked"] = res["frontier_plain"][0] / res["frontier_masked"][0]
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
