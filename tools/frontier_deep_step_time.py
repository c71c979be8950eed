#!/usr/bin/env python3
"""The exact L = 3 training steps with every launch over a device list (SPEX_STEP_FRONTIER_DEEP) against the forms the
project had: one process, ONE stepper built with frontier=True over a graph handle and its transposed handle, its forms switched
between windows that alternate:

  whole          the whole-graph one-call step (`stepper.frontier = False`)
  depth1         the frontier step (layer 2 and the product behind the batch kernel's push over F1; two whole-graph launches left)
  depth2         frontier_depth = 2 with dense Adam (no whole-graph launch; the clears and the Adam pass still walk whole tables)
  depth2_sparse  frontier_depth = 2 with row-sparse Adam over F3 (no launch walks a whole table)

A window is ONE native epoch call (epoch_bce / epoch_bpr) over `steps` copies of the batch, unmasked or at keep_prob < 1 (the in-kernel
sampled mask, a fresh seed per step).  Measured: the exact BCE step at B = 256 / 2 048 and the exact BPR step at T = 256 / 2 048, d = 64,
on Epinion2 (cache-resident) or spex_amd.datasets.scaled_graph(K) (2^K nodes: HBM-resident from K = 22).  HIP events around the window;
every figure is the median over the windows with (min, max) — a difference inside that spread is not a difference.  The row counts
are those of the window's last step.

--push-ab: instead, the two list-driven push kernels alone (spex_spmm_push_rows_f32 against spex_spmm_push_list_f32) over the F1 and
the F2 list of the B = 256 batch, masked and unmasked, alternating launches timed one by one.

usage: python tools/frontier_deep_step_time.py --graph epinion2|22|24 [--windows 7] [--steps N] [--keep-probs 1.0,0.3] [--push-ab]
                                               [--out profiles/frontier_deep/timing.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from frontier_dropout_step_time import load, transposed_handle, window_us  # noqa: E402
from frontier_step_time import draw  # noqa: E402
from spex_amd import ops  # noqa: E402
from spex_amd.graph import SpexGraph  # noqa: E402
from spex_amd.trainer import LightGCNStepper  # noqa: E402

FORMS = {"whole": (False, 1, False), "depth1": (True, 1, False), "depth2": (True, 2, False), "depth2_sparse": (True, 2, True)}


def push_ab(a, g, rowptr, n, n_u, batch, dev):
    """One row per (list, mask): microseconds per launch of either kernel, median (min, max) over alternating launches."""
    rows = []
    src, out = torch.randn(n, 64, device=dev), torch.zeros(n, 64, device=dev)
    rp = torch.as_tensor(np.asarray(rowptr), device=dev).long()
    for kp in (float(x) for x in a.keep_probs.split(",")):
        g.set_edge_mask(*((0,) if kp >= 1.0 else (2, None, kp, 12345)))
        fr = ops.FrontierRows(n, dev).update(batch[0], batch[1], 0, n_u).expand(g).expand2(g)
        counts = fr.counts.tolist()
        for name, cell in (("F1", fr.count_f), ("F2", fr.count_f2)):
            fns = {"push_rows": lambda: ops.spmm_push_rows(g, fr, src, out, True, count=cell),
                   "push_list": lambda: ops.spmm_push_list(g, fr, src, out, count=cell)}
            got = {k: [] for k in fns}
            for fn in fns.values():
                fn()
            for _ in range(a.windows):
                for k, fn in fns.items():
                    got[k].append(window_us(fn, 1))
            lst = fr.list[:cell.item()].long()
            row = {"graph": a.graph, "n": n, "keep_prob": kp, "list": name, "rows": cell.item(), "entries": int((rp[lst + 1] - rp[lst]).sum().item()),
                   "counts": counts, "launches": a.windows}
            for k, v in got.items():
                row[k + "_us"] = (float(np.median(v)), float(min(v)), float(max(v)))
            row["push_rows_over_push_list"] = row["push_rows_us"][0] / row["push_list_us"][0]
            rows.append(row)
            print(json.dumps(row), flush=True)
    g.set_edge_mask(0)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="epinion2")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=0, help="steps per window (0: 200 on Epinion2, 6 on the scaled graphs)")
    ap.add_argument("--keep-probs", default="1.0,0.3")
    ap.add_argument("--cells", default="bce:256,bce:2048,bpr:256,bpr:2048")
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--push-ab", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frontier_deep_step_time.py: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    dev = torch.device("cuda:0")
    csr, E0, n_u = load(a.graph, dev)
    rowptr = csr[0]
    g = SpexGraph(*csr, device=dev)
    n = g.n_rows
    rng = np.random.default_rng(0)
    cells = [(c.split(":")[0], int(c.split(":")[1])) for c in a.cells.split(",")]
    batches = {k: draw(rng, rowptr, n_u, n, k, dev) for k in sorted({k for _, k in cells} | {256})}
    rows = []
    if a.push_ab:
        rows = push_ab(a, g, rowptr, n, n_u, batches[256], dev)
    else:
        gt = transposed_handle(*csr, dev)
        steps = a.steps or (200 if a.graph == "epinion2" else 6)
        labels = {k: (torch.rand(k, device=dev) < 1 / 6).float() for k in batches}
        acc = torch.zeros(2, 1, device=dev)
        st = LightGCNStepper(g, E0.clone(), n_u, n_layers=3, lr=1e-3, weight_decay=1e-4, graph_t=gt, frontier=True)
        forms = {f: FORMS[f] for f in a.forms.split(",")}
        seed = [0]
        for kp in (float(x) for x in a.keep_probs.split(",")):
            for kind, k in cells:
                u, p, ng = (x.repeat(steps) for x in batches[k])
                y = labels[k].repeat(steps)

                def run(form):
                    frontier, depth, sparse = forms[form]
                    st.sparse_adam = False
                    st.frontier, st.frontier_depth = frontier, depth
                    st.sparse_adam = sparse
                    seed[0] += 1
                    if kind == "bce":
                        st.epoch_bce(u, p, y, k, acc[0], acc[1], keep_prob=kp, drop_seed=seed[0])
                    else:
                        st.epoch_bpr(u, p, ng, k, acc[0], acc[1], keep_prob=kp, drop_seed=seed[0])

                got, counts = {f: [] for f in forms}, {}
                for f in forms:
                    run(f)                                       # warm-up: allocations, the first touch of every table
                for _ in range(a.windows):
                    for f in forms:
                        got[f].append(window_us(lambda f=f: run(f), steps))
                        if forms[f][0]:
                            counts[f] = st._front.counts.tolist()
                row = {"graph": a.graph, "n": n, "nnz": g.nnz, "L": 3, "keep_prob": kp,
                       "step": f"exact {kind.upper()} step, {'B' if kind == 'bce' else 'T'} = {k}", "windows": a.windows, "steps_per_window": steps}
                if "depth2_sparse" in counts:
                    row["Bset_F1_F2_F3_rows"] = counts["depth2_sparse"]
                elif "depth2" in counts:
                    row["Bset_F1_F2_rows"] = counts["depth2"][:3]
                for f, v in got.items():
                    row[f + "_us"] = (float(np.median(v)), float(min(v)), float(max(v)))
                for f in ("depth2", "depth2_sparse"):
                    if f in got and "depth1" in got:
                        row["depth1_over_" + f] = row["depth1_us"][0] / row[f + "_us"][0]
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
