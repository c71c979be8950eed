#!/usr/bin/env python3
"""The one-call exact L = 2 frontier steps with row-sparse Adam (LightGCNStepper(frontier=True, sparse_adam=True),
SPEX_STEP_SPARSE_ADAM) against the same steps with dense Adam: one process, ONE graph handle, a dense-Adam frontier stepper and a
sparse-Adam one, their windows alternating.

Measured: the exact BCE step at B = 256 / 2 048 and the exact BPR step at T = 256 / 2 048, L = 2, d = 64, on Epinion2
(cache-resident) or on spex_amd.datasets.scaled_graph(K) (2^K nodes: HBM-resident from K = 22).  Every time includes every launch of
the step, the clears among them.  |F1| and |F2| of the configuration's batch are printed with it: the sparse form's Adam pass, clears
and loss sum cost |F2| rows, the dense form's N.  Timing: HIP events around a window of back-to-back steps; every figure is the
median over the windows with (min, max) — a difference inside that spread is not a difference.  --trace: no timing; three BCE steps
(B = 256) of the sparse form for a kernel trace taken around this script in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/sparse_adam_step_time.py --graph 24 --trace).

usage: python tools/sparse_adam_step_time.py --graph epinion2|22|24 [--windows 9] [--steps N] [--out profiles/sparse_adam/timing.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from frontier_step_time import alternate, build, draw  # noqa: E402
from spex_amd.trainer import LightGCNStepper  # noqa: E402

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="epinion2")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=0, help="steps per window (0: 400 on Epinion2, 6 on the scaled graphs)")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sparse_adam_step_time.py: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    dev = torch.device("cuda:0")
    g, E0, n_u, rowptr = build(a.graph, dev)
    n = g.n_rows
    rng = np.random.default_rng(0)
    batches = {k: draw(rng, rowptr, n_u, n, k, dev) for k in (256, 2048)}
    labels = {k: (torch.rand(k, device=dev) < 1 / 6).float() for k in batches}
    acc = torch.zeros(1, device=dev)
    make = lambda sparse: LightGCNStepper(g, E0.clone(), n_u, n_layers=2, lr=1e-3, weight_decay=1e-4, frontier=True, sparse_adam=sparse)
    if a.trace:
        st = make(True)
        u, p, _ = batches[256]
        for _ in range(3):
            st.step_bce(u, p, labels[256], loss_acc=acc, batch_rows_only=True)
        torch.cuda.synchronize()
        print("frontier rows |Bset|, |F1|, |F2|:", st._front.counts.tolist()[:3], "of", n)
        return
    steps = a.steps or (400 if a.graph == "epinion2" else 6)
    st = {"dense": make(False), "sparse": make(True)}
    rows = []
    for kind, k in (("bce", 256), ("bce", 2048), ("bpr", 256), ("bpr", 2048)):
        u, p, ng = batches[k]
        if kind == "bce":
            fns = {m: (lambda s=s: s.step_bce(u, p, labels[k], loss_acc=acc, batch_rows_only=True)) for m, s in st.items()}
        else:
            fns = {m: (lambda s=s: s.step_bpr_exact(u, p, ng, loss_acc=acc, batch_rows_only=True)) for m, s in st.items()}
        res = alternate(fns, steps, a.windows, 3)
        cnt = st["sparse"]._front.counts.tolist()
        row = {"graph": a.graph, "n": n, "nnz": g.nnz, "L": 2, "step": f"exact {kind.upper()} step, {'B' if kind == 'bce' else 'T'} = {k}",
               "Bset_rows": cnt[0], "F1_rows": cnt[1], "F2_rows": cnt[2], "F2_share": cnt[2] / n, "windows": a.windows,
               "steps_per_window": steps, "dense_adam_us": res["dense"], "sparse_adam_us": res["sparse"],
               "dense_over_sparse": res["dense"][0] / res["sparse"][0]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
