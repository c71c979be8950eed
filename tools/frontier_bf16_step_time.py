#!/usr/bin/env python3
"""The four forms of the one-call exact training steps on ONE stepper (one arena, one set of moments), switched through
`stepper.frontier` and `stepper.gather_dtype` in alternating windows of one process:

    whole fp32 | whole bf16 (SPEX_STEP_BF16_GATHER) | frontier fp32 (SPEX_STEP_FRONTIER) | frontier bf16 (both flags)

The first three are code that predates the combined mode; the fourth is compared with frontier fp32 and with whole bf16 in the same
run.  Measured: the exact BCE step at B = 256 / 2 048 and the exact BPR step at T = 256 / 2 048 (whole-graph forms: push or dense by
the step's own choice; frontier forms: push at any T), L = 2 and 3, d = 64, on Epinion2 (cache-resident) or on
spex_amd.datasets.scaled_graph(K) (2^K nodes: HBM-resident from K = 22).  Graph, batches and timing are those of
tools/frontier_step_time.py: HIP events around a window of back-to-back steps, every figure the median over the windows with
(min, max) — a difference inside that spread is not a difference.  A switch to bf16 after fp32 steps re-casts the shadow once, in the
warm-up steps in front of the windows and in the first step of a bf16 window that follows an fp32 one (one streaming cast per
window, counted: that is what a schedule that switches pays).

usage: python tools/frontier_bf16_step_time.py --graph epinion2|22|24 [--windows 7] [--steps N] [--out profiles/frontier_bf16/timing.jsonl]"""
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

FORMS = {"whole_fp32": (False, None), "whole_bf16": (False, torch.bfloat16), "frontier_fp32": (True, None), "frontier_bf16": (True, torch.bfloat16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="epinion2")
    ap.add_argument("--windows", type=int, default=0, help="0: 7 on Epinion2 and at 2^22, 5 at 2^24")
    ap.add_argument("--steps", type=int, default=0, help="steps per window (0: 200 on Epinion2, 6 at 2^22, 4 at 2^24)")
    ap.add_argument("--layers", default="2,3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frontier_bf16_step_time.py: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    dev = torch.device("cuda:0")
    g, E0, n_u, rowptr = build(a.graph, dev)
    n = g.n_rows
    rng = np.random.default_rng(0)
    batches = {k: draw(rng, rowptr, n_u, n, k, dev) for k in (256, 2048)}
    labels = {k: (torch.rand(k, device=dev) < 1 / 6).float() for k in batches}
    acc = torch.zeros(1, device=dev)
    windows = a.windows or (5 if a.graph == "24" else 7)
    steps = a.steps or {"epinion2": 200, "24": 4}.get(a.graph, 6)
    for L in (int(x) for x in a.layers.split(",")):
        st = LightGCNStepper(g, E0.clone(), n_u, n_layers=L, lr=1e-3, weight_decay=1e-4, frontier=True)

        def run(form, kind, k):
            st.frontier, st.gather_dtype = FORMS[form]
            u, p, ng = batches[k]
            if kind == "bce":
                st.step_bce(u, p, labels[k], loss_acc=acc, batch_rows_only=True)
            else:
                st.step_bpr_exact(u, p, ng, loss_acc=acc, batch_rows_only=True)

        for kind, k in (("bce", 256), ("bce", 2048), ("bpr", 256), ("bpr", 2048)):
            res = alternate({f: (lambda f=f: run(f, kind, k)) for f in FORMS}, steps, windows, 2)
            f1 = st._front.counts.tolist()
            row = {"graph": a.graph, "n": n, "nnz": g.nnz, "L": L, "step": f"exact {kind.upper()} step, {'B' if kind == 'bce' else 'T'} = {k}",
                   "Bset_rows": f1[0], "F1_rows": f1[1], "windows": windows, "steps_per_window": steps}
            row.update({f + "_us": res[f] for f in FORMS})
            row["frontier_fp32_over_frontier_bf16"] = res["frontier_fp32"][0] / res["frontier_bf16"][0]
            row["whole_bf16_over_frontier_bf16"] = res["whole_bf16"][0] / res["frontier_bf16"][0]
            print(json.dumps(row), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
        assert torch.isfinite(st.E0).all()
        del st, run
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
