#!/usr/bin/env python3
"""Step and epoch times of the exact LightGCN BCE step at d = 64 / 128 / 256 on Epinion2 (tests/golden/epinion2_dataset.npz), B = 256,
L = 3: us per step of the one-call step (LightGCNStepper.step_bce(.., loss_acc=.., batch_rows_only=True) where the stepper takes it
in one library call) and of the launch-by-launch step (batch_rows_only=False), seconds per epoch of train_epoch's native branch (one
library call for the whole epoch) and of a Python loop over the same batches.  A form the stepper does not have at a width is
reported as null.  The epoch is the reference's size (every observed pair + five negatives: 4 906 batches), training-shaped (users
arrive in proportion to their degree), drawn from a fixed seed.

usage: python tools/wide_step_time.py [--out FILE] [--widths 64,128,256]
Every width runs in a child process of its own under a time limit; the first failure ends the run (nothing more is started on the
GPU).  One JSON line per width on stdout (and appended to FILE)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, N_U, N_I = 256, 3, 3186, 12407


def measure(d, steps, repeats):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from spex_amd.datasets import epinion2_tables, load_epinion2
    from spex_amd.graph import SpexGraph, lightgcn_norm_adj
    from spex_amd.trainer import LightGCNStepper, train_epoch
    if not torch.cuda.is_available():
        raise SystemExit("wide_step_time: needs a GPU (no CPU fallback: a CPU time says nothing)")
    dev = torch.device("cuda:0")
    train = load_epinion2()["train"]
    csr = lightgcn_norm_adj(train[:, 0], train[:, 1], N_U - 1, N_I)
    E0 = np.concatenate(epinion2_tables(N_U, N_I, dim=d))
    rng = np.random.default_rng(7)
    n = 6 * len(train)
    k = rng.integers(0, len(train), n)
    users, items = train[k, 0].astype(np.int64), train[k, 1].astype(np.int64)
    neg = rng.random(n) < 5 / 6
    items[neg] = rng.integers(0, N_I, int(neg.sum()))
    arrays = (users, items, (~neg).astype(np.float32))
    u_d, i_d, y_d = (torch.from_numpy(a).to(dev) for a in arrays)
    graph = SpexGraph(*csr)

    def stepper():
        return LightGCNStepper(graph, torch.from_numpy(E0.copy()).to(dev), N_U, n_layers=L, lr=1e-3)

    def step_us(st, rows_only):
        acc = torch.zeros(1, device=dev)
        def run(k0, count):
            for s in range(k0, k0 + count):
                o = (s % (n // B)) * B
                st.step_bce(u_d[o:o + B], i_d[o:o + B], y_d[o:o + B], loss_acc=acc, batch_rows_only=rows_only)
            torch.cuda.synchronize()
        run(0, 200)                                             # warm-up: code objects, workspaces, the descriptor
        out = []
        for r in range(repeats):
            t0 = time.perf_counter()
            run(200 + r * steps, steps)
            out.append((time.perf_counter() - t0) / steps * 1e6)
        return out

    def epoch_s(st, native):
        out = []
        for r in range(repeats + 1):                            # (the first epoch is the warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if native:
                train_epoch(st, None, batch_size=B, arrays=arrays)
            else:
                acc = torch.zeros(1, device=dev)
                for o in range(0, n, B):
                    st.step_bce(u_d[o:o + B], i_d[o:o + B], y_d[o:o + B], loss_acc=acc, batch_rows_only=True)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out[1:]

    st = stepper()
    one_call = bool(st._one_call_ok(u_d[:B], i_d[:B], y_d[:B]))
    res = {"d": d, "B": B, "L": L, "batches_per_epoch": (n + B - 1) // B, "steps_per_window": steps,
           "one_call_step_us": step_us(stepper(), True) if one_call else None,
           "launch_by_launch_step_us": step_us(stepper(), False),
           "native_epoch_s": epoch_s(stepper(), True) if one_call else None,
           "python_loop_epoch_s": epoch_s(stepper(), False),
           "python_loop_step_form": "one call per step" if one_call else "launch by launch"}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--widths", default="64,128,256")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one", type=int, help="(internal) measure this width in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds per width")
    a = ap.parse_args()
    if a.one is not None:
        return measure(a.one, a.steps, a.repeats)
    for d in (int(w) for w in a.widths.split(",")):
        # `timeout -k 10 LIMIT python tools/wide_step_time.py --one d`, the widths chained as with &&: a failure ends the run
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(d), "--steps", str(a.steps),
                            "--repeats", str(a.repeats)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"wide_step_time: d = {d} ended with status {r.returncode}; nothing more is started")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
