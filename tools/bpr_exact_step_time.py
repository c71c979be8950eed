#!/usr/bin/env python3
"""Step times of the exact BPR step (BPR through the propagation, L2, Adam) on Epinion2 (tests/golden/epinion2_dataset.npz), d = 64
(--recdim 128 / 256: the wide kernels), L = 3, weight_decay 1e-4, at T = 256 and T = 2 048: us per step of
  * the one-call step (LightGCNStepper.step_bpr_exact(.., loss_acc=.., batch_rows_only=True)), fast and deterministic,
  * the launch-by-launch step_bpr_exact (whole-graph propagation, dense scoring gradient, all-pull backward),
  * the native epoch (LightGCNStepper.epoch_bpr: one library call for the window), per step.
The forms ALTERNATE in one process: every repeat times one window of --steps steps of each form in turn, by device events (the
window's elapsed time on the GPU, host-bound gaps included), after a warm-up of each.  Three repeats by default; per form the
per-repeat figures, their median and their spread (max - min) are printed.  Triples: one bpr_epoch_triples draw from a fixed seed.

usage: python tools/bpr_exact_step_time.py [--out FILE] [--T 256,2048] [--steps 2000] [--repeats 3] [--recdim 64|128|256]
       python tools/bpr_exact_step_time.py --profile 256      (300 one-call steps and nothing else: for rocprofv3 --kernel-trace --stats)
       python tools/bpr_exact_step_time.py --sweep 256,512,1024,2048 [--out FILE]   (the fast path's push and dense forms, forced)
Every T runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per T on stdout."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, N_U, N_I, WD = 3, 3186, 12407, 1e-4
D = 64            # --recdim


def setup(T):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from spex_amd.datasets import epinion2_tables, load_epinion2
    from spex_amd.graph import SpexGraph, lightgcn_norm_adj
    from spex_amd.trainer import LightGCNStepper, bpr_epoch_triples
    if not torch.cuda.is_available():
        raise SystemExit("bpr_exact_step_time: needs a GPU (no CPU fallback: a CPU time says nothing)")
    dev = torch.device("cuda:0")
    train = load_epinion2()["train"]
    csr = lightgcn_norm_adj(train[:, 0], train[:, 1], N_U - 1, N_I)
    E0 = np.concatenate(epinion2_tables(N_U, N_I, dim=D))
    arrays = bpr_epoch_triples(train[:, :2], N_U, N_I, np.random.default_rng(7))
    dev_arrays = tuple(torch.from_numpy(a).to(dev) for a in arrays)
    graph = SpexGraph(*csr)

    def stepper(deterministic=False):
        return LightGCNStepper(graph, torch.from_numpy(E0.copy()).to(dev), N_U, n_layers=L, lr=1e-3, deterministic=deterministic,
                               weight_decay=WD)
    return torch, dev, dev_arrays, stepper


def measure(T, steps, repeats):
    torch, dev, (u_d, p_d, n_d), stepper = setup(T)
    n_batches = u_d.numel() // T
    acc = torch.zeros(2, 1, device=dev)

    def steps_leg(st, one_call):
        def run(k0, count):
            for s in range(k0, k0 + count):
                o = (s % n_batches) * T
                st.step_bpr_exact(u_d[o:o + T], p_d[o:o + T], n_d[o:o + T], loss_acc=acc[0], batch_rows_only=one_call)
        return run

    def epoch_leg(st):
        def run(k0, count):
            while count > 0:                                    # one library call per pass over the drawn triples
                k = min(count, n_batches)
                st.epoch_bpr(u_d, p_d, n_d, T, acc[0], acc[1], max_steps=k)
                count -= k
        return run

    legs = {"one_call_step_us": steps_leg(stepper(), True), "launch_by_launch_step_us": steps_leg(stepper(), False),
            "one_call_deterministic_step_us": steps_leg(stepper(True), True), "native_epoch_step_us": epoch_leg(stepper())}
    for run in legs.values():                                   # warm-up: code objects, workspaces, descriptors
        run(0, 200)
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for r in range(repeats):
        for name, run in legs.items():                          # the forms alternate inside every repeat
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(200 + r * steps, steps)
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / steps)
    res = {"T": T, "L": L, "d": D, "weight_decay": WD, "steps_per_window": steps, "repeats": repeats}
    for name, xs in out.items():
        res[name] = [round(x, 2) for x in xs]
        res[name.replace("_us", "_median_us")] = round(sorted(xs)[len(xs) // 2], 2)
        res[name.replace("_us", "_spread_us")] = round(max(xs) - min(xs), 2)
    print(json.dumps(res), flush=True)


def sweep(T, steps, repeats):
    """The fast path's two forms at one T, forced and alternating: push (first backward product pushed from the batch kernel, L - 1
    pull products) against dense (gradient rows into g_out, L pull products).  What the step's threshold constant is fixed from."""
    torch, dev, (u_d, p_d, n_d), stepper = setup(T)
    n_batches = u_d.numel() // T
    acc = torch.zeros(1, device=dev)
    sts = {}
    for form in ("push", "dense"):
        sts[form] = stepper()
        sts[form].bpr_backward = form

    def run(st, k0, count):
        for s in range(k0, k0 + count):
            o = (s % n_batches) * T
            st.step_bpr_exact(u_d[o:o + T], p_d[o:o + T], n_d[o:o + T], loss_acc=acc, batch_rows_only=True)

    for st in sts.values():
        run(st, 0, 200)
    torch.cuda.synchronize()
    out = {k: [] for k in sts}
    for r in range(repeats):
        for form, st in sts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(st, 200 + r * steps, steps)
            e1.record()
            e1.synchronize()
            out[form].append(round(e0.elapsed_time(e1) * 1e3 / steps, 2))
    res = {"T": T, "L": L, "steps_per_window": steps, "push_step_us": out["push"], "dense_step_us": out["dense"]}
    if D != 64:
        res["d"] = D
    print(json.dumps(res), flush=True)


def profile(T):
    torch, dev, (u_d, p_d, n_d), stepper = setup(T)
    st, acc = stepper(), torch.zeros(1, device=dev)
    for s in range(300):
        o = (s % (u_d.numel() // T)) * T
        st.step_bpr_exact(u_d[o:o + T], p_d[o:o + T], n_d[o:o + T], loss_acc=acc, batch_rows_only=True)
    torch.cuda.synchronize()
    print(json.dumps({"T": T, "steps": 300, "loss_sum": acc.item()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--T", default="256,2048")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one", type=int, help="(internal) measure this T in this process")
    ap.add_argument("--profile", type=int, help="300 one-call steps at this T, nothing else")
    ap.add_argument("--sweep", help="comma-separated T: the push and the dense form of the fast path, forced, alternating")
    ap.add_argument("--one-sweep", type=int, help="(internal) sweep this T in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds per T")
    ap.add_argument("--recdim", type=int, default=64, choices=(64, 128, 256), help="embedding width")
    a = ap.parse_args()
    global D
    D = a.recdim
    if a.profile is not None:
        return profile(a.profile)
    if a.one is not None:
        return measure(a.one, a.steps, a.repeats)
    if a.one_sweep is not None:
        return sweep(a.one_sweep, a.steps, a.repeats)
    child = "--one-sweep" if a.sweep else "--one"
    for T in (int(w) for w in (a.sweep or a.T).split(",")):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), child, str(T), "--steps", str(a.steps),
                            "--repeats", str(a.repeats), "--recdim", str(D)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bpr_exact_step_time: T = {T} ended with status {r.returncode}; nothing more is started")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
