#!/usr/bin/env python3
"""Multi-epoch exact BPR training on Epinion2 (tests/golden/epinion2_dataset.npz; d = 64, L = 3, weight_decay 1e-4) with the triples
drawn on the host against drawn on the device, at T = 256 and T = 2 048: ms per epoch of
  (a) train_epochs_bpr with the host sampler (bpr_epoch_triples over a numpy Generator): the next epoch's draw on a second thread
      beside the current epoch's native call,
  (b) train_epochs_bpr with a BprDeviceSampler: the whole window is one native call, every epoch's triples drawn by a kernel.
Each window is --epochs epochs, wall clock around the call plus a final synchronisation; the two forms ALTERNATE in one process over
--repeats windows after a warm-up window of each.  Also the samplers alone: the host sampler in ms per epoch (--repeats calls after a
first one), the kernel by device events (the mean of 50 launches after a warm-up launch, both laws).

usage: python tools/bpr_sampler_time.py [--out FILE] [--T 256,2048] [--epochs 10] [--repeats 3]
Every T runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per T on stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, N_U, N_I, WD = 3, 3186, 12407, 1e-4


def measure(T, epochs, repeats):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from spex_amd.datasets import epinion2_tables, load_epinion2
    from spex_amd.graph import SpexGraph, lightgcn_norm_adj
    from spex_amd.trainer import BprDeviceSampler, LightGCNStepper, bpr_epoch_triples, train_epochs_bpr
    if not torch.cuda.is_available():
        raise SystemExit("bpr_sampler_time: needs a GPU (no CPU fallback: a CPU time says nothing)")
    dev = torch.device("cuda:0")
    train = load_epinion2()["train"]
    pairs = train[:, :2]
    csr = lightgcn_norm_adj(train[:, 0], train[:, 1], N_U - 1, N_I)
    E0 = np.concatenate(epinion2_tables(N_U, N_I, dim=64))
    graph = SpexGraph(*csr)
    stepper = lambda: LightGCNStepper(graph, torch.from_numpy(E0.copy()).to(dev), N_U, n_layers=L, lr=1e-3, weight_decay=WD)
    rng = np.random.default_rng(7)
    host_sampler = lambda: bpr_epoch_triples(pairs, N_U, N_I, rng)
    dev_sampler = BprDeviceSampler(pairs, N_U, N_I, dev, seed=7)
    legs = {"host_sampler": (stepper(), host_sampler), "device_sampler": (stepper(), dev_sampler)}
    first = {"host_sampler": 0, "device_sampler": 0}

    def window(name, n_epochs):
        st, sampler = legs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kw = {"first_epoch": first[name]} if name == "device_sampler" else {}
        losses = train_epochs_bpr(st, sampler, n_epochs, batch_size=T, **kw)
        torch.cuda.synchronize()
        first[name] += n_epochs
        return (time.perf_counter() - t0) * 1e3 / n_epochs, losses

    for name in legs:                                           # warm-up: code objects, workspaces, descriptors, the pinned pools
        window(name, 2)
    out = {name: [] for name in legs}
    last_loss = {}
    for _ in range(repeats):
        for name in legs:                                       # the forms alternate inside every repeat
            ms, losses = window(name, epochs)
            out[name].append(ms)
            last_loss[name] = losses[-1]
    # the samplers alone
    host_sampler()
    host_ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        host_sampler()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    kernel_us = {}
    for by in ("user", "interaction"):
        s = BprDeviceSampler(pairs, N_U, N_I, dev, seed=7, by=by)
        bufs = s.epoch_buffers()
        from spex_amd import ops
        draw = lambda e: ops.sample_bpr_triples(s.rowptr, s.items, s.active, N_I, s.n, s.seed, e, by=by, out=bufs)
        draw(0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for e in range(50):
            draw(e + 1)
        e1.record()
        e1.synchronize()
        kernel_us[by] = round(e0.elapsed_time(e1) * 1e3 / 50, 2)
    steps = -(-len(pairs) // T)
    res = {"T": T, "L": L, "d": 64, "weight_decay": WD, "triples_per_epoch": len(pairs), "steps_per_epoch": steps, "epochs_per_window": epochs,
           "repeats": repeats}
    for name, xs in out.items():
        res[name + "_epoch_ms"] = [round(x, 2) for x in xs]
        res[name + "_epoch_median_ms"] = round(sorted(xs)[len(xs) // 2], 2)
        res[name + "_epoch_spread_ms"] = round(max(xs) - min(xs), 2)
        res[name + "_last_epoch_loss"] = round(last_loss[name], 4)
    res["host_sampler_alone_ms"] = [round(x, 2) for x in host_ms]
    res["device_sampler_kernel_us"] = kernel_us
    res["device_faster_by_more_than_the_spread"] = bool(min(out["host_sampler"]) - max(out["device_sampler"])
                                                        > max(res["host_sampler_epoch_spread_ms"], res["device_sampler_epoch_spread_ms"]))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--T", default="256,2048")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one", type=int, help="(internal) measure this T in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds per T")
    a = ap.parse_args()
    if a.one is not None:
        return measure(a.one, a.epochs, a.repeats)
    for T in (int(w) for w in a.T.split(",")):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(T), "--epochs", str(a.epochs),
                            "--repeats", str(a.repeats)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bpr_sampler_time: T = {T} ended with status {r.returncode}; nothing more is started")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
