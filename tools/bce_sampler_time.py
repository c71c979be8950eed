#!/usr/bin/env python3
"""Multi-epoch BCE training on Epinion2 (tests/golden/epinion2_dataset.npz; d = 64, L = 3, 5 negatives per positive: 1 255 824
samples per epoch) with the epoch prepared on the host against drawn on the device, at B = 256 and B = 2 048: ms per epoch of
  (a) train_epochs with a LightTrainData: ng_sample() + the DataLoader's shuffle for the next epoch on a second host thread beside the
      current epoch's native call, three arrays uploaded per epoch,
  (b) train_epochs with a BceDeviceSampler: the whole window is one native call, every epoch drawn and shuffled by one kernel launch,
  (c) the native epoch alone: LightGCNStepper.epoch_bce over one pre-drawn device-resident epoch, again and again (the steps and
      nothing else: what (b) should cost).
Each window is --epochs epochs, wall clock around the call plus a final synchronisation; the forms ALTERNATE in one process over
--repeats windows after a warm-up window of each.  Also the samplers alone: epoch_arrays() on the host in ms per epoch (--repeats
calls after a first one), the kernel by device events (the mean of 50 launches after a warm-up launch).

usage: python tools/bce_sampler_time.py [--out FILE] [--B 256,2048] [--epochs 5] [--repeats 3]
Every B runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per B on stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, N_U, N_I = 3, 3186, 12407


def measure(B, epochs, repeats):
    import numpy as np
    import scipy.sparse as sp
    import torch
    for p in (ROOT, os.path.join(ROOT, "spex_amd", "dropin")):
        sys.path.insert(0, p)
    import utility1.dataloader as dl
    from spex_amd import ops
    from spex_amd.datasets import epinion2_tables, load_epinion2
    from spex_amd.graph import SpexGraph, lightgcn_norm_adj
    from spex_amd.trainer import BceDeviceSampler, LightGCNStepper, epoch_arrays, train_epochs
    if not torch.cuda.is_available():
        raise SystemExit("bce_sampler_time: needs a GPU (no CPU fallback: a CPU time says nothing)")
    dev = torch.device("cuda:0")
    train = load_epinion2()["train"]
    pairs = train[:, :2]
    csr = lightgcn_norm_adj(train[:, 0], train[:, 1], N_U - 1, N_I)
    E0 = np.concatenate(epinion2_tables(N_U, N_I, dim=64))
    graph = SpexGraph(*csr)
    stepper = lambda: LightGCNStepper(graph, torch.from_numpy(E0.copy()).to(dev), N_U, n_layers=L, lr=1e-3)
    np.random.seed(7)
    torch.manual_seed(7)
    mat = sp.csr_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(N_U, N_I)).todok()
    host_data = dl.LightTrainData(pairs.tolist(), N_I, mat)
    dev_sampler = BceDeviceSampler.from_train_data(host_data, n_users=N_U, seed=7, device=dev)
    fixed = dev_sampler.draw(0)                                  # (c)'s pre-drawn epoch
    legs = {"host_sampler": stepper(), "device_sampler": stepper(), "native_epoch_alone": stepper()}
    first = {"device_sampler": 0}

    def window(name, n_epochs):
        st = legs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "host_sampler":
            losses = train_epochs(st, host_data, n_epochs, batch_size=B)
        elif name == "device_sampler":
            losses = train_epochs(st, dev_sampler, n_epochs, batch_size=B, first_epoch=first[name])
            first[name] += n_epochs
        else:
            acc = torch.zeros(n_epochs, 2, 1, device=dev)
            for e in range(n_epochs):
                st.epoch_bce(*fixed, B, acc[e, 0], acc[e, 1])
            losses = None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n_epochs, losses

    for name in legs:                                           # warm-up: code objects, workspaces, descriptors, the pinned pools
        window(name, 2)
    out = {name: [] for name in legs}
    last_loss = {}
    for _ in range(repeats):
        for name in legs:                                       # the forms alternate inside every repeat
            ms, losses = window(name, epochs)
            out[name].append(ms)
            if losses is not None:
                last_loss[name] = losses[-1]
    # the samplers alone
    epoch_arrays(host_data)
    host_ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        epoch_arrays(host_data)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    bufs = dev_sampler.epoch_buffers()
    draw = lambda e: ops.sample_bce_epoch(dev_sampler.rowptr, dev_sampler.items, dev_sampler.pos_user, dev_sampler.pos_item, dev_sampler.num_ng, N_I,
                                          dev_sampler.seed, e, out=bufs)
    draw(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for e in range(50):
        draw(e + 1)
    e1.record()
    e1.synchronize()
    kernel_us = round(e0.elapsed_time(e1) * 1e3 / 50, 2)
    steps = -(-dev_sampler.n // B)
    res = {"B": B, "L": L, "d": 64, "samples_per_epoch": dev_sampler.n, "steps_per_epoch": steps, "epochs_per_window": epochs, "repeats": repeats}
    med = {}
    for name, xs in out.items():
        med[name] = sorted(xs)[len(xs) // 2]
        res[name + "_epoch_ms"] = [round(x, 2) for x in xs]
        res[name + "_epoch_median_ms"] = round(med[name], 2)
        res[name + "_epoch_spread_ms"] = round(max(xs) - min(xs), 2)
        res[name + "_us_per_step"] = round(med[name] * 1e3 / steps, 2)
        if name in last_loss:
            res[name + "_last_epoch_loss"] = round(last_loss[name], 4)
    res["last_epoch_loss_relative_difference"] = round(abs(last_loss["device_sampler"] - last_loss["host_sampler"]) / abs(last_loss["host_sampler"]), 5)
    res["host_epoch_arrays_alone_ms"] = [round(x, 2) for x in host_ms]
    res["device_sampler_kernel_us"] = kernel_us
    spread = max(res["host_sampler_epoch_spread_ms"], res["device_sampler_epoch_spread_ms"])
    res["device_not_slower_than_host_beyond_the_spread"] = bool(med["device_sampler"] - med["host_sampler"] <= spread)
    res["device_faster_by_more_than_both_spreads"] = bool(min(out["host_sampler"]) - max(out["device_sampler"]) > spread)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--B", default="256,2048")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one", type=int, help="(internal) measure this B in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds per B")
    a = ap.parse_args()
    if a.one is not None:
        return measure(a.one, a.epochs, a.repeats)
    for B in (int(w) for w in a.B.split(",")):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), "--epochs", str(a.epochs),
                            "--repeats", str(a.repeats)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bce_sampler_time: B = {B} ended with status {r.returncode}; nothing more is started")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
