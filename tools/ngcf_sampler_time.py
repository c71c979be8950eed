#!/usr/bin/env python3
"""Multi-epoch single-layer NGCF training on Epinion2 (tests/golden/epinion2_dataset.npz in the drop-in's file format; 3 072 users per
epoch, 1 217 538 samples) with the epoch prepared on the host against drawn on the device, at B = 256 and B = 2 048: ms per epoch of
  (a) train_epochs_ngcf with a Data: Data.sample_epoch (the blocked replay of the `random` stream) + the DataLoader's shuffle for the
      next epoch on a second host thread beside the current epoch's native call, three arrays uploaded per epoch,
  (b) train_epochs_ngcf with an NgcfDeviceSampler: the whole window is one native call, every epoch drawn and shuffled by one kernel
      launch,
  (c) the native epoch alone: NGCFStepper.epoch over one pre-drawn device-resident epoch, again and again (the steps and nothing else:
      what (b) should cost).
Each window is --epochs epochs, wall clock around the call plus a final synchronisation; the forms ALTERNATE in one process, on ONE
stepper (see measure()), over --repeats windows after a warm-up window of each.  Also the samplers alone: epoch_arrays_ngcf() on the
host in ms per epoch (--repeats calls after a first one), the kernel by device events (the mean of 50 launches after a warm-up
launch).

usage: python tools/ngcf_sampler_time.py [--out FILE] [--B 256,2048] [--epochs 5] [--repeats 3] [--separate-steppers]
Every B runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per B on stdout."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_epinion2(root):
    """Epinion2 as NGCF's <root>/epinion2/rec/{train,test,negative}.txt (data_process_rec.py's format)."""
    import numpy as np
    e = np.load(os.path.join(ROOT, "tests", "golden", "epinion2_dataset.npz"))
    rec = os.path.join(root, "epinion2", "rec")
    os.makedirs(rec)
    pairs = e["train"].astype(np.int64)
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
    with open(os.path.join(rec, "train.txt"), "w") as f:
        users, start = np.unique(pairs[:, 0], return_index=True)
        for k, u in enumerate(users):
            end = start[k + 1] if k + 1 < len(users) else len(pairs)
            f.write(str(u) + "".join(" %d" % i for i in pairs[start[k]:end, 1]) + "\n")
    with open(os.path.join(rec, "test.txt"), "w") as f:
        for u, p in zip(e["test_users"].astype(int), e["test_pos"].astype(int)):
            f.write("%d %d\n" % (u, p))
    with open(os.path.join(rec, "negative.txt"), "w") as f:
        for u, negs in zip(e["test_users"].astype(int), e["test_neg"].astype(np.int64)):
            f.write(str(u) + "".join(" %d" % i for i in negs) + "\n")
    return os.path.join(root, "epinion2")


def measure(B, epochs, repeats, separate=False):
    import random
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.argv = [sys.argv[0]]                                     # (the drop-in's parser reads the command line at import)
    from spex_amd import ops
    from spex_amd.dropin.ngcf.utility.load_data import Data
    from spex_amd.ngcf import NGCF
    from spex_amd.trainer import NGCFStepper, NgcfDeviceSampler, epoch_arrays_ngcf, train_epochs_ngcf
    if not torch.cuda.is_available():
        raise SystemExit("ngcf_sampler_time: needs a GPU (no CPU fallback: a CPU time says nothing)")
    dev = torch.device("cuda:0")
    random.seed(7)
    np.random.seed(7)
    torch.manual_seed(7)
    data = Data(path=write_epinion2(tempfile.mkdtemp()), batch_size=B)
    _, norm, _ = data.get_adj_mat()
    args = argparse.Namespace(embed_size=64, layer_size="[64]", mess_dropout="[0.1]", regs="[1e-5]")

    def stepper():
        model = NGCF({"n_users": data.n_users, "n_items": data.n_items, "norm_adj": norm}, "cuda", args).to(dev)
        model.train()
        return NGCFStepper(model, lr=1e-3)

    dev_sampler = NgcfDeviceSampler(data, seed=7, device=dev)
    fixed = dev_sampler.draw(0)                                  # (c)'s pre-drawn epoch
    # ONE stepper serves all three legs.  Identical steppers built one after another differ among themselves by ~5 ms per epoch on the
    # same work, each repeating to 0.1 ms (where the allocator places a stepper's tables): with --separate-steppers the native epoch
    # alone took 78.73 ms on its stepper and 84.35 ms on the shared one at B = 2 048 (profiles/ngcf_sampler/) — more than what the legs
    # are compared for.  On one stepper the legs differ in where the epoch comes from and in nothing else.
    legs = ("host_sampler", "device_sampler", "native_epoch_alone")
    shared = None if separate else stepper()
    steppers = {name: shared or stepper() for name in legs}
    first = {"device_sampler": 0}

    def window(name, n_epochs):
        st = steppers[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "host_sampler":
            losses = train_epochs_ngcf(st, data, n_epochs, batch_size=B)
        elif name == "device_sampler":
            losses = train_epochs_ngcf(st, dev_sampler, n_epochs, batch_size=B, first_epoch=first[name])
            first[name] += n_epochs
        else:
            acc = torch.zeros(n_epochs, 2, 1, device=dev)
            for e in range(n_epochs):
                st.epoch(*fixed, B, acc[e, 0], acc[e, 1])
            losses = None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n_epochs, losses

    for name in legs:                                           # warm-up: code objects, descriptors, the pinned pools
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
    epoch_arrays_ngcf(data)
    host_ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        epoch_arrays_ngcf(data)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    bufs = dev_sampler.epoch_buffers()
    s = dev_sampler
    draw = lambda e: ops.sample_ngcf_epoch(s.pop, s.user, s.pos_off, s.pos_item, s.row_off, s.row_rank, s.seed, e, out=bufs)
    draw(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for e in range(50):
        draw(e + 1)
    e1.record()
    e1.synchronize()
    kernel_us = round(e0.elapsed_time(e1) * 1e3 / 50, 2)
    steps = -(-dev_sampler.n // B)
    res = {"B": B, "L": 1, "d": 64, "samples_per_epoch": dev_sampler.n, "steps_per_epoch": steps, "epochs_per_window": epochs, "repeats": repeats,
           "one_stepper_for_all_legs": not separate}
    med = {}
    for name, xs in out.items():
        med[name] = sorted(xs)[len(xs) // 2]
        res[name + "_epoch_ms"] = [round(x, 2) for x in xs]
        res[name + "_epoch_median_ms"] = round(med[name], 2)
        res[name + "_epoch_spread_ms"] = round(max(xs) - min(xs), 2)
        res[name + "_us_per_step"] = round(med[name] * 1e3 / steps, 2)
        if name in last_loss:
            res[name + "_last_epoch_loss"] = round(last_loss[name], 4)       # (one model trains on through every window)
    res["host_epoch_arrays_alone_ms"] = [round(x, 2) for x in host_ms]
    res["device_sampler_kernel_us"] = kernel_us
    # the acceptance: (b) within (c)'s measured spread plus the kernel's own time, and not slower than (a)
    allowance = res["native_epoch_alone_epoch_spread_ms"] + kernel_us * 1e-3
    res["device_minus_native_alone_ms"] = round(med["device_sampler"] - med["native_epoch_alone"], 2)
    res["device_within_native_alone_spread_plus_kernel"] = bool(med["device_sampler"] - med["native_epoch_alone"] <= allowance)
    res["device_not_slower_than_host"] = bool(med["device_sampler"] <= med["host_sampler"])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--B", default="256,2048")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one", type=int, help="(internal) measure this B in this process")
    ap.add_argument("--separate-steppers", action="store_true", help="a stepper of its own per leg (see measure())")
    ap.add_argument("--limit", type=int, default=240, help="seconds per B")
    a = ap.parse_args()
    if a.one is not None:
        return measure(a.one, a.epochs, a.repeats, a.separate_steppers)
    for B in (int(w) for w in a.B.split(",")):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), "--epochs", str(a.epochs),
                            "--repeats", str(a.repeats)] + (["--separate-steppers"] if a.separate_steppers else []), capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"ngcf_sampler_time: B = {B} ended with status {r.returncode}; nothing more is started")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
