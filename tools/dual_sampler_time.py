#!/usr/bin/env python3
"""Multi-epoch dual-task training (main_auto_expert_s.py: BASELINE config 5) on Epinion2 (tests/golden/epinion2_dataset.npz and
trust_epinion2_paths.npz; d = 64, L = 3, 5 negatives per positive: 1 255 824 samples and 27 004 trust paths per epoch) with the epoch
prepared on the host against drawn on the device, at B = 256 and B = 2 048 (cap = 3 x (paths // batches), the driver's rule: 15 and
129): ms per epoch of
  (a) train_epochs_dual with a LightTrainData: ng_sample(), the shuffle, the per-batch random.sample path cuts and the gathers for
      the next epoch on a second host thread beside the current epoch's native call, six arrays uploaded per epoch,
  (b) train_epochs_dual with a DualDeviceSampler: two launches per epoch on the sampler's stream beside the previous epoch's steps,
      one native call per epoch over the sampler's buffers, the counts the only thing the host waits for,
  (c) the native epoch alone: DualTaskStepper.epoch_strided over one pre-drawn device-resident epoch, again and again (the steps and
      nothing else: what (b) should cost).
Each window is --epochs epochs, wall clock around the call plus a final synchronisation; the forms ALTERNATE in one process over
--repeats windows after a warm-up window of each.  Also the samplers alone: epoch_arrays_dual() on the host in ms per epoch
(--repeats calls after a first one), the two kernels by device events (the mean of 50 launches after a warm-up launch).

usage: python tools/dual_sampler_time.py [--out FILE] [--B 256,2048] [--epochs 3] [--repeats 3]
Every B runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per B on stdout."""
import argparse
import collections
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_U = 3186


def measure(B, epochs, repeats):
    import numpy as np
    import torch
    for p in (ROOT, os.path.join(ROOT, "spex_amd", "dropin")):
        sys.path.insert(0, p)
    sys.argv = sys.argv[:1]
    import lg_parser
    import utility1.dataloader as dl
    import utility1.model_expert_s as mex
    import utility1.utils as utils
    from utility2.utils import Data
    from spex_amd import ops
    from spex_amd.datasets import materialise_epinion2
    from spex_amd.trainer import DualDeviceSampler, DualTaskStepper, epoch_arrays_dual, train_epochs_dual
    if not torch.cuda.is_available():
        raise SystemExit("dual_sampler_time: needs a GPU (no CPU fallback: a CPU time says nothing)")
    dev = torch.device("cuda:0")
    args = lg_parser.parse_args_r(["--dataset", "epinion2", "--data_path", materialise_epinion2(tempfile.mkdtemp())])
    dataset = dl.Loader(args)
    t = np.load(os.path.join(ROOT, "tests", "golden", "trust_epinion2_paths.npz"))
    raw = ([r[:l].tolist() for r, l in zip(t["train_paths"].astype(np.int64), t["train_len"])], t["train_targets"].astype(np.int64).tolist())
    trust = Data(raw, dataset.n_users, shuffle=False)
    by_user = collections.defaultdict(list)
    for k, p in enumerate(raw[0]):
        by_user[p[0]].append(k)
    host_data = dl.LightTrainData(dataset.rec_train_data, dataset.m_item, dataset.train_mat)
    n = len(host_data._ps) * (1 + host_data.num_ng)
    steps = -(-n // B)
    cap = 3 * max(1, len(raw[0]) // steps)

    def stepper():
        utils.set_seed(args.seed)
        net = mex.LightGCN(args, dataset).to(dev)
        return DualTaskStepper(net, path_capacity=cap, path_len=trust.len_max, lr=args.lr, batch_capacity=B)

    utils.set_seed(7)
    dev_sampler = DualDeviceSampler.from_train_data(host_data, trust, cap, B, n_users=N_U, seed=7, device=dev)
    fixed = dev_sampler.draw(0)                                  # (c)'s pre-drawn epoch
    fixed_counts = fixed[6].cpu().numpy()
    legs = {"host_thread": stepper(), "device_sampler": stepper(), "native_epoch_alone": stepper()}
    first = {"device_sampler": 0}

    def window(name, n_epochs):
        st = legs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "host_thread":
            losses = train_epochs_dual(st, host_data, trust, by_user, cap, n_epochs, batch_size=B)
        elif name == "device_sampler":
            losses = train_epochs_dual(st, dev_sampler, n_epochs, first_epoch=first[name])
            first[name] += n_epochs
        else:
            for _ in range(n_epochs):
                st.loss_acc.zero_()
                st.epoch_strided(fixed[0], fixed[1], fixed[2], B, fixed[3], fixed[4], fixed[5], cap, fixed_counts)
                st.join()
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
                last_loss[name] = [float(x) for x in losses[-1]]
    # the samplers alone
    epoch_arrays_dual(host_data, trust, by_user, cap, B)
    host_ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        epoch_arrays_dual(host_data, trust, by_user, cap, B)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    s, b = dev_sampler, dev_sampler.bce
    draws = {"bce_epoch_kernel_us": lambda e: ops.sample_bce_epoch(b.rowptr, b.items, b.pos_user, b.pos_item, b.num_ng, b.n_items, s.seed, e, out=fixed[:3]),
             "path_kernel_us": lambda e: ops.sample_dual_task_paths(fixed[0], B, s.path_rowptr, s.path_idx, s.paths, s.path_l, s.path_tgt, cap, s.seed, e,
                                                                    out=fixed[3:])}
    kernel_us = {}
    for name in ("path_kernel_us", "bce_epoch_kernel_us"):      # (the path kernel first: over the users of the pre-drawn epoch)
        draws[name](0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for e in range(50):
            draws[name](e + 1)
        e1.record()
        e1.synchronize()
        kernel_us[name] = round(e0.elapsed_time(e1) * 1e3 / 50, 2)
    res = {"B": B, "L": int(legs["host_thread"].L), "d": 64, "cap": cap, "samples_per_epoch": n, "steps_per_epoch": steps, "paths": len(raw[0]),
           "mean_paths_per_step": round(float(fixed_counts.mean()), 2), "epochs_per_window": epochs, "repeats": repeats}
    med = {}
    for name, xs in out.items():
        med[name] = sorted(xs)[len(xs) // 2]
        res[name + "_epoch_ms"] = [round(x, 2) for x in xs]
        res[name + "_epoch_median_ms"] = round(med[name], 2)
        res[name + "_epoch_spread_ms"] = round(max(xs) - min(xs), 2)
        res[name + "_us_per_step"] = round(med[name] * 1e3 / steps, 2)
        if name in last_loss:
            res[name + "_last_epoch_losses"] = [round(x, 4) for x in last_loss[name]]
    res["host_epoch_arrays_dual_alone_ms"] = [round(x, 2) for x in host_ms]
    res.update(kernel_us)
    res["device_not_slower_than_host_beyond_its_spread"] = bool(med["device_sampler"] - med["host_thread"] <= res["device_sampler_epoch_spread_ms"])
    res["device_above_the_floor_ms"] = round(med["device_sampler"] - med["native_epoch_alone"], 2)
    res["device_above_the_floor_beyond_its_spread"] = bool(res["device_above_the_floor_ms"] > res["device_sampler_epoch_spread_ms"])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--B", default="256,2048")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one", type=int, help="(internal) measure this B in this process")
    ap.add_argument("--limit", type=int, default=300, help="seconds per B")
    a = ap.parse_args()
    if a.one is not None:
        return measure(a.one, a.epochs, a.repeats)
    for B in (int(w) for w in a.B.split(",")):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), "--epochs", str(a.epochs),
                            "--repeats", str(a.repeats)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"dual_sampler_time: B = {B} ended with status {r.returncode}; nothing more is started")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
