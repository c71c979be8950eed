"""The one-call BPR step on Epinion2 (d = 64) with its last layer inside the BPR launch (SPEX_STEP_FUSED_LAST=1) against the
whole-graph schedule (=0): us per step by HIP events, both forms forced, over a sweep of batch sizes T — the measurement the
constant of step_fuses_last (spex_amd/csrc/spmm.hip) is fixed from.  One JSON line per (L, T).
usage: python tools/fused_last_time.py [--layers 3] [--T 256 1024 2048 4096 8192] [--steps 400] [--reps 5] [--batch bench|light|heavy]
SPEX_LIB=<path> times another build of the library.
--batch shapes the triples by the number S of 64-entry segments behind each 4-triple workgroup of the fused launch (12 slot rows;
16 waves, so S <= 16 is one pass of Phase A and S > 16 two): `bench` (default) draws users and items uniformly; `light` gives every
workgroup S <= 16 and `heavy` 17 <= S <= 28, both with the SAME list of entries per workgroup (each workgroup within 2 % of its
target), whose total is the uniform batch's to within a few percent.  The segment histogram of the batch is printed to stderr and kept in the row."""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if os.environ.get("SPEX_LIB"):
    from spex_amd import _lib as _l
    _l.LIB_PATH = os.path.abspath(os.environ["SPEX_LIB"])
from spex_amd.datasets import load_epinion2, xavier_uniform_np
from spex_amd.graph import SpexGraph, lightgcn_norm_adj
from spex_amd.trainer import LightGCNStepper
dev = torch.device("cuda:0")


def timed(fn, n, reps):
    """us per call: median and minimum over `reps` timed regions of n calls."""
    for _ in range(30): fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    return float(np.median(out)), float(min(out))


def group_shapes(deg, n_u, tu, tp, tn):
    """(entries, segments) behind every 4-triple workgroup: rows cut into 64-entry segments the way the kernel cuts them."""
    d = np.stack([deg[tu], deg[n_u + 1 + tp], deg[n_u + 1 + tn]], 1)
    return d.reshape(-1, 12).sum(1), ((d + 63) // 64).reshape(-1, 12).sum(1)


def draw_batch(kind, T, deg, n_u, n_i, rng):
    """T triples (T a multiple of 4 unless kind == 'bench').  light / heavy: a pool of candidate workgroups — a third drawn uniformly, two thirds
    with rows weighted towards full last segments (light) or nearly empty ones (heavy), so that either class reaches every target — is
    filtered by S, and workgroup k takes the unused candidate whose entry count is nearest to target k.  The targets are a uniform
    batch's entries per workgroup, clipped to 385 .. 450: the range both classes reach on Epinion2 (S >= 17 takes five rows beyond 64
    entries, S <= 16 forbids much more), with bounds that keep the sum within 1 % of the uniform batch's.  A heavy batch leans on the
    users of 65 .. 76 entries, so it names fewer distinct rows (the row reports `distinct_rows`): more same-row atomics than light."""
    tu, tp, tn = (rng.integers(0, hi, T) for hi in (n_u, n_i, n_i))
    if kind == "bench":
        return tu, tp, tn
    assert T % 4 == 0, "--batch light / heavy shape whole workgroups: T must be a multiple of 4"
    E, _ = group_shapes(deg, n_u, tu, tp, tn)
    target = np.clip(E, 385, 450)
    fill = deg / np.maximum(64 * ((deg + 63) // 64), 1)              # how full a row's segments are
    over = (deg > 0) & ((deg - 1) % 64 < 12)                         # a last segment of at most 12 entries: the cheapest segments
    ws = [np.ones(len(deg)), np.where(deg > 0, fill ** 4 if kind == "light" else (1.0 - fill) ** 2, 0.0) + 1e-3,
          (fill ** 8 if kind == "light" else over.astype(float)) + 1e-3]
    part = 4 * 200000
    cu = np.concatenate([rng.choice(n_u, part, p=w[:n_u] / w[:n_u].sum()) for w in ws])
    cp = np.concatenate([rng.choice(n_i, part, p=w[n_u + 1:] / w[n_u + 1:].sum()) for w in ws])
    cn = np.concatenate([rng.choice(n_i, part, p=w[n_u + 1:] / w[n_u + 1:].sum()) for w in ws])
    Ec, Sc = group_shapes(deg, n_u, cu, cp, cn)
    ok = np.flatnonzero(Sc <= 16 if kind == "light" else (Sc >= 17) & (Sc <= 28))
    ok = ok[np.argsort(Ec[ok], kind="stable")]
    Es, used, pick = Ec[ok], np.zeros(len(ok), bool), []
    for t in target:
        i = int(np.clip(np.searchsorted(Es, t), 0, len(Es) - 1))
        lo, hi = i, i
        while used[lo] and lo > 0: lo -= 1
        while used[hi] and hi < len(Es) - 1: hi += 1
        cand = [c for c in (lo, hi) if not used[c]]
        j = min(cand, key=lambda c: abs(int(Es[c]) - int(t)))
        assert abs(int(Es[j]) - int(t)) <= 0.02 * t, (kind, int(t), int(Es[j]))
        used[j] = True
        pick.append(ok[j])
    g = (4 * np.array(pick)[:, None] + np.arange(4)[None, :]).ravel()
    return cu[g], cp[g], cn[g]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, nargs="+", default=[3])
    ap.add_argument("--T", type=int, nargs="+", default=[256, 1024, 2048, 4096, 8192])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", choices=["bench", "light", "heavy"], default="bench")
    a = ap.parse_args()
    tr = load_epinion2()["train"]
    n_u, n_i = 3185, 12407
    csr = lightgcn_norm_adj(tr[:, 0], tr[:, 1], n_u, n_i)
    deg = np.diff(csr[0])
    g = SpexGraph(*csr, device=dev)
    rng = np.random.default_rng(13)
    E0 = torch.from_numpy(np.concatenate([xavier_uniform_np(n_u + 1, 64, rng), xavier_uniform_np(n_i, 64, rng)])).to(dev)
    for L in a.layers:
        for T in a.T:
            hu, hp, hn = draw_batch(a.batch, T, deg, n_u, n_i, rng)
            tu, tp, tn = (torch.from_numpy(h).to(dev) for h in (hu, hp, hn))
            row = {"graph": "epinion2", "n_rows": n_u + 1 + n_i, "L": L, "T": T}
            if a.batch != "bench" or T % 4 == 0:
                E, S = group_shapes(deg, n_u, hu, hp, hn)
                hist = np.bincount(S)
                row.update(batch=a.batch, entries=int(E.sum()), entries_per_wg={"p10": int(np.percentile(E, 10)), "median": int(np.median(E)),
                           "p90": int(np.percentile(E, 90)), "max": int(E.max())}, distinct_rows=len(set(hu) | set(n_u + 1 + hp) | set(n_u + 1 + hn)),
                           segments={"mean": round(float(S.mean()), 2), "max": int(S.max()), "wg_le16": int((S <= 16).sum()),
                                     "wg_gt16": int((S > 16).sum()), "hist": {str(k): int(v) for k, v in enumerate(hist) if v}})
                print("batch %s T %d: %d entries, segments per workgroup %s" % (a.batch, T, E.sum(), row["segments"]), file=sys.stderr)
            for form in ("0", "1"):
                os.environ["SPEX_STEP_FUSED_LAST"] = form
                st = LightGCNStepper(g, E0.clone(), n_u + 1, n_layers=L, lr=1e-3)
                med, best = timed(lambda: st.step_bpr_sgd(tu, tp, tn), a.steps, a.reps)
                row["fused_us" if form == "1" else "whole_graph_us"] = {"median": round(med, 2), "min": round(best, 2)}
            del os.environ["SPEX_STEP_FUSED_LAST"]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
