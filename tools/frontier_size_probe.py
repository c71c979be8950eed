#!/usr/bin/env python3
"""What a training batch can reach, counted on the CPU (no GPU): the rows and stored entries of the batch's rows (Bset), of Bset and
its neighbours (F1, the frontier SPEX_STEP_FRONTIER works on) and of two hops, on Epinion2 and spex_amd.datasets.scaled_graph(K).
The batch counted is a BCE batch of B samples as an epoch holds them (draw_batch: one positive to five negatives; a positive is a
uniformly drawn training pair, so its item is degree-weighted; a negative's item is uniform); the entries of a row set are the gathers
a row-list launch over it would issue.  One JSON line per (graph, batch); --markdown prints the table of DESIGN.md 4.20.
--keep-prob P (< 1): beside them the sets of the same batch under edge dropout — every stored entry kept with
probability P (a seeded Bernoulli draw per entry: the sizes do not depend on which generator draws it), F1 = Bset U the columns of the
KEPT entries of Bset's rows, F2 likewise from F1; --markdown then prints the masked beside the unmasked rows.

usage: python tools/frontier_size_probe.py [--graphs epinion2,20,22] [--batches 256,2048] [--keep-prob 0.3] [--markdown]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spex_amd.datasets import load_epinion2, scaled_graph  # noqa: E402
from spex_amd.graph import lightgcn_norm_adj  # noqa: E402


def graph(which):
    if which == "epinion2":
        n_u, n_i = 3186, 12407
        tr = load_epinion2()["train"]
        rowptr, col, _ = lightgcn_norm_adj(tr[:, 0], tr[:, 1], n_u - 1, n_i)
        return np.asarray(rowptr, np.int64), np.asarray(col), n_u
    rowptr, col, _, n_u = scaled_graph(int(which))
    return np.asarray(rowptr, np.int64), np.asarray(col), n_u


def neighbours(rowptr, col, rows, keep=None):
    """rows U their stored columns (keep given: the columns of their kept entries), sorted."""
    mark = np.zeros(len(rowptr) - 1, bool)
    mark[rows] = True
    lens = (rowptr[rows + 1] - rowptr[rows]).astype(np.int64)
    first = np.repeat(rowptr[rows] - (np.cumsum(lens) - lens), lens)        # entry index = position in the concatenation + this
    e = first + np.arange(int(lens.sum()), dtype=np.int64)
    if keep is not None:
        e = e[keep[e]]
    mark[col[e]] = True
    return np.flatnonzero(mark)


def draw_batch(rowptr, col, n_u, B, rng, num_ng=5):
    """B (user, item) samples as a BCE epoch holds them: a training pair drawn uniformly among the stored entries of the user rows
    (so its user is activity-weighted and its item degree-weighted), kept as a positive with probability 1 / (num_ng + 1), its item
    otherwise replaced by a uniform one (a negative of the same user)."""
    n = len(rowptr) - 1
    e = rng.integers(0, int(rowptr[n_u]), B)
    users = np.searchsorted(rowptr, e, side="right") - 1
    items = col[e].astype(np.int64) - n_u
    negative = rng.random(B) >= 1.0 / (num_ng + 1)
    items[negative] = rng.integers(0, n - n_u, int(negative.sum()))
    return users, items


def probe(which, B, seed=0, loaded=None, keep_prob=1.0, hops=2):
    rowptr, col, n_u = loaded or graph(which)
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    deg = np.diff(rowptr)
    users, items = draw_batch(rowptr, col, n_u, B, np.random.default_rng(seed))
    bset = np.unique(np.concatenate([users, items + n_u]))
    f1 = neighbours(rowptr, col, bset)
    f2 = neighbours(rowptr, col, f1)
    ent = lambda rows: int(deg[rows].sum())
    masked, deep = {}, {}
    if hops >= 3:               # the three-hop set: the rows a deep frontier step's gradient can touch (SPEX_STEP_FRONTIER_DEEP)
        f3 = neighbours(rowptr, col, f2)
        deep.update({"three_hop_rows": len(f3), "three_hop_entries": ent(f3), "three_hop_share_of_rows": len(f3) / n})
    if keep_prob < 1.0:
        keep = np.random.default_rng(seed + 101).random(nnz) < keep_prob
        f1m = neighbours(rowptr, col, bset, keep)
        f2m = neighbours(rowptr, col, f1m, keep)
        if hops >= 3:
            f3m = neighbours(rowptr, col, f2m, keep)
            masked.update({"three_hop_rows_masked": len(f3m), "three_hop_entries_masked": ent(f3m)})
        masked = {**masked, "keep_prob": keep_prob, "F1_rows_masked": len(f1m), "F1_entries_masked": ent(f1m), "two_hop_rows_masked": len(f2m),
                  "two_hop_entries_masked": ent(f2m)}
    return {**masked, **deep, "graph": which, "n": n, "nnz": nnz, "B": B, "Bset_rows": len(bset), "Bset_entries": ent(bset), "F1_rows": len(f1),
            "F1_entries": ent(f1), "F1_share_of_nnz": ent(f1) / nnz, "two_hop_rows": len(f2), "two_hop_entries": ent(f2),
            "two_hop_share_of_nnz": ent(f2) / nnz}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="epinion2,20,22")
    ap.add_argument("--batches", default="256")
    ap.add_argument("--keep-prob", type=float, default=1.0)
    ap.add_argument("--hops", type=int, default=2, choices=(2, 3), help="3: also |F3|, the three-hop set")
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    rows = []
    for g in a.graphs.split(","):
        loaded = graph(g)
        rows += [probe(g, int(b), loaded=loaded, keep_prob=a.keep_prob, hops=a.hops) for b in a.batches.split(",")]
    if not a.markdown:
        for r in rows:
            print(json.dumps(r))
        return
    k = lambda x: f"{x / 1e6:.2f} M" if x >= 1e6 else (f"{x / 1e3:.1f} k" if x >= 1e4 else str(x))
    if a.hops >= 3:
        m = a.keep_prob < 1.0
        print("| graph | batch | batch rows | F1 rows | F2 rows | F3 rows (share of N) |" + (f" F1 / F2 / F3 rows at keep_prob {a.keep_prob:g} |" if m else ""))
        print("|---|---|---|---|---|---|" + ("---|" if m else ""))
        for r in rows:
            print(f"| {r['graph']} (N {r['n']}, nnz {k(r['nnz'])}) | B = {r['B']} | {r['Bset_rows']} | {k(r['F1_rows'])} | {k(r['two_hop_rows'])} | "
                  f"{k(r['three_hop_rows'])} ({100 * r['three_hop_share_of_rows']:.0f} %) |"
                  + (f" {k(r['F1_rows_masked'])} / {k(r['two_hop_rows_masked'])} / {k(r['three_hop_rows_masked'])} |" if m else ""))
        return
    if a.keep_prob < 1.0:
        print(f"| graph | batch | batch rows | F1 rows: unmasked / keep_prob {a.keep_prob:g} | F2 rows: unmasked / keep_prob {a.keep_prob:g} |")
        print("|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['graph']} (N {r['n']}, nnz {k(r['nnz'])}) | B = {r['B']} | {r['Bset_rows']} | {k(r['F1_rows'])} / {k(r['F1_rows_masked'])} | "
                  f"{k(r['two_hop_rows'])} / {k(r['two_hop_rows_masked'])} |")
        return
    print("| graph | batch | batch rows / entries | + their neighbours: rows / entries (share of nnz) | two hops: rows / entries (share of nnz) |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['graph']} (N {r['n']}, nnz {k(r['nnz'])}) | B = {r['B']} | {r['Bset_rows']} / {k(r['Bset_entries'])} | "
              f"{k(r['F1_rows'])} / {k(r['F1_entries'])} ({100 * r['F1_share_of_nnz']:.1f} %) | "
              f"{k(r['two_hop_rows'])} / {k(r['two_hop_entries'])} ({100 * r['two_hop_share_of_nnz']:.0f} %) |")


if __name__ == "__main__":
    main()
