"""Mean shift mode seeking on the device (pn_mean_shift_device_f32) against the route a caller had before.

For n x dim f32 blob rows (n / 1000 blobs of sigma 0.05 in the unit cube, a tenth of the rows uniform background), the
bandwidth h = 2 sigma sqrt(dim), and scikit-learn's bin seeds at bin size h (``mean_shift_bin_seeds``; when the grid gives
more than --max-seeds cells, an evenly strided subset of them).  In 16 and 128 dimensions nearly every row is a cell of
its own and a cell's centre lies up to h sqrt(dim) / 2 from its row, beyond every row's reach: when more than half of the
bin seeds are dead after one step, an evenly strided subset of the rows themselves are the seeds instead (what
scikit-learn does without bin seeding, subsampled), and ``seed_kind`` says so.  Interleaved in one process:
  * step: one iteration -- mean_shift_modes_device(max_iter = 1) against one iteration of the old route;
  * modes: a whole mean_shift_modes_device(tol = 1e-3 h) against the old route run for the same number of iterations.
The old route, per iteration and for ALL seeds: query_radius_device at h (capacity kept from the iteration before with a
quarter of slack, the total read back, the call repeated when it did not fit), then a torch segment mean in f64
(index_add_ of the listed rows, divided by the list lengths).  It has no stopping rule of its own here: it is given the
iteration count the new entry needed.  Recorded with the times: the seed-steps the new entry ran against seeds x
iterations, and the largest difference of a live seed's mode between the two routes.
--sklearn adds sklearn.cluster.MeanShift(bandwidth = h, seeds) on the host CPU (n_jobs = 16) at n <= 10^5.
Appends one JSON line to profiles/mean_shift_bench.jsonl (--out).
usage: python tools/bench_mean_shift.py [--reps 5] [--shapes 100000x2,100000x16,1000000x128] [--max-seeds 2048] [--sklearn]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petal_neighbors_amd as pn  # noqa: E402
from bench_mst import DEV, blob_rows, interleaved  # noqa: E402

SIGMA = 0.05


class OldRoute:
    """query_radius_device + a torch segment mean, every seed every iteration"""

    def __init__(self, tree, x, h):
        self.tree, self.x, self.h, self.cap = tree, x, h, 0

    def step(self, pos):
        ns = pos.shape[0]
        while True:
            off, idx, total = self.tree.query_radius_device(pos, self.h, max(self.cap, 1))
            tot = int(total.item())  # (the caller's round trip: did the lists fit?)
            if tot <= self.cap:
                break
            self.cap = tot + tot // 4
        lengths = off[1:] - off[:-1]
        seg = torch.repeat_interleave(torch.arange(ns, device=pos.device), lengths)
        sums = torch.zeros((ns, pos.shape[1]), dtype=torch.float64, device=pos.device)
        sums.index_add_(0, seg, self.x[idx[:tot]].double())
        new = (sums / lengths.clamp_min(1).double()[:, None]).float()
        return torch.where((lengths > 0)[:, None], new, pos)

    def run(self, seeds, iterations):
        pos = seeds
        for _ in range(iterations):
            pos = self.step(pos)
        return pos


def measure(n, dim, max_seeds, reps, with_sklearn):
    x = blob_rows(n, dim, max(1, n // 1000), SIGMA, 0.10, 3)
    h = 2.0 * SIGMA * math.sqrt(dim)
    xs = x.cpu().numpy()
    cells = pn.mean_shift_bin_seeds(xs, h, 1)
    n_cells = cells.shape[0]
    if n_cells > max_seeds:
        cells = cells[:: -(-n_cells // max_seeds)]
    seeds = torch.from_numpy(np.ascontiguousarray(cells, dtype=np.float32)).to(DEV)
    tree = pn.BallTree.from_device(x)
    tol = 1e-3 * h
    rec = {"n": n, "dim": dim, "h": round(h, 5), "bin_cells": int(n_cells), "seed_kind": "bins"}
    _, pw1, _, _, _ = tree.mean_shift_modes_device(h, seeds, tol=0.0, max_iter=1)
    rec["dead_bin_seeds"] = int((pw1 == 0).sum().item())
    if 2 * rec["dead_bin_seeds"] > seeds.shape[0]:
        cells = xs[:: -(-n // max_seeds)]
        seeds = torch.from_numpy(np.ascontiguousarray(cells, dtype=np.float32)).to(DEV)
        rec["seed_kind"] = "rows"
    ns = seeds.shape[0]
    rec["seeds"] = int(ns)
    m, pw, it, sh, work = tree.mean_shift_modes_device(h, seeds, tol=tol)
    iterations = work[0]
    old = OldRoute(tree, x, h)
    ref = [None]

    def new_step():
        tree.mean_shift_modes_device(h, seeds, tol=0.0, max_iter=1)

    def old_step():
        old.step(seeds)

    def new_modes():
        tree.mean_shift_modes_device(h, seeds, tol=tol)

    def old_modes():
        ref[0] = old.run(seeds, iterations)

    ts_new, ts_old, tm_new, tm_old = interleaved([new_step, old_step, new_modes, old_modes], reps)
    med = lambda v: float(np.median(v))  # noqa: E731
    live = pw > 0
    rec.update({
        "iterations": int(iterations), "seed_steps": int(work[1]), "seeds_x_iterations": int(ns * iterations),
        "dead_seeds": int((~live).sum().item()), "points_within_mean": round(float(pw[live].double().mean().item()), 1) if bool(live.any()) else 0.0,
        "step_ms": [round(v, 2) for v in ts_new], "old_step_ms": [round(v, 2) for v in ts_old],
        "modes_ms": [round(v, 2) for v in tm_new], "old_modes_ms": [round(v, 2) for v in tm_old],
        "step_over_old_median": round(med(ts_new) / med(ts_old), 4),
        "modes_over_old_median": round(med(tm_new) / med(tm_old), 4),
        "max_abs_mode_diff_to_old": float((m[live] - ref[0][live]).abs().max().item()) if bool(live.any()) else 0.0})
    t0 = time.perf_counter()
    centres, cp, cos, nc = tree.mean_shift_merge_device(m, pw, h)
    rec["centres"] = int(nc.item())  # (waits for the merge)
    rec["merge_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    labels = tree.mean_shift_labels_device(centres, h, n_centres=rec["centres"])
    torch.cuda.synchronize()
    rec["labels_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    del labels
    if with_sklearn and n <= 100000:
        from sklearn.cluster import MeanShift
        t0 = time.perf_counter()
        sk = MeanShift(bandwidth=h, seeds=cells, n_jobs=16).fit(xs)
        rec["sklearn_host_cpu"] = {"fit_ms_16_jobs": round((time.perf_counter() - t0) * 1e3, 1),
                                   "centres": int(len(sk.cluster_centers_)), "n_iter": int(sk.n_iter_)}
    tree.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="100000x2,100000x16,1000000x128")
    ap.add_argument("--max-seeds", type=int, default=2048)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mean_shift_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_mean_shift"}
    for shape in args.shapes.split(","):
        n, dim = (int(v) for v in shape.split("x"))
        res[shape] = measure(n, dim, args.max_seeds, args.reps, args.sklearn)
        torch.cuda.empty_cache()
        print(shape, json.dumps(res[shape]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
