#!/usr/bin/env python3
"""pn_silhouette_device_* at scale, next to pn_pairwise_device_* on the same rows: time per call by device events, and the
time per evaluated (row, row) pair of each.  The silhouette evaluates n * M ordered pairs (M members, here all n rows);
pairwise evaluates the n (n - 1) / 2 pairs above the diagonal and stores n * n values.

    python tools/bench_silhouette.py [--reps R] [--no-pairwise] > profiles/silhouette_bench.jsonl   (on the GPU box)

Kernel times proper come from a run of its own under `rocprofv3 --kernel-trace --stats` (sil_sweep_kernel,
exact_pairwise_kernel); the event times here include the sort, the two gathers and the finish.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

import petal_neighbors_amd as pn
from petal_neighbors_amd import distance as dist


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def one(n, d, dtype, n_clusters, reps, pairwise):
    g = torch.Generator(device="cuda").manual_seed(n * 131 + d)
    x = torch.rand((n, d), generator=g, device="cuda", dtype=dtype)
    codes = torch.randint(0, n_clusters, (n,), generator=g, device="cuda", dtype=torch.int64)
    tree = pn.BallTree.from_device(x)
    outs = tree.silhouette_device(codes, n_clusters)
    ms = timed(lambda: tree.silhouette_device(codes, n_clusters, None, *outs), reps)  # (the outputs in the signature's order)
    assert int(outs[6].item()) == 0 and int(outs[5].item()) == n
    rec = {"workload": f"silhouette {n} x {d} {'f32' if x.element_size() == 4 else 'f64'}, {n_clusters} clusters",
           "silhouette_ms": round(ms, 3), "silhouette_ns_per_pair": round(ms * 1e6 / (float(n) * n), 6),
           "silhouette_ops_T": round(3.0 * d * n * n / ms / 1e9, 2), "score": float(outs[4].item())}
    if pairwise:
        out = torch.empty((n, n), device="cuda", dtype=dtype)
        pms = timed(lambda: dist.pairwise_device(x, out), reps)
        rec.update({"pairwise_ms": round(pms, 3), "pairwise_ns_per_pair": round(pms * 1e6 / (n * (n - 1) / 2.0), 6)})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-pairwise", action="store_true")
    ap.add_argument("--shapes", default="20000x128,100000x128,100000x16")
    ap.add_argument("--f64", action="store_true", help="also the f64 tree at the first shape")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    for n, d in shapes:
        print(json.dumps(one(n, d, torch.float32, 16, a.reps, not a.no_pairwise)), flush=True)
    if a.f64:
        n, d = shapes[0]
        print(json.dumps(one(n, d, torch.float64, 16, a.reps, not a.no_pairwise)), flush=True)


if __name__ == "__main__":
    main()
