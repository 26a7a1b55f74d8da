#!/usr/bin/env python3
"""pn_kmeans_init_device_* at scale, next to kmeans_plusplus (the torch loop it stands beside) on the same tree, in one
session on one device: time per call by device events for the greedy seeding (trials = 2 + floor(ln k)), for trials = 1
(classic k-means++, the like-for-like comparison: the torch loop tries one row per round) and for the torch loop.

    python tools/bench_kmeans_init.py [--reps R] [--no-torch] > profiles/kmeans_init_bench.jsonl   (on the GPU box)

The floor of a round is one read of the corpus: bytes_per_round / the HBM rate.  Kernel times proper (kpp_sweep_kernel,
kpp_pick_kernel) come from a run of its own under `rocprofv3 --kernel-trace --stats` (--no-torch --reps 1 keeps it short);
the event times here include the picks between the sweeps and, for the torch loop, its host round trips.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

import petal_neighbors_amd as pn


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


def one(n, d, k, reps, with_torch):
    g = torch.Generator(device="cuda").manual_seed(n * 131 + d)
    x = torch.rand((n, d), generator=g, device="cuda", dtype=torch.float32)
    tree = pn.BallTree.euclidean(x.cpu().numpy())  # (host-built: kmeans_plusplus needs the rows on the host)
    trials = min(2 + int(math.log(k)), 16)
    outs = tree.kmeans_init_device(k, 0)
    greedy = timed(lambda: tree.kmeans_init_device(k, 0, None, *outs), reps)
    classic = timed(lambda: tree.kmeans_init_device(k, 0, 1, *outs), reps)
    assert int(outs[1].min().item()) >= 0
    ld = (d + 7) // 8 * 8
    rec = {"workload": f"kmeans_init {n} x {d} f32, k = {k}", "trials": trials, "greedy_ms": round(greedy, 3),
           "classic_ms": round(classic, 3), "greedy_us_per_round": round(greedy * 1e3 / k, 2),
           "classic_us_per_round": round(classic * 1e3 / k, 2), "bytes_per_round": n * ld * 4}
    if with_torch:
        rec["torch_loop_ms"] = round(timed(lambda: tree.kmeans_plusplus(k, 0), 1), 3)
        rec["classic_over_torch"] = round(classic / rec["torch_loop_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--shapes", default="1000000x128x64,1000000x128x1024,100000x16x64")
    a = ap.parse_args()
    for s in a.shapes.split(","):
        n, d, k = (int(v) for v in s.split("x"))
        print(json.dumps(one(n, d, k, a.reps, not a.no_torch)), flush=True)


if __name__ == "__main__":
    main()
