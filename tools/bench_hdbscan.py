"""HDBSCAN labels on the device (pn_hdbscan_device_f32) against the tree they are cut from.

For n x 16 f32 rows (uniform, and the Gaussian blobs of tests/test_gpu_dbscan.py at the same density), interleaved in one
process, with min_samples = 10 and min_cluster_size = 25:
  * hdbscan_device: core distances + MST + dendrogram + extraction, total ms;
  * mutual_reachability_mst: core distances + MST alone -- what the library offered before pn_hdbscan_*; the difference
    is the tail this tool is about (the dendrogram and the extraction: no host wait, a few hundred short launches);
  * linkage_device on the finished tree's edges: the dendrogram alone.
Appends one JSON line to profiles/hdbscan_bench.jsonl (--out).
usage: python tools/bench_hdbscan.py [--reps 5] [--n 100000,1000000] [--only uniform|blobs] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petal_neighbors_amd as pn  # noqa: E402
from bench_mst import DEV, interleaved, rows_of  # noqa: E402

MIN_SAMPLES = 10
MIN_CLUSTER_SIZE = 25


def measure(kind, n, reps):
    x = rows_of(kind, n)
    tree = pn.BallTree.from_device(x)
    labels = torch.empty(n, dtype=torch.int64, device=DEV)
    prob = torch.empty(n, dtype=torch.float32, device=DEV)
    ncl = torch.zeros(1, dtype=torch.int64, device=DEV)
    edges = tree.mutual_reachability_mst(MIN_SAMPLES)
    left = torch.empty(n - 1, dtype=torch.int64, device=DEV)
    right = torch.empty(n - 1, dtype=torch.int64, device=DEV)
    size = torch.empty(n - 1, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)

    def hdbscan():
        tree.hdbscan_device(MIN_CLUSTER_SIZE, MIN_SAMPLES, out_labels=labels, out_probabilities=prob, out_n_clusters=ncl)

    def mst():
        tree.mutual_reachability_mst(MIN_SAMPLES)

    def linkage():
        tree.linkage_device(edges=edges, out_left=left, out_right=right, out_weight=edges[2], out_size=size, out_error=err)

    th, tm, tl = interleaved([hdbscan, mst, linkage], reps)
    med = lambda v: float(np.median(v))  # noqa: E731
    rec = {
        "n": n, "dim": 16, "min_samples": MIN_SAMPLES, "min_cluster_size": MIN_CLUSTER_SIZE,
        "hdbscan_ms": [round(v, 2) for v in th], "mst_ms": [round(v, 2) for v in tm], "linkage_ms": [round(v, 2) for v in tl],
        "tail_ms_median": round(med(th) - med(tm), 2), "hdbscan_over_mst_median": round(med(th) / med(tm), 4),
        "n_clusters": int(ncl.item()), "noise_rows": int((labels < 0).sum().item()),
    }
    tree.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", default="100000,1000000")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdbscan_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_hdbscan"}
    for kind in ("uniform", "blobs"):
        if args.only not in ("", kind):
            continue
        for n in (int(v) for v in args.n.split(",")):
            tag = f"{kind}_{n}"
            res[tag] = measure(kind, n, args.reps)
            torch.cuda.empty_cache()
            print(tag, json.dumps(res[tag]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
