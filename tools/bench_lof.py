"""Local Outlier Factor on the device (pn_lof_device_f32) against the self-query it is built on.

For n x 16 f32 rows (uniform, and the Gaussian blobs of tools/bench_mst.py), k = 20, interleaved in one process:
  * lof_device: the k self-query, chunk by chunk, + pack + the lrd pass + the lof pass, total ms;
  * query_self_device(k): the graph alone, into the caller's [n, k] tensors -- what a caller had to pull down before;
the quotient is the tail this tool is about (three HBM-bound launches per call and one pack per 2^18-row chunk).
--trace adds each of the three kernels' duration per call: a child process makes two calls under rocprofv3
--kernel-trace (the first one with its workspace allocations), a kernel's durations are summed over both (pack runs once
per 2^18-row chunk) and halved.  Appends one JSON line to profiles/lof_bench.jsonl (--out).
usage: python tools/bench_lof.py [--reps 5] [--n 100000,1000000] [--only uniform|blobs] [--trace] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petal_neighbors_amd as pn  # noqa: E402
from bench_mst import DEV, interleaved, rows_of  # noqa: E402

K = 20
KERNELS = ("lof_pack_kernel", "lof_lrd_kernel", "lof_lof_kernel")


def measure(kind, n, reps):
    x = rows_of(kind, n)
    tree = pn.BallTree.from_device(x)
    lof = torch.empty(n, dtype=torch.float64, device=DEV)
    lrd = torch.empty(n, dtype=torch.float64, device=DEV)
    kdist = torch.empty(n, dtype=torch.float32, device=DEV)
    oi = torch.empty((n, K), dtype=torch.int64, device=DEV)
    od = torch.empty((n, K), dtype=torch.float32, device=DEV)

    def fit():
        tree.lof_device(K, out_lof=lof, out_lrd=lrd, out_kdist=kdist)

    def graph():
        tree.query_self_device(K, out_idx=oi, out_dist=od)

    tf, tg = interleaved([fit, graph], reps)
    med = lambda v: float(np.median(v))  # noqa: E731
    rec = {
        "n": n, "dim": 16, "k": K,
        "lof_ms": [round(v, 2) for v in tf], "query_self_ms": [round(v, 2) for v in tg],
        "tail_ms_median": round(med(tf) - med(tg), 3), "lof_over_query_self_median": round(med(tf) / med(tg), 4),
        "max_lof": float(lof.max().item()), "rows_above_1p5": int((lof > 1.5).sum().item()),
    }
    tree.close()
    return rec


def traced_kernel_ms(kind, n):
    """each LOF kernel's duration per lof_device call: summed over a fresh child process's two calls (the first is its
    warm-up) and over a call's chunks, halved"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "lof", "--", sys.executable,
               os.path.abspath(__file__), "--child", kind, str(n)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        total = {k: 0.0 for k in KERNELS}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in KERNELS:
                    if k in row["Name"]:
                        total[k] += float(row["TotalDurationNs"]) / 1e6
    return {k: round(v / 2, 3) for k, v in total.items()}


def child(kind, n):
    x = rows_of(kind, n)
    tree = pn.BallTree.from_device(x)
    for _ in range(2):
        tree.lof_device(K)
    torch.cuda.synchronize()
    tree.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", default="100000,1000000")
    ap.add_argument("--only", default="")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lof_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_lof"}
    for kind in ("uniform", "blobs"):
        if args.only not in ("", kind):
            continue
        for n in (int(v) for v in args.n.split(",")):
            tag = f"{kind}_{n}"
            res[tag] = measure(kind, n, args.reps)
            torch.cuda.empty_cache()
            if args.trace:
                res[tag]["kernel_ms"] = traced_kernel_ms(kind, n)
            print(tag, json.dumps(res[tag]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
