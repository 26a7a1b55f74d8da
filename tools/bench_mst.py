"""The mutual-reachability MST on the device (pn_mst_device_f32) against the self-queries it is built from.

For n x 16 f32 rows (uniform, and the Gaussian blobs of tests/test_gpu_dbscan.py at the same density), without cores and
with the k = 10 core distances (query_self_device(10)'s last column), interleaved in one process:
  * mst_device: total ms, rounds and rows scanned (pn_mst_*'s work_out);
  * query_self_device(1) on the handle's own engine: what round 0 of the un-cored call should cost;
  * one query_self_device(1) pass on the exact engine, times the rounds: what Boruvka without the three shortcuts costs.
--trace also runs each configuration once in a child process under `rocprofv3 --kernel-trace --stats` and adds the summed
duration of the masked scan kernel (mst_scan_kernel).  Appends one JSON line to profiles/mst_bench.jsonl (--out).
usage: python tools/bench_mst.py [--reps 3] [--n 100000,1000000] [--only uniform|blobs] [--trace] [--out FILE]"""
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
import petal_neighbors_amd as pn  # noqa: E402
from petal_neighbors_amd import _lib  # noqa: E402

DEV = "cuda:0"
K_CORE = 10


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, reps):
    """ms of each rep of every function, alternated (after one warm-up call of each)"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(out, fns):
            t.append(one(f))
    return out


def uniform_rows(n, dim, seed):
    x = torch.empty((n, dim), dtype=torch.float32, device=DEV)
    rc = _lib.lib().pn_fill_uniform_device_f32(x.data_ptr(), n * dim, seed, 0, 0, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return x


def blob_rows(n, dim, nb, sigma, background, seed):
    rng = np.random.default_rng(seed)
    centres = rng.random((nb, dim))
    n_bg = int(round(n * background))
    which = rng.integers(0, nb, n - n_bg)
    pts = np.concatenate([centres[which] + sigma * rng.standard_normal((n - n_bg, dim)), rng.random((n_bg, dim))])
    return torch.from_numpy(pts[rng.permutation(n)].astype(np.float32)).to(DEV)


def rows_of(kind, n):
    if kind == "uniform":
        return uniform_rows(n, 16, 0x5E1F5EEE)
    return blob_rows(n, 16, max(1, n * 12 // 12000), 0.05, 0.10, 3)


def measure(kind, n, cored, reps):
    x = rows_of(kind, n)
    tree = pn.BallTree.from_device(x)
    core = None
    if cored:
        core = tree.query_self_device(K_CORE)[1][:, -1].contiguous()
    src = torch.empty(n - 1, dtype=torch.int64, device=DEV)
    dst = torch.empty(n - 1, dtype=torch.int64, device=DEV)
    wgt = torch.empty(n - 1, dtype=torch.float32, device=DEV)
    oi = torch.empty((n, 1), dtype=torch.int64, device=DEV)
    od = torch.empty((n, 1), dtype=torch.float32, device=DEV)

    def mst():
        tree.mst_device(core, out_src=src, out_dst=dst, out_weight=wgt)

    def nn_auto():
        tree.set_engine("auto")
        tree.query_self_device(1, out_idx=oi, out_dist=od)

    def nn_exact():
        tree.set_engine("exact")
        tree.query_self_device(1, out_idx=oi, out_dist=od)
        tree.set_engine("auto")

    tm, ta, te = interleaved([mst, nn_auto, nn_exact], reps)
    rounds, scanned = tree.last_mst_work
    med = lambda v: float(np.median(v))  # noqa: E731
    rec = {
        "n": n, "dim": 16, "k_core": K_CORE if cored else 0, "rounds": rounds, "rows_scanned": scanned,
        "rows_scanned_over_n": round(scanned / n, 3),
        "mst_ms": [round(v, 2) for v in tm], "self_1nn_ms": [round(v, 2) for v in ta],
        "self_1nn_exact_engine_ms": [round(v, 2) for v in te],
        "mst_over_self_1nn_median": round(med(tm) / med(ta), 3),
        "mst_over_rounds_x_exact_pass_median": round(med(tm) / (rounds * med(te)), 4),
        "total_weight": float(wgt.double().sum().item()),
    }
    tree.close()
    return rec


def traced_scan_ms(kind, n, cored):
    """summed duration of mst_scan_kernel over ONE mst_device call (plus its warm-up: halved), in a fresh child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mst", "--", sys.executable,
               os.path.abspath(__file__), "--child", kind, str(n), "1" if cored else "0"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        total = 0.0
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "mst_scan_kernel" in row["Name"]:
                    total += float(row["TotalDurationNs"]) / 1e6
    return round(total / 2, 2)


def child(kind, n, cored):
    x = rows_of(kind, n)
    tree = pn.BallTree.from_device(x)
    core = tree.query_self_device(K_CORE)[1][:, -1].contiguous() if cored else None
    for _ in range(2):
        tree.mst_device(core)
    torch.cuda.synchronize()
    tree.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), sys.argv[4] == "1")
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", default="100000,1000000")
    ap.add_argument("--only", default="")
    ap.add_argument("--cores", default="0,1", help="0: without cores, 1: with the k = 10 cores")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mst_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_mst"}
    for kind in ("uniform", "blobs"):
        if args.only not in ("", kind):
            continue
        for n in (int(v) for v in args.n.split(",")):
            for cored in (c == "1" for c in args.cores.split(",")):
                tag = f"{kind}_{n}_{'k10' if cored else 'plain'}"
                res[tag] = measure(kind, n, cored, args.reps)
                torch.cuda.empty_cache()
                if args.trace:
                    res[tag]["scan_kernel_ms"] = traced_scan_ms(kind, n, cored)
                print(tag, json.dumps(res[tag]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
