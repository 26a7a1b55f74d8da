"""k-NN classification and regression on the device (pn_knn_classify_device_f32, pn_knn_regress_device_f32 and the _self
form of the vote) against the plain k-NN query they are built on.

For n x 16 uniform f32 rows, 10^5 uniform queries and k = 20, each shape in a child process of its own, every variant
interleaved with the yardstick and medians taken, for both weightings:
  * query_device(k): the lists alone, into the caller's [nq, k] tensors -- the yardstick (the same pipeline, the same
    handle, the same queries);
  * knn_classify_device without proba, and with proba at 10 classes;
  * knn_regress_device with n_out = 1 and n_out = 64;
  * knn_classify_self_device against query_self_device(k).
A variant's tail is its median minus the yardstick's; the ratio is tail / yardstick.  The vote and the mean are one launch
per 2^18-query chunk behind the chunk's k-NN answer (plus one memset of the proba rows), so the tail is that launch.
--trace adds the duration of each knn_* kernel per call from a child under rocprofv3 --kernel-trace.
Appends one JSON line to profiles/knn_predict_bench.jsonl (--out).
usage: python tools/bench_knn_predict.py [--reps 7] [--n 100000,1000000] [--nq 100000] [--trace] [--out FILE]"""
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
from bench_mst import DEV, interleaved, uniform_rows  # noqa: E402

K, CLASSES, WIDE = 20, 10, 64
WEIGHTINGS = ("uniform", "distance")
KERNELS = ("knn_vote_group_kernel", "knn_vote_wave_kernel", "knn_mean_row_kernel")


def setup(n, nq):
    x, q = uniform_rows(n, 16, 0x5E1F5EEE), uniform_rows(nq, 16, 0x0BADC0DE)
    tree = pn.BallTree.from_device(x)
    g = torch.Generator(device=DEV).manual_seed(7)
    labels = torch.randint(0, CLASSES, (n,), generator=g, device=DEV, dtype=torch.int64)
    y = torch.randn((n, WIDE), generator=g, device=DEV, dtype=torch.float64)
    return tree, q, labels, y


def variants(tree, q, labels, y, n, nq):
    """name -> (callable, yardstick name)"""
    oi = torch.empty((nq, K), dtype=torch.int64, device=DEV)
    od = torch.empty((nq, K), dtype=torch.float32, device=DEV)
    si = torch.empty((n, K), dtype=torch.int64, device=DEV)
    sd = torch.empty((n, K), dtype=torch.float32, device=DEV)
    pred = torch.empty(nq, dtype=torch.int64, device=DEV)
    proba = torch.empty((nq, CLASSES), dtype=torch.float64, device=DEV)
    out1 = torch.empty(nq, dtype=torch.float64, device=DEV)
    outw = torch.empty((nq, WIDE), dtype=torch.float64, device=DEV)
    spred = torch.empty(n, dtype=torch.int64, device=DEV)
    y1 = y[:, 0].contiguous()
    v = {"query": (lambda: tree.query_device(q, K, out_idx=oi, out_dist=od), None),
         "query_self": (lambda: tree.query_self_device(K, out_idx=si, out_dist=sd), None)}
    for w in WEIGHTINGS:
        v[f"classify_{w}"] = (lambda w=w: tree.knn_classify_device(q, K, labels, CLASSES, w, out_pred=pred), "query")
        v[f"classify_proba_{w}"] = (lambda w=w: tree.knn_classify_device(q, K, labels, CLASSES, w, True, out_pred=pred,
                                                                        out_proba=proba), "query")
        v[f"regress_1_{w}"] = (lambda w=w: tree.knn_regress_device(q, K, y1, w, out=out1), "query")
        v[f"regress_{WIDE}_{w}"] = (lambda w=w: tree.knn_regress_device(q, K, y, w, out=outw), "query")
        v[f"classify_self_{w}"] = (lambda w=w: tree.knn_classify_self_device(K, labels, CLASSES, w, out_pred=spred),
                                   "query_self")
    return v


def child(n, nq, reps):
    tree, q, labels, y = setup(n, nq)
    v = variants(tree, q, labels, y, n, nq)
    names = list(v)
    times = dict(zip(names, interleaved([v[name][0] for name in names], reps)))
    med = {name: float(np.median(t)) for name, t in times.items()}
    rec = {"n": n, "nq": nq, "dim": 16, "k": K, "reps": reps}
    for name in names:
        rec[name + "_ms"] = [round(t, 3) for t in times[name]]
        base = v[name][1]
        if base:
            rec[name + "_tail_ms_median"] = round(med[name] - med[base], 3)
            rec[name + "_tail_over_" + base + "_median"] = round((med[name] - med[base]) / med[base], 4)
    tree.close()
    print("RESULT " + json.dumps(rec), flush=True)


def traced(n, nq):
    """two calls of every variant but the yardsticks under a kernel trace; each knn_* kernel's time per call"""
    tree, q, labels, y = setup(n, nq)
    v = variants(tree, q, labels, y, n, nq)
    for _ in range(2):
        for name, (fn, base) in v.items():
            if base:
                fn()
    torch.cuda.synchronize()
    tree.close()


def traced_kernel_ms(n, nq):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "knn", "--", sys.executable,
               os.path.abspath(__file__), "--traced", str(n), str(nq)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        total, calls = {k: 0.0 for k in KERNELS}, {k: 0 for k in KERNELS}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in KERNELS:
                    if k in row["Name"]:
                        total[k] += float(row["TotalDurationNs"]) / 1e6
                        calls[k] += int(row["Calls"])
    return {k: {"ms_per_launch": round(total[k] / calls[k], 4), "launches": calls[k]} for k in KERNELS if calls[k]}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--traced":
        traced(int(sys.argv[2]), int(sys.argv[3]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", default="100000,1000000")
    ap.add_argument("--nq", type=int, default=100000)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_predict_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_knn_predict", "library": os.path.basename(pn._lib.LIB_PATH)}
    for n in (int(s) for s in args.n.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), str(args.nq), str(args.reps)]
        p = subprocess.run(cmd, check=True, capture_output=True, text=True)
        rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        if args.trace:
            rec["kernel_ms"] = traced_kernel_ms(n, args.nq)
        res[f"uniform_{n}"] = rec
        print(f"uniform_{n}", json.dumps(rec), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
