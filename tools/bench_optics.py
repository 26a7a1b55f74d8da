"""OPTICS on the device (pn_optics_device_f32): the whole call and its stages.

For n x 16 f32 rows (the Gaussian blobs of tools/bench_mst.py), min_samples = 10 and a max_eps found by bisection on the
counting pass for a mean list length of about 45 entries, interleaved in one process:
  * optics_device: the whole call (cores, count, fill, ordering), total ms;
  * the stages through the public entry points a call is built from: query_self_device(min_samples) = the core
    distances; query_radius_self_device(radii, capacity 0) = the counting pass with the call's per-row radii (max_eps where
    the core is defined, 0 elsewhere); the same with the exact capacity and distances = the fill (64-bit ids; the call's
    own fill goes by pieces and repacks to 32-bit ids); optics_dbscan_device at 0.8 max_eps = the extraction;
  * the ordering stage: total - cores - count - fill (derived), and with --trace the duration of the one
    optics_order_kernel launch from a child process under rocprofv3 --kernel-trace (the second of two calls), which is the
    stage itself; microseconds per step = that / n.
--sklearn adds sklearn.cluster.OPTICS(min_samples + 1, max_eps, n_jobs=16) on the same rows on the CPU (minutes at 10^5).
Appends one JSON line to profiles/optics_bench.jsonl (--out).
usage: python tools/bench_optics.py [--reps 3] [--n 100000,1000000] [--trace] [--sklearn N] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petal_neighbors_amd as pn  # noqa: E402
from bench_mst import DEV, interleaved, rows_of  # noqa: E402

MS = 10
TARGET = 45.0


def mean_degree(tree, eps):
    off, _, _, tot = tree.query_radius_self_device(np.float32(eps), 0)
    return float(tot.item()) / len(off[:-1])


def find_eps(tree):
    """bisection on the counting pass: the max_eps whose mean list length is about TARGET"""
    lo, hi = 0.05, 0.6
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        if mean_degree(tree, mid) < TARGET:
            lo = mid
        else:
            hi = mid
    return float(np.float32(0.5 * (lo + hi)))


def measure(n, reps, eps=None):
    x = rows_of("blobs", n)
    tree = pn.BallTree.from_device(x)
    if eps is None:
        eps = find_eps(tree)
    eps = np.float32(eps)
    ordering = torch.empty(n, dtype=torch.int64, device=DEV)
    reach = torch.empty(n, dtype=torch.float32, device=DEV)
    pred = torch.empty(n, dtype=torch.int64, device=DEV)
    core = torch.empty(n, dtype=torch.float32, device=DEV)
    tree.optics_device(MS, eps, out_ordering=ordering, out_reachability=reach, out_predecessor=pred, out_core=core)
    radii = torch.where(core < float(eps), torch.full_like(core, float(eps)), torch.zeros_like(core)).contiguous()
    off, _, _, tot = tree.query_radius_self_device(radii, 0)
    total = int(tot.item())
    deg = (off[1:] - off[:-1])
    oi = torch.empty((n, MS), dtype=torch.int64, device=DEV)
    od = torch.empty((n, MS), dtype=torch.float32, device=DEV)
    g_idx = torch.empty(max(total, 1), dtype=torch.int64, device=DEV)
    g_dist = torch.empty(max(total, 1), dtype=torch.float32, device=DEV)
    labels = torch.empty(n, dtype=torch.int64, device=DEV)

    def whole():
        tree.optics_device(MS, eps, out_ordering=ordering, out_reachability=reach, out_predecessor=pred, out_core=core)

    def cores():
        tree.query_self_device(MS, out_idx=oi, out_dist=od)

    def count():
        tree.query_radius_self_device(radii, 0, out_offsets=off)

    def fill():
        tree.query_radius_self_device(radii, total, with_distance=True, out_offsets=off, out_idx=g_idx, out_dist=g_dist)

    def extract():
        tree.optics_dbscan_device(np.float32(0.8) * eps, ordering, reach, core, out_labels=labels)

    tw, tc, tn, tf, te = interleaved([whole, cores, count, fill, extract], reps)
    med = lambda v: float(np.median(v))  # noqa: E731
    derived = med(tw) - med(tc) - med(tn) - med(tf)
    rec = {
        "n": n, "dim": 16, "min_samples": MS, "max_eps": float(eps),
        "stored_entries": total, "mean_degree_all_rows": round(total / n, 2),
        "mean_degree_core_rows": round(total / max(int((core < float(eps)).sum().item()), 1), 2),
        "max_degree": int(deg.max().item()), "rows_without_core": int((core >= float(eps)).sum().item()),
        "rows_with_inf_reach": int(torch.isinf(reach).sum().item()),
        "optics_s": [round(v / 1e3, 4) for v in tw], "cores_s": round(med(tc) / 1e3, 4), "count_s": round(med(tn) / 1e3, 4),
        "fill_s": round(med(tf) / 1e3, 4), "extraction_s": round(med(te) / 1e3, 5),
        "ordering_s_derived": round(derived / 1e3, 4), "ordering_us_per_step_derived": round(derived * 1e3 / n, 3),
        "ordering_share_of_call_derived": round(derived / med(tw), 3),
        "clusters_at_0p8": int(labels.max().item()) + 1,
    }
    tree.close()
    return rec, x, float(eps)


def traced_order_ms(n, eps):
    """the ordering kernel's duration in the second optics_device call of a fresh child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "optics", "--", sys.executable,
               os.path.abspath(__file__), "--child", str(n), repr(eps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        durs = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows = [r for r in csv.DictReader(open(f)) if "optics_order_kernel" in r["Kernel_Name"]]
            rows.sort(key=lambda r: int(r["Start_Timestamp"]))
            durs += [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
    return durs[-1] if durs else None


def child(n, eps):
    x = rows_of("blobs", n)
    tree = pn.BallTree.from_device(x)
    for _ in range(2):
        tree.optics_device(MS, np.float32(eps))
    torch.cuda.synchronize()
    tree.close()


def sklearn_seconds(x, eps):
    from sklearn.cluster import OPTICS
    pts = x.cpu().numpy()
    t = time.time()
    OPTICS(min_samples=MS + 1, max_eps=eps, n_jobs=16).fit(pts)
    return round(time.time() - t, 2)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), float(sys.argv[3]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", default="100000,1000000")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--sklearn", type=int, default=0, help="also time scikit-learn on the CPU at this n (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optics_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_optics"}
    eps = None
    for n in (int(v) for v in args.n.split(",")):
        tag = f"blobs_{n}"
        res[tag], x, eps = measure(n, args.reps, eps)  # (the first shape's max_eps serves every shape: the same density)
        if args.trace:
            try:
                ms = traced_order_ms(n, eps)
                res[tag]["ordering_s_traced"] = round(ms / 1e3, 4)
                res[tag]["ordering_us_per_step_traced"] = round(ms * 1e3 / n, 3)
            except Exception as e:  # (no profiler on this box: the derived figure stands alone)
                res[tag]["trace_error"] = str(e)[:200]
        if args.sklearn == n:
            try:
                res[tag]["sklearn_optics_s_16_cpus"] = sklearn_seconds(x, eps)
            except ImportError:
                res[tag]["sklearn_optics_s_16_cpus"] = None
        del x
        torch.cuda.empty_cache()
        print(tag, json.dumps(res[tag]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
