"""Kernel density sums on the device (pn_kde_device_f32) against the two-call route they replace.

For n x dim f32 uniform rows and 10^4 uniform queries, interleaved in one process:
  * kde: kernel_density_device -- the cutoff kernel, the counting pass, the lists with distances piece by piece into
    workspace scratch, one wave per query, total ms;
  * two_call: what a caller had before -- query_radius_with_distance_device at the same cutoffs with capacity 0 to size
    the buffers (the total read back), the same call again with that capacity, then the terms and a segment sum in torch.
Two legs per shape: epanechnikov with h = the median distance to the 30th neighbour of a query sample (about 30 terms per
query), and gaussian with atol = 1e-6 n and h = that distance / sqrt(2 ln 1e6), so that its cutoff is the same radius.
At shapes of up to 10^5 rows also the slow case: gaussian with atol = 0 over 256 queries (every row is a term of every query).
--sklearn adds sklearn.neighbors.KernelDensity (ball_tree, the same atol, rtol = 0) on 16 CPU threads at n <= 10^5.
Appends one JSON line to profiles/kde_bench.jsonl (--out).
usage: python tools/bench_kde.py [--reps 5] [--shapes 100000x16,1000000x128] [--nq 10000] [--sklearn] [--out FILE]"""
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
from bench_mst import DEV, interleaved, uniform_rows  # noqa: E402


def two_call(tree, q, cut, h, kernel):
    """the sums by the parent surface: size, list, reduce"""
    nq = q.shape[0]
    _, _, _, total = tree.query_radius_with_distance_device(q, cut, 0)
    cap = int(total.item())  # (the caller's sizing round trip)
    off, _, dist, _ = tree.query_radius_with_distance_device(q, cut, max(cap, 1))
    lengths = off[1:] - off[:-1]
    seg = torch.repeat_interleave(torch.arange(nq, device=q.device), lengths)
    d = dist[:cap].double()
    hh = h.double()[seg]
    t = 1.0 - (d * d) / (hh * hh) if kernel == "epanechnikov" else torch.exp(-((d * d) / (2.0 * (hh * hh))))
    return torch.zeros(nq, dtype=torch.float64, device=q.device).index_add_(0, seg, t)


def sklearn_ms(x, q, h, kernel, atol):
    from concurrent.futures import ThreadPoolExecutor
    from sklearn.neighbors import KernelDensity
    xs, qs = x.cpu().numpy().astype(np.float64), q.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    kd = KernelDensity(bandwidth=h, kernel=kernel, algorithm="ball_tree", atol=atol / len(xs), rtol=0).fit(xs)
    t1 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(kd.score_samples, np.array_split(qs, 16)))
    t2 = time.perf_counter()
    return {"fit_ms": round((t1 - t0) * 1e3, 1), "score_ms_16_threads": round((t2 - t1) * 1e3, 1)}


def measure(n, dim, nq, reps, with_sklearn, slow_case):
    x = uniform_rows(n, dim, 0x5E1F5EEE)
    q = uniform_rows(nq, dim, 0x5E1F5EEF)
    tree = pn.BallTree.from_device(x)
    _, d31 = tree.query_device(q[:512].contiguous(), 31)
    r30 = float(d31[:, 30].median().item())
    rec = {"n": n, "dim": dim, "nq": nq, "r30": round(r30, 5)}
    out = (torch.empty(nq, dtype=torch.float64, device=DEV), torch.empty(nq, dtype=torch.int64, device=DEV),
           torch.empty(nq, dtype=torch.float32, device=DEV))
    legs = (("epanechnikov", r30, 0.0), ("gaussian", r30 / math.sqrt(2.0 * math.log(1e6)), 1e-6 * n))
    for kernel, h, atol in legs:
        ht = torch.full((nq,), h, dtype=torch.float32, device=DEV)

        def kde():
            tree.kernel_density_device(q, ht, kernel, atol, out_sum=out[0], out_count=out[1], out_cutoff=out[2])

        kde()
        torch.cuda.synchronize()
        cut = out[2].clone()
        ref = [None]

        def old():
            ref[0] = two_call(tree, q, cut, ht, kernel)

        tk, to = interleaved([kde, old], reps)
        med = lambda v: float(np.median(v))  # noqa: E731
        s, want = out[0], ref[0]
        leg = {"h": round(h, 6), "atol": atol, "kde_ms": [round(v, 2) for v in tk], "two_call_ms": [round(v, 2) for v in to],
               "kde_over_two_call_median": round(med(tk) / med(to), 4), "terms_per_query": round(float(out[1].double().mean().item()), 2),
               "max_rel_diff_to_two_call": float(((s - want).abs() / want.clamp_min(1e-300)).max().item())}
        if with_sklearn and n <= 100000:
            leg["sklearn"] = sklearn_ms(x, q, h, kernel, atol)
        rec[kernel] = leg
    if slow_case:
        qs = q[:256].contiguous()
        hs = r30 / math.sqrt(2.0 * math.log(1e6))
        (ts,) = interleaved([lambda: tree.kernel_density_device(qs, hs, "gaussian", 0.0)], reps)
        rec["gaussian_atol_0_256_queries_ms"] = [round(v, 2) for v in ts]
    tree.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="100000x16,1000000x128")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kde_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_kde"}
    for shape in args.shapes.split(","):
        n, dim = (int(v) for v in shape.split("x"))
        res[shape] = measure(n, dim, args.nq, args.reps, args.sklearn, n <= 100000)
        torch.cuda.empty_cache()
        print(shape, json.dumps(res[shape]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
