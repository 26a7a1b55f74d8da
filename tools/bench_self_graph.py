"""Self-queries (pn_query_self_device_f32 / pn_query_radius_self_device_f32) against the same work done by hand.

k-NN: 1M x 128 f32, k = 10: query_self_device(10) against query_device(rows already in HBM, 11), interleaved in one
process.  Radius: 1M x 16 f32, r = the median 21st-nearest distance of 1024 sample rows (lists of about 20 others):
query_radius_self_device against query_radius_device(rows, r), interleaved.  Prints one JSON line.
usage: python tools/bench_self_graph.py [--reps 7] [--n 1000000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import petal_neighbors_amd as pn  # noqa: E402
from petal_neighbors_amd import _lib  # noqa: E402


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fa, fb, reps):
    """ms of each rep of fa and fb, alternated (after one warm-up call of each)"""
    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(one(fa))
        tb.append(one(fb))
    return ta, tb


def rows(n, dim, seed):
    x = torch.empty((n, dim), dtype=torch.float32, device="cuda:0")
    rc = _lib.lib().pn_fill_uniform_device_f32(x.data_ptr(), n * dim, seed, 0, 0, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    n, k, reps = args.n, 10, args.reps
    res = {"tool": "bench_self_graph", "n": n}

    x = rows(n, 128, 0x5E1F5EED)
    t0 = time.perf_counter()
    tree = pn.BallTree.from_device(x)
    torch.cuda.synchronize()
    res["build_s_1m_x_128"] = round(time.perf_counter() - t0, 3)
    oi = torch.empty((n, k), dtype=torch.int64, device="cuda:0")
    od = torch.empty((n, k), dtype=torch.float32, device="cuda:0")
    pi = torch.empty((n, k + 1), dtype=torch.int64, device="cuda:0")
    pd = torch.empty((n, k + 1), dtype=torch.float32, device="cuda:0")
    ts, tq = interleaved(lambda: tree.query_self_device(k, out_idx=oi, out_dist=od),
                         lambda: tree.query_device(x, k + 1, out_idx=pi, out_dist=pd), reps)
    res["knn_k"] = k
    res["knn_self_ms"] = [round(v, 2) for v in ts]
    res["knn_query_k1_ms"] = [round(v, 2) for v in tq]
    res["knn_self_over_query_median"] = round(float(np.median(ts)) / float(np.median(tq)), 4)
    res["knn_self_over_query_min"] = round(min(ts) / min(tq), 4)
    del tree, oi, od, pi, pd, x
    torch.cuda.empty_cache()

    y = rows(n, 16, 0x5E1F5EEE)
    t16 = pn.BallTree.from_device(y)
    sample = y[torch.arange(0, n, n // 1024, device="cuda:0")[:1024]].contiguous()
    _, sd = t16.query_device(sample, 21)
    r = float(torch.median(sd[:, 20]).item())
    # device memory the handle's workspace takes for the self-query (every workspace buffer only grows, so after the calls
    # it is the high-water mark): free memory that went, less what torch reserved for the outputs meanwhile
    torch.cuda.synchronize()
    free0, res0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    _, _, _, tot = t16.query_radius_self_device(r, 0)
    torch.cuda.synchronize()
    total = int(tot.item())
    cap = total + n  # room for the lists with each row itself, for the reference call
    ro = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    ri = torch.empty(cap, dtype=torch.int64, device="cuda:0")
    rt = torch.empty(1, dtype=torch.int64, device="cuda:0")
    t16.query_radius_self_device(r, total, out_offsets=ro, out_idx=ri, out_total=rt)
    torch.cuda.synchronize()
    free1, res1 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    res["radius_self_workspace_mb"] = round(((free0 - free1) - (res1 - res0)) / 2**20, 1)
    res["radius_result_mb"] = round(total * 8 / 2**20, 1)
    ts, tq = interleaved(lambda: t16.query_radius_self_device(r, total, out_offsets=ro, out_idx=ri, out_total=rt),
                         lambda: t16.query_radius_device(y, r, cap, out_offsets=ro, out_idx=ri, out_total=rt), reps)
    res["radius_r"] = r
    res["radius_mean_list"] = round(total / n, 2)
    res["radius_self_ms"] = [round(v, 2) for v in ts]
    res["radius_query_ms"] = [round(v, 2) for v in tq]
    res["radius_self_over_query_median"] = round(float(np.median(ts)) / float(np.median(tq)), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
