"""Self-queries over row shards (pn_sharded_query_self_device_f32 / pn_sharded_query_radius_self_f32) against the
single index's self-query over the same rows, on one GPU.

k-NN: 1M x 128 f32, k = 10: query_self_device of a single index, of the rank handle at world 1 with the exchange forced
(rows all-gather, packed all-gather, slice merge), and of 2, 4 and 8 virtual shards on the one device; interleaved
repetitions, medians.  Radius: 1M x 16 f32, r = the median 21st-nearest distance of 1024 sample rows (as
tools/bench_self_graph.py): the host entry query_radius_self of the single index, the forced-exchange rank handle and 2
virtual shards (wall clock: the host entries end with the lists in host memory).  Prints one JSON line.
usage: python tools/bench_sharded_self.py [--reps 5] [--n 1000000]"""
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


def timed_device(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def interleaved(fns, reps, timer):
    """ms of each rep of every fn, alternated (after one warm-up call of each)"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, f in fns.items():
            out[name].append(timer(f))
    return out


def rows(n, dim, seed):
    x = torch.empty((n, dim), dtype=torch.float32, device="cuda:0")
    rc = _lib.lib().pn_fill_uniform_device_f32(x.data_ptr(), n * dim, seed, 0, 0, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return x


def rank_handle(x):
    sh = pn.ShardedIndex.from_rank_device(x, x.shape[0], 0, 1, pn.ShardedIndex.unique_id(), 0)
    sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)
    return sh


def summarise(res, prefix, times, base):
    for name, t in times.items():
        res[f"{prefix}_{name}_ms"] = [round(v, 2) for v in t]
        res[f"{prefix}_{name}_median_ms"] = round(float(np.median(t)), 2)
        res[f"{prefix}_{name}_over_single"] = round(float(np.median(t)) / float(np.median(times[base])), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    n, k, reps = args.n, 10, args.reps
    res = {"tool": "bench_sharded_self", "n": n, "knn_k": k}

    x = rows(n, 128, 0x5E1F5EED)
    host = x.cpu().numpy()
    handles = {"single": pn.BallTree.from_device(x), "rank_w1_exchange": rank_handle(x)}
    for g in (2, 4, 8):
        handles[f"virtual{g}"] = pn.ShardedIndex.from_host(host, [0] * g)
    oi = torch.empty((n, k), dtype=torch.int64, device="cuda:0")
    od = torch.empty((n, k), dtype=torch.float32, device="cuda:0")
    want = None
    for name, h in handles.items():  # every handle's answer is the single index's, bit for bit
        h.query_self_device(k, out_idx=oi, out_dist=od)
        torch.cuda.synchronize()
        got = (oi.cpu().numpy().tobytes(), od.cpu().numpy().tobytes())
        want = want or got
        assert got == want, name
    fns = {name: (lambda h=h: h.query_self_device(k, out_idx=oi, out_dist=od)) for name, h in handles.items()}
    summarise(res, "knn", interleaved(fns, reps, timed_device), "single")
    del handles, fns, oi, od, x, host
    torch.cuda.empty_cache()

    y = rows(n, 16, 0x5E1F5EEE)
    single = pn.BallTree.from_device(y)
    sample = y[torch.arange(0, n, n // 1024, device="cuda:0")[:1024]].contiguous()
    _, sd = single.query_device(sample, 21)
    r = float(torch.median(sd[:, 20]).item())
    handles = {"single": single, "rank_w1_exchange": rank_handle(y), "virtual2": pn.ShardedIndex.from_host(y.cpu().numpy(), [0, 0])}
    want = None
    for name, h in handles.items():
        o, i, _ = h.query_radius_self(r)
        got = (o.tobytes(), i.tobytes())
        want = want or got
        assert got == want, name
    res["radius_r"] = r
    res["radius_mean_list"] = round(int(np.frombuffer(want[0], dtype=np.uint64)[-1]) / n, 2)
    fns = {name: (lambda h=h: h.query_radius_self(r)) for name, h in handles.items()}
    summarise(res, "radius_host", interleaved(fns, reps, timed_host), "single")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
