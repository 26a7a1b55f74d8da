"""Device radius search with and without distances / nearest-first order, 1M x 128 f32, 10^4 device-resident queries.

Times, interleaved on one device, pn_query_radius_device_f32, pn_query_radius_with_distance_device_f32 (flags 0) and the
same with PN_RADIUS_SORTED, at three radii whose mean list length is about 2, 30 and 300 (picked from the 1000 nearest
distances of 512 sample queries, printed with the measured lengths); then one r = +inf query against the whole
corpus, sorted and not.
usage: python tools/bench_radius_distance.py [--reps 10]   (one JSON line per case: medians and the spread of the reps)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import petal_neighbors_amd as pn  # noqa: E402
from petal_neighbors_amd import _lib  # noqa: E402


def timed(fn, reps):
    """median ms of `reps` calls (CUDA events on the current stream)"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    args = ap.parse_args()
    n, dim, nq = args.n, 128, args.nq
    L = _lib.lib()
    pts = torch.empty((n, dim), dtype=torch.float32, device="cuda:0")
    qs = torch.empty((nq, dim), dtype=torch.float32, device="cuda:0")
    L.pn_fill_uniform_device_f32(pts.data_ptr(), n * dim, 0x5EED0001, 0, 0, None)
    L.pn_fill_uniform_device_f32(qs.data_ptr(), nq * dim, 0x5EED0002, 0, 0, None)
    torch.cuda.synchronize()
    tree = pn.BallTree.from_device(pts)
    _, kd = tree.query_device(qs[:512], 1000)
    kd = np.sort(kd.cpu().numpy().ravel())
    for target in (2, 30, 300):
        # the radius whose mean list length over the sample is `target`: the (target * 512)-th smallest sampled distance
        r = float(np.nextafter(kd[target * 512 - 1], np.float32(np.inf)))
        _, _, tot = tree.query_radius_device(qs, r, 0)
        torch.cuda.synchronize()
        cap = int(tot.item())
        offs = torch.empty(nq + 1, dtype=torch.int64, device="cuda:0")
        idx = torch.empty(max(cap, 1), dtype=torch.int64, device="cuda:0")
        dist = torch.empty(max(cap, 1), dtype=torch.float32, device="cuda:0")
        tt = torch.empty(1, dtype=torch.int64, device="cuda:0")
        calls = {
            "indices": lambda: tree.query_radius_device(qs, r, cap, out_offsets=offs, out_idx=idx, out_total=tt),
            "with_distance": lambda: tree.query_radius_with_distance_device(qs, r, cap, False, offs, idx, dist, tt),
            "with_distance_sorted": lambda: tree.query_radius_with_distance_device(qs, r, cap, True, offs, idx, dist, tt),
        }
        for f in calls.values():  # warm the workspaces
            f()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.reps):  # interleaved
            for k, f in calls.items():
                ms[k].append(timed(f, 1))
        res = {k: round(float(np.median(v)), 3) for k, v in ms.items()}
        spread = {k: [round(float(x), 3) for x in np.percentile(v, [0, 25, 75, 100])] for k, v in ms.items()}
        print(json.dumps({"case": f"mean_len_{target}", "n": n, "dim": dim, "nq": nq, "radius": r,
                          "mean_list_len": round(cap / nq, 2), "total": cap, "ms": res,
                          "ms_min_p25_p75_max": spread,
                          "distance_overhead": round(res["with_distance"] / res["indices"] - 1, 4),
                          "sort_overhead_vs_distance": round(res["with_distance_sorted"] / res["with_distance"] - 1, 4)}),
              flush=True)
    q1 = qs[:1]
    offs = torch.empty(2, dtype=torch.int64, device="cuda:0")
    idx = torch.empty(n, dtype=torch.int64, device="cuda:0")
    dist = torch.empty(n, dtype=torch.float32, device="cuda:0")
    tt = torch.empty(1, dtype=torch.int64, device="cuda:0")
    calls = {
        "indices": lambda: tree.query_radius_device(q1, float("inf"), n, out_offsets=offs, out_idx=idx, out_total=tt),
        "with_distance": lambda: tree.query_radius_with_distance_device(q1, float("inf"), n, False, offs, idx, dist, tt),
        "with_distance_sorted": lambda: tree.query_radius_with_distance_device(q1, float("inf"), n, True, offs, idx, dist,
                                                                               tt),
    }
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, f in calls.items():
            ms[k].append(timed(f, 1))
    res = {k: round(float(np.median(v)), 3) for k, v in ms.items()}
    print(json.dumps({"case": "one_query_r_inf", "n": n, "dim": dim, "nq": 1, "list_len": int(tt.item()), "ms": res}),
          flush=True)


if __name__ == "__main__":
    main()
