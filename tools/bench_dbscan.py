"""DBSCAN on the device (pn_dbscan_device_f32) against the two radius self-query calls that produce the graph it replaces.

Time: 1M x 16 f32 uniform rows at the radius of profiles/self_graph_bench.jsonl (lists of about 24, one giant cluster:
the worst case for hooking), min_samples = 10: dbscan_device against query_radius_self_device(r, 0, include_self=True)
followed by the call with the exact capacity -- the graph alone, without any clustering of it -- interleaved in one
process.  The same for Gaussian blobs with a uniform background (many clusters).  Memory: a clump of 32768 x 8 rows with
every pair inside eps, whose CSR graph would hold 2^30 entries: the handle's workspace high-water mark next to that.
Appends one JSON line to profiles/dbscan_bench.jsonl (--out).
usage: python tools/bench_dbscan.py [--reps 7] [--n 1000000] [--only uniform|blobs|clump] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import petal_neighbors_amd as pn  # noqa: E402
from petal_neighbors_amd import _lib  # noqa: E402

DEV = "cuda:0"
R_UNIFORM = 0.6450758576393127  # profiles/self_graph_bench.jsonl: mean list 24.09 with the rows themselves left out


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


def time_against_the_graph(x, eps, min_samples, reps, tag, res):
    n = x.shape[0]
    tree = pn.BallTree.from_device(x)
    _, _, _, tot = tree.query_radius_self_device(eps, 0, include_self=True)
    torch.cuda.synchronize()
    total = int(tot.item())
    ro = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    ri = torch.empty(max(total, 1), dtype=torch.int64, device=DEV)
    rt = torch.empty(1, dtype=torch.int64, device=DEV)
    lab = torch.empty(n, dtype=torch.int64, device=DEV)
    core = torch.empty(n, dtype=torch.uint8, device=DEV)
    ncl = torch.empty(1, dtype=torch.int64, device=DEV)

    def graph():
        tree.query_radius_self_device(eps, 0, include_self=True, out_offsets=ro, out_idx=ri, out_total=rt)
        tree.query_radius_self_device(eps, total, include_self=True, out_offsets=ro, out_idx=ri, out_total=rt)

    def dbscan():
        tree.dbscan_device(eps, min_samples, out_labels=lab, out_core=core, out_n_clusters=ncl)

    td, tg = interleaved(dbscan, graph, reps)
    labels = lab.cpu().numpy()
    res[tag] = {
        "n": n, "dim": x.shape[1], "eps": eps, "min_samples": min_samples, "mean_list": round(total / n, 2),
        "graph_mb": round(total * 8 / 2**20, 1), "n_clusters": int(ncl.item()),
        "noise": int(np.count_nonzero(labels < 0)), "core": int(core.sum().item()),
        "largest_cluster": int(np.bincount(labels[labels >= 0]).max()) if (labels >= 0).any() else 0,
        "dbscan_ms": [round(v, 2) for v in td], "graph_two_calls_ms": [round(v, 2) for v in tg],
        "dbscan_over_graph_median": round(float(np.median(td)) / float(np.median(tg)), 4),
    }
    tree.close()


def clump_memory(res):
    n, dim = 32768, 8
    x = uniform_rows(n, dim, 0xC10B) * 1e-3
    tree = pn.BallTree.from_device(x)
    lab = torch.empty(n, dtype=torch.int64, device=DEV)
    core = torch.empty(n, dtype=torch.uint8, device=DEV)
    ncl = torch.empty(1, dtype=torch.int64, device=DEV)
    # every workspace buffer only grows, so after the call the memory that went is the high-water mark: free memory that
    # went, less what torch reserved meanwhile
    torch.cuda.synchronize()
    free0, res0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    ms = one(lambda: tree.dbscan_device(1.0, 10, out_labels=lab, out_core=core, out_n_clusters=ncl))
    torch.cuda.synchronize()
    free1, res1 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    res["clump"] = {
        "n": n, "dim": dim, "graph_entries": n * n, "graph_mb": round(n * n * 8 / 2**20, 1),
        "dbscan_workspace_mb": round(((free0 - free1) - (res1 - res0)) / 2**20, 1),
        "n_clusters": int(ncl.item()), "one_cluster": bool((lab == 0).all().item() and core.all().item()),
        "dbscan_ms_first_call": round(ms, 1),
    }
    tree.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_dbscan"}
    if args.only in ("", "clump"):
        clump_memory(res)
    if args.only in ("", "uniform"):
        time_against_the_graph(uniform_rows(args.n, 16, 0x5E1F5EEE), R_UNIFORM, 10, args.reps, "uniform", res)
        torch.cuda.empty_cache()
    if args.only in ("", "blobs"):
        # the blobs of tests/test_gpu_dbscan.py (12 per 12000 rows, sigma 0.05, 10 % background) at the same density
        nb = max(1, args.n * 12 // 12000)
        time_against_the_graph(blob_rows(args.n, 16, nb, 0.05, 0.10, 3), 0.2, 10, args.reps, "blobs", res)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
