"""k-means on the device (pn_kmeans_assign_device_f32, pn_kmeans_device_f32) against the route a caller had before.

For n x dim f32 blob rows (1024 blobs of sigma 0.05 in the unit cube, a tenth of the rows uniform background) and nc
initial centres taken from the rows at an even stride.  Interleaved in one process, the median of --reps:
  * assign: one pn_kmeans_assign_device_f32 asked for the labels alone under PN_ENGINE_AUTO, PN_ENGINE_EXACT and
    PN_ENGINE_BF16 against mean_shift_labels_device at the same shape -- the label kernel a caller had, which gives
    no distances or inertia either;
  * iteration: kmeans_device(max_iter = 1) -- an assignment, an update and the assignment to the moved centres -- against
    the old route doing the same: labels, a torch index_add_ mean in f64, labels again.
Recorded with the times: the rows the forced filter listed for the exact kernel (the listed-row rate); the filter
kernel's own time (km_assign_filter_kernel in a torch.profiler kernel trace of three forced calls, a run of its own
after the timed ones) and its share of the bf16 MFMA peak (2.5 PFLOP/s dense), both for the 3 x 2 n nc_pad dp FLOP its
three MFMAs per step issue and for the 2 n nc dim FLOP of the products themselves; and the share the WHOLE forced call
reaches, which also packs the rows, re-ranks and answers the listed rows.
--line adds the sweep the planner's line was drawn from: nc = 4 .. 128 at every shape given with nc = 64, exact against
forced filter.
Appends one JSON line to profiles/kmeans_bench.jsonl (--out).
usage: python tools/bench_kmeans.py [--reps 5] [--shapes 100000x16x64,1000000x128x64,1000000x128x1024,1000000x128x4096]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petal_neighbors_amd as pn  # noqa: E402
from petal_neighbors_amd import _lib  # noqa: E402
from petal_neighbors_amd.errors import check  # noqa: E402
from bench_mst import DEV, blob_rows, interleaved  # noqa: E402

PEAK_BF16 = 2.5e15


def old_iteration(tree, x, centres):
    labels = tree.mean_shift_labels_device(centres, 1.0)
    sums = torch.zeros((centres.shape[0], x.shape[1]), dtype=torch.float64, device=x.device)
    sums.index_add_(0, labels, x.double())
    counts = torch.bincount(labels, minlength=centres.shape[0])
    new = torch.where((counts > 0)[:, None], (sums / counts.clamp_min(1).double()[:, None]).float(), centres)
    return new, tree.mean_shift_labels_device(new, 1.0)


def med(v):
    return round(float(np.median(v)), 3)


def filter_kernel_ms(run):
    """mean device time of km_assign_filter_kernel over three calls of run(), or None where the trace has no such kernel"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                run()
            torch.cuda.synchronize()
        for e in prof.key_averages():
            if "km_assign_filter_kernel" in e.key and e.count:
                total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                if total:
                    return total / e.count * 1e-3
    except Exception as exc:  # noqa: BLE001
        print("no kernel trace:", exc, flush=True)
    return None


def measure(x, tree, nc, reps, iteration=True):
    n, dim = x.shape
    init = x[:: max(1, n // nc)][:nc].contiguous()
    rec = {"n": n, "dim": dim, "nc": nc}

    labels_only = torch.empty(n, dtype=torch.int64, device=x.device)
    st = torch.cuda.current_stream(x.device).cuda_stream

    def assign(engine):
        def run():
            tree.set_engine(engine)
            check(_lib.lib().pn_kmeans_assign_device_f32(tree._h, init.data_ptr(), nc, 0, labels_only.data_ptr(), None, None,
                                                         C.c_void_p(st)))
        return run

    def old_assign():
        tree.mean_shift_labels_device(init, 1.0)

    fns = [assign("auto"), assign("exact"), assign("bf16"), old_assign]
    t_auto, t_exact, t_bf16, t_old = interleaved(fns, reps)
    tree.set_engine("bf16")
    before = tree.stats()["fallback_queries"]
    labels, _, _ = tree.kmeans_assign_device(init)
    torch.cuda.synchronize()
    listed = tree.stats()["fallback_queries"] - before
    tree.set_engine("auto")
    assert torch.equal(labels, tree.mean_shift_labels_device(init, 1.0))
    dp, nc_pad = -(-dim // 16) * 16, -(-nc // 32) * 32
    rec.update({"assign_auto_ms": med(t_auto), "assign_exact_ms": med(t_exact), "assign_bf16_ms": med(t_bf16),
                "old_labels_ms": med(t_old), "auto_over_old": round(med(t_auto) / med(t_old), 4),
                "listed_rows": int(listed), "listed_rate": round(listed / n, 6),
                "bf16_call_share_of_mfma_peak": round(2.0 * n * nc_pad * dp / (med(t_bf16) * 1e-3) / PEAK_BF16, 4)})
    if iteration:
        t_k = filter_kernel_ms(assign("bf16"))
        tree.set_engine("auto")
        if t_k:
            rec.update({"filter_kernel_ms": round(t_k, 3),
                        "filter_kernel_share_of_mfma_peak_issued": round(6.0 * n * nc_pad * dp / (t_k * 1e-3) / PEAK_BF16, 4),
                        "filter_kernel_share_of_mfma_peak_products": round(2.0 * n * nc * dim / (t_k * 1e-3) / PEAK_BF16, 4)})
        ref = [None]

        def new_it():
            tree.kmeans_device(init, 0.0, 1)

        def old_it():
            ref[0] = old_iteration(tree, x, init)

        t_new, t_oldit = interleaved([new_it, old_it], reps)
        c, lab = tree.kmeans_device(init, 0.0, 1)[:2]
        rec.update({"iteration_ms": med(t_new), "old_iteration_ms": med(t_oldit),
                    "iteration_over_old": round(med(t_new) / med(t_oldit), 4),
                    "max_abs_centre_diff_to_old": float((c - ref[0][0]).abs().max().item()),
                    "labels_differ_from_old": int((lab != ref[0][1]).sum().item())})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="100000x16x64,1000000x128x64,1000000x128x1024,1000000x128x4096")
    ap.add_argument("--line", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.jsonl"))
    args = ap.parse_args()
    res = {"tool": "bench_kmeans"}
    cache = {}
    for i, shape in enumerate(args.shapes.split(",")):
        n, dim, nc = (int(v) for v in shape.split("x"))
        if (n, dim) not in cache:
            cache.clear()
            torch.cuda.empty_cache()
            x = blob_rows(n, dim, 1024, 0.05, 0.10, 3)
            cache[(n, dim)] = (x, pn.BallTree.from_device(x))
        x, tree = cache[(n, dim)]
        res[shape] = measure(x, tree, nc, args.reps)
        print(shape, json.dumps(res[shape]), flush=True)
        if args.line and nc == 64:
            res["line_" + f"{n}x{dim}"] = [
                {k: v for k, v in measure(x, tree, c, args.reps, iteration=False).items()
                 if k in ("nc", "assign_exact_ms", "assign_bf16_ms", "old_labels_ms")} for c in (4, 8, 16, 32, 64, 128)]
            print("line", json.dumps(res["line_" + f"{n}x{dim}"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
