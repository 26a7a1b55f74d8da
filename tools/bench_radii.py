"""Per-query radii against the scalar radius call, 1M x 128 f32, 10^4 device-resident queries (the headline's radius run).

Three figures at the radius profiles/r04_bench_c2_radius_nn.json used (the median nearest-neighbour distance), indices only:
  (a) pn_query_radius_device_f32 of a PARENT build of the library (--parent-lib <path to its libpetal_mi355x.so>)
  (b) the same call of this build
  (c) pn_query_radii_device_f32 of this build with a constant array
(a) runs in processes of its own (PN_LIBRARY_PATH), alternating with the process that times (b) and (c) call by call, all
on one device; the spread of (a) over its runs is the yardstick for (b) - (a) and (c) - (a).  Every figure is the median
of device-event times of single calls; the host clock around the same synchronised calls is recorded next to it.
Then, for the record: a heavy-tailed batch (radius of query q = its k_q-th neighbour distance, k_q log-uniform in 1 .. 200)
through the new entry point with distances, against one scalar call at the largest radius with distances, filtered afterwards.
usage (GPU): python tools/bench_radii.py [--parent-lib PATH] [--runs 5] [--reps 20] [--out profiles/radii_c2.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS = 3.4869062900543213  # profiles/r04_bench_c2_radius_nn.json: the median nearest-neighbour distance of this workload


def worker(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import petal_neighbors_amd as pn
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    n, dim, nq = args.n, 128, args.nq
    pts = torch.empty((n, dim), dtype=torch.float32, device="cuda:0")
    qs = torch.empty((nq, dim), dtype=torch.float32, device="cuda:0")
    L.pn_fill_uniform_device_f32(pts.data_ptr(), n * dim, 0x5EED0001, 0, 0, None)
    L.pn_fill_uniform_device_f32(qs.data_ptr(), nq * dim, 0x5EED0002, 0, 0, None)
    torch.cuda.synchronize()
    tree = pn.BallTree.from_device(pts)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

    def interleaved(calls, reps):
        for f in calls.values():  # warm the workspaces
            f()
            f()
        torch.cuda.synchronize()
        ev, host = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(reps):
            for k, f in calls.items():
                e, h = timed(f)
                ev[k].append(e)
                host[k].append(h)
        return ({k: round(float(np.median(v)), 4) for k, v in ev.items()},
                {k: round(float(np.median(v)), 4) for k, v in host.items()})

    r = RADIUS
    _, _, tot = tree.query_radius_device(qs, r, 0)
    torch.cuda.synchronize()
    cap = int(tot.item())
    offs = torch.empty(nq + 1, dtype=torch.int64, device="cuda:0")
    idx = torch.empty(max(cap, 1), dtype=torch.int64, device="cuda:0")
    tt = torch.empty(1, dtype=torch.int64, device="cuda:0")
    calls = {"scalar": lambda: tree.query_radius_device(qs, r, cap, out_offsets=offs, out_idx=idx, out_total=tt)}
    res = {"total": cap}
    if not args.scalar_only:
        rad = torch.full((nq,), r, dtype=torch.float32, device="cuda:0")
        calls["radii"] = lambda: tree.query_radius_device(qs, rad, cap, out_offsets=offs, out_idx=idx, out_total=tt)
    res["ms"], res["host_ms"] = interleaved(calls, args.reps)
    if not args.scalar_only:  # the two entry points give the same answer
        want = (offs.clone(), idx.clone())
        calls["scalar"]()
        torch.cuda.synchronize()
        res["radii_equals_scalar"] = bool(torch.equal(offs, want[0]) and torch.equal(idx, want[1]))
    if args.heavy_tail:
        kmax = 200
        kd = torch.empty((nq, kmax), dtype=torch.float32, device="cuda:0")
        ki = torch.empty((nq, kmax), dtype=torch.int64, device="cuda:0")
        tree.query_device(qs, kmax, out_idx=ki, out_dist=kd)
        torch.cuda.synchronize()
        kq = np.clip(np.exp(np.random.default_rng(8103).uniform(0.0, np.log(kmax + 1.0), nq)).astype(np.int64), 1, kmax)
        kdh = kd.cpu().numpy()
        radii_h = np.nextafter(kdh[np.arange(nq), kq - 1], np.float32(np.inf))
        radii = torch.from_numpy(radii_h).to("cuda:0")
        rmax = float(radii_h.max())
        total = int(kq.sum())
        _, _, tmax = tree.query_radius_device(qs, rmax, 0)
        torch.cuda.synchronize()
        cmax = int(tmax.item())
        ht = {"k_max": kmax, "total": total, "r_max": rmax, "total_at_r_max": cmax}
        if cmax > args.max_entries:
            ht["workaround"] = f"not measured: {cmax} entries at the largest radius exceed --max-entries"
        o1 = torch.empty(nq + 1, dtype=torch.int64, device="cuda:0")
        i1 = torch.empty(total + nq, dtype=torch.int64, device="cuda:0")
        d1 = torch.empty(total + nq, dtype=torch.float32, device="cuda:0")
        hcalls = {"radii": lambda: tree.query_radius_with_distance_device(qs, radii, total + nq, False, o1, i1, d1, tt)}
        if cmax <= args.max_entries:
            o2 = torch.empty(nq + 1, dtype=torch.int64, device="cuda:0")
            i2 = torch.empty(max(cmax, 1), dtype=torch.int64, device="cuda:0")
            d2 = torch.empty(max(cmax, 1), dtype=torch.float32, device="cuda:0")

            def workaround():
                tree.query_radius_with_distance_device(qs, rmax, cmax, False, o2, i2, d2, tt)
                row = torch.repeat_interleave(torch.arange(nq, device="cuda:0"), o2[1:] - o2[:-1], output_size=cmax)
                keep = d2[:cmax] < radii[row]
                return i2[:cmax][keep], d2[:cmax][keep], torch.bincount(row[keep], minlength=nq)
            hcalls["scalar_at_r_max_then_filter"] = workaround
        tree.stats(reset=True)
        hcalls["radii"]()
        torch.cuda.synchronize()
        ht["fallback_queries_per_call"] = int(tree.stats()["fallback_queries"])
        ht["ms"], ht["host_ms"] = interleaved(hcalls, max(3, args.reps // 4))
        res["heavy_tail"] = ht
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--max-entries", type=int, default=150_000_000)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--scalar-only", action="store_true")
    ap.add_argument("--heavy-tail", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def run(lib, extra):
        env = dict(os.environ)
        env.pop("PN_LIBRARY_PATH", None)
        if lib:
            env["PN_LIBRARY_PATH"] = os.path.abspath(lib)
            env["PN_LIBRARY_OLDER"] = "1"  # (a parent build does not export the new symbols: _lib.py leaves them unbound)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(args.reps), "--n", str(args.n),
               "--nq", str(args.nq), "--max-entries", str(args.max_entries)] + extra
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:  # a failed run ends the measurement: nothing more is started on the device
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"worker failed with status {p.returncode}")
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])

    a, bc = [], []
    for i in range(args.runs):  # alternating processes on one device
        if args.parent_lib:
            a.append(run(args.parent_lib, ["--scalar-only"]))
        bc.append(run(None, ["--heavy-tail"] if i == args.runs - 1 else []))
        print(f"run {i}: a {a[-1]['ms'] if a else None}  b/c {bc[-1]['ms']}", flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {"workload": f"{args.n} x 128 f32 uniform[0,1), {args.nq} device-resident queries, indices only, r = {RADIUS}",
           "unit": "ms per batch: median over the runs of each run's median device-event time of single calls",
           "runs": args.runs, "reps_per_run": args.reps, "results_per_batch": bc[0]["total"],
           "b_scalar_this_build": {"ms": med([x["ms"]["scalar"] for x in bc]), "runs": [x["ms"]["scalar"] for x in bc],
                                   "host_clock_runs": [x["host_ms"]["scalar"] for x in bc]},
           "c_radii_constant_array": {"ms": med([x["ms"]["radii"] for x in bc]), "runs": [x["ms"]["radii"] for x in bc],
                                      "host_clock_runs": [x["host_ms"]["radii"] for x in bc]},
           "radii_equals_scalar": all(x["radii_equals_scalar"] for x in bc)}
    if a:
        am = [x["ms"]["scalar"] for x in a]
        out["a_scalar_parent_build"] = {"ms": med(am), "runs": am, "host_clock_runs": [x["host_ms"]["scalar"] for x in a]}
        out["a_spread_max_minus_min"] = round(max(am) - min(am), 4)
        out["b_minus_a"] = round(out["b_scalar_this_build"]["ms"] - med(am), 4)
        out["c_minus_a"] = round(out["c_radii_constant_array"]["ms"] - med(am), 4)
    else:
        out["a_scalar_parent_build"] = "not measured (no --parent-lib)"
    out["heavy_tail"] = bc[-1].get("heavy_tail")
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
