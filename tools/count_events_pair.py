"""Where a wave of the paired main-pass kernels spends its run, per role (leading half = waves 0-3, lagging half =
waves 4-7), at C2 (1M x 128, 10k queries, k = 10).  Needs a PN_DIAG_FLAGS=-DPN_DIAG_BF_COUNT build, loaded with
PN_LIBRARY_PATH (add -DPN_DIAG_PAIR_MEET=1 for today's one-tile schedule under the two-tile kernel's entry).
usage: count_events_pair.py [waves]     (waves: PN_OPT_BF16_WAVES, default 0 = the library's choice; 16 / 32 force a kernel)
The stamps cost: every chain is bracketed by two s_memtime and an lgkmcnt(0) behind it, so shares are comparable between
two stamped builds, not with an unstamped run."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import petal_neighbors_amd as pn
from petal_neighbors_amd import _lib

L = _lib.lib()
waves = int(sys.argv[1]) if len(sys.argv) > 1 else 0
n, dim, nq, k = int(os.environ.get("PN_N", 1_000_000)), 128, 10_000, 10
pts = torch.empty((n, dim), dtype=torch.float32, device="cuda:0")
qs = torch.empty((nq, dim), dtype=torch.float32, device="cuda:0")
L.pn_fill_uniform_device_f32(pts.data_ptr(), n * dim, 0x5EED0001, 0, 0, None)
L.pn_fill_uniform_device_f32(qs.data_ptr(), nq * dim, 0x5EED0002, 0, 0, None)
torch.cuda.synchronize()
t = pn.BallTree.from_device(pts)
t.set_engine("bf16")
t.set_option(_lib.PN_OPT_BF16_WAVES, waves)
reads = []
for name in ("pn_debug_read_bf", "pn_debug_read_bf_lag"):
    f = getattr(L, name)
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int]
    reads.append(f)
out = [(C.c_ulonglong * 16)(), (C.c_ulonglong * 16)()]
t.query_device(qs, k); torch.cuda.synchronize()
for f, o in zip(reads, out): f(o, 1)   # (the index build's calibration launch and the warm-up call: dropped)
t.query_device(qs, k); torch.cuda.synchronize()
for f, o in zip(reads, out): f(o, 1)
res = {"waves_option": waves, "flags": os.environ.get("PN_LIBRARY_PATH", ""), "roles": {}}
for role, o in zip(("lead_waves_0_3", "lag_waves_4_7"), out):
    run = float(o[7])
    res["roles"][role] = {
        "run_cycles_sum": run,
        "meeting_share": o[6] / run,          # arrival at bf_wait_dma .. leaving s_barrier
        "bf_slow_share": o[3] / run,
        "chains_share": (o[9] + o[10]) / run,  # chain A without the meeting inside it, chain B
        "bf_slow_entries": int(o[0]), "cycles_per_entry": o[3] / max(o[0], 1),
    }
st = t.stats()
res["fallback_queries"] = st["fallback_queries"]
res["candidates_per_query"] = st["candidates"] / max(st["queries"], 1)
print(json.dumps(res, indent=1))
