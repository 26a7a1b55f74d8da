"""The paired main-pass kernel with two row tiles per workgroup meeting (bf16_filter_kernel_meet_pair<KS, CI, 2>: one
s_barrier per PAIR of tiles, a ring of six LDS tile buffers), forced with PN_OPT_BF16_WAVES = 32.  On one handle the
same call is answered by this kernel, by the 4-wave kernel (PN_OPT_BF16_WAVES = 4) and by the exact engine: indices
and distance bits must be equal, and stats() candidates, evaluations and fallback_queries equal to the 4-wave kernel's
(same cells, same writers, same order of a wave's appends).  A child process under PN_DEBUG_PLAN checks that every
case really launched the two-tile kernel and at which run length.

Shapes: the smallest at which the schedule can go wrong.  The kernel is forced below the automatic choice's run
length the way tests/test_gpu_bf16_pair.py does (the option forces it wherever it applies).  The plan gives a workgroup
no fewer than ~9-12 row tiles and caps the workgroups of two or three query tiles, so the shortest aligned runs a call
can reach on these corpora are 16 tiles long, 32 with three query tiles (RUNS below, asserted from the plan's own debug
line): runs of one to four tiles -- a run that is all prologue, or whose only iteration is half a super-tile -- cannot
be reached through a call, their guards stay argued in the kernel's comment, and no such case is constructed another way.  What is reached:
  * even:  64 row tiles in 4 ranges of 16 (two query tiles) or 2 of 32 (three) -- every run a whole number of tile
           pairs, the shortest run;
  * odd:   68 row tiles in 4 ranges of 17, or 66 in 2 of 33 -- every run ends with half a super-tile (one tile, one
           barrier), the odd length right after the shortest run;
  * mixed: 66 row tiles in ranges of 16 and 17, or 67 in ranges of 33 and 34, the last tile partial;
  * sweep: 20 000 rows of 16 / 64 / 96 / 128 columns (KS and the DMA pieces per wave differ), k = 1 and k = 10;
  * five_columns: rows of very different norms keep the error columns -- the other tile layout (CI off), KS = 9;
each with three query tiles (600 queries: the last pair's upper half has no queries) and with two (512)."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, uniform

pytestmark = pytest.mark.gpu
FOUR, PAIR2 = 4, 32
SEG = 2  # PN_OPT_SEGMENTS


def _u(n, dim, nq, seed):
    return uniform((n, dim), seed), uniform((nq, dim), seed + 1)


def _heterogeneous():
    rng = np.random.default_rng(9)
    pts = uniform((20000, 128), 31) * (10.0 ** rng.integers(-2, 3, size=(20000, 1))).astype(np.float32)
    qs = pts[rng.integers(0, 20000, size=600)] + uniform((600, 128), 32) * np.float32(0.01)
    return pts, qs


# name -> (data key, builder, queries used, k, options, layout (2: norm in the accumulator, 1: five columns, None: the index's choice))
CASES = {}
# (two query tiles get 4 row ranges on these corpora, three get 2: the row counts differ so that the parities hold)
for _name, _nq, _rows in (("even", 512, 64 * 64), ("odd", 512, 68 * 64), ("mixed", 512, 65 * 64 + 40),
                          ("even", 600, 64 * 64), ("odd", 600, 66 * 64), ("mixed", 600, 66 * 64 + 40)):
    CASES["%s_%d" % (_name, _nq)] = (("short", _rows), lambda r=_rows: _u(r, 128, 600, 6100 + r), _nq, 1, {SEG: 66}, 2)
for _d in (16, 64, 96, 128):
    for _k in (1, 10):
        # (16 columns are too few for the norm-in-the-accumulator layout: five columns, KS = 2; at 64 and 96 columns the
        # index decides by the rows' norms: printed, not asserted)
        CASES["dim_%d_k%d" % (_d, _k)] = (("dim", _d), lambda d=_d: _u(20000, d, 600, 6200 + d), 600, _k, {}, {16: 1, 128: 2}.get(_d))
CASES["dim_128_k10_512"] = (("dim", 128), lambda: _u(20000, 128, 600, 6200 + 128), 512, 10, {}, 2)
CASES["five_columns_k10"] = ("het", _heterogeneous, 600, 10, {}, 1)
CASES["five_columns_k1_512"] = ("het", _heterogeneous, 512, 1, {}, 1)

# The plan's answer for the short-run cases, (row tiles, workgroups per query tile, run_tiles = tiles // workgroups):
# what the parity of the run lengths below rests on.  The sweep's run lengths are printed, and only their existence
# and the kernel are asserted.
RUNS = {"even_512": (64, 4, 16), "odd_512": (68, 4, 17), "mixed_512": (66, 4, 16),
        "even_600": (64, 2, 32), "odd_600": (66, 2, 33), "mixed_600": (67, 2, 33)}

_DATA = {}


def _data(case):
    key, build = CASES[case][:2]
    if key not in _DATA:
        _DATA[key] = build()
    return _DATA[key]


def _tree(pn, pts, opts):
    from petal_neighbors_amd import _lib
    tree = pn.BallTree.euclidean(pts)
    assert tree.bf16_eligible
    tree.set_option(_lib.PN_OPT_SHARED_THRESHOLDS, 0)
    for o, v in opts.items():
        tree.set_option(o, v)
    return tree


def _run_lengths(n_tiles, per_tile):
    return [(s + 1) * n_tiles // per_tile - s * n_tiles // per_tile for s in range(per_tile)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_two_tile_kernel_4_wave_kernel_and_exact_engine_agree(pn, case):
    from petal_neighbors_amd import _lib
    _, _, nq, k, opts, layout = CASES[case]
    pts, qs = _data(case)
    tree = _tree(pn, pts, opts)
    print(case, "layout", tree.bf16_layout)
    assert layout is None or tree.bf16_layout == layout
    got = {}
    for waves in (PAIR2, FOUR):
        tree.set_engine("bf16")
        tree.set_option(_lib.PN_OPT_BF16_WAVES, waves)
        tree.stats(reset=True)
        idx, dist = tree.query_batch(qs[:nq], k)
        st = tree.stats()
        got[waves] = (idx, dist, (st["candidates"], st["evaluations"], st["fallback_queries"]))
    tree.set_engine("exact")
    eidx, edist = tree.query_batch(qs[:nq], k)
    print(case, "candidates, evaluations, fallback queries:", got[PAIR2][2], "4-wave:", got[FOUR][2])
    for waves in (PAIR2, FOUR):
        assert got[waves][1].tobytes() == edist.tobytes(), "distances differ from the exact engine's (%d)" % waves
        assert np.array_equal(got[waves][0], eidx), "indices differ from the exact engine's (%d)" % waves
    assert got[PAIR2][2] == got[FOUR][2]
    assert got[PAIR2][2][0] > 0


def _busy(torch, stream, ms_target=150.0):
    """enqueue roughly ms_target of matrix products on `stream` (tests/test_gpu_async.py)"""
    a = torch.rand((4096, 4096), device="cuda")
    b = torch.rand((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        c = a @ b
    torch.cuda.synchronize()
    one = max((time.perf_counter() - t0) * 1e3, 0.05)
    reps = int(min(max(ms_target / one, 8), 4000))
    with torch.cuda.stream(stream):
        for _ in range(reps):
            c = a @ b
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev, c


def test_repeated_calls_on_a_busy_stream(pn):
    """Two calls enqueued back to back behind other work on the caller's stream: both come back before the stream has
    drained and both give the exact engine's answer (the second call's launch reuses the first one's workspace, cells
    and six-buffer kernel while the first may not have started)."""
    import torch
    from petal_neighbors_amd import _lib
    pts, qs = _data("odd_600")
    tree = _tree(pn, pts, {SEG: 66})
    tree.set_engine("exact")
    eidx, edist = tree.query_batch(qs, 1)
    tree.set_engine("bf16")
    tree.set_option(_lib.PN_OPT_BF16_WAVES, PAIR2)
    dq = torch.from_numpy(qs).cuda()
    tree.query_device(dq, 1)  # warm-up: workspaces, plans
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ev, keep = _busy(torch, stream)
    assert not ev.query(), "the stream drained before the test could look"
    with torch.cuda.stream(stream):
        i1, d1 = tree.query_device(dq, 1)
        i1, d1 = i1.clone(), d1.clone()
        i2, d2 = tree.query_device(dq, 1)
    assert not ev.query(), "a call waited for its stream"
    stream.synchronize()
    for i, d in ((i1, d1), (i2, d2)):
        assert d.cpu().numpy().tobytes() == edist.tobytes()
        assert np.array_equal(i.cpu().numpy().astype(np.uint64), eidx.astype(np.uint64))
    del keep


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import petal_neighbors_amd as pn
from petal_neighbors_amd import _lib
import test_gpu_bf16_pair_meet as T
for name in sorted(T.CASES):
    _, _, nq, k, opts, _ = T.CASES[name]
    pts, qs = T._data(name)
    tree = T._tree(pn, pts, opts)
    tree.set_engine("bf16")
    tree.set_option(_lib.PN_OPT_BF16_WAVES, T.PAIR2)
    sys.stderr.write("\nCASE %s\n" % name)
    sys.stderr.flush()
    tree.query_batch(qs[:nq], k)
"""


def test_every_case_launches_the_two_tile_kernel_at_its_run_length(tmp_path):
    """PN_DEBUG_PLAN (a fresh process: the switch is read once) names the main-pass kernel of a call and the plan's run
    length: no parity case above may pass without the two-tile kernel, and the short-run cases must be the even, odd and
    mixed runs they are named after."""
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    env = dict(os.environ, PN_DEBUG_PLAN="1")
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for chunk in r.stderr.split("\nCASE ")[1:]:
        name = chunk.split("\n", 1)[0].strip()
        kern = re.findall(r"^bf16 main pass: kernel (\S+) grid (\d+) x (\d+)$", chunk, re.M)
        plan = re.findall(r"^bf16_plan: .*$", chunk, re.M)
        assert kern and plan, (name, chunk[-1500:])
        seen[name] = (kern, plan[0])
    assert set(seen) == set(CASES)
    for name in sorted(CASES):
        kern, plan = seen[name]
        nq = CASES[name][2]
        q_tiles = (nq + 255) // 256
        per = int(re.search(r" per_tile (\d+) ", plan).group(1))
        run = int(re.search(r" run_tiles (\d+)$", plan).group(1))
        n_tiles = (len(_data(name)[0]) + 63) // 64
        runs = _run_lengths(n_tiles, per)
        print("%-22s q_tiles %d row tiles %d per_tile %d run_tiles %d runs %s" % (name, q_tiles, n_tiles, per, run, sorted(set(runs))))
        assert " cap 64 " in plan and " aligned 1 " in plan and " n_refresh 0 " in plan and " q_tiles %d " % q_tiles in plan, plan
        assert all(kk == ("pair2", str((q_tiles + 1) // 2 * per), "512") for kk in kern), (name, kern, plan)
        assert run == n_tiles // per and min(runs) == run
        if name in RUNS:
            assert (n_tiles, per, run) == RUNS[name], (name, n_tiles, per, run)
    for nq in (512, 600):
        assert all(r % 2 == 0 for r in _run_lengths(*RUNS["even_%d" % nq][:2]))
        assert all(r % 2 == 1 for r in _run_lengths(*RUNS["odd_%d" % nq][:2]))
        assert {r % 2 for r in _run_lengths(*RUNS["mixed_%d" % nq][:2])} == {0, 1}
        assert RUNS["odd_%d" % nq][2] == RUNS["even_%d" % nq][2] + 1  # the odd length right after the shortest run
