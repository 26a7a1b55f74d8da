"""The two ends of the main-pass kernel choice meet: what bf16_main_kernel (csrc/bf16_launch.h, tested on the CPU by
test_bf16_choice.py) decides in the plan is what the launcher runs, and the answers are the oracle's.

One child process under PN_DEBUG_PLAN (a fresh process: the switch is read once) makes every call of CALLS on a
20000 x 64 uniform corpus, compares each answer bit for bit with the oracle's brute force, and announces each call on
stderr; the test then reads which main-pass kernel each call launched.

EXPECT was RECORDED, not derived: the same child ran against the library built from the commit before the choice moved
into the plan (8dd9a9a, where the launcher chose), on an MI355X (256 CUs: 512 workgroup slots); the kernels it named
are the literal table below.  A radius pass is not a main pass of a k-NN call and names no kernel."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, uniform

pytestmark = pytest.mark.gpu

# name: (kind, queries, k, PN_OPT_BF16_WAVES)
CALLS = {}
for _w in (0, 4, 8, 16):
    CALLS["k10_nq600_waves%d" % _w] = ("knn", 600, 10, _w)
for _w in (0, 8, 16):
    CALLS["k100_nq600_waves%d" % _w] = ("knn", 600, 100, _w)
for _w in (8, 16):
    CALLS["k10_nq256_waves%d" % _w] = ("knn", 256, 10, _w)
CALLS["radius_nq600_waves16"] = ("radius", 600, 0, 16)

# the kernels named on stderr per call, recorded on the parent commit's library (see above)
EXPECT = {
    "k10_nq600_waves0": ["8"],      # 3 query tiles x 10 runs of 31-32 tiles: short runs
    "k10_nq600_waves4": ["4"],
    "k10_nq600_waves8": ["8"],
    "k10_nq600_waves16": ["pair"],
    "k100_nq600_waves0": ["8"],     # 128-slot buffers
    "k100_nq600_waves8": ["8"],
    "k100_nq600_waves16": ["4"],    # the paired kernel serves 64-slot buffers only
    "k10_nq256_waves8": ["8"],
    "k10_nq256_waves16": ["4"],     # one query tile: nothing to pair
    "radius_nq600_waves16": [],
}


def run_calls(pn, oracle, err):
    """Every call of CALLS, announced on `err`; raises where an answer differs from the oracle's brute force."""
    from petal_neighbors_amd import _lib
    pts, qs = uniform((20000, 64), 6101), uniform((600, 64), 6102)
    tree = pn.BallTree.euclidean(pts)
    assert tree.bf16_eligible
    tree.set_engine("bf16")
    want = {k: oracle.brute_knn(pts, qs, k) for k in (10, 100)}
    radius = np.float32(float(want[10][1][0, 4]) * 1.000001)  # query 0 has four rows within it: a handful per query
    for name, (kind, nq, k, waves) in CALLS.items():
        tree.set_option(_lib.PN_OPT_BF16_WAVES, waves)
        err.write("\nCASE %s\n" % name)
        err.flush()
        if kind == "knn":
            idx, dist = tree.query_batch(qs[:nq], k)
            assert dist.tobytes() == want[k][1][:nq].tobytes(), name + ": distances differ"
            assert np.array_equal(idx, want[k][0][:nq]), name + ": indices differ"
        else:
            offsets, idx = tree.query_radius_batch(qs[:nq], radius)
            lists = [oracle.brute_radius(pts, qs[q], radius) for q in range(nq)]
            assert np.array_equal(offsets, np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)), name
            assert np.array_equal(idx, np.concatenate(lists).astype(np.uint64)), name + ": neighbours differ"
            assert 0 < len(idx) < 40 * nq, (name, len(idx))  # (not vacuous, and no overflow to the exact engine)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import oracle
import petal_neighbors_amd as pn
import test_gpu_bf16_choice as T
oracle.build()
T.run_calls(pn, oracle, sys.stderr)
"""


def kernels_named(stderr):
    """{call: [kernel named per main-pass launch]} from a child's stderr."""
    seen = {}
    for chunk in stderr.split("\nCASE ")[1:]:
        name = chunk.split("\n", 1)[0].strip()
        seen[name] = [k for k, _, _ in re.findall(r"^bf16 main pass: kernel (\S+) grid (\d+) x (\d+)$", chunk, re.M)]
    return seen


def test_every_call_launches_the_kernel_the_parent_library_launched(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    env = dict(os.environ, PN_DEBUG_PLAN="1")
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = kernels_named(r.stderr)
    assert set(seen) == set(CALLS) == set(EXPECT)
    assert seen == EXPECT, {n: (seen[n], EXPECT[n]) for n in CALLS if seen[n] != EXPECT[n]}
    assert len(re.findall(r"^bf16_plan: ", r.stderr, re.M)) == sum(c[0] == "knn" for c in CALLS.values())
