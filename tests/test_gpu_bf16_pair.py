"""The paired main-pass kernel of the bf16 tier (bf16_filter_kernel_pair: one 8-wave workgroup serves two adjacent
query tiles over one row range, the SIMD partners in anti-phase), forced with PN_OPT_BF16_WAVES = 16.  Answers are
compared bit for bit with the oracle's brute force; a child process under PN_DEBUG_PLAN checks which kernel every
one of these calls really launched, so that the parity tests cannot pass without the kernel.

The shapes are the smallest at which this kernel can go wrong AND applies (64-slot buffers: see CASES): the shortest
runs this corpus can have (an aligned grid needs a workgroup per query tile and the plan gives a workgroup ~9-12 row tiles
at the least, so runs of one to four tiles cannot be reached through a call and their guards in the kernel stay
unexercised: PN_OPT_SEGMENTS = 66 / 33 / 22 / 16 on a 66-tile corpus all come out as 16- and 17-tile runs with a partial
last tile), a long run, full pairs and pairs whose upper half has no queries (odd number of query tiles), every
KS of both layouts, frequent survivors, ties, an f64 index."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, uniform

pytestmark = pytest.mark.gpu
PAIR = 16


SEG = 2  # PN_OPT_SEGMENTS


def _u(n, dim, nq, seed, dtype=np.float32):
    return uniform((n, dim), seed, dtype), uniform((nq, dim), seed + 1, dtype)


def _heterogeneous():
    # rows of very different norms keep the per-row error columns: D = 128 then takes nine MFMA steps (KS = 9)
    rng = np.random.default_rng(9)
    pts = uniform((20000, 128), 31) * (10.0 ** rng.integers(-2, 3, size=(20000, 1))).astype(np.float32)
    qs = pts[rng.integers(0, 20000, size=520)] + uniform((520, 128), 32) * np.float32(0.01)
    return pts, qs


def _duplicated():
    base = uniform((20000, 32), 41)
    pts = np.concatenate([base, base[:10000], base[:6000]]).astype(np.float32)  # exact duplicates -> distance ties
    qs = np.concatenate([base[:300], uniform((300, 32), 42)]).astype(np.float32)
    return pts, qs


def _clustered():
    # sorted by cluster: all neighbours of a query sit in one segment, whose checks find survivors all the time --
    # rare path and compactions in both roles
    rng = np.random.default_rng(3)
    centers = rng.random((16, 48), dtype=np.float32) * 10
    pts = np.concatenate([c + 0.05 * rng.standard_normal((2300, 48), dtype=np.float32) for c in centers]).astype(np.float32)
    qs = (centers[rng.integers(0, 16, 600)] + 0.05 * rng.standard_normal((600, 48), dtype=np.float32)).astype(np.float32)
    return pts, qs


# name -> (data key, data builder, queries used, k, {option: value}, the paired kernel applies).
# A buffer has 64 slots while k' <= 16, and the plan's k' grows with the relevant rows PER SEGMENT (2 k + 4 over the
# segments of a query): the shapes give k = 10 at least 8 segments per query tile, k = 25 at least 17, k = 1 at least 2 --
# test_every_case_launches_the_kernel_it_is_meant_for checks under PN_DEBUG_PLAN that this worked out.
CASES = {}
# 66 row tiles, the last one partial.  The plan caps the workgroups of two query tiles at a sixteenth of the (query tile,
# row tile) pairs, so 66 / 33 / 22 / 16 ranges all come out as 4 ranges of 16-17 tiles: prologue, drain, a partial tile.
for _s in (66, 33, 22, 16):
    CASES["short_runs_%d" % _s] = ("short", lambda: _u(4200, 128, 512, 5101), 512, 1, {SEG: _s}, True)
CASES["long_run"] = ("long", lambda: _u(70000, 128, 1000, 5103), 1000, 10, {SEG: 8}, True)  # 8 ranges of 136-137 tiles
# one full pair (257, 512); odd numbers of query tiles, the last pair's upper half without queries (600: 3, 1100: 5);
# three pairs with a partial last tile (1300); two full pairs (1024); a single query tile: the kernel does not apply
for _nq in (257, 512, 600, 1100, 1300, 1024, 256, 1):
    CASES["pairs_%d" % _nq] = ("pairs", lambda: _u(20000, 64, 1300, 5105), _nq, 10, {}, _nq > 256)
for _d in (128, 96, 64, 33, 17, 8):  # every KS of the norm-in-the-accumulator layout and of short rows
    CASES["dim_%d" % _d] = (("dim", _d), functools.partial(_u, 20000, _d, 600, 5200 + _d), 600, 10, {}, True)
CASES["five_columns_ks9"] = ("het", _heterogeneous, 520, 10, {}, True)
for _k in (1, 10, 25):
    CASES["duplicated_k%d" % _k] = ("dup", _duplicated, 600, _k, {}, True)
    CASES["clustered_k%d" % _k] = ("clu", _clustered, 600, _k, {}, True)
CASES["f64"] = ("f64", lambda: _u(20000, 96, 600, 5301, np.float64), 600, 10, {}, True)

_DATA, _ORACLE = {}, {}


def _data(case):
    key, build = CASES[case][:2]
    if key not in _DATA:
        _DATA[key] = build()
    return _DATA[key]


def _tree(pn, pts, opts=None, waves=PAIR):
    from petal_neighbors_amd import _lib
    tree = pn.BallTree.euclidean(pts)
    assert tree.bf16_eligible
    tree.set_engine("bf16")
    tree.set_option(_lib.PN_OPT_BF16_WAVES, waves)
    for o, v in (opts or {}).items():
        tree.set_option(o, v)
    return tree


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_brute_force(pn, oracle_mod, case):
    key, _, nq, k, opts, _ = CASES[case]
    pts, qs = _data(case)
    if (key, k) not in _ORACLE:  # once per (corpus, queries, k); cases with fewer queries slice it
        _ORACLE[(key, k)] = oracle_mod.brute_knn(pts, qs, k)
    oi, od = _ORACLE[(key, k)]
    tree = _tree(pn, pts, opts)
    if case == "five_columns_ks9":
        assert tree.bf16_layout == 1
    idx, dist = tree.query_batch(qs[:nq], k)
    assert dist.tobytes() == od[:nq].tobytes(), "distances differ"
    assert np.array_equal(idx, oi[:nq]), "indices differ"


def test_candidate_statistics_equal_the_4_wave_kernels(pn):
    """Same seeds, same 64 queries per wave, same row order per segment: the paired kernel keeps and evaluates exactly
    the candidates the 4-wave kernel does (two runs of the 4-wave kernel agree with each other first)."""
    from petal_neighbors_amd import _lib
    pts, qs = _data("long_run")
    got = []
    for waves in (4, 4, PAIR):
        tree = _tree(pn, pts, {SEG: 8, _lib.PN_OPT_SHARED_THRESHOLDS: 0}, waves=waves)
        tree.stats(reset=True)
        idx, dist = tree.query_batch(qs, 10)
        st = tree.stats()
        got.append((st["candidates"], st["evaluations"], idx, dist))
    print("candidates, evaluations:", [g[:2] for g in got])
    assert got[0][:2] == got[1][:2], "the 4-wave kernel does not reproduce its own statistics"
    assert got[2][:2] == got[0][:2]
    assert np.array_equal(got[2][2], got[0][2]) and got[2][3].tobytes() == got[0][3].tobytes()


# The child: every parity case's call, then the calls on which the kernel must NOT apply, each announced on stderr
_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import petal_neighbors_amd as pn
from petal_neighbors_amd import _lib
import test_gpu_bf16_pair as T
def call(name, pts, qs, k, opts, waves=T.PAIR):
    tree = T._tree(pn, pts, opts, waves=waves)
    sys.stderr.write("\nCASE %s\n" % name)
    sys.stderr.flush()
    tree.query_batch(qs, k)
for name in sorted(T.CASES):
    key, _, nq, k, opts, _ = T.CASES[name]
    pts, qs = T._data(name)
    call(name, pts, qs[:nq], k, opts)
pts, qs = T._u(82000, 64, 600, 7)
call("refreshers", pts, qs, 10, {T.SEG: 4, _lib.PN_OPT_SEED_MODEL: 0, _lib.PN_OPT_SHARED_THRESHOLDS: 44})
pts, qs = T._data("pairs_600")
call("k100", pts, qs[:600], 100, {})
# the library's own choice on a grid that leaves workgroup slots empty: 3 query tiles x 4 ranges of 320 tiles, 64-slot buffers
pts, qs = T._u(82000, 64, 600, 7)
call("auto_few_tiles", pts, qs, 1, {T.SEG: 4, _lib.PN_OPT_SHARED_THRESHOLDS: 0}, waves=0)  # (no refreshers: the kernel could run)
"""


def test_every_case_launches_the_kernel_it_is_meant_for(tmp_path):
    """PN_DEBUG_PLAN names the main-pass kernel of a call (a fresh process: the switch is read once).  Every parity
    case above must have run the paired kernel -- they are not allowed to pass without it -- and the 4-wave kernel
    where the paired one must not apply: a single query tile, refreshers on, 128-slot buffers (k = 100) -- or is not
    chosen: the automatic choice on a grid that leaves workgroup slots empty."""
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
    expect = {name: c[5] for name, c in CASES.items()}
    expect.update(refreshers=False, k100=False, auto_few_tiles=False)
    assert set(seen) == set(expect)
    for name, applies in expect.items():
        kern, plan = seen[name]
        if applies:
            assert all(kk == ("pair", kk[1], "512") for kk in kern), (name, kern, plan)
        else:
            assert all(kk[0] == "4" and kk[2] == "256" for kk in kern), (name, kern, plan)
    assert " n_refresh 0 " not in seen["refreshers"][1], seen["refreshers"][1]  # (not vacuous: refreshers really on)
    assert " cap 128 " in seen["k100"][1], seen["k100"][1]
    # the automatic choice leaves a grid that does not fill the workgroup slots to the 4-wave kernel, although the
    # paired kernel would apply (64-slot buffers, 3 query tiles, runs of 320 tiles)
    few = seen["auto_few_tiles"][1]
    assert " cap 64 " in few and " q_tiles 3 " in few and " n_wg 12 " in few and " n_refresh 0 " in few, few
    assert " q_tiles 1 " in seen["pairs_256"][1] and " q_tiles 1 " in seen["pairs_1"][1]
    # the empty upper half: an odd number of query tiles on a grid of (q_tiles + 1) / 2 pairs
    for name, qt in (("pairs_600", 3), ("pairs_1100", 5)):
        kern, plan = seen[name]
        per = int(re.search(r" per_tile (\d+) ", plan).group(1))
        assert " q_tiles %d " % qt in plan and int(kern[0][1]) == (qt + 1) // 2 * per, (name, kern, plan)
