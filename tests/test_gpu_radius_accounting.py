"""What a call adds to pn_stats.queries and pn_stats.fallback_queries, for every entry point that goes through the device
radius pipeline (radius_device_enqueue / radius_self_enqueue of csrc/index.hip).  Each pass of the pipeline is told two
things by its caller: whether it counts its queries (``count_queries``: queries += nq, on the host) and whether the
queries its first tier lists for the exact scan are added to the device counter behind fallback_queries
(``add_listed``).  The self pipeline hands its own ``count_queries`` on to every row chunk and adds the listed rows where
it counts AND has one radius per row.

One Euclidean f32 index of 4096 x 8 rows under PN_ENGINE_BF16 (the smallest shape the first tier serves), Q = 600
external queries.  The radius R = 0.5 lists about 20 of the 4096 rows per query (tests/test_gpu_density_chunks.py: 20.6 at
0.5, the longest list 170 under radii up to 0.6), below the 224 entries a first-tier list holds, so a query at R stays
in the filter (the test asserts the longest list).  A radius of 0, -1 or NaN cannot be served by the first tier and is
listed by definition (tests/test_gpu_radii.py, test_edge_radii_euclidean); its list is empty.  Every 7th query and every
97th row gets one.

Expected growth (queries, fallback_queries), derived by hand from the call sites (N rows, Q queries, KQ / KN of them with
a listed radius):

  dbscan                     count: self pipeline, counts, scalar radius (adds no listed)       fill: counts nothing,
                             adds nothing                                                                      (N, 0)
  optics                     cores: the k-NN self-query counts its N rows; count: self pipeline told not to count, hence
                             adds nothing although it has radii; fill: nothing            (N, what query_self adds)
  kde, one h per query       count: device pipeline, counts, adds listed; fill: nothing                       (Q, KQ)
  kde_self, one h per row    count: self pipeline, counts, radii: adds listed; fill: nothing                  (N, KN)
  mean_shift, max_iter = 2   per iteration: count over the seeds still moving, counts, adds listed; fill: nothing.  The
                             seeds with a listed bandwidth have an empty list and are dead after the first iteration, so
                             the second lists none.  With tol = 0 the seeds that go on are those whose first shift is
                             > 0 (a dead seed's is NaN), A2 of them by a separate one-step call:      (Q + A2, KQ)
  query_radius_self          scalar radius: first pass counts, adds nothing (no radii); second pass counts nothing
                             host (N, 0), device (N, 0)
  query_radius_self, radii   first pass counts and adds listed; second pass neither: host (N, KN), device (N, KN)
  query_radii                host: neither pass counts (as pn_query_radius_*), the first adds listed:          (0, KQ)
                             device: one pass, counts and adds listed:                                         (Q, KQ)

OPTICS is the one entry whose fallback_queries growth is not decided by the two booleans alone: the radius passes add
nothing, the k-NN self-query of its first step adds the rows its first tier could not prove.  query_self(MIN_SAMPLES_OPTICS)
is that self-query on its own and is measured right before, in each round: OPTICS must grow both counters by exactly what
it did.  (The first k-NN call at a k on a fresh handle may send every query to the second tier and widen the plan for the
calls after it -- 4096 of 4096 here -- so the fixture makes one such call before anything is measured.)  With
MIN_SAMPLES_OPTICS = 16 of about 20 neighbours a good part of the rows has no core distance below R, hence radius 0 in
both radius passes -- listed by definition, so a pass that added its listed rows would show (the test asserts there are
such rows).  Everything is asserted exactly, and equal at both piece sizes: the default (2^27 entries: one piece) and
1000 entries, at least five pieces of every graph here (asserted from the counts).
"""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

PN_OPT_DBSCAN_PIECE, PN_OPT_OPTICS_PIECE, PN_OPT_KDE_PIECE, PN_OPT_MS_PIECE = 11, 13, 14, 15
PIECE_OPTS = (PN_OPT_DBSCAN_PIECE, PN_OPT_OPTICS_PIECE, PN_OPT_KDE_PIECE, PN_OPT_MS_PIECE)
N, DIM, Q = 4096, 8, 600
R = np.float32(0.5)
MIN_SAMPLES = 4
MIN_SAMPLES_OPTICS = 16
SMALL_PIECE = 1000
LISTED = np.array([0.0, -1.0, np.nan], dtype=np.float32)


def _radii(count, every):
    r = np.full(count, R, dtype=np.float32)
    bad = np.arange(0, count, every)
    r[bad] = np.resize(LISTED, len(bad))
    return r, len(bad)


@pytest.fixture(scope="module")
def setup(pn):
    tree = pn.BallTree.euclidean(uniform((N, DIM), 0xACC00001))
    assert tree.bf16_eligible
    tree.set_engine("bf16")
    tree.query_self(MIN_SAMPLES_OPTICS)  # (the k-NN plan settles: see the module's text on OPTICS)
    yield tree, uniform((Q, DIM), 0xACC00002)
    tree.close()


def _growths(tree, qs):
    """{entry: (growth of queries, growth of fallback_queries)} over one call each, and what the calls returned"""
    import torch
    rq, kq = _radii(Q, 7)
    rn, kn = _radii(N, 97)
    qd, rqd, rnd = torch.from_numpy(qs).cuda(), torch.from_numpy(rq).cuda(), torch.from_numpy(rn).cuda()
    torch.cuda.synchronize()
    seen = {}
    calls = {
        "dbscan": lambda: tree.dbscan(R, MIN_SAMPLES),
        "query_self": lambda: tree.query_self(MIN_SAMPLES_OPTICS),
        "optics": lambda: tree.optics(MIN_SAMPLES_OPTICS, R),
        "kde": lambda: tree.kernel_density_raw(qs, rq, "epanechnikov"),
        "kde_self": lambda: tree.kernel_density_raw(None, rn, "epanechnikov"),
        "mean_shift": lambda: tree.mean_shift_modes(rq, qs, tol=0.0, max_iter=2, full=True),
        "radius_self_host": lambda: tree.query_radius_self(R, with_distance=True),
        "radius_self_device": lambda: tree.query_radius_self_device(R, 64 * N, with_distance=True),
        "radii_self_host": lambda: tree.query_radius_self(rn, with_distance=True),
        "radii_self_device": lambda: tree.query_radius_self_device(rnd, 64 * N, with_distance=True),
        "radii_host": lambda: tree.query_radius_with_distance_batch(qs, rq),
        "radii_device": lambda: tree.query_radius_with_distance_device(qd, rqd, 64 * Q),
    }
    out = {}
    for name, call in calls.items():
        before = tree.stats()
        seen[name] = call()
        torch.cuda.synchronize()
        after = tree.stats()
        out[name] = (after["queries"] - before["queries"], after["fallback_queries"] - before["fallback_queries"])
    return out, seen, kq, kn


def test_queries_and_fallback_queries_grow_as_the_call_sites_say(setup):
    tree, qs = setup
    try:
        default, seen, kq, kn = _growths(tree, qs)
        for opt in PIECE_OPTS:
            tree.set_option(opt, SMALL_PIECE)
        small, _, _, _ = _growths(tree, qs)
    finally:
        for opt in PIECE_OPTS:
            tree.set_option(opt, 0)
    for name in default:
        print(f"{name}: (queries, fallback_queries) grew by {default[name]} at the default piece, {small[name]} at {SMALL_PIECE}")
    # the graphs are cut: every list is shorter than the small piece, so a graph of T entries has at least T / piece pieces
    self_off = seen["radius_self_host"][0]
    kde_cnt, self_cnt = seen["kde"][1], seen["kde_self"][1]
    core = seen["optics"][3]
    optics_total = int(np.diff(self_off.astype(np.int64))[np.isfinite(core)].sum())
    totals = {"dbscan": int(self_off[-1]) + N, "optics": optics_total, "kde": int(kde_cnt.sum()), "kde_self": int(self_cnt.sum()),
              "mean_shift": int(kde_cnt.sum())}  # (its first iteration asks the lists of "kde")
    print(f"entries per graph: {totals}; longest list {int(max(kde_cnt.max(), np.diff(self_off.astype(np.int64)).max() + 1))}")
    assert max(kde_cnt.max(), np.diff(self_off.astype(np.int64)).max() + 1) < min(SMALL_PIECE, 224)
    for name, total in totals.items():
        assert total >= 5 * SMALL_PIECE, f"{name}: {total} entries are fewer than five pieces of {SMALL_PIECE}"
    iterations, seed_steps = seen["mean_shift"][4]
    first_shift = tree.mean_shift_modes(_radii(Q, 7)[0], qs, tol=0.0, max_iter=1, full=True)[3]
    a2 = int(np.count_nonzero(first_shift > 0))  # (NaN, a dead seed, compares false)
    print(f"mean shift: {a2} of {Q} seeds go on after the first step; the library reports {seed_steps} seed-steps")
    assert iterations == 2 and 0 < a2 <= Q - kq  # the second iteration ran, without the dead
    undefined = int(np.count_nonzero(~np.isfinite(core)))
    print(f"optics: {undefined} of {N} rows without a core distance below R (radius 0 in the radius passes)")
    assert undefined >= 100
    want = {
        "dbscan": (N, 0),
        "kde": (Q, kq),
        "kde_self": (N, kn),
        "mean_shift": (Q + a2, kq),
        "radius_self_host": (N, 0),
        "radius_self_device": (N, 0),
        "radii_self_host": (N, kn),
        "radii_self_device": (N, kn),
        "radii_host": (0, kq),
        "radii_device": (Q, kq),
    }
    for name, w in want.items():
        assert default[name] == w, f"{name} at the default piece: grew by {default[name]}, the call sites say {w}"
        assert small[name] == w, f"{name} at pieces of {SMALL_PIECE}: grew by {small[name]}, the call sites say {w}"
    for got, at in ((default, "the default piece"), (small, f"pieces of {SMALL_PIECE}")):
        assert got["query_self"][0] == N and got["query_self"][1] <= N, f"query_self at {at}: grew by {got['query_self']}"
        assert got["optics"] == got["query_self"], f"optics at {at}: grew by {got['optics']}, query_self by {got['query_self']}"
