"""pn_nearest_foreign_* and the rounds of pn_mst_* through the plans of the bf16 first tier that take more than one stage per
segment (csrc/foreign.hip: fr_plan, fr_filter_kernel's two data buffers and three meta buffers, fr_rerank_kernel's merge).

fr_plan cuts the stream of A stages into nseg = clamp(4 n_cu / qt, 1, n_stages) segments, qt the listed-row tiles of a launch:
a segment holds two stages or more only where qt * n_stages > 4 n_cu.  The index stays small here (N = 700 rows, a 700 x 700
numpy reference) and the LIST is long instead: rows= may repeat row numbers (include/petal_mi355x.h: "any order, repeats
allowed").  Every case derives its list from the device's CU count and asserts, through a mirror of fr_sub / fr_plan, that it
lands in the plan it is named for -- on a device with another CU count it gets the same plan shape or fails loudly.

Two ways a wrong filter shows.  Unsound (a lifted key too high): a wrong answer is proven, the bits differ from numpy's.
Loose (a lifted key too low): the answers stay right and rows leak to the exact scan; only pn_stats shows it.  The header:
"the counters depend on the data alone" -- the accumulator of a pair (i, j) is one K chain whatever stage, tile or segment
j falls in and every reduction is an integer minimum of (key, j), so a listed row costs the same candidates and is proven or
not whatever the plan: the counters of a long list are the sum over its positions of what the rows cost when each is listed
once (the one-stage-per-segment plan).  That is an equality, not a tolerance.
"""
import functools

import numpy as np
import pytest

from conftest import uniform
from test_gpu_nearest_foreign import brute_force, engines, fold_distances

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE, PN_OPT_MST_BATCH, PN_OPT_FOREIGN_FILTER = 3, 12, 17
N = 700  # a partial last stage in every width class: 5 * 128 + 60 = 10 * 64 + 60 = 21 * 32 + 28
TILE = 128  # listed rows per workgroup (kFrRows)
MIN_LAUNCH = 64  # a launch of fewer listed rows takes the exact scan (kFrMinLaunch)
F32, F64 = np.float32, np.float64


# ---- the mirror of foreign.hip's planning
def padded(dim):
    return (dim + 15) // 16 * 16


def fr_sub(dp):
    return 4 if dp <= 48 else 2 if dp <= 96 else 1


def fr_plan(n, dp, nq, n_cu):
    """(qt, nseg, seg_stages) of one launch of nq listed rows against n indexed rows"""
    qt = -(-nq // TILE)
    srows, target = 32 * fr_sub(dp), 4 * n_cu
    n_stages = -(-n // srows)
    nseg = min(max(target // max(qt, 1), 1), n_stages)
    seg_stages = -(-n_stages // nseg)
    return qt, -(-n_stages // seg_stages), seg_stages


def stages_by_segment(n, dp, seg_stages):
    n_stages = -(-n // (32 * fr_sub(dp)))
    return tuple(min(seg_stages, n_stages - s) for s in range(0, n_stages, seg_stages))


def launches(m, batch):
    batch = batch or 1 << 18
    return [min(batch, m - r0) for r0 in range(0, m, batch)]


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan_of(name, dim, n_cu, n=N):
    """(m, batch) of the named plan, asserted through the mirror; batch 0 = the default"""
    dp, T = padded(dim), 4 * n_cu
    srows = 32 * fr_sub(dp)
    n_stages = -(-n // srows)
    assert n_stages >= 6 and n % srows, "every class: several stages, the last one partial"
    if name == "one_segment":  # every stage in one segment: both data buffers and all three meta buffers reused
        m, batch = TILE * T, 0
        assert launches(m, batch) == [m] and fr_plan(n, dp, m, n_cu) == (T, 1, n_stages)
    elif name == "three_segments":  # uneven segments, a partial last listed tile, a three-way merge
        qt = T // 3
        m, batch = TILE * qt - 50, 0
        assert launches(m, batch) == [m] and fr_plan(n, dp, m, n_cu) == (qt, 3, -(-n_stages // 3))
        assert stages_by_segment(n, dp, -(-n_stages // 3)) == {128: (2, 2, 2), 64: (4, 4, 3), 32: (8, 8, 6)}[srows]
    elif name == "recomputed":  # the first nseg = 4 gives seg_stages = 2, and with it nseg = 3
        qt = T // 4
        m, batch = TILE * qt, 0
        assert srows == 128 and T // qt == 4 and fr_plan(n, dp, m, n_cu) == (qt, 3, 2)
    elif name == "batches":  # three full launches and a shorter one: different plans in one scratch buffer
        m = TILE * T
        batch = 5 * m // 16
        lens = launches(m, batch)
        assert len(lens) == 4 and lens[:3] == [batch] * 3 and MIN_LAUNCH <= lens[3] < batch
        plans = [fr_plan(n, dp, q, n_cu) for q in lens]
        assert plans[0] != plans[3] and plans[0][2] > 1, plans
    else:  # "short_tail": the last launch has 63 rows and takes the exact scan
        assert name == "short_tail"
        batch = 32 * T
        m = 2 * batch + 63
        assert launches(m, batch) == [batch, batch, 63] and fr_plan(n, dp, batch, n_cu)[2] > 1
    return m, batch


def describe(name, dim, n_cu, m, batch, n=N):
    plans = sorted(set((q,) + fr_plan(n, padded(dim), q, n_cu) for q in launches(m, batch) if q >= MIN_LAUNCH), reverse=True)
    return f"plan {name} dim={dim} n_cu={n_cu} m={m}: " + "; ".join(
        f"launch of {q}: qt={qt} nseg={nseg} seg_stages={ss} {stages_by_segment(n, padded(dim), ss)}" for q, qt, nseg, ss in plans)


# ---- data whose meta data (cn, group code, core key) differs from stage to stage and from row to row
@functools.lru_cache(maxsize=None)
def dataset(kind, dim, dtype):
    """(rows, their distances in the reference's fold): computed once, shared, never written to"""
    rng = np.random.default_rng(1000 * dim + len(kind))
    if kind == "uniform":
        x = uniform((N, dim), 61 + dim, dtype)
    elif kind in ("blobs", "scattered_blobs"):
        # tight (spread 0.01) and far from the origin (centres near 1000): without the centring the slack, about 2^-12
        # |x - mu|^2, would be 10^4 times a squared distance.  With random group codes a row's nearest foreign row is a blob
        # mate at d^2 about 2 * 0.01^2 dim, and after the centring |x - mu|^2 is about s^2 dim, s the scatter of the centres
        # per coordinate: the slack is 2^-12 s^2 / (2 * 10^-4) of that d^2 in every dim.  s = 0.1: 1 %, the tier can tell
        # blob mates apart.  s = 50 ("scattered_blobs"): 3000 times it, every blob mate's lifted key sits on its floor.
        centres = 1000.0 + (0.1 if kind == "blobs" else 50.0) * rng.standard_normal((6, dim))
        x = (centres[rng.integers(0, 6, N)] + 0.01 * rng.standard_normal((N, dim))).astype(dtype)
    else:  # "extremes": zero rows, a tiny row, and more than M + 1 = 4 equal keys decided by j across stages and segments
        x = uniform((N, dim), 67 + dim, dtype)
        copies = 5 + 23 * np.arange(30)  # 30 copies of one row, over every stage of the wide classes and most of the narrow
        x[copies] = x[copies[0]]
        others = rng.permutation(np.setdiff1d(np.arange(N), copies))
        x[others[:10]] = 0
        x[others[10]] = 0
        x[others[10], dim // 2] = 1e-25
    x.setflags(write=False)
    d = fold_distances(x)
    d.setflags(write=False)
    return x, d


def random_groups(seed):
    return np.random.default_rng(seed).integers(0, 7, N)  # (no period that could divide a stage)


def spiky_core(d, seed, dtype):
    """a few times the typical nearest distance on about a tenth of the rows, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    typical = np.median(np.sort(d, axis=1)[:, 1])
    return np.where(rng.random(N) < 0.1, rng.random(N) * 4 * typical, 0).astype(dtype)


def long_list(seed, m):
    """(perm, rows): every row R or R + 1 times, rows = R copies of perm and then perm[:m % N]"""
    perm = np.random.default_rng(seed).permutation(N)
    return perm, np.tile(perm, m // N + 1)[:m].astype(np.uint64)


def tier_counters(tree, groups, core, rows=None):
    """(candidates, fallback rows) of one call under the forced tier, the handle's other counters checked on the way"""
    tree.stats(reset=True)
    out = tree.nearest_foreign(groups, core, rows=rows)
    s = tree.stats(reset=True)
    assert s["evaluations"] == s["candidates"] and s["queries"] == len(out[0])
    return out, s["candidates"], s["fallback_queries"]


def cost_of_prefix(tree, groups, core, perm, rem):
    """what the rows perm[:rem] cost when each is listed once (a launch under 64 rows would miss the tier: listed k times)"""
    if rem == 0:
        return 0, 0
    k = -(-MIN_LAUNCH // rem)
    _, c, f = tier_counters(tree, groups, core, np.tile(perm[:rem], k).astype(np.uint64))
    assert c % k == 0 and f % k == 0
    return c // k, f // k


def same_bits(got, want, where):
    idx, w = got
    assert np.array_equal(idx, want[0]), where
    assert np.array_equal(w.view(want[1].dtype), want[1]), where


def check_plan(pn, kind, dim, dtype, name):
    n_cu = cu_count()
    m, batch = plan_of(name, dim, n_cu)
    print(describe(name, dim, n_cu, m, batch))
    x, d = dataset(kind, dim, dtype)
    tree = pn.BallTree.euclidean(x)
    if batch:
        tree.set_option(PN_OPT_MST_BATCH, batch)
    groups = random_groups(dim + len(name))
    perm, rows = long_list(dim + m, m)
    counted = sum(q for q in launches(m, batch) if q >= MIN_LAUNCH)  # (a prefix of the list: only the last launch is short)
    cores = {"none": None, "knn5": tree.query_self(5)[1][:, -1].copy(), "spiky": spiky_core(d, dim, dtype)}
    for cname, core in cores.items():
        every = brute_force(d, groups, core)
        want = every[0][rows.astype(np.int64)], every[1][rows.astype(np.int64)]
        for ename, t in engines(tree):
            where = (name, kind, dim, cname, ename)
            if ename != "filter":
                same_bits(t.nearest_foreign(groups, core, rows=rows), want, where)
                continue
            once, c1, f1 = tier_counters(t, groups, core)  # every row once: one stage per segment
            same_bits(once, every, where)
            print(f"fallback {kind} dim={dim} {np.dtype(dtype).name} core={cname}: f1/N = {f1}/{N} = {f1 / N:.4f}, c1 = {c1}")
            assert c1 > 0 and f1 < N, where  # (not by handing every row to the exact scan)
            c_rem, f_rem = cost_of_prefix(t, groups, core, perm, counted % N)
            got, c, f = tier_counters(t, groups, core, rows)
            same_bits(got, want, where)
            assert (c, f) == (counted // N * c1 + c_rem, counted // N * f1 + f_rem), where
            assert c <= 3 * counted, where


DTYPE_IDS = {F32: "f32", F64: "f64"}
# one_segment and three_segments in both element types at one dim of each width class (the 64-bit keys change the meta
# buffers' size and alignment); the class edges -- dp 48 | 64 is sub 4 | 2, dp 96 | 112 is sub 2 | 1, and 48 and 96 carry
# exactly kFrPrefetch = 6 chunks per thread -- in one type each; 160: the widest row, 130,560 LDS bytes with 64-bit keys
PLAN_CASES = [(p, dim, dt) for p in ("one_segment", "three_segments") for dim in (48, 70, 160) for dt in (F32, F64)]
PLAN_CASES += [(p, dim, dt) for p in ("one_segment", "three_segments") for dim, dt in ((49, F64), (96, F32), (97, F64))]
PLAN_CASES += [("recomputed", 48, F32), ("recomputed", 33, F64)]
PLAN_CASES += [("batches", 48, F64), ("batches", 70, F32), ("batches", 160, F64)]
PLAN_CASES += [("short_tail", 48, F32), ("short_tail", 70, F64), ("short_tail", 160, F32)]


@pytest.mark.parametrize("kind", ["uniform", "blobs", "extremes"])
@pytest.mark.parametrize("name,dim,dtype", PLAN_CASES, ids=[f"{p}-{dim}-{DTYPE_IDS[dt]}" for p, dim, dt in PLAN_CASES])
def test_plans_against_brute_force_and_the_one_stage_counters(pn, name, dim, dtype, kind):
    check_plan(pn, kind, dim, dtype, name)


def test_a_launch_the_tier_cannot_prove_goes_to_the_exact_scan_whole(pn):
    """blobs whose centres scatter widely (dataset()): every row has four foreign blob mates and more, the slack exceeds
    their squared distances thousands of times, so their lifted keys are all the floor 0 and tau is (0, the fourth j); the
    true weight is positive: no row is proven, and each costs its three candidates.  The exact scan then takes the whole
    launch through the tier's list of unproven rows."""
    dim, dtype = 70, F32
    m, _ = plan_of("one_segment", dim, cu_count())
    x, d = dataset("scattered_blobs", dim, dtype)
    groups = random_groups(8)
    foreign_mates = ((d < 1) & (groups[:, None] != groups[None, :])).sum(axis=1)
    assert foreign_mates.min() >= 4 and d[~np.eye(N, dtype=bool)].min() > 0
    _, rows = long_list(8, m)
    every = brute_force(d, groups, None)
    tree = pn.BallTree.euclidean(x).set_option(PN_OPT_FOREIGN_FILTER, 1)
    got, c, f = tier_counters(tree, groups, None, rows)
    same_bits(got, (every[0][rows.astype(np.int64)], every[1][rows.astype(np.int64)]), "scattered")
    assert (c, f) == (3 * m, m)


def test_the_first_unsupported_width_is_refused_when_forced(pn):
    n_cu = cu_count()
    m, _ = plan_of("three_segments", 160, n_cu)  # (the list that takes the widest supported row through three segments)
    x, d = dataset("uniform", 161, F32)
    groups = random_groups(161)
    _, rows = long_list(161, m)
    tree = pn.BallTree.euclidean(x).set_option(PN_OPT_FOREIGN_FILTER, 1)
    every = brute_force(d, groups, None)
    got, c, f = tier_counters(tree, groups, None, rows)
    same_bits(got, (every[0][rows.astype(np.int64)], every[1][rows.astype(np.int64)]), 161)
    assert (c, f) == (0, 0)


def test_device_form_returns_the_host_entrys_bytes(pn):
    import torch
    dim, dtype = 70, F32
    m, _ = plan_of("three_segments", dim, cu_count())
    x, d = dataset("uniform", dim, dtype)
    groups = random_groups(5)
    core = spiky_core(d, 9, dtype)
    _, rows = long_list(3, m)
    tree = pn.BallTree.euclidean(x).set_option(PN_OPT_INDEX_BASE, 1000).set_option(PN_OPT_FOREIGN_FILTER, 1)
    every = brute_force(d, groups, core)
    idx, w = tree.nearest_foreign(groups, core, rows=rows)
    same_bits((idx - np.uint64(1000), w), (every[0][rows.astype(np.int64)], every[1][rows.astype(np.int64)]), "host")
    tree.stats(reset=True)
    di, dw = tree.nearest_foreign_device(torch.from_numpy(groups.astype(np.int32)).cuda(), torch.from_numpy(core).cuda(),
                                         rows=torch.from_numpy(rows.astype(np.int64)).cuda())
    assert di.cpu().numpy().tobytes() == idx.tobytes() and dw.cpu().numpy().tobytes() == w.tobytes()
    assert tree.stats()["candidates"] > 0


# ---- core values the tier sees: the reference on the keys, as the header states them (NaN above +inf, a negative core
# acts as 0, -0 counts as +0; the weight is written back as the value of its key: the canonical quiet NaN, +0)
def brute_force_on_keys(d, groups, core):
    u, quiet_nan = (np.uint32, 0x7FC00000) if d.dtype == np.float32 else (np.uint64, 0x7FF8000000000000)
    with np.errstate(invalid="ignore"):
        ck = np.where(np.isnan(core), u(quiet_nan), np.where(core <= 0, u(0), core.view(u)))
    keys = np.maximum(np.maximum(d.view(u), ck[:, None]), ck[None, :])  # (d is finite and >= +0: its bits are its key)
    foreign = groups[:, None] != groups[None, :]
    assert foreign.any(axis=1).all()
    j = np.argmin(np.where(foreign, keys, ~u(0)), axis=1)  # (the first minimum: the smallest j among equal keys)
    return j.astype(np.uint64), keys[np.arange(len(keys)), j]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_nan_inf_negative_and_minus_zero_cores(pn, dtype):
    x, d = dataset("uniform", 20, dtype)
    tree = pn.BallTree.euclidean(x)
    core = tree.query_self(5)[1][:, -1].copy()
    where = np.random.default_rng(11).permutation(N)
    core[where[0:6]] = np.nan
    core[where[6]] = -np.nan  # (a NaN of another bit pattern: written back as the canonical one)
    core[where[7:12]] = np.inf
    core[where[12:30]] = -0.0
    core[where[30:50]] *= -1
    core[where[50]] = -np.inf
    groups = random_groups(20)
    want = brute_force_on_keys(d, groups, core)
    for ename, t in engines(tree):
        t.stats(reset=True)
        same_bits(t.nearest_foreign(groups, core), want, ename)
        if ename == "filter":
            assert t.stats()["candidates"] > 0


def test_a_norm_beyond_the_guard_sends_the_call_to_the_exact_scan(pn):
    x = np.array(dataset("uniform", 20, F32)[0])
    x[123, 4] = 2e15  # its squared distance to the mean is beyond 2^100, the f32 fold (4e30) stays finite
    d = fold_distances(x)
    assert np.isfinite(d).all()
    groups = random_groups(21)
    tree = pn.BallTree.euclidean(x).set_option(PN_OPT_FOREIGN_FILTER, 1)
    got, c, f = tier_counters(tree, groups, None)
    same_bits(got, brute_force(d, groups, None), "guard")
    assert (c, f) == (0, 0)


def test_a_list_beyond_the_exact_scans_segment_target(pn):
    """more listed rows in one launch than 8 n_cu tiles of 64, on few indexed rows: the exact scan's scratch is sized by
    the launch (min(batch, listed rows)), not by the indexed rows"""
    m = 64 * 8 * cu_count() + 4 * TILE
    assert launches(m, 0) == [m]
    x, d = dataset("uniform", 48, F32)
    groups = random_groups(48)
    _, rows = long_list(4, m)
    every = brute_force(d, groups, None)
    tree = pn.BallTree.euclidean(x)
    for ename, t in engines(tree):
        same_bits(t.nearest_foreign(groups, None, rows=rows), (every[0][rows.astype(np.int64)], every[1][rows.astype(np.int64)]), ename)


# ---- the rounds of pn_mst_* through segments of three stages
def test_mst_rounds_through_multi_stage_segments(pn):
    n, dim, n_cu = 6000, 16, cu_count()
    assert fr_plan(n, padded(dim), n, n_cu) == (47, 16, 3) and -(-n // 128) == 47, "the first round: 47 stages, 3 per segment"
    print(f"plan mst dim={dim} n_cu={n_cu} m={n}: qt=47 nseg=16 seg_stages=3 {stages_by_segment(n, padded(dim), 3)}")
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((8, dim))[rng.integers(0, 8, n)] * 4 + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)
    tree = pn.BallTree.euclidean(x)
    core = tree.query_self(5)[1][:, -1].copy()
    exact = tree.set_engine("exact").mst(core)
    work = tree.last_mst_work
    tree.set_engine("auto").set_option(PN_OPT_FOREIGN_FILTER, 1)
    for batch in (0, 1000):
        tree.set_option(PN_OPT_MST_BATCH, batch).stats(reset=True)
        got = tree.mst(core)
        assert all(np.array_equal(a, b) for a, b in zip(got[:2], exact[:2])), batch
        assert np.array_equal(got[2].view(np.uint32), exact[2].view(np.uint32)), batch
        assert tree.last_mst_work == work and tree.stats()["candidates"] > 0, batch
