"""The bf16 first tier of pn_nearest_foreign_* / pn_mst_* on Cosine indexes, against numpy alone: for row
i the partner j of another group that minimises (key(w), j), w = max(d, core[i], core[j]) with -0 as +0, d the reference's
Cosine::distance in the index's dtype; no foreign row: idx 2^64 - 1, the value of the greatest signed key."""
import numpy as np
import pytest

from conftest import ROOT, uniform

gpu = pytest.mark.gpu
PN_OPT_INDEX_BASE, PN_OPT_FOREIGN_FILTER = 3, 17
N = 300  # no multiple of 32 or 128: a last partial A tile, and listed-row tiles with empty lanes
GROUPINGS = [np.arange(N), np.arange(N) % 2, (np.arange(N) == N - 1) * 9, np.full(N, 3)]  # singletons .. one group


def cosine_distances(x):  # sequential unfused dot, the norms' own folds and sqrt, 1 - dot / (n_i n_j)
    dot, sq = np.zeros((len(x), len(x)), dtype=x.dtype), np.zeros(len(x), dtype=x.dtype)
    for k in range(x.shape[1]):
        dot += x[:, None, k] * x[None, :, k]
        sq += x[:, k] * x[:, k]
    return x.dtype.type(1) - dot / (np.sqrt(sq)[:, None] * np.sqrt(sq)[None, :])


def brute_force(d, groups, core):
    w = d if core is None else np.maximum(np.maximum(d, core[:, None]), core[None, :])
    w, foreign = w + w.dtype.type(0), groups[:, None] != groups[None, :]
    j = np.argmin(np.where(foreign, w, np.inf), axis=1)  # (the first minimum: the smallest j among equal weights)
    u, some = np.uint32 if w.dtype == np.float32 else np.uint64, foreign.any(axis=1)
    return np.where(some, j.astype(np.uint64), ~np.uint64(0)), np.where(some, w[np.arange(N), j].view(u), ~u(0) >> u(1))


def make_data(kind, dim, dtype):
    rng = np.random.default_rng(7 + dim)
    if kind == "cone":  # six tight blobs far from the origin: nearly every gap is below the tier's slack
        centres = 1000.0 + 50.0 * rng.standard_normal((6, dim))
        return (centres[rng.integers(0, 6, N)] + 0.01 * rng.standard_normal((N, dim))).astype(dtype)
    x = (uniform((N, dim), 5, dtype) - dtype(0.5)).astype(dtype)  # spread angles
    if kind == "parallel":  # 20 positive multiples of one row over the groups: distances 0 or a few ulp below it
        x[rng.choice(N, 20, replace=False)] = (x[5][None, :] * rng.uniform(0.25, 4.0, (20, 1))).astype(dtype)
    return x


def check(got, want, rows=slice(None), base=0):
    assert np.array_equal(got[0], want[0][rows] + np.uint64(base)) and np.array_equal(got[1].view(want[1].dtype), want[1][rows])


@gpu
@pytest.mark.parametrize("kind", ["uniform", "cone", "parallel"])
@pytest.mark.parametrize("dim", [8, 20, 130])  # the minimum; padded to 32; dp = 144
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_against_brute_force(pn, dtype, dim, kind):
    x = make_data(kind, dim, dtype)
    tree, d = pn.BallTree.new(x, pn.distance.Cosine()), cosine_distances(x)
    for groups in GROUPINGS:
        for core in (None, tree.query_self(5)[1][:, -1].copy()):
            want = brute_force(d, groups, core)
            check(tree.set_option(PN_OPT_FOREIGN_FILTER, 0).set_engine("exact").nearest_foreign(groups, core), want)
            check(tree.set_engine("auto").set_option(PN_OPT_FOREIGN_FILTER, 3).nearest_foreign(groups, core), want)
            check(tree.set_option(PN_OPT_FOREIGN_FILTER, 0).nearest_foreign(groups, core), want)


@gpu
def test_the_tier_answers_and_counts(pn):
    """Every row is provable: the least gap between a row's nearest and fourth-nearest foreign row is 5.5e-3 (in f64), the
    tier's whole slack below 1e-3.  Observed: 900 candidates, 0 rows left to the exact scan."""
    from petal_neighbors_amd import _lib
    tree = pn.BallTree.new(make_data("uniform", 20, np.float32), pn.distance.Cosine()).set_option(PN_OPT_FOREIGN_FILTER, 3)
    tree.nearest_foreign(GROUPINGS[1])
    s = tree.stats()
    assert s["queries"] == N and s["candidates"] > 0 and s["evaluations"] == s["candidates"] and s["fallback_queries"] <= N // 10
    tree.set_option(PN_OPT_FOREIGN_FILTER, 1).nearest_foreign(GROUPINGS[1])  # 1 names the Euclidean tier alone
    assert tree.stats()["candidates"] == s["candidates"]
    assert _lib.lib().pn_index_set_option(tree._h, PN_OPT_FOREIGN_FILTER, 4) == _lib.PN_ERR_INVALID


@gpu
def test_a_zero_row_sends_the_call_to_the_exact_scan(pn):
    x = make_data("uniform", 20, np.float32)
    x[7] = 0
    tree = pn.BallTree.new(x, pn.distance.Cosine()).set_option(PN_OPT_FOREIGN_FILTER, 3)
    got = tree.nearest_foreign(GROUPINGS[1])
    assert tree.stats()["candidates"] == 0
    want = tree.set_option(PN_OPT_FOREIGN_FILTER, 2).nearest_foreign(GROUPINGS[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


@gpu
def test_mst_rounds_through_the_tier(pn):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((8, 16))[rng.integers(0, 8, 2000)] * 4 + 0.3 * rng.standard_normal((2000, 16)) - 0.5).astype(np.float32)
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    core = tree.query_self(5)[1][:, -1].copy()
    exact, work = tree.set_engine("exact").mst(core), tree.last_mst_work
    tree.set_engine("auto").set_option(PN_OPT_FOREIGN_FILTER, 3).stats(reset=True)
    got = tree.mst(core)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, exact))
    assert tree.last_mst_work == work and tree.stats()["candidates"] > 0


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_index_base_and_device_form(pn, dtype):
    import torch
    x, groups = make_data("uniform", 20, dtype), np.arange(N) % 7
    tree = pn.BallTree.new(x, pn.distance.Cosine()).set_option(PN_OPT_INDEX_BASE, 1000).set_option(PN_OPT_FOREIGN_FILTER, 3)
    core = tree.query_self(5)[1][:, -1].copy()
    want = brute_force(cosine_distances(x), groups, core)
    rows = np.concatenate([[299, 0, 17, 17, 128, 64, 31], np.arange(0, N, 3)]).astype(np.uint64)  # (>= 64 rows: the tier)
    tree.stats(reset=True)
    idx, w = tree.nearest_foreign(groups, core, rows=rows)
    assert tree.stats()["candidates"] > 0
    check((idx, w), want, rows.astype(int), 1000)
    check(tree.nearest_foreign(groups, core, rows=rows[:7]), want, rows[:7].astype(int), 1000)  # a short list: the exact scan
    di, dw = tree.nearest_foreign_device(torch.from_numpy(groups.astype(np.int32)).cuda(), torch.from_numpy(core).cuda(),
                                         rows=torch.from_numpy(rows.astype(np.int64)).cuda())
    assert np.array_equal(di.cpu().numpy().view(np.uint64), idx) and np.array_equal(dw.cpu().numpy(), w)
    assert [len(a) for a in tree.nearest_foreign(groups, core, rows=np.flatnonzero(groups > 99))] == [0, 0]  # an empty list


def test_option_value_3_without_a_gpu():
    from petal_neighbors_amd import _lib
    assert _lib.lib().pn_index_set_option(None, PN_OPT_FOREIGN_FILTER, 3) == _lib.PN_ERR_INVALID and "index is NULL" in _lib.last_error()
    header = open(ROOT + "/include/petal_mi355x.h").read()
    assert "3 = the first tier of the handle's metric" in header[header.index("PN_OPT_FOREIGN_FILTER = 17"):][:900]
