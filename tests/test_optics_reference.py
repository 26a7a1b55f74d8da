"""The numpy restatement of the OPTICS contract (tests/optics_reference.py: cpu_optics, cpu_extract) against
scikit-learn, and hand-made tie cases that pin the tie rules without it.

scikit-learn's OPTICS(min_samples = ms + 1, max_eps, metric="precomputed") fed with the SAME distance matrix must give
EQUAL ordering_ and predecessor_ (its min_samples counts the row itself); with metric="euclidean" its own pairwise
distances differ in the last bits and break the exact ties reach = core[p] differently, which is why the contract is
"scikit-learn's algorithm on this library's distances".  The matrix is the reference's fold in f64; max_eps is no
entry of it, so '<' and scikit-learn's '<=' select the same lists.
"""
import numpy as np
import pytest

from optics_reference import core_from_lists, cpu_extract, cpu_optics, csr_from_dense, same_partition


def fold_matrix(x):
    acc = np.zeros((len(x), len(x)), dtype=x.dtype)
    for k in range(x.shape[1]):
        diff = x[:, None, k] - x[None, :, k]
        acc = acc + diff * diff
    return np.sqrt(acc)


def blob_set(seed, n, dim, nb, sigma, background):
    rng = np.random.default_rng(seed)
    centres = rng.random((nb, dim))
    n_bg = int(round(n * background))
    which = rng.integers(0, nb, n - n_bg)
    pts = np.concatenate([centres[which] + sigma * rng.standard_normal((n - n_bg, dim)), rng.random((n_bg, dim))])
    return pts[rng.permutation(n)]


@pytest.fixture(scope="module", params=[(1500, 2, 5, 0.05), (1200, 8, 9, 0.45)], ids=["1500x2-ms5", "1200x8-ms9"])
def case(request):
    sk = pytest.importorskip("sklearn.cluster")
    n, dim, ms, eps = request.param
    d = fold_matrix(blob_set(1, n, dim, 6, 0.04, 0.15))
    assert not np.any(d == eps)
    off, idx, dist = csr_from_dense(d, eps)
    got = cpu_optics(off, idx, dist, ms)
    ref = sk.OPTICS(min_samples=ms + 1, max_eps=eps, metric="precomputed", cluster_method="dbscan", eps=eps).fit(d)
    return sk, eps, got, ref


def test_ordering_and_predecessor_equal_scikit_learn(case):
    sk, eps, (ordering, reach, pred, core), ref = case
    n = len(ordering)
    n_inf = int(np.count_nonzero(np.isinf(reach)))
    assert 1 < n_inf < n and 0 < np.count_nonzero(np.isinf(core)) < n  # (several components, some rows without a core)
    assert np.array_equal(ordering.astype(np.int64), ref.ordering_)
    assert np.array_equal(pred, ref.predecessor_)
    assert np.array_equal(np.isinf(reach), np.isinf(ref.reachability_))
    fin = np.isfinite(reach)
    assert np.max(np.abs(reach[fin] - ref.reachability_[fin])) <= 1e-14
    assert np.array_equal(np.isinf(core), np.isinf(ref.core_distances_))
    fin = np.isfinite(core)
    assert np.max(np.abs(core[fin] - ref.core_distances_[fin])) <= 1e-14


@pytest.mark.parametrize("frac", [0.5, 0.8, 1.0])
def test_extraction_equals_cluster_optics_dbscan(case, frac):
    sk, eps, (ordering, reach, pred, core), ref = case
    e = frac * eps
    assert not np.any(reach == e) and not np.any(core == e)
    labels, ncl = cpu_extract(ordering, reach, core, e)
    want = sk.cluster_optics_dbscan(reachability=reach, core_distances=core, ordering=ordering.astype(np.int64), eps=e)
    assert np.array_equal(labels, want)
    assert ncl == int(labels.max()) + 1 and ncl >= 2


# ---- tie cases by hand: no scikit-learn needed
def run(x, ms, eps):
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    return cpu_optics(*csr_from_dense(fold_matrix(x), eps), ms)


def test_eight_collinear_equidistant_points():
    inf = np.inf
    x = np.arange(8.0)
    # one other row: every core distance is the spacing, every reachability ties with it
    o, r, p, c = run(x, 1, 1.5)
    assert o.tolist() == list(range(8)) and p.tolist() == [-1, 0, 1, 2, 3, 4, 5, 6]
    assert r.tolist() == [inf] + [1.0] * 7 and c.tolist() == [1.0] * 8
    # two other rows: the ends' cores are 2; row 2 is first reached at 2 from row 0, then improved to 1 from row 1
    o, r, p, c = run(x, 2, 2.5)
    assert o.tolist() == list(range(8)) and p.tolist() == [-1, 0, 1, 2, 3, 4, 5, 6]
    assert r.tolist() == [inf, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0] and c.tolist() == [2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0]
    # the same points in another row order: the walk starts at row 0 = the point x = 4 and alternates by the row tie-break
    perm = [4, 3, 5, 2, 6, 1, 7, 0]
    o, r, p, c = run(x[perm], 1, 1.5)
    assert o.tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and p.tolist() == [-1, 0, 0, 1, 2, 3, 4, 5]
    # max_eps below the spacing: no lists, no cores, rows in index order
    o, r, p, c = run(x, 1, 1.0)
    assert o.tolist() == list(range(8)) and np.isinf(r).all() and np.isinf(c).all() and (p == -1).all()


def test_duplicate_rows_keep_their_first_predecessor():
    inf = np.inf
    # rows 0, 1, 2 are the same point, row 3 lies at distance 1
    o, r, p, c = run([0.0, 0.0, 0.0, 1.0], 2, 2.0)
    assert o.tolist() == [0, 1, 2, 3]
    assert r.tolist() == [inf, 0.0, 0.0, 1.0] and c.tolist() == [0.0, 0.0, 0.0, 1.0]
    assert p.tolist() == [-1, 0, 0, 0]  # (strict '<': an equal offer from row 1 or 2 changes nothing)


def test_two_rows_equidistant_from_a_third():
    inf = np.inf
    # rows 1 and 2 both at distance 1 from row 0 and 2 apart: the lower row goes first
    o, r, p, c = run([0.0, 1.0, -1.0], 1, 1.5)
    assert o.tolist() == [0, 1, 2] and r.tolist() == [inf, 1.0, 1.0] and p.tolist() == [-1, 0, 0]
    # an isolated row 0 is picked first all the same (lowest row among the unreached), then row 1 starts the chain
    o, r, p, c = run([5.0, -1.0, 0.0, 1.0], 1, 1.5)
    assert o.tolist() == [0, 1, 2, 3] and r.tolist() == [inf, inf, 1.0, 1.0] and p.tolist() == [-1, -1, 1, 2]
    assert c.tolist() == [inf, 1.0, 1.0, 1.0]
    # a smaller reachability beats a lower row: row 3 (0.5 from row 0) before row 1 (1 from row 0)
    o, r, p, c = run([0.0, 1.0, 9.0, -0.5], 1, 1.2)
    assert o.tolist() == [0, 3, 1, 2] and r.tolist() == [inf, 1.0, inf, 0.5] and p.tolist() == [-1, 0, -1, 0]


def test_extraction_rules_by_hand():
    inf = np.inf
    ordering = np.array([0, 1, 2, 3, 4, 5], dtype=np.uint64)
    reach = np.array([inf, 0.2, 0.3, 0.9, 0.25, inf])
    core = np.array([0.2, 0.3, inf, 0.25, 0.4, inf])
    labels, ncl = cpu_extract(ordering, reach, core, 0.5)
    assert labels.tolist() == [0, 0, 0, 1, 1, -1] and ncl == 2   # row 2: a border row; row 5: far and not near
    labels, ncl = cpu_extract(ordering, reach, core, 0.25)       # strict: 0.25 is neither < 0.25
    assert labels.tolist() == [0, 0, -1, -1, -1, -1] and ncl == 1
    assert same_partition(np.array([0, 0, 1, 2]), np.array([5, 5, 3, 0]))
    assert not same_partition(np.array([0, 0, 1, 2]), np.array([5, 4, 3, 0]))
    assert not same_partition(np.array([0, 1, 1, 2]), np.array([5, 5, 5, 0]))
    assert core_from_lists(np.array([0, 2, 2]), np.array([3.0, 1.0]), 2).tolist() == [3.0, inf]
