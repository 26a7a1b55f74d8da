"""The Python binding against the ctypes table, without a GPU: ``_lib.lib`` is replaced by a stub whose every attribute
records its call and returns ``PN_OK``; every host-side (NumPy) method of a fake ``BallTree`` (n = 10, dim = 4, f32 and
f64) and of a fake ``ShardedIndex`` (n = local_rows = 10) is driven through it.  Each recorded call must name a declared
symbol, carry as many arguments as its ``argtypes``, each one acceptable to its argtype, and hand a scalar radius / eps /
bandwidth over as the ctypes type of the handle's suffix."""
import ctypes as C

import numpy as np
import pytest

N, DIM = 10, 4


class Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
            return 0  # PN_OK
        return record


@pytest.fixture
def stub(pn, monkeypatch):
    from petal_neighbors_amd import _lib
    s = Stub()
    monkeypatch.setattr(_lib, "lib", lambda: s)
    return s


def _check(calls, sfx):
    """the four assertions on every recorded call; returns the set of symbols seen"""
    from petal_neighbors_amd import _lib
    other = "f64" if sfx == "f32" else "f32"
    for name, args in calls:
        assert name in _lib.SIGNATURES, name
        argtypes = _lib.SIGNATURES[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for i, (a, t) in enumerate(zip(args, argtypes)):
            t.from_param(a)  # raises where ctypes would refuse the argument
        if name.endswith("_" + sfx) and name[:-3] + other in _lib.SIGNATURES:
            # the slots where the twin's signature differs are the scalars of the element type
            for a, t, u in zip(args, argtypes, _lib.SIGNATURES[name[:-3] + other][1]):
                if t is not u and t in (C.c_float, C.c_double):
                    assert type(a) is _lib.REAL[sfx], (name, type(a))
        assert not name.endswith("_" + other), (name, sfx)
    return {name for name, _ in calls}


def _fake_tree(pn, sfx):
    bt = pn.BallTree
    t = bt.__new__(bt)
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    t._h, t._sfx, t.dtype, t._n, t._dim, t.device = C.c_void_p(1), sfx, dt, N, DIM, 0
    t.metric, t.points = pn.distance.Euclidean(), np.zeros((N, DIM), dtype=dt)
    return t, dt


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_every_host_method_of_ball_tree_calls_the_table(pn, stub, sfx):
    t, dt = _fake_tree(pn, sfx)
    q, p = np.zeros((3, DIM), dtype=dt), np.zeros(DIM, dtype=dt)
    rq, rn = np.full(3, 0.5, dtype=dt), np.full(N, 0.5, dtype=dt)
    # tree accessors (the stub's tree has no nodes: the node check is answered here)
    assert t.num_nodes() == 0
    t.num_nodes = lambda: 4
    t.children_of(1), t.points_of(1), t.radius_of(1), t.compare_nodes(1, 2), t.node_distance_lower_bound(1, 2)
    t._centroid_of(1)
    # k-NN and radius searches: scalar and one radius per query
    t.query(p, 3), t.query_batch(q, 3), t.query_nearest(p)
    for r, rs in ((0.5, 0.5), (np.float32(0.5), 0.5), (rq, rn)):
        t.query_radius_batch(q, r)
        for sort in (False, True):
            t.query_radius_with_distance_batch(q, r, sort)
            t.query_radius_self(rs, with_distance=True, sort=sort, include_self=sort)
        t.query_radius_self(rs)
        t.query_radius_count(q, r)
    t.query_radius(p, 0.5), t.query_radius_with_distance(p, 0.5, True)
    t.two_point_correlation(q, np.array([0.1, 0.2]))
    t.query_self(3), t.query_self(3, include_self=True)
    # clustering
    t.dbscan(0.5, 3)
    t.mst(), t.mst(rn)
    z = np.zeros(N - 1, dtype=np.uint64)
    t.linkage(), t.linkage(rn), t.linkage(edges=(z, z, np.zeros(N - 1, dtype=dt)))
    t.hdbscan(3), t.hdbscan(3, 2)
    t.lof(3), t.lof(3, full=True)
    t.lof_score(q, 3, np.ones(N), rn)
    t.optics(3), t.optics(3, 0.5)
    t.optics_dbscan(0.5, np.arange(N, dtype=np.uint64), rn, rn)
    # densities: scalar and per-query bandwidths
    for h, hs in ((0.5, 0.5), (rq, rn)):
        t.kernel_density(q, h), t.kernel_density(q, h, "tophat", 0.1, True, False)
        t.kernel_density_self(hs), t.kernel_density_self(hs, include_self=True)
        t.kernel_density_raw(q, h), t.kernel_density_raw(None, hs, include_self=True)
    # k-means, mean shift
    c = np.zeros((2, DIM), dtype=dt)
    t.kmeans_assign(c)
    t.kmeans(c), t.kmeans(c, full=True), t.kmeans(c, abs_tol=0.0)
    if sfx == "f32":
        t.kmeans_bounds(c)
    for seeds in (None, q):
        ns = N if seeds is None else 3
        t.mean_shift_modes(0.5, seeds), t.mean_shift_modes(0.5, seeds, full=True)
        t.mean_shift_modes(np.full(ns, 0.5, dtype=dt), seeds, tol=1e-3)
        t.mean_shift(0.5, seeds), t.mean_shift(0.5, seeds, cluster_all=False)
    t.mean_shift_merge(q, np.ones(3, dtype=np.uint64), 0.5)
    t.mean_shift_labels(c, 0.5), t.mean_shift_labels(c, 0.5, cluster_all=False)
    # options, lifetime
    t.set_option(2, 1), t.set_engine("exact"), t.stats(), t.stats(reset=True)
    t.close()
    seen = _check(stub.calls, sfx)
    stems = ["query", "query_nearest", "query_radius", "query_radius_with_distance", "query_radii", "query_self",
             "query_radius_self", "query_radii_self", "dbscan", "mst", "linkage", "hdbscan", "lof", "lof_score", "optics",
             "optics_dbscan", "kde", "kde_self", "kmeans_assign", "kmeans", "mean_shift", "mean_shift_merge",
             "mean_shift_labels", "tree_radius_of", "tree_node_distance_lower_bound"]
    # (pn_free is not among them: every list the stub "returns" is empty)
    want = {f"pn_{s}_{sfx}" for s in stems} | {"pn_index_set_option", "pn_index_get_stats", "pn_index_destroy"}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_every_host_method_of_sharded_index_calls_the_table(pn, stub, sfx):
    from petal_neighbors_amd.sharded import ShardedIndex
    s = ShardedIndex.__new__(ShardedIndex)
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    s._h, s._sfx, s.dtype, s.n, s.local_rows, s.device = C.c_void_p(1), sfx, dt, N, N, None
    q = np.zeros((3, DIM), dtype=dt)
    s.query(q[0], 3), s.query_batch(q, 3)
    s.query_radius_batch(q, 0.5)
    s.query_self(3), s.query_self(3, include_self=True)
    for sort in (False, True):
        s.query_radius_with_distance_batch(q, 0.5, sort)
        s.query_radius_self(0.5, with_distance=True, sort=sort, include_self=sort)
    s.query_radius_self(0.5)
    s.set_option(2, 1), s.set_engine("exact"), s.stats()
    done = len(stub.calls)
    # one radius per query: there is no pn_sharded_query_radii_*, the call fails before the library is reached
    radii = np.full(3, 0.5, dtype=dt)
    for call in (lambda: s.query_radius_batch(q, radii), lambda: s.query_radius_with_distance_batch(q, radii),
                 lambda: s.query_radius_self(np.full(N, 0.5, dtype=dt))):
        with pytest.raises(TypeError):
            call()
    assert len(stub.calls) == done
    s.close()
    seen = _check(stub.calls, sfx)
    want = {f"pn_sharded_{m}_{sfx}" for m in ("query", "query_radius", "query_radius_with_distance", "query_self",
                                              "query_radius_self")}
    assert want | {"pn_sharded_set_option", "pn_sharded_get_stats", "pn_sharded_destroy"} <= seen
