"""The host entry points of the clustering, density and prediction families stage their inputs and outputs through ONE
buffer of the workspace (HostIo, csrc/index.hip).  Here every one of them runs on one handle, in an order that makes
the shared buffer be reused, outgrown and reused smaller, and each result is compared with the same call on a FRESH
handle of the same rows.  Every family's results depend on the data alone, so the comparison is bit for bit throughout
(as in the families' own device-against-host tests).  Two passes on the same handle: every optional output requested,
then every optional output NULL (KDE must keep one of sum / count: the large call keeps the sum, the small one the count).

777 rows of 5 columns: the odd count leaves the 4-byte and 1-byte arrays of a call off an 8-byte boundary.  Calls that
continue another call's result (merge, labels, lof_score, optics_dbscan, linkage) take it from the full pass on fresh
handles, so both passes and both kinds of handle are given the same inputs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM = 777, 5
EPS, MIN_SAMPLES, H_MS, K_LOF, K_KNN, N_CLASSES = 0.09, 5, 0.2, 10, 5, 4
EPANECHNIKOV = 2
i64, u64, f64 = np.int64, np.uint64, np.float64


def blobs(dtype):
    """three tight blobs and a uniform background: clusters and noise for DBSCAN / HDBSCAN / OPTICS"""
    rng = np.random.RandomState(0x10A)
    centres = np.array([[0.2] * DIM, [0.5, 0.8, 0.5, 0.2, 0.5], [0.8] * DIM])
    member = rng.randint(0, 4, N)  # 3: background
    x = np.where((member == 3)[:, None], rng.uniform(0.0, 1.0, (N, DIM)),
                 centres[np.minimum(member, 2)] + 0.04 * rng.standard_normal((N, DIM)))
    return np.ascontiguousarray(x, dtype=dtype), member.astype(i64)


def ptr(a):
    return None if a is None else a.ctypes.data


class Run:
    """the calls of the sequence against one handle; `prev`: the full pass on fresh handles (None while it is made)"""

    def __init__(self, pn, x, member, full, prev):
        from petal_neighbors_amd import _lib
        self.pn, self.x, self.member, self.full, self.prev = pn, x, member, full, prev
        self.dt = x.dtype.type
        self.sfx = "f32" if self.dt == np.float32 else "f64"
        self.L, self.err = _lib.lib(), _lib.last_error
        rng = np.random.RandomState(0x10B)
        self.q2000 = rng.uniform(0.0, 1.0, (2000, DIM)).astype(self.dt)
        self.q33 = np.ascontiguousarray(np.concatenate([x[:5], rng.uniform(0.0, 1.0, (28, DIM)).astype(self.dt)]))
        self.radii = (0.05 + 0.25 * rng.uniform(0.0, 1.0, 33)).astype(self.dt)
        self.h7 = (0.1 + 0.1 * rng.uniform(0.0, 1.0, 7)).astype(self.dt)
        self.targets = np.ascontiguousarray(rng.standard_normal((N, 2)))

    def call(self, stem, *args):
        rc = getattr(self.L, f"pn_{stem}_{self.sfx}")(*args)
        assert rc == 0, (stem, rc, self.err())

    def opt(self, *shape_dtype):
        return np.zeros(*shape_dtype) if self.full else None

    def rows(self, q):
        return [ptr(q), q.shape[0], q.shape[1], q.shape[1]]

    # ---- the calls: each returns {name: array} of what it asked for
    def kmeans(self, h):
        init = np.ascontiguousarray(self.x[[0, 1, 2]])
        o = dict(centres=np.zeros((3, DIM), self.dt), labels=np.zeros(N, i64), dist=self.opt(N, self.dt), counts=self.opt(3, u64),
                 inertia=self.opt(1, f64), iterations=self.opt(1, u64), shift2=self.opt(1, f64))
        self.call("kmeans", h, ptr(init), 3, 1e-9, 40, 0, *[ptr(a) for a in o.values()])
        return o

    def kde(self, h, q, bw, keep):
        o = dict(sum=np.zeros(len(q), f64) if self.full or keep == "sum" else None,
                 count=np.zeros(len(q), u64) if self.full or keep == "count" else None, cutoff=self.opt(len(q), self.dt))
        self.call("kde", h, *self.rows(q), ptr(bw), len(bw), EPANECHNIKOV, 0.0, 0, *[ptr(a) for a in o.values()])
        return o

    def kde_2000(self, h):
        return self.kde(h, self.q2000, np.array([0.15], self.dt), "sum")

    def kde_7(self, h):
        return self.kde(h, self.q2000[:7].copy(), self.h7, "count")

    def dbscan(self, h):
        o = dict(labels=np.zeros(N, i64), core=self.opt(N, np.uint8), n_clusters=self.opt(1, u64))
        self.call("dbscan", h, EPS, MIN_SAMPLES, 0, *[ptr(a) for a in o.values()])
        return o

    def mean_shift(self, h):
        seeds, bw = np.ascontiguousarray(self.x[::15][:51]), np.array([H_MS], self.dt)
        o = dict(modes=np.zeros((51, DIM), self.dt), points=np.zeros(51, u64), iterations=self.opt(51, np.uint32),
                 shift=self.opt(51, f64), work=self.opt(2, u64))
        self.call("mean_shift", h, *self.rows(seeds), ptr(bw), 1, 1e-4, 30, 0, *[ptr(a) for a in o.values()])
        return o

    def ms_merge(self, h):
        ms = self.prev["mean_shift"]
        o = dict(centres=np.zeros((51, DIM), self.dt), centre_points=self.opt(51, u64), centre_of_seed=self.opt(51, i64),
                 n_centres=np.zeros(1, u64))
        self.call("mean_shift_merge", h, ptr(ms["modes"]), 51, ptr(ms["points"]), H_MS, 0, *[ptr(a) for a in o.values()])
        nc = int(o["n_centres"][0])  # (only that many centres are written)
        o["centres"] = o["centres"][:nc]
        if self.full:
            o["centre_points"] = o["centre_points"][:nc]
        return o

    def ms_labels(self, h):
        centres = np.ascontiguousarray(self.prev["ms_merge"]["centres"])
        o = dict(labels=np.zeros(N, i64))
        self.call("mean_shift_labels", h, ptr(centres), len(centres), H_MS, 0, ptr(o["labels"]))
        return o

    def lof(self, h):
        o = dict(lof=np.zeros(N, f64), lrd=self.opt(N, f64), kdist=self.opt(N, self.dt))
        self.call("lof", h, K_LOF, 0, *[ptr(a) for a in o.values()])
        return o

    def lof_score(self, h):
        fit = self.prev["lof"]
        o = dict(score=np.zeros(33, f64))
        self.call("lof_score", h, *self.rows(self.q33), K_LOF, ptr(fit["lrd"]), ptr(fit["kdist"]), 0, ptr(o["score"]))
        return o

    def optics(self, h):
        o = dict(ordering=np.zeros(N, u64), reachability=np.zeros(N, self.dt), predecessor=self.opt(N, i64),
                 core_distances=self.opt(N, self.dt))
        self.call("optics", h, MIN_SAMPLES, float("inf"), 0, *[ptr(a) for a in o.values()])
        return o

    def optics_dbscan(self, h):
        op = self.prev["optics"]
        o = dict(labels=np.zeros(N, i64), n_clusters=self.opt(1, u64))
        self.call("optics_dbscan", h, ptr(op["ordering"]), ptr(op["reachability"]), ptr(op["core_distances"]), EPS, 0,
                  *[ptr(a) for a in o.values()])
        return o

    def mst(self, h):
        core = self.prev["lof"]["kdist"] if self.full else None  # (an optional INPUT: absent in the NULL pass)
        o = dict(src=np.zeros(N - 1, u64), dst=np.zeros(N - 1, u64), weight=np.zeros(N - 1, self.dt), work=self.opt(2, u64))
        self.call("mst", h, ptr(core), 0, *[ptr(a) for a in o.values()])
        return o

    def linkage(self, h):
        e = self.prev["mst"]
        o = dict(left=np.zeros(N - 1, u64), right=np.zeros(N - 1, u64), weight=np.zeros(N - 1, self.dt), size=np.zeros(N - 1, u64))
        self.call("linkage", h, ptr(e["src"]), ptr(e["dst"]), ptr(e["weight"]), 0, *[ptr(a) for a in o.values()])
        return o

    def hdbscan(self, h):
        o = dict(labels=np.zeros(N, i64), probabilities=self.opt(N, self.dt), n_clusters=self.opt(1, u64))
        self.call("hdbscan", h, MIN_SAMPLES, 10, 0, *[ptr(a) for a in o.values()])
        return o

    def knn_classify(self, h):
        o = dict(pred=np.zeros(33, i64), proba=self.opt((33, N_CLASSES), f64))
        self.call("knn_classify", h, *self.rows(self.q33), K_KNN, ptr(self.member), N_CLASSES, 0, *[ptr(a) for a in o.values()])
        return o

    def knn_regress(self, h):
        o = dict(out=np.zeros((33, 2), f64))
        self.call("knn_regress", h, *self.rows(self.q33), K_KNN, ptr(self.targets), 2, 0, ptr(o["out"]))
        return o

    def query_radii(self, h):
        off = np.zeros(34, u64)
        idx, dist = C.c_void_p(), C.c_void_p()
        try:
            self.call("query_radii", h, *self.rows(self.q33), ptr(self.radii), 0, ptr(off), C.byref(idx),
                      C.byref(dist) if self.full else None)
            total = int(off[-1])
            assert total >= 5  # (five of the queries are rows)
            o = dict(offsets=off, idx=np.frombuffer((C.c_uint64 * total).from_address(idx.value), dtype=u64).copy())
            if self.full:
                o["dist"] = np.frombuffer((C.c_char * (total * self.x.itemsize)).from_address(dist.value), dtype=self.dt).copy()
        finally:
            for p in (idx, dist):
                if p.value:
                    self.L.pn_free(p)
        return o

    # the order makes the one buffer be reused, outgrown (kde_2000, lof, optics) and reused smaller
    SEQUENCE = ["kmeans", "kde_2000", "dbscan", "kde_7", "mean_shift", "ms_merge", "ms_labels", "lof", "lof_score", "optics",
                "optics_dbscan", "mst", "linkage", "hdbscan", "knn_classify", "knn_regress", "query_radii", "kmeans"]

    def on_fresh_handles(self):
        out = {}
        if self.prev is None:  # (the full pass feeds itself: a call continues calls before it in the sequence)
            self.prev = out
        for name in self.SEQUENCE[:-1]:
            tree = self.pn.BallTree.euclidean(self.x)
            out[name] = getattr(self, name)(tree._h)
            tree.close()
        return out

    def on_one_handle(self, tree):
        return [(name, getattr(self, name)(tree._h)) for name in self.SEQUENCE]


def same(got, want, what):
    assert list(got) == list(want), what
    for name in want:
        g, w = got[name], want[name]
        assert (g is None) == (w is None), (what, name)
        if w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def case(pn, request):
    x, member = blobs(request.param)
    full = Run(pn, x, member, True, None).on_fresh_handles()
    tree = pn.BallTree.euclidean(x)  # THE handle of this element type: both passes run on it
    yield dict(pn=pn, x=x, member=member, full=full, tree=tree)
    tree.close()


def test_the_data_has_clusters_and_noise(case):
    f = case["full"]
    for name in ("dbscan", "optics_dbscan", "hdbscan"):
        assert int(f[name]["n_clusters"][0]) >= 2 and (f[name]["labels"] == -1).any() and (f[name]["labels"] >= 0).any(), name
    assert 1 <= len(f["ms_merge"]["centres"]) < 51 and f["kde_2000"]["count"].max() > 0


@pytest.mark.parametrize("full", [True, False], ids=["every_optional_output", "optional_outputs_null"])
def test_one_handle_gives_what_fresh_handles_give(case, full):
    run = Run(case["pn"], case["x"], case["member"], full, case["full"])
    want = case["full"] if full else run.on_fresh_handles()
    for step, (name, got) in enumerate(run.on_one_handle(case["tree"])):
        same(got, want[name], f"step {step}: {name}")
