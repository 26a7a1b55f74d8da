"""The m nearest centres of every row on an MI355X (petal-neighbors_amd/csrc/kmeans_nearest.hip) against the folds of
tests/kmeans_reference.py, ordered per row by np.lexsort((centre, key)): labels equal, distances bit for bit, under the
three engines and with the filter forced; column 0 is kmeans_assign; twins are refused and answered right; on separated
groups the filter lists nothing; the device entry equals the host entry."""
import functools

import numpy as np
import pytest

import kmeans_reference as ref
from conftest import uniform
from test_gpu_bf16 import CASES as FAMILIES  # the data families of the k-NN filter's tests

pytestmark = pytest.mark.gpu

MODES = ["exact", "auto", "bf16", "forced"]  # the three engines, and PN_ENGINE_AUTO with PN_OPT_KMEANS_FILTER = 1


def _set_mode(tree, mode):
    """False where the handle refuses PN_ENGINE_BF16 (its k-NN tier cannot serve the index): `forced` covers the filter"""
    from petal_neighbors_amd import _lib
    from petal_neighbors_amd.errors import PetalError
    tree.set_option(_lib.PN_OPT_KMEANS_FILTER, 1 if mode == "forced" else 0)
    try:
        tree.set_engine("auto" if mode == "forced" else mode)
    except PetalError:
        assert mode == "bf16" and not tree.bf16_eligible
        return False
    return True


def _as(x, dtype):
    x = x.astype(dtype)
    if dtype == np.float64:  # low bits an f32 cannot hold, so that the f64 fold is really exercised
        x = x * (1.0 + 2.0 ** -30)
    return np.ascontiguousarray(x)


def _same_bits(a, b):
    """equal bit for bit, a NaN standing for any NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(na, nb) and \
        np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


def _want(X, C, m, dist=None):
    """labels [n][m] and distances by np.lexsort((centre, key)) of the reference's folds; beyond nc: -1 and NaN"""
    n, nc = X.shape[0], C.shape[0]
    lab, d = np.full((n, m), -1, dtype=np.int64), np.full((n, m), np.nan, dtype=X.dtype)
    if nc:
        dist = ref.fold_matrix(X, C) if dist is None else dist[:n, :nc]
        keys, take = ref._keys(dist), min(m, nc)
        order = np.stack([np.lexsort((np.arange(nc), keys[i])) for i in range(n)])[:, :take]
        lab[:, :take], d[:, :take] = order, dist[np.arange(n)[:, None], order]
    return lab, d


def _check(pn, X, C, m, want, modes=MODES):
    """every mode's answer equals `want`; returns the rows the filter listed (bf16 and forced agree), None if it never ran"""
    tree = pn.BallTree.euclidean(X)
    eligible, listed = 8 <= X.shape[1] <= 320 and C.shape[0] > m, None
    for mode in modes:
        if not _set_mode(tree, mode):
            continue
        before = tree.stats()
        labels, dist = tree.kmeans_nearest(C, m)
        after = tree.stats()
        assert np.array_equal(labels, want[0]), f"{mode}: labels differ at rows {np.flatnonzero((labels != want[0]).any(1))[:8]}"
        assert _same_bits(dist, want[1]), f"{mode}: distances differ"
        assert after["queries"] - before["queries"] == X.shape[0]
        added = after["fallback_queries"] - before["fallback_queries"]
        if eligible and mode in ("bf16", "forced"):
            assert listed is None or listed == added, "the listed rows do not depend on how the filter was chosen"
            listed = added
        else:  # (PN_ENGINE_AUTO leaves shapes this small to the exact kernel; nc <= m is always its)
            assert added == 0, mode
    return listed


@functools.lru_cache(maxsize=2)
def _corpus(dim, dtype):
    X, C = _as(uniform((129, dim), 100 + dim), dtype), _as(uniform((65, dim), 200 + dim), dtype)
    return X, C, ref.fold_matrix(X, C)


# (n, nc): m > nc, m = nc, nc = m + 1 for the m below; the 32-centre tile; the 64- and 128-row tiles
SHAPES = [(1, 1), (63, 31), (64, 32), (65, 33), (129, 65), (128, 9), (64, 3)]


# dim 200: the one filter launch (four waves, one centre buffer) the other widths do not take
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [1, 2, 3, 8])
@pytest.mark.parametrize("dim", [7, 8, 17, 128, 200, 257, 320, 321])
def test_nearest_bit_for_bit_at_the_tile_edges(pn, dim, m, dtype):
    X, C, dist = _corpus(dim, dtype)
    for n, nc in SHAPES:
        _check(pn, X[:n].copy(), C[:nc].copy(), m, _want(X[:n], C[:nc], m, dist))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_column_0_is_kmeans_assign_on_the_data_families(pn, name, dtype):
    for dim in (33, 128):
        X, C = _as(FAMILIES[name](257, dim, 31), dtype), _as(FAMILIES[name](65, dim, 32), dtype)
        want = _want(X, C, 3)
        _check(pn, X, C, 3, want)
        tree = pn.BallTree.euclidean(X)
        _set_mode(tree, "forced")
        labels, dist = tree.kmeans_nearest(C, 3)
        al, ad, _ = tree.kmeans_assign(C)
        assert np.array_equal(labels[:, 0], al) and _same_bits(dist[:, 0], ad)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_twins_are_refused_and_ordered_by_number(pn, m):
    X, half = uniform((300, 64), 41), uniform((20, 64), 42)
    C = np.concatenate([half, half])  # every centre twice: centre c and its twin c + 20
    listed = _check(pn, X, C, m, _want(X, C, m), modes=["forced"])
    if m != 2:  # the m-th and the (m + 1)-th are twins: no row can be proven
        assert listed == X.shape[0]
    labels, _ = pn.BallTree.euclidean(X).kmeans_nearest(C, 2)
    assert np.array_equal(labels[:, 1], labels[:, 0] + 20)


def test_the_filter_filters_on_separated_groups(pn):
    rng = np.random.default_rng(7)
    groups = (10.0 * rng.random((75, 128))).astype(np.float32)
    C = np.repeat(groups, 4, axis=0)
    C[np.arange(300), np.tile(np.arange(4), 75)] += np.float32(0.2)  # member a of a group: + 0.2 along axis a
    own = rng.integers(0, 75, 8192)
    X = (groups[own] + rng.normal(0.0, 0.01, (8192, 128))).astype(np.float32)
    x64, c64 = X.astype(np.float64), C.astype(np.float64)
    d2 = (x64 ** 2).sum(1)[:, None] + (c64 ** 2).sum(1)[None, :] - 2.0 * x64 @ c64.T
    part = np.partition(d2, (3, 4), axis=1)
    slack = 8.0 * np.sqrt((x64 ** 2).sum(1).max()) * np.sqrt((c64 ** 2).sum(1).max()) * 2.0 ** -8
    # the condition: a generous bf16 slack separates every row's fourth nearest centre from its fifth
    assert (part[:, 4] - part[:, 3]).min() > slack, ((part[:, 4] - part[:, 3]).min(), slack)
    tree = pn.BallTree.euclidean(X)
    tree.set_engine("exact")
    el, ed = tree.kmeans_nearest(C, 4)
    assert np.array_equal(np.sort(el, axis=1), 4 * own[:, None] + np.arange(4))
    tree.set_engine("bf16")
    before = tree.stats()["fallback_queries"]
    labels, dist = tree.kmeans_nearest(C, 4)
    listed = tree.stats()["fallback_queries"] - before
    assert np.array_equal(labels, el) and dist.tobytes() == ed.tobytes()
    assert listed == 0, f"a sound bound of the stated form lists no row here, the filter listed {listed}"
    wl, wd = _want(X[:256], C, 4)  # (the reference's fold on a part: the whole is the exact engine's, checked above)
    assert np.array_equal(labels[:256], wl) and dist[:256].tobytes() == wd.tobytes()


def test_device_entry_equals_the_host_entry(pn):
    import torch
    X, C = uniform((1000, 40), 5), uniform((70, 40), 6)
    tree = pn.BallTree.euclidean(X)
    _set_mode(tree, "forced")
    hl, hd = tree.kmeans_nearest(C, 5)
    assert np.array_equal(hl, _want(X, C, 5)[0])
    dc = torch.from_numpy(C).cuda()
    dl, dd = tree.kmeans_nearest_device(dc, 5)  # outputs allocated
    side = torch.cuda.Stream()
    ol, od = torch.empty((1000, 5), dtype=torch.int64, device="cuda"), torch.empty((1000, 5), device="cuda")
    torch.cuda.synchronize()
    sl, sd = tree.kmeans_nearest_device(dc, 5, out_labels=ol, out_dist=od, stream=side.cuda_stream)
    side.synchronize()
    assert sl is ol and sd is od
    for labels, dist in ((dl, dd), (sl, sd)):
        assert np.array_equal(labels.cpu().numpy(), hl) and dist.cpu().numpy().tobytes() == hd.tobytes()
