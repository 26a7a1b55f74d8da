"""tests/density_reference.py -- the KDE sums and the mean shift step over CSR lists from anywhere, vectorised -- against
the per-query loops they stand in for, on the CPU, bit for bit: ``kde_sums`` against ``ref_terms`` / ``ref_sums`` of
tests/test_gpu_kde.py, ``ms_step`` against ``fold64`` and the loop body of ``ref_step`` of tests/test_gpu_mean_shift.py
(imported, not restated).  Then the want sides of tests/test_gpu_density_chunks.py, every condition asserted.
"""
import numpy as np
import pytest

from density_reference import kde_sums, kde_terms, ms_step, with_self
from test_gpu_kde import COMPACT, SMOOTH, ref_sums, ref_terms
from test_gpu_mean_shift import fold64

LENGTHS = [0, 1, 63, 64, 65, 129, 300, 0, 7, 200, 64, 1, 511, 128, 0]
DT = [np.float32, np.float64]


def random_lists(seed, dtype, n_rows, lengths=LENGTHS):
    """CSR lists of the given lengths over rows 0 .. n_rows - 1, ascending row index, distances in [0, 1) with zeros and a
    value a few ulp below 0 among them (a Cosine distance's)"""
    rng = np.random.default_rng(seed)
    cnt = np.array(lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)])
    idx = np.concatenate([np.sort(rng.choice(n_rows, m, replace=False)) for m in cnt]).astype(np.int64)
    dist = rng.random(int(off[-1])).astype(dtype)
    dist[rng.integers(0, len(dist), 20)] = 0
    dist[rng.integers(0, len(dist), 5)] = -np.finfo(dtype).eps
    return off, idx, dist


def loop_step(x, seeds, off, idx):
    """the loop body of test_gpu_mean_shift.ref_step over given lists"""
    out = seeds.copy()
    shift = np.full(len(seeds), np.nan)
    for q in range(len(seeds)):
        lst = idx[off[q]:off[q + 1]]
        if len(lst) == 0:
            continue
        s = fold64(x[lst].astype(np.float64))
        out[q] = (s / float(len(lst))).astype(x.dtype)
        dd = out[q].astype(np.float64) - seeds[q].astype(np.float64)
        shift[q] = np.sqrt(fold64(dd * dd))
    return out, np.diff(off).astype(np.uint64), shift


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel", COMPACT + SMOOTH)
def test_kde_sums_equal_ref_sums(dtype, kernel):
    off, idx, dist = random_lists(1, dtype, 600)
    rng = np.random.default_rng(2)
    h = rng.uniform(0.5, 2.0, len(LENGTHS)).astype(dtype)
    hr = np.repeat(h.astype(np.float64), np.diff(off))
    assert kde_terms(kernel, dist, hr).tobytes() == ref_terms(kernel, dist, hr).tobytes()
    got, got_cnt = kde_sums(off, dist, h, kernel)
    want, want_cnt = ref_sums(off.astype(np.uint64), dist, h, kernel)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes() and np.array_equal(got_cnt, want_cnt)
    assert got_cnt.tolist() == LENGTHS and (got[np.array(LENGTHS) == 0] == 0).all()
    # a list alone is summed as it is among the others (the grouping by length changes nothing)
    for q in (3, 5, 12):
        one, _ = kde_sums(np.array([0, LENGTHS[q]]), dist[off[q]:off[q + 1]], h[q:q + 1], kernel)
        assert one.tobytes() == got[q:q + 1].tobytes()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel", ["epanechnikov", "gaussian", "tophat"])
def test_kde_sums_leave_an_entry_out_by_position(dtype, kernel):
    off, idx, dist = random_lists(3, dtype, 600)
    cnt = np.diff(off)
    h = np.random.default_rng(4).uniform(0.5, 2.0, len(cnt)).astype(dtype)
    for where in ("first", "middle", "last", "none"):
        skip = {"first": np.zeros_like(cnt), "middle": cnt // 2, "last": cnt - 1, "none": np.full_like(cnt, -1)}[where]
        skip = np.where(cnt > 0, skip, -1)
        keep = np.ones(len(dist), dtype=bool)
        keep[(off[:-1] + skip)[skip >= 0]] = False
        k_off = np.concatenate([[0], np.cumsum(cnt - (skip >= 0))])
        got, got_cnt = kde_sums(off, dist, h, kernel, skip)
        want, want_cnt = ref_sums(k_off.astype(np.uint64), dist[keep], h, kernel)
        assert got.tobytes() == want.tobytes() and np.array_equal(got_cnt, want_cnt), where
        if where != "none":
            assert np.array_equal(got_cnt, (cnt - (cnt > 0)).astype(np.uint64))
            assert got_cnt.tolist().count(63) >= 1 and got_cnt.tolist().count(64) >= 1  # (a list falls below a multiple of 64)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dim", [1, 2, 8, 63, 64, 65, 200])
def test_ms_step_equals_the_loop(dtype, dim):
    rng = np.random.default_rng(dim)
    x = rng.random((600, dim)).astype(dtype)
    off, idx, _ = random_lists(5 + dim, dtype, 600)
    seeds = rng.random((len(LENGTHS), dim)).astype(dtype)
    got = ms_step(x, seeds, off, idx)
    want = loop_step(x, seeds, off, idx)
    for g, w, name in zip(got, want, ("positions", "points_within", "shift")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    dead = np.array(LENGTHS) == 0
    assert np.isnan(got[2][dead]).all() and np.array_equal(got[0][dead], seeds[dead]) and np.isfinite(got[2][~dead]).all()


def test_with_self_puts_every_live_row_into_its_own_list():
    rng = np.random.default_rng(6)
    n = 400
    m = rng.random((n, n)) < 0.1
    np.fill_diagonal(m, False)
    m[7, :7] = False      # the own entry first,
    m[9, 10:] = False     # last,
    m[11] = False         # and alone
    rows, cols = np.nonzero(m)
    off = np.concatenate([[0], np.cumsum(m.sum(axis=1))])
    dist = (1.0 + rng.random(len(cols))).astype(np.float32)
    live = rng.random(n) < 0.9
    live[[7, 9, 11]] = True
    s_off, s_idx, s_dist, s_pos = with_self(off, cols, dist, live)
    m2 = m.copy()
    m2[np.arange(n), np.arange(n)] = live
    r2, c2 = np.nonzero(m2)
    assert np.array_equal(s_off, np.concatenate([[0], np.cumsum(m2.sum(axis=1))])) and np.array_equal(s_idx, c2)
    assert np.array_equal(s_dist[r2 != c2], dist) and (s_dist[r2 == c2] == 0).all()
    assert (s_pos[~live] == -1).all() and np.array_equal(s_idx[(s_off[:-1] + s_pos)[live]], np.flatnonzero(live))
    assert s_pos[7] == 0 and s_pos[9] == s_off[10] - s_off[9] - 1 and s_off[12] - s_off[11] == 1


# ---- the want sides of tests/test_gpu_density_chunks.py run here with every condition they assert
def test_the_want_side_of_the_chunk_tests(oracle_mod):
    from test_gpu_density_chunks import want_side
    w = want_side(oracle_mod)
    assert set(w["big"]["kde"]) == {(k, i) for k in COMPACT for i in (False, True)} and w["big"]["n"] > w["control"]["n"]


def test_the_f64_want_side_of_the_chunk_tests(oracle_mod):
    from test_gpu_density_chunks import want_side
    w = want_side(oracle_mod, np.float64)
    s, cnt = w["big"]["kde"]["epanechnikov", False]
    assert s.dtype == np.float64 and (s >= 0).all() and 25 < cnt.mean() < 40


def test_the_bandwidths_of_the_external_queries():
    from test_gpu_density_chunks import CHUNK, SAMPLE, ext_bandwidths
    h = ext_bandwidths()
    bad = ~(h > 0)
    assert bad[:CHUNK].sum() > 5 and bad[CHUNK:].sum() > 5 and bad[SAMPLE].sum() >= 3
    assert bad[SAMPLE][:50].any() and bad[SAMPLE][50:150].any()
