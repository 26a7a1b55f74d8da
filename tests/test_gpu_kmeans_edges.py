"""k-means on an MI355X where petal-neighbors_amd/csrc/kmeans.hip changes shape and tests/test_gpu_kmeans.py does not go.
The contract and the helpers are that module's: labels equal, distances and inertia equal by their bits, the query
counter advanced by n per assignment.  The want side is tests/kmeans_reference.py (assign_matrix for the many-centre
shapes, pinned to assign in tests/test_kmeans_reference.py; kmeans for the loop).

  * 2 to 6 centres: the exact kernel's unroll of four with its re-read last centre, the filter's one tile with 30 to 26
    padding centres;
  * near-twin centres at chosen places of the filter's accumulator: the runner-up in the same lane, in the lane 32 away,
    in an earlier or a later centre tile, before or after the nearest -- a lost runner-up proves a row with the wrong twin;
  * 4095 / 4096 / 4097 centres, and one handle regrown and reused across centre counts;
  * the whole loop at 4097 centres (two scan chunks, a run of 3996 empty clusters, a cluster of two segments in the last
    centre) and with more centres than rows;
  * the loop at other widths (the column passes of the segment sums, the 64-column stride of the move) and around the
    sort length's step at 1024 rows;
  * the line from which PN_ENGINE_AUTO takes the filter, one row below it and on it.
"""
import numpy as np
import pytest

import kmeans_reference as ref
from conftest import uniform
from test_gpu_kmeans import MODES, _as, _check_assign, _same, _same_bits, _set_mode

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- a. centre counts 2 to 6
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dim", [8, 320])
def test_two_to_six_centres(pn, dim, dtype):
    X = _as(uniform((65, dim), 300 + dim), dtype)
    C = _as(uniform((6, dim), 400 + dim), dtype)
    for n in (1, 65):
        for nc in (2, 3, 4, 5, 6):
            Cn = C[:nc].copy()
            Cn[nc - 1] = X[0] + dtype(2.0 ** -6)  # the last centre, the one the unroll of four reads again, has a member
            want = ref.assign_matrix(X[:n], Cn)
            assert want[0][0] == nc - 1 and (n == 1 or len(set(want[0].tolist())) == nc)
            _check_assign(pn, X[:n].copy(), Cn, want)


# ------------------------------------------------------------------------------ b. near-twin centres at chosen places
TWIN_SITES, TWIN_ROWS_PER_SITE = 48, 40
TWIN_PERM_SEEDS = (11, 12, 13)  # three fixed permutations of the 96 centre numbers


def _twin_problem(dim, dtype, t):
    """48 sites uniform in [0, 8)^dim; twin 0 of a site is the site, twin 1 the site moved by 2^-t |site| along a random
    unit vector; rows site[own] + 0.05 normal, 40 per site.  Unpermuted: the twins of site s are centres 2 s and 2 s + 1."""
    rng = np.random.default_rng(3)
    sites = 8.0 * rng.random((TWIN_SITES, dim))
    u = rng.standard_normal((TWIN_SITES, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    second = sites + 2.0 ** -t * np.linalg.norm(sites, axis=1, keepdims=True) * u
    own = np.tile(np.arange(TWIN_SITES), TWIN_ROWS_PER_SITE)
    rows = sites[own] + 0.05 * rng.standard_normal((len(own), dim))
    C = np.empty((2 * TWIN_SITES, dim))
    C[0::2], C[1::2] = sites, second
    return np.ascontiguousarray(rows.astype(dtype)), np.ascontiguousarray(C.astype(dtype)), own


def _twin_class(a, b):
    """where the twins a, b lie in the filter's accumulator: centre tiles of 32, and within a tile the centres
    8 g + 4 h + j of the lane half h"""
    if a >> 5 != b >> 5:
        return "tiles"
    return "same half" if (a >> 2) & 1 == (b >> 2) & 1 else "other half"


TWIN_CASES = [(np.float32, t) for t in (6, 10, 14, 18, 22)] + [(np.float64, t) for t in (6, 14, 22, 30, 40, 50)]


@pytest.mark.parametrize("dtype,t", TWIN_CASES, ids=[f"{np.dtype(d).name}-t{t}" for d, t in TWIN_CASES])
@pytest.mark.parametrize("dim", [16, 272])  # (272: the two-wave workgroup of 64 rows, dp > 256)
def test_near_twin_centres_at_chosen_places(pn, dim, dtype, t):
    X, C0, own = _twin_problem(dim, dtype, t)
    n, nc = X.shape[0], C0.shape[0]
    assert (n, nc) == (1920, 96)
    D0 = ref.fold_matrix(X, C0)  # (a permutation of the centres permutes its columns)
    srt = np.sort(D0.astype(np.float64), axis=1)
    lab0 = np.argmin(ref._keys(D0), axis=1)
    assert np.array_equal(lab0 >> 1, own), "every row's nearest centre is one of its site's two"
    assert np.array_equal(np.argsort(D0, axis=1, kind="stable")[:, 1] >> 1, own), "... and so is the second nearest"
    ratio = float((srt[:, 2] / srt[:, 1]).min())
    assert ratio >= 5.0, f"the third nearest centre is only {ratio:.2f} times as far as the second"
    ties = int(np.count_nonzero(srt[:, 0] == srt[:, 1]))
    seen = set()  # (class, is the nearer twin the lower-numbered one)
    trials = []
    for seed in TWIN_PERM_SEEDS:
        perm = np.random.default_rng(seed).permutation(nc)  # centre 2 s + j of the recipe gets the number perm[2 s + j]
        C = np.empty_like(C0)
        C[perm] = C0
        D = np.empty_like(D0)
        D[:, perm] = D0
        labels = np.argmin(ref._keys(D), axis=1).astype(np.int64)  # (exact ties: the lower centre NUMBER, under this perm)
        want = (labels, D[np.arange(n), labels])
        a, b = perm[2 * own], perm[2 * own + 1]
        assert np.all((labels == a) | (labels == b))
        for i in range(n):
            seen.add((_twin_class(int(a[i]), int(b[i])), bool(labels[i] == min(a[i], b[i]))))
        trials.append((C, want))
    missing = {(c, low) for c in ("same half", "other half", "tiles") for low in (True, False)} - seen
    assert not missing, f"the three permutations miss {sorted(missing)}"
    first = float(np.mean(lab0 == 2 * own))
    listed = [_check_assign(pn, X, C, want) for C, want in trials]
    print(f"near twins D={dim} {np.dtype(dtype).name} t={t}: listed {listed} of {n} rows, third/second >= {ratio:.1f}, "
          f"the first twin nearer on {100 * first:.1f} %, {ties} exact ties")
    if t == max(tt for d, tt in TWIN_CASES if d == dtype):
        assert min(listed) >= 1, "twins closer than the filter resolves must be refused"


# ---------------------------------------------------------------------------------------- c. many centres, assignment
def _many_centres(dtype):
    X = _as(uniform((300, 16), 61), dtype)
    C = _as(uniform((4097, 16), 62), dtype)
    C[4096] = C[7]  # a twin across the whole range: the lower number must win
    X[5] = C[7] + dtype(2.0 ** -8)  # rows that have it as their nearest centre
    X[6] = C[7]
    X[299] = C[4095] - dtype(2.0 ** -9)  # ... and the last centre of the first 4096
    return X, C


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_assignment_to_4095_4096_4097_centres(pn, dtype):
    X, C = _many_centres(dtype)
    full = ref.fold_matrix(X, C)
    keys = ref._keys(full)
    for nc in (4095, 4096, 4097):
        labels = np.argmin(keys[:, :nc], axis=1).astype(np.int64)
        assert labels[5] == 7 and labels[6] == 7 and full[6, 7] == 0
        assert (nc == 4095 or labels[299] == 4095) and labels.max() < 4096
        listed = _check_assign(pn, X, C[:nc].copy(), (labels, full[np.arange(300), labels]))
        if nc == 4097:
            assert listed >= 2, "rows 5 and 6 have two nearest centres the filter cannot tell apart"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_handle_across_centre_counts(pn, dtype):
    """nc = 2, 4097, 33, 4097 on one handle, host and device entries in turn: the centre image and the transfer buffer
    grow, are reused smaller, and the repeat must give the bytes of the first call"""
    import torch
    X, C = _many_centres(dtype)
    want = {nc: ref.assign_matrix(X, C[:nc]) for nc in (2, 33, 4097)}
    tree = pn.BallTree.euclidean(X)
    for mode in MODES:
        assert _set_mode(tree, mode)
        got = []
        for step, nc in enumerate((2, 4097, 33, 4097)):
            wl, wd = want[nc]
            before = tree.stats()["queries"]
            if (step + MODES.index(mode)) % 2:
                dl, dd, di = tree.kmeans_assign_device(torch.from_numpy(C[:nc].copy()).cuda())
                torch.cuda.synchronize()
                labels, dist, inertia = dl.cpu().numpy(), dd.cpu().numpy(), float(di.cpu().numpy()[0])
            else:
                labels, dist, inertia = tree.kmeans_assign(C[:nc].copy())
            what = f"{mode}, call {step} with {nc} centres"
            assert tree.stats()["queries"] - before == 300, what
            assert np.array_equal(labels, wl), what
            assert _same_bits(dist, wd), what
            assert _same_bits(np.float64(inertia), np.float64(ref.inertia(wl, wd))), what
            got.append(labels.tobytes() + dist.tobytes() + np.float64(inertia).tobytes())
        assert got[3] == got[1], f"{mode}: the second call with 4097 centres differs from the first"
    tree.close()


# ------------------------------------------------------------------------------------------------ d, e. the whole loop
def _check_loop(pn, X, init, max_iter, want):
    """every mode's k-means equal to the reference in every output, then the device entry"""
    import torch
    tree = pn.BallTree.euclidean(X)
    for mode in MODES:
        if not _set_mode(tree, mode):
            continue
        before = tree.stats()["queries"]
        _same(tree.kmeans(init, abs_tol=0.0, max_iter=max_iter, full=True), want)
        assert tree.stats()["queries"] - before == (want[5] + 1) * X.shape[0], mode
    _set_mode(tree, "forced")
    c, l, d, n_, i, it, s2 = tree.kmeans_device(torch.from_numpy(init).cuda(), 0.0, max_iter)
    torch.cuda.synchronize()
    _same((c.cpu().numpy(), l.cpu().numpy(), i.cpu().numpy()[0], d.cpu().numpy(), n_.cpu().numpy().astype(np.uint64),
           int(it.cpu().numpy()[0]), s2.cpu().numpy()[0]), want)
    tree.close()


def test_whole_kmeans_with_4097_centres(pn):
    rng = np.random.default_rng(4097)
    dim, nc = 8, 4097
    spread = rng.random((4000, dim))
    blob_at = np.full(dim, 3.0)
    blob = blob_at + 0.01 * rng.standard_normal((5000, dim))
    X = np.concatenate([blob, spread])[rng.permutation(9000)].astype(np.float32)
    init = np.empty((nc, dim), dtype=np.float32)
    init[:100] = spread[:100].astype(np.float32)  # (rows of the corpus)
    init[100:4096] = (-500.0 - np.arange(100, 4096, dtype=np.float64))[:, None]  # empty, distinct, and they stay put
    init[4096] = blob_at  # the last centre, the first of the second scan chunk
    X, init = np.ascontiguousarray(X), np.ascontiguousarray(init)
    want = ref.kmeans(X, init, 0.0, 2)
    counts = want[3]
    assert counts[4096] > 4096, "the last cluster spans two segments"
    assert counts[100:4096].sum() == 0 and np.array_equal(want[0][100:4096], init[100:4096])
    assert np.count_nonzero(counts[:100]) >= 2
    assert want[5] == 2 and want[6] > 0.0
    _check_loop(pn, X, init, 2, want)


def test_whole_kmeans_with_more_centres_than_rows(pn):
    X = uniform((2, 8), 71)
    init = uniform((5, 8), 72)
    want = ref.kmeans(X, init, 0.0, 2)
    assert want[3].sum() == 2 and np.count_nonzero(want[3]) <= 2
    _check_loop(pn, X, init, 2, want)


def _width_problem(n, dim, dtype):
    """_segment_problem of tests/test_gpu_kmeans.py cut down: four clusters of unequal sizes on n rows, and a fifth centre
    no row is near; the initial centres are off their clusters, so the centres move in every column"""
    rng = np.random.default_rng(100 + dim)
    sizes = [n // 5, n // 4, n // 3]
    sizes.append(n - sum(sizes))
    centres = np.zeros((5, dim))
    for c in range(5):
        centres[c, c % dim] = 10.0 * (c + 1)
    centres[4] = -500.0
    own = np.repeat(np.arange(4), sizes)
    rng.shuffle(own)
    X = centres[own] + rng.normal(0.0, 0.5, (n, dim))
    init = centres + rng.normal(0.0, 0.3, centres.shape)
    init[4] = -500.0
    return _as(X.astype(np.float32), dtype), _as(init.astype(np.float32), dtype), sizes


@pytest.mark.parametrize("dim,dtype", [(9, np.float32), (65, np.float32), (136, np.float32), (200, np.float32),
                                       (321, np.float32), (136, np.float64)])
def test_whole_kmeans_at_other_widths(pn, dim, dtype):
    X, init, sizes = _width_problem(3000, dim, dtype)
    want = ref.kmeans(X, init, 0.0, 3)
    assert want[3].tolist() == sizes + [0] and np.array_equal(want[0][4], init[4])
    assert want[5] >= 2, "the first update moves the centres"
    assert np.all(want[0][:4] != init[:4]), "every column of every live centre moved"
    _check_loop(pn, X, init, 3, want)


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025])
def test_whole_kmeans_around_the_sort_length(pn, n):
    X = uniform((n, 8), 80 + n)
    init = uniform((3, 8), 81)
    want = ref.kmeans(X, init, 0.0, 3)
    assert want[3].sum() == n
    _check_loop(pn, X, init, 3, want)


# ------------------------------------------------------------------------------------------------- f. the auto line
# PN_ENGINE_AUTO takes the filter from 64 centres, 64 columns and n nc D >= 8e9 on (16e9 below 128 columns): DESIGN.md
# 4.22.  Twin centres (C, then C again) make the filter list every row and the exact path none, so the increase of
# fallback_queries over a call says which path it took.
AUTO_WORK, AUTO_WORK_NARROW = 8e9, 16e9


def _auto_line_case(pn, X, CC, distinct, filtered):
    """CC: ``distinct`` centres, each of which occurs a second time further on (and perhaps a centre far from every row)"""
    from petal_neighbors_amd import _lib
    n = X.shape[0]
    tree = pn.BallTree.euclidean(X)
    tree.set_engine("auto")
    tree.set_option(_lib.PN_OPT_KMEANS_FILTER, 0)
    before = tree.stats()
    labels, dist, inertia = tree.kmeans_assign(CC)
    after = tree.stats()
    added = after["fallback_queries"] - before["fallback_queries"]
    assert after["queries"] - before["queries"] == n
    assert added == (n if filtered else 0), f"{n} x {X.shape[1]}, {len(CC)} centres: {added} rows listed"
    tree.set_engine("exact")
    el, ed, ei = tree.kmeans_assign(CC)
    tree.close()
    assert np.array_equal(labels, el) and _same_bits(dist, ed) and _same_bits(np.float64(inertia), np.float64(ei))
    assert labels.max() < distinct, "of two equal centres the lower number wins"
    wl, wd = ref.assign_matrix(X[:64], CC)
    assert np.array_equal(labels[:64], wl) and _same_bits(dist[:64], wd)


@pytest.mark.parametrize("dim,n,filtered", [(320, 6103, False), (320, 6104, True), (112, 34877, False), (112, 34878, True),
                                            (64, 61035, False), (64, 61036, True), (63, 62008, False), (63, 70000, False)])
def test_the_auto_line_in_the_work(pn, dim, n, filtered):
    nc = 4096
    work, line = float(n) * nc * dim, AUTO_WORK if dim >= 128 else AUTO_WORK_NARROW
    if dim >= 64:  # the smallest shapes on the line: one row fewer is below it
        assert (work >= line) == filtered and (filtered or float(n + 1) * nc * dim >= line)
    else:
        assert work >= line
    C = uniform((nc // 2, dim), 91 + dim)
    _auto_line_case(pn, uniform((n, dim), 90 + dim), np.ascontiguousarray(np.concatenate([C, C])), nc // 2, filtered)


@pytest.fixture(scope="module")
def long_corpus():
    """396 826 rows of 320 columns: a block of 1024 uniform rows again and again, each row offset in column 0"""
    n, dim = 396826, 320
    block = uniform((1024, dim), 95)
    X = np.ascontiguousarray(np.tile(block, ((n + 1023) // 1024, 1))[:n])
    X[:, 0] += (np.arange(n, dtype=np.float64) * 2.0 ** -19).astype(np.float32)
    return X


@pytest.mark.parametrize("nc,filtered", [(62, False), (63, False), (64, True)])
def test_the_auto_line_in_the_centre_count(pn, long_corpus, nc, filtered):
    """62 and 64 centres as 31 and 32 twins; 63 as 31 twins and a centre far from every row -- there the work is past
    8e9 (396 826 is the fewest rows for that) and the centre count alone keeps the filter off"""
    X = long_corpus
    n, dim = X.shape
    assert float(n) * 63 * dim >= AUTO_WORK > float(n - 1) * 63 * dim and float(n) * 64 * dim >= AUTO_WORK
    C = uniform((nc // 2, dim), 96)
    CC = np.concatenate([C, C])
    if nc % 2:
        CC = np.concatenate([CC, np.full((1, dim), -50.0, dtype=np.float32)])
    assert len(CC) == nc
    _auto_line_case(pn, X, np.ascontiguousarray(CC), nc // 2, filtered)
