"""KDE and mean shift beyond one 2^18-query pipeline chunk, against references that never touch the library.

Both families cut their queries (or the seeds still moving) into pieces of at most 2^18 and address every piece by hand;
their counting pass hands all queries to the radius pipeline in one call.  Two shapes put a piece behind 2^18:

a. The rows of tests/test_gpu_graph_chunks.py -- n = 2^18 + 3000 uniform in the plane, the rows 262140 .. 262150 equal --
   as their own queries and seeds.  The want side (``want_side``, which runs without a GPU in
   tests/test_density_reference.py) is the grid lists at R = 0.0062, about 32 entries per row, checked against the oracle
   on a sample, under tests/density_reference.py: compact kernels, the mean shift step and the labels bit for bit, the
   gaussian within the bound of tests/test_gpu_kde.py over the lists cut at the returned cutoff.  The same recipe cut to
   n = 2^18 exactly -- one full chunk, no remainder -- is the control.
b. nq = 2^18 + 3000 external queries against 4096 x 8 f32 rows, the smallest index the auto engine serves on the bf16
   tier, one bandwidth per query.  The want side of a call that long is the same call made in two parts, [0, 2^18) and
   [2^18, nq), and a sample of 200 queries -- the first 50, the 100 around the boundary, the last 50 -- through the
   references of tests/test_gpu_kde.py and tests/test_gpu_mean_shift.py, its counts against oracle.brute_radius.
   H_EXT = 0.5 was chosen on the CPU: oracle.brute_radius over the first 2000 queries lists 20.6 rows on average at
   H_EXT (0.44: 8.6, 0.47: 13.5) and 26.3 under the bandwidths H_EXT * (0.8 .. 1.2), the longest list 170.

mean_shift_merge at 2^18 seeds (sequential rounds of 1024 ranks: a benchmark shape) and sharded handles (which have
neither family) are not covered here.
"""
import numpy as np
import pytest

from conftest import uniform
from density_reference import kde_sums, ms_step, with_self
from graph_reference_large import truncate_lists
from test_gpu_graph_chunks import CHUNK, N, R, full_lists, pieces_of
from test_gpu_kde import COMPACT, check as kde_check, cutoff_within_bounds, smooth_bound, smooth_cutoff
from test_gpu_mean_shift import check_step, lib_dist, loop_of_steps

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE = 3
PN_OPT_KDE_PIECE = 14
PN_OPT_MS_PIECE = 15
NAMED = np.r_[262139:262152, CHUNK - 1, CHUNK, N - 1]  # the rows a failure message speaks of
H_GAUSS, ATOL_GAUSS = 0.0012, 1.0
H_LABELS = 2.0 ** -7
N_CENTRES = 37
H_EXT = 0.5
FIELDS = ("modes", "points_within", "iterations", "shift")


# --------------------------------------------------------------------------------------------------- comparisons
def where(bad, n):
    bad = np.flatnonzero(bad)
    named = [int(i) for i in NAMED if i < n and bad.size and i in bad]
    return (f"{bad.size} of {n} differ, first at {bad[:5].tolist()}, last at {bad[-3:].tolist()} (2^18 = {CHUNK}); "
            f"of the rows {NAMED[0]} .. {NAMED[-4]}, {CHUNK - 1}, {CHUNK}, {N - 1}: {named}")


def same(got, want, what):
    """array equality, floats by their bits (a NaN equals a NaN); a failure names the first differing positions"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    if got.dtype.kind == "f":
        u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
        bad = (got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    if bad.ndim == 2:
        bad = bad.any(axis=1)
    assert not bad.any(), f"{what}: {where(bad, len(bad))}"


def same_all(got, want, what, names):
    for g, w, name in zip(got, want, names):
        same(g, w, f"{what}: {name}")


# ----------------------------------------------------------------------------------------------------- want side
def bandwidths(dtype):
    """one bandwidth per row, R * u_i with u_i uniform in [0.5, 1]; every 97th is 0, negative or NaN"""
    u = np.random.default_rng(97).uniform(0.5, 1.0, N)
    h = (R * u).astype(dtype)
    bad = np.arange(0, N, 97)
    h[bad] = np.resize(np.array([0.0, -1.0, np.nan], dtype=dtype), len(bad))
    return h


def cut_lists(off, dist, h):
    """(keep mask, offsets) of the entries with dist < h of their list (one h per list, or a scalar)"""
    cnt = np.diff(off)
    rows = np.repeat(np.arange(len(cnt)), cnt)
    with np.errstate(invalid="ignore"):
        keep = dist < (h[rows] if np.ndim(h) else h)
    out = np.zeros(len(cnt) + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(rows[keep], minlength=len(cnt)))
    return keep, out


def self_lists(off, idx, dist, h):
    """the lists (off, idx, dist) without the rows themselves, cut at h (a scalar or one per row), with the rows of h > 0
    put into their own lists at distance 0: (offsets, distances, the own entry's position or -1, h per row)"""
    n = len(off) - 1
    hq = np.full(n, h, dtype=dist.dtype) if np.ndim(h) == 0 else np.asarray(h, dtype=dist.dtype)
    keep, c_off = cut_lists(off, dist, hq)
    s_off, _, s_dist, s_pos = with_self(c_off, idx[keep], dist[keep], hq > 0)
    return s_off, s_dist, s_pos, hq


def kde_self_want(lists, kernel, include, h=None):
    """(sum, count) of the self entry over ``self_lists``: where the entry excludes the rows, they are left out of their
    lists by position, as the device does; h: the bandwidth where it is not the cutoff"""
    s_off, s_dist, s_pos, hq = lists
    return kde_sums(s_off, s_dist, hq if h is None else np.full(len(hq), h, dtype=hq.dtype), kernel, None if include else s_pos)


def label_centres(pts):
    """37 centres: rows from both sides of the boundary, two of them (5 and 20) moved to the same distance 2^-9 left and
    right of one row, the last one to exactly H_LABELS above another row; (centres, the tie's row, the edge's row)"""
    dt = pts.dtype.type
    rng = np.random.default_rng(37)
    centres = pts[np.r_[rng.integers(0, CHUNK, N_CENTRES - 12), rng.integers(CHUNK, N, 12)]].copy()
    inner = (pts > 0.25).all(axis=1) & (pts < 0.75).all(axis=1)
    tie, edge = (int(i) for i in CHUNK + 10 + np.flatnonzero(inner[CHUNK + 10:])[:2])
    centres[5] = pts[tie] + np.array([2.0 ** -9, 0], dtype=dt)
    centres[20] = pts[tie] - np.array([2.0 ** -9, 0], dtype=dt)
    centres[36] = pts[edge] + np.array([0, H_LABELS], dtype=dt)
    return np.ascontiguousarray(centres), tie, edge


def labels_want(pts, centres):
    """the dense n x 37 matrix by the library's distance, argmin by (distance, centre number): (labels, nearest distance)"""
    d = np.stack([lib_dist(None, pts, c) for c in centres], axis=1)
    lab = np.argmin(d, axis=1).astype(np.int64)  # (the first of equal minima: the lower centre)
    return lab, d[np.arange(len(pts)), lab], d


def want_side(oracle_mod, dtype=np.float32):
    """everything case a compares against, with every condition asserted: runs without a GPU.  f64: the one KDE case."""
    dt = dtype
    w = {"dt": dt}
    pts, off, idx, dist = full_lists(oracle_mod, dt)
    print(f"lists at R = {R}: {float(off[-1]) / N:.1f} entries per row")
    assert 25 < float(off[-1]) / N < 40
    assert np.count_nonzero(dist[off[262140]:off[262141]] == 0) == 10  # (the planted duplicates)
    w["pts"] = pts
    w["h_rows"] = h_rows = bandwidths(dt)
    for kind, bad in (("zero", h_rows == 0), ("negative", h_rows < 0), ("NaN", np.isnan(h_rows))):
        assert bad[:CHUNK].sum() >= 5 and bad[CHUNK:].sum() >= 5, kind  # in both halves of the boundary
    if dt == np.float64:
        w["big"] = {"n": N, "kde": {("epanechnikov", False): kde_self_want(self_lists(off, idx, dist, dt(R)), "epanechnikov", False)}}
        return w
    # the gaussian cutoff: below R, so the lists cut at it are the call's lists
    c_gauss = smooth_cutoff("gaussian", float(dt(H_GAUSS)), N, ATOL_GAUSS)
    print(f"gaussian cutoff of h = {H_GAUSS}, atol = {ATOL_GAUSS}: about {c_gauss:.6f}")
    assert 0.0059 < c_gauss and c_gauss * (1.0 + 2.0 ** -20) < R
    for name, n in (("big", N), ("control", CHUNK)):
        t_off, t_idx, t_dist = truncate_lists(off, idx, dist, n)
        c = {"n": n, "lists": (t_off, t_idx, t_dist), "kde": {}, "kde_rows": {}}
        at_r = self_lists(t_off, t_idx, t_dist, dt(R))
        for kernel in COMPACT:
            for include in (False, True):
                c["kde"][kernel, include] = kde_self_want(at_r, kernel, include)
            assert np.array_equal(c["kde"][kernel, False][1], np.diff(t_off).astype(np.uint64)), name
            assert np.array_equal(c["kde"][kernel, True][1], np.diff(t_off).astype(np.uint64) + np.uint64(1)), name
        # (left out by position is left out of the list: the lists without the rows give the same bits)
        plain = kde_sums(t_off, t_dist, np.full(n, R, dtype=dt), "epanechnikov")
        assert plain[0].tobytes() == c["kde"]["epanechnikov", False][0].tobytes(), name
        at_h = self_lists(t_off, t_idx, t_dist, h_rows[:n])
        for include in (False, True):
            c["kde_rows"][include] = kde_self_want(at_h, "linear", include)
        cnt = c["kde_rows"][False][1]
        print(f"{name}: one bandwidth per row: {float(cnt.mean()):.1f} entries per row")
        assert 10 < cnt.mean() < 25 and (cnt[~(h_rows[:n] > 0)] == 0).all(), name
        assert np.array_equal(c["kde_rows"][True][1] - cnt, (h_rows[:n] > 0).astype(np.uint64)), name
        g_cnt = np.diff(cut_lists(t_off, t_dist, dt(c_gauss))[1])
        print(f"{name}: gaussian: {float(g_cnt.mean()):.1f} entries per row at the cutoff")
        assert 25 < g_cnt.mean() < 35, name
        # mean shift: every row is in its own list at distance 0 < R
        s_off, s_idx, _, _ = with_self(t_off, t_idx, t_dist)
        assert np.array_equal(s_off, at_r[0]), name
        c["s_off"] = s_off
        c["step"] = step = ms_step(pts[:n], pts[:n], s_off, s_idx)
        assert (step[1] == np.diff(t_off).astype(np.uint64) + np.uint64(1)).all() and np.isfinite(step[2]).all(), name
        assert np.array_equal(step[0][262140:min(262151, n)], np.repeat(step[0][262140:262141], min(262151, n) - 262140, axis=0))
        c["tol"] = tol = float(np.median(step[2]))
        for side, part in (("below 2^18", step[2][:CHUNK]), ("from 2^18", step[2][CHUNK:])):
            go, stop = int((part > tol).sum()), int((part <= tol).sum())
            print(f"{name}: tol = {tol:.6g}: rows {side}: {stop} stop after the first step, {go} go on")
            assert part.size == 0 or (stop >= 1000 and go >= 1000), f"{name}: {side}"
        w[name] = c
    # the pieces of the self entry and of the first mean shift step: the lists with the rows themselves
    s_off = w["big"]["s_off"]
    total = int(s_off[-1])
    w["piece"] = piece = total // 3 + 1000
    cut = pieces_of(s_off, N, piece)
    print(f"pieces of {piece} of {total} entries: {cut}; default piece: {pieces_of(s_off, N, 1 << 27)}")
    assert any(b <= CHUNK for a, b in cut) and any(a < CHUNK < b for a, b in cut)  # inside a chunk, and across the boundary
    assert pieces_of(s_off, N, 1 << 27) == [(0, CHUNK), (CHUNK, N)]               # the default piece ends at the limit
    # the labels
    centres, tie, edge = label_centres(pts)
    lab, near, d = labels_want(pts, centres)
    assert centres.shape == (N_CENTRES, 2) and N_CENTRES % 4 != 0
    assert d[tie, 5] == d[tie, 20] == near[tie] == dt(2.0 ** -9) and lab[tie] == 5          # equidistant: the lower number
    assert near[edge] == dt(H_LABELS) and lab[edge] == 36 and np.sort(d[edge])[1] > dt(H_LABELS)  # at exactly h: an orphan
    orphan = np.where(near < dt(H_LABELS), lab, -1)
    print(f"labels: {len(np.unique(lab))} centres used, {int((orphan >= 0).sum())} rows within h = {H_LABELS} of their centre")
    assert len(np.unique(lab)) == N_CENTRES and orphan[edge] == -1 and orphan[tie] == 5
    assert (orphan[:CHUNK] >= 0).sum() >= 100 and (orphan[CHUNK:] >= 0).sum() >= 10
    w["labels"] = {"centres": centres, True: lab, False: orphan}
    return w


@pytest.fixture(scope="module")
def want(oracle_mod):
    return want_side(oracle_mod)


@pytest.fixture(scope="module")
def trees(pn, want):
    out = {"big": pn.BallTree.euclidean(want["pts"]), "control": pn.BallTree.euclidean(np.ascontiguousarray(want["pts"][:CHUNK]))}
    yield out
    for t in out.values():
        t.close()


# ------------------------------------------------------------------------------------------- a. the KDE self entry
KDE_OUT = ("sum", "count", "cutoff")


@pytest.mark.parametrize("name", ["big", "control"])
@pytest.mark.parametrize("kernel", COMPACT)
def test_kde_self_compact_kernels(want, trees, name, kernel):
    w, tree = want[name], trees[name]
    for include in (False, True):
        s, cnt, cut = tree.kernel_density_raw(None, R, kernel, include_self=include)
        what = f"{name}: kernel_density_raw(None, {R}, {kernel}, include_self={include})"
        same(cnt, w["kde"][kernel, include][1], what + ": count")
        same(cut, np.full(w["n"], R, dtype=np.float32), what + ": cutoff")
        same(s, w["kde"][kernel, include][0], what + ": sum")


@pytest.mark.parametrize("name", ["big", "control"])
def test_kde_self_one_bandwidth_per_row(want, trees, name):
    w, tree = want[name], trees[name]
    h = want["h_rows"][:w["n"]]
    for include in (False, True):
        s, cnt, cut = tree.kernel_density_raw(None, h, "linear", include_self=include)
        what = f"{name}: kernel_density_raw(None, one h per row, linear, include_self={include})"
        same(cnt, w["kde_rows"][include][1], what + ": count")
        same(cut, h, what + ": cutoff")
        same(s, w["kde_rows"][include][0], what + ": sum")


@pytest.mark.parametrize("name", ["big", "control"])
def test_kde_self_gaussian(want, trees, name):
    w, tree = want[name], trees[name]
    t_off, t_idx, t_dist = w["lists"]
    n = w["n"]
    for include in (False, True):
        s, cnt, cut = tree.kernel_density_raw(None, H_GAUSS, "gaussian", ATOL_GAUSS, include_self=include)
        what = f"{name}: kernel_density_raw(None, {H_GAUSS}, gaussian, atol = {ATOL_GAUSS}, include_self={include})"
        assert (cut == cut[0]).all() and cut[0] < np.float32(R), what
        assert cutoff_within_bounds(cut, smooth_cutoff("gaussian", float(np.float32(H_GAUSS)), n, ATOL_GAUSS)), what
        # the want lists: the grid lists cut at the returned cutoff
        w_sum, w_cnt = kde_self_want(self_lists(t_off, t_idx, t_dist, cut[0]), "gaussian", include, np.float32(H_GAUSS))
        same(cnt, w_cnt, what + ": count")
        dev, bound = np.abs(s - w_sum), smooth_bound(w_sum, w_cnt)
        print(f"{what}: largest |S_dev - S_ref| / bound = {float((dev[bound > 0] / bound[bound > 0]).max(initial=0.0)):.3f}")
        assert (dev <= bound).all(), f"{what}: sum beyond the bound: {where(dev > bound, n)}"


def test_kde_self_pieces_index_base_and_device_entry(want, trees):
    import torch
    tree, w = trees["big"], want["big"]
    w_sum, w_cnt = w["kde"]["epanechnikov", False]
    h = want["h_rows"]
    r_sum, r_cnt = w["kde_rows"][False]
    try:
        tree.set_option(PN_OPT_KDE_PIECE, want["piece"])  # pieces inside the chunks and across the boundary
        cut_a = tree.kernel_density_raw(None, R, "epanechnikov")
        rows_a = tree.kernel_density_raw(None, h, "linear")
        tree.set_option(PN_OPT_KDE_PIECE, 0)              # the default: a piece ends at the 2^18-query limit
        cut_b = tree.kernel_density_raw(None, R, "epanechnikov")
        rows_b = tree.kernel_density_raw(None, h, "linear")
        same_all(cut_a, cut_b, f"pieces of {want['piece']} entries against the default piece", KDE_OUT)
        same_all(rows_a, rows_b, f"pieces of {want['piece']} entries against the default piece, one h per row", KDE_OUT)
        same(cut_a[0], w_sum, f"pieces of {want['piece']} entries: sum")
        same(cut_a[1], w_cnt, f"pieces of {want['piece']} entries: count")
        same(rows_a[0], r_sum, f"pieces of {want['piece']} entries, one h per row: sum")
        same(rows_a[1], r_cnt, f"pieces of {want['piece']} entries, one h per row: count")
        tree.set_option(PN_OPT_INDEX_BASE, 1 << 33)
        same_all(tree.kernel_density_raw(None, R, "epanechnikov"), cut_b, "index base 2^33", KDE_OUT)
        same_all(tree.kernel_density_raw(None, h, "linear"), rows_b, "index base 2^33, one h per row", KDE_OUT)
    finally:
        tree.set_option(PN_OPT_KDE_PIECE, 0)
        tree.set_option(PN_OPT_INDEX_BASE, 0)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        dev = tree.kernel_density_self_device(R, "epanechnikov", stream=st.cuda_stream)
        dev_rows = tree.kernel_density_self_device(torch.from_numpy(h).cuda(), "linear", include_self=True, stream=st.cuda_stream)
    st.synchronize()
    for got, host, what in ((dev, cut_b, "device entry"), (dev_rows, tree.kernel_density_raw(None, h, "linear", include_self=True),
                                                           "device entry, one h per row, with the rows")):
        same(got[0].cpu().numpy(), host[0], what + ": sum")
        same(got[1].cpu().numpy().astype(np.uint64), host[1], what + ": count")
        same(got[2].cpu().numpy(), host[2], what + ": cutoff")
    same(dev_rows[0].cpu().numpy(), w["kde_rows"][True][0], "device entry, one h per row, with the rows: sum against the reference")


def test_kde_self_f64(pn, oracle_mod):
    w = want_side(oracle_mod, np.float64)
    tree = pn.BallTree.euclidean(w["pts"])
    s, cnt, cut = tree.kernel_density_raw(None, R, "epanechnikov")
    tree.close()
    same(cnt, w["big"]["kde"]["epanechnikov", False][1], "f64: count")
    same(cut, np.full(N, R, dtype=np.float64), "f64: cutoff")
    same(s, w["big"]["kde"]["epanechnikov", False][0], "f64: sum")


# --------------------------------------------------------------------------------------- a. mean shift, seeds = rows
@pytest.mark.parametrize("name", ["big", "control"])
def test_mean_shift_one_step(want, trees, name):
    w, tree = want[name], trees[name]
    n = w["n"]
    w_modes, w_pw, w_shift = w["step"]
    for seeds, how in ((None, "PN_MS_SEED_ROWS"), (want["pts"][:n], "the rows as seeds")):
        modes, pw, it, sh, work = tree.mean_shift_modes(R, seeds, tol=0.0, max_iter=1, full=True)
        what = f"{name}: one step, {how}"
        same(pw, w_pw, what + ": points_within")
        same(it, np.ones(n, dtype=np.uint32), what + ": iterations")
        same(modes, w_modes, what + ": modes")
        same(sh, w_shift, what + ": shift")
        assert work == (1, n), what


@pytest.mark.parametrize("name", ["big", "control"])
def test_mean_shift_iteration_across_the_boundary(want, trees, name):
    import torch
    w, tree = want[name], trees[name]
    n, tol = w["n"], w["tol"]
    pts = np.ascontiguousarray(want["pts"][:n])
    ref = loop_of_steps(tree, pts, R, tol, 4, limit=CHUNK)  # (single steps of at most 2^18 positions)
    try:
        tree.set_option(PN_OPT_MS_PIECE, want["piece"])
        got = tree.mean_shift_modes(R, None, tol=tol, max_iter=4, full=True)
        tree.set_option(PN_OPT_MS_PIECE, 0)
        again = tree.mean_shift_modes(R, None, tol=tol, max_iter=4, full=True)
    finally:
        tree.set_option(PN_OPT_MS_PIECE, 0)
    same_all(got[:4], again[:4], f"{name}: pieces of {want['piece']} entries against the default piece", FIELDS)
    same_all(got[:4], ref[:4], f"{name}: the iteration against repeated steps", FIELDS)
    assert got[4] == again[4] == ref[4], name
    modes, pw, it, sh, work = got
    # the first step against the reference over the grid lists: the seeds it stops, and nobody else, have 1 iteration
    first = w["step"][2] <= tol
    same(it == 1, first, f"{name}: the seeds that stop after the first step")
    same(modes[first], w["step"][0][first], f"{name}: the modes of the seeds that stop after the first step")
    same(sh[first], w["step"][2][first], f"{name}: the shifts of the seeds that stop after the first step")
    for side, part in (("below 2^18", it[:CHUNK]), ("from 2^18", it[CHUNK:])):
        print(f"{name}: iterations of the rows {side}: {dict(zip(*np.unique(part, return_counts=True)))}")
        assert part.size == 0 or len(np.unique(part)) >= 2, f"{name}: {side}"
    assert (pw > 0).all() and work[1] == int(it.sum()) + int((pw == 0).sum()) and work[0] == int(it.max())
    if name == "big":
        dm, dpw, dit, dsh, dwork = tree.mean_shift_modes_device(R, torch.from_numpy(pts).cuda(), tol=tol, max_iter=4)
        dev = (dm.cpu().numpy(), dpw.cpu().numpy().astype(np.uint64), dit.cpu().numpy().astype(np.uint32), dsh.cpu().numpy())
        same_all(dev, got[:4], "the device entry against the host entry", FIELDS)
        assert dwork == work


def test_mean_shift_labels(want, trees):
    import torch
    tree, w = trees["big"], want["labels"]
    dc = torch.from_numpy(w["centres"]).cuda()
    for cluster_all in (True, False):
        what = f"mean_shift_labels({N_CENTRES} centres, {H_LABELS}, cluster_all={cluster_all})"
        same(tree.mean_shift_labels(w["centres"], H_LABELS, cluster_all), w[cluster_all], what)
        same(tree.mean_shift_labels_device(dc, H_LABELS, cluster_all).cpu().numpy(), w[cluster_all], what + ", device entry")


# ------------------------------------------------------------------ b. external queries beyond one chunk, bf16 tier
GAUSS_EXT = 0.18  # times sqrt(2 ln(4096 / 1e-3)) = 5.52: the gaussian's cutoffs are about the compact kernels'
SAMPLE = np.r_[0:50, CHUNK - 50:CHUNK + 50, N - 50:N]


def ext_bandwidths():
    h = (H_EXT * (0.8 + 0.4 * uniform((N,), 0xD3C2, np.float64))).astype(np.float32)
    bad = np.arange(0, N, 97)
    h[bad] = np.resize(np.array([0.0, -1.0, np.nan], dtype=np.float32), len(bad))
    return h


@pytest.fixture(scope="module")
def ext(pn, oracle_mod):
    x = uniform((4096, 8), 0xD3C0, np.float32)
    q = uniform((N, 8), 0xD3C1, np.float32)
    h = ext_bandwidths()
    assert not (h[SAMPLE] > 0).all() and (~(h[:CHUNK] > 0)).sum() > 5 and (~(h[CHUNK:] > 0)).sum() > 5
    tree = pn.BallTree.euclidean(x)
    assert tree.bf16_eligible
    # the sample's lists by the oracle: one count per sampled query, and the mean the bandwidth was chosen for
    counts = np.array([len(oracle_mod.brute_radius(x, q[i], h[i])) for i in SAMPLE])
    flat = np.array([len(oracle_mod.brute_radius(x, q[i], np.float32(H_EXT))) for i in range(2000)])
    print(f"H_EXT = {H_EXT}: {float(flat.mean()):.1f} rows per list over the first 2000 queries")
    assert 10 < flat.mean() < 40
    yield {"x": x, "q": q, "h": h, "tree": tree, "counts": counts}
    tree.close()


@pytest.mark.parametrize("kernel, atol", [("epanechnikov", 0.0), ("gaussian", 1e-3)])
def test_external_kde(ext, oracle_mod, kernel, atol):
    import torch
    tree, x, q, h = ext["tree"], ext["x"], ext["q"], ext["h"]
    hk = h if kernel == "epanechnikov" else (h * np.float32(GAUSS_EXT)).astype(np.float32)
    whole = tree.kernel_density_raw(q, hk, kernel, atol)
    parts = [tree.kernel_density_raw(q[a:b], hk[a:b], kernel, atol) for a, b in ((0, CHUNK), (CHUNK, N))]
    same_all(whole, [np.concatenate(p) for p in zip(*parts)], f"{kernel}: the whole call against its two parts", KDE_OUT)
    live = hk > 0
    print(f"{kernel}: {float(whole[1][live].mean()):.1f} rows per list")
    assert 10 < whole[1][live].mean() < 40 and (whole[1][~live] == 0).all() and (whole[0][~live] == 0).all()
    same(tree.query_radius_count(q, whole[2]), whole[1], f"{kernel}: query_radius_count at the returned cutoffs")
    small = kde_check(tree, q[SAMPLE], hk[SAMPLE], kernel, f"{kernel}: the sample", atol=atol)
    oracle_counts = np.array([len(oracle_mod.brute_radius(x, q[i], c)) for i, c in zip(SAMPLE, small[2])])
    same(small[1], oracle_counts.astype(np.uint64), f"{kernel}: the sample's counts against the oracle")
    if kernel == "epanechnikov":
        same(small[1], ext["counts"].astype(np.uint64), "the sample's counts against the oracle at h")
    same_all([v[SAMPLE] for v in whole], small, f"{kernel}: the whole call at the sample against the small call", KDE_OUT)
    if kernel == "epanechnikov":
        s, c, cut = tree.kernel_density_device(torch.from_numpy(q).cuda(), torch.from_numpy(hk).cuda(), kernel, atol)
        torch.cuda.synchronize()
        same_all((s.cpu().numpy(), c.cpu().numpy().astype(np.uint64), cut.cpu().numpy()), whole, "device entry", KDE_OUT)


def test_external_mean_shift_one_step(ext):
    tree, x, q, h = ext["tree"], ext["x"], ext["q"], ext["h"]
    whole = tree.mean_shift_modes(h, q, tol=0.0, max_iter=1, full=True)
    parts = [tree.mean_shift_modes(h[a:b], q[a:b], tol=0.0, max_iter=1, full=True) for a, b in ((0, CHUNK), (CHUNK, N))]
    same_all(whole[:4], [np.concatenate(p) for p in zip(*[p[:4] for p in parts])], "one step: the whole call against its two parts",
             FIELDS)
    assert whole[4] == (1, N)
    pw = check_step(tree, x, np.ascontiguousarray(q[SAMPLE]), h[SAMPLE], "one step: the sample")
    same(pw, ext["counts"].astype(np.uint64), "one step: the sample's points_within against the oracle")
    small = tree.mean_shift_modes(h[SAMPLE], np.ascontiguousarray(q[SAMPLE]), tol=0.0, max_iter=1, full=True)
    same_all([v[SAMPLE] for v in whole[:4]], small[:4], "one step: the whole call at the sample against the small call", FIELDS)


def test_external_mean_shift_iteration(ext):
    import torch
    tree, q, h = ext["tree"], ext["q"], ext["h"]
    small = tree.mean_shift_modes(h[SAMPLE], np.ascontiguousarray(q[SAMPLE]), tol=0.0, max_iter=1, full=True)  # (pinned above)
    tol = float(np.nanmedian(small[3]))
    ref = loop_of_steps(tree, q, h, tol, 3, limit=CHUNK)
    got = tree.mean_shift_modes(h, q, tol=tol, max_iter=3, full=True)
    same_all(got[:4], ref[:4], "the iteration against repeated steps", FIELDS)
    assert got[4] == ref[4]
    modes, pw, it, sh, work = got
    for side, part in (("below 2^18", it[:CHUNK]), ("from 2^18", it[CHUNK:])):
        print(f"iterations of the seeds {side}: {dict(zip(*np.unique(part, return_counts=True)))}")
        assert len(np.unique(part[part > 0])) >= 2, side  # the seeds retire at different times
    assert work[1] == int(it.sum()) + int((pw == 0).sum()) and work[0] == 3
    dm, dpw, dit, dsh, dwork = tree.mean_shift_modes_device(torch.from_numpy(h).cuda(), torch.from_numpy(q).cuda(), tol=tol, max_iter=3)
    dev = (dm.cpu().numpy(), dpw.cpu().numpy().astype(np.uint64), dit.cpu().numpy().astype(np.uint32), dsh.cpu().numpy())
    same_all(dev, got[:4], "the device entry against the host entry", FIELDS)
    assert dwork == work
