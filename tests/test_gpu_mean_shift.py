"""pn_mean_shift_*: mean shift on the device against the contract written in plain numpy.

The contract (include/petal_mi355x.h) is stated over the library's own radius lists, so the reference here calls
``query_radius_batch(seeds, h)`` itself and does everything above the lists in numpy: every column of the listed rows in
f64, added 64 entries at a time into 64 lane partials, the partials folded in lane order, divided by the list's length and
rounded to the tree's type; the shift in the same shape over the columns.  What is compared is therefore the new code
alone, bit for bit.  The merge is compared with a sequential greedy over the library's Euclidean distance, the labels with
a k = 1 query on an index made of the centres, and the whole with scikit-learn's MeanShift.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE = 3
PN_OPT_MS_PIECE = 15
MERGE_ROUND = 1024  # consecutive ranks one round of the merge decides (csrc/pn_internal.h: kMsMergeRound)


# ------------------------------------------------------------------------------------------------ numpy reference
def fold64(v):
    """the fixed shape of every sum: ``v`` [m][...] in list order -> 64 lane partials (entry j to partial j mod 64, ascending
    j within a partial, from 0.0), folded in lane order"""
    m = v.shape[0]
    rows = max(1, -(-m // 64))
    pad = np.zeros((rows * 64,) + v.shape[1:], dtype=np.float64)
    pad[:m] = v
    p = np.zeros((64,) + v.shape[1:], dtype=np.float64)
    for r in range(rows):
        p = p + pad[r * 64:(r + 1) * 64]
    s = p[0].copy()
    for lane in range(1, 64):
        s = s + p[lane]
    return s


def ref_step(tree, x, seeds, h, base=0):
    """one step of every seed over the library's own lists: (new positions, points_within, shift)"""
    ns = seeds.shape[0]
    hq = np.full(ns, h, dtype=tree.dtype) if np.ndim(h) == 0 else np.asarray(h, dtype=tree.dtype)
    off, idx = tree.query_radius_batch(seeds, hq)
    off = off.astype(np.int64)
    idx = idx.astype(np.int64) - base
    out = seeds.copy()
    pw = np.diff(off).astype(np.uint64)
    shift = np.full(ns, np.nan)
    for q in range(ns):
        m = int(pw[q])
        if m == 0:
            continue
        lst = idx[off[q]:off[q + 1]]
        assert (np.diff(lst) > 0).all()
        s = fold64(x[lst].astype(np.float64))
        out[q] = (s / float(m)).astype(tree.dtype)
        dd = out[q].astype(np.float64) - seeds[q].astype(np.float64)
        shift[q] = np.sqrt(fold64(dd * dd))
    return out, pw, shift


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ ({int(gn.sum())} against {int(wn.sum())})"
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    bad = np.flatnonzero(got.view(u)[~gn] != want.view(u)[~wn])
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:5]}: {got[~gn][bad[:5]]} against {want[~wn][bad[:5]]}"


def check_step(tree, x, seeds, h, what, base=0):
    """``max_iter = 1`` against the reference; returns points_within"""
    modes, pw, it, sh, work = tree.mean_shift_modes(h, seeds, tol=0.0, max_iter=1, full=True)
    want_m, want_pw, want_sh = ref_step(tree, x, seeds, h, base)
    assert modes.dtype == tree.dtype and pw.dtype == np.uint64 and it.dtype == np.uint32 and sh.dtype == np.float64
    assert np.array_equal(pw, want_pw), f"{what}: points_within against the list lengths"
    same_bits(modes, want_m, what + ": modes")
    same_bits(sh, want_sh, what + ": shift")
    assert np.array_equal(it, (want_pw > 0).astype(np.uint32)), what
    assert work == (1, seeds.shape[0]), what
    dead = want_pw == 0
    assert np.array_equal(modes[dead], seeds[dead]) and np.isnan(sh[dead]).all()
    return pw


DT = [np.float32, np.float64]


# ---- 1. one step, bit for bit
@pytest.mark.parametrize("dt", DT)
def test_one_step_on_the_bf16_tier(pn, dt):
    x = uniform((20000, 16), 0x3E50, dt)
    seeds = np.concatenate([uniform((300, 16), 0x3E51, dt), np.full((3, 16), 40.0, dtype=dt) * np.array([[1], [-1], [2]], dtype=dt)])
    tree = pn.BallTree.euclidean(x)
    assert tree.bf16_eligible
    pw = check_step(tree, x, seeds, 1.0, "20000 x 16")
    print(f"20000 x 16: lists of {int(pw[:300].min())} .. {int(pw[:300].max())} entries, mean {float(pw[:300].mean()):.1f}")
    assert pw[:300].min() < 64 and pw[:300].max() >= 200 and (pw[300:] == 0).all()
    # the piece size never changes a result
    want = tree.mean_shift_modes(1.0, seeds, tol=0.0, max_iter=1, full=True)
    tree.set_option(PN_OPT_MS_PIECE, 1000)
    got = tree.mean_shift_modes(1.0, seeds, tol=0.0, max_iter=1, full=True)
    tree.set_option(PN_OPT_MS_PIECE, 0)
    for g, w, name in zip(got[:4], want[:4], ("modes", "points_within", "iterations", "shift")):
        same_bits(g, w, "PN_OPT_MS_PIECE = 1000: " + name)
    # PN_OPT_INDEX_BASE affects no output (the lists carry it)
    tree.set_option(PN_OPT_INDEX_BASE, 1000)
    check_step(tree, x, seeds[:64], 1.0, "20000 x 16, index base 1000", base=1000)
    tree.close()


@pytest.mark.parametrize("dt", DT)
def test_one_step_on_the_exact_scan(pn, dt):
    x = uniform((3000, 3), 0x3E52, dt)
    x[500:600] = x[500]  # a block of 100 duplicate rows
    seeds = uniform((200, 3), 0x3E53, dt)
    seeds[7] = x[500]
    tree = pn.BallTree.euclidean(x)
    pw = check_step(tree, x, seeds, 0.2, "3000 x 3")
    assert pw.min() < 64 < pw.max() and pw[7] >= 100
    # a list that is the duplicates alone: the mean of equal values is the value
    modes, pw1 = tree.mean_shift_modes(1e-4, seeds[7:8], tol=0.0, max_iter=1)
    assert pw1[0] == 100 and np.array_equal(modes[0], x[500])
    # one bandwidth per seed, 0, negative and NaN among them: those seeds are dead, the others untouched
    h = (0.2 * (0.5 + uniform((200,), 0x3E54, np.float64))).astype(dt)
    h[[0, 5, 9]] = [0.0, -1.0, np.nan]
    pw = check_step(tree, x, seeds, h, "3000 x 3, one h per seed")
    assert (pw[[0, 5, 9]] == 0).all() and (np.delete(pw, [0, 5, 9]) > 0).all()
    tree.set_option(PN_OPT_INDEX_BASE, 7)
    check_step(tree, x, seeds, h, "3000 x 3, index base 7", base=7)
    # hand-placed list lengths around the wave width
    xd, sd = x.astype(np.float64), seeds.astype(np.float64)
    hm = np.empty(6, dtype=dt)
    for i, m in enumerate((0, 1, 63, 64, 65, 129)):
        d = np.sort(np.sqrt(((xd - sd[20 + i]) ** 2).sum(axis=1)))
        hm[i] = d[0] / 2 if m == 0 else (d[m - 1] + d[m]) / 2
    pw = check_step(tree, x, seeds[20:26], hm, "3000 x 3, m = 0, 1, 63, 64, 65, 129", base=7)
    assert pw.tolist() == [0, 1, 63, 64, 65, 129]
    tree.close()


@pytest.mark.parametrize("dt", DT)
def test_one_step_on_wide_rows(pn, dt):
    x = uniform((5000, 200), 0x3E55, dt)
    seeds = uniform((60, 200), 0x3E56, dt)
    tree = pn.BallTree.euclidean(x)
    pw = check_step(tree, x, seeds, 5.5, "5000 x 200")
    print(f"5000 x 200: lists of {int(pw.min())} .. {int(pw.max())} entries")
    assert pw.max() > 64
    tree.close()


# ---- 2. iteration equals repeated steps
H2, TOL2 = 6.0, 6e-3


def blobs(dt):
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.standard_normal((2000, 16)) for _ in range(3)])
    x[2000:4000, 0] += 12.0
    x[4000:, 1] += 12.0
    x = x.astype(dt)
    seeds = np.concatenate([x[::20], np.full((2, 16), 100.0, dtype=dt) * np.array([[1], [-1]], dtype=dt)])
    return x, seeds


@pytest.fixture(scope="module", params=["f32", "f64"])
def case2(request, pn):
    dt = np.float32 if request.param == "f32" else np.float64
    x, seeds = blobs(dt)
    tree = pn.BallTree.euclidean(x)
    full = tree.mean_shift_modes(H2, seeds, tol=TOL2, full=True)
    yield {"x": x, "seeds": seeds, "tree": tree, "dt": dt, "full": full, "n_iter": tree.last_n_iter}
    tree.close()


def loop_of_steps(tree, seeds, h, tol, max_iter, limit=None):
    """the iteration as repeated ``max_iter = 1`` calls over the seeds still moving; ``h`` a scalar or one bandwidth per
    seed; ``limit``: every such call takes at most that many positions (the longer ones are made in parts)"""
    ns = seeds.shape[0]
    per_seed = np.ndim(h) != 0

    def one_step(pos, hh):
        step = len(pos) if limit is None else limit
        parts = [tree.mean_shift_modes(hh[a:a + step] if per_seed else hh, pos[a:a + step], tol=0.0, max_iter=1, full=True)
                 for a in range(0, len(pos), step)]
        return [np.concatenate([p[i] for p in parts]) for i in range(4)]

    modes = seeds.copy()
    pw = np.zeros(ns, dtype=np.uint64)
    it = np.zeros(ns, dtype=np.uint32)
    sh = np.full(ns, np.nan)
    act = np.arange(ns)
    pos = seeds.copy()
    hh = np.asarray(h, dtype=tree.dtype) if per_seed else h
    steps = iters = 0
    t = 0
    while act.size:
        t += 1
        iters += 1
        steps += act.size
        m1, p1, _, s1 = one_step(pos, hh)
        dead = p1 == 0
        stop = dead | (s1 <= tol) | (t == max_iter)
        modes[act[stop]] = np.where(dead[stop, None], pos[stop], m1[stop])
        pw[act[stop]] = p1[stop]
        it[act[stop]] = np.where(dead[stop], t - 1, t)
        sh[act[stop]] = s1[stop]
        act, pos = act[~stop], m1[~stop]
        if per_seed:
            hh = hh[~stop]
    return modes, pw, it, sh, (iters, steps)


def test_iteration_equals_repeated_steps(case2):
    tree, seeds = case2["tree"], case2["seeds"]
    got = case2["full"]
    want = loop_of_steps(tree, seeds, H2, TOL2, 300)
    for g, w, name in zip(got[:4], want[:4], ("modes", "points_within", "iterations", "shift")):
        same_bits(g, w, name)
    assert got[4] == want[4]
    it, pw = got[2], got[1]
    print(f"iterations {sorted(set(it.tolist()))}, work {got[4]}")
    assert (pw[-2:] == 0).all() and (it[-2:] == 0).all() and (pw[:-2] > 0).all()
    assert len(set(it[:-2].tolist())) > 1, "the seeds must retire at different times"
    # stopped seeds are not queried again: every live seed costs its iterations, every dead one the query that found it dead
    assert got[4][1] == int(it.sum()) + int((pw == 0).sum())
    assert got[4][0] == int(it.max()) and case2["n_iter"] == int(it.max())
    assert (got[3][:-2] <= TOL2).all()


def test_max_iter_cuts_every_seed(case2):
    tree, seeds = case2["tree"], case2["seeds"]
    got = tree.mean_shift_modes(H2, seeds, tol=TOL2, max_iter=2, full=True)
    want = loop_of_steps(tree, seeds, H2, TOL2, 2)
    for g, w, name in zip(got[:4], want[:4], ("modes", "points_within", "iterations", "shift")):
        same_bits(g, w, name)
    assert (got[2][:-2] == 2).all() and (got[3][:-2] > TOL2).all() and got[4] == (2, 2 * (len(seeds) - 2) + 2)


def test_seed_rows_and_device_entries(case2):
    import torch
    tree, x, seeds, dt = case2["tree"], case2["x"], case2["seeds"], case2["dt"]
    a = tree.mean_shift_modes(H2, None, tol=TOL2, max_iter=3, full=True)
    b = tree.mean_shift_modes(H2, x, tol=TOL2, max_iter=3, full=True)
    for g, w, name in zip(a[:4], b[:4], ("modes", "points_within", "iterations", "shift")):
        same_bits(g, w, "PN_MS_SEED_ROWS: " + name)
    assert a[4] == b[4]
    dev = torch.device("cuda", tree.device)
    want = case2["full"]
    # a strided view of the seeds, and one bandwidth per seed
    wide = torch.zeros((len(seeds), 24), dtype=torch.from_numpy(seeds).dtype, device=dev)
    wide[:, :16] = torch.from_numpy(seeds).to(dev)
    ht = torch.full((len(seeds),), H2, dtype=wide.dtype, device=dev)
    for h, s in ((H2, torch.from_numpy(seeds).to(dev)), (ht, wide[:, :16])):
        m, pw, it, sh, work = tree.mean_shift_modes_device(h, s, tol=TOL2)
        torch.cuda.synchronize()
        same_bits(m.cpu().numpy(), want[0], "device: modes")
        assert np.array_equal(pw.cpu().numpy().astype(np.uint64), want[1])
        assert np.array_equal(it.cpu().numpy().astype(np.uint32), want[2])
        same_bits(sh.cpu().numpy(), want[3], "device: shift")
        assert work == want[4]
    m, pw, it, sh, work = tree.mean_shift_modes_device(H2, None, tol=TOL2, max_iter=3)
    same_bits(m.cpu().numpy(), a[0], "device, PN_MS_SEED_ROWS: modes")
    assert np.array_equal(pw.cpu().numpy().astype(np.uint64), a[1]) and work == a[4]
    # merge and labels: the device entries against the host entries
    centres, cp, cos = tree.mean_shift_merge(want[0], want[1], dt(H2))
    dc, dcp, dcos, dnc = tree.mean_shift_merge_device(torch.from_numpy(want[0]).to(dev),
                                                      torch.from_numpy(want[1].astype(np.int64)).to(dev), H2)
    nc = int(dnc.cpu()[0])
    assert nc == len(centres)
    same_bits(dc.cpu().numpy()[:nc], centres, "device: centres")
    assert np.array_equal(dcp.cpu().numpy()[:nc].astype(np.uint64), cp) and np.array_equal(dcos.cpu().numpy(), cos)
    for cluster_all in (True, False):
        lab = tree.mean_shift_labels(centres, H2, cluster_all)
        dl = tree.mean_shift_labels_device(dc, H2, cluster_all, n_centres=nc)
        assert np.array_equal(dl.cpu().numpy(), lab)


# ---- 3. the merge against a sequential greedy over the library's distance
def lib_dist(pn, rows, b):
    """the library's Euclidean distance of every row of ``rows`` to ``b`` in the rows' type: the reference metric's
    sequential unfused fold and a correctly rounded square root"""
    s = np.zeros(rows.shape[0], dtype=rows.dtype)
    for k in range(rows.shape[1]):
        diff = rows[:, k] - b[k]
        s = s + diff * diff
    return np.sqrt(s)


def check_lib_dist(pn, modes):
    from petal_neighbors_amd import _lib
    f = getattr(_lib.lib(), "pn_euclidean_f32" if modes.dtype == np.float32 else "pn_euclidean_f64")
    rng = np.random.default_rng(5)
    for j in rng.integers(0, len(modes), 40):
        d = lib_dist(pn, modes, modes[j])
        for i in rng.integers(0, len(modes), 10):
            want = f(modes[i].ctypes.data_as(C.c_void_p), modes[j].ctypes.data_as(C.c_void_p), modes.shape[1])
            assert d[i] == modes.dtype.type(want)


def greedy_merge(pn, modes, pw, h):
    ns = len(pw)
    live = np.flatnonzero(pw > 0)
    order = live[np.lexsort((live, -pw[live].astype(np.int64)))]
    cos = np.full(ns, -1, dtype=np.int64)
    centre_seed = []
    rows = np.empty((0, modes.shape[1]), dtype=modes.dtype)
    for s in order:
        near = np.flatnonzero(lib_dist(pn, rows, modes[s]) < h)
        if near.size:
            cos[s] = near[0]
        else:
            cos[s] = len(centre_seed)
            centre_seed.append(s)
            rows = np.concatenate([rows, modes[s:s + 1]])
    centre_seed = np.array(centre_seed, dtype=np.int64)
    return modes[centre_seed], pw[centre_seed], cos


def check_merge(pn, tree, modes, pw, h, what):
    check_lib_dist(pn, modes)
    centres, cp, cos = tree.mean_shift_merge(modes, pw, h)
    wc, wcp, wcos = greedy_merge(pn, modes, pw, h)
    assert len(centres) == len(wc), f"{what}: {len(centres)} centres against {len(wc)}"
    same_bits(centres, wc, what + ": centres")
    assert np.array_equal(cp, wcp), what + ": centre_points"
    assert np.array_equal(cos, wcos), what + ": centre_of_seed"
    return centres, cos


def test_merge_of_the_blob_modes(pn, case2):
    modes, pw = case2["full"][0], case2["full"][1]
    centres, cos = check_merge(pn, case2["tree"], modes, pw, case2["dt"](H2), "blobs")
    assert len(centres) == 3 and (cos[-2:] == -1).all() and sorted(set(cos[:-2].tolist())) == [0, 1, 2]


@pytest.mark.parametrize("dt", DT)
def test_merge_synthetic(pn, dt):
    """2000 modes x 3 at h = 1: 1100 lattice points 2 apart (more centres than one round decides), 400 exact duplicates of
    them, 100 chains a - b - c with d(a, b) = d(b, c) = 0.625 and d(a, c) = 1.25, 100 modes at distance exactly 1 of a
    lattice point, 100 dead seeds; points_within from 1 .. 5, so most ranks are decided by the seed number; shuffled"""
    rng = np.random.default_rng(0x3E57)
    g = np.stack(np.meshgrid(np.arange(11), np.arange(10), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 3) * 2.0
    assert len(g) == 1100
    dup = g[rng.integers(0, 1100, 400)]
    base = g[rng.choice(1100, 100, replace=False)]
    a = base + np.array([0.0, 0.25, 0.0])
    b = a + np.array([0.625, 0.0, 0.0])
    c = b + np.array([0.625, 0.0, 0.0])
    edge = g[rng.integers(0, 1100, 100)] + np.array([0.0, 0.0, 1.0])
    dead = rng.random((100, 3)) * 20.0
    modes = np.concatenate([g, dup, a, b, c, edge, dead]).astype(dt)
    assert len(modes) == 2000
    pw = rng.integers(1, 6, 2000).astype(np.uint64)
    pw[1900:] = 0
    perm = rng.permutation(2000)
    modes, pw = np.ascontiguousarray(modes[perm]), pw[perm]
    tree = pn.BallTree.euclidean(np.zeros((4, 3), dtype=dt))
    centres, cos = check_merge(pn, tree, modes, pw, dt(1.0), "synthetic")
    print(f"synthetic: {len(centres)} centres")
    assert len(centres) > MERGE_ROUND and (cos[pw == 0] == -1).all() and (cos[pw > 0] >= 0).all()
    # an empty call, and a call of dead seeds alone
    e = tree.mean_shift_merge(np.zeros((0, 3), dtype=dt), np.zeros(0, dtype=np.uint64), 1.0)
    assert e[0].shape == (0, 3) and len(e[1]) == 0 and len(e[2]) == 0
    e = tree.mean_shift_merge(modes[:5], np.zeros(5, dtype=np.uint64), 1.0)
    assert e[0].shape == (0, 3) and (e[2] == -1).all()
    tree.close()


# ---- 4. the labels
@pytest.mark.parametrize("dt", DT)
def test_labels_equal_a_k1_query_on_the_centres(pn, dt):
    x = uniform((3000, 3), 0x3E58, dt) * dt(4.0)
    centres = np.concatenate([np.array([[0, 0, 0], [2, 0, 0]], dtype=dt), uniform((5, 3), 0x3E59, dt) * dt(4.0)])
    x[0] = [1, 0, 0]        # equidistant from centres 0 and 1: the lower number
    x[1] = [0, 0, -1]       # at distance exactly h = 1 of centre 0, farther from the others: an orphan
    x[2] = [0, 0, -0.9375]  # inside
    x[3] = [-3, -3, -3]     # far from every centre
    tree = pn.BallTree.euclidean(x)
    ctree = pn.BallTree.euclidean(centres)
    ki, kd = ctree.query_batch(x, 1)
    want = ki[:, 0].astype(np.int64)
    lab = tree.mean_shift_labels(centres, 1.0)
    assert lab.dtype == np.int64 and np.array_equal(lab, want)
    assert lab[0] == 0 and lab[1] == 0 and kd[1, 0] == 1.0
    orph = tree.mean_shift_labels(centres, 1.0, cluster_all=False)
    assert np.array_equal(orph, np.where(kd[:, 0] < dt(1.0), want, -1))
    assert orph[0] == -1 and orph[1] == -1 and orph[2] == 0 and orph[3] == -1 and (orph >= 0).sum() > 100
    # no centre: every row is an orphan, with or without the rule
    for cluster_all in (True, False):
        assert (tree.mean_shift_labels(np.zeros((0, 3), dtype=dt), 1.0, cluster_all) == -1).all()
    ctree.close()
    tree.close()


def test_labels_of_the_blobs(pn, case2):
    tree, x, dt = case2["tree"], case2["x"], case2["dt"]
    centres, _, _ = tree.mean_shift_merge(case2["full"][0], case2["full"][1], dt(H2))
    ctree = pn.BallTree.euclidean(centres)
    ki, _ = ctree.query_batch(x, 1)
    assert np.array_equal(tree.mean_shift_labels(centres, H2), ki[:, 0].astype(np.int64))
    labels, c2 = tree.mean_shift(H2, case2["seeds"], tol=TOL2)
    same_bits(c2, centres, "mean_shift: centres")
    assert np.array_equal(labels, ki[:, 0].astype(np.int64)) and tree.last_n_iter == case2["n_iter"]
    ctree.close()


# ---- 5. against scikit-learn
def test_against_scikit_learn(pn, case2):
    """scikit-learn's MeanShift(bandwidth = 6, seeds) on the blobs gives 3 centres and the blob partition; every mode lies
    within 0.0031 of its centre and at least 11.9 from the others, so '<' against '<=' and the tie-break cannot matter.
    Asserted: the same number of centres, the same partition of the rows, exactly one scikit-learn centre within h of each
    of ours.  The largest centre-to-centre distance is printed (a CPU restatement of the contract: 9.6e-6)."""
    try:
        from sklearn.cluster import MeanShift
    except Exception as e:  # noqa: BLE001
        pytest.skip(f"scikit-learn does not import: {e}")
    tree, x, seeds = case2["tree"], case2["x"], case2["seeds"]
    sk = MeanShift(bandwidth=H2, seeds=seeds).fit(x)
    labels, centres = tree.mean_shift(H2, seeds, tol=TOL2)
    assert len(sk.cluster_centers_) == 3 and len(centres) == 3
    d = np.sqrt(((centres.astype(np.float64)[:, None, :] - sk.cluster_centers_.astype(np.float64)[None, :, :]) ** 2).sum(axis=2))
    assert ((d < H2).sum(axis=1) == 1).all()
    match = d.argmin(axis=1)
    assert sorted(match.tolist()) == [0, 1, 2]
    print(f"{np.dtype(case2['dt']).name}: largest distance of a centre from scikit-learn's = {float(d.min(axis=1).max()):.3e}")
    assert np.array_equal(match[labels], sk.labels_)
    blob = np.repeat(np.arange(3), 2000)
    assert len(set(zip(labels.tolist(), blob.tolist()))) == 3
