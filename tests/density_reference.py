"""The KDE and mean shift contracts of include/petal_mi355x.h over CSR lists that come from anywhere, vectorised, for
checks at 3 10^5 lists where the per-query Python loops of tests/test_gpu_kde.py (``ref_sums``) and
tests/test_gpu_mean_shift.py (``ref_step``) no longer fit and where the lists must not come from the library.  Each is
proven bit for bit against the loop it replaces in tests/test_density_reference.py.

The shape of every sum is the header's: entry j of a list to lane partial j mod 64, ascending j within a partial, from
+0.0; the 64 partials folded in lane order.  A list padded with +0.0 to a multiple of 64 gives the same bits (x + 0.0 is
x for every x a partial can hold), so lists are grouped by their number of 64-entry rows and each group is one dense block.
"""
import numpy as np

_BLOCK_BYTES = 1 << 26  # the dense block of one group, at most


def kde_terms(kernel, dist, h):
    """the terms of list entries at distances ``dist`` (the tree's type) under the bandwidths ``h`` (f64, one per entry):
    d = max((double)dist, +0.0), every operation an IEEE f64 one in the header's order"""
    d = np.maximum(dist.astype(np.float64), 0.0)
    h = np.asarray(h, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kernel == "tophat":
            return np.ones_like(d)
        if kernel == "epanechnikov":
            return 1.0 - (d * d) / (h * h)
        if kernel == "linear":
            return 1.0 - d / h
        if kernel == "gaussian":
            return np.exp(-((d * d) / (2.0 * (h * h))))
        if kernel == "exponential":
            return np.exp(-(d / h))
    raise ValueError(kernel)


def _groups(cnt, width):
    """(rows of 64, list numbers) per group of lists with the same number of 64-entry rows, cut into blocks of at most
    _BLOCK_BYTES of f64 at ``width`` values per entry"""
    rows_of = np.maximum(-(-cnt // 64), 1)
    for rows in np.unique(rows_of):
        which = np.flatnonzero(rows_of == rows)
        step = max(int(_BLOCK_BYTES // (int(rows) * 64 * 8 * max(width, 1))), 1)
        for a in range(0, len(which), step):
            yield int(rows), which[a:a + step]


def _fold_lists(values, off, cnt):
    """values [entries][...] (f64) in list order -> [lists][...]: every list's sum in the 64-partial shape"""
    tail = values.shape[1:]
    out = np.zeros((len(cnt),) + tail, dtype=np.float64)
    for rows, which in _groups(cnt, int(np.prod(tail, dtype=np.int64))):
        c = cnt[which]
        pad = np.zeros((len(which), rows * 64) + tail, dtype=np.float64)
        li = np.repeat(np.arange(len(which)), c)
        pos = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        pad[li, pos] = values[np.repeat(off[which], c) + pos]
        p = np.zeros((len(which), 64) + tail, dtype=np.float64)
        for r in range(rows):
            p = p + pad[:, r * 64:(r + 1) * 64]
        s = p[:, 0].copy()
        for lane in range(1, 64):
            s = s + p[:, lane]
        out[which] = s
    return out


def kde_sums(off, dist, h, kernel, skip=None):
    """(sums f64, counts uint64) of the CSR lists (off, dist) with one bandwidth per list ``h`` (the tree's type).  ``skip``
    (optional, one per list): the position within the list of an entry that is left out, the positions behind it moving up
    by one -- the self entry without the own row; a negative value leaves nothing out."""
    off = np.asarray(off).astype(np.int64)
    cnt = np.diff(off)
    if skip is not None:
        skip = np.asarray(skip, dtype=np.int64)
        assert skip.shape == cnt.shape and (skip < cnt).all()
        out = skip >= 0
        keep = np.ones(len(dist), dtype=bool)
        keep[(off[:-1] + skip)[out]] = False
        dist = dist[keep]
        cnt = cnt - out
        off = np.concatenate([[0], np.cumsum(cnt)])
    t = kde_terms(kernel, dist, np.repeat(np.asarray(h).astype(np.float64), cnt))
    return _fold_lists(t, off, cnt), cnt.astype(np.uint64)


def ms_step(x, seeds, off, idx):
    """one mean shift step of every seed over the CSR lists (off, idx) of rows of ``x``: (new positions in the rows' type,
    points_within uint64, shift f64).  Every column of the listed rows in f64 in the 64-partial shape, divided by the
    list's length and rounded to the rows' type; the shift from ((double)p' - (double)p)^2 per column, column c to partial
    c mod 64, in the same shape, then the square root.  A seed with an empty list stays where it is; its shift is NaN."""
    off = np.asarray(off).astype(np.int64)
    idx = np.asarray(idx).astype(np.int64)
    cnt = np.diff(off)
    ns, dim = seeds.shape
    assert len(cnt) == ns and x.shape[1] == dim and x.dtype == seeds.dtype
    out = seeds.copy()
    shift = np.full(ns, np.nan)
    cols = -(-dim // 64) * 64
    for rows, which in _groups(cnt, dim):
        which = which[cnt[which] > 0]
        if which.size == 0:
            continue
        c = cnt[which]
        li = np.repeat(np.arange(len(which)), c)
        pos = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        pad = np.zeros((len(which), rows * 64, dim), dtype=np.float64)
        pad[li, pos] = x[idx[np.repeat(off[which], c) + pos]].astype(np.float64)
        p = np.zeros((len(which), 64, dim), dtype=np.float64)
        for r in range(rows):
            p = p + pad[:, r * 64:(r + 1) * 64]
        s = p[:, 0].copy()
        for lane in range(1, 64):
            s = s + p[:, lane]
        new = (s / c.astype(np.float64)[:, None]).astype(x.dtype)
        out[which] = new
        dd = new.astype(np.float64) - seeds[which].astype(np.float64)
        t = np.zeros((len(which), cols), dtype=np.float64)
        t[:, :dim] = dd * dd
        q = np.zeros((len(which), 64), dtype=np.float64)
        for r in range(cols // 64):
            q = q + t[:, r * 64:(r + 1) * 64]
        f = q[:, 0].copy()
        for lane in range(1, 64):
            f = f + q[:, lane]
        shift[which] = np.sqrt(f)
    return out, cnt.astype(np.uint64), shift


def with_self(off, idx, dist, live=None):
    """the lists (off, idx, dist) of rows 0 .. n - 1 without the rows themselves -> the lists with row i in its own list at
    distance 0, in ascending row order, and the position of that entry per list (-1 where ``live`` is False: such a row's
    list is left as it is)"""
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    cnt = np.diff(off)
    live = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    rows = np.repeat(np.arange(n), cnt)
    below = np.bincount(rows[idx < rows], minlength=n)  # entries in front of the own one
    new_off = np.concatenate([[0], np.cumsum(cnt + live)])
    n_idx = np.empty(int(new_off[-1]), dtype=np.int64)
    n_dist = np.zeros(int(new_off[-1]), dtype=dist.dtype)
    at = new_off[:-1] + below
    taken = np.zeros(len(n_idx), dtype=bool)
    taken[at[live]] = True
    n_idx[at[live]] = np.flatnonzero(live)
    n_idx[~taken] = idx
    n_dist[~taken] = dist
    return new_off, n_idx, n_dist, np.where(live, below, -1)
