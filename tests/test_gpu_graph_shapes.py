"""Every graph entry point, and the KDE, mean shift and k-means entries that borrow the same workspace scratch
(tests/fuzz_graph.py: one handle, one dense want side, two passes) at the smallest shapes where the code underneath changes.  Nothing above the k-NN layer ran on rows wider than 16 columns before: D > 128 is where the
bf16 tier switches to the K-chunked kernel and the chunked image layout, n >= 4096 with D >= 8 is where the auto engine
moves the self-queries to the tier at all.

    n                 D         element type, metric        what changes there
    4095, 4096, 4097  8         f32 Euclidean               tier threshold on n (also the one-launch small-corpus limit)
    4096              7         f32 Euclidean               tier threshold on D (D = 8: the row above)
    4200              128, 129  f32 and f64 Euclidean       last narrow width, first wide width (one K-chunk plus a column)
    4200              200       f32 Cosine, f32 Euclidean   wide, not a multiple of the chunk
    4096              768       f32 Euclidean               many K-chunks (the benchmarked width)
    4200              136       f64 Euclidean, and a family wide with ties, zero weights, NaN keys
                                with 30 duplicated rows and 2 NaN rows

The rows are Gaussian blobs with a uniform background of a tenth of the rows.  eps / max_eps were picked per case as the
median distance to the 25th / 50th nearest other row of the dense matrix, rounded to three digits: 10 .. 60 entries per
eps-list, the background rows beyond every radius (infinite cores, noise).  Each case's parameters stand next to it in
GRID; its conditions (fuzz_graph.conditions) hold without a redraw, which is asserted.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
#        n     D    dtype cosine family      nb  sigma  k   ms  m   eps      max_eps
GRID = [
    (4095, 8,   F32, False, "blobs",    12, 0.05, 10, 6, 10, 0.135  , 0.152),
    (4096, 8,   F32, False, "blobs",    12, 0.05, 10, 6, 10, 0.135  , 0.152),
    (4097, 8,   F32, False, "blobs",    12, 0.05, 10, 6, 10, 0.136  , 0.152),
    (4096, 7,   F32, False, "blobs",    12, 0.05, 10, 6, 10, 0.122  , 0.139),
    (4200, 128, F32, False, "blobs",    8,  0.05, 10, 6, 10, 0.731  , 0.747),
    (4200, 128, F64, False, "blobs",    8,  0.05, 10, 6, 10, 0.731  , 0.747),
    (4200, 129, F32, False, "blobs",    8,  0.05, 10, 6, 10, 0.735  , 0.75),
    (4200, 129, F64, False, "blobs",    8,  0.05, 10, 6, 10, 0.735  , 0.75),
    (4200, 200, F32, True,  "blobs",    8,  0.05, 10, 6, 10, 0.0254 , 0.0263),
    (4200, 200, F32, False, "blobs",    8,  0.05, 10, 6, 10, 0.93   , 0.946),
    (4096, 768, F32, False, "blobs",    8,  0.05, 10, 6, 10, 1.893  , 1.91),
    (4200, 136, F64, False, "blobs",    8,  0.05, 10, 6, 10, 0.756  , 0.772),
    (4200, 136, F64, False, "dups_nan", 8,  0.05, 10, 6, 10, 0.756  , 0.772),
]


def params_of(row, seed):
    n, dim, dt, cosine, family, nb, sigma, k, ms, m, eps, max_eps = row
    p = {"n": n, "dim": dim, "dtype": dt, "cosine": cosine, "family": family, "nb": nb, "sigma": sigma, "background": 0.1,
         "k": k, "ms": ms, "m": m, "seed": seed}
    if eps is not None:
        p.update(eps=eps, max_eps=max_eps)
    return p


def case_id(row):
    return f"{row[0]}x{row[1]}-{np.dtype(row[2]).name}-{'cosine' if row[3] else 'euclidean'}-{row[4]}"


@pytest.mark.parametrize("index", range(len(GRID)), ids=[case_id(r) for r in GRID])
def test_every_graph_entry_point_on_one_handle(pn, oracle_mod, index):
    import fuzz_graph
    rng = np.random.default_rng(500 + index)
    redraws = fuzz_graph.run_case(params_of(GRID[index], 40 + index), rng)
    assert redraws == 0  # the fixed grid needs no redraw
