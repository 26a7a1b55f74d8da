"""The f32 MFMA tier (index.hip mfma_plan / run_mfma: mfma_filter_v2 -> select_rerank) at the boundaries of its plan:
the k' at which the candidate buffers change kind and capacity (30 | 31, 94 | 95), at which the re-rank's cells grow
(160 | 161), the last k' the tier admits (192 | 193), both kernel structures, the wide-row gate, the other branch of
the k' rule (many query tiles), and the largest segment count (33) where the re-rank's LDS decides how many workgroups
may share a query tile.  Every answer is the oracle's brute force bit for bit -- no tolerances -- and every case that
the tier is meant to serve proves from the statistics that it did: a call that fell through to the exact scan adds no
candidates.

k' below is mfma_slots(): k + 2 + k // 16 while query tiles * 3 <= CUs, else k + 6 (k < 16) or k + k // 4 + 4.
"""
import threading

import numpy as np
import pytest

from conftest import uniform
from test_gpu_parity import _check_knn, _same_dist

pytestmark = pytest.mark.gpu


def _queries(pts, nq, seed):
    """one third corpus rows (distance 0: worst cancellation for the GEMM expansion), two thirds fresh draws"""
    return np.concatenate([pts[: nq // 3], uniform((nq - nq // 3, pts.shape[1]), seed, np.float32)])


def _served(tree, nq, k):
    """What test_mfma_engine_vs_oracle asserts of a call the tier served; False: no filter tier ran at all."""
    st = tree.stats()
    assert st["hot_launches"] == 0 and st["queries"] == nq, st
    if st["candidates"] == 0:
        return False
    assert st["candidates"] >= nq * k, st
    return True


def _oracle_threads(oracle_mod, pts, qs, k, threads=12):
    """oracle.brute_knn with the queries spread over a few threads (ctypes drops the GIL)"""
    nq = len(qs)
    idx = np.empty((nq, k), dtype=np.uint64)
    dist = np.empty((nq, k), dtype=pts.dtype)
    step = (nq + threads - 1) // threads

    def work(lo):
        idx[lo:lo + step], dist[lo:lo + step] = oracle_mod.brute_knn(pts, qs[lo:lo + step], k)
    ts = [threading.Thread(target=work, args=(lo,)) for lo in range(0, nq, step)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return idx, dist


def _check_prefix(got, ref, k, where):
    """the oracle's k smallest are the first k of its k_max smallest (one total order: distance, then index)"""
    (gi, gd), (ri, rd) = got, ref
    assert _same_dist(gd, rd[:, :k]), f"distances differ ({where})"
    assert np.array_equal(gi, ri[:, :k]), f"indices differ ({where})"


# ------------------------------------------------- 1-3, 5: few segments; k' through k, through the option, structures
@pytest.fixture(scope="module")
def narrow():
    pts = uniform((9000, 32), 0xA11CE + 9032, np.float32)
    return pts, _queries(pts, 96, 0xB0B + 9000)


@pytest.mark.parametrize("k,kp", [(27, 30), (28, 31), (87, 94), (88, 95), (149, 160), (150, 161), (179, 192), (180, 193)])
def test_kprime_boundaries_through_k(pn, oracle_mod, narrow, k, kp):
    """k' = 30 | 31: LDS -> HBM candidate buffers, 64 -> 128 slots; 94 | 95: 128 -> 256 slots; 160 | 161: the re-rank's
    cells 160 -> 192; 192: the last k' the tier admits; 193: the exact scan answers."""
    pts, qs = narrow
    assert k + 2 + k // 16 == kp
    tree = _check_knn(pn, oracle_mod, pts, qs, k, "mfma")
    assert _served(tree, len(qs), k) == (kp <= 192)


@pytest.mark.parametrize("slots", [30, 31, 94, 95, 192, 193])
def test_kprime_boundaries_through_filter_slots(pn, oracle_mod, narrow, slots):
    from petal_neighbors_amd import _lib
    pts, qs = narrow
    tree = _check_knn(pn, oracle_mod, pts, qs, 10, "mfma", {_lib.PN_OPT_FILTER_SLOTS: slots})
    assert _served(tree, len(qs), 10) == (slots <= 192)


@pytest.mark.parametrize("structure", [2, 3])
@pytest.mark.parametrize("k,slots,kp", [(27, 0, 30), (28, 0, 31), (50, 0, 55), (10, 30, 30), (10, 31, 31), (10, 40, 40)])
def test_kprime_boundaries_on_both_structures(pn, oracle_mod, narrow, structure, k, slots, kp):
    """Structure 3 (HBM candidate buffers) serves every k' here; structure 2 (LDS buffers of 64 slots) holds k' <= 30
    and hands a larger one to the next tier -- an answer, not PN_ERR_UNSUPPORTED."""
    from petal_neighbors_amd import _lib
    pts, qs = narrow
    assert (slots or k + 2 + k // 16) == kp
    tree = _check_knn(pn, oracle_mod, pts, qs, k, "mfma", {_lib.PN_OPT_MFMA_STRUCTURE: structure,
                                                          _lib.PN_OPT_FILTER_SLOTS: slots})
    assert _served(tree, len(qs), k) == (structure == 3 or kp <= 30)


@pytest.mark.parametrize("k,kp", [(27, 30), (28, 31)])
def test_wide_rows_gate(pn, oracle_mod, k, kp):
    """D = 200 (rows padded to 256): the slab-accumulating kernel has LDS candidate buffers only, k' <= 30."""
    pts = uniform((6000, 200), 0xD1CE + 6200, np.float32)
    qs = _queries(pts, 64, 0xFACE + 6000)
    assert k + 2 + k // 16 == kp
    tree = _check_knn(pn, oracle_mod, pts, qs, k, "mfma")
    assert _served(tree, len(qs), k) == (kp <= 30)


# ------------------------------------------------------------------------------------------- 4: 33 segments per query
BIG_N = 66048  # 1032 row tiles: the fewest rows at which a query tile gets its 32 workgroups, i.e. 33 segments


@pytest.fixture(scope="module")
def big(pn, oracle_mod):
    pts = uniform((BIG_N, 16), 0xA11CE + BIG_N + 16, np.float32)
    qs = _queries(pts, 2176, 0xB0B + BIG_N)
    tree = pn.BallTree.euclidean(pts)
    tree.set_engine("mfma")
    return dict(pts=pts, qs=qs, tree=tree, few=oracle_mod.brute_knn(pts, qs[:24], 179),
                many=_oracle_threads(oracle_mod, pts, qs, 160))


@pytest.mark.parametrize("k", [10, 100, 149, 150, 160, 179])
def test_33_segments_one_query_tile(big, k):
    """24 queries against 66 048 rows: 33 (segment, query) cells of up to k' entries meet in the re-rank's LDS.  Up to
    k = 149 (k' = 160) all 33 fit; beyond, the plan gives the query tile fewer workgroups -- the tier still serves."""
    tree, qs = big["tree"], big["qs"][:24]
    tree.stats(reset=True)
    _check_prefix(tree.query_batch(qs, k), big["few"], k, f"k={k}")
    assert _served(tree, len(qs), k)


@pytest.mark.parametrize("nq", [2048, 2176])
@pytest.mark.parametrize("k", [149, 160])
def test_33_segments_all_workgroups(big, nq, k):
    """2 048 queries: every workgroup of the device is in the plan, still 33 segments; 2 176: one fewer per tile."""
    tree, qs = big["tree"], big["qs"][:nq]
    tree.stats(reset=True)
    gi, gd = tree.query_batch(qs, k)
    ri, rd = big["many"]
    _check_prefix((gi, gd), (ri[:nq], rd[:nq]), k, f"nq={nq} k={k}")
    assert _served(tree, nq, k)


# --------------------------------------------------------------------------- 6: the k' rule of many query tiles
def test_many_query_tiles(pn, oracle_mod):
    """11 008 queries = 86 tiles of 128, more than a third of the CUs: k' = k + k // 4 + 4.  k = 21 | 22: k' = 30 | 31;
    150 | 151: 191 | 192; 152: 194, refused."""
    pts = uniform((8192, 8), 0xA11CE + 8192 + 8, np.float32)
    qs = _queries(pts, 11008, 0xB0B + 8192)
    ref = _oracle_threads(oracle_mod, pts, qs, 152)
    tree = pn.BallTree.euclidean(pts)
    tree.set_engine("mfma")
    for k, kp in ((21, 30), (22, 31), (150, 191), (151, 192), (152, 194)):
        assert k + k // 4 + 4 == kp
        tree.stats(reset=True)
        _check_prefix(tree.query_batch(qs, k), ref, k, f"k={k}")
        assert _served(tree, len(qs), k) == (kp <= 192), k


# ----------------------------------------------------------- 7: engine auto once the bf16 tier has turned itself off
def test_auto_engine_after_bf16_tier_stepped_aside(pn, oracle_mod):
    """Tight clusters far apart (test_bf16_hostile_data_falls_back_and_stays_exact's family): bf16 resolves nothing
    inside a cluster, every call leaves all its queries unproven and raises the index's plan level -- the first may
    only retire the seed model -- so that after three the bf16 tier is off and the f32 MFMA tier takes engine auto's
    calls: 66 048 rows and k = 160 put it at 33 segments and k' = 172."""
    import torch
    rng = np.random.default_rng(9)
    cen = (rng.random((8, 16), dtype=np.float32) * 100).astype(np.float32)
    pts = (cen[rng.integers(0, 8, BIG_N)] + 0.01 * rng.standard_normal((BIG_N, 16), dtype=np.float32)).astype(np.float32)
    qs = (pts[rng.integers(0, BIG_N, 128)] + 0.001 * rng.standard_normal((128, 16), dtype=np.float32)).astype(np.float32)
    tree = pn.BallTree.euclidean(pts)
    assert tree.bf16_eligible and tree.mfma_eligible
    ri, rd = oracle_mod.brute_knn(pts, qs, 160)
    for call in range(3):
        tree.stats(reset=True)
        _check_prefix(tree.query_batch(qs, 5), (ri, rd), 5, f"call {call}")
        assert tree.stats()["fallback_queries"] * 16 > len(qs), "this call should have raised the bf16 plan level"
    tree.stats(reset=True)
    _check_prefix(tree.query_batch(qs[:24], 160), (ri[:24], rd[:24]), 160, "host call")
    assert _served(tree, 24, 160)
    stream = torch.cuda.Stream()
    qd = torch.from_numpy(qs[:24]).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        di, dd = tree.query_device(qd, 160)
    stream.synchronize()
    _check_prefix((di.cpu().numpy().astype(np.uint64), dd.cpu().numpy()), (ri[:24], rd[:24]), 160, "device call")
