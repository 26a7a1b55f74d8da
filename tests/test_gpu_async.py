"""The *_device entry points are asynchronous (include/petal_mi355x.h, "Asynchronous device API"): a call enqueues its
work on the caller's stream and returns -- no hipStreamSynchronize, no read-back of the unproven-query count (round 1
had one).  Observable from outside: put something slow on the stream first; the call must come back while that is
still running, and the answers must still be the oracle's once the stream has drained."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _busy(torch, stream, ms_target=150.0):
    """enqueue roughly ms_target of matrix products on `stream`; returns an event recorded behind them"""
    a = torch.rand((4096, 4096), device="cuda")
    b = torch.rand((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        c = a @ b
    torch.cuda.synchronize()
    one = max((time.perf_counter() - t0) * 1e3, 0.05)
    reps = int(min(max(ms_target / one, 8), 4000))
    with torch.cuda.stream(stream):
        for _ in range(reps):
            c = a @ b
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev, c


@pytest.mark.parametrize("engine", ["auto", "exact"])
def test_query_device_returns_before_its_stream_has_drained(pn, oracle_mod, engine):
    import torch
    rng = np.random.default_rng(5)
    pts = rng.random((60000, 64), dtype=np.float32)
    qs = rng.random((700, 64), dtype=np.float32)
    qs[3] = pts[17]          # an exact hit
    qs[5, 0] = np.nan        # a query only the second tier can answer: the call must not wait to learn that
    tree = pn.BallTree.euclidean(pts)
    tree.set_engine(engine)
    dq = torch.from_numpy(qs).cuda()
    tree.query_device(dq, 10)            # warm-up: workspaces, plans
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ev, keep = _busy(torch, stream)
    assert not ev.query(), "the stream drained before the test could look (box too fast for the filler)"
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        idx, dist = tree.query_device(dq, 10)
    dt = (time.perf_counter() - t0) * 1e3
    still_busy = not ev.query()
    assert still_busy, f"pn_query_device_f32 came back only after the work queued in front of it had finished ({dt:.1f} ms)"
    assert dt < 50.0, f"enqueueing took {dt:.1f} ms"
    stream.synchronize()
    oidx, odist = oracle_mod.brute_knn(pts, qs, 10)
    assert dist.cpu().numpy().tobytes() == odist.tobytes()
    assert np.array_equal(idx.cpu().numpy().astype(np.uint64), oidx)
    del keep


def test_sharded_query_device_is_asynchronous_too(pn, oracle_mod):
    import torch
    rng = np.random.default_rng(6)
    pts = rng.random((50000, 32), dtype=np.float32)
    qs = rng.random((513, 32), dtype=np.float32)
    sh = pn.ShardedIndex.from_host(pts, devices=[0, 0, 0])     # three virtual shards: local merge, no exchange
    dq = torch.from_numpy(qs).cuda()
    sh.query_device(dq, 7)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ev, keep = _busy(torch, stream)
    assert not ev.query()
    with torch.cuda.stream(stream):
        idx, dist = sh.query_device(dq, 7)
    assert not ev.query(), "pn_sharded_query_device_f32 waited for its stream"
    stream.synchronize()
    oidx, odist = oracle_mod.brute_knn(pts, qs, 7)
    assert dist.cpu().numpy().tobytes() == odist.tobytes()
    assert np.array_equal(idx.cpu().numpy().astype(np.uint64), oidx)
    del keep


# The two tests below call with LARGER shapes than their warm-up, so the workspace's buffers are outgrown behind the
# filler: an outgrown allocation must be retired to the workspace's list (DevBuf::ensure), never freed on the spot --
# hipFree waits for the whole device, filler included.  Every workspace buffer gets that list by being a member of
# WorkspaceBufs (index.hip).
def _grow_corpus():
    return np.random.default_rng(7).random((20000, 32), dtype=np.float32)


def test_query_device_outgrows_its_buffers_without_waiting(pn, oracle_mod):
    import torch
    pts = _grow_corpus()
    qs = np.random.default_rng(8).random((2048, 32), dtype=np.float32)
    tree = pn.BallTree.euclidean(pts)
    dq = torch.from_numpy(qs).cuda()
    tree.query_device(dq[:64], 5)        # warm-up: every query-sized buffer at 64 queries, k = 5
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ev, keep = _busy(torch, stream)
    assert not ev.query(), "the stream drained before the test could look (box too fast for the filler)"
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        idx, dist = tree.query_device(dq, 10)
    dt = (time.perf_counter() - t0) * 1e3
    still_busy = not ev.query()
    assert still_busy, f"pn_query_device_f32 waited for the device when its buffers grew ({dt:.1f} ms)"
    assert dt < 50.0, f"enqueueing took {dt:.1f} ms"
    stream.synchronize()
    oidx, odist = oracle_mod.brute_knn(pts, qs, 10)
    assert dist.cpu().numpy().tobytes() == odist.tobytes()
    assert np.array_equal(idx.cpu().numpy().astype(np.uint64), oidx)
    del keep


def test_lof_device_outgrows_its_graph_store_without_waiting(pn):
    import torch
    pts = _grow_corpus()
    tree = pn.BallTree.euclidean(pts)
    tree.lof_device(3)                   # warm-up: the graph store (w_lof) at k = 3
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ev, keep = _busy(torch, stream)
    assert not ev.query(), "the stream drained before the test could look (box too fast for the filler)"
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        lof, _, _ = tree.lof_device(20)
    dt = (time.perf_counter() - t0) * 1e3
    still_busy = not ev.query()
    assert still_busy, f"pn_lof_device_f32 waited for the device when its graph store grew ({dt:.1f} ms)"
    assert dt < 50.0, f"enqueueing took {dt:.1f} ms"
    stream.synchronize()
    want = pn.BallTree.euclidean(pts).lof(20)    # the host entry on a fresh handle
    assert lof.cpu().numpy().tobytes() == want.tobytes()
    del keep


# pn_kmeans_assign_device_* "never waits" (the header): with the filter forced its whole chain -- packing, the MFMA
# filter, re-rank and proof, the exact kernel over the listed rows, the inertia -- is enqueued behind the filler, the
# count of listed rows staying on the device.
def _kmeans_assign_behind_the_filler(pn, warm_nc, nc, what):
    import torch
    import kmeans_reference as ref
    from petal_neighbors_amd import _lib
    pts = _grow_corpus()
    cs = np.random.default_rng(9).random((max(warm_nc, nc), 32), dtype=np.float32)
    cs[0] = cs[1] = pts[17]              # twins on a row: a row the proof must refuse, so the list is not empty
    tree = pn.BallTree.euclidean(pts)
    tree.set_option(_lib.PN_OPT_KMEANS_FILTER, 1)
    dc = torch.from_numpy(cs).cuda()
    tree.kmeans_assign_device(dc[:warm_nc].contiguous())     # warm-up: the row image, the centre image at warm_nc
    torch.cuda.synchronize()
    centres = dc[:nc].contiguous()
    stream = torch.cuda.Stream()
    ev, keep = _busy(torch, stream)
    assert not ev.query(), "the stream drained before the test could look (box too fast for the filler)"
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        labels, dist, inertia = tree.kmeans_assign_device(centres)
    dt = (time.perf_counter() - t0) * 1e3
    still_busy = not ev.query()
    assert still_busy, f"pn_kmeans_assign_device_f32 {what} ({dt:.1f} ms)"
    assert dt < 50.0, f"enqueueing took {dt:.1f} ms"
    stream.synchronize()
    wl, wd = ref.assign(pts, cs[:nc])
    assert np.array_equal(labels.cpu().numpy(), wl)
    assert dist.cpu().numpy().tobytes() == wd.tobytes()
    assert inertia.cpu().numpy()[0].tobytes() == np.float64(ref.inertia(wl, wd)).tobytes()
    assert wl[17] == 0 and wd[17] == 0 and tree.stats()["fallback_queries"] >= 1
    del keep


def test_kmeans_assign_device_returns_before_its_stream_has_drained(pn):
    _kmeans_assign_behind_the_filler(pn, 40, 40, "came back only after the work queued in front of it had finished")


def test_kmeans_assign_device_outgrows_its_centre_image_without_waiting(pn):
    _kmeans_assign_behind_the_filler(pn, 2, 300, "waited for the device when its centre image grew")
