"""bench.py --dump-outputs without a GPU: dump_outputs() on host arrays shaped like the timed path's answers -- dtypes,
the 64 MB limit, the fixed seeded sample of queries beyond it and the radius mode's CSR rebuilt over that sample."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("pn_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _knn(nq, k, seed=7):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 40, (nq, k), dtype=np.int64), rng.random((nq, k), dtype=np.float32)


def _csr(nq, seed=8):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 40, nq))]).astype(np.uint64)
    return off, rng.integers(0, 1 << 40, int(off[-1]), dtype=np.uint64)


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_answers_are_written_whole(bench, tmp_path):
    idx, dst = _knn(300, 10)
    names = bench.dump_outputs(str(tmp_path), 300, {"indices": idx, "distances": dst})
    assert names == ["distances", "indices"] and sorted(os.listdir(tmp_path)) == ["distances.npy", "indices.npy"]
    gi, gd = np.load(tmp_path / "indices.npy"), np.load(tmp_path / "distances.npy")
    assert gi.dtype == np.float64 and gd.dtype == np.float32
    assert np.array_equal(gi.astype(np.int64), idx) and gd.tobytes() == dst.tobytes()


def test_large_answers_keep_a_fixed_sample_within_the_limit(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    idx, dst = _knn(5000, 10)  # 5000 x 10 x (8 + 4) bytes: 600 kB
    bench.dump_outputs(str(tmp_path / "a"), 5000, {"indices": idx, "distances": dst})
    bench.dump_outputs(str(tmp_path / "b"), 5000, {"indices": idx, "distances": dst})
    assert _size(tmp_path / "a") <= 64 << 10
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    r = rows.astype(np.int64)
    assert rows.dtype == np.float64 and len(r) > 400 and (np.diff(r) > 0).all() and r[-1] < 5000
    assert np.array_equal(np.load(tmp_path / "a" / "indices.npy").astype(np.int64), idx[r])
    assert np.load(tmp_path / "a" / "distances.npy").tobytes() == dst[r].tobytes()
    for f in os.listdir(tmp_path / "a"):  # the same sample from run to run
        assert np.load(tmp_path / "a" / f).tobytes() == np.load(tmp_path / "b" / f).tobytes(), f


@pytest.mark.parametrize("limit", [64 << 20, 32 << 10])
def test_radius_lists(bench, tmp_path, monkeypatch, limit):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    nq = 3000
    off, ids = _csr(nq)
    bench.dump_outputs(str(tmp_path), nq, {}, lists=(off, ids))
    assert _size(tmp_path) <= limit
    go, gids = np.load(tmp_path / "offsets.npy"), np.load(tmp_path / "ids.npy")
    assert go.dtype == gids.dtype == np.float64 and int(go[0]) == 0 and int(go[-1]) == len(gids)
    rows = (np.load(tmp_path / "query_rows.npy").astype(np.int64) if os.path.exists(tmp_path / "query_rows.npy")
            else np.arange(nq))
    assert (len(rows) == nq) == (limit == 64 << 20) and len(go) == len(rows) + 1
    for j, a in enumerate(rows):
        assert np.array_equal(gids[int(go[j]):int(go[j + 1])].astype(np.uint64), ids[int(off[a]):int(off[a + 1])]), a
