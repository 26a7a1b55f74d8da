"""CPU-side checks of pn_query_radius_with_distance_* (no GPU compute calls): the symbols are declared, listed in the ctypes
table and exported; bad arguments fail before any device is touched; the Python methods exist and validate their
inputs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["pn_query_radius_with_distance_f32", "pn_query_radius_with_distance_f64",
       "pn_query_radius_with_distance_device_f32", "pn_query_radius_with_distance_device_f64",
       "pn_sharded_query_radius_with_distance_f32", "pn_sharded_query_radius_with_distance_f64",
       "pn_sharded_query_radius_with_distance_device_f32", "pn_sharded_query_radius_with_distance_device_f64"]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    assert re.search(r"#define\s+PN_RADIUS_SORTED\s+1\b", hdr) and _lib.PN_RADIUS_SORTED == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert _lib.lib().pn_abi_version() == 3


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    ct = C.c_float if sfx == "f32" else C.c_double
    q = np.zeros((2, 4), dtype=np.float32 if sfx == "f32" else np.float64)
    off = np.zeros(3, dtype=np.uint64)
    oi, od = C.c_void_p(0), C.c_void_p(0)
    host = getattr(L, f"pn_query_radius_with_distance_{sfx}")
    ok_args = (q.ctypes.data, 2, 4, 4, ct(1.0))
    # NULL outputs, unknown flag bits, NULL index
    assert host(None, *ok_args, 0, off.ctypes.data, C.byref(oi), None) == _lib.PN_ERR_INVALID
    assert host(None, *ok_args, 0, off.ctypes.data, None, C.byref(od)) == _lib.PN_ERR_INVALID
    assert host(None, *ok_args, 0, None, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID
    for flags in (2, 4, 0x80000000):
        assert host(None, *ok_args, flags, off.ctypes.data, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID
        assert "flags" in _lib.last_error()
    assert host(None, *ok_args, 1, off.ctypes.data, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID
    assert "index is NULL" in _lib.last_error()
    dev = getattr(L, f"pn_query_radius_with_distance_device_{sfx}")
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    # d_dist NULL with capacity > 0; d_idx NULL; d_offsets NULL; unknown flags
    assert dev(None, p, 1, 4, 4, ct(1.0), 0, p, p, None, 4, None, None) == _lib.PN_ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert dev(None, p, 1, 4, 4, ct(1.0), 0, p, None, p, 4, None, None) == _lib.PN_ERR_INVALID
    assert dev(None, p, 1, 4, 4, ct(1.0), 0, None, p, p, 4, None, None) == _lib.PN_ERR_INVALID
    assert dev(None, p, 1, 4, 4, ct(1.0), 3, p, p, p, 4, None, None) == _lib.PN_ERR_INVALID
    assert "flags" in _lib.last_error()
    # the sharded entry points: NULL handle / outputs, unknown flags
    sh = getattr(L, f"pn_sharded_query_radius_with_distance_{sfx}")
    assert sh(None, *ok_args, 0, off.ctypes.data, C.byref(oi), None) == _lib.PN_ERR_INVALID
    assert sh(None, *ok_args, 2, off.ctypes.data, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID
    shd = getattr(L, f"pn_sharded_query_radius_with_distance_device_{sfx}")
    assert shd(None, p, 1, 4, 4, ct(1.0), 0, p, p, p, 4, None, None) == _lib.PN_ERR_INVALID
    # capacity 0 needs no buffers: the NULL index is what fails
    assert dev(None, p, 1, 4, 4, ct(1.0), 1, p, None, None, 0, None, None) == _lib.PN_ERR_INVALID
    assert "index is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    for name in ("query_radius_with_distance", "query_radius_with_distance_batch", "query_radius_with_distance_device"):
        assert callable(getattr(bt, name, None)), name
    for name in ("query_radius_with_distance_batch", "query_radius_with_distance_device"):
        assert callable(getattr(pn.ShardedIndex, name, None)), name
    sig = inspect.signature(bt.query_radius_with_distance_device)
    assert list(sig.parameters)[1:] == ["queries", "distance", "capacity", "sort", "out_offsets", "out_idx", "out_dist",
                                        "out_total", "stream"]
    assert inspect.signature(bt.query_radius_with_distance).parameters["sort"].default is False
    # validation that needs no handle: the methods reject bad queries before calling the library
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype = "f32", np.dtype(np.float32)
    with pytest.raises(ValueError):
        fake.query_radius_with_distance(np.zeros((2, 3), np.float32), 1.0)  # a point must be 1-D
    with pytest.raises(ValueError):
        fake.query_radius_with_distance_batch(np.zeros(3, np.float32), 1.0)  # queries must be 2-D
    with pytest.raises(ValueError):
        fake.query_radius_with_distance_device(np.zeros((2, 3), np.float32), 1.0, 4)  # not a CUDA tensor


def test_cpp_mirror_compiles_with_the_new_method(tmp_path):
    src = tmp_path / "wd.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "std::pair<std::vector<size_t>, std::vector<float>> f(const petal::BallTree<float> &t, const float *p) {\n"
                   "    return t.query_radius_with_distance(p, 4, 0.5f, true);\n}\n"
                   "std::pair<std::vector<size_t>, std::vector<double>> g(const petal::BallTree<double> &t, const double *p) {\n"
                   "    return t.query_radius_with_distance(p, 4, 0.5, false);\n}\n"
                   "std::pair<std::vector<size_t>, std::vector<float>> h(const petal::ShardedBallTreeT<float> &t, const float *p) {\n"
                   "    return t.query_radius_with_distance(p, 4, 0.5f, true);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
