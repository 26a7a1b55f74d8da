"""CPU-side checks of the sharded self-queries pn_sharded_query_self_* / pn_sharded_query_radius_self_* (no GPU compute
calls): the symbols are declared, listed in the ctypes table and exported; bad flags and NULL arguments fail with
PN_ERR_INVALID before any device is touched; the Python and C++ methods exist and validate their arguments."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["pn_sharded_query_self_f32", "pn_sharded_query_self_f64", "pn_sharded_query_self_device_f32",
       "pn_sharded_query_self_device_f64", "pn_sharded_query_radius_self_f32", "pn_sharded_query_radius_self_f64",
       "pn_sharded_query_radius_self_device_f32", "pn_sharded_query_radius_self_device_f64"]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    note = hdr[hdr.index("Additive within version 3"):hdr.index("#define PN_ABI_VERSION")]
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert "pn_sharded_query_self_" in note and "pn_sharded_query_radius_self_" in note
    assert "Not for row-sharded handles" not in hdr
    assert _lib.lib().pn_abi_version() == 3


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_knn_bad_arguments_fail_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_sharded_query_self_{sfx}")
    dev = getattr(L, f"pn_sharded_query_self_device_{sfx}")
    # unknown flag bits -- PN_RADIUS_SORTED among them on a k-NN call
    for flags in (_lib.PN_RADIUS_SORTED, 4, 3, 0x80000000):
        assert host(None, 3, flags, p, p) == _lib.PN_ERR_INVALID
        assert "flags" in _lib.last_error()
        assert dev(None, 3, flags, p, p, None) == _lib.PN_ERR_INVALID
        assert "flags" in _lib.last_error()
    for flags in (0, _lib.PN_SELF_INCLUDE):
        assert host(None, 3, flags, p, p) == _lib.PN_ERR_INVALID
        assert "handle is NULL" in _lib.last_error()
        assert dev(None, 3, flags, p, p, None) == _lib.PN_ERR_INVALID
        assert "handle is NULL" in _lib.last_error()
    assert host(None, 3, 0, None, p) == _lib.PN_ERR_INVALID
    assert dev(None, 3, 0, p, None, None) == _lib.PN_ERR_INVALID


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_radius_bad_arguments_fail_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    ct = C.c_float if sfx == "f32" else C.c_double
    off = np.zeros(3, dtype=np.uint64)
    oi, od = C.c_void_p(0), C.c_void_p(0)
    host = getattr(L, f"pn_sharded_query_radius_self_{sfx}")
    assert host(None, ct(1.0), 0, None, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID  # NULL offsets
    assert "NULL" in _lib.last_error()
    assert host(None, ct(1.0), 0, off.ctypes.data, None, C.byref(od)) == _lib.PN_ERR_INVALID  # NULL idx_out
    assert "NULL" in _lib.last_error()
    for flags in (4, 8, 0x80000000):
        assert host(None, ct(1.0), flags, off.ctypes.data, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID
        assert "flags" in _lib.last_error()
    assert host(None, ct(1.0), _lib.PN_RADIUS_SORTED, off.ctypes.data, C.byref(oi), None) == _lib.PN_ERR_INVALID
    assert "PN_RADIUS_SORTED" in _lib.last_error()
    for flags in (0, 1, 2, 3):  # every valid combination reaches the handle check
        assert host(None, ct(1.0), flags, off.ctypes.data, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID
        assert "handle is NULL" in _lib.last_error()
    assert host(None, ct(1.0), _lib.PN_SELF_INCLUDE, off.ctypes.data, C.byref(oi), None) == _lib.PN_ERR_INVALID
    assert "handle is NULL" in _lib.last_error()
    dev = getattr(L, f"pn_sharded_query_radius_self_device_{sfx}")
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    assert dev(None, ct(1.0), 0, None, p, p, 4, None, None) == _lib.PN_ERR_INVALID  # NULL offsets
    assert dev(None, ct(1.0), 0, p, None, p, 4, None, None) == _lib.PN_ERR_INVALID  # NULL d_idx, capacity > 0
    assert "NULL" in _lib.last_error()
    assert dev(None, ct(1.0), 1, p, p, None, 4, None, None) == _lib.PN_ERR_INVALID  # sorted without distances
    assert "PN_RADIUS_SORTED" in _lib.last_error()
    assert dev(None, ct(1.0), 4, p, p, p, 4, None, None) == _lib.PN_ERR_INVALID
    assert "flags" in _lib.last_error()
    assert dev(None, ct(1.0), 3, p, None, None, 0, None, None) == _lib.PN_ERR_INVALID  # a count needs no lists
    assert "handle is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    from petal_neighbors_amd.sharded import ShardedIndex
    for name in ("query_self", "query_self_device", "query_radius_self", "query_radius_self_device"):
        assert callable(getattr(ShardedIndex, name, None)), name
        # the names and arguments of the BallTree methods
        assert (list(inspect.signature(getattr(ShardedIndex, name)).parameters)
                == list(inspect.signature(getattr(pn.BallTree, name)).parameters)), name
    fake = ShardedIndex.__new__(ShardedIndex)
    fake._h, fake._sfx, fake.dtype, fake.n, fake.local_rows, fake.device = None, "f32", np.dtype(np.float32), 10, 10, None
    with pytest.raises(ValueError):
        fake.query_self(-1)
    with pytest.raises(ValueError):
        fake.query_radius_self(1.0, sort=True)  # sorted lists need distances
    with pytest.raises(ValueError):
        fake.query_radius_self_device(1.0, -1)
    with pytest.raises(ValueError):
        fake.query_self_device(3)  # no single GPU behind the handle


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "ssg.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "std::pair<std::vector<size_t>, std::vector<float>> f(const petal::ShardedBallTreeT<float> &t) {\n"
                   "    return t.query_self(10, false);\n}\n"
                   "petal::SelfRadius<double> g(const petal::ShardedBallTreeT<double> &t) {\n"
                   "    return t.query_radius_self(0.5, true, true, false);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
