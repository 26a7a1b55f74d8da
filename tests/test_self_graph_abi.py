"""CPU-side checks of the self-queries pn_query_self_* / pn_query_radius_self_* (no GPU compute calls): the symbols are
declared, listed in the ctypes table and exported; PN_SELF_INCLUDE is 2; bad flags and NULL arguments fail with
PN_ERR_INVALID before any device is touched; the Python and C++ methods exist."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["pn_query_self_f32", "pn_query_self_f64", "pn_query_self_device_f32", "pn_query_self_device_f64",
       "pn_query_radius_self_f32", "pn_query_radius_self_f64", "pn_query_radius_self_device_f32",
       "pn_query_radius_self_device_f64"]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    assert re.search(r"#define\s+PN_SELF_INCLUDE\s+2\b", hdr) and _lib.PN_SELF_INCLUDE == 2
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert _lib.lib().pn_abi_version() == 3


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_knn_bad_arguments_fail_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_query_self_{sfx}")
    dev = getattr(L, f"pn_query_self_device_{sfx}")
    # unknown flag bits -- PN_RADIUS_SORTED among them on a k-NN call
    for flags in (1, 4, 3, 0x80000000):
        assert host(None, 3, flags, p, p) == _lib.PN_ERR_INVALID
        assert "flags" in _lib.last_error()
        assert dev(None, 3, flags, p, p, None) == _lib.PN_ERR_INVALID
        assert "flags" in _lib.last_error()
    # PN_SELF_INCLUDE is a k-NN flag: the NULL index is what fails
    assert host(None, 3, _lib.PN_SELF_INCLUDE, p, p) == _lib.PN_ERR_INVALID
    assert "index is NULL" in _lib.last_error()
    assert dev(None, 3, 0, p, p, None) == _lib.PN_ERR_INVALID
    assert "index is NULL" in _lib.last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_radius_bad_arguments_fail_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    ct = C.c_float if sfx == "f32" else C.c_double
    off = np.zeros(3, dtype=np.uint64)
    oi, od = C.c_void_p(0), C.c_void_p(0)
    host = getattr(L, f"pn_query_radius_self_{sfx}")
    assert host(None, ct(1.0), 0, None, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID  # NULL offsets
    assert host(None, ct(1.0), 0, off.ctypes.data, None, C.byref(od)) == _lib.PN_ERR_INVALID  # NULL idx_out
    assert "NULL" in _lib.last_error()
    for flags in (4, 8, 0x80000000):
        assert host(None, ct(1.0), flags, off.ctypes.data, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID
        assert "flags" in _lib.last_error()
    # sorted lists need their distances
    assert host(None, ct(1.0), _lib.PN_RADIUS_SORTED, off.ctypes.data, C.byref(oi), None) == _lib.PN_ERR_INVALID
    assert "PN_RADIUS_SORTED" in _lib.last_error()
    # every valid flag combination reaches the handle check (distances optional without PN_RADIUS_SORTED)
    for flags in (0, 1, 2, 3):
        assert host(None, ct(1.0), flags, off.ctypes.data, C.byref(oi), C.byref(od)) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
    assert host(None, ct(1.0), 2, off.ctypes.data, C.byref(oi), None) == _lib.PN_ERR_INVALID
    assert "index is NULL" in _lib.last_error()
    dev = getattr(L, f"pn_query_radius_self_device_{sfx}")
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    assert dev(None, ct(1.0), 0, None, p, p, 4, None, None) == _lib.PN_ERR_INVALID  # NULL offsets
    assert dev(None, ct(1.0), 0, p, None, p, 4, None, None) == _lib.PN_ERR_INVALID  # NULL d_idx, capacity > 0
    assert "NULL" in _lib.last_error()
    assert dev(None, ct(1.0), 1, p, p, None, 4, None, None) == _lib.PN_ERR_INVALID  # sorted without distances
    assert "PN_RADIUS_SORTED" in _lib.last_error()
    assert dev(None, ct(1.0), 4, p, p, p, 4, None, None) == _lib.PN_ERR_INVALID
    assert "flags" in _lib.last_error()
    # capacity 0 only counts: no list buffers needed, the NULL index is what fails
    assert dev(None, ct(1.0), 3, p, None, None, 0, None, None) == _lib.PN_ERR_INVALID
    assert "index is NULL" in _lib.last_error()
    assert dev(None, ct(1.0), 0, p, p, None, 4, None, None) == _lib.PN_ERR_INVALID
    assert "index is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    for name in ("query_self", "query_self_device", "query_radius_self", "query_radius_self_device"):
        assert callable(getattr(bt, name, None)), name
    assert list(inspect.signature(bt.query_self).parameters)[1:] == ["k", "include_self"]
    assert list(inspect.signature(bt.query_self_device).parameters)[1:] == ["k", "include_self", "out_idx", "out_dist",
                                                                             "stream"]
    assert list(inspect.signature(bt.query_radius_self).parameters)[1:] == ["r", "with_distance", "sort", "include_self"]
    sig = inspect.signature(bt.query_radius_self_device)
    assert list(sig.parameters)[1:4] == ["r", "capacity", "with_distance"]
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n = "f32", np.dtype(np.float32), 10
    with pytest.raises(ValueError):
        fake.query_self(-1)
    with pytest.raises(ValueError):
        fake.query_radius_self(1.0, sort=True)  # sorted lists need distances
    with pytest.raises(ValueError):
        fake.query_radius_self_device(1.0, -1)


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "sg.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "std::pair<std::vector<size_t>, std::vector<float>> f(const petal::BallTree<float> &t) {\n"
                   "    return t.query_self(10, false);\n}\n"
                   "petal::SelfRadius<double> g(const petal::BallTree<double> &t) {\n"
                   "    return t.query_radius_self(0.5, true, true, false);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
