"""CPU-side checks of pn_query_radii_{,device_,self_,self_device_}{f32,f64} -- one radius per query -- without a GPU
compute call: the symbols are declared, listed in the ctypes table and exported; bad arguments fail before any device is
touched; the Python methods take arrays and validate them; the C++ overloads compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = [f"pn_query_radii_{mid}{sfx}" for mid in ("", "device_", "self_", "self_device_") for sfx in ("f32", "f64")]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    assert len(NEW) == 8
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert re.search(r"#define\s+PN_ABI_VERSION\s+3\b", hdr)
    assert _lib.lib().pn_abi_version() == 3  # additive: callers detect the entry points by symbol


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    INV = _lib.PN_ERR_INVALID
    dt = np.float32 if sfx == "f32" else np.float64
    q = np.zeros((2, 4), dtype=dt)
    rad = np.ones(2, dtype=dt)
    off = np.zeros(3, dtype=np.uint64)
    oi, od = C.c_void_p(0), C.c_void_p(0)
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)  # stands for any non-NULL device pointer: nothing may look at it
    SORTED, INCLUDE = _lib.PN_RADIUS_SORTED, _lib.PN_SELF_INCLUDE

    host = getattr(L, f"pn_query_radii_{sfx}")
    qa = (q.ctypes.data, 2, 4, 4)
    # NULL radii with nq > 0 (every other argument in order, the handle apart: the radii are what is reported)
    assert host(None, *qa, None, 0, off.ctypes.data, C.byref(oi), C.byref(od)) == INV
    assert "radii" in _lib.last_error()
    # NULL outputs (the distance output alone may be NULL)
    assert host(None, *qa, rad.ctypes.data, 0, None, C.byref(oi), C.byref(od)) == INV
    assert host(None, *qa, rad.ctypes.data, 0, off.ctypes.data, None, C.byref(od)) == INV
    assert "NULL" in _lib.last_error()
    # unknown flag bits; PN_SELF_INCLUDE belongs to the self entry points
    for flags in (INCLUDE, 4, 0x80000000, SORTED | INCLUDE):
        assert host(None, *qa, rad.ctypes.data, flags, off.ctypes.data, C.byref(oi), C.byref(od)) == INV
        assert "flags" in _lib.last_error()
    # PN_RADIUS_SORTED without a distance output
    assert host(None, *qa, rad.ctypes.data, SORTED, off.ctypes.data, C.byref(oi), None) == INV
    assert "PN_RADIUS_SORTED" in _lib.last_error()
    # everything in order but the index
    for do in (C.byref(od), None):
        assert host(None, *qa, rad.ctypes.data, 0, off.ctypes.data, C.byref(oi), do) == INV
        assert "index is NULL" in _lib.last_error()

    dev = getattr(L, f"pn_query_radii_device_{sfx}")
    da = (p, 2, 4, 4)
    assert dev(None, *da, None, 0, p, p, p, 4, None, None) == INV
    assert "radii" in _lib.last_error()
    assert dev(None, *da, p, 0, None, p, p, 4, None, None) == INV       # d_offsets
    assert dev(None, *da, p, 0, p, None, p, 4, None, None) == INV       # capacity > 0 with a NULL d_idx
    assert "NULL" in _lib.last_error() and "index" not in _lib.last_error()
    assert dev(None, *da, p, SORTED, p, p, None, 4, None, None) == INV  # sorted lists need the distances
    assert "PN_RADIUS_SORTED" in _lib.last_error()
    for flags in (INCLUDE, 8):
        assert dev(None, *da, p, flags, p, p, p, 4, None, None) == INV
        assert "flags" in _lib.last_error()
    # capacity 0 needs no list buffers, and distances are optional: the NULL index is what fails
    assert dev(None, *da, p, SORTED, p, None, None, 0, None, None) == INV
    assert "index is NULL" in _lib.last_error()
    assert dev(None, *da, p, 0, p, p, None, 4, None, None) == INV
    assert "index is NULL" in _lib.last_error()

    sh = getattr(L, f"pn_query_radii_self_{sfx}")
    assert sh(None, None, 0, off.ctypes.data, C.byref(oi), C.byref(od)) == INV
    assert "radii" in _lib.last_error()
    assert sh(None, rad.ctypes.data, 0, None, C.byref(oi), C.byref(od)) == INV
    assert sh(None, rad.ctypes.data, 0, off.ctypes.data, None, C.byref(od)) == INV
    assert sh(None, rad.ctypes.data, 4, off.ctypes.data, C.byref(oi), C.byref(od)) == INV
    assert "flags" in _lib.last_error()
    assert sh(None, rad.ctypes.data, SORTED, off.ctypes.data, C.byref(oi), None) == INV
    assert "PN_RADIUS_SORTED" in _lib.last_error()
    assert sh(None, rad.ctypes.data, SORTED | INCLUDE, off.ctypes.data, C.byref(oi), C.byref(od)) == INV  # (valid flags)
    assert "index is NULL" in _lib.last_error()

    shd = getattr(L, f"pn_query_radii_self_device_{sfx}")
    assert shd(None, None, 0, p, p, p, 4, None, None) == INV
    assert "radii" in _lib.last_error()
    assert shd(None, p, 0, None, p, p, 4, None, None) == INV
    assert shd(None, p, 0, p, None, p, 4, None, None) == INV
    assert "NULL" in _lib.last_error() and "index" not in _lib.last_error()
    assert shd(None, p, 16, p, p, p, 4, None, None) == INV
    assert "flags" in _lib.last_error()
    assert shd(None, p, SORTED, p, p, None, 4, None, None) == INV
    assert "PN_RADIUS_SORTED" in _lib.last_error()
    assert shd(None, p, INCLUDE, p, None, None, 0, None, None) == INV
    assert "index is NULL" in _lib.last_error()


def test_python_methods_take_arrays_and_validate_them(pn):
    """on an instance without a handle: a bad array raises before the library is called (a call would crash on the
    missing handle), a scalar is not looked at by the array checks"""
    bt = pn.BallTree
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake._dim, fake.device = "f32", np.dtype(np.float32), 5, 3, 0
    qs = np.zeros((4, 3), np.float32)
    assert fake._radii(0.5, 4) is None and fake._radii(np.float32(0.5), 4) is None and fake._radii(np.array(0.5), 4) is None
    ok = fake._radii([0.1, 0.2, 0.3, 0.4], 4)
    assert ok.dtype == np.float32 and ok.shape == (4,) and ok.flags.c_contiguous
    assert fake._radii(np.ones(8, np.float32)[::2], 4).flags.c_contiguous
    for method in (fake.query_radius_batch, fake.query_radius_with_distance_batch):
        with pytest.raises(ValueError):
            method(qs, np.ones(3, np.float32))        # length
        with pytest.raises(ValueError):
            method(qs, np.ones((4, 1), np.float32))   # rank
        with pytest.raises(ValueError):
            method(qs, np.ones(4, np.float64))        # dtype
        with pytest.raises(ValueError):
            method(qs, np.ones(4, np.int32))
    for bad in (np.ones(4, np.float32), np.ones((5, 1), np.float32), np.ones(5, np.float64)):
        with pytest.raises(ValueError):
            fake.query_radius_self(bad)
    with pytest.raises(ValueError):
        fake.query_radius_self(np.ones(5, np.float32), sort=True)  # sorted lists need distances
    # device methods: the radii are a CUDA tensor of the tree's element type
    # (the check itself: a device method rejects host queries before it looks at the radii; CUDA tensors of a wrong
    # length, rank, dtype, device or stride are tried on the GPU, tests/test_gpu_radii.py)
    import torch
    assert fake._radii_device(0.5, 4, None) is None and fake._radii_device(np.float32(0.5), 4, None) is None
    assert fake._radii_device(torch.tensor(0.5), 4, None) is None  # a 0-d tensor is a scalar, as it was before
    for bad in (np.ones(4, np.float32), torch.ones(4, dtype=torch.float32), [0.1, 0.2, 0.3, 0.4]):
        with pytest.raises(ValueError):
            fake._radii_device(bad, 4, torch.device("cpu"))  # not a CUDA tensor
    f64 = bt.__new__(bt)
    f64._sfx, f64.dtype, f64._n = "f64", np.dtype(np.float64), 5
    with pytest.raises(ValueError):
        f64.query_radius_batch(np.zeros((4, 3)), np.ones(4, np.float32))
    assert f64._radii(np.ones(5), 5).dtype == np.float64


def test_cpp_overloads_compile(tmp_path):
    src = tmp_path / "radii.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "petal::SelfRadius<float> f(const petal::BallTree<float> &t, const float *q, const float *r) {\n"
                   "    petal::SelfRadius<float> a = t.query_radius_self(r, true, true, false);\n"
                   "    petal::SelfRadius<float> b = t.query_radius_self(0.5f, true, true, false);\n"
                   "    b = t.query_radius_self(0, true, true, false);  // a literal 0 is still the scalar radius\n"
                   "    a.idx.insert(a.idx.end(), b.idx.begin(), b.idx.end());\n"
                   "    return a.idx.empty() ? t.query_radii(q, 3, 4, r, true, true) : a;\n}\n"
                   "petal::SelfRadius<double> g(const petal::BallTree<double, petal::distance::Cosine> &t, const double *q,\n"
                   "                            const double *r) {\n"
                   "    petal::SelfRadius<double> a = t.query_radius_self(r, false, false, true);\n"
                   "    return a.idx.empty() ? t.query_radii(q, 3, 4, r, false, false) : a;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
