"""CPU-side checks of pn_kmeans_nearest_* (no GPU compute calls): the four symbols are declared, listed in the ctypes table
with one entry per C parameter, exported, present in the Rust extern block and (the host pair) in the C++ mirror; the ABI
version is still 3; bad arguments fail in the documented order -- flags, m, labels, centres, index -- before any device is
touched; the Python methods exist and validate."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = [f"pn_kmeans_nearest_{dev}{sfx}" for dev in ("", "device_") for sfx in ("f32", "f64")]


def test_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "petal_neighbors.hpp")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    for name in NAMES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1).split(",")
        assert len(decl) == (8 if "device" in name else 7), name
        assert len(_lib.SIGNATURES[name][1]) == len(decl) and name in exported, name
        n_rust = re.search(r"pub fn " + name + r"\(([^;]*?)\)\s*->\s*c_int;", rust, re.S).group(1).count(":")
        assert n_rust == len(decl), name
        assert ("device" in name) or name + "(" in hpp, name
    assert re.search(r"#define\s+PN_ABI_VERSION\s+3\b", hdr) and _lib.lib().pn_abi_version() == 3
    assert re.search(r"#define\s+PN_KMEANS_NEAREST_MAX\s+8\b", hdr) and _lib.PN_KMEANS_NEAREST_MAX == 8
    assert "pn_kmeans_nearest_{,device_}{f32,f64}" in hdr[:hdr.index("#define PN_ABI_VERSION")]


@pytest.mark.parametrize("name", NAMES)
def test_bad_arguments_fail_in_order_before_the_device(pn, name):
    from petal_neighbors_amd import _lib
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    extra = (None,) if "device" in name else ()

    def call(centres, nc, m, flags, labels):
        return getattr(_lib.lib(), name)(None, centres, nc, m, flags, labels, None, *extra)

    for args, phrase in (((None, 2, 0, 4, None), "flags"),          # flags first, whatever else is wrong
                         ((None, 2, 0, 0, None), "m must be"),      # m == 0
                         ((None, 2, 9, 0, None), "m must be"),      # m > 8
                         ((None, 2, 8, 0, None), "labels is NULL"),
                         ((None, 2, 1, 0, p), "centres is NULL"),
                         ((p, 2, 3, 0, p), "index is NULL"),
                         ((None, 0, 1, 0, p), "index is NULL")):    # (no centres: the input may be NULL)
        assert call(*args) == _lib.PN_ERR_INVALID and phrase in _lib.last_error(), (args, _lib.last_error())


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    assert list(inspect.signature(bt.kmeans_nearest).parameters)[1:] == ["centres", "m"]
    assert list(inspect.signature(bt.kmeans_nearest_device).parameters)[1:] == ["centres", "m", "out_labels", "out_dist",
                                                                                "stream"]
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake._dim, fake.device = "f32", np.dtype(np.float32), 10, 4, 0
    fake.metric = pn.distance.Euclidean()
    c = np.zeros((3, 4), dtype=np.float32)
    for bad in (np.zeros((3, 3), dtype=np.float32), np.zeros((3, 5), dtype=np.float32), np.zeros(4, dtype=np.float32)):
        with pytest.raises(ValueError):
            fake.kmeans_nearest(bad, 2)
    for m in (0, 9, -1):
        with pytest.raises(ValueError):
            fake.kmeans_nearest(c, m)
    with pytest.raises(ValueError):  # the device method takes CUDA tensors only
        fake.kmeans_nearest_device(c, 2)
    fake.metric = pn.distance.Cosine()
    with pytest.raises(ValueError):
        fake.kmeans_nearest(c, 2)
