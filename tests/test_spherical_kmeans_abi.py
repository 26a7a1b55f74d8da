"""CPU-side checks of pn_spherical_kmeans_* (no GPU compute calls): the eight symbols are declared, listed in the ctypes
table with one entry per C parameter, exported, present in the Rust extern block and (host entries) in the C++ mirror, the
ABI version is still 3; bad arguments fail in pn_kmeans_*'s order before any device is touched; the Python methods exist
and validate."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FAMILIES = ["spherical_kmeans_assign", "spherical_kmeans_assign_device", "spherical_kmeans", "spherical_kmeans_device"]
NAMES = [f"pn_{fam}_{sfx}" for fam in FAMILIES for sfx in ("f32", "f64")]


def test_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "petal_neighbors.hpp")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    assert re.search(r"#define\s+PN_ABI_VERSION\s+3\b", hdr) and _lib.lib().pn_abi_version() == 3
    for name in NAMES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1).split(",")
        # the arguments of the Euclidean sibling, one for one
        twin = re.search(r"\bint\s+" + name.replace("spherical_", "") + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1).split(",")
        assert [" ".join(a.split()) for a in decl] == [" ".join(a.split()) for a in twin], name
        assert name in exported and len(_lib.SIGNATURES[name][1]) == len(decl), name
        n_rust = re.search(r"pub fn " + name + r"\(([^;]*?)\)\s*->\s*c_int;", rust, re.S).group(1).count(":")
        assert n_rust == len(decl), name
        assert "device" in name or name + "(" in hpp, name
    head = hdr[:hdr.index("#define PN_ABI_VERSION")]
    assert "pn_spherical_kmeans_{,device_}{f32,f64}, pn_spherical_kmeans_assign_{,device_}{f32,f64}" in head
    assert "Spherical k-means on Cosine indexes: pn_spherical_kmeans_* below" in hdr


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)(1, 1, 1, 1, 1, 1, 1, 1)
    p = C.addressof(buf)
    for name, extra in ((f"pn_spherical_kmeans_{sfx}", ()), (f"pn_spherical_kmeans_device_{sfx}", (None,))):
        def call(fl, tol, mi, cout, labels, init, nc):
            return getattr(L, name)(None, init, nc, tol, mi, fl, cout, labels, None, None, None, None, None, *extra)
        # each step is wrong in everything that comes later too: the earlier error wins
        for args, word in (((4, -1.0, 0, None, None, None, 0), "flags"), ((0, float("nan"), 0, None, None, None, 0), "tol"),
                           ((0, 0.0, 0, None, None, None, 0), "max_iter"), ((0, 0.0, 1, None, None, None, 0), "labels is NULL"),
                           ((0, 0.0, 1, None, p, None, 0), "centres_out is NULL"), ((0, 0.0, 1, p, p, None, 0), "centres is NULL"),
                           ((0, 0.0, 1, p, p, p, 0), "at least one centre"), ((0, 0.0, 1, p, p, p, 2), "index is NULL")):
            assert call(*args) == _lib.PN_ERR_INVALID and word in _lib.last_error(), word
    for name, extra in ((f"pn_spherical_kmeans_assign_{sfx}", ()), (f"pn_spherical_kmeans_assign_device_{sfx}", (None,))):
        f = getattr(L, name)
        for args, word in (((None, 2, 8, None, None, None), "flags"), ((None, 2, 0, None, p, p), "labels is NULL"),
                           ((None, 2, 0, p, None, None), "centres is NULL"), ((None, 0, 0, p, None, None), "index is NULL")):
            assert f(None, *args, *extra) == _lib.PN_ERR_INVALID and word in _lib.last_error(), word


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    sig = {name: list(inspect.signature(getattr(bt, name)).parameters)[1:] for name in FAMILIES}
    assert sig["spherical_kmeans"][:4] == ["centres_or_k", "tol", "max_iter", "seed"]
    assert sig["spherical_kmeans_assign"] == ["centres"] and sig["spherical_kmeans_assign_device"][0] == "centres"
    assert sig["spherical_kmeans_device"][:3] == ["centres", "abs_tol", "max_iter"]
    assert "default_rng(seed)" in bt.spherical_kmeans.__doc__
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake._dim, fake.device = "f32", np.dtype(np.float32), 10, 4, 0
    fake.points = np.zeros((10, 4), dtype=np.float32)
    c = np.zeros((3, 4), dtype=np.float32)
    calls = (lambda c: fake.spherical_kmeans(c), lambda c: fake.spherical_kmeans_assign(c),
             lambda c: fake.spherical_kmeans_assign_device(c), lambda c: fake.spherical_kmeans_device(c, 0.0))
    fake.metric = pn.distance.Euclidean()  # Cosine trees only
    for call in calls:
        with pytest.raises(ValueError, match="Cosine"):
            call(c)
    fake.metric = pn.distance.Cosine()
    for bad in (np.zeros((3, 3), dtype=np.float32), np.zeros((3, 5), dtype=np.float32), np.zeros(4, dtype=np.float32)):
        for call in calls[:2]:
            with pytest.raises(ValueError):
                call(bad)
    for kw in ({"tol": -1.0}, {"tol": float("nan")}, {"max_iter": 0}):
        with pytest.raises(ValueError):
            fake.spherical_kmeans(c, **kw)
    for k in (0, 11):
        with pytest.raises(ValueError):
            fake.spherical_kmeans(k)
    for call in calls[2:]:  # the device methods take CUDA tensors only
        with pytest.raises(ValueError):
            call(c)
