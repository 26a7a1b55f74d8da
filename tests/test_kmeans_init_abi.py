"""CPU-side checks of pn_kmeans_init_* (no GPU compute calls): the four symbols are in the ctypes table with one entry per C
parameter, exported, and present in the Rust extern block and the C++ mirror; bad arguments fail in the documented order --
flags, trials, centres_out, nc, the index -- before any device is touched; the Python methods exist and validate."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = [f"pn_kmeans_init_{dev}{sfx}" for dev in ("", "device_") for sfx in ("f32", "f64")]


def test_symbols_listed_with_one_entry_per_parameter(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "petal_neighbors.hpp")).read()
    L = _lib.lib()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m and name in _lib.SIGNATURES and hasattr(L, name), name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == (8 if "device" in name else 7), name
        assert f"pub fn {name}(" in rust, name
        assert "device" in name or name + "(" in hpp, name
    assert L.pn_abi_version() == 3


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for name, extra in ((f"pn_kmeans_init_{sfx}", ()), (f"pn_kmeans_init_device_{sfx}", (None,))):
        def call(flags, trials, centres, nc, f=getattr(L, name), extra=extra):
            return f(None, nc, trials, 0, flags, centres, None, *extra)
        steps = [((1, 17, None, 0), "flags"), ((0, 17, None, 0), "trials"), ((0, 16, None, 0), "centres_out is NULL"),
                 ((0, 0, p, 0), "at least one centre"), ((0, 1, p, 1), "index is NULL")]
        for args, phrase in steps:
            assert call(*args) == _lib.PN_ERR_INVALID, (name, args)
            assert phrase in _lib.last_error(), (name, args, _lib.last_error())


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    sig = {name: list(inspect.signature(getattr(bt, name)).parameters)[1:]
           for name in ("kmeans_init", "kmeans_init_device", "kmeans")}
    assert sig["kmeans_init"] == ["k", "seed", "trials"]
    assert sig["kmeans_init_device"] == ["k", "seed", "trials", "out_centres", "out_rows", "stream"]
    assert sig["kmeans"][-1] == "init" and inspect.signature(bt.kmeans).parameters["init"].default == "torch"
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake._dim, fake.device = "f32", np.dtype(np.float32), 10, 4, 0
    fake.metric = pn.distance.Euclidean()
    bad = [lambda: fake.kmeans_init(0), lambda: fake.kmeans_init(11), lambda: fake.kmeans_init(3, trials=17),
           lambda: fake.kmeans_init(3, trials=-1), lambda: fake.kmeans_init(3, seed=-1), lambda: fake.kmeans_init(3, seed=2 ** 64),
           lambda: fake.kmeans_init_device(11), lambda: fake.kmeans(3, init="host")]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    fake.metric = pn.distance.Cosine()
    for call in (lambda: fake.kmeans_init(3), lambda: fake.kmeans_init_device(3)):
        with pytest.raises(ValueError):
            call()
