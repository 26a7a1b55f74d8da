"""CPU-side checks of pn_silhouette_* (no GPU compute calls): the four symbols are in the ctypes table with one entry per C
parameter and exported; bad arguments fail in the documented order -- flags, samples_out, codes, n_clusters, rows / n_rows,
the index -- before any device is touched; the Python methods exist and validate."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = [f"pn_silhouette_{dev}{sfx}" for dev in ("", "device_") for sfx in ("f32", "f64")]


def test_symbols_listed_with_one_entry_per_parameter(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    L = _lib.lib()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m and name in _lib.SIGNATURES and hasattr(L, name), name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == (14 if "device" in name else 12), name
    assert L.pn_abi_version() == 3


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for name, extra in ((f"pn_silhouette_{sfx}", ()), (f"pn_silhouette_device_{sfx}", (None, None))):
        def call(flags, samples, codes, nc, rows, n_rows, f=getattr(L, name), extra=extra):
            return f(None, codes, nc, rows, n_rows, flags, samples, None, None, None, None, None, *extra)
        steps = [((1, None, None, 0, None, 3), "flags"), ((0x80000000, None, None, 0, p, 0), "flags"),
                 ((0, None, None, 0, None, 3), "samples_out is NULL"), ((0, p, None, 0, None, 3), "codes is NULL"),
                 ((0, p, p, 0, None, 3), "n_clusters"), ((0, p, p, 1, p, 0), "n_clusters"),
                 ((0, p, p, 2, None, 3), "rows and n_rows"), ((0, p, p, 2, p, 0), "rows and n_rows"),
                 ((0, p, p, 2, None, 0), "index is NULL"), ((0, p, p, 2 ** 40, p, 2), "index is NULL")]
        for args, phrase in steps:
            assert call(*args) == _lib.PN_ERR_INVALID, (name, args)
            assert phrase in _lib.last_error(), (name, args, _lib.last_error())


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    sig = {name: list(inspect.signature(getattr(bt, name)).parameters)[1:]
           for name in ("silhouette_samples", "silhouette_score", "silhouette_device")}
    assert sig["silhouette_samples"] == ["labels", "rows", "ignore", "full"]
    assert sig["silhouette_score"] == ["labels", "rows", "ignore"]
    assert sig["silhouette_device"][:3] == ["codes", "n_clusters", "rows"] and sig["silhouette_device"][-1] == "stream"
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake._dim, fake.device = "f32", np.dtype(np.float32), 10, 4, 0
    fake.metric = pn.distance.Euclidean()
    labels = np.arange(10) % 3
    bad = [lambda: fake.silhouette_samples(labels[:9]), lambda: fake.silhouette_samples(labels.reshape(2, 5)),
           lambda: fake.silhouette_samples(np.zeros(10)),                     # one cluster
           lambda: fake.silhouette_score(labels % 2, ignore=1),                # one cluster once the label is ignored
           lambda: fake.silhouette_samples(labels, rows=[3, 10]), lambda: fake.silhouette_samples(labels, rows=[-1]),
           lambda: fake.silhouette_samples(labels, rows=[]), lambda: fake.silhouette_samples(labels, rows=[0.5]),
           lambda: fake.silhouette_device(labels, 3),                          # CUDA tensors only
           lambda: fake.silhouette_device(labels, 1)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    fake.metric = pn.distance.Cosine()
    for call in (lambda: fake.silhouette_samples(labels), lambda: fake.silhouette_score(labels),
                 lambda: fake.silhouette_device(labels, 3)):
        with pytest.raises(ValueError):
            call()
