"""CPU-side checks of pn_dbscan_* (no GPU compute calls): the symbols are declared, listed in the ctypes table and
exported; PN_OPT_DBSCAN_PIECE is 11 and the ABI version still 3; bad arguments fail with PN_ERR_INVALID, in the documented
order, before any device is touched; the Python methods exist and validate; the C++ mirror compiles."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["pn_dbscan_f32", "pn_dbscan_f64", "pn_dbscan_device_f32", "pn_dbscan_device_f64"]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    assert re.search(r"\bPN_OPT_DBSCAN_PIECE\s*=\s*11\b", hdr) and _lib.PN_OPT_DBSCAN_PIECE == 11
    assert re.search(r"#define\s+PN_ABI_VERSION\s+3\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert _lib.lib().pn_abi_version() == 3
    assert re.search(r"Not yet: row-sharded handles", hdr)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    ct = C.c_float if sfx == "f32" else C.c_double
    buf = (C.c_int64 * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_dbscan_{sfx}")
    dev = getattr(L, f"pn_dbscan_device_{sfx}")
    calls = [lambda fl, ms, lab: host(None, ct(1.0), ms, fl, lab, None, None),
             lambda fl, ms, lab: dev(None, ct(1.0), ms, fl, lab, None, None, None)]
    for call in calls:
        # unknown flags come first: the self-queries' bits mean nothing here
        for flags in (1, 2, 4, 0x80000000):
            assert call(flags, 0, None) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        # then min_samples, then the output, then the handle
        assert call(0, 0, None) == _lib.PN_ERR_INVALID
        assert "min_samples" in _lib.last_error()
        assert call(0, 5, None) == _lib.PN_ERR_INVALID
        assert "labels is NULL" in _lib.last_error()
        assert call(0, 5, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
    # core and n_clusters are optional: with them given the NULL index is still what fails
    assert host(None, ct(0.5), 1, 0, p, p, p) == _lib.PN_ERR_INVALID
    assert "index is NULL" in _lib.last_error()
    # the option is checked by the handle's setter
    assert L.pn_index_set_option(None, _lib.PN_OPT_DBSCAN_PIECE, 0) == _lib.PN_ERR_INVALID


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    for name in ("dbscan", "dbscan_device"):
        assert callable(getattr(bt, name, None)), name
    assert list(inspect.signature(bt.dbscan).parameters)[1:] == ["eps", "min_samples"]
    assert list(inspect.signature(bt.dbscan_device).parameters)[1:] == ["eps", "min_samples", "out_labels", "out_core",
                                                                         "out_n_clusters", "stream"]
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n = "f32", np.dtype(np.float32), 10
    for bad in (0, -3):
        with pytest.raises(ValueError):
            fake.dbscan(0.5, bad)
        with pytest.raises(ValueError):
            fake.dbscan_device(0.5, bad)


def test_cpp_mirror_compiles_with_dbscan(tmp_path):
    src = tmp_path / "db.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "petal::Dbscan f(const petal::BallTree<float> &t) { return t.dbscan(0.5f, 10); }\n"
                   "size_t g(const petal::BallTree<double> &t) {\n"
                   "    petal::Dbscan r = t.dbscan(0.25, 4);\n"
                   "    return r.n_clusters + r.labels.size() + r.core.size();\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
