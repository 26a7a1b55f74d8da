"""CPU-side checks of pn_mst_* (no GPU compute calls): the symbols are declared, listed in the ctypes table and exported;
PN_OPT_MST_BATCH is 12 and the ABI version still 3; bad arguments fail in the documented order -- flags, NULL outputs,
NULL index -- with the offending name in pn_last_error(), before any device is touched; the Python methods exist and
validate; the C++ mirror compiles."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["pn_mst_f32", "pn_mst_f64", "pn_mst_device_f32", "pn_mst_device_f64"]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    assert re.search(r"\bPN_OPT_MST_BATCH\s*=\s*12\b", hdr) and _lib.PN_OPT_MST_BATCH == 12
    assert re.search(r"#define\s+PN_ABI_VERSION\s+3\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert _lib.lib().pn_abi_version() == 3
    # what this version leaves out is stated under the declarations
    assert re.search(r"Not in this version: row-sharded handles", hdr)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn " + name + r"\(", rust), name


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_mst_{sfx}")
    dev = getattr(L, f"pn_mst_device_{sfx}")
    calls = [lambda fl, s, d, w: host(None, None, fl, s, d, w, None),
             lambda fl, s, d, w: dev(None, None, fl, s, d, w, None, None),
             lambda fl, s, d, w: host(None, p, fl, s, d, w, p),       # (core and work_out given: nothing changes)
             lambda fl, s, d, w: dev(None, p, fl, s, d, w, p, None)]
    for call in calls:
        # unknown flags come first: no flag is defined, the self-queries' bits mean nothing here
        for flags in (1, 2, 4, 0x80000000):
            assert call(flags, None, None, None) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        # then the outputs, by name, then the handle
        assert call(0, None, p, p) == _lib.PN_ERR_INVALID
        assert "src_out is NULL" in _lib.last_error()
        assert call(0, p, None, p) == _lib.PN_ERR_INVALID
        assert "dst_out is NULL" in _lib.last_error()
        assert call(0, p, p, None) == _lib.PN_ERR_INVALID
        assert "weight_out is NULL" in _lib.last_error()
        assert call(0, p, p, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
    # the option is checked by the handle's setter
    assert L.pn_index_set_option(None, _lib.PN_OPT_MST_BATCH, 0) == _lib.PN_ERR_INVALID


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    for name in ("mst", "mst_device", "mutual_reachability_mst"):
        assert callable(getattr(bt, name, None)), name
    assert list(inspect.signature(bt.mst).parameters)[1:] == ["core"]
    assert list(inspect.signature(bt.mst_device).parameters)[1:] == ["core", "out_src", "out_dst", "out_weight", "stream"]
    assert list(inspect.signature(bt.mutual_reachability_mst).parameters)[1:] == ["min_samples"]
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n = "f32", np.dtype(np.float32), 10
    for bad in (np.zeros(9, dtype=np.float32), np.zeros((10, 1), dtype=np.float32), np.zeros(11)):
        with pytest.raises(ValueError):
            fake.mst(bad)
    for bad in (0, -3, 10):
        with pytest.raises(ValueError):
            fake.mutual_reachability_mst(bad)


def test_cpp_mirror_compiles_with_mst(tmp_path):
    src = tmp_path / "mst.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "petal::Mst<float> f(const petal::BallTree<float> &t) { return t.mst(); }\n"
                   "size_t g(const petal::BallTree<double> &t, const double *core) {\n"
                   "    petal::Mst<double> r = t.mst(core);\n"
                   "    return r.src.size() + r.dst.size() + r.weight.size() + r.rounds + r.rows_scanned;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
