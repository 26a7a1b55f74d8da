"""CPU-side checks of pn_lof_* and pn_lof_score_* (no GPU compute calls): the eight symbols are declared with the stated
signatures, listed in the ctypes table, exported and present in the Rust extern block, the ABI version is still 3; the
header states the contract; bad arguments fail in the documented order -- flags, NULL outputs / inputs, NULL index --
before any device is touched; the Python methods exist and raise ValueError on k = 0, k = n and arrays of the wrong
length; the C++ mirror compiles."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIT = ["pn_lof_f32", "pn_lof_f64", "pn_lof_device_f32", "pn_lof_device_f64"]
SCORE = ["pn_lof_score_f32", "pn_lof_score_f64", "pn_lof_score_device_f32", "pn_lof_score_device_f64"]


def _decl(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    assert re.search(r"#define\s+PN_ABI_VERSION\s+3\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in FIT + SCORE:
        assert name in _lib.SIGNATURES and name in exported, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
    assert _lib.lib().pn_abi_version() == 3
    for sfx, ct in (("f32", "float"), ("f64", "double")):
        assert _decl(hdr, f"pn_lof_{sfx}") == [
            "const pn_index *index", "size_t k", "unsigned flags", "double *lof", "double *lrd", f"{ct} *kdist"]
        assert _decl(hdr, f"pn_lof_device_{sfx}") == [
            "const pn_index *index", "size_t k", "unsigned flags", "double *d_lof", "double *d_lrd", f"{ct} *d_kdist",
            "void *stream"]
        assert _decl(hdr, f"pn_lof_score_{sfx}") == [
            "const pn_index *index", f"const {ct} *queries", "size_t nq", "size_t q_cols", "ptrdiff_t q_row_stride",
            "size_t k", "const double *lrd", f"const {ct} *kdist", "unsigned flags", "double *score_out"]
        assert _decl(hdr, f"pn_lof_score_device_{sfx}") == [
            "const pn_index *index", f"const {ct} *d_queries", "size_t nq", "size_t q_cols", "size_t q_row_stride",
            "size_t k", "const double *d_lrd", f"const {ct} *d_kdist", "unsigned flags", "double *d_score", "void *stream"]
        # the ctypes table has one entry per C parameter
        for fam in ("lof", "lof_device", "lof_score", "lof_score_device"):
            assert len(_lib.SIGNATURES[f"pn_{fam}_{sfx}"][1]) == len(_decl(hdr, f"pn_{fam}_{sfx}")), fam
    # the contract is stated under the declarations
    for phrase in (r"1e-10", r"list order", r"np\.maximum", r"n \* k \* \(4 \+ sizeof T\) \+ n \* \(8 \+ sizeof T\) bytes",
                   r"score_samples", r"negative_outlier_factor_"):
        assert re.search(phrase, hdr), phrase


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_lof_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_lof_{sfx}")
    dev = getattr(L, f"pn_lof_device_{sfx}")
    calls = [lambda fl, k, lof: host(None, k, fl, lof, None, None),
             lambda fl, k, lof: dev(None, k, fl, lof, None, None, None),
             lambda fl, k, lof: host(None, k, fl, lof, p, p),      # (the optional outputs given: nothing changes)
             lambda fl, k, lof: dev(None, k, fl, lof, p, p, None)]
    for call in calls:
        # unknown flags come first, whatever else is wrong
        for flags in (1, 2, 4, 0x80000000):
            assert call(flags, 0, None) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        # then the output, then the handle: both before k, which needs the handle's n
        assert call(0, 0, None) == _lib.PN_ERR_INVALID
        assert "lof is NULL" in _lib.last_error()
        assert call(0, 0, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
        assert call(0, 5, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_lof_score_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_lof_score_{sfx}")
    dev = getattr(L, f"pn_lof_score_device_{sfx}")

    def call_host(fl, nq, q, lrd, kdist, out):
        return host(None, q, nq, 2, 2, 3, lrd, kdist, fl, out)

    def call_dev(fl, nq, q, lrd, kdist, out):
        return dev(None, q, nq, 2, 2, 3, lrd, kdist, fl, out, None)

    for call in (call_host, call_dev):
        for flags in (1, 2, 0x80000000):
            assert call(flags, 1, None, None, None, None) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        assert call(0, 1, p, p, p, None) == _lib.PN_ERR_INVALID
        assert "score_out is NULL" in _lib.last_error()
        for i, name in enumerate(["queries", "lrd", "kdist"]):  # nq > 0: the first NULL input is named
            args = [p] * 3
            args[i] = None
            assert call(0, 1, *args, p) == _lib.PN_ERR_INVALID
            assert f"{name} is NULL" in _lib.last_error()
        # nq = 0: the inputs are not looked at; the handle is
        assert call(0, 0, None, None, None, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
        assert call(0, 1, p, p, p, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    for name in ("lof", "lof_device", "lof_score", "lof_score_device"):
        assert callable(getattr(bt, name, None)), name
    assert list(inspect.signature(bt.lof).parameters)[1:] == ["k", "full"]
    assert inspect.signature(bt.lof).parameters["k"].default == 20
    assert inspect.signature(bt.lof).parameters["full"].default is False
    assert list(inspect.signature(bt.lof_device).parameters)[1:] == ["k", "out_lof", "out_lrd", "out_kdist", "stream"]
    assert inspect.signature(bt.lof_device).parameters["k"].default == 20
    assert list(inspect.signature(bt.lof_score).parameters)[1:] == ["queries", "k", "lrd", "kdist"]
    assert list(inspect.signature(bt.lof_score_device).parameters)[1:] == ["queries", "k", "lrd", "kdist", "out", "stream"]
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake.device = "f32", np.dtype(np.float32), 10, 0
    q = np.zeros((3, 4), dtype=np.float32)
    lrd, kdist = np.ones(10), np.ones(10, dtype=np.float32)
    for k in (0, -1, 10, 11):
        with pytest.raises(ValueError):
            fake.lof(k)
        with pytest.raises(ValueError):
            fake.lof(k, full=True)
        with pytest.raises(ValueError):
            fake.lof_device(k)
        with pytest.raises(ValueError):
            fake.lof_score(q, k, lrd, kdist)
        with pytest.raises(ValueError):
            fake.lof_score_device(q, k, lrd, kdist)
    # a fit of the wrong length
    for bad_lrd, bad_kdist in ((np.ones(9), kdist), (lrd, np.ones(11, dtype=np.float32)), (np.ones((10, 1)), kdist)):
        with pytest.raises(ValueError):
            fake.lof_score(q, 3, bad_lrd, bad_kdist)
    # the device methods take CUDA tensors only
    with pytest.raises(ValueError):
        fake.lof_score_device(q, 3, lrd, kdist)
    for name in ("out_lof", "out_lrd", "out_kdist"):
        with pytest.raises(ValueError):
            fake.lof_device(3, **{name: np.empty(10, dtype=np.float32 if name == "out_kdist" else np.float64)})


def test_cpp_mirror_compiles_with_lof(tmp_path):
    src = tmp_path / "lof.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "size_t f(const petal::BallTree<float> &t, const float *q) {\n"
                   "    petal::Lof<float> fit = t.lof(20);\n"
                   "    std::vector<double> s = t.lof_score(q, 7, fit, 20);\n"
                   "    return fit.lof.size() + fit.lrd.size() + fit.kdist.size() + s.size();\n}\n"
                   "double g(const petal::BallTree<double> &t, const double *q) {\n"
                   "    petal::Lof<double> fit = t.lof(5);\n"
                   "    const std::vector<double> &kd = fit.kdist;\n"
                   "    return t.lof_score(q, 1, fit, 5)[0] + kd[0];\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
