"""CPU-side checks of pn_linkage_* and pn_hdbscan_* (no GPU compute calls): the eight symbols are declared with the
stated signatures, listed in the ctypes table and exported, the ABI version is still 3; bad arguments fail in the
documented order -- flags, NULL arrays, NULL index -- before any device is touched; the Python methods exist and raise
ValueError on min_cluster_size = 1, min_samples = 0 and min_samples = n; the C++ mirror compiles."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LINKAGE = ["pn_linkage_f32", "pn_linkage_f64", "pn_linkage_device_f32", "pn_linkage_device_f64"]
HDBSCAN = ["pn_hdbscan_f32", "pn_hdbscan_f64", "pn_hdbscan_device_f32", "pn_hdbscan_device_f64"]


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
    for name in LINKAGE + HDBSCAN:
        assert name in _lib.SIGNATURES and name in exported, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
    assert _lib.lib().pn_abi_version() == 3
    for sfx, ct in (("f32", "float"), ("f64", "double")):
        assert _decl(hdr, f"pn_linkage_{sfx}") == [
            "const pn_index *index", "const uint64_t *src", "const uint64_t *dst", f"const {ct} *weight", "unsigned flags",
            "uint64_t *left_out", "uint64_t *right_out", f"{ct} *weight_out", "uint64_t *size_out"]
        assert _decl(hdr, f"pn_linkage_device_{sfx}") == [
            "const pn_index *index", "const uint64_t *d_src", "const uint64_t *d_dst", f"const {ct} *d_weight",
            "unsigned flags", "uint64_t *d_left", "uint64_t *d_right", f"{ct} *d_weight_out", "uint64_t *d_size",
            "int32_t *d_error", "void *stream"]
        assert _decl(hdr, f"pn_hdbscan_{sfx}") == [
            "const pn_index *index", "size_t min_samples", "size_t min_cluster_size", "unsigned flags", "int64_t *labels",
            f"{ct} *probabilities", "uint64_t *n_clusters"]
        assert _decl(hdr, f"pn_hdbscan_device_{sfx}") == [
            "const pn_index *index", "size_t min_samples", "size_t min_cluster_size", "unsigned flags", "int64_t *d_labels",
            f"{ct} *d_probabilities", "uint64_t *d_n_clusters", "void *stream"]
        # the ctypes table has one entry per C parameter
        for fam in ("linkage", "linkage_device", "hdbscan", "hdbscan_device"):
            assert len(_lib.SIGNATURES[f"pn_{fam}_{sfx}"][1]) == len(_decl(hdr, f"pn_{fam}_{sfx}")), fam
    # the contract is stated under the declarations, and what this version leaves out
    for phrase in (r"TRUE SPLIT", r"FALLS OUT", r"2\^-100", r"strictly greater", r"ascending lowest member row",
                   r"Not in this version: row-sharded handles, allow_single_cluster"):
        assert re.search(phrase, hdr), phrase


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_hdbscan_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_int64 * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_hdbscan_{sfx}")
    dev = getattr(L, f"pn_hdbscan_device_{sfx}")
    calls = [lambda fl, ms, m, lab: host(None, ms, m, fl, lab, None, None),
             lambda fl, ms, m, lab: dev(None, ms, m, fl, lab, None, None, None),
             lambda fl, ms, m, lab: host(None, ms, m, fl, lab, p, p),      # (the optional outputs given: nothing changes)
             lambda fl, ms, m, lab: dev(None, ms, m, fl, lab, p, p, None)]
    for call in calls:
        # unknown flags come first, whatever else is wrong
        for flags in (1, 2, 4, 0x80000000):
            assert call(flags, 0, 0, None) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        # then the output, then the handle: both before the sizes, which need the handle's n
        assert call(0, 0, 0, None) == _lib.PN_ERR_INVALID
        assert "labels is NULL" in _lib.last_error()
        assert call(0, 0, 1, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
        assert call(0, 5, 5, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_linkage_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_linkage_{sfx}")
    dev = getattr(L, f"pn_linkage_device_{sfx}")
    names = ["src", "dst", "weight", "left_out", "right_out", "weight_out", "size_out"]

    def call_host(fl, a):
        return host(None, a[0], a[1], a[2], fl, a[3], a[4], a[5], a[6])

    def call_dev(fl, a):
        return dev(None, a[0], a[1], a[2], fl, a[3], a[4], a[5], a[6], None, None)

    for call in (call_host, call_dev):
        for flags in (1, 2, 0x80000000):
            assert call(flags, [None] * 7) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        for i, name in enumerate(names):  # the first NULL array is named
            args = [p] * 7
            args[i] = None
            assert call(0, args) == _lib.PN_ERR_INVALID
            assert f"{name} is NULL" in _lib.last_error()
        assert call(0, [p] * 7) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    for name in ("linkage", "linkage_device", "hdbscan", "hdbscan_device"):
        assert callable(getattr(bt, name, None)), name
    assert list(inspect.signature(bt.linkage).parameters)[1:3] == ["core", "edges"]
    assert list(inspect.signature(bt.hdbscan).parameters)[1:] == ["min_cluster_size", "min_samples"]
    assert inspect.signature(bt.hdbscan).parameters["min_samples"].default is None
    assert list(inspect.signature(bt.hdbscan_device).parameters)[1:] == [
        "min_cluster_size", "min_samples", "out_labels", "out_probabilities", "out_n_clusters", "stream"]
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake.device = "f32", np.dtype(np.float32), 10, 0
    for m, k in ((1, None), (1, 3), (0, 3), (5, 0), (5, -2), (5, 10), (5, 11)):
        with pytest.raises(ValueError):
            fake.hdbscan(m, k)
        with pytest.raises(ValueError):
            fake.hdbscan_device(m, k)
    # the default for min_samples is min_cluster_size, capped at n - 1
    assert fake._hdbscan_args(5, None) == (5, 5) and fake._hdbscan_args(50, None) == (50, 9)
    # edges of the wrong length, and core together with edges
    z = np.zeros(8, dtype=np.uint64)
    with pytest.raises(ValueError):
        fake.linkage(edges=(z, z, np.zeros(8, dtype=np.float32)))
    z = np.zeros(9, dtype=np.uint64)
    with pytest.raises(ValueError):
        fake.linkage(core=np.zeros(10, dtype=np.float32), edges=(z, z, np.zeros(9, dtype=np.float32)))


def test_cpp_mirror_compiles_with_linkage_and_hdbscan(tmp_path):
    src = tmp_path / "hdb.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "petal::Linkage<float> f(const petal::BallTree<float> &t) { return t.linkage(); }\n"
                   "size_t g(const petal::BallTree<double> &t, const double *core) {\n"
                   "    petal::Linkage<double> l = t.linkage(core), l2 = t.linkage(t.mst());\n"
                   "    petal::Hdbscan<double> h = t.hdbscan(25, 8), h2 = t.hdbscan(5);\n"
                   "    return l.left.size() + l.right.size() + l.size.size() + l2.weight.size() + h.labels.size() +\n"
                   "           h.probabilities.size() + h.n_clusters + h2.n_clusters;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
