"""CPU-side checks of pn_optics_* and pn_optics_dbscan_* (no GPU compute calls): the eight symbols are declared with the
stated signatures, listed in the ctypes table, exported and present in the Rust extern block; PN_OPT_OPTICS_PIECE is 13
and the ABI version still 3; the header states the contract; bad arguments fail in the documented order -- flags, NULL
outputs / inputs, NULL index -- before any device is touched; the Python methods exist with the documented signatures
and validate; the C++ mirror compiles."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ORDER = ["pn_optics_f32", "pn_optics_f64", "pn_optics_device_f32", "pn_optics_device_f64"]
EXTRACT = ["pn_optics_dbscan_f32", "pn_optics_dbscan_f64", "pn_optics_dbscan_device_f32", "pn_optics_dbscan_device_f64"]


def _decl(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    assert re.search(r"\bPN_OPT_OPTICS_PIECE\s*=\s*13\b", hdr) and _lib.PN_OPT_OPTICS_PIECE == 13
    assert re.search(r"#define\s+PN_ABI_VERSION\s+3\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ORDER + EXTRACT:
        assert name in _lib.SIGNATURES and name in exported, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
    assert _lib.lib().pn_abi_version() == 3
    # the symbol list at the top of the header names the family
    assert "pn_optics_{,device_}{f32,f64}" in hdr and "pn_optics_dbscan_{,device_}{f32,f64}" in hdr
    for sfx, ct in (("f32", "float"), ("f64", "double")):
        assert _decl(hdr, f"pn_optics_{sfx}") == [
            "const pn_index *index", "size_t min_samples", f"{ct} max_eps", "unsigned flags", "uint64_t *ordering",
            f"{ct} *reachability", "int64_t *predecessor", f"{ct} *core_distances"]
        assert _decl(hdr, f"pn_optics_device_{sfx}") == [
            "const pn_index *index", "size_t min_samples", f"{ct} max_eps", "unsigned flags", "uint64_t *d_ordering",
            f"{ct} *d_reachability", "int64_t *d_predecessor", f"{ct} *d_core_distances", "void *stream"]
        assert _decl(hdr, f"pn_optics_dbscan_{sfx}") == [
            "const pn_index *index", "const uint64_t *ordering", f"const {ct} *reachability",
            f"const {ct} *core_distances", f"{ct} eps", "unsigned flags", "int64_t *labels", "uint64_t *n_clusters"]
        assert _decl(hdr, f"pn_optics_dbscan_device_{sfx}") == [
            "const pn_index *index", "const uint64_t *d_ordering", f"const {ct} *d_reachability",
            f"const {ct} *d_core_distances", f"{ct} eps", "unsigned flags", "int64_t *d_labels", "uint64_t *d_n_clusters",
            "int32_t *d_error", "void *stream"]
        for fam in ("optics", "optics_device", "optics_dbscan", "optics_dbscan_device"):
            assert len(_lib.SIGNATURES[f"pn_{fam}_{sfx}"][1]) == len(_decl(hdr, f"pn_{fam}_{sfx}")), fam
    # the contract is stated under the declarations
    for phrase in (r"min_samples >= 1 counts OTHER rows", r"WITHOUT PN_OPT_INDEX_BASE", r"ties broken by the\s+\*?\s*lower row",
                   r"up to this library's\s+\*?\s*distance arithmetic", r"E \* \(4 \+ sizeof T\) \+ 8 \(n \+ 1\) bytes",
                   r"BLOCKS THE HOST ONCE", r"NOT pn_dbscan_\*'s \"lowest member row\" numbering", r"isolated \+inf entry",
                   r"cluster_optics_dbscan", r"ONE launch of ONE workgroup"):
        assert re.search(phrase, hdr), phrase


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_optics_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    ct = C.c_float if sfx == "f32" else C.c_double
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_optics_{sfx}")
    dev = getattr(L, f"pn_optics_device_{sfx}")
    calls = [lambda fl, ms, o, r: host(None, ms, ct(1.0), fl, o, r, None, None),
             lambda fl, ms, o, r: dev(None, ms, ct(1.0), fl, o, r, None, None, None),
             lambda fl, ms, o, r: host(None, ms, ct(1.0), fl, o, r, p, p),      # (the optional outputs given: nothing changes)
             lambda fl, ms, o, r: dev(None, ms, ct(1.0), fl, o, r, p, p, None)]
    for call in calls:
        # unknown flags come first, whatever else is wrong
        for flags in (1, 2, 4, 0x80000000):
            assert call(flags, 0, None, None) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        # then the required outputs, then the handle: all before min_samples, which needs the handle's n
        assert call(0, 0, None, p) == _lib.PN_ERR_INVALID
        assert "ordering is NULL" in _lib.last_error()
        assert call(0, 0, p, None) == _lib.PN_ERR_INVALID
        assert "reachability is NULL" in _lib.last_error()
        assert call(0, 0, p, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
        assert call(0, 5, p, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
    # the option is checked by the handle's setter
    assert L.pn_index_set_option(None, _lib.PN_OPT_OPTICS_PIECE, 0) == _lib.PN_ERR_INVALID


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_optics_dbscan_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    ct = C.c_float if sfx == "f32" else C.c_double
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    host = getattr(L, f"pn_optics_dbscan_{sfx}")
    dev = getattr(L, f"pn_optics_dbscan_device_{sfx}")
    calls = [lambda fl, o, r, c, lab: host(None, o, r, c, ct(0.5), fl, lab, None),
             lambda fl, o, r, c, lab: dev(None, o, r, c, ct(0.5), fl, lab, None, None, None),
             lambda fl, o, r, c, lab: host(None, o, r, c, ct(0.5), fl, lab, p),
             lambda fl, o, r, c, lab: dev(None, o, r, c, ct(0.5), fl, lab, p, p, None)]
    for call in calls:
        for flags in (1, 2, 0x80000000):
            assert call(flags, None, None, None, None) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        assert call(0, p, p, p, None) == _lib.PN_ERR_INVALID
        assert "labels is NULL" in _lib.last_error()
        for i, name in enumerate(["ordering", "reachability", "core_distances"]):  # the first NULL input is named
            args = [p] * 3
            args[i] = None
            assert call(0, *args, p) == _lib.PN_ERR_INVALID
            assert f"{name} is NULL" in _lib.last_error()
        assert call(0, p, p, p, p) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    for name in ("optics", "optics_device", "optics_dbscan", "optics_dbscan_device"):
        assert callable(getattr(bt, name, None)), name
    assert list(inspect.signature(bt.optics).parameters)[1:] == ["min_samples", "max_eps"]
    assert inspect.signature(bt.optics).parameters["max_eps"].default == np.inf
    assert list(inspect.signature(bt.optics_device).parameters)[1:] == [
        "min_samples", "max_eps", "out_ordering", "out_reachability", "out_predecessor", "out_core", "stream"]
    assert list(inspect.signature(bt.optics_dbscan).parameters)[1:] == ["eps", "ordering", "reachability", "core_distances"]
    assert list(inspect.signature(bt.optics_dbscan_device).parameters)[1:5] == ["eps", "ordering", "reachability",
                                                                                "core_distances"]
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake.device = "f32", np.dtype(np.float32), 10, 0
    for bad in (0, -1, 10, 11):
        with pytest.raises(ValueError):
            fake.optics(bad)
        with pytest.raises(ValueError):
            fake.optics(bad, 0.5)
        with pytest.raises(ValueError):
            fake.optics_device(bad, 0.5)
    o, r, c = np.arange(10, dtype=np.uint64), np.ones(10, dtype=np.float32), np.ones(10, dtype=np.float32)
    for bo, br, bc in ((o[:9], r, c), (o, np.ones(11, dtype=np.float32), c), (o, r, np.ones((10, 1), dtype=np.float32))):
        with pytest.raises(ValueError):
            fake.optics_dbscan(0.5, bo, br, bc)
    # the device methods take CUDA tensors only
    with pytest.raises(ValueError):
        fake.optics_dbscan_device(0.5, o, r, c)
    for name in ("out_ordering", "out_reachability", "out_predecessor", "out_core"):
        with pytest.raises(ValueError):
            fake.optics_device(3, 0.5, **{name: np.empty(10, dtype=np.float32)})


def test_cpp_mirror_compiles_with_optics(tmp_path):
    src = tmp_path / "optics.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "size_t f(const petal::BallTree<float> &t) {\n"
                   "    petal::Optics<float> o = t.optics(5, 0.5f);\n"
                   "    petal::OpticsDbscan d = t.optics_dbscan(o, 0.25f);\n"
                   "    return o.ordering.size() + o.predecessor.size() + d.labels.size() + d.n_clusters;\n}\n"
                   "double g(const petal::BallTree<double> &t) {\n"
                   "    petal::Optics<double> o = t.optics(9);\n"
                   "    return o.reachability[0] + o.core_distances[0] + (double)t.optics_dbscan(o, 1.0).n_clusters;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
