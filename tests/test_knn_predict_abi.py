"""CPU-side checks of pn_knn_classify_* and pn_knn_regress_* (no GPU compute calls): the sixteen symbols are declared with
the stated parameter lists, listed in the ctypes table, exported and present in the Rust extern block, the ABI version is
still 3; the header states the contract; bad arguments fail in the documented order -- flags, NULL output, NULL inputs,
NULL index -- before any device is touched; the Python methods exist with the stated signatures and validate their
arguments; the host methods, driven through a stubbed library, call declared symbols of the handle's suffix; the C++
mirror compiles."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FAMILIES = ["knn_classify", "knn_classify_device", "knn_classify_self", "knn_classify_self_device",
            "knn_regress", "knn_regress_device", "knn_regress_self", "knn_regress_self_device"]
NAMES = [f"pn_{fam}_{sfx}" for fam in FAMILIES for sfx in ("f32", "f64")]


def _decl(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_symbols_declared_listed_and_exported(pn):
    from petal_neighbors_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "petal_mi355x.h")).read()
    assert re.search(r"#define\s+PN_ABI_VERSION\s+3\b", hdr)
    assert re.search(r"#define\s+PN_KNN_WEIGHT_DISTANCE\s+1u?\b", hdr) and _lib.PN_KNN_WEIGHT_DISTANCE == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (pn_[a-z0-9_]+)", out.stdout))
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert len(NAMES) == 16
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in exported, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
    assert _lib.lib().pn_abi_version() == 3
    for sfx, ct in (("f32", "float"), ("f64", "double")):
        qh = ["const pn_index *index", f"const {ct} *queries", "size_t nq", "size_t q_cols", "ptrdiff_t q_row_stride", "size_t k"]
        qd = ["const pn_index *index", f"const {ct} *d_queries", "size_t nq", "size_t q_cols", "size_t q_row_stride", "size_t k"]
        sf = ["const pn_index *index", "size_t k"]
        assert _decl(hdr, f"pn_knn_classify_{sfx}") == qh + [
            "const int64_t *labels", "size_t n_classes", "unsigned flags", "int64_t *pred_out", "double *proba_out"]
        assert _decl(hdr, f"pn_knn_classify_device_{sfx}") == qd + [
            "const int64_t *d_labels", "size_t n_classes", "unsigned flags", "int64_t *d_pred", "double *d_proba", "void *stream"]
        assert _decl(hdr, f"pn_knn_classify_self_{sfx}") == sf + [
            "const int64_t *labels", "size_t n_classes", "unsigned flags", "int64_t *pred_out", "double *proba_out"]
        assert _decl(hdr, f"pn_knn_classify_self_device_{sfx}") == sf + [
            "const int64_t *d_labels", "size_t n_classes", "unsigned flags", "int64_t *d_pred", "double *d_proba", "void *stream"]
        assert _decl(hdr, f"pn_knn_regress_{sfx}") == qh + [
            "const double *targets", "size_t n_out", "unsigned flags", "double *out"]
        assert _decl(hdr, f"pn_knn_regress_device_{sfx}") == qd + [
            "const double *d_targets", "size_t n_out", "unsigned flags", "double *d_out", "void *stream"]
        assert _decl(hdr, f"pn_knn_regress_self_{sfx}") == sf + [
            "const double *targets", "size_t n_out", "unsigned flags", "double *out"]
        assert _decl(hdr, f"pn_knn_regress_self_device_{sfx}") == sf + [
            "const double *d_targets", "size_t n_out", "unsigned flags", "double *d_out", "void *stream"]
        for fam in FAMILIES:  # the ctypes table has one entry per C parameter
            assert len(_lib.SIGNATURES[f"pn_{fam}_{sfx}"][1]) == len(_decl(hdr, f"pn_{fam}_{sfx}")), fam
    # the contract is stated above the declarations, and the additive note names the new entries
    for phrase in (r"PN_KNN_WEIGHT_DISTANCE", r"list order", r"smallest", r"`-1`", r"1024", r"_get_weights", r"pairwise"):
        assert re.search(phrase, hdr), phrase
    note = hdr[hdr.index("Additive within version 3"):hdr.index("#define PN_ABI_VERSION")]
    assert "pn_knn_classify_" in note and "pn_knn_regress_" in note


def _callers(L, sfx, p, q="P", values="P", out="P", nq=1, flags=0, proba=None, width=2, k=3):
    """the eight entries with one set of arguments: q / values / out are 'P' (the buffer) or None"""
    g = lambda x: p if x == "P" else x  # noqa: E731
    f = lambda fam: getattr(L, f"pn_{fam}_{sfx}")  # noqa: E731
    return {
        "knn_classify": lambda h: f("knn_classify")(h, g(q), nq, 2, 2, k, g(values), width, flags, g(out), proba),
        "knn_classify_device": lambda h: f("knn_classify_device")(h, g(q), nq, 2, 2, k, g(values), width, flags, g(out), proba, None),
        "knn_classify_self": lambda h: f("knn_classify_self")(h, k, g(values), width, flags, g(out), proba),
        "knn_classify_self_device": lambda h: f("knn_classify_self_device")(h, k, g(values), width, flags, g(out), proba, None),
        "knn_regress": lambda h: f("knn_regress")(h, g(q), nq, 2, 2, k, g(values), width, flags, g(out)),
        "knn_regress_device": lambda h: f("knn_regress_device")(h, g(q), nq, 2, 2, k, g(values), width, flags, g(out), None),
        "knn_regress_self": lambda h: f("knn_regress_self")(h, k, g(values), width, flags, g(out)),
        "knn_regress_self_device": lambda h: f("knn_regress_self_device")(h, k, g(values), width, flags, g(out), None),
    }


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    for fam in FAMILIES:
        classify, self_ = "classify" in fam, "self" in fam
        values_name, out_name = ("labels", "pred_out") if classify else ("targets", "out")
        # unknown flags come first, whatever else is wrong
        for flags in (2, 4, 3, 0x80000000):
            assert _callers(L, sfx, p, None, None, None, flags=flags, width=0, k=0)[fam](None) == _lib.PN_ERR_INVALID, fam
            assert "flags" in _lib.last_error(), fam
        for flags in (0, 1):  # both weightings are known
            # then the required output
            assert _callers(L, sfx, p, None, None, None, flags=flags, width=0, k=0)[fam](None) == _lib.PN_ERR_INVALID
            assert f"{out_name} is NULL" in _lib.last_error(), fam
            # then the first NULL input, named
            if not self_:
                assert _callers(L, sfx, p, None, None, "P", flags=flags, width=0, k=0)[fam](None) == _lib.PN_ERR_INVALID
                assert "queries is NULL" in _lib.last_error(), fam
            assert _callers(L, sfx, p, "P", None, "P", flags=flags, width=0, k=0)[fam](None) == _lib.PN_ERR_INVALID
            assert f"{values_name} is NULL" in _lib.last_error(), fam
            # then the handle: before n_classes / n_out and k
            assert _callers(L, sfx, p, "P", "P", "P", flags=flags, width=0, k=0)[fam](None) == _lib.PN_ERR_INVALID
            assert "index is NULL" in _lib.last_error(), fam
            assert _callers(L, sfx, p, "P", "P", "P", flags=flags, k=2000)[fam](None) == _lib.PN_ERR_INVALID
            assert "index is NULL" in _lib.last_error(), fam
        if not self_:  # nq = 0: the inputs are not looked at; the handle is
            assert _callers(L, sfx, p, None, None, "P", nq=0)[fam](None) == _lib.PN_ERR_INVALID
            assert "index is NULL" in _lib.last_error(), fam


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    sig = lambda name: inspect.signature(getattr(bt, name))  # noqa: E731
    assert list(sig("knn_classify").parameters)[1:] == ["queries", "k", "labels", "weights", "proba"]
    assert list(sig("knn_classify_self").parameters)[1:] == ["k", "labels", "weights", "proba"]
    assert list(sig("knn_regress").parameters)[1:] == ["queries", "k", "targets", "weights"]
    assert list(sig("knn_regress_self").parameters)[1:] == ["k", "targets", "weights"]
    assert list(sig("knn_classify_device").parameters)[1:] == [
        "queries", "k", "labels", "n_classes", "weights", "proba", "out_pred", "out_proba", "stream"]
    assert list(sig("knn_classify_self_device").parameters)[1:] == [
        "k", "labels", "n_classes", "weights", "proba", "out_pred", "out_proba", "stream"]
    assert list(sig("knn_regress_device").parameters)[1:] == ["queries", "k", "targets", "weights", "out", "stream"]
    assert list(sig("knn_regress_self_device").parameters)[1:] == ["k", "targets", "weights", "out", "stream"]
    for name in FAMILIES:
        assert sig(name).parameters["weights"].default == "uniform", name
        if "classify" in name:
            assert sig(name).parameters["proba"].default is False, name
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake.device = "f32", np.dtype(np.float32), 10, 0
    q = np.zeros((3, 4), dtype=np.float32)
    labels, y = np.arange(10) % 3, np.ones((10, 2))
    for k in (0, -1, 11):
        with pytest.raises(ValueError):
            fake.knn_classify(q, k, labels)
        with pytest.raises(ValueError):
            fake.knn_regress(q, k, y)
        with pytest.raises(ValueError):
            fake.knn_classify_device(q, k, labels, 3)
        with pytest.raises(ValueError):
            fake.knn_regress_device(q, k, y)
    for k in (0, 10, 11):  # the row itself is left out: k <= n - 1
        with pytest.raises(ValueError):
            fake.knn_classify_self(k, labels)
        with pytest.raises(ValueError):
            fake.knn_regress_self(k, y)
        with pytest.raises(ValueError):
            fake.knn_classify_self_device(k, labels, 3)
        with pytest.raises(ValueError):
            fake.knn_regress_self_device(k, y)
    for bad in (np.arange(9), np.zeros((10, 1), dtype=np.int64), np.zeros((2, 5), dtype=np.int64)):
        with pytest.raises(ValueError):
            fake.knn_classify(q, 3, bad)
        with pytest.raises(ValueError):
            fake.knn_classify_self(3, bad, proba=True)
    for bad in (np.ones((9, 2)), np.ones(9), np.ones((10, 2, 1)), np.ones((10, 0)), np.ones(10, dtype=np.complex128)):
        with pytest.raises(ValueError):
            fake.knn_regress(q, 3, bad)
        with pytest.raises(ValueError):
            fake.knn_regress_self(3, bad)
    for weights in ("gaussian", None, 1):
        with pytest.raises(ValueError):
            fake.knn_classify(q, 3, labels, weights=weights)
        with pytest.raises(ValueError):
            fake.knn_classify_self(3, labels, weights)
        with pytest.raises(ValueError):
            fake.knn_regress(q, 3, y, weights)
        with pytest.raises(ValueError):
            fake.knn_regress_self(3, y, weights=weights)
    # the device methods take CUDA tensors only
    with pytest.raises(ValueError):
        fake.knn_classify_device(q, 3, labels, 3)
    with pytest.raises(ValueError):
        fake.knn_classify_self_device(3, labels.astype(np.int64), 3)
    with pytest.raises(ValueError):
        fake.knn_regress_device(q, 3, y)
    with pytest.raises(ValueError):
        fake.knn_regress_self_device(3, y)
    for c in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            fake.knn_classify_self_device(3, labels, c)


# ---- the host methods through a stubbed library (the Stub and the checks of tests/test_binding_calls.py)
class Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
            return 0  # PN_OK
        return record


def _check(calls, sfx):
    from petal_neighbors_amd import _lib
    other = "f64" if sfx == "f32" else "f32"
    for name, args in calls:
        assert name in _lib.SIGNATURES, name
        argtypes = _lib.SIGNATURES[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for a, t in zip(args, argtypes):
            t.from_param(a)  # raises where ctypes would refuse the argument
        assert name.endswith("_" + sfx) and not name.endswith("_" + other), (name, sfx)
    return [name for name, _ in calls]


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_host_methods_call_the_table(pn, monkeypatch, sfx):
    from petal_neighbors_amd import _lib
    stub = Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    bt = pn.BallTree
    t = bt.__new__(bt)
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    t._h, t._sfx, t.dtype, t._n, t._dim, t.device = C.c_void_p(1), sfx, dt, 10, 4, 0
    q = np.zeros((3, 4), dtype=dt)
    labels = np.array(list("abcab" * 2))
    pred = t.knn_classify(q, 3, labels)
    assert pred.shape == (3,) and pred.dtype == labels.dtype
    pred, proba, classes = t.knn_classify(q, 3, labels, weights="distance", proba=True)
    assert proba.shape == (3, 3) and classes.tolist() == ["a", "b", "c"]
    pred, proba, classes = t.knn_classify_self(3, labels, proba=True)
    assert pred.shape == (10,) and proba.shape == (10, 3)
    assert t.knn_classify_self(9, np.arange(10), "distance").dtype == np.arange(10).dtype
    assert t.knn_regress(q, 10, np.arange(10)).shape == (3,)              # integer targets, 1-D in, 1-D out
    assert t.knn_regress(q, 1, np.ones((10, 5), dtype=np.float32), "distance").shape == (3, 5)
    assert t.knn_regress_self(2, np.ones(10)).shape == (10,)
    assert t.knn_regress_self(2, np.ones((10, 1)), weights="distance").shape == (10, 1)
    assert t.knn_classify(np.zeros((0, 4), dtype=dt), 3, labels).shape == (0,)  # no queries: no call
    seen = _check(stub.calls, sfx)
    assert seen == [f"pn_{fam}_{sfx}" for fam in ("knn_classify", "knn_classify", "knn_classify_self", "knn_classify_self",
                                                  "knn_regress", "knn_regress", "knn_regress_self", "knn_regress_self")]
    flags = [args[8] if "self" not in name else args[4] for name, args in stub.calls]
    assert flags == [0, 1, 0, 1, 0, 1, 0, 1]
    widths = [args[7] if "self" not in name else args[3] for name, args in stub.calls]
    assert widths == [3, 3, 3, 10, 1, 5, 1, 1]


def test_cpp_mirror_compiles_with_knn_predict(tmp_path):
    src = tmp_path / "knn.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "size_t f(const petal::BallTree<float> &t, const float *q, const std::vector<int64_t> &lab,\n"
                   "         const std::vector<double> &y) {\n"
                   "    petal::KnnClasses a = t.knn_classify(q, 7, 5, lab, 3);\n"
                   "    petal::KnnClasses b = t.knn_classify_self(5, lab, 3, true, true);\n"
                   "    std::vector<double> r = t.knn_regress(q, 7, 5, y, 2, true);\n"
                   "    std::vector<double> s = t.knn_regress_self(5, y, 2);\n"
                   "    return a.pred.size() + b.proba.size() + r.size() + s.size();\n}\n"
                   "double g(const petal::BallTree<double> &t, const double *q, const std::vector<int64_t> &lab,\n"
                   "         const std::vector<double> &y) {\n"
                   "    petal::KnnClasses a = t.knn_classify(q, 1, 5, lab, 3, false, true);\n"
                   "    const std::vector<int64_t> &p = t.knn_classify_self(2, lab, 3).pred;\n"
                   "    return a.proba[0] + (double)p[0] + t.knn_regress(q, 1, 5, y, 1)[0] + t.knn_regress_self(5, y, 1, true)[0];\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_the_unit_is_built_without_contraction(pn):
    import importlib.util as u
    spec = u.spec_from_file_location("pn_build", os.path.join(ROOT, "petal-neighbors_amd", "build.py"))
    b = u.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("knn_predict.hip", ["-ffp-contract=off"]) in b.UNITS
