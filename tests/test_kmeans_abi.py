"""CPU-side checks of pn_kmeans_* (no GPU compute calls): the nine symbols are declared with the stated signatures, listed
in the ctypes table, exported and present in the Rust extern block and the C++ mirror, the ABI version is still 3; the
header states the contract; bad arguments fail in the documented order -- flags, tol, max_iter, NULL outputs, NULL
inputs, nc == 0, NULL index -- before any device is touched; the Python methods exist and validate; kmeans.hip is built
unfused and its kernels do not spill."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FAMILIES = ["kmeans_assign", "kmeans_assign_device", "kmeans", "kmeans_device"]
NAMES = [f"pn_{fam}_{sfx}" for fam in FAMILIES for sfx in ("f32", "f64")] + ["pn_kmeans_bounds_f32"]


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
    hpp = open(os.path.join(ROOT, "include", "petal_neighbors.hpp")).read()
    assert len(NAMES) == 9
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in exported, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
        assert len(_lib.SIGNATURES[name][1]) == len(_decl(hdr, name)), name  # one ctypes entry per C parameter
        n_rust = re.search(r"pub fn " + name + r"\(([^;]*?)\)\s*->\s*c_int;", rust, re.S).group(1).count(":")
        assert n_rust == len(_decl(hdr, name)), name
    for name in ("pn_kmeans_assign_f32", "pn_kmeans_assign_f64", "pn_kmeans_f32", "pn_kmeans_f64"):
        assert name + "(" in hpp, name
    assert _lib.lib().pn_abi_version() == 3
    # listed among the additions of version 3
    head = hdr[:hdr.index("#define PN_ABI_VERSION")]
    assert "pn_kmeans_{,device_}{f32,f64}, pn_kmeans_assign_{,device_}{f32,f64}, pn_kmeans_bounds_f32" in head
    for sfx, ct in (("f32", "float"), ("f64", "double")):
        assert _decl(hdr, f"pn_kmeans_assign_{sfx}") == [
            "const pn_index *index", f"const {ct} *centres", "size_t nc", "unsigned flags", "int64_t *labels_out",
            f"{ct} *dist_out", "double *inertia_out"]
        assert _decl(hdr, f"pn_kmeans_assign_device_{sfx}") == [
            "const pn_index *index", f"const {ct} *d_centres", "size_t nc", "unsigned flags", "int64_t *d_labels",
            f"{ct} *d_dist", "double *d_inertia", "void *stream"]
        assert _decl(hdr, f"pn_kmeans_{sfx}") == [
            "const pn_index *index", f"const {ct} *init_centres", "size_t nc", "double tol", "size_t max_iter",
            "unsigned flags", f"{ct} *centres_out", "int64_t *labels_out", f"{ct} *dist_out", "uint64_t *counts_out",
            "double *inertia_out", "uint64_t *iterations_out", "double *shift2_out"]
        assert _decl(hdr, f"pn_kmeans_device_{sfx}") == [
            "const pn_index *index", f"const {ct} *d_init_centres", "size_t nc", "double tol", "size_t max_iter",
            "unsigned flags", f"{ct} *d_centres", "int64_t *d_labels", f"{ct} *d_dist", "uint64_t *d_counts",
            "double *d_inertia", "uint64_t *d_iterations", "double *d_shift2", "void *stream"]
    assert _decl(hdr, "pn_kmeans_bounds_f32") == ["const pn_index *index", "const float *centres", "size_t nc",
                                                  "double *bounds_out"]
    # the option that forces the filter, in the header and in the Python table
    assert re.search(r"\bPN_OPT_KMEANS_FILTER\s*=\s*16\b", hdr) and _lib.PN_OPT_KMEANS_FILTER == 16
    assert "PN_OPT_KMEANS_FILTER. */" in head
    # the contract is stated above the declarations
    for phrase in (r"pn_mean_shift_labels_\*\(centres, nc, h, flags = 0\)", r"SUM4096", r"segments of 4096 terms",
                   r"P_l = \(\(\(0\.0 \+ t_l\) \+ t_\(l\+64\)\) \+ \.\.\.\)", r"\(\(S_0 \+ S_1\) \+ S_2\)",
                   r"no\s+\*?\s*floating-point atomics", r"ascending row index", r"the centre is unchanged",
                   r"\(T\)\(S / \(double\)m_c\)", r"column col to partial col mod 64",
                   r"shift2 = \(\(\(0\.0 \+ t_0\) \+ t_1\) \+ \.\.\.\) in centre order", r"shift2 <= tol",
                   r"t == max_iter", r"one more assignment to the final centres", r"PN_OPT_INDEX_BASE affects no output",
                   r"pn_stats\.queries advances by n per assignment", r"pn_stats\.fallback_queries",
                   r"BLOCKS THE HOST ONCE PER ITERATION", r"pn_kmeans_assign_device_\* never waits",
                   r"a Cosine index:\s+\*?\s*PN_ERR_UNSUPPORTED", r"4 \* dp \+ 32 bytes per row",
                   r"Not in this version: Cosine / spherical k-means, row-sharded handles, mini-batch"):
        assert re.search(phrase, hdr), phrase


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)(1, 1, 1, 1, 1, 1, 1, 1)
    p = C.addressof(buf)
    nan = float("nan")

    def host(fl, tol, mi, cout, labels, init, nc):
        return getattr(L, f"pn_kmeans_{sfx}")(None, init, nc, tol, mi, fl, cout, labels, None, None, None, None, None)

    def dev(fl, tol, mi, cout, labels, init, nc):
        return getattr(L, f"pn_kmeans_device_{sfx}")(None, init, nc, tol, mi, fl, cout, labels, None, None, None, None, None,
                                                    None)

    for call in (host, dev):
        # 1. unknown flags come first, whatever else is wrong (k-means has no flags)
        for flags in (1, 2, 4, 8, 0x80000000):
            assert call(flags, -1.0, 0, None, None, None, 0) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        # 2. tol
        for tol in (-1.0, -1e-300, nan):
            assert call(0, tol, 0, None, None, None, 0) == _lib.PN_ERR_INVALID
            assert "tol" in _lib.last_error()
        # 3. max_iter
        assert call(0, 0.0, 0, None, None, None, 0) == _lib.PN_ERR_INVALID
        assert "max_iter" in _lib.last_error()
        # 4. the required outputs
        for cout in (None, p):
            assert call(0, 0.0, 1, cout, None, None, 0) == _lib.PN_ERR_INVALID
            assert "labels is NULL" in _lib.last_error()
        assert call(0, 0.0, 1, None, p, None, 0) == _lib.PN_ERR_INVALID
        assert "centres_out is NULL" in _lib.last_error()
        # 5. the inputs
        for nc in (0, 2):
            assert call(0, 0.0, 1, p, p, None, nc) == _lib.PN_ERR_INVALID
            assert "centres is NULL" in _lib.last_error()
        # 6. nc == 0
        assert call(0, 0.0, 1, p, p, p, 0) == _lib.PN_ERR_INVALID
        assert "at least one centre" in _lib.last_error()
        # 7. the handle (the optional outputs may all be NULL)
        assert call(0, 0.0, 1, p, p, p, 2) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
        assert call(0, 1e300, 2 ** 40, p, p, p, 1) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()

    # assignment: flags, the output, the input, the handle; nc == 0 is allowed
    for name, extra in ((f"pn_kmeans_assign_{sfx}", ()), (f"pn_kmeans_assign_device_{sfx}", (None,))):
        f = getattr(L, name)
        for flags in (1, 4, 8):
            assert f(None, None, 2, flags, None, None, None, *extra) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        assert f(None, None, 2, 0, None, p, p, *extra) == _lib.PN_ERR_INVALID
        assert "labels is NULL" in _lib.last_error()
        assert f(None, None, 2, 0, p, None, None, *extra) == _lib.PN_ERR_INVALID
        assert "centres is NULL" in _lib.last_error()
        for nc, c in ((2, p), (0, None)):
            assert f(None, c, nc, 0, p, None, None, *extra) == _lib.PN_ERR_INVALID
            assert "index is NULL" in _lib.last_error()
    if sfx == "f32":
        f = L.pn_kmeans_bounds_f32
        assert f(None, p, 2, None) == _lib.PN_ERR_INVALID and "bounds_out is NULL" in _lib.last_error()
        assert f(None, None, 2, p) == _lib.PN_ERR_INVALID and "centres is NULL" in _lib.last_error()
        assert f(None, p, 2, p) == _lib.PN_ERR_INVALID and "index is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    sig = {name: list(inspect.signature(getattr(bt, name)).parameters)[1:] for name in (
        "kmeans", "kmeans_assign", "kmeans_device", "kmeans_assign_device", "kmeans_plusplus", "kmeans_bounds")}
    assert sig["kmeans"][:4] == ["centres_or_k", "tol", "max_iter", "seed"]
    assert sig["kmeans_assign"] == ["centres"]
    assert sig["kmeans_assign_device"][0] == "centres" and sig["kmeans_device"][:3] == ["centres", "abs_tol", "max_iter"]
    assert sig["kmeans_plusplus"] == ["k", "seed"]
    d = inspect.signature(bt.kmeans).parameters
    assert (d["tol"].default, d["max_iter"].default, d["seed"].default) == (1e-4, 300, None)
    assert "NOT" in bt.kmeans_plusplus.__doc__ and "bit-contractual" in bt.kmeans_plusplus.__doc__
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake._dim, fake.device = "f32", np.dtype(np.float32), 10, 4, 0
    fake.metric = pn.distance.Euclidean()
    fake.points = np.zeros((10, 4), dtype=np.float32)
    c = np.zeros((3, 4), dtype=np.float32)
    for kw in ({"tol": -1.0}, {"tol": float("nan")}, {"max_iter": 0}, {"max_iter": -3}, {"abs_tol": -1.0}):
        with pytest.raises(ValueError):
            fake.kmeans(c, **kw)
    # the centres have the tree's columns, and there is at least one
    for bad in (np.zeros((3, 3), dtype=np.float32), np.zeros((3, 5), dtype=np.float32), np.zeros(4, dtype=np.float32)):
        with pytest.raises(ValueError):
            fake.kmeans(bad)
        with pytest.raises(ValueError):
            fake.kmeans_assign(bad)
    with pytest.raises(ValueError):
        fake.kmeans(np.zeros((0, 4), dtype=np.float32))
    for k in (0, -1, 11):
        with pytest.raises(ValueError):
            fake.kmeans_plusplus(k, 0)
    # the device methods take CUDA tensors only
    with pytest.raises(ValueError):
        fake.kmeans_assign_device(c)
    with pytest.raises(ValueError):
        fake.kmeans_device(c, 0.0)
    # a tree built from a device tensor has no rows on the host to scale tol by
    fake.points = None
    with pytest.raises(ValueError):
        fake.kmeans(c)
    # Euclidean trees only
    fake.points = np.zeros((10, 4), dtype=np.float32)
    fake.metric = pn.distance.Cosine()
    for call in (lambda: fake.kmeans(c), lambda: fake.kmeans_assign(c), lambda: fake.kmeans_plusplus(2, 0),
                 lambda: fake.kmeans_assign_device(c), lambda: fake.kmeans_device(c, 0.0)):
        with pytest.raises(ValueError):
            call()


def test_cpp_mirror_compiles_with_kmeans(tmp_path):
    src = tmp_path / "km.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "size_t f(const petal::BallTree<float> &t, const float *c) {\n"
                   "    petal::KMeans<float> a = t.kmeans_assign(c, 3);\n"
                   "    petal::KMeans<float> b = t.kmeans(c, 3, 1e-4, 10);\n"
                   "    const std::vector<int64_t> &l = b.labels;\n"
                   "    return a.labels.size() + b.counts[0] + b.n_iter + l.size() + (size_t)(a.inertia + b.shift2 + b.dist[0]);\n}\n"
                   "double g(const petal::BallTree<double> &t, const double *c) {\n"
                   "    petal::KMeans<double> a = t.kmeans(c, 2, 0.0);\n"
                   "    return a.centres[0] + a.inertia + t.kmeans_assign(c, 2).dist[0];\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_kmeans_kernels_are_built_and_do_not_spill():
    """kmeans.hip is a unit of the build, compiled with -ffp-contract=off; none of its kernels spills or uses scratch, and
    the filter kernel contracts on the matrix cores"""
    import importlib.util as u
    spec = u.spec_from_file_location("pn_build", os.path.join(ROOT, "petal-neighbors_amd", "build.py"))
    b = u.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("kmeans.hip", ["-ffp-contract=off"]) in b.UNITS
    b.build(keep_asm=("kmeans",))
    text = open(os.path.join(ROOT, "petal-neighbors_amd", "build", "kmeans.s")).read()
    names = re.findall(r"\.name:\s+(_Z\S*km_assign_filter_kernel\S*)", text)
    assert len(names) == 4, names  # the filter and its diagnostic twin, four and two waves per workgroup
    assert len(re.findall(r"\.name:\s+(_Z\S*km_segment_sums_kernel\S*)", text)) == 4  # f32 and f64, 8 and 16 columns
    assert "v_mfma_f32_32x32x16_bf16" in text
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    spills += [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) >= 20 and not any(spills) and not any(scratch), (spills, scratch)
