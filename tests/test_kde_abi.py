"""CPU-side checks of pn_kde_* (no GPU compute calls): the eight symbols are declared with the stated signatures, listed in
the ctypes table, exported and present in the Rust extern block, the ABI version is still 3; PN_OPT_KDE_PIECE and the five
kernel constants are in the header; the header states the contract; bad arguments fail in the documented order -- flags,
kernel, atol, NULL outputs, NULL inputs, n_h, NULL index -- before any device is touched; the Python methods exist and
raise ValueError on bad bandwidths, tolerances, kernel names and array lengths; the C++ mirror compiles; the five
normalisers agree with scikit-learn's."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FAMILIES = ["kde", "kde_device", "kde_self", "kde_self_device"]
NAMES = [f"pn_{fam}_{sfx}" for fam in FAMILIES for sfx in ("f32", "f64")]
KERNELS = {"gaussian": 0, "tophat": 1, "epanechnikov": 2, "exponential": 3, "linear": 4}


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
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in exported, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
    assert _lib.lib().pn_abi_version() == 3
    tail = ["int kernel", "double atol", "unsigned flags"]
    for sfx, ct in (("f32", "float"), ("f64", "double")):
        assert _decl(hdr, f"pn_kde_{sfx}") == [
            "const pn_index *index", f"const {ct} *queries", "size_t nq", "size_t q_cols", "ptrdiff_t q_row_stride",
            f"const {ct} *h", "size_t n_h"] + tail + ["double *sum_out", "uint64_t *count_out", f"{ct} *cutoff_out"]
        assert _decl(hdr, f"pn_kde_device_{sfx}") == [
            "const pn_index *index", f"const {ct} *d_queries", "size_t nq", "size_t q_cols", "size_t q_row_stride",
            f"const {ct} *d_h", "size_t n_h"] + tail + ["double *d_sum", "uint64_t *d_count", f"{ct} *d_cutoff", "void *stream"]
        assert _decl(hdr, f"pn_kde_self_{sfx}") == [
            "const pn_index *index", f"const {ct} *h", "size_t n_h"] + tail + [
            "double *sum_out", "uint64_t *count_out", f"{ct} *cutoff_out"]
        assert _decl(hdr, f"pn_kde_self_device_{sfx}") == [
            "const pn_index *index", f"const {ct} *d_h", "size_t n_h"] + tail + [
            "double *d_sum", "uint64_t *d_count", f"{ct} *d_cutoff", "void *stream"]
        # the ctypes table has one entry per C parameter
        for fam in FAMILIES:
            assert len(_lib.SIGNATURES[f"pn_{fam}_{sfx}"][1]) == len(_decl(hdr, f"pn_{fam}_{sfx}")), fam
    # the option and the kernels, in the header and in the Python table
    assert re.search(r"\bPN_OPT_KDE_PIECE\s*=\s*14\b", hdr) and _lib.PN_OPT_KDE_PIECE == 14
    for name, num in KERNELS.items():
        assert re.search(r"\bPN_KDE_" + name.upper() + r"\s*=\s*%d\b" % num, hdr), name
        assert getattr(_lib, "PN_KDE_" + name.upper()) == num
    # the contract is stated above the declarations
    for phrase in (r"lane partial P_l = \(\.\.\.\(\(0\.0 \+ t_l\) \+ t_\{l\+64\}\) \+ t_\{l\+128\} \.\.\.\)",
                   r"S = \(\.\.\.\(\(P_0 \+ P_1\) \+ P_2\) \.\.\. \+ P_63\)", r"S_all - atol <= S <= S_all",
                   r"d = max\(\(double\)dist, \+0\.0\)", r"ascending row index", r"1\.0 \+ 2\^-30", r"BLOCKS\s+\*?\s*THE HOST ONCE"):
        assert re.search(phrase, hdr), phrase


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)(1, 1, 1, 1, 1, 1, 1, 1)
    p = C.addressof(buf)

    def q_host(fl, kern, atol, s, c, q, h, n_h, nq=2):
        return getattr(L, f"pn_kde_{sfx}")(None, q, nq, 2, 2, h, n_h, kern, atol, fl, s, c, None)

    def q_dev(fl, kern, atol, s, c, q, h, n_h, nq=2):
        return getattr(L, f"pn_kde_device_{sfx}")(None, q, nq, 2, 2, h, n_h, kern, atol, fl, s, c, None, None)

    def s_host(fl, kern, atol, s, c, q, h, n_h, nq=2):
        return getattr(L, f"pn_kde_self_{sfx}")(None, h, n_h, kern, atol, fl, s, c, None)

    def s_dev(fl, kern, atol, s, c, q, h, n_h, nq=2):
        return getattr(L, f"pn_kde_self_device_{sfx}")(None, h, n_h, kern, atol, fl, s, c, None, None)

    for call, self_entry in ((q_host, False), (q_dev, False), (s_host, True), (s_dev, True)):
        # 1. unknown flags come first, whatever else is wrong (PN_SELF_INCLUDE = 2 belongs to the self entries alone)
        for flags in (1, 4, 0x80000000) + (() if self_entry else (2,)):
            assert call(flags, 9, -1.0, None, None, None, None, 7) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        # 2. the kernel
        for kern in (-1, 5, 6):
            assert call(0, kern, -1.0, None, None, None, None, 7) == _lib.PN_ERR_INVALID
            assert "kernel" in _lib.last_error()
        # 3. atol
        for atol in (-1.0, float("nan"), float("inf")):
            assert call(0, 0, atol, None, None, None, None, 7) == _lib.PN_ERR_INVALID
            assert "atol" in _lib.last_error()
        # 4. the outputs: one of sum and count is enough
        assert call(0, 0, 0.0, None, None, None, None, 7) == _lib.PN_ERR_INVALID
        assert "both NULL" in _lib.last_error()
        # 5. the inputs
        for s, c in ((p, None), (None, p), (p, p)):
            if not self_entry:
                assert call(0, 0, 0.0, s, c, None, p, 7) == _lib.PN_ERR_INVALID
                assert "queries is NULL" in _lib.last_error()
            assert call(0, 0, 0.0, s, c, p, None, 7) == _lib.PN_ERR_INVALID
            assert "h is NULL" in _lib.last_error()
        # 6. n_h (the self entries learn the number of rows from the handle: they name the handle first)
        if not self_entry:
            for n_h in (0, 3, 7):
                assert call(0, 0, 0.0, p, p, p, p, n_h) == _lib.PN_ERR_INVALID
                assert "n_h" in _lib.last_error()
            # nq = 0: the inputs are not looked at; n_h and the handle are
            assert call(0, 0, 0.0, p, p, None, None, 2, nq=0) == _lib.PN_ERR_INVALID
            assert "n_h" in _lib.last_error()
            assert call(0, 0, 0.0, p, p, None, None, 1, nq=0) == _lib.PN_ERR_INVALID
            assert "index is NULL" in _lib.last_error()
        # 7. the handle
        for n_h in (1, 2):
            assert call(0, 4, 1.0, p, p, p, p, n_h) == _lib.PN_ERR_INVALID
            assert "index is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    sig = {name: list(inspect.signature(getattr(bt, name)).parameters)[1:] for name in (
        "kernel_density", "kernel_density_self", "kernel_density_device", "kernel_density_self_device",
        "query_radius_count", "two_point_correlation")}
    assert sig["kernel_density"] == ["queries", "h", "kernel", "atol", "return_log", "normalize"]
    assert sig["kernel_density_self"] == ["h", "kernel", "atol", "return_log", "normalize", "include_self"]
    assert sig["kernel_density_device"] == ["queries", "h", "kernel", "atol", "out_sum", "out_count", "out_cutoff", "stream"]
    assert sig["kernel_density_self_device"] == ["h", "kernel", "atol", "include_self", "out_sum", "out_count", "out_cutoff",
                                                 "stream"]
    assert sig["query_radius_count"] == ["queries", "r"] and sig["two_point_correlation"] == ["queries", "r"]
    d = inspect.signature(bt.kernel_density).parameters
    assert (d["kernel"].default, d["atol"].default, d["return_log"].default, d["normalize"].default) == (
        "gaussian", 0.0, False, True)
    assert inspect.signature(bt.kernel_density_self).parameters["include_self"].default is False
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake._dim, fake.device = "f32", np.dtype(np.float32), 10, 4, 0
    fake.metric = pn.distance.Euclidean()
    q = np.zeros((3, 4), dtype=np.float32)
    for h in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fake.kernel_density(q, h)
        with pytest.raises(ValueError):
            fake.kernel_density_self(h)
        with pytest.raises(ValueError):
            fake.kernel_density_self_device(h)
    for atol in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fake.kernel_density(q, 0.5, atol=atol)
        with pytest.raises(ValueError):
            fake.kernel_density_self(0.5, atol=atol)
        with pytest.raises(ValueError):
            fake.kernel_density_self_device(0.5, atol=atol)
    for kernel in ("cosine", "Gaussian", "", None):
        with pytest.raises(ValueError):
            fake.kernel_density(q, 0.5, kernel=kernel)
        with pytest.raises(ValueError):
            fake.kernel_density_self(0.5, kernel=kernel)
        with pytest.raises(ValueError):
            fake.kernel_density_self_device(0.5, kernel=kernel)
    # one bandwidth per query / per row, of the tree's dtype
    for h in (np.ones(2, dtype=np.float32), np.ones(4, dtype=np.float32), np.ones((3, 1), dtype=np.float32),
              np.ones(3, dtype=np.float64)):
        with pytest.raises(ValueError):
            fake.kernel_density(q, h)
        with pytest.raises(ValueError):
            fake.query_radius_count(q, h)
    for h in (np.ones(9, dtype=np.float32), np.ones(11, dtype=np.float32)):
        with pytest.raises(ValueError):
            fake.kernel_density_self(h)
    # the device methods take CUDA tensors only
    with pytest.raises(ValueError):
        fake.kernel_density_device(q, 0.5)
    with pytest.raises(ValueError):
        fake.kernel_density_self_device(np.ones(10, dtype=np.float32))
    for name, dt in (("out_sum", np.float64), ("out_count", np.int64), ("out_cutoff", np.float32)):
        with pytest.raises(ValueError):
            fake.kernel_density_self_device(0.5, **{name: np.empty(10, dtype=dt)})
    with pytest.raises(ValueError):
        fake.two_point_correlation(q, 0.5)  # r is a 1-D array
    # the normalisers are volumes of Euclidean balls
    fake.metric = pn.distance.Cosine()
    with pytest.raises(ValueError):
        fake.kernel_density(q, 0.5)
    with pytest.raises(ValueError):
        fake.kernel_density_self(0.5, kernel="tophat", normalize=True)


def test_cpp_mirror_compiles_with_kde(tmp_path):
    src = tmp_path / "kde.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "size_t f(const petal::BallTree<float> &t, const float *q, const float *h) {\n"
                   "    petal::Kde<float> a = t.kernel_density(q, 7, 0.5f);\n"
                   "    petal::Kde<float> b = t.kernel_density(q, 7, h, 7, PN_KDE_EPANECHNIKOV, 1e-3);\n"
                   "    petal::Kde<float> c = t.kernel_density_self(0.5f, PN_KDE_LINEAR, 0.0, true);\n"
                   "    std::vector<size_t> n = t.query_radius_count(q, 7, 0.25f);\n"
                   "    return a.sum.size() + b.count.size() + c.cutoff.size() + n.size();\n}\n"
                   "double g(const petal::BallTree<double> &t, const double *q) {\n"
                   "    petal::Kde<double> a = t.kernel_density(q, 1, 0.5, PN_KDE_EXPONENTIAL, 1e-6);\n"
                   "    const std::vector<double> &c = a.cutoff;\n"
                   "    return a.sum[0] + c[0] + (double)t.kernel_density_self(0.5).count[0];\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_normalisers_agree_with_scikit_learn(pn, dim):
    """The normaliser alone: scikit-learn's log density minus the log of the numpy-summed terms over the same f64
    distances, against kde_log_norm - log(n).  Within 1e-9 in log (measured: 2.7e-10 at the worst on sums of thousands of
    terms); the margin is for lgamma / log and the summation order of 50 terms."""
    try:
        from sklearn.neighbors import KernelDensity
    except Exception as e:  # noqa: BLE001
        pytest.skip(f"scikit-learn does not import: {e}")
    from petal_neighbors_amd.ball_tree import kde_log_norm
    rng = np.random.default_rng(0x4DE + dim)
    x = rng.random((50, dim))
    q = rng.random((20, dim))
    h = 0.75  # (wide enough that no compact kernel gives an empty sum)
    d = np.sqrt(((q[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    terms = {"gaussian": np.exp(-(d * d) / (2.0 * h * h)), "tophat": (d < h).astype(np.float64),
             "epanechnikov": np.where(d < h, 1.0 - (d * d) / (h * h), 0.0), "exponential": np.exp(-d / h),
             "linear": np.where(d < h, 1.0 - d / h, 0.0)}
    for kernel, t in terms.items():
        s = t.sum(axis=1)
        assert (s > 0).all(), kernel
        sk = KernelDensity(bandwidth=h, kernel=kernel, algorithm="ball_tree", atol=0, rtol=0).fit(x).score_samples(q)
        want = sk - np.log(s) + np.log(len(x))
        got = float(kde_log_norm(kernel, dim, h))
        assert np.abs(want - got).max() <= 1e-9, (kernel, dim, float(np.abs(want - got).max()))


def test_kde_kernels_are_built_and_do_not_spill():
    """kde.hip is a unit of the build, compiled with -ffp-contract=off; none of its kernels spills or uses scratch"""
    import importlib.util as u
    spec = u.spec_from_file_location("pn_build", os.path.join(ROOT, "petal-neighbors_amd", "build.py"))
    b = u.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("kde.hip", ["-ffp-contract=off"]) in b.UNITS
    b.build(keep_asm=("kde",))
    text = open(os.path.join(ROOT, "petal-neighbors_amd", "build", "kde.s")).read()
    names = re.findall(r"\.name:\s+(_Z\S*kde_sum_kernel\S*)", text)
    assert len(names) == 2, names  # f32 and f64
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    spills += [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) >= 5 and not any(spills) and not any(scratch), (spills, scratch)
