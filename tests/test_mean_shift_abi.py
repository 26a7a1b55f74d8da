"""CPU-side checks of pn_mean_shift_* (no GPU compute calls): the twelve symbols are declared with the stated signatures,
listed in the ctypes table, exported and present in the Rust extern block, the ABI version is still 3; PN_OPT_MS_PIECE and
the two flags are in the header and in the Python table; the header states the contract; bad arguments fail in the
documented order -- flags, tol, max_iter, NULL outputs, NULL inputs, n_h, s_cols, NULL index -- before any device is
touched; the Python methods exist and raise ValueError; the C++ mirror compiles; the kernels are built unfused and do
not spill; mean_shift_bin_seeds gives scikit-learn's bins."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FAMILIES = ["mean_shift", "mean_shift_device", "mean_shift_merge", "mean_shift_merge_device", "mean_shift_labels",
            "mean_shift_labels_device"]
NAMES = [f"pn_{fam}_{sfx}" for fam in FAMILIES for sfx in ("f32", "f64")]


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
    assert len(NAMES) == 12
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in exported, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
    assert _lib.lib().pn_abi_version() == 3
    for sfx, ct in (("f32", "float"), ("f64", "double")):
        mid = ["size_t n_h", "double tol", "size_t max_iter", "unsigned flags"]
        assert _decl(hdr, f"pn_mean_shift_{sfx}") == [
            "const pn_index *index", f"const {ct} *seeds", "size_t ns", "size_t s_cols", "ptrdiff_t s_row_stride",
            f"const {ct} *h"] + mid + [f"{ct} *modes_out", "uint64_t *points_within_out", "uint32_t *iterations_out",
                                      "double *shift_out", "uint64_t *work"]
        assert _decl(hdr, f"pn_mean_shift_device_{sfx}") == [
            "const pn_index *index", f"const {ct} *d_seeds", "size_t ns", "size_t s_cols", "size_t s_row_stride",
            f"const {ct} *d_h"] + mid + [f"{ct} *d_modes", "uint64_t *d_points_within", "uint32_t *d_iterations",
                                        "double *d_shift", "uint64_t *work", "void *stream"]
        assert _decl(hdr, f"pn_mean_shift_merge_{sfx}") == [
            "const pn_index *index", f"const {ct} *modes", "size_t ns", "const uint64_t *points_within", f"{ct} h",
            "unsigned flags", f"{ct} *centres_out", "uint64_t *centre_points_out", "int64_t *centre_of_seed_out",
            "uint64_t *n_centres_out"]
        assert _decl(hdr, f"pn_mean_shift_merge_device_{sfx}") == [
            "const pn_index *index", f"const {ct} *d_modes", "size_t ns", "const uint64_t *d_points_within", f"{ct} h",
            "unsigned flags", f"{ct} *d_centres", "uint64_t *d_centre_points", "int64_t *d_centre_of_seed",
            "uint64_t *d_n_centres", "void *stream"]
        assert _decl(hdr, f"pn_mean_shift_labels_{sfx}") == [
            "const pn_index *index", f"const {ct} *centres", "size_t nc", f"{ct} h", "unsigned flags", "int64_t *labels"]
        assert _decl(hdr, f"pn_mean_shift_labels_device_{sfx}") == [
            "const pn_index *index", f"const {ct} *d_centres", "size_t nc", f"{ct} h", "unsigned flags", "int64_t *d_labels",
            "void *stream"]
        for fam in FAMILIES:  # the ctypes table has one entry per C parameter
            assert len(_lib.SIGNATURES[f"pn_{fam}_{sfx}"][1]) == len(_decl(hdr, f"pn_{fam}_{sfx}")), fam
    # the option and the flags, in the header and in the Python table
    assert re.search(r"\bPN_OPT_MS_PIECE\s*=\s*15\b", hdr) and _lib.PN_OPT_MS_PIECE == 15
    assert re.search(r"#define\s+PN_MS_SEED_ROWS\s+4\b", hdr) and _lib.PN_MS_SEED_ROWS == 4
    m = re.search(r"#define\s+PN_MS_ORPHANS\s+(\d+)\b", hdr)
    assert m and int(m.group(1)) == _lib.PN_MS_ORPHANS
    # (the flag bits of the library do not collide)
    bits = [_lib.PN_RADIUS_SORTED, _lib.PN_SELF_INCLUDE, _lib.PN_MS_SEED_ROWS, _lib.PN_MS_ORPHANS]
    assert all(b and b & (b - 1) == 0 for b in bits) and len(set(bits)) == 4
    # the contract is stated above the declarations
    for phrase in (r"P_l = \(\.\.\.\(\(0\.0 \+ \(double\)x\[L_l\]\[c\]\) \+ \(double\)x\[L_\{l\+64\}\]\[c\]\) \+ \.\.\.\)",
                   r"S_c = \(\.\.\.\(\(P_0 \+ P_1\) \+ P_2\) \.\.\. \+ P_63\)", r"p'_c = \(T\)\(S_c / \(double\)m\)",
                   r"column c goes to partial c mod 64", r"ascending row index", r"shift <= tol or t == max_iter",
                   r"max_iter = 1 is exactly one step", r"never queried again", r"points_within descending, seed number ascending",
                   r"one 64-bit key", r"pn_euclidean_\*", r"lowest-numbered centre", r"PN_MS_ORPHANS", r"nc == 0 gives all -1",
                   r"BLOCKS THE HOST\s+\*?\s*TWICE PER ITERATION", r"Merge and labels\s+\*?\s*never wait",
                   r"a Cosine index: PN_ERR_UNSUPPORTED"):
        assert re.search(phrase, hdr), phrase


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_fail_in_order_before_the_device(pn, sfx):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)(1, 1, 1, 1, 1, 1, 1, 1)
    p = C.addressof(buf)
    nan = float("nan")

    def host(fl, tol, mi, modes, pw, seeds, h, n_h, s_cols=2, ns=2):
        return getattr(L, f"pn_mean_shift_{sfx}")(None, seeds, ns, s_cols, 2, h, n_h, tol, mi, fl, modes, pw, None, None, None)

    def dev(fl, tol, mi, modes, pw, seeds, h, n_h, s_cols=2, ns=2):
        return getattr(L, f"pn_mean_shift_device_{sfx}")(None, seeds, ns, s_cols, 2, h, n_h, tol, mi, fl, modes, pw, None,
                                                        None, None, None)

    for call in (host, dev):
        # 1. unknown flags come first, whatever else is wrong (PN_MS_ORPHANS belongs to the labels)
        for flags in (1, 2, 8, 0x80000000):
            assert call(flags, -1.0, 0, None, None, None, None, 7, 0) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        # 2. tol
        for tol in (-1.0, -1e-300, nan):
            assert call(0, tol, 0, None, None, None, None, 7, 0) == _lib.PN_ERR_INVALID
            assert "tol" in _lib.last_error()
        # 3. max_iter
        assert call(4, 0.0, 0, None, None, None, None, 7, 0) == _lib.PN_ERR_INVALID
        assert "max_iter" in _lib.last_error()
        # 4. the outputs
        for modes, pw in ((None, None), (p, None), (None, p)):
            assert call(0, 0.0, 1, modes, pw, None, None, 7, 0) == _lib.PN_ERR_INVALID
            assert "modes or points_within is NULL" in _lib.last_error()
        # 5. the inputs
        assert call(0, 0.0, 1, p, p, None, None, 7, 0) == _lib.PN_ERR_INVALID
        assert "seeds is NULL" in _lib.last_error()
        assert call(4, 0.0, 1, p, p, p, None, 7, 0) == _lib.PN_ERR_INVALID
        assert "seeds must be NULL" in _lib.last_error()
        for fl, seeds in ((0, p), (4, None)):
            assert call(fl, 0.0, 1, p, p, seeds, None, 7, 0) == _lib.PN_ERR_INVALID
            assert "h is NULL" in _lib.last_error()
        # 6. n_h (with PN_MS_SEED_ROWS the number of seeds comes from the handle: only 0 is wrong before it)
        for n_h in (0, 3, 7):
            assert call(0, 0.0, 1, p, p, p, p, n_h, 0) == _lib.PN_ERR_INVALID
            assert "n_h" in _lib.last_error()
        assert call(4, 0.0, 1, p, p, None, p, 0, 0) == _lib.PN_ERR_INVALID
        assert "n_h" in _lib.last_error()
        # 7. s_cols
        for n_h in (1, 2):
            assert call(0, 0.0, 1, p, p, p, p, n_h, 0) == _lib.PN_ERR_INVALID
            assert "s_cols" in _lib.last_error()
        # 8. the handle
        for fl, seeds, n_h in ((0, p, 1), (0, p, 2), (4, None, 1), (4, None, 5)):
            assert call(fl, 0.0, 1, p, p, seeds, p, n_h) == _lib.PN_ERR_INVALID
            assert "index is NULL" in _lib.last_error()

    # merge: flags, outputs, inputs, the handle
    for name, extra in ((f"pn_mean_shift_merge_{sfx}", ()), (f"pn_mean_shift_merge_device_{sfx}", (None,))):
        f = getattr(L, name)
        for flags in (1, 4, 8):
            assert f(None, None, 2, None, 1.0, flags, None, None, None, None, *extra) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        for c, nc in ((None, None), (p, None), (None, p)):
            assert f(None, None, 2, None, 1.0, 0, c, None, None, nc, *extra) == _lib.PN_ERR_INVALID
            assert "centres or n_centres is NULL" in _lib.last_error()
        for m, pw in ((None, None), (p, None), (None, p)):
            assert f(None, m, 2, pw, 1.0, 0, p, None, None, p, *extra) == _lib.PN_ERR_INVALID
            assert "modes or points_within is NULL" in _lib.last_error()
        assert f(None, p, 2, p, 1.0, 0, p, None, None, p, *extra) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
        assert f(None, None, 0, None, 1.0, 0, p, None, None, p, *extra) == _lib.PN_ERR_INVALID
        assert "index is NULL" in _lib.last_error()
    # labels: flags (PN_MS_ORPHANS is theirs), the output, the input, the handle
    for name, extra in ((f"pn_mean_shift_labels_{sfx}", ()), (f"pn_mean_shift_labels_device_{sfx}", (None,))):
        f = getattr(L, name)
        for flags in (1, 2, 4, 12):
            assert f(None, None, 2, 1.0, flags, None, *extra) == _lib.PN_ERR_INVALID
            assert "flags" in _lib.last_error()
        assert f(None, None, 2, 1.0, 8, None, *extra) == _lib.PN_ERR_INVALID
        assert "labels is NULL" in _lib.last_error()
        assert f(None, None, 2, 1.0, 8, p, *extra) == _lib.PN_ERR_INVALID
        assert "centres is NULL" in _lib.last_error()
        for nc, c in ((2, p), (0, None)):
            assert f(None, c, nc, 1.0, 0, p, *extra) == _lib.PN_ERR_INVALID
            assert "index is NULL" in _lib.last_error()


def test_python_methods_exist_and_validate(pn):
    bt = pn.BallTree
    sig = {name: list(inspect.signature(getattr(bt, name)).parameters)[1:] for name in (
        "mean_shift_modes", "mean_shift_modes_device", "mean_shift_merge", "mean_shift_merge_device", "mean_shift_labels",
        "mean_shift_labels_device", "mean_shift")}
    assert sig["mean_shift_modes"] == ["h", "seeds", "tol", "max_iter", "full"]
    assert sig["mean_shift_modes_device"][:4] == ["h", "seeds", "tol", "max_iter"]
    assert sig["mean_shift_merge"] == ["modes", "points_within", "h"]
    assert sig["mean_shift_merge_device"][:3] == ["modes", "points_within", "h"]
    assert sig["mean_shift_labels"] == ["centres", "h", "cluster_all"]
    assert sig["mean_shift_labels_device"][:3] == ["centres", "h", "cluster_all"]
    assert sig["mean_shift"] == ["h", "seeds", "cluster_all", "tol", "max_iter"]
    d = inspect.signature(bt.mean_shift_modes).parameters
    assert (d["seeds"].default, d["tol"].default, d["max_iter"].default, d["full"].default) == (None, None, 300, False)
    d = inspect.signature(bt.mean_shift).parameters
    assert (d["seeds"].default, d["cluster_all"].default, d["tol"].default, d["max_iter"].default) == (None, True, None, 300)
    assert inspect.signature(bt.mean_shift_labels).parameters["cluster_all"].default is True
    assert list(inspect.signature(pn.mean_shift_bin_seeds).parameters) == ["X", "bin_size", "min_bin_freq"]
    fake = bt.__new__(bt)
    fake._sfx, fake.dtype, fake._n, fake._dim, fake.device = "f32", np.dtype(np.float32), 10, 4, 0
    fake.metric = pn.distance.Euclidean()
    q = np.zeros((3, 4), dtype=np.float32)
    for kw in ({"tol": -1.0}, {"tol": float("nan")}, {"max_iter": 0}, {"max_iter": -3}):
        with pytest.raises(ValueError):
            fake.mean_shift_modes(0.5, q, **kw)
        with pytest.raises(ValueError):
            fake.mean_shift_modes(0.5, **kw)
        with pytest.raises(ValueError):
            fake.mean_shift(0.5, q, **kw)
        with pytest.raises(ValueError):
            fake.mean_shift_modes_device(0.5, **kw)
    # the seeds have the tree's columns; one bandwidth per seed has the seeds' length, the tree's dtype, and needs a tol
    for seeds in (np.zeros((3, 3), dtype=np.float32), np.zeros((3, 5), dtype=np.float32), np.zeros(4, dtype=np.float32)):
        with pytest.raises(ValueError):
            fake.mean_shift_modes(0.5, seeds)
    for h in (np.ones(2, dtype=np.float32), np.ones(4, dtype=np.float32), np.ones((3, 1), dtype=np.float32),
              np.ones(3, dtype=np.float64)):
        with pytest.raises(ValueError):
            fake.mean_shift_modes(h, q, tol=1e-3)
    with pytest.raises(ValueError):
        fake.mean_shift_modes(np.ones(3, dtype=np.float32), q)  # (no tol)
    with pytest.raises(ValueError):
        fake.mean_shift_modes(np.ones(9, dtype=np.float32), tol=1e-3)  # (seeds = rows: n bandwidths)
    with pytest.raises(ValueError):
        fake.mean_shift(np.ones(3, dtype=np.float32), q)
    # merge and labels take one bandwidth and arrays of the right shape
    pw = np.ones(3, dtype=np.uint64)
    for modes, p_, h in ((np.zeros((3, 3), dtype=np.float32), pw, 0.5), (q, np.ones(2, dtype=np.uint64), 0.5),
                         (q, pw, np.ones(3, dtype=np.float32)), (np.zeros(4, dtype=np.float32), pw, 0.5)):
        with pytest.raises(ValueError):
            fake.mean_shift_merge(modes, p_, h)
    for centres, h in ((np.zeros((2, 3), dtype=np.float32), 0.5), (np.zeros(4, dtype=np.float32), 0.5),
                       (np.zeros((2, 4), dtype=np.float32), np.ones(2, dtype=np.float32))):
        with pytest.raises(ValueError):
            fake.mean_shift_labels(centres, h)
    # the device methods take CUDA tensors only
    with pytest.raises(ValueError):
        fake.mean_shift_modes_device(0.5, q)
    with pytest.raises(ValueError):
        fake.mean_shift_merge_device(q, pw, 0.5)
    with pytest.raises(ValueError):
        fake.mean_shift_labels_device(q, 0.5)
    # Euclidean trees only
    fake.metric = pn.distance.Cosine()
    for call in (lambda: fake.mean_shift_modes(0.5, q), lambda: fake.mean_shift(0.5), lambda: fake.mean_shift_merge(q, pw, 0.5),
                 lambda: fake.mean_shift_labels(q, 0.5), lambda: fake.mean_shift_modes_device(0.5)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        pn.mean_shift_bin_seeds(np.zeros(5), 1.0)
    with pytest.raises(ValueError):
        pn.mean_shift_bin_seeds(np.zeros((5, 2)), -1.0)


def test_cpp_mirror_compiles_with_mean_shift(tmp_path):
    src = tmp_path / "ms.cpp"
    src.write_text('#include "petal_neighbors.hpp"\n'
                   "size_t f(const petal::BallTree<float> &t, const float *q) {\n"
                   "    petal::MeanShift<float> a = t.mean_shift(0.5f);\n"
                   "    petal::MeanShift<float> b = t.mean_shift_modes(0.5f, q, 7, 1e-3, 10);\n"
                   "    t.mean_shift_merge(b, 0.5f);\n"
                   "    t.mean_shift_labels(b, 0.5f, false);\n"
                   "    const std::vector<int64_t> &l = b.labels;\n"
                   "    return a.labels.size() + b.n_centres + b.centre_points.size() + b.seed_steps + l.size();\n}\n"
                   "double g(const petal::BallTree<double> &t) {\n"
                   "    petal::MeanShift<double> a = t.mean_shift(0.5, nullptr, 0, false, 1e-4, 5);\n"
                   "    return a.shift[0] + a.centres[0] + (double)a.centre_of_seed[0] + (double)a.iterations[0];\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_mean_shift_kernels_are_built_and_do_not_spill():
    """mean_shift.hip is a unit of the build, compiled with -ffp-contract=off; none of its kernels spills or uses
    scratch"""
    import importlib.util as u
    spec = u.spec_from_file_location("pn_build", os.path.join(ROOT, "petal-neighbors_amd", "build.py"))
    b = u.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert ("mean_shift.hip", ["-ffp-contract=off"]) in b.UNITS
    b.build(keep_asm=("mean_shift",))
    text = open(os.path.join(ROOT, "petal-neighbors_amd", "build", "mean_shift.s")).read()
    names = re.findall(r"\.name:\s+(_Z\S*ms_step_kernel\S*)", text)
    assert len(names) == 4, names  # f32 and f64, 8 and 16 columns per pass
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    spills += [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) >= 20 and not any(spills) and not any(scratch), (spills, scratch)


def test_bin_seeds_equal_scikit_learn():
    """mean_shift_bin_seeds against sklearn.cluster.get_bin_seeds as a set of rows, on 1500 x 2 blobs"""
    try:
        from sklearn.cluster import get_bin_seeds
        from sklearn.datasets import make_blobs
    except Exception as e:  # noqa: BLE001
        pytest.skip(f"scikit-learn does not import: {e}")
    import petal_neighbors_amd as pn
    X, _ = make_blobs(n_samples=1500, n_features=2, centers=[[1, 1], [-1, -1], [1, -1]], cluster_std=0.6, random_state=0)
    for bin_size, freq in ((0.7, 1), (0.7, 5), (0.31, 2), (2.5, 1)):
        want = get_bin_seeds(X, bin_size, freq)
        got = pn.mean_shift_bin_seeds(X, bin_size, freq)
        assert got.shape == want.shape and got.shape[0] < 1500, (bin_size, freq)
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist())), (bin_size, freq)
    assert pn.mean_shift_bin_seeds(X, 0) is X
