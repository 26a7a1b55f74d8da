"""CPU-side checks of csrc/km_filter.h, the code the small MFMA filters share (kmeans.hip, kmeans_nearest.hip,
spherical_kmeans.hip, foreign.hip): the MFMA chain, the exact-side helpers and the proof's tau' are written once, in the
header; the launchers of an assignment are one family; and none of the four units' kernels spills or uses scratch."""
import importlib.util as u
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "petal-neighbors_amd", "csrc")
UNITS = ("kmeans", "kmeans_nearest", "spherical_kmeans", "foreign")
MFMA = "__builtin_amdgcn_mfma_f32_32x32x16_bf16"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _build_module():
    spec = u.spec_from_file_location("pn_build", os.path.join(ROOT, "petal-neighbors_amd", "build.py"))
    b = u.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_the_chain_and_the_proof_are_written_once():
    hdr = _src("km_filter.h")
    assert hdr.count(MFMA) == 3  # one chain: a . b, a . bl, al . b
    assert '#include "km_pack.h"' in hdr
    for helper in ("km_mfma_chain", "km_load_row_tile", "km_gather_row_tile", "km_sqrt", "km_dist_key", "km_stage_rows",
                   "km_proof_rhs", "km_tau_floor", "km_euclid_push_down", "km_zero_kernel", "km_lds_fence"):
        assert re.search(r"\b" + helper + r"\b", hdr), helper
    for unit in UNITS:
        text = _src(unit + ".hip")
        assert '#include "km_filter.h"' in text, unit
        assert MFMA not in text, unit
        assert "km_mfma_chain(" in text, unit
        # no definition of a helper of its own: a name with one of these endings is only ever the header's, called
        for m in re.finditer(r"\b(\w+_(?:stage_rows|proof_rhs|sqrt|zero_kernel|lds_fence))\b", text):
            assert m.group(1).startswith("km_"), (unit, m.group(1))
        assert not re.search(r"__device__[^;{]*\bkm_(stage_rows|proof_rhs|sqrt|tau_floor|euclid_push_down)\s*\(", text), unit
        assert not re.search(r"__global__[^;{]*\b\w+_zero_kernel\s*\(", text), unit
        # tau' = xn + tau - E and its 2^-49: the header's expression alone
        assert "1.7763568394002505e-15" not in text, unit
        assert not re.search(r"\(\s*xnr?\s*\+\s*\(double\)\s*\w+\s*\)\s*-\s*slack", text), unit
        assert "typedef" not in text or "ext_vector_type" not in text, unit
    assert _src("km_filter.h").count("1.7763568394002505e-15") == 1


def test_one_launcher_family():
    internal = _src("pn_internal.h")
    assert "launch_skm_" not in internal and "skm_update_enqueue" not in internal
    for name in ("launch_km_pack_rows", "launch_km_pack_centres", "launch_km_rerank", "launch_km_exact", "km_update_enqueue"):
        assert re.search(r"template <typename T, bool SPH[^>]*>\s*hipError_t " + name + r"\(", internal), name
    index = _src("index.hip")
    assert "launch_skm_" not in index and "skm_update_enqueue" not in index
    # one chain on the host: each launcher of an assignment is called once for the filter path
    body = index[index.index("static int km_assign_enqueue("):index.index("static int km_assign_device(")]
    for name in ("launch_km_pack_centres", "launch_km_filter", "launch_km_rerank"):
        assert body.count(name) == 1, name
    assert body.count("launch_km_exact") == 2  # behind the filter, and alone
    # nsel and cc are cleared by the launchers, by a kernel: no memset of them in the host chains
    nearest = index[index.index("static int kn_enqueue("):index.index("static int kn_device(")]
    assert "hipMemsetAsync" not in body and "hipMemsetAsync" not in nearest
    for unit in UNITS:
        assert "hipMemsetAsync" not in _src(unit + ".hip"), unit
    assert "hipMemsetAsync" not in _src("km_filter.h")
    assert os.path.join(CSRC, "km_filter.h") in _build_module().HEADERS


@pytest.mark.parametrize("unit", UNITS)
def test_kernels_do_not_spill(unit):
    """No kernel of the unit spills a register, vector or scalar, or uses scratch."""
    b = _build_module()
    assert (unit + ".hip", ["-ffp-contract=off"]) in b.UNITS
    b.build(keep_asm=UNITS)
    text = open(os.path.join(ROOT, "petal-neighbors_amd", "build", unit + ".s")).read()
    assert "v_mfma_f32_32x32x16_bf16" in text
    names = re.findall(r"\.name:\s+(_Z\S+)", text)
    vs = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    ss = [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(names) == len(vs) == len(ss) == len(scratch) >= 10
    bad = [(n, a, b_, c) for n, a, b_, c in zip(names, vs, ss, scratch) if a or b_ or c]
    print(unit, len(names), "kernels; spilling:", bad)
    assert not bad, bad
