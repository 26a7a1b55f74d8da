"""Static audit of the paired main-pass kernel (bf16_filter_kernel_pair) from the code object's notes (CPU only): an
instantiation for every KS of both layouts, each within 256 VGPRs -- two waves per SIMD in one 8-wave workgroup --
without spills or scratch."""
import os
import re
import shutil
import subprocess

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"


def _kernel_notes(tmp_path):
    import importlib.util as u
    spec = u.spec_from_file_location("pn_build", os.path.join(ROOT, "petal-neighbors_amd", "build.py"))
    b = u.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    work = tmp_path / "bf16_filter.o"
    shutil.copy(os.path.join(ROOT, "petal-neighbors_amd", "build", "bf16_filter.o"), work)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(work)], check=True, capture_output=True,
                   cwd=tmp_path)
    co = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert len(co) == 1, co
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / co[0])], check=True,
                          capture_output=True, text=True).stdout
    out = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                     for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                               "max_flat_workgroup_size")}
    return out


def test_paired_kernel_has_every_instantiation_within_its_register_budget(tmp_path):
    notes = {n: v for n, v in _kernel_notes(tmp_path).items() if "bf16_filter_kernel_pair" in n}
    seen = set()
    for name, v in notes.items():
        m = re.search(r"bf16_filter_kernel_pairILi(\d+)ELb([01])EEE", name)
        assert m, name
        seen.add((int(m.group(1)), bool(int(m.group(2)))))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= 256, (name, v)
        assert v["max_flat_workgroup_size"] == 512, (name, v)
    # norm-in-the-accumulator layout: KS 2 .. 8; five extra columns: KS 2 .. 9 (launch_bf16_filter)
    want = {(ks, True) for ks in range(2, 9)} | {(ks, False) for ks in range(2, 10)}
    assert seen == want, sorted(want ^ seen)
