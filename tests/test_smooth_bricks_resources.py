"""CPU (cross-compile only): the brick-layout kernels of the export smoothing (csrc/mesh_smooth.hip)
compile for gfx950 with no scratch, no spills and at most 128 VGPRs, and the staged iteration keeps
its LDS (the 12^3 tile of doubles, 144 presence words, the 256-entry table of the byte-coded bounds:
16 448 bytes) within 18 KB, so that the eight 256-thread workgroups a CU's wave slots admit (at most
64 VGPRs: eight waves per SIMD) also fit its 160 KB of LDS."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
isa = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa)

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and not shutil.which("hipcc"),
                                reason="hipcc not available")

ITERATION = [f"smooth_brick_kernel<{c},{d},256>" for c in (0, 1) for d in (0, 1)]
NEW = ITERATION + ["smooth_brick_energy_kernel", "brick_flag_kernel", "brick_gather_kernel",
                   "brick_scatter_kernel"]


@pytest.fixture(scope="module")
def kernels():
    txt = isa.compile_asm(os.path.join(isa.CSRC, "mesh_smooth.hip"))
    md = isa.metadata(txt)
    out = {}
    for name, body in isa.bodies(txt):
        ops = [ln.split()[0] for ln in body if ln[:1] in " \t" and ln.split()]
        out[isa.demangle_short(name)] = (md[name], ops)
    return out


def test_every_new_kernel_is_there(kernels):
    assert set(NEW) <= set(kernels), sorted(kernels)


@pytest.mark.parametrize("name", NEW)
def test_no_scratch_no_spills_and_at_most_128_vgprs(kernels, name):
    md, ops = kernels[name]
    assert md["scratch"] == 0 and md["vspill"] == 0 and md["sspill"] == 0, md
    assert sum(o.startswith("scratch_") for o in ops) == 0
    assert md["vgpr"] + md["agpr"] <= 128, md
    if name.startswith("smooth_brick_kernel") and ",0,256>" in name:
        assert md["vgpr"] + md["agpr"] <= 64, md          # eight waves per SIMD


@pytest.mark.parametrize("name", ITERATION + ["smooth_brick_energy_kernel"])
def test_lds_of_the_staged_kernels(kernels, name):
    md, _ = kernels[name]
    staged = ",1,256>" not in name
    assert md["lds"] <= 18 * 1024, md
    assert (md["lds"] >= 12 * 12 * 12 * 8) == staged, md
