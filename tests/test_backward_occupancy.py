"""CPU (cross-compile only): the MLP part of the geometry backward (sdf_fd_bwd_pipe_kernel) fits two
waves per SIMD — at most 256 VGPR + AGPR per lane, no scratch, no spill — and two workgroups per CU
(at most 80 KB of LDS per 256-thread workgroup), so that the other drawings' kernels can share its CUs.
The 7-level instantiation (f32 layer 0) stays at one wave per SIMD but shares the LDS budget."""
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


@pytest.fixture(scope="module")
def pipe_kernels():
    txt = isa.compile_asm(os.path.join(isa.CSRC, "hashgrid_mfma.hip"))
    md = isa.metadata(txt)
    out = {}
    for name, body in isa.bodies(txt):
        short = isa.demangle_short(name)
        if short.startswith("sdf_fd_bwd_pipe_kernel"):
            ops = [ln.split()[0] for ln in body if ln[:1] in " \t" and ln.split()]
            out[short] = (md[name], ops)
    return out


def test_every_instantiation_is_there(pipe_kernels):
    assert set(pipe_kernels) == {f"sdf_fd_bwd_pipe_kernel<10,{a}>" for a in (4, 5, 6, 7)}


@pytest.mark.parametrize("act", [4, 5, 6, 7])
def test_no_scratch_and_two_workgroups_of_lds_per_cu(pipe_kernels, act):
    md, ops = pipe_kernels[f"sdf_fd_bwd_pipe_kernel<10,{act}>"]
    assert md["scratch"] == 0 and md["vspill"] == 0, md
    assert sum(o.startswith("scratch_") for o in ops) == 0
    assert 0 < md["lds"] <= 80 * 1024, md


@pytest.mark.parametrize("act", [4, 5, 6])
def test_two_waves_per_simd(pipe_kernels, act):
    md, _ = pipe_kernels[f"sdf_fd_bwd_pipe_kernel<10,{act}>"]
    # vgpr_count is the unified count on gfx950: architectural VGPRs + AGPRs (the round-6 form: 460 / 204)
    assert md["vgpr"] <= 256, md
