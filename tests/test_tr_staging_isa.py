"""CPU (cross-compile only): the two backward kernels stage the operands of their contractions over
the points through csrc/tr_stage.h — packed 8-byte stores, transposing reads.  The conflict counts of
that layout are static_asserts of the header (the build fails on a conflict); here: the generated
gfx950 code has no two-byte LDS store left, reads through ds_read_b64_tr_b16, and keeps the register
budgets the kernels' residency depends on."""
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


def _kernels(fname, prefix):
    txt = isa.compile_asm(os.path.join(isa.CSRC, fname))
    md = isa.metadata(txt)
    out = {}
    for name, body in isa.bodies(txt):
        short = isa.demangle_short(name)
        if short.startswith(prefix):
            out[short] = (md[name], [ln.split()[0] for ln in body if ln[:1] in " \t" and ln.split()])
    return out


def _check_staging(md, ops, name):
    assert not any(o.startswith("ds_write_b16") for o in ops), name
    assert not any(o.startswith("ds_write_b8") for o in ops), name
    assert ops.count("ds_read_b64_tr_b16") > 0, name
    assert md["scratch"] == 0 and md["vspill"] == 0, (name, md)
    assert sum(o.startswith("scratch_") for o in ops) == 0, name


def test_pipelined_geometry_backward_stages_packed_and_fits_two_waves_per_simd():
    ks = _kernels("hashgrid_mfma.hip", "sdf_fd_bwd_pipe_kernel")
    assert sorted(ks) == [f"sdf_fd_bwd_pipe_kernel<10,{a}>" for a in (4, 5, 6, 7)]
    for name, (md, ops) in ks.items():
        _check_staging(md, ops, name)
        # 6 contractions in the code (centre: 2 per point half, offsets: 1) x 24 transposing reads
        assert ops.count("ds_read_b64_tr_b16") == 144, name
        assert md["lds"] <= 78592, (name, md)                 # not above the [unit][point] images' 77 KB
        if name != "sdf_fd_bwd_pipe_kernel<10,7>":
            assert md["vgpr"] <= 256, (name, md)              # two waves per SIMD
        else:
            assert md["vgpr"] <= 512, (name, md)


def test_texture_backward_stages_packed():
    ks = _kernels("texture_mlp.hip", "texture_bwd_kernel")
    assert len(ks) == 3
    for name, (md, ops) in ks.items():
        _check_staging(md, ops, name)
        assert md["vgpr"] <= 512, (name, md)
    # the kernel of the optimisation step: not above the 491 registers of the [unit][sample] images
    assert ks["texture_bwd_kernel<1,1>"][0]["vgpr"] <= 491
