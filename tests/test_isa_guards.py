"""CPU (cross-compile only): static guards against code-generation pitfalls that have already
cost a measurable factor on the MI355X ("Compiler / runtime pitfalls").  hipcc emits
gfx950 assembly without a GPU; tools/isa_stats.py parses it."""
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


def _kernels(fname):
    txt = isa.compile_asm(os.path.join(isa.CSRC, fname))
    md = isa.metadata(txt)
    out = {}
    for name, body in isa.bodies(txt):
        ops = [ln.split()[0] for ln in body if ln[:1] in " \t" and ln.split()]
        out[isa.demangle_short(name)] = (md[name], ops)
    return out


def test_weight_gradient_kernel_keeps_its_accumulators_in_place():
    ks = _kernels("style_train.hip")
    wg = {k: v for k, v in ks.items() if k.startswith("conv_wgrad_kernel")}
    assert len(wg) == 15
    for name, (md, ops) in wg.items():
        mfma = sum(o.startswith("v_mfma") for o in ops)
        movs = ops.count("v_accvgpr_mov_b32")
        assert mfma in (4, 8), name
        assert movs <= 16, f"{name}: {movs} accumulator copies around {mfma} MFMAs"
        assert md["scratch"] == 0 and md["vspill"] <= 1, (name, md)
        assert sum(o.startswith("scratch_") for o in ops) == 0, name
    for name, (md, ops) in ks.items():
        assert md["scratch"] == 0, (name, md)


def test_dominant_nsr_kernels_have_no_scratch():
    ks = _kernels("hashgrid_mfma.hip")
    hot = [k for k in ks if k.startswith("sdf_fd_bwd_mfma_kernel") or k.startswith("sdf_fd_scatter")]
    assert len(hot) == 6       # the general MLP-part kernel <NL = 10 | 12, cache or not> + the scatter <10 | 12>
    for name in hot:
        md, ops = ks[name]
        assert md["scratch"] == 0 and md["vspill"] == 0, (name, md)
        assert sum(o.startswith("scratch_") for o in ops) == 0, name
        assert md["vgpr"] <= 512
    # <NL=10, feature cache>: the gather path and its level metadata are compiled out (SGPR spills
    # 130 -> 36 when that was introduced, with a few more allowed for the per-workgroup range scalars)
    # (round 3: the two point halves as straight-line code with hand-placed load waits doubled the
    # scalars kept in vector lanes, 43 -> 87; measured faster all the same, profiles/round3_ab_k1_load_waits.txt)
    md, _ = ks["sdf_fd_bwd_mfma_kernel<10,1>"]
    assert md["sspill"] <= 96, md


def test_asm_valu_statements_stay_out_of_files_with_matrix_instructions():
    """An asm statement that reads an MFMA accumulator gets none of the MFMA -> VALU wait states the
    compiler inserts for its own instructions (round 6: the texture forward's ReLU as `asm("v_max_f32")`
    composited colours 0.12 off).  dsu_relu's asm form is opt-in per file (DSU_RELU_ONE_VMAX), and a
    file that opts in, or carries a VALU asm statement of its own, has no matrix instruction."""
    import re
    for f in sorted(os.listdir(isa.CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        src = open(os.path.join(isa.CSRC, f)).read()
        valu_asm = re.search(r'asm\s*(volatile)?\s*\(\s*"v_', src) is not None and f != "common.h"
        if "#define DSU_RELU_ONE_VMAX" in src or valu_asm:
            assert "__builtin_amdgcn_mfma" not in src, f
            for inc in re.findall(r'#include "([^"]+)"', src):
                p = os.path.join(isa.CSRC, inc)
                if os.path.exists(p):
                    assert "__builtin_amdgcn_mfma" not in open(p).read(), (f, inc)
