"""The fused NeuS shading / compositing kernels (csrc/nsr_render.hip: composite_fwd_kernel,
composite_bwd_kernel, shade_prep_fwd_kernel, shade_prep_bwd_kernel) against the float64
restatement in tests/neus_composite_ref.py (pinned by tests/test_neus_composite_host.py), at the
ray lengths around the 64-lane chunk boundaries, with empty rays, saturating alphas, both ends of
cos_anneal_ratio, the kinks of iter_cos and inv_s outside its clip.

Tolerances of the generated case: the restatement is run in float32 on the same inputs; a kernel
output may deviate from float64 by four times what that float32 run does (largest deviation
relative to the largest reference magnitude of the output).  The factor allows for another
summation order and the device's expf."""
import functools

import numpy as np
import pytest
import torch

import neus_composite_ref as ncr
from drawingspinup_amd import ops

pytestmark = pytest.mark.gpu

INV_INIT = float(np.exp(3.0))          # the initial value: largest reference alpha 0.07
INV_SAT = 60.0                         # ~ 6 % of the reference alphas above 0.99
SAMPLE_OUT = ("alpha", "weights", "d_sdf", "d_normal", "d_rgb")
# Hand cases are too small for a measured float32 deviation to mean much.  They use the float32
# vs float64 deviation of the restatement on the generated case (2e-6 for comp, 3.5e-5 for alpha,
# weights and the sample gradients, relative to the largest magnitude), times the same four.
HAND_COMP, HAND_SAMPLE = 4 * 2e-6, 4 * 3.5e-5


@functools.lru_cache(maxsize=None)
def case_of(axis_aligned):
    return ncr.generated_case(axis_aligned)


@functools.lru_cache(maxsize=None)
def refs(axis_aligned, inv_s, car, d_weights, branch=None):
    """(float64 reference, float32 run of the same restatement); computed once, read only."""
    case = case_of(axis_aligned)
    return (ncr.reference(case, inv_s, car, d_weights, torch.float64, branch),
            ncr.reference(case, inv_s, car, d_weights, torch.float32, branch))


def run_kernels(dev, case, inv_s, car, d_weights, backward=True):
    """The case through ops.neus_composite_fwd / bwd -> dict of float64 CPU tensors."""
    t = lambda k: torch.from_numpy(case[k]).to(dev)
    counts = torch.as_tensor(np.asarray(case["counts"]), dtype=torch.int64)
    off = ncr.offsets(counts).to(torch.int32).to(dev)
    cnt = counts.to(torch.int32).to(dev)
    inv = torch.tensor([inv_s], dtype=torch.float32, device=dev)
    args = (t("sdf"), t("normal"), t("rgb"), t("rays_d"), t("t_starts"), t("t_ends"), off, cnt,
            inv, car)
    comp, alpha, w = ops.neus_composite_fwd(*args)
    out = {"comp": comp, "alpha": alpha, "weights": w}
    if backward:
        dw = t("d_weights") if d_weights else None
        d_sdf, d_normal, d_rgb, d_inv = ops.neus_composite_bwd(*args, alpha, w, t("d_comp"), dw)
        out.update(d_sdf=d_sdf, d_normal=d_normal, d_rgb=d_rgb, d_inv_s=d_inv)
    return {k: v.double().cpu() for k, v in out.items()}


def dev_of(got, want, sel=None):
    """Largest deviation relative to the largest reference magnitude (over `sel`)."""
    got, want = got.double(), want.double()
    if sel is not None:
        got, want = got[sel], want[sel]
    if want.numel() == 0:
        return 0.0
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------ the generated case
@pytest.mark.parametrize("d_weights", [False, True], ids=["dcomp", "dcomp+dw"])
@pytest.mark.parametrize("car", [0.0, 0.075, 1.0])
@pytest.mark.parametrize("inv_s", [INV_INIT, INV_SAT], ids=["init", "saturating"])
@pytest.mark.parametrize("axis_aligned", [False, True], ids=["randdir", "axisdir"])
def test_composite_kernels_match_float64(dev, axis_aligned, inv_s, car, d_weights):
    r64, r32 = refs(axis_aligned, inv_s, car, d_weights)
    # conditions on the reference alone
    keep = r64["alpha"] <= 0.99
    if inv_s == INV_INIT:
        assert float(r64["alpha"].max()) < 0.9 and bool(keep.all())
    else:
        assert 0.01 < float((~keep).double().mean()) < 0.25
    got = run_kernels(dev, case_of(axis_aligned), inv_s, car, d_weights)
    fails = []
    for k in ("comp",) + SAMPLE_OUT:
        sel = keep if k in ("d_sdf", "d_normal") else None
        f32, ker = dev_of(r32[k], r64[k], sel), dev_of(got[k], r64[k], sel)
        print(f"{k:9s} float32 {f32:.2e}  kernel {ker:.2e}  ratio {ker / max(f32, 1e-300):.2f}")
        if not ker <= 4 * f32:
            fails.append((k, ker, f32))
    assert torch.isfinite(got["d_sdf"]).all() and torch.isfinite(got["d_normal"]).all()
    if inv_s == INV_INIT:
        scale = float(r64["d_inv_abs"])           # the signed sum cancels
        f32 = abs(float(r32["d_inv_s"]) - float(r64["d_inv_s"])) / scale
        ker = abs(float(got["d_inv_s"]) - float(r64["d_inv_s"])) / scale
        print(f"d_inv_s   float32 {f32:.2e}  kernel {ker:.2e}  ratio {ker / max(f32, 1e-300):.2f}"
              f"  (sum {float(r64['d_inv_s']):.3e}, abs sum {scale:.3e})")
        if not ker <= 4 * f32:
            fails.append(("d_inv_s", ker, f32))
    assert not fails, fails
    # empty rays: their comp rows are exactly zero
    empty = torch.as_tensor(np.asarray(case_of(axis_aligned)["counts"]) == 0)
    assert (got["comp"][empty] == 0).all()


@pytest.mark.parametrize("car,branch", [(0.0, 0), (1.0, 1)])
@pytest.mark.parametrize("axis_aligned", [False, True], ids=["randdir", "axisdir"])
def test_each_end_of_cos_anneal_silences_one_relu_branch(dev, axis_aligned, car, branch):
    """car = 0 / 1 against the reference evaluated with only the first / second relu term."""
    r64, r32 = refs(axis_aligned, INV_INIT, car, True, branch)
    got = run_kernels(dev, case_of(axis_aligned), INV_INIT, car, True)
    for k in ("comp",) + SAMPLE_OUT:
        f32, ker = dev_of(r32[k], r64[k]), dev_of(got[k], r64[k])
        print(f"{k:9s} float32 {f32:.2e}  kernel {ker:.2e}")
        assert ker <= 4 * f32, k


# ------------------------------------------------------------------ hand cases
def small_case(counts, axis_aligned=True, seed=5):
    return ncr.generated_case(axis_aligned, counts, seed)


def test_all_rays_empty(dev):
    """comp is exactly zero and nothing else is written: no sample output, no d_inv_s."""
    case = small_case((0, 0, 0, 0, 0))
    got = run_kernels(dev, case, INV_INIT, 0.075, False)
    assert got["comp"].shape == (5, 8) and (got["comp"] == 0).all()
    assert got["alpha"].numel() == 0 and float(got["d_inv_s"]) == 0.0
    # samples that belong to no ray: the backward leaves their rows alone
    n = 7
    z = lambda *s: torch.zeros(*s, device=dev)
    cnt = torch.zeros(5, dtype=torch.int32, device=dev)
    inv = torch.tensor([INV_INIT], device=dev)
    rays_d = torch.tensor([[0.0, 0.0, 1.0]] * 5, device=dev)
    args = (z(n), z(n, 3), z(n, 3), rays_d, z(n), z(n) + 0.1, cnt, cnt, inv, 0.075)
    comp, _, _ = ops.neus_composite_fwd(*args)
    assert (comp == 0).all()
    keep = torch.full((n,), -7.0, device=dev)
    _, _, _, d_inv = ops.neus_composite_bwd(*args, z(n), z(n), torch.ones(5, 8, device=dev),
                                            None, d_sdf_out=keep)
    assert (keep == -7.0).all() and float(d_inv) == 0.0


def test_one_sample_on_one_ray(dev):
    case = small_case((1,))
    case["sdf"][:] = 0.01                       # prev_cdf ~ 0.55
    r64 = ncr.reference(case, INV_INIT, 0.075, True)
    got = run_kernels(dev, case, INV_INIT, 0.075, True)
    f = lambda x: np.float32(float(x))
    a = got["alpha"][0]
    # alpha = ((pc - nc) + 1e-5) / (pc + 1e-5) with pc, nc ~ 0.5, each within a few float32 ulps
    # (expf, one sum, one quotient): |d alpha| <~ (|d pc| + |d nc|) / pc ~ 12 * 2^-24 / 0.55
    assert abs(float(a) - float(r64["alpha"][0])) < 2e-6
    # T = 1: the weight is alpha, and each accumulation is one float32 product
    assert float(got["weights"][0]) == float(a)
    mid = (f(case["t_starts"][0]) + f(case["t_ends"][0])) / np.float32(2)
    want = [f(a), f(a) * mid] + [f(a) * f(v) for v in case["rgb"][0]] \
        + [f(a) * f(v) for v in case["normal"][0]]
    assert got["comp"][0].tolist() == [float(v) for v in want]
    for k in ("d_sdf", "d_normal", "d_rgb"):
        assert dev_of(got[k], r64[k]) <= HAND_SAMPLE, k
    assert abs(float(got["d_inv_s"]) - float(r64["d_inv_s"])) <= HAND_SAMPLE * float(r64["d_inv_abs"])


@pytest.mark.parametrize("car", [0.0, 0.075, 1.0])
def test_iter_cos_kinks_take_relu_one_sided_gradient(dev, car):
    """true_cos == 0 (the second relu's argument exactly 0) and true_cos == 1 (the first relu's
    argument exactly 0): torch's relu has gradient 0 at 0, so the chain-rule part of d_normal
    vanishes for that branch while the w * d_comp[5:8] part stays."""
    case = small_case((6, 3))
    d0, d1 = case["rays_d"][0], case["rays_d"][1]
    assert d0.tolist() == [0.0, 0.0, 1.0] and d1.tolist() == [0.0, 0.0, -1.0]
    case["normal"][0] = (1.0, 0.0, 0.0)         # perpendicular
    case["normal"][1] = d0                      # equal to rays_d
    case["normal"][2] = (0.0, -1.0, 0.0)        # perpendicular
    case["normal"][6] = d1                      # equal to rays_d on the second ray
    case["normal"][7] = (0.6, 0.8, 0.0)         # perpendicular
    r64 = ncr.reference(case, INV_INIT, car, True)
    got = run_kernels(dev, case, INV_INIT, car, True)
    assert dev_of(got["comp"], r64["comp"]) <= HAND_COMP
    for k in SAMPLE_OUT:
        print(k, dev_of(got[k], r64[k]))
        assert dev_of(got[k], r64[k]) <= HAND_SAMPLE, k
    dc = torch.from_numpy(case["d_comp"])[ncr.ray_index(case["counts"]), 5:8]   # per sample
    w_dc = got["weights"].float()[:, None] * dc              # one float32 product, as the kernel's
    exact = [1, 6] + ([0, 2, 7] if car == 1.0 else [])      # both relus flat there
    assert torch.equal(got["d_normal"].float()[exact], w_dc[exact])
    assert (r64["d_normal"] - r64["weights"][:, None] * dc.double())[exact].abs().max() < 1e-15
    if car != 1.0:                               # the first relu is live at true_cos == 0
        assert (got["d_normal"].float() - w_dc)[[0, 2, 7]].abs().max() > 0


@pytest.mark.parametrize("outside,clipped", [(1e-7, 1e-6), (2e6, 1e6)])
def test_inv_s_outside_its_clip(dev, outside, clipped):
    """The forward equals the forward at the clipped value, d_inv_s is exactly 0, the other
    gradients are those at the clipped value."""
    case = case_of(True)
    a = run_kernels(dev, case, outside, 0.075, True)
    b = run_kernels(dev, case, clipped, 0.075, True)
    for k in ("comp",) + SAMPLE_OUT:
        assert torch.equal(a[k], b[k]), k
    assert float(a["d_inv_s"]) == 0.0
    if clipped == 1e-6:                          # on the clip's edge the gradient passes
        assert float(b["d_inv_s"]) != 0.0
        # (float32(1e-6) lies below the float64 1e-6, so the restatement is asked in float32)
        assert float(ncr.reference(case, clipped, 0.075, True, torch.float32)["d_inv_s"]) != 0.0
    assert float(ncr.reference(case, outside, 0.075, True)["d_inv_abs"]) == 0.0


def test_backward_twice_gives_the_same_and_d_inv_s_does_not_double(dev):
    case = case_of(False)
    r64, _ = refs(False, INV_INIT, 0.075, True)
    a = run_kernels(dev, case, INV_INIT, 0.075, True)
    b = run_kernels(dev, case, INV_INIT, 0.075, True)
    for k in ("d_sdf", "d_normal", "d_rgb"):
        assert torch.equal(a[k], b[k]), k
    # one atomic add per ray, in any order: each rounds a partial sum of at most abs-sum size
    n_rays = len(case["counts"])
    assert abs(float(a["d_inv_s"]) - float(b["d_inv_s"])) <= n_rays * 2.0 ** -24 * float(r64["d_inv_abs"])


# ------------------------------------------------------------------ shade_prep
def shade_inputs(n, seed=0):
    g = np.random.default_rng(seed)
    mag = 10.0 ** g.uniform(-6, 3, size=(n, 1))
    grad = (ncr.unit(g.normal(size=(n, 3))) * mag).astype(np.float32)
    if n > 3:
        grad[3] = 0.0
    return (torch.from_numpy(grad), torch.from_numpy(g.normal(size=(n, 13)).astype(np.float32)),
            torch.from_numpy(g.normal(size=(n, 3)).astype(np.float32)),
            torch.from_numpy(g.normal(size=(n, 16)).astype(np.float32)))


def test_shade_prep_fwd_matches_float64(dev):
    grad, feat, _, _ = shade_inputs(1000)
    normal, tex_in = ops.shade_prep_fwd(grad.to(dev), feat.to(dev))
    n64, _ = ncr.shade_prep(grad, feat)
    # with u = 2^-24 the largest relative rounding of one operation: the sum of squares (3 u,
    # halved by the root), the root, the reciprocal and the product (u each) give 4.5 u at worst,
    # on components of size <= 1
    err = float((normal.cpu().double() - n64).abs().max())
    print(f"shade_prep_fwd normal: {err:.2e} = {err / 2.0 ** -24:.2f} u")
    assert err <= 5 * 2.0 ** -24
    assert (normal[3] == 0).all()                               # the zero row: exactly 0
    assert torch.equal(tex_in[:, :13].cpu(), feat)              # bit for bit
    assert torch.equal(tex_in[:, 13:], normal)


def shade_bwd_ref(grad, d_normal, d_tex_in, dtype):
    g = grad.to(dtype).clone().requires_grad_(True)
    f = torch.zeros(grad.shape[0], 13, dtype=dtype, requires_grad=True)
    normal, tex_in = ncr.shade_prep(g, f, dtype)
    loss = (tex_in * d_tex_in.to(dtype)).sum()
    if d_normal is not None:
        loss = loss + (normal * d_normal.to(dtype)).sum()
    loss.backward()
    return g.grad, f.grad


@pytest.mark.parametrize("with_d_normal", [True, False], ids=["dn", "nodn"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_shade_prep_bwd_matches_float64_autograd(dev, n, with_d_normal):
    grad, _, d_normal, d_tex_in = shade_inputs(n, seed=n)
    dn = d_normal if with_d_normal else None
    g64, f64 = shade_bwd_ref(grad, dn, d_tex_in, torch.float64)
    g32, _ = shade_bwd_ref(grad, dn, d_tex_in, torch.float32)
    if n > 3:       # the zero row: d / 1e-12 on both sides
        total = d_tex_in[3, 13:].double() + (d_normal[3].double() if with_d_normal else 0.0)
        assert torch.equal(g64[3], total / 1e-12)
    # d_grad scales with 1 / |grad| (1e-3 .. 1e12): rows are compared relative to |dn| / |grad|
    total = d_tex_in[:, 13:].double() + (d_normal.double() if with_d_normal else 0.0)
    scale = total.norm(dim=1) / grad.double().norm(dim=1).clamp_min(1e-12)
    row_dev = lambda x: float(((x.double() - g64).abs().amax(1) / scale).max())
    # plain call
    d_grad, d_feat = ops.shade_prep_bwd(grad.to(dev), None if dn is None else dn.to(dev),
                                        d_tex_in.to(dev))
    f32, ker = row_dev(g32), row_dev(d_grad.cpu())
    print(f"n {n}: d_grad float32 {f32:.2e}  kernel {ker:.2e}")
    # a one-row float32 run can be nearly exact by luck (0.2 u, u = 2^-24, where 255 rows give
    # 3 u); the kernel's normalisation, dot, product, difference and scaling round 12 times
    assert ker <= 4 * max(f32, 3 * 2.0 ** -24)
    assert torch.equal(d_feat.cpu(), d_tex_in[:, :13]) and torch.equal(f64.float(), d_tex_in[:, :13])
    # out= form: row prefixes of larger buffers; the rows behind stay as they were
    buf_g = torch.full((n + 5, 3), -3.0, device=dev)
    buf_f = torch.full((n + 5, 13), -5.0, device=dev)
    o_g, o_f = ops.shade_prep_bwd(grad.to(dev), None if dn is None else dn.to(dev),
                                  d_tex_in.to(dev), out=(buf_g[:n], buf_f[:n]))
    assert o_g.data_ptr() == buf_g.data_ptr() and o_f.data_ptr() == buf_f.data_ptr()
    assert torch.equal(buf_g[:n], d_grad) and torch.equal(buf_f[:n], d_feat)
    assert (buf_g[n:] == -3.0).all() and (buf_f[n:] == -5.0).all()
