"""Pins tests/neus_composite_ref.py (the float64 restatement the fused shading / compositing
kernels are held to in tests/test_gpu_nsr_composite.py) before any kernel is compared with it:
against the reference's own forward on tests/golden/nsr_step_reference.npz, and against
oracle/nerfacc_ref.py.  CPU only."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import neus_composite_ref as ncr
from oracle import nerfacc_ref as nr

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "nsr_step_reference.npz"))


def rel_max(got, want):
    """Largest deviation relative to the largest reference magnitude."""
    got = np.asarray(got, np.float64).ravel()
    want = np.asarray(want, np.float64).ravel()
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_restatement_matches_reference_forward_fixture():
    """The reference's own sdf / sdf_grad / midpoints / intervals through the restatement give its
    weights, opacity, depth and composite normal.  Bounds: four times the residue a float64
    prototype of this comparison measured (1.9e-6, 1.3e-5, 1.6e-5, 1.5e-5), which comes from the
    fixture's float32 values and the rebuilt interval ends."""
    t = lambda k: torch.from_numpy(GOLD[k])
    ri = GOLD["fwd.ray_indices"]
    n_rays = GOLD["rays"].shape[0]
    assert (np.diff(ri) >= 0).all()
    counts = np.bincount(ri, minlength=n_rays)
    assert (counts == 0).sum() == 92 and (counts > 192).sum() == 72    # what the fixture covers
    mid, half = t("fwd.points").double(), t("fwd.intervals").double() / 2
    normal, _ = ncr.shade_prep(t("fwd.sdf_grad_samples"), torch.zeros(len(ri), 13))
    inv_s = torch.exp(10.0 * t("sd.variance.variance").double()).reshape(1)
    comp, alpha, w = ncr.composite(t("fwd.sdf_samples"), normal, torch.zeros(len(ri), 3),
                                   t("rays")[:, 3:6], mid - half, mid + half, counts, inv_s,
                                   float(GOLD["cos_anneal_ratio"]))
    errs = {"weights": rel_max(w, GOLD["fwd.weights"]),
            "opacity": rel_max(comp[:, 0], GOLD["fwd.opacity"]),
            "depth": rel_max(comp[:, 1], GOLD["fwd.depth"])}
    valid = GOLD["fwd.rays_valid"].ravel()
    cn = F.normalize(comp[:, 5:8], p=2, dim=-1)
    errs["normal"] = rel_max(cn[valid], GOLD["fwd.comp_normal"][valid])
    print(errs)
    assert errs["weights"] <= 4 * 1.9e-6
    assert errs["opacity"] <= 4 * 1.3e-5
    assert errs["depth"] <= 4 * 1.6e-5
    assert errs["normal"] <= 4 * 1.5e-5
    assert np.array_equal((comp[:, 0] > 0).numpy(), valid)
    assert (comp[counts == 0] == 0).all()
    assert (comp[:, 2:5] == 0).all()                                   # rgb was fed as zero


def test_restatement_agrees_with_the_nerfacc_restatement():
    """alpha -> weights, the accumulation, and autograd's d_alpha against oracle/nerfacc_ref.py's
    serial loops (float64 on both sides), on the generated case; d_alpha where alpha <= 0.99."""
    case = ncr.generated_case()
    counts = case["counts"]
    t = lambda k: torch.from_numpy(case[k]).double()
    for inv_s in (float(np.exp(3.0)), 60.0):
        _, alpha, _ = ncr.composite(t("sdf"), t("normal"), t("rgb"), t("rays_d"), t("t_starts"),
                                    t("t_ends"), counts, torch.tensor([inv_s]), 0.075)
        a = alpha.clone().requires_grad_(True)
        w = a * ncr.exclusive_cumprod(1.0 - a, counts)
        w_ref = nr.render_weight_from_alpha(alpha.numpy(), counts)
        np.testing.assert_allclose(w.detach().numpy(), w_ref, rtol=1e-12, atol=1e-300)
        ri = ncr.ray_index(counts)
        vals = torch.cat([t("rgb"), t("normal")], 1)
        acc = torch.zeros(len(counts), 6, dtype=torch.float64).index_add(0, ri, w.detach()[:, None] * vals)
        np.testing.assert_allclose(
            acc.numpy(), nr.accumulate_along_rays(w_ref, vals.numpy(), ri.numpy(), len(counts)),
            rtol=1e-12, atol=1e-15)
        gw = t("d_weights")
        (w * gw).sum().backward()
        ga_ref = nr.render_weight_from_alpha_bwd(alpha.numpy(), counts, gw.numpy())
        ok = alpha.numpy() <= 0.99
        assert ok.sum() > 0.7 * ok.size
        # the serial rule subtracts a running sum from the total: absolute error ~ 1e-16 * |total|,
        # divided by 1 - alpha >= 0.01
        np.testing.assert_allclose(a.grad.numpy()[ok], ga_ref[ok], rtol=1e-9, atol=1e-11)


def test_generated_case_meets_its_conditions():
    """The conditions the GPU tests rely on, on the reference alone."""
    assert tuple(ncr.COUNTS) == (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 0, 7)
    for axis in (False, True):
        case = ncr.generated_case(axis)
        np.testing.assert_allclose(np.linalg.norm(case["normal"], axis=1), 1.0, atol=1e-6)
        np.testing.assert_allclose(np.linalg.norm(case["rays_d"], axis=1), 1.0, atol=1e-6)
        if axis:
            assert (np.abs(case["rays_d"][:, 2]) == 1).all() and (case["rays_d"][:, :2] == 0).all()
        for car in (0.0, 0.075, 1.0):
            lo = ncr.reference(case, np.exp(3.0), car)["alpha"]
            hi = ncr.reference(case, 60.0, car)["alpha"]
            assert float(lo.max()) < 0.9
            assert 0.01 < float((hi > 0.99).double().mean()) < 0.25


def test_shade_prep_restatement():
    g = torch.Generator().manual_seed(3)
    grad = torch.randn(40, 3, generator=g, dtype=torch.float64)
    grad[5] = 0.0
    feat = torch.randn(40, 13, generator=g, dtype=torch.float64)
    normal, tex_in = ncr.shade_prep(grad, feat)
    want = grad / grad.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    assert torch.equal(normal, want) or float((normal - want).abs().max()) < 1e-15
    assert (normal[5] == 0).all()
    assert tex_in.shape == (40, 16)
    assert torch.equal(tex_in[:, :13], feat) and torch.equal(tex_in[:, 13:], normal)
