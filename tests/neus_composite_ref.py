"""Float64 restatement of the fused NeuS shading and compositing rules (csrc/nsr_render.hip:
composite_fwd/bwd_kernel, shade_prep_fwd/bwd_kernel; the reference's neus.py:90-112 get_alpha and
:143-153 normalize / weights / accumulate) as plain differentiable torch expressions, plus the
generated case the tests share.  The backward is autograd of these expressions.  Test
infrastructure only: torch and numpy, no GPU, no code shared with the product.
"""
import numpy as np
import torch
import torch.nn.functional as F

# The chunk boundaries of the 64-lane walk, empty rays first / in the middle / next to last, and
# 15 rays so that the last workgroup (4 rays each) holds three.
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 0, 7)
STEP = 0.0034


def ray_index(counts):
    counts = torch.as_tensor(counts, dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(counts.numel()), counts)


def offsets(counts):
    counts = torch.as_tensor(counts, dtype=torch.int64)
    return torch.cumsum(counts, 0) - counts


def exclusive_cumprod(x, counts):
    """Per ray: out[j] = prod_{k<j} x[k] (1 for a ray's first sample)."""
    parts = []
    for seg in torch.split(x, [int(c) for c in counts]):
        if seg.numel():
            parts.append(torch.cat([seg.new_ones(1), torch.cumprod(seg, 0)[:-1]]))
    return torch.cat(parts) if parts else x.new_zeros(0)


def iter_cos(true_cos, car, branch=None):
    """neus.py:98-99.  `branch` 0 / 1 keeps only the first / second relu term (what car = 0 /
    car = 1 must reduce to)."""
    a = F.relu(-true_cos * 0.5 + 0.5) * (1.0 - car)
    b = F.relu(-true_cos) * car
    if branch == 0:
        return -a
    if branch == 1:
        return -b
    return -(a + b)


def composite(sdf, normal, rgb, rays_d, t_starts, t_ends, counts, inv_s, car,
              dtype=torch.float64, branch=None):
    """sdf (N), normal / rgb (N,3), rays_d (R,3), t_starts / t_ends (N), counts (R) ints,
    inv_s a one-element tensor (or one equal value per sample, which lets autograd hand back the
    per-sample contributions to its gradient), car a float -> (comp (R,8), alpha (N), weights (N))
    in `dtype`.  comp columns: opacity, depth at the interval midpoints, rgb, normal."""
    c = lambda t: t.to(dtype)
    sdf, normal, rgb, rays_d, t_starts, t_ends = map(c, (sdf, normal, rgb, rays_d, t_starts, t_ends))
    counts = [int(v) for v in counts]
    ri = ray_index(counts)
    inv = c(inv_s).reshape(-1).clip(1e-6, 1e6)
    dirs = rays_d[ri]
    dists = t_ends - t_starts
    mid = (t_starts + t_ends) / 2.0
    true_cos = (dirs * normal).sum(-1)
    ic = iter_cos(true_cos, car, branch)
    nxt = sdf + ic * dists * 0.5
    prv = sdf - ic * dists * 0.5
    pc = torch.sigmoid(prv * inv)
    nc = torch.sigmoid(nxt * inv)
    alpha = (((pc - nc) + 1e-5) / (pc + 1e-5)).clip(0.0, 1.0)
    weights = alpha * exclusive_cumprod(1.0 - alpha, counts)
    vals = torch.cat([torch.ones_like(mid)[:, None], mid[:, None], rgb, normal], 1)
    comp = torch.zeros((len(counts), 8), dtype=dtype).index_add(0, ri, weights[:, None] * vals)
    return comp, alpha, weights


def shade_prep(grad, feature, dtype=torch.float64):
    """grad (n,3), feature (n,13) -> (normal (n,3), tex_in (n,16) = [feature | normal])."""
    normal = F.normalize(grad.to(dtype), p=2, dim=-1, eps=1e-12)
    return normal, torch.cat([feature.to(dtype), normal], 1)


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def generated_case(axis_aligned=False, counts=COUNTS, seed=11):
    """The generated case: float32 numpy inputs (what both the kernels and the restatement get).
    Along each ray the sdf ramps from +0.3 to -0.3 with noise 0.02; unit random normals; rays_d
    unit random or (0,0,+-1); contiguous steps of 0.0034; random-normal d_comp and d_weights."""
    g = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    R, N = len(counts), int(counts.sum())
    sdf = np.concatenate([np.linspace(0.3, -0.3, c) if c > 1 else np.full(c, 0.3) for c in counts]
                         + [np.zeros(0)]) + 0.02 * g.normal(size=N)
    near = g.uniform(0.2, 1.5, size=R)
    j = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0)])
    ts = np.repeat(near, counts) + STEP * j
    if axis_aligned:
        rays_d = np.zeros((R, 3))
        rays_d[:, 2] = np.where(np.arange(R) % 2 == 0, 1.0, -1.0)
    else:
        rays_d = unit(g.normal(size=(R, 3)))
    case = {
        "sdf": sdf, "normal": unit(g.normal(size=(N, 3))), "rgb": g.random((N, 3)),
        "rays_d": rays_d, "t_starts": ts, "t_ends": ts + STEP,
        "d_comp": g.normal(size=(R, 8)), "d_weights": g.normal(size=N),
    }
    case = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in case.items()}
    case["counts"] = counts
    return case


def reference(case, inv_s, car, d_weights=False, dtype=torch.float64, branch=None):
    """Forward and autograd backward of `composite` on a case dict.  -> dict of `dtype` tensors:
    comp, alpha, weights, d_sdf, d_normal, d_rgb, d_inv_s (1), and d_inv_abs, the sum of the
    absolute per-sample contributions to d_inv_s (its scale: the signed sum cancels)."""
    t = lambda k: torch.from_numpy(case[k]).to(dtype)
    leaf = {k: t(k).requires_grad_(True) for k in ("sdf", "normal", "rgb")}
    N = leaf["sdf"].numel()
    # one inv_s leaf per sample, so that autograd hands back the per-sample contributions
    inv_raw = torch.full((max(N, 1),), float(np.float32(inv_s)), dtype=dtype, requires_grad=True)
    comp, alpha, w = composite(leaf["sdf"], leaf["normal"], leaf["rgb"], t("rays_d"), t("t_starts"),
                               t("t_ends"), case["counts"], inv_raw[:N], car, dtype, branch)
    loss = (comp * t("d_comp")).sum()
    if d_weights:
        loss = loss + (w * t("d_weights")).sum()
    if N:
        loss.backward()
    z = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    dinv = z(inv_raw)[:N]
    return {"comp": comp.detach(), "alpha": alpha.detach(), "weights": w.detach(),
            "d_sdf": z(leaf["sdf"]), "d_normal": z(leaf["normal"]), "d_rgb": z(leaf["rgb"]),
            "d_inv_s": dinv.sum().reshape(1), "d_inv_abs": dinv.abs().sum().reshape(1)}

