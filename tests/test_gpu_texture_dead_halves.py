"""The texture backward skips 32-sample halves whose d_rgb rows are all zero (samples behind the front
surface of the NSR fit) and hands the live halves out evenly (csrc/tex_partition.h).  Here: the kernel the
optimisation step runs (shaded inputs, the forward's ReLU pattern) against float64 autograd, with the
harness and the bounds of tests/test_gpu_tr_staging.py restated — d_x: rtol 1e-4, atol 1e-5 of the largest
entry; parameter gradients: 2e-4 of the largest entry — over every way a half can be dead; and the bitmap
the compositing backward hands over in the step."""
import numpy as np
import pytest
import torch

from drawingspinup_amd import _lib, ops

pytestmark = pytest.mark.gpu

SIZES = [32, 64, 65, 96, 257, 1000, 4100]
TAIL = 8


def _tex_params(seed, dev):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev)
    return [mk(64, 16) * 0.3, mk(64) * 0.1, mk(64, 64) * 0.15, mk(64) * 0.1, mk(3, 64) * 0.2, mk(3) * 0.1], mk


def _live_samples(pattern, n):
    """bool (n,): which samples carry a colour gradient"""
    halves = (n + 31) // 32
    half = torch.zeros(halves, dtype=torch.bool)
    lone = []
    if pattern == "all_live":
        half[:] = True
    elif pattern == "alternating":
        half[::2] = True
    elif pattern == "dead_prefix":
        half[(halves + 1) // 2:] = True
    elif pattern == "dead_suffix":
        half[:(halves + 1) // 2] = True
    elif pattern == "lone_first":                      # one live sample at position 0 of otherwise dead halves
        lone = [32 * k for k in range(0, halves, 3)]
    elif pattern == "lone_last":                       # ... at position 31 (or the last sample of a partial half)
        lone = [min(32 * k + 31, n - 1) for k in range(0, halves, 3)]
    elif pattern == "last_half_dead":
        half[:-1] = True
    elif pattern == "last_half_live":
        half[-1] = True
    else:
        assert pattern == "all_dead"
    live = half.repeat_interleave(32)[:n].clone()
    live[lone] = True
    return live


PATTERNS = ["all_dead", "all_live", "alternating", "dead_prefix", "dead_suffix", "lone_first", "lone_last",
            "last_half_dead", "last_half_live"]


def _shaded_parameter_grads(params, partials, dev):
    tmap = torch.from_numpy(ops.texture_partial_map()).to(dev).long()
    rec = partials.record
    nb, stride, npart = int(rec.nblocks), int(rec.stride), int(rec.n)
    ws = partials.keep[0][:nb * stride].view(nb, stride)[:, :npart].sum(0)
    flat = torch.zeros(sum(t.numel() for t in params), device=dev)
    flat.index_add_(0, tmap[tmap >= 0], ws[tmap >= 0])
    out, off = [], 0
    for t in params:
        out.append(flat[off:off + t.numel()].view_as(t))
        off += t.numel()
    return out


def _run(params, feat, grad, rgb, mask, d_rgb, d_nrm, dev):
    """texture_bwd_kernel<true, true>: (d_feature (n + TAIL, 13), d_grad, parameter gradients)"""
    b = ops.texture_bwd_shaded_partials(params, feat, grad, rgb, d_rgb, d_nrm, TAIL, h1_mask=mask)
    return [b[1].clone(), b[0].clone()] + [g.clone() for g in _shaded_parameter_grads(params, b[3], dev)]


def _reference(params, feat, grad, d_rgb, d_nrm):
    px = [p.double().clone().requires_grad_(True) for p in params]
    f, gr = feat.double().clone().requires_grad_(True), grad.double().clone().requires_grad_(True)
    nrm = torch.nn.functional.normalize(gr, dim=-1)
    h = torch.relu(torch.nn.functional.linear(torch.cat([f, nrm], -1), px[0], px[1]))
    h = torch.relu(torch.nn.functional.linear(h, px[2], px[3]))
    rgb = torch.sigmoid(torch.nn.functional.linear(h, px[4], px[5]))
    ((rgb * d_rgb.double()).sum() + (nrm * d_nrm.double()).sum()).backward()
    return torch.cat([f.grad, gr.grad], -1), [p.grad for p in px]


def _check(out, n, ref_dx, ref_gp, tag):
    d_x = torch.cat([out[0][:n], out[1]], -1).double()
    big = float(ref_dx.abs().max())
    print(f"{tag} d_x: max diff {float((d_x - ref_dx).abs().max()):.3e} of {big:.3e}")
    torch.testing.assert_close(d_x, ref_dx, rtol=1e-4, atol=1e-5 * big)
    for got, ref in zip(out[2:], ref_gp):
        scale = float(ref.abs().max()) + 1e-12
        err = float((got.double() - ref).abs().max())
        print(f"{tag} {tuple(ref.shape)}: max diff {err:.3e} of {scale:.3e}")
        assert err < 2e-4 * scale, (tag, tuple(ref.shape))


def _case(dev, n, pattern, caps):
    params, mk = _tex_params(7000 + n, dev)
    feat, grad = mk(n, 13) * 0.5, mk(n, 3)
    d_nrm = mk(n, 3) * 0.1
    d_nrm = torch.where(d_nrm == 0, torch.full_like(d_nrm, 0.01), d_nrm)     # non-zero everywhere
    live = _live_samples(pattern, n).to(dev)
    d_rgb = mk(n, 3)
    d_rgb = torch.where(d_rgb == 0, torch.full_like(d_rgb, 0.5), d_rgb) * live[:, None]
    d_rgb_tiny = torch.where(live[:, None], d_rgb, torch.full_like(d_rgb, 1e-30))
    ref_dx, ref_gp = _reference(params, feat, grad, d_rgb, d_nrm)
    _, rgb, mask = ops.texture_fwd_shaded(params, feat, grad, with_mask=True)
    lib = _lib.lib()
    try:
        for cap in caps:
            assert lib.dsu_set_onewave_grid_cap(cap) == 0
            tag = f"n={n} {pattern} cap={cap}"
            out = _run(params, feat, grad, rgb, mask, d_rgb, d_nrm, dev)
            assert not bool(out[0][n:].any()), tag                      # tail rows
            assert not bool(out[0][:n][~live].any()), tag               # d_feature of the dead samples: exact zeros
            _check(out, n, ref_dx, ref_gp, tag)
            again = _run(params, feat, grad, rgb, mask, d_rgb, d_nrm, dev)
            for a_, b_ in zip(out, again):
                assert torch.equal(a_, b_), tag
            # the same call with nothing to skip: 1e-30 instead of the zeros moves no output beyond the bounds
            tiny = _run(params, feat, grad, rgb, mask, d_rgb_tiny, d_nrm, dev)
            _check(tiny, n, ref_dx, ref_gp, tag + " 1e-30")
            dx_a = torch.cat([out[0][:n], out[1]], -1).double()
            dx_b = torch.cat([tiny[0][:n], tiny[1]], -1).double()
            torch.testing.assert_close(dx_a, dx_b, rtol=1e-4, atol=1e-5 * float(ref_dx.abs().max()))
            for a_, b_, ref in zip(out[2:], tiny[2:], ref_gp):
                assert float((a_ - b_).abs().max()) <= 2e-4 * (float(ref.abs().max()) + 1e-12), tag
    finally:
        assert lib.dsu_set_onewave_grid_cap(0) == 0


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_dead_halves_are_skipped_and_the_rest_matches_float64_autograd(dev, n, pattern):
    _case(dev, n, pattern, (0, 192))


def test_dead_halves_under_a_grid_cap_that_binds(dev):
    """192 CUs cap the grid from 49 153 samples on: 50 000 samples run on 196 workgroups without the cap
    and on 192 with it, and the live halves are dealt out over whichever was launched."""
    _case(dev, 50000, "alternating", (0, 192))


def test_stand_alone_backward_skips_dead_halves_too(dev):
    """texture_bwd_kernel<false, false> (plain (n,16) rows): the rows of dead samples come back as zeros."""
    n = 257
    params, mk = _tex_params(7100, dev)
    x = mk(n, 16)
    live = _live_samples("alternating", n).to(dev)
    d_rgb = (mk(n, 3) + 0.01) * live[:, None]
    px = [p.double().clone().requires_grad_(True) for p in params]
    xr = x.double().clone().requires_grad_(True)
    h = torch.relu(torch.nn.functional.linear(xr, px[0], px[1]))
    h = torch.relu(torch.nn.functional.linear(h, px[2], px[3]))
    torch.sigmoid(torch.nn.functional.linear(h, px[4], px[5])).backward(d_rgb.double())
    d_x, gp = ops.texture_bwd(params, x, ops.texture_fwd(params, x), d_rgb)
    assert not bool(d_x[~live].any())
    big = float(xr.grad.abs().max())
    torch.testing.assert_close(d_x.double(), xr.grad, rtol=1e-4, atol=1e-5 * big)
    for got, p in zip(gp, px):
        assert float((got.double() - p.grad).abs().max()) < 2e-4 * (float(p.grad.abs().max()) + 1e-12)


def test_compositing_backward_hands_over_the_live_halves(dev):
    """Rays that saturate (alpha -> 1 behind the surface: the f32 transmittance underflows to 0) next to rays
    that do not and an empty ray: the bitmap of dsu_neus_composite_bwd_live is the one recomputed from d_rgb,
    and d_rgb has exact zeros for it to find."""
    g = torch.Generator().manual_seed(11)
    counts = torch.tensor([70, 0, 33, 130, 5, 64, 1, 97, 200, 31], dtype=torch.int32)
    offsets = torch.cumsum(counts, 0, dtype=torch.int32) - counts
    n, n_rays = int(counts.sum()), counts.numel()
    dist = 0.01
    sdf, ts = torch.empty(n), torch.empty(n)
    for r in range(n_rays):
        c, o = int(counts[r]), int(offsets[r])
        t = torch.arange(c, dtype=torch.float32) * dist
        ts[o:o + c] = t
        # even rays cross a surface after a few samples and stay inside; odd rays stay outside
        sdf[o:o + c] = (0.05 - t) if r % 2 == 0 else 0.3 + 0.1 * torch.rand(c, generator=g)
    rays_d = torch.tensor([[0.0, 0.0, 1.0]]).repeat(n_rays, 1)
    normal = torch.tensor([[0.0, 0.0, -1.0]]).repeat(n, 1)
    rgb = torch.rand(n, 3, generator=g)
    inv_s = torch.tensor([200.0])
    to = lambda t: t.to(dev)
    args = [to(sdf), to(normal), to(rgb), to(rays_d), to(ts), to(ts + dist), to(offsets), to(counts), to(inv_s), 1.0]
    comp, alpha, w = ops.neus_composite_fwd(*args)
    d_comp = to(torch.rand(n_rays, 8, generator=g) + 0.1)
    d_sdf, d_normal, d_rgb, d_inv, live = ops.neus_composite_bwd_live(*args, alpha, w, d_comp)
    want = ops.neus_composite_bwd(*args, alpha, w, d_comp)
    for a_, b_ in zip((d_sdf, d_normal, d_rgb, d_inv), want):
        assert torch.equal(a_, b_)
    lit = (d_rgb != 0).any(-1).cpu()
    assert bool(lit.any()) and not bool(lit.all())                     # saturating rays leave exact zeros
    halves = (n + 31) // 32
    pad = torch.zeros(halves * 32, dtype=torch.bool)
    pad[:n] = lit
    half_live = pad.view(halves, 32).any(-1).numpy()
    assert 0 < int(half_live.sum()) < halves
    words = np.zeros((halves + 31) // 32, dtype=np.uint32)
    for k in np.nonzero(half_live)[0]:
        words[k >> 5] |= np.uint32(1) << np.uint32(k & 31)
    got = live.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, words)
