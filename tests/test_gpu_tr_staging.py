"""The backward kernels' [point][column] staging images (csrc/tr_stage.h: packed 8-byte stores, operand
fragments read back with the transposing LDS read): a wrong lane map lands a unit or a point on the
wrong entry, a stale image row leaks an earlier call's points, a partly filled wave reads rows nobody
wrote.  The shapes are the smallest at which each can show: point halves that are empty, full and off
by one, the <= 64 and <= 128 point tails whose evaluations the waves share, more than one workgroup."""
import pytest
import torch

from drawingspinup_amd import ops

pytestmark = pytest.mark.gpu

CFG = ops.HashGridConfig()
EPS, RADIUS = 1.0 / 128, 1.0


def _table(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(CFG.n_entries, 2, generator=g) * 2 - 1) * scale).half()


def _mlp(seed, din=23):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(64, din, generator=g) * 0.3, torch.randn(64, generator=g) * 0.05,
            torch.randn(13, 64, generator=g) * 0.2, torch.randn(13, generator=g) * 0.1]


@pytest.fixture(scope="module")
def net(dev):
    return _table(61, 0.5).to(dev), [m.to(dev) for m in _mlp(62)]


def _points(n, dev):
    g = torch.Generator().manual_seed(63 + n % 7)
    return (torch.rand(n, 3, generator=g) * 2 - 1).to(dev)


def _upstream(n, dev):
    g = torch.Generator().manual_seed(64)
    return [torch.randn(n, generator=g).to(dev), (torch.randn(n, 3, generator=g) * 0.1).to(dev),
            (torch.randn(n, 13, generator=g) * 0.1).to(dev), (torch.randn(n, generator=g) * 1e-4).to(dev)]


def _both(net, pts, d, active):
    """(general kernel, pipelined kernel): the call without a feature cache re-gathers the same f16
    features and runs sdf_fd_bwd_mfma_kernel, the call with the forward's cache sdf_fd_bwd_pipe_kernel."""
    tab, mlp = net
    fwd = ops.sdf_fd_fwd(CFG, tab, mlp, pts, RADIUS, EPS, active, enc_cache=True)
    general = ops.sdf_fd_bwd(CFG, tab, mlp, pts, RADIUS, EPS, active, *d)
    piped = ops.sdf_fd_bwd(CFG, tab, mlp, pts, RADIUS, EPS, active, *d, enc_cache=fwd[4])
    return general, piped, fwd[4]


@pytest.mark.parametrize("active", [4, 5, 6])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 95, 97, 127, 128, 129, 191, 193, 255, 257, 300])
def test_pipelined_kernel_equals_the_general_kernel_at_partial_waves(dev, net, active, n):
    """Harness and bounds of test_sdf_fd_bwd_pipelined_kernel_equals_the_general_kernel (n < 1000:
    5e-4 of a tensor's largest entry; g_b1 bit for bit where every workgroup's range is whole 256-point
    iterations — none of these n is)."""
    pts, d = _points(n, dev), _upstream(n, dev)
    (gt0, gm0), (gt1, gm1), _ = _both(net, pts, d, active)
    whole = n % 256 == 0 and (n <= 256 * 256 or n % (256 * 256) == 0)
    for k, (a_, b_) in enumerate(zip(gm0, gm1)):
        if whole and k == 3:
            assert torch.equal(a_, b_)
        else:
            err, big = float((a_ - b_).abs().max()), float(a_.abs().max())
            print(f"n={n} active={active} tensor {k}: max diff {err:.3e} of {big:.3e}")
            assert err <= 5e-4 * big, (k, n, active)
    assert int(((gt0 != 0) ^ (gt1 != 0)).sum()) <= 8
    assert float((gt0 - gt1).abs().max()) <= 5e-4 * float(gt0.abs().max())


@pytest.mark.parametrize("kind", ["d_sdf", "feature_column"])
@pytest.mark.parametrize("p", [0, 31, 32, 63, 64, 200, 255])
def test_one_hot_upstream_gradient_lands_on_the_general_kernels_entries(dev, net, p, kind):
    """One point carries a gradient, on the SDF output only or on one feature column only: a permuted
    unit or point of the staged images puts g_w0 / g_w1 on other entries than the general kernel's."""
    n, active = 256, 5
    pts = _points(n, dev)
    d = [torch.zeros(n, device=dev), torch.zeros(n, 3, device=dev), torch.zeros(n, 13, device=dev),
         torch.zeros(n, device=dev)]
    if kind == "d_sdf":
        d[0][p] = 1.0
    else:
        d[2][p, 1 + p % 12] = 1.0
    (_, gm0), (_, gm1), _ = _both(net, pts, d, active)
    for k in (0, 2):                                   # g_w0, g_w1
        err, big = float((gm0[k] - gm1[k]).abs().max()), float(gm0[k].abs().max())
        print(f"p={p} {kind} tensor {k}: max diff {err:.3e} of {big:.3e}")
        assert big > 0.0
        assert err <= 5e-4 * big, (k, p, kind)


def test_zero_upstream_gradients_give_exactly_zero_parameter_gradients(dev, net):
    n, active = 256, 5
    pts = _points(n, dev)
    d = [torch.zeros(n, device=dev), torch.zeros(n, 3, device=dev), torch.zeros(n, 13, device=dev),
         torch.zeros(n, device=dev)]
    _, (gt1, gm1), _ = _both(net, pts, d, active)
    for g in gm1:
        assert not bool(g.any())
    assert not bool(gt1.any())


@pytest.mark.parametrize("active", [4, 5, 6])
def test_a_call_leaves_nothing_in_the_images_for_the_next(dev, net, active):
    """n = 257 and then n = 33 gives the bits of a fresh n = 33 (the images live in LDS, but the partial
    vectors and the dIn buffer are reused); two identical calls give the same bits: the partial sums have
    a fixed order."""
    tab, mlp = net

    def run(n):
        pts, d = _points(n, dev), _upstream(n, dev)
        fwd = ops.sdf_fd_fwd(CFG, tab, mlp, pts, RADIUS, EPS, active, enc_cache=True)
        return ops.sdf_fd_bwd(CFG, tab, mlp, pts, RADIUS, EPS, active, *d, enc_cache=fwd[4])[1]
    fresh = [g.clone() for g in run(33)]
    run(257)
    after = run(33)
    again = run(33)
    for a_, b_, c_ in zip(fresh, after, again):
        assert torch.equal(a_, b_)
        assert torch.equal(b_, c_)


# ---------------------------------------------------------------- texture MLP backward

def _tex_params(seed, dev):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev)
    return [mk(64, 16) * 0.3, mk(64) * 0.1, mk(64, 64) * 0.15, mk(64) * 0.1, mk(3, 64) * 0.2, mk(3) * 0.1], mk


def _tex_reference(params, x, d_rgb):
    """float64 autograd of sigmoid(16 -> 64 -> 64 -> 3 with ReLU) on the f32 inputs"""
    px = [p.double().clone().requires_grad_(True) for p in params]
    xr = x.double().clone().requires_grad_(True)
    h = torch.relu(torch.nn.functional.linear(xr, px[0], px[1]))
    h = torch.relu(torch.nn.functional.linear(h, px[2], px[3]))
    torch.sigmoid(torch.nn.functional.linear(h, px[4], px[5])).backward(d_rgb.double())
    return xr.grad, [p.grad for p in px]


def _check_tex(d_x, gp, ref_dx, ref_gp, tag):
    big = float(ref_dx.abs().max())
    print(f"{tag} d_x: max diff {float((d_x.double() - ref_dx).abs().max()):.3e} of {big:.3e}")
    torch.testing.assert_close(d_x.double(), ref_dx, rtol=1e-4, atol=1e-5 * big)
    for got, ref in zip(gp, ref_gp):
        scale = float(ref.abs().max()) + 1e-12
        err = float((got.double() - ref).abs().max())
        print(f"{tag} {tuple(ref.shape)}: max diff {err:.3e} of {scale:.3e}")
        assert err < 2e-4 * scale, (tag, tuple(ref.shape))


TEX_N = [1, 31, 32, 33, 63, 64, 65, 127, 129, 255, 257, 1000]


@pytest.mark.parametrize("n", TEX_N)
def test_texture_backward_matches_float64_autograd(dev, n):
    """texture_bwd_kernel<false, false> (exact recompute): bounds of test_texture_mlp_kernels_match_torch."""
    params, mk = _tex_params(n, dev)
    x, d_rgb = mk(n, 16), mk(n, 3)
    ref_dx, ref_gp = _tex_reference(params, x, d_rgb)
    rgb = ops.texture_fwd(params, x)
    d_x, gp = ops.texture_bwd(params, x, rgb, d_rgb)
    _check_tex(d_x, gp, ref_dx, ref_gp, f"n={n}")


def _shaded_parameter_grads(params, partials, dev):
    """the deferred parameter sums of dsu_texture_bwd_shaded_partials (the reduction the scatter launch
    would do), as in test_texture_backward_with_the_forwards_relu_pattern"""
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


def _shaded_with_mask(params, feat, grad, d_rgb, d_nrm, dev):
    """texture_bwd_kernel<true, true>, what the NSR step runs: (d_feature, d_grad, parameter gradients)"""
    _, rgb, mask = ops.texture_fwd_shaded(params, feat, grad, with_mask=True)
    b = ops.texture_bwd_shaded_partials(params, feat, grad, rgb, d_rgb, d_nrm, 8, h1_mask=mask)
    return b[0], b[1], _shaded_parameter_grads(params, b[3], dev)


def _shaded_reference(params, feat, grad, d_rgb, d_nrm):
    px = [p.double().clone().requires_grad_(True) for p in params]
    f, gr = feat.double().clone().requires_grad_(True), grad.double().clone().requires_grad_(True)
    nrm = torch.nn.functional.normalize(gr, dim=-1)
    h = torch.relu(torch.nn.functional.linear(torch.cat([f, nrm], -1), px[0], px[1]))
    h = torch.relu(torch.nn.functional.linear(h, px[2], px[3]))
    rgb = torch.sigmoid(torch.nn.functional.linear(h, px[4], px[5]))
    ((rgb * d_rgb.double()).sum() + (nrm * d_nrm.double()).sum()).backward()
    return f.grad, gr.grad, [p.grad for p in px]


@pytest.mark.parametrize("n", TEX_N)
def test_texture_backward_with_the_relu_mask_matches_float64_autograd(dev, n):
    """The same bounds for the kernel the optimisation runs (shaded inputs, layer 1 of the recompute as
    bf16 x 3 under the forward's ReLU pattern)."""
    params, mk = _tex_params(2000 + n, dev)
    feat, grad = mk(n, 13) * 0.5, mk(n, 3)
    d_rgb, d_nrm = mk(n, 3), mk(n, 3) * 0.1
    ref_df, ref_dg, ref_gp = _shaded_reference(params, feat, grad, d_rgb, d_nrm)
    d_grad, d_feat, gp = _shaded_with_mask(params, feat, grad, d_rgb, d_nrm, dev)
    assert not bool(d_feat[n:].any())                    # tail rows zeroed
    _check_tex(torch.cat([d_feat[:n], d_grad], -1), gp, torch.cat([ref_df, ref_dg], -1), ref_gp, f"mask n={n}")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("s", [0, 31, 32, 63])
def test_texture_one_hot_d_rgb(dev, s, masked):
    n = 64
    params, mk = _tex_params(3000 + s, dev)
    d_rgb = torch.zeros(n, 3, device=dev)
    d_rgb[s, s % 3] = 1.0
    if masked:
        feat, grad = mk(n, 13) * 0.5, mk(n, 3)
        d_nrm = torch.zeros(n, 3, device=dev)
        ref_df, ref_dg, ref_gp = _shaded_reference(params, feat, grad, d_rgb, d_nrm)
        d_grad, d_feat, gp = _shaded_with_mask(params, feat, grad, d_rgb, d_nrm, dev)
        _check_tex(torch.cat([d_feat[:n], d_grad], -1), gp, torch.cat([ref_df, ref_dg], -1), ref_gp, f"one-hot mask s={s}")
    else:
        x = mk(n, 16)
        ref_dx, ref_gp = _tex_reference(params, x, d_rgb)
        d_x, gp = ops.texture_bwd(params, x, ops.texture_fwd(params, x), d_rgb)
        _check_tex(d_x, gp, ref_dx, ref_gp, f"one-hot s={s}")


@pytest.mark.parametrize("masked", [False, True])
def test_texture_zero_upstream_gives_exactly_zero_parameter_gradients(dev, masked):
    n = 257
    params, mk = _tex_params(4000, dev)
    d_rgb = torch.zeros(n, 3, device=dev)
    if masked:
        feat, grad = mk(n, 13) * 0.5, mk(n, 3)
        _, _, gp = _shaded_with_mask(params, feat, grad, d_rgb, torch.zeros(n, 3, device=dev), dev)
    else:
        x = mk(n, 16)
        _, gp = ops.texture_bwd(params, x, ops.texture_fwd(params, x), d_rgb)
    for g in gp:
        assert not bool(g.any())


@pytest.mark.parametrize("masked", [False, True])
def test_texture_call_leaves_nothing_in_the_images_for_the_next(dev, masked):
    params, mk = _tex_params(5000, dev)
    data = {n: (mk(n, 13) * 0.5, mk(n, 3), mk(n, 3), mk(n, 3) * 0.1) for n in (33, 257)}

    def run(n):
        feat, grad, d_rgb, d_nrm = data[n]
        if masked:
            d_grad, d_feat, gp = _shaded_with_mask(params, feat, grad, d_rgb, d_nrm, dev)
            return [d_grad.clone(), d_feat.clone()] + [g.clone() for g in gp]
        x = torch.cat([feat, grad], -1)
        d_x, gp = ops.texture_bwd(params, x, ops.texture_fwd(params, x), d_rgb)
        return [d_x.clone()] + [g.clone() for g in gp]
    fresh = run(33)
    run(257)
    after = run(33)
    again = run(33)
    for a_, b_, c_ in zip(fresh, after, again):
        assert torch.equal(a_, b_)
        assert torch.equal(b_, c_)
