"""The diffusion leaf kernels (norm_act.hip, attention.hip) against float64, on the inputs where
they can go wrong: groups far from zero, every dispatch branch of GroupNorm, the UNet's fused q|k
layout, trained-scale logits, tail masks in every segment.  References, inputs and bounds live in
mv_leaf_ref.py; test_mv_leaf_ref_host.py shows on the CPU that the bounds are reachable in float32
and that the inputs tell a cancelling variance apart."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_leaf_ref as L  # noqa: E402
from drawingspinup_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

G = L.GN_GROUPS


# ---------------------------------------------------------------------------------- GroupNorm
@functools.lru_cache(maxsize=None)
def _gn_data(case, kind):
    C = case[3]
    return L.gn_input(case, kind), L.affine(C, C), torch.ones(C).half(), torch.zeros(C).half()


@pytest.mark.parametrize("kind", ["offset", "randn"])
@pytest.mark.parametrize("eps", L.GN_EPS)
@pytest.mark.parametrize("case", L.GN_CASES, ids=L.gn_case_id)
def test_groupnorm_float64(dev, case, eps, kind):
    B, H, W, C = case
    x, (gamma, beta), one, zero = _gn_data(case, kind)
    xd = x.to(dev)
    worst = 0.0
    for silu in (False, True):
        ref = L.group_norm64(x, gamma, beta, G, eps, silu)
        got = ops.groupnorm_nhwc_f16(xd, gamma.to(dev), beta.to(dev), G, eps, silu).cpu()
        assert got.shape == x.shape and got.dtype == torch.float16
        worst = max(worst, L.elem_error(got, ref))
        if kind == "offset":        # the all-zero group comes out as exactly beta / silu(beta)
            zb, zg = L.gn_zero_group(case)
            cpg = C // G
            bz = beta[zg * cpg:(zg + 1) * cpg]
            z = got[zb, :, zg * cpg:(zg + 1) * cpg]
            if not silu:            # (0 - 0) * rstd * gamma + beta: nothing rounds
                assert torch.equal(z, bz.expand_as(z)), "zero group is not beta"
            else:                   # the device's fast exp: one f16 ulp of the expected value
                want = L.silu64(bz.double()).half().double()
                assert bool(((z.double() - want).abs() <= L.f16_ulp(want)).all()), "zero group is not silu(beta)"
    ref1 = L.group_norm64(x, one, zero, G, eps)
    floor = L.rstd_error(ref1.half(), x, G, eps)
    stat = L.rstd_error(ops.groupnorm_nhwc_f16(xd, one.to(dev), zero.to(dev), G, eps, False).cpu(),
                        x, G, eps)
    print(f"groupnorm {L.gn_case_id(case)} eps {eps:g} {kind}: element-wise {worst / L.ELEM_BOUND:.3g} of "
          f"the bound; fitted rstd off by {stat:.3g} = {stat / floor:.3g} floors ({floor:.2e})")
    assert worst <= L.ELEM_BOUND
    assert stat <= L.STAT_MARGIN * floor


@pytest.mark.parametrize("C,groups", [(324, 27), (320, 33)], ids=["C%8", "C%G"])
def test_groupnorm_refuses_and_writes_nothing(dev, C, groups):
    x = torch.randn(1, 16, C, device=dev).half()
    w = torch.ones(C, device=dev).half()
    out = torch.full_like(x, 7.0)
    ws = torch.full((2 * 64,), 7.0, device=dev)
    rc = _lib.lib().dsu_groupnorm_nhwc_f16(_lib.ptr(x), _lib.ptr(w), _lib.ptr(w), 1, 16, C, groups, 1e-5,
                                           0, _lib.ptr(ws), _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all())
    with pytest.raises(_lib.DsuError):
        ops.groupnorm_nhwc_f16(x, w, w, groups)


# ---------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows,C", L.LN_CASES)
def test_layernorm_float64(dev, rows, C):
    x = L.ln_input(rows, C)
    gamma, beta = L.affine(C, C)
    got = ops.layernorm_f16(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5).cpu()
    err = L.elem_error(got, L.layer_norm64(x, gamma, beta, 1e-5))
    one, zero = torch.ones(C).half(), torch.zeros(C).half()
    xr = x.reshape(rows, 1, C)
    floor = L.rstd_error(L.layer_norm64(x, one, zero, 1e-5).half().reshape(rows, 1, C), xr, 1, 1e-5)
    got1 = ops.layernorm_f16(x.to(dev), one.to(dev), zero.to(dev), 1e-5).cpu()
    stat = L.rstd_error(got1.reshape(rows, 1, C), xr, 1, 1e-5)
    print(f"layernorm ({rows}, {C}): element-wise {err / L.ELEM_BOUND:.3g} of the bound; fitted rstd off "
          f"by {stat:.3g} = {stat / floor:.3g} floors ({floor:.2e})")
    assert err <= L.ELEM_BOUND
    assert stat <= L.STAT_MARGIN * floor


def test_layernorm_empty_and_refusals(dev):
    w = torch.ones(2056, device=dev).half()
    out = ops.layernorm_f16(torch.empty(0, 320, device=dev).half(), w[:320], w[:320])
    assert out.shape == (0, 320) and out.dtype == torch.float16
    for C in (2056, 12):
        with pytest.raises(_lib.DsuError):
            ops.layernorm_f16(torch.zeros(3, C, device=dev).half(), w[:C], w[:C])


# ---------------------------------------------------------------------------------- GEGLU
@pytest.mark.parametrize("D", [64, 8])
def test_geglu_grid_float64(dev, D):
    h = L.geglu_grid(D)
    ref = L.geglu64(h)
    got = ops.geglu_f16(h.to(dev)).cpu()
    assert got.shape == ref.shape
    keep = ref.abs() < L.GEGLU_FINITE
    err = L.elem_error(got[keep], ref[keep])
    print(f"geglu D={D}: element-wise {err / L.ELEM_BOUND:.3g} of the bound")
    assert err <= L.ELEM_BOUND


def test_geglu_empty_and_refusal(dev):
    out = ops.geglu_f16(torch.empty(0, 128, device=dev).half())
    assert out.shape == (0, 64) and out.dtype == torch.float16
    with pytest.raises(_lib.DsuError):
        ops.geglu_f16(torch.zeros(3, 24, device=dev).half())               # D = 12


# ---------------------------------------------------------------------------------- attention
TOL = dict(rtol=2e-3, atol=2e-3)          # test_gpu_attention.py's own
TOL_LATE = dict(rtol=3e-3, atol=3e-3)     # a late key carries the row maximum (its spiked-scores case)


def _qkv(B, N, C, seed, scale=1.0, Nk=None):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, N, C, generator=g) * scale).half()
    k = (torch.randn(B, Nk or N, C, generator=g) * scale).half()
    v = torch.randn(B, Nk or N, C, generator=g).half()
    return q, k, v


def _run(dev, q, k, v, table, heads, seg_len, scale=None):
    vt = v.transpose(1, 2).contiguous().to(dev)
    return ops.mv_attention(q.to(dev), k.to(dev), vt, table.to(dev), heads, seg_len, scale).cpu()


def _check(dev, q, k, v, table, heads, seg_len, scale=None, tol=TOL):
    ref = L.segment_attention64(q, k, v, table, heads, seg_len, scale)
    out = _run(dev, q, k, v, table, heads, seg_len, scale)
    assert out.shape == q.shape and out.dtype == torch.float16
    torch.testing.assert_close(out.double(), ref, **tol)
    return out, ref


@pytest.mark.parametrize("N,C", [(64, 320), (16, 1280)], ids=["d40", "d160"])
def test_attention_fused_qk_layout(dev, N, C):
    """q and k as the two halves of one (B, N, 2C) projection, token stride 2C: the UNet's layout."""
    B, heads = 6, 8
    g = torch.Generator().manual_seed(11)
    qk = torch.randn(B, N, 2 * C, generator=g).half()
    v = torch.randn(B, N, C, generator=g).half()
    table = L.mv_table(B, 6)
    ref = L.segment_attention64(qk[..., :C], qk[..., C:], v, table, heads, N)
    qkd, vt, tbl = qk.to(dev), v.transpose(1, 2).contiguous().to(dev), table.to(dev)
    q, k = qkd[..., :C], qkd[..., C:]
    assert q.stride(1) == 2 * C and not k.is_contiguous()
    out = ops.mv_attention(q, k, vt, tbl, heads, N)
    flat = ops.mv_attention(q.contiguous(), k.contiguous(), vt, tbl, heads, N)
    assert torch.equal(out, flat)
    torch.testing.assert_close(out.cpu().double(), ref, **TOL)


def test_attention_head_dim_64(dev):
    q, k, v = _qkv(4, 36, 512, 12)
    _check(dev, q, k, v, L.joint_table(4), 8, 36)


@pytest.mark.parametrize("table,B,N", [("mv", 6, 64), ("joint", 4, 68)])
def test_attention_trained_scale_logits(dev, table, B, N):
    """q, k four times unit normal: scaled logits of std about 16, row maxima above 50."""
    q, k, v = _qkv(B, N, 320, 13, scale=4.0)
    tbl = L.mv_table(B, 6) if table == "mv" else L.joint_table(B)
    logits = torch.einsum("bqhd,bkhd->bhqk", q.double().reshape(B, N, 8, 40), k.double().reshape(B, N, 8, 40))
    assert float(logits.max()) * 40 ** -0.5 > 50
    _check(dev, q, k, v, tbl, 8, N)


def _ramp_qk(B, N, C, seed, descending):
    """Every query scores key j at about 100 j / N (100 (N - 1 - j) / N if descending), plus noise."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(0, 2, (C,), generator=g).double() * 2 - 1
    ramp = torch.arange(N, dtype=torch.float64) / N
    if descending:
        ramp = ramp.flip(0)
    q = (4.0 * w + 0.1 * torch.randn(B, N, C, generator=g, dtype=torch.float64)).half()
    k = (4.0 * ramp[None, :, None] * w + 0.1 * torch.randn(B, N, C, generator=g, dtype=torch.float64)).half()
    v = torch.randn(B, N, C, generator=g).half()
    return q, k, v


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_attention_ramped_maxima(dev, descending):
    """Ascending: every 64-key tile of the 192 raises the running maximum and rescales the sum.
    Descending: the maximum sits in the first tile and the later tiles underflow to 0."""
    B, N, C = 2, 192, 320
    q, k, v = _ramp_qk(B, N, C, 14, descending)
    tbl = torch.tensor([[0], [1]], dtype=torch.int32)
    s = torch.einsum("qd,kd->qk", q[0, :, :40].double(), k[0, :, :40].double()) * 40 ** -0.5
    tiles = s.reshape(N, 3, 64).max(-1).values
    step = tiles[:, 1:] - tiles[:, :-1]
    assert bool((step < -20).all()) if descending else bool((step > 20).all())
    _check(dev, q, k, v, tbl, 8, N, tol=TOL if descending else TOL_LATE)


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("seg_len", [4, 36, 68, 100])
def test_attention_tail_mask_every_segment(dev, seg_len, S):
    """seg_len off the 64-key tile in each of S segments.  The key tensor is 4 tokens longer than
    seg_len and those 4 would win every row (keys aligned with all queries, values of 1000) if the
    mask let them through in any segment."""
    B, C, heads = 3, 320, 8
    q, k, v = _qkv(B, seg_len, C, 15 + seg_len + S, Nk=seg_len + 4)
    k[:, seg_len:] = 3.0 * q.float().mean(1, keepdim=True).sign().half()
    q = (q.float() + 0.5 * q.float().mean(1, keepdim=True).sign()).half()
    v[:, seg_len:] = 1000.0
    tbl = torch.tensor([[(b + s) % B for s in range(S)] for b in range(B)], dtype=torch.int32)
    out, _ = _check(dev, q, k, v, tbl, heads, seg_len)
    assert float(out.abs().max()) < 8.0


@pytest.mark.parametrize("Nq", [1, 33, 129])
def test_attention_partly_filled_waves(dev, Nq):
    """Nq off the 32-query wave and the 128-query workgroup, and different from seg_len."""
    g = torch.Generator().manual_seed(16)
    q = torch.randn(2, Nq, 320, generator=g).half()
    _, k, v = _qkv(2, 68, 320, 17)
    _check(dev, q, k, v, L.joint_table(2), 8, 68)


@pytest.mark.parametrize("rows", [[[0], [1], [2]], [[2, 0], [0, 1], [1, 2]], [[1, 1], [0, 2], [2, 2]]],
                         ids=["identity", "permuted", "repeated"])
def test_attention_tables(dev, rows):
    q, k, v = _qkv(3, 36, 320, 18)
    _check(dev, q, k, v, torch.tensor(rows, dtype=torch.int32), 8, 36)


def test_attention_offset_values(dev):
    """V = randn + 50: rows stay convex combinations, so no output exceeds max V by more than an ulp."""
    q, k, v = _qkv(6, 64, 320, 19)
    v = (v.float() + 50.0).half()
    out, _ = _check(dev, q, k, v, L.mv_table(6, 6), 8, 64)
    assert float(out.max()) <= float(v.max()) + 2.0 ** -5       # one f16 ulp in [32, 64)
    assert float(out.min()) >= float(v.min()) - 2.0 ** -5


def test_attention_explicit_scale(dev):
    q, k, v = _qkv(4, 36, 320, 20)
    out, ref = _check(dev, q, k, v, L.joint_table(4), 8, 36, scale=0.05)
    default = L.segment_attention64(q, k, v, L.joint_table(4), 8, 36)
    assert float((ref - default).abs().max()) > 0.05            # the scale is not a no-op here


def test_attention_refusals(dev):
    q, k, v = _qkv(2, 8, 320, 21)
    tbl = torch.tensor([[0], [1]], dtype=torch.int32)
    with pytest.raises(_lib.DsuError):
        _run(dev, q[:, :6], k[:, :6], v[:, :6], tbl, 8, 6)                 # seg_len % 4 != 0
    q, k, v = _qkv(2, 8, 384, 22)
    with pytest.raises(_lib.DsuError):
        _run(dev, q, k, v, tbl, 8, 8)                                      # head dim 48
