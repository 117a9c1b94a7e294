"""The inputs and bounds of test_gpu_mv_leaf_edges.py, checked without the code under test.

For every GroupNorm case a float32 implementation with a CENTRED variance meets both bounds (they
are reachable), and one with var = E[x^2] - E[x]^2 breaks the statistics bound wherever a group sits
off zero (the inputs discriminate).  segment_attention64 is pinned to the restated processors of
oracle.mv_ref on the two table structures those know."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_leaf_ref as L  # noqa: E402
from oracle import mv_ref as mr  # noqa: E402

_GN = [(case, eps) for case in L.GN_CASES for eps in L.GN_EPS]
_GN_IDS = [f"{L.gn_case_id(c)}-eps{e:g}" for c, e in _GN]


def _bounds(fn, x, C, eps, silu_too=True):
    """(element-wise error / ELEM_BOUND at gamma, beta drawn; the same with SiLU;
    rstd error, its floor) of the f16-returning implementation fn."""
    G = L.GN_GROUPS
    gamma, beta = L.affine(C, C)
    e0 = L.elem_error(fn(x, gamma, beta, G, eps, False), L.group_norm64(x, gamma, beta, G, eps, False))
    e1 = L.elem_error(fn(x, gamma, beta, G, eps, True), L.group_norm64(x, gamma, beta, G, eps, True))
    one, zero = torch.ones(C).half(), torch.zeros(C).half()
    ref = L.group_norm64(x, one, zero, G, eps)
    floor = L.rstd_error(ref.half(), x, G, eps)
    stat = L.rstd_error(fn(x, one, zero, G, eps), x, G, eps)
    return max(e0, e1) / L.ELEM_BOUND, stat, floor


@pytest.mark.parametrize("case,eps", _GN, ids=_GN_IDS)
def test_groupnorm_bounds_reachable_and_sharp(case, eps):
    C = case[3]
    assert L.has_offset_group(case[0], L.GN_GROUPS)
    x = L.gn_input(case, "offset")
    el, stat, floor = _bounds(L.group_norm_f32_centred, x, C, eps)
    el1, stat1, _ = _bounds(L.group_norm_f32_onepass, x, C, eps)
    print(f"{L.gn_case_id(case)} eps {eps:g}: floor {floor:.2e}; centred f32: elem {el:.2f} of bound, "
          f"rstd {stat / floor:.2f} floors; one-pass f32: elem {el1:.3g} of bound, rstd {stat1 / floor:.3g} floors")
    assert el <= 1.0 and stat <= L.STAT_MARGIN * floor
    assert stat1 > L.STAT_MARGIN * floor, "the offset inputs do not tell the one-pass variance apart"
    # zero-mean data: both forms pass, which is why the randn runs alone never noticed
    xr = L.gn_input(case, "randn")
    for fn in (L.group_norm_f32_centred, L.group_norm_f32_onepass):
        el, stat, floor = _bounds(fn, xr, C, eps)
        assert el <= 1.0 and stat <= L.STAT_MARGIN * floor


@pytest.mark.parametrize("case", L.GN_CASES, ids=L.gn_case_id)
def test_offset_groups_layout(case):
    B, H, W, C = case
    G, cpg = L.GN_GROUPS, C // L.GN_GROUPS
    x = L.gn_input(case, "offset")
    assert x.dtype == torch.float16 and x.shape == (B, H * W, C)
    xg = x.double().reshape(B, H * W, G, cpg)
    zb, zg = L.gn_zero_group(case)
    for b in range(B):
        for g in range(G):
            k = (g + 3 * b) % 8
            v = xg[b, :, g]
            if (b, g) == (zb, zg):
                assert bool((v == 0).all())
                continue
            n = v.numel()
            assert abs(float(v.mean()) - L.OFF[k]) < 6 * L.STD[k] / n ** 0.5 + abs(L.OFF[k]) * 2 ** -11
            assert 0.7 * L.STD[k] < float(v.std()) < 1.3 * L.STD[k]
    # the zero group's expected output is exactly beta / silu(beta)
    gamma, beta = L.affine(C, C)
    for silu in (False, True):
        ref = L.group_norm64(x, gamma, beta, G, 1e-5, silu).reshape(B, H * W, G, cpg)[zb, :, zg]
        want = beta.double().reshape(G, cpg)[zg]
        want = L.silu64(want) if silu else want
        assert torch.equal(ref, want.expand_as(ref))


def test_f16_ulp():
    v = torch.tensor([0.0, 2.0 ** -20, 0.05, -0.1, 1.0, 1.5, 1000.0], dtype=torch.float64)
    want = [2.0 ** -24, 2.0 ** -24, 2.0 ** -15, 2.0 ** -14, 2.0 ** -10, 2.0 ** -10, 0.5]
    assert L.f16_ulp(v).tolist() == want
    h = torch.tensor([0.05, 0.1, 1.0, 1000.0]).half()
    up = (h.view(torch.int16) + 1).view(torch.float16)
    assert ((up.double() - h.double()) == L.f16_ulp(h.double())).all()


def test_references_match_torch():
    """The written-out float64 formulas against torch's own float64 operators."""
    F = torch.nn.functional
    x = L.gn_input((2, 5, 7, 320), "offset")
    gamma, beta = L.affine(320, 1)
    want = F.group_norm(x.double().permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-6)
    torch.testing.assert_close(L.group_norm64(x, gamma, beta, 32, 1e-6), want.permute(0, 2, 1),
                               rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(L.group_norm64(x, gamma, beta, 32, 1e-6, True),
                               F.silu(want).permute(0, 2, 1), rtol=1e-9, atol=1e-9)
    r = L.ln_input(5, 320)
    torch.testing.assert_close(L.layer_norm64(r, gamma, beta, 1e-5),
                               F.layer_norm(r.double(), (320,), gamma.double(), beta.double(), 1e-5),
                               rtol=1e-9, atol=1e-9)
    h = L.geglu_grid(8)
    a, g = h.double().chunk(2, -1)
    torch.testing.assert_close(L.geglu64(h), a * F.gelu(g), rtol=1e-12, atol=1e-300)
    # fitted_rstd recovers the exact 1/std from an unrounded result, whatever mean was subtracted
    one, zero = torch.ones(320).half(), torch.zeros(320).half()
    y = L.group_norm64(x, one, zero, 32, 1e-5) + 0.25
    _, rstd = L.group_stats64(x, 32, 1e-5)
    fit = L.fitted_rstd(y, x, 32)
    live = ~torch.isnan(fit)
    assert int((~live).sum()) == 1 and bool(torch.isnan(fit[L.gn_zero_group((2, 5, 7, 320))]))
    torch.testing.assert_close(fit[live], rstd[live], rtol=1e-10, atol=0)


@pytest.mark.parametrize("rows,C", L.LN_CASES)
def test_layernorm_bounds_reachable(rows, C):
    x = L.ln_input(rows, C)
    gamma, beta = L.affine(C, C)
    got = torch.nn.functional.layer_norm(x.float(), (C,), gamma.float(), beta.float(), 1e-5).half()
    assert L.elem_error(got, L.layer_norm64(x, gamma, beta, 1e-5)) <= L.ELEM_BOUND
    one, zero = torch.ones(C).half(), torch.zeros(C).half()
    xr = x.reshape(rows, 1, C)
    floor = L.rstd_error(L.layer_norm64(x, one, zero, 1e-5).half().reshape(rows, 1, C), xr, 1, 1e-5)
    got = torch.nn.functional.layer_norm(x.float(), (C,), None, None, 1e-5).half()
    assert L.rstd_error(got.reshape(rows, 1, C), xr, 1, 1e-5) <= L.STAT_MARGIN * floor


@pytest.mark.parametrize("D", [64, 8])
def test_geglu_grid_and_f32(D):
    h = L.geglu_grid(D)
    assert h.shape[1] == 2 * D and h.shape[0] * D >= len(L.GEGLU_GATES) * len(L.GEGLU_VALUES)
    pairs = {(float(a), float(g)) for a, g in zip(h[:, :D].flatten(), h[:, D:].flatten())}
    assert len(pairs) == len(L.GEGLU_GATES) * len(L.GEGLU_VALUES)
    ref = L.geglu64(h)
    keep = ref.abs() < L.GEGLU_FINITE
    assert bool(keep.any()) and not bool(keep.all())          # the grid reaches past f16's range
    a, g = h.float().chunk(2, -1)
    got = (a * (0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752)))).half()
    err = L.elem_error(got[keep], ref[keep])
    print(f"geglu D={D}: float32 stand-in at {err / L.ELEM_BOUND:.2f} of the bound")
    assert err <= L.ELEM_BOUND


def _qkv(B, N, C, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N, C, generator=g).half() for _ in range(3)]


@pytest.mark.parametrize("N,C,heads", [(20, 320, 8), (8, 512, 8)])
def test_segment_attention_matches_restated_processors(N, C, heads):
    q, k, v = _qkv(12, N, C, 7)
    got = L.segment_attention64(q, k, v, L.mv_table(12, 6), heads, N)
    torch.testing.assert_close(got, mr.mv_attention_core(q.double(), k.double(), v.double(), heads, 6),
                               rtol=1e-12, atol=1e-12)
    got = L.segment_attention64(q, k, v, L.joint_table(12), heads, N)
    torch.testing.assert_close(got, mr.joint_attention_core(q.double(), k.double(), v.double(), heads),
                               rtol=1e-12, atol=1e-12)


def test_segment_attention_table_seg_len_and_scale():
    """What the restated processors cannot express: any table, a seg_len shorter than the key
    tensor, an explicit scale."""
    q, k, v = _qkv(3, 5, 80, 8)
    k2, v2 = _qkv(3, 12, 80, 9)[:2]
    tbl = torch.tensor([[2, 2], [0, 1], [1, 0]], dtype=torch.int32)
    got = L.segment_attention64(q, k2, v2, tbl, 2, 8, 0.05)
    for b in range(3):
        kk = torch.cat([k2[int(t), :8] for t in tbl[b]]).double()
        vv = torch.cat([v2[int(t), :8] for t in tbl[b]]).double()
        for h in range(2):
            s = slice(40 * h, 40 * h + 40)
            want = torch.softmax(q[b, :, s].double() @ kk[:, s].T * 0.05, -1) @ vv[:, s]
            torch.testing.assert_close(got[b, :, s], want, rtol=1e-12, atol=1e-12)
