"""Float64 references and hard inputs for the diffusion leaf kernels (norm_act.hip, attention.hip).

Plain torch on the CPU: written-out formulas on the f16 inputs, no device, no oracle/_ref.  Used by
test_mv_leaf_ref_host.py (which checks the inputs and bounds without the code under test) and by
test_gpu_mv_leaf_edges.py (which holds the kernels to them)."""
import math

import torch

# per-group offset / spread of offset_groups(): group g of image b takes entry (g + 3 b) % 8.
# Neighbouring groups differ, so statistics applied to the wrong group of a super-group show.
OFF = [0.0, 8.0, 60.0, -500.0, 1000.0, -30.0, 200.0, 3.0]
STD = [1.0, 1.0, 0.5, 1.0, 2.0, 0.25, 1.0, 4.0]

# element-wise bound: |got - ref| <= ELEM_BOUND * max(|ref|, 1).  Half an f16 ulp (2^-11 |ref|) is
# the output rounding nobody avoids; the other three halves cover the f32 mean of a group at
# |mean| = 1000 and the device's fast exp in SiLU.
ELEM_BOUND = 2.0 ** -9
# statistics bound: |fitted_rstd(got) / rstd64 - 1| <= STAT_MARGIN * floor, the floor being the same
# quantity for round_f16(ref), i.e. the part of the slope error that output rounding alone causes.
STAT_MARGIN = 4.0


def offset_groups(B, HW, C, G, seed, zero_group=None):
    """(B, HW, C) f16: group g of image b is randn * STD[k] + OFF[k], k = (g + 3 b) % 8, drawn in
    float64 and rounded to f16 once.  zero_group = (b, g) sets that one group to all zeros."""
    cpg = C // G
    assert cpg * G == C
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, G, cpg, generator=gen, dtype=torch.float64)
    k = (torch.arange(G)[None, :] + 3 * torch.arange(B)[:, None]) % 8          # (B, G)
    off = torch.tensor(OFF, dtype=torch.float64)[k][:, None, :, None]
    std = torch.tensor(STD, dtype=torch.float64)[k][:, None, :, None]
    x = x * std + off
    if zero_group is not None:
        x[zero_group[0], :, zero_group[1], :] = 0.0
    return x.reshape(B, HW, C).half()


def has_offset_group(B, G):
    """offset_groups(B, ., ., G) holds a group with OFF != 0 (always, unless B * G == 1)."""
    k = (torch.arange(G)[None, :] + 3 * torch.arange(B)[:, None]) % 8
    return bool((torch.tensor(OFF)[k] != 0).any())


def _grouped(x, G):
    B, HW, C = x.shape
    return x.reshape(B, HW, G, C // G)


def group_stats64(x, G, eps):
    """mean and 1/sqrt(var + eps) per (image, group), float64, centred (biased) variance."""
    xg = _grouped(x.double(), G)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, 1.0 / torch.sqrt(var + eps)


def silu64(y):
    return y / (1.0 + torch.exp(-y))


def group_norm64(x, gamma, beta, G, eps, silu=False):
    """x (B, HW, C) f16, gamma / beta (C,) f16 -> (B, HW, C) float64."""
    mean, rstd = group_stats64(x, G, eps)
    xg = _grouped(x.double(), G)
    y = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(x.shape)
    y = y * gamma.double() + beta.double()
    return silu64(y) if silu else y


def layer_norm64(x, gamma, beta, eps):
    """x (rows, C) f16 -> (rows, C) float64."""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def geglu64(h):
    """h (rows, 2 D) f16 -> h[:, :D] * gelu(h[:, D:]) with the exact (erf) GELU, float64."""
    a, g = h.double().chunk(2, -1)
    return a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))))


def segment_attention64(q, k, v, table, heads, seg_len, scale=None):
    """q (Bq, Nq, C), k / v (Bk, Nk >= seg_len, C), table (Bq, S) of batch indices into k / v.
    Query batch b attends to cat(k[table[b, s], :seg_len] for s): softmax(q k^T scale) v per head,
    float64.  Returns (Bq, Nq, C)."""
    Bq, Nq, C = q.shape
    d = C // heads
    if scale is None:
        scale = d ** -0.5
    q, k, v = q.double(), k.double(), v.double()
    out = torch.empty(Bq, Nq, C, dtype=torch.float64)
    for b in range(Bq):
        src = [int(t) for t in table[b]]
        kk = torch.cat([k[t, :seg_len] for t in src], 0)       # (S * seg_len, C)
        vv = torch.cat([v[t, :seg_len] for t in src], 0)
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            logits = (q[b, :, sl] @ kk[:, sl].T) * scale
            logits = logits - logits.max(-1, keepdim=True).values
            p = torch.exp(logits)
            out[b, :, sl] = (p / p.sum(-1, keepdim=True)) @ vv[:, sl]
    return out


def fitted_rstd(y, x, G):
    """Least-squares slope of y on x - mean64 per (image, group): with gamma = 1, beta = 0 and no
    SiLU this is the 1 / std that produced y, whatever mean was subtracted (x - mean64 sums to
    zero, so a constant shift of y does not move the slope).  Thousands of elements average the
    f16 rounding of y out.  nan for a constant group."""
    xg = _grouped(x.double(), G)
    d = xg - xg.mean(dim=(1, 3), keepdim=True)
    yg = _grouped(y.double(), G)
    return (yg * d).sum(dim=(1, 3)) / (d * d).sum(dim=(1, 3))


def rstd_error(y, x, G, eps):
    """max over the non-constant groups of |fitted_rstd(y) / rstd64 - 1|.  Only a group that is
    constant in x is left out; a nan or inf anywhere else in y is an error, not a gap."""
    _, rstd = group_stats64(x, G, eps)
    xg = _grouped(x.double(), G)
    live = ((xg - xg.mean(dim=(1, 3), keepdim=True)) ** 2).sum(dim=(1, 3)) > 0
    r = (fitted_rstd(y, x, G) / rstd - 1.0).abs()[live]
    assert bool(torch.isfinite(r).all()), "non-finite output in a non-constant group"
    return float(r.max())


def f16_ulp(v):
    """Spacing of f16 at |v| (float64 tensor in, float64 out): 2^(e - 10) for 2^e <= |v| < 2^(e+1),
    2^-24 below the normal range."""
    _, e = torch.frexp(v.abs().double())           # |v| = m 2^e, m in [0.5, 1)
    e = torch.where(v == 0, torch.full_like(e, -13), e)      # frexp(0) has exponent 0
    return torch.pow(2.0, (e.double() - 11.0).clamp(min=-24.0))


def elem_error(got, ref):
    """max |got - ref| / max(|ref|, 1): to be held against ELEM_BOUND."""
    ref = ref.double()
    return float(((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())


# ---- float32 stand-ins: what a kernel with f32 statistics can and cannot reach (host test only)
def _finish32(xg, mean, var, shape, gamma, beta, eps, silu):
    y = ((xg - mean[:, None, :, None]) * torch.rsqrt(var + eps)[:, None, :, None]).reshape(shape)
    y = y * gamma.float() + beta.float()
    if silu:
        y = y / (1.0 + torch.exp(-y))
    return y.half()


def group_norm_f32_centred(x, gamma, beta, G, eps, silu=False):
    """Two passes in float32: the mean, then the mean of (x - mean)^2.  f16 result."""
    xg = _grouped(x.float(), G)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return _finish32(xg, mean, var, x.shape, gamma, beta, eps, silu)


def group_norm_f32_onepass(x, gamma, beta, G, eps, silu=False):
    """One pass in float32: var = sum(x^2)/n - mean^2 clamped at 0 (cancels off zero).  f16 result."""
    xg = _grouped(x.float(), G)
    n = xg.shape[1] * xg.shape[3]
    mean = xg.sum(dim=(1, 3)) / n
    var = ((xg * xg).sum(dim=(1, 3)) / n - mean * mean).clamp(min=0.0)
    return _finish32(xg, mean, var, x.shape, gamma, beta, eps, silu)


# ---- the cases, shared by the host and the device test
GN_GROUPS = 32
# (B, H, W, C): the smallest shape that reaches each dispatch branch of dsu_groupnorm_nhwc_f16
GN_CASES = [
    (1, 16, 16, 320),     # super-group, 4 groups per super-group (10 channels per group)
    (1, 16, 16, 640),     # super-group, 2 groups (20)
    (1, 16, 16, 256),     # super-group, 1 group (8)
    (2, 5, 7, 320),       # fused small, values kept in registers
    (2, 15, 15, 1280),    # fused small, second read (HW * cpg / 2 > 4096, HW < 256)
    (2, 48, 48, 128),     # fused small, 4 channels per group (the VAE's 128 channels)
    (1, 5, 7, 640),       # statistics + apply (B * G < 64)
    (1, 5, 7, 2560),      # statistics + apply, channel range split (C / 8 > 256)
]
GN_EPS = [1e-5, 1e-6]
LN_CASES = [(1, 8), (5, 320), (4, 640), (7, 1280), (3, 2048)]      # (rows, C)


def gn_case_id(case):
    return "x".join(str(v) for v in case)


def gn_zero_group(case):
    """The (image, group) that gn_input() zeroes: never group 0 of image 0, never the last."""
    B = case[0]
    return (B - 1, 13)


def gn_input(case, kind):
    """kind 'offset': offset_groups with one all-zero group; 'randn': unit normal, zero mean."""
    B, H, W, C = case
    seed = 1000 + C + H
    if kind == "offset":
        return offset_groups(B, H * W, C, GN_GROUPS, seed, zero_group=gn_zero_group(case))
    gen = torch.Generator().manual_seed(seed + 1)
    return torch.randn(B, H * W, C, generator=gen, dtype=torch.float64).half()


def affine(C, seed):
    gen = torch.Generator().manual_seed(seed)
    gamma = (1 + 0.1 * torch.randn(C, generator=gen)).half()
    beta = (0.1 * torch.randn(C, generator=gen)).half()
    return gamma, beta


def ln_input(rows, C):
    """(rows, C) f16, row r drawn like group 0 of image r: OFF / STD entry (3 r) % 8."""
    return offset_groups(rows, 1, C, 1, 2000 + C + rows).reshape(rows, C)


GEGLU_GATES = [0.0, 1e-4, -1e-4, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 12.0, -12.0, 60.0, -60.0, -4.2,
               -5.0, 2.0 ** -14, -2.0 ** -14]
GEGLU_VALUES = [0.0, 1e-3, 1.0, -1.0, 7.5, -100.0, 1000.0, -1000.0, 937.5]
GEGLU_FINITE = 6e4          # entries with |ref| below this are compared (f16 tops out at 65504)


def geglu_grid(D):
    """(rows, 2 D) f16 holding every (value, gate) pair of the two lists, the grid repeated to fill
    the last row."""
    pairs = [(a, g) for g in GEGLU_GATES for a in GEGLU_VALUES]
    rows = (len(pairs) + D - 1) // D
    pairs = [pairs[i % len(pairs)] for i in range(rows * D)]
    a = torch.tensor([p[0] for p in pairs], dtype=torch.float64).reshape(rows, D)
    g = torch.tensor([p[1] for p in pairs], dtype=torch.float64).reshape(rows, D)
    return torch.cat([a, g], -1).half()


def mv_table(B, V):
    return torch.tensor([[(b // V) * V + s for s in range(V)] for b in range(B)], dtype=torch.int32)


def joint_table(B):
    half = B // 2
    return torch.tensor([[b % half, b % half + half] for b in range(B)], dtype=torch.int32)
