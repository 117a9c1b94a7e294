"""Float64 / integer restatement of the mip-mapped frame-rendering rule (include/dsu_hip.h,
"Mip-mapped frames": dsu_mip_pyramid_build, DSU_TEX_TRILINEAR) in numpy.  Test
infrastructure only.

Pyramid: T_0 = T, T_k = ceil(T_{k-1} / 2), L levels down to size 1.  Level 0 is the input.  Texel
(r, c) of level k >= 1 is the rounded mean (2 sum + n) // (2 n) of the covered level-0 texels in rows
[2^k r, 2^k (r + 1)) and the columns likewise, clipped to the image — taken here by brute force over
the level-0 block, with no carried sums —, then `gutter` rounds of uv_ref.dilate on that level;
alpha = 255 where covered after the rounds, else the whole texel is 0.

Sampling: rho per (frame, face) from the screen vertices and the uvs (footprint), level k and
weight t from rho (lod), the level coordinates x_j = (x_0 - (2^j - 1) / 2) / 2^j and the blend
((1 - t) B_k + t B_{k+1}) / 255 rounded once to f32 (sample).  Visibility is frame_render_ref's.
"""
import numpy as np

import frame_render_ref as R
import frame_render_tex_ref as TR
import uv_ref

TRILINEAR = "trilinear"


def level_sizes(T):
    sizes = [int(T)]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + 1) // 2)
    return sizes


def level_offsets(T):
    """Texel offset of every level in the pyramid buffer, and the total as the last entry."""
    return [0] + list(np.cumsum([s * s for s in level_sizes(T)]))


def pyramid(image, covered=None, gutter=2):
    """image (T,T,4) uint8, covered (T,T) bool or None -> list of (T_k,T_k,4) uint8 levels."""
    image = np.asarray(image, np.uint8)
    T = image.shape[0]
    assert image.shape == (T, T, 4)
    cov = np.ones((T, T), bool) if covered is None else np.asarray(covered).astype(bool)
    levels = [image.copy()]
    rgb = image[..., :3].astype(np.int64) * cov[..., None]
    for k, Tk in enumerate(level_sizes(T)):
        if k == 0:
            continue
        b = 1 << k
        out = np.zeros((Tk, Tk, 3), np.uint8)
        has = np.zeros((Tk, Tk), bool)
        for r in range(Tk):
            for c in range(Tk):
                n = int(cov[b * r:b * (r + 1), b * c:b * (c + 1)].sum())
                if n:
                    total = rgb[b * r:b * (r + 1), b * c:b * (c + 1)].reshape(-1, 3).sum(0)
                    out[r, c] = (2 * total + n) // (2 * n)
                    has[r, c] = True
        out, has = uv_ref.dilate(out, has, gutter)
        levels.append(np.concatenate([out * has[..., None].astype(np.uint8),
                                      np.where(has, 255, 0).astype(np.uint8)[..., None]], -1))
    return levels


def flatten(levels):
    """The pyramid buffer: (sum T_k^2, 4) uint8."""
    return np.concatenate([lv.reshape(-1, 4) for lv in levels])


def footprint(a, b, c, ta, tb, tc, T, h):
    """rho per face: a, b, c (n,>=2) float64 screen vertices (from f32), ta, tb, tc (n,2) float64 uvs
    (from f32), h = span / N."""
    with np.errstate(all="ignore"):
        e1x, e1y, e2x, e2y = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
        p1, q1 = (tb[:, 0] - ta[:, 0]) * float(T), (tb[:, 1] - ta[:, 1]) * float(T)
        p2, q2 = (tc[:, 0] - ta[:, 0]) * float(T), (tc[:, 1] - ta[:, 1]) * float(T)
        det = e1x * e2y - e1y * e2x
        dpx, dpy = (p1 * e2y - p2 * e1y) / det, (p2 * e1x - p1 * e2x) / det
        dqx, dqy = (q1 * e2y - q2 * e1y) / det, (q2 * e1x - q1 * e2x) / det
        gx, gy = dpx * dpx + dqx * dqx, dpy * dpy + dqy * dqy
        rho = np.sqrt((h * h) * np.where(gx > gy, gx, gy))
    return np.where(det == 0.0, 0.0, rho)


def lod(rho, L):
    """rho (n,) -> k (n,) int64, t (n,) float64."""
    rho = np.asarray(rho, np.float64)
    with np.errstate(invalid="ignore"):
        up = np.isfinite(rho) & (rho > 1.0)
    safe = np.where(up, rho, 1.0)
    e = np.frexp(safe)[1].astype(np.int64) - 1               # floor(log2 rho), from the exponent
    top = e >= L - 1
    k = np.where(up, np.where(top, L - 1, e), 0)
    t = np.where(up & ~top, np.ldexp(safe, -e.astype(np.int32)) - 1.0, 0.0)
    return k, t


def _blend(level, x, y):
    """The bilinear filter's four-term expression on one level, before division and rounding."""
    Tj = level.shape[0]
    top = float(Tj - 1)
    x, y = np.clip(x, 0.0, top), np.clip(y, 0.0, top)
    c0, r0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    c1, r1 = np.minimum(c0 + 1, Tj - 1), np.minimum(r0 + 1, Tj - 1)
    fx, fy = (x - c0)[:, None], (y - r0)[:, None]
    p00, p01 = level[r0, c0, :3].astype(np.float64), level[r0, c1, :3].astype(np.float64)
    p10, p11 = level[r1, c0, :3].astype(np.float64), level[r1, c1, :3].astype(np.float64)
    return (((1.0 - fx) * (1.0 - fy)) * p00 + (fx * (1.0 - fy)) * p01 + ((1.0 - fx) * fy) * p10
            + (fx * fy) * p11)


def sample(levels, tx, ty, k, t):
    """levels from pyramid(); tx, ty (n,) float64 (any values: non-finite -> 0); k, t from lod()
    -> (n,3) float64 holding f32 values."""
    T = levels[0].shape[0]
    tx, ty = np.asarray(tx, np.float64), np.asarray(ty, np.float64)
    tx, ty = np.where(np.isfinite(tx), tx, 0.0), np.where(np.isfinite(ty), ty, 0.0)
    x0, y0 = tx, float(T - 1) - ty
    out = np.zeros((len(tx), 3))
    for j in np.unique(k):
        sel = np.nonzero(k == j)[0]
        j = int(j)
        s, half = float(1 << j), (float(1 << j) - 1.0) / 2.0
        B0 = _blend(levels[j], (x0[sel] - half) / s, (y0[sel] - half) / s)
        val = B0 / 255.0
        two = t[sel] != 0.0
        if two.any():
            s1, half1 = float(2 << j), (float(2 << j) - 1.0) / 2.0
            w = t[sel][two][:, None]
            B1 = _blend(levels[j + 1], (x0[sel][two] - half1) / s1, (y0[sel][two] - half1) / s1)
            val[two] = ((1.0 - w) * B0[two] + w * B1) / 255.0
        out[sel] = val.astype(np.float32).astype(np.float64)
    return out


def sample_rho(levels, tx, ty, rho):
    """What dsu_mip_sample_host computes: level and weight from rho, then the sample."""
    k, t = lod(rho, len(levels))
    return sample(levels, tx, ty, k, t)


def render_frame(sv, faces, uv, levels, pos, cx, cy, span, S, ss, base=None):
    """One mip-mapped frame: the dict of frame_render_tex_ref.render_frame (tex_fragile empty: the
    blend is continuous in the coordinates and in rho), plus lod_k (N,N) int64, -1 where empty."""
    faces = np.asarray(faces)
    if base is None:
        base = R.render_frame(sv, faces, np.zeros((len(sv), 3), np.float32), pos, cx, cy, span, S, ss)
    N = S * ss
    T, L = levels[0].shape[0], len(levels)
    xs, ys = R.lattice(N, cx, cy, span)
    sv64 = np.asarray(sv, np.float32).astype(np.float64)
    uv64 = np.asarray(uv, np.float32).astype(np.float64)
    covered = base["face_id"] >= 0
    rgb = np.zeros((N, N, 3))
    lod_k = np.full((N, N), -1, np.int64)
    Rr, Cc = np.nonzero(covered)
    if len(Rr):
        fc = faces[base["face_id"][Rr, Cc]]
        a, b, c = sv64[fc[:, 0]], sv64[fc[:, 1]], sv64[fc[:, 2]]
        w0, w1, w2 = R._edge(xs[Cc], ys[Rr], a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1])
        area = w0 + w1 + w2
        ta, tb, tc = uv64[fc[:, 0]], uv64[fc[:, 1]], uv64[fc[:, 2]]
        with np.errstate(invalid="ignore", over="ignore"):
            u = (w0 * ta[:, 0] + w1 * tb[:, 0] + w2 * tc[:, 0]) / area
            v = (w0 * ta[:, 1] + w1 * tb[:, 1] + w2 * tc[:, 1]) / area
            tx, ty = TR.texel_coordinates(u, v, T)
        k, t = lod(footprint(a, b, c, ta, tb, tc, T, float(span) / float(N)), L)
        rgb[Rr, Cc] = sample(levels, tx, ty, k, t)
        lod_k[Rr, Cc] = k
    acc = np.zeros((S, S, 3))
    cnt = np.zeros((S, S))
    for sy in range(ss):
        for sx in range(ss):
            cv = covered[sy::ss, sx::ss]
            acc += np.where(cv[..., None], rgb[sy::ss, sx::ss], 0.0)
            cnt += cv
    v = np.where(cnt[..., None] > 0, acc / np.maximum(cnt, 1)[..., None], 0.0)
    out = dict(base)
    out["pixels"] = base["pixels"].copy()
    out["pixels"][..., :3] = v
    out["color_u8"] = base["color_u8"].copy()
    out["color_u8"][..., :3] = R.quantise(v)
    out["tex_fragile"] = np.zeros((N, N), bool)
    out["lod_k"] = lod_k
    return out


def render(screen, faces, uv, levels, pos, cx, cy, span, S, ss, base=None):
    """All frames (base: frame_render_ref.render's)."""
    per = [render_frame(sv, faces, uv, levels, pos, cx, cy, span, S, ss,
                        None if base is None else {k: v[i] for k, v in base.items()})
           for i, sv in enumerate(np.asarray(screen))]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}
