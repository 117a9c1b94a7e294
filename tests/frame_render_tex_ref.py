"""Float64 restatement of the textured frame-rendering rule (include/dsu_hip.h,
"Textured frames": dsu_mesh_render_ortho with a tex) in numpy.  Test infrastructure only.

Visibility is frame_render_ref.render_frame's, unchanged.  For a covered sample whose winner is face
(a, b, c): u = (w0 ua + w1 ub + w2 uc) / area, v likewise (uvs f32 widened to float64), tx = u T,
ty = v T, non-finite -> 0.  Image row r, column c holds uv T = (c, T - 1 - r).
  nearest:  c = clamp(floor(tx + 0.5), 0, T - 1), r = clamp(T - 1 - floor(ty + 0.5), 0, T - 1),
            value = f32(u8) / f32(255).
  bilinear: x = clamp(tx, 0, T - 1), y = clamp(T - 1 - ty, 0, T - 1), c0 = floor(x), c1 = min(c0 + 1,
            T - 1), rows likewise, fx = x - c0, fy = y - r0, value = ((1-fx)(1-fy) p00 + fx(1-fy) p01 +
            (1-fx) fy p10 + fx fy p11) / 255 in float64 in this order, rounded to f32.
Per pixel: float64 mean over the covered samples in row-major order, uint8 = floor(v 255 + 0.5).
"""
import numpy as np

import frame_render_ref as R

NEAREST, BILINEAR = "nearest", "bilinear"


def texel_coordinates(u, v, T):
    """tx, ty = uv T with non-finite values taken as 0."""
    tx, ty = np.asarray(u, np.float64) * float(T), np.asarray(v, np.float64) * float(T)
    return np.where(np.isfinite(tx), tx, 0.0), np.where(np.isfinite(ty), ty, 0.0)


def sample(image, tx, ty, filter):
    """image (T,T,>=3) uint8, tx / ty (n,) float64 finite -> (n,3) float64 holding f32 values."""
    image = np.asarray(image)
    T = image.shape[0]
    top = float(T - 1)
    tx, ty = np.asarray(tx, np.float64), np.asarray(ty, np.float64)
    if filter == NEAREST:
        c = np.clip(np.floor(tx + 0.5), 0.0, top).astype(np.int64)
        r = np.clip(top - np.floor(ty + 0.5), 0.0, top).astype(np.int64)
        return (image[r, c, :3].astype(np.float32) / np.float32(255.0)).astype(np.float64)
    if filter != BILINEAR:
        raise ValueError(filter)
    x, y = np.clip(tx, 0.0, top), np.clip(top - ty, 0.0, top)
    c0, r0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    c1, r1 = np.minimum(c0 + 1, T - 1), np.minimum(r0 + 1, T - 1)
    fx, fy = (x - c0)[:, None], (y - r0)[:, None]
    p00, p01 = image[r0, c0, :3].astype(np.float64), image[r0, c1, :3].astype(np.float64)
    p10, p11 = image[r1, c0, :3].astype(np.float64), image[r1, c1, :3].astype(np.float64)
    val = (((1.0 - fx) * (1.0 - fy)) * p00 + (fx * (1.0 - fy)) * p01 + ((1.0 - fx) * fy) * p10
           + (fx * fy) * p11) / 255.0
    return val.astype(np.float32).astype(np.float64)


def render_frame(sv, faces, uv, image, pos, cx, cy, span, S, ss, filter=BILINEAR, base=None):
    """One textured frame: the dict of frame_render_ref.render_frame with the colour channels of
    `pixels` and `color_u8` taken from the texture, plus tex_fragile (N,N) bool: for nearest, covered
    samples whose tx + 0.5 or ty + 0.5 lies within 1e-6 of an integer (the texel could flip on a
    last-bit difference); empty for bilinear, which is continuous across texel boundaries.
    base: frame_render_ref.render_frame's result for the same mesh and window (any colours), when
    the caller has it already: visibility and the position pass are taken from it."""
    faces = np.asarray(faces)
    if base is None:
        base = R.render_frame(sv, faces, np.zeros((len(sv), 3), np.float32), pos, cx, cy, span, S, ss)
    N = S * ss
    T = np.asarray(image).shape[0]
    xs, ys = R.lattice(N, cx, cy, span)
    sv64 = np.asarray(sv, np.float32).astype(np.float64)
    uv64 = np.asarray(uv, np.float32).astype(np.float64)
    covered = base["face_id"] >= 0
    rgb = np.zeros((N, N, 3))
    tex_fragile = np.zeros((N, N), bool)
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
            tx, ty = texel_coordinates(u, v, T)
        rgb[Rr, Cc] = sample(image, tx, ty, filter)
        if filter == NEAREST:
            near = lambda t: np.abs(t + 0.5 - np.round(t + 0.5)) < 1e-6
            tex_fragile[Rr, Cc] = near(tx) | near(ty)
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
    out["tex_fragile"] = tex_fragile
    return out


def render(screen, faces, uv, image, pos, cx, cy, span, S, ss, filter=BILINEAR, base=None):
    """All frames: the dict of render_frame with a leading frame axis (base: frame_render_ref.render's)."""
    per = [render_frame(sv, faces, uv, image, pos, cx, cy, span, S, ss, filter,
                        None if base is None else {k: v[i] for k, v in base.items()})
           for i, sv in enumerate(np.asarray(screen))]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}
