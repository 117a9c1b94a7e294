"""Float64 restatement of the anisotropic frame-rendering rule (include/dsu_hip.h, "Anisotropic
frames": DSU_TEX_ANISOTROPIC, dsu_aniso_sample_host) in numpy, written from the header's text.  Test
infrastructure only.

Per (frame, face): A, B, C, D from the texel-per-sample Jacobian, s1 = sqrt(m + r), s2 = |D| / s1, the
unit major axis, N = min(ceil(s1 / s2), cap) probes and the level (k, t) of rho' = s1 / N (footprint).
Per sample: the unrounded trilinear values of the N probes along the axis, summed in ascending order,
divided by N and by 255, rounded once to f32 (sample).  The pyramid and the level rule are
frame_render_mip_ref's, visibility is frame_render_ref's.
"""
import numpy as np

import frame_render_mip_ref as MR
import frame_render_ref as R

ANISOTROPIC = "anisotropic"
MAX_ANISO = 16


def footprint(a, b, c, ta, tb, tc, T, h, cap, L):
    """a, b, c (n,>=2) float64 screen vertices (from f32), ta, tb, tc (n,2) float64 uvs (from f32),
    h = span / N_lattice, cap in 1..16, L levels -> dict of (n,) arrays: s1, N (int64), ax, ay, rho, k, t."""
    assert 1 <= int(cap) <= MAX_ANISO
    a, b, c, ta, tb, tc = (np.asarray(x, np.float64) for x in (a, b, c, ta, tb, tc))
    h = float(h)
    with np.errstate(all="ignore"):
        e1x, e1y, e2x, e2y = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
        p1, q1 = (tb[:, 0] - ta[:, 0]) * float(T), (tb[:, 1] - ta[:, 1]) * float(T)
        p2, q2 = (tc[:, 0] - ta[:, 0]) * float(T), (tc[:, 1] - ta[:, 1]) * float(T)
        det = e1x * e2y - e1y * e2x
        dpx, dpy = (p1 * e2y - p2 * e1y) / det, (p2 * e1x - p1 * e2x) / det
        dqx, dqy = (q1 * e2y - q2 * e1y) / det, (q2 * e1x - q1 * e2x) / det
        hh = h * h
        A, C = hh * (dpx * dpx + dpy * dpy), hh * (dqx * dqx + dqy * dqy)
        B, D = hh * (dpx * dqx + dpy * dqy), hh * (dpx * dqy - dpy * dqx)
        m, d = (A + C) * 0.5, (A - C) * 0.5
        r = np.sqrt(d * d + B * B)
        s1 = np.sqrt(m + r)
        ok = det != 0.0
        for q in (A, B, C, D, r, s1):
            ok = ok & np.isfinite(q)
        s2 = np.abs(D) / s1
        vx, vy = np.where(d >= 0.0, d + r, B), np.where(d >= 0.0, B, r - d)
        n = np.sqrt(vx * vx + vy * vy)
        unit = ok & (n != 0.0) & np.isfinite(n)
        ax, ay = np.where(unit, vx / n, 1.0), np.where(unit, vy / n, 0.0)
        q = np.ceil(s1 / s2)
        many = np.where(q < float(cap), q, float(cap))        # compared in float64, before the conversion
        N = np.where(~(s1 > 1.0), 1.0, np.where(~(s2 > 0.0), float(cap), many))
        N = np.where(ok, N, 1.0)
        s1 = np.where(ok, s1, 0.0)
        rho = np.where(ok, s1 / N, 0.0)
    k, t = MR.lod(rho, L)
    return {"s1": s1, "N": N.astype(np.int64), "ax": ax, "ay": ay, "rho": rho, "k": k, "t": t}


def _value(levels, tx, ty, k, t):
    """The unrounded trilinear value at (k, t): B_k, or (1 - t) B_k + t B_{k+1}; (n,3) float64."""
    T = levels[0].shape[0]
    tx, ty = np.where(np.isfinite(tx), tx, 0.0), np.where(np.isfinite(ty), ty, 0.0)
    x0, y0 = tx, float(T - 1) - ty
    out = np.zeros((len(tx), 3))
    for j in np.unique(k):
        sel = np.nonzero(k == j)[0]
        j = int(j)
        s, half = float(1 << j), (float(1 << j) - 1.0) / 2.0
        val = MR._blend(levels[j], (x0[sel] - half) / s, (y0[sel] - half) / s)
        two = t[sel] != 0.0
        if two.any():
            s_up, half_up = float(2 << j), (float(2 << j) - 1.0) / 2.0
            w = t[sel][two][:, None]
            up = MR._blend(levels[j + 1], (x0[sel][two] - half_up) / s_up, (y0[sel][two] - half_up) / s_up)
            val[two] = (1.0 - w) * val[two] + w * up
        out[sel] = val
    return out


def sample(levels, tx, ty, fp):
    """levels from frame_render_mip_ref.pyramid(); tx, ty (n,) float64 as formed (uv T: a non-finite
    coordinate is taken as 0 per probe); fp from footprint() -> (n,3) float64 holding f32 values."""
    tx, ty = np.asarray(tx, np.float64), np.asarray(ty, np.float64)
    N = fp["N"]
    total = np.zeros((len(tx), 3))
    with np.errstate(all="ignore"):
        for i in range(int(N.max()) if len(N) else 0):
            sel = np.nonzero(N > i)[0]
            o = (float(2 * i + 1) / (2 * N[sel]).astype(np.float64) - 0.5) * fp["s1"][sel]
            total[sel] += _value(levels, tx[sel] + o * fp["ax"][sel], ty[sel] + o * fp["ay"][sel],
                                 fp["k"][sel], fp["t"][sel])
    return ((total / N.astype(np.float64)[:, None]) / 255.0).astype(np.float32).astype(np.float64)


def render_frame(sv, faces, uv, levels, pos, cx, cy, span, S, ss, cap, base=None):
    """One anisotropic frame: the dict of frame_render_mip_ref.render_frame with lod_k the probes' level,
    plus probes (N,N) int64 (the N of the sample's face, 0 where empty) and rgb (N,N,3) per sample."""
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
    probes = np.zeros((N, N), np.int64)
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
            tx, ty = u * float(T), v * float(T)
        fp = footprint(a, b, c, ta, tb, tc, T, float(span) / float(N), cap, L)
        rgb[Rr, Cc] = sample(levels, tx, ty, fp)
        lod_k[Rr, Cc] = fp["k"]
        probes[Rr, Cc] = fp["N"]
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
    out["probes"] = probes
    out["rgb"] = rgb
    return out


def render(screen, faces, uv, levels, pos, cx, cy, span, S, ss, cap, base=None):
    """All frames (base: frame_render_ref.render's)."""
    per = [render_frame(sv, faces, uv, levels, pos, cx, cy, span, S, ss, cap,
                        None if base is None else {k: v[i] for k, v in base.items()})
           for i, sv in enumerate(np.asarray(screen))]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}
