"""Float64 restatement of the frame-rendering rule (include/dsu_hip.h, dsu_mesh_render_ortho and
dsu_pos_edge_u8) in numpy, plus the small meshes the tests render.  Test infrastructure only.

Rule.  Fine lattice N = S * ss; sample (R, C) at x = cx + ((C + 0.5) / N - 0.5) * span,
y = cy - ((R + 0.5) / N - 0.5) * span.  Edge functions of the f32 vertices in float64, both
orientations, edges inclusive, area = w0 + w1 + w2 != 0.  z = (w0 za + w1 zb + w2 zc) / area rounded
to f32, largest z wins, equal z -> lowest face.  Per pixel: alpha = covered / ss^2, rgb = mean over
the covered samples (row-major) of (w0 va + w1 vb + w2 vc) / area, uint8 = floor(v 255 + 0.5).
"""
import numpy as np


def lattice(N, cx, cy, span):
    i = np.arange(N, dtype=np.float64)
    t = ((i + 0.5) / float(N) - 0.5) * float(span)
    return float(cx) + t, float(cy) - t          # xs over columns, ys over rows


def _edge(px, py, ax, ay, bx, by, cx, cy):
    w0 = (px - bx) * (cy - by) - (py - by) * (cx - bx)
    w1 = (px - cx) * (ay - cy) - (py - cy) * (ax - cx)
    w2 = (px - ax) * (by - ay) - (py - ay) * (bx - ax)
    return w0, w1, w2


def quantise(v):
    return np.floor(np.asarray(v, np.float64) * 255.0 + 0.5).astype(np.uint8)


def render_frame(sv, faces, colour, pos, cx, cy, span, S, ss):
    """One frame.  sv (V,3) f32.  Returns dict: face_id (N,N) i32, depth (N,N) f32, fragile (N,N) bool,
    pixels (S,S,8) f64 (colour rgb, alpha, pos rgb, alpha), color_u8 / pos_u8 (S,S,4)."""
    N = S * ss
    xs, ys = lattice(N, cx, cy, span)
    sv = np.asarray(sv, np.float32).astype(np.float64)
    face_id = np.full((N, N), -1, np.int32)
    best = np.full((N, N), -np.inf, np.float32)
    z1 = np.full((N, N), -np.inf)                 # two largest covering depths (f64), for `fragile`
    z2 = np.full((N, N), -np.inf)
    near_edge = np.zeros((N, N), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for m, (ia, ib, ic) in enumerate(np.asarray(faces)):
            a, b, c = sv[ia], sv[ib], sv[ic]
            xmin, xmax = min(a[0], b[0], c[0]), max(a[0], b[0], c[0])
            ymin, ymax = min(a[1], b[1], c[1]), max(a[1], b[1], c[1])
            c0 = max(int(np.searchsorted(xs, xmin, "left")) - 1, 0)
            c1 = min(int(np.searchsorted(xs, xmax, "right")), N - 1)
            r0 = max(int(np.searchsorted(-ys, -ymax, "left")) - 1, 0)
            r1 = min(int(np.searchsorted(-ys, -ymin, "right")), N - 1)
            if c1 < c0 or r1 < r0:
                continue
            px, py = xs[None, c0:c1 + 1], ys[r0:r1 + 1, None]
            w0, w1, w2 = _edge(px, py, a[0], a[1], b[0], b[1], c[0], c[1])
            area = w0 + w1 + w2
            ok = area != 0.0
            inside = ok & (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0)))
            sl = (slice(r0, r1 + 1), slice(c0, c1 + 1))
            wmin = np.minimum(np.minimum(np.abs(w0), np.abs(w1)), np.abs(w2))
            near_edge[sl] |= ok & (wmin < 1e-9 * np.abs(area))
            if not inside.any():
                continue
            z64 = (w0 * a[2] + w1 * b[2] + w2 * c[2]) / area
            z32 = z64.astype(np.float32) + np.float32(0.0)
            win = inside & (z32 > best[sl])          # faces in index order: ties keep the lower one
            best[sl] = np.where(win, z32, best[sl])
            face_id[sl] = np.where(win, m, face_id[sl])
            zc = np.where(inside, z64, -np.inf)
            top, sec = z1[sl], z2[sl]
            z2[sl] = np.maximum(np.minimum(top, zc), sec)
            z1[sl] = np.maximum(top, zc)
    covered = face_id >= 0
    with np.errstate(invalid="ignore"):
        fragile = near_edge | (covered & np.isfinite(z2) & (z1 - z2 < 1e-6 * span))
    depth = np.where(covered, best, np.float32(0.0)).astype(np.float32)
    # attributes of the winners
    attr = np.zeros((N, N, 6))
    R, C = np.nonzero(covered)
    if len(R):
        fc = np.asarray(faces)[face_id[R, C]]
        a, b, c = sv[fc[:, 0]], sv[fc[:, 1]], sv[fc[:, 2]]
        w0, w1, w2 = _edge(xs[C], ys[R], a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1])
        area = w0 + w1 + w2
        both = np.concatenate([np.clip(np.asarray(colour, np.float32), 0, 1),
                               np.clip(np.asarray(pos, np.float32), 0, 1)], 1).astype(np.float64)
        attr[R, C] = (w0[:, None] * both[fc[:, 0]] + w1[:, None] * both[fc[:, 1]]
                      + w2[:, None] * both[fc[:, 2]]) / area[:, None]
    acc = np.zeros((S, S, 6))
    cnt = np.zeros((S, S))
    for sy in range(ss):
        for sx in range(ss):
            cv = covered[sy::ss, sx::ss]
            acc += np.where(cv[..., None], attr[sy::ss, sx::ss], 0.0)
            cnt += cv
    v = np.where(cnt[..., None] > 0, acc / np.maximum(cnt, 1)[..., None], 0.0)
    alpha = cnt / float(ss * ss)
    pixels = np.concatenate([v[..., :3], alpha[..., None], v[..., 3:], alpha[..., None]], -1)
    q = quantise(pixels)
    return {"face_id": face_id, "depth": depth, "fragile": fragile, "pixels": pixels,
            "color_u8": q[..., :4], "pos_u8": q[..., 4:]}


def render(screen, faces, colour, pos, cx, cy, span, S, ss):
    """All frames: the dict of render_frame with a leading frame axis."""
    per = [render_frame(sv, faces, colour, pos, cx, cy, span, S, ss) for sv in np.asarray(screen)]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def frames_tensor(color_u8, pos_u8):
    """DatasetFullImages with mask and pos on, from the uint8 images (entry/data.py): (F,6,S,S) f32."""
    c = color_u8.astype(np.float32) / np.float32(255.0)
    p = pos_u8.astype(np.float32) / np.float32(255.0)
    half = np.float32(0.5)
    rgb = (c[..., :3] - half) / half
    xy = (p[..., :2] - half) / half
    out = np.concatenate([rgb, c[..., 3:4], xy], -1)
    return np.ascontiguousarray(np.moveaxis(out, -1, 1))


def pos_edge(pos_u8):
    """pos2edge on one (H,W,4) RGBA8 position image, stored inverted (255 = no edge)."""
    ch = pos_u8[..., :3].astype(np.float32) / np.float32(255.0)
    ch[pos_u8[..., 3] < 255] = 2.0
    best = np.zeros(pos_u8.shape[:2])
    for k in range(3):
        p = np.pad(ch[..., k].astype(np.float64), 1, mode="reflect")     # BORDER_REFLECT_101
        gx = (p[:-2, 2:] - p[:-2, :-2]) + 2.0 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
        gy = (p[2:, :-2] - p[:-2, :-2]) + 2.0 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
        best = np.maximum(best, np.sqrt(gx * gx + gy * gy))
    return np.where(best > 0.3, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ meshes
def quad(x0, y0, x1, y1, z, first=0):
    """Axis-aligned rectangle at depth z: 4 vertices, 2 triangles (vertex ids from `first`)."""
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int64) + first
    return v, f


def grid_mesh(n, x0, y0, step, z_of=None):
    """(n+1)^2 vertices on a regular grid from (x0, y0) with spacing `step`, 2 n^2 triangles."""
    j, i = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, y = x0 + i * step, y0 + j * step
    z = np.zeros_like(x) if z_of is None else z_of(i, j)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float64)
    k = (j[:-1, :-1] * (n + 1) + i[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([k, k + 1, k + n + 2], 1), np.stack([k, k + n + 2, k + n + 1], 1)])
    return v, f.astype(np.int64)


def icosphere(subdiv):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
         [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5],
         [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.asarray(v), np.asarray(f, np.int64)


def noisy_icosphere(subdiv, radius, amp, seed):
    v, f = icosphere(subdiv)
    rng = np.random.default_rng(seed)
    k = rng.normal(size=(4, 3)) * 3.0
    bump = sum(np.sin(v @ kk + ph) for kk, ph in zip(k, rng.uniform(0, 6.28, 4))) / 4.0
    return v * (radius * (1.0 + amp * bump))[:, None], f


def torus(nu, nv, R, r):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), r * np.sin(w), (R + r * np.cos(w)) * np.sin(u)], -1)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return v.reshape(-1, 3), np.asarray(f, np.int64)


def merge(*meshes):
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(v); fs.append(f + n); n += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def turn(v, angle, tilt=0.0):
    """v turned about the y axis by `angle`, then about x by `tilt`."""
    c, s = np.cos(angle), np.sin(angle)
    out = np.stack([c * v[:, 0] + s * v[:, 2], v[:, 1], -s * v[:, 0] + c * v[:, 2]], -1)
    c, s = np.cos(tilt), np.sin(tilt)
    return np.stack([out[:, 0], c * out[:, 1] - s * out[:, 2], s * out[:, 1] + c * out[:, 2]], -1)


def vertex_colours(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def general_cases():
    """name -> (screen (3,V,3) f32, faces, colour, pos): three frames of a rotation."""
    from drawingspinup_amd.animate import position_colours
    out = {}
    meshes = {"icosphere": noisy_icosphere(3, 0.5, 0.25, 11),
              "torus": torus(48, 20, 0.42, 0.17),
              "two_blobs": merge((lambda m: (m[0] + [0.12, 0.05, 0.1], m[1]))(noisy_icosphere(2, 0.3, 0.3, 5)),
                                 (lambda m: (m[0] - [0.1, 0.04, 0.12], m[1]))(noisy_icosphere(2, 0.33, 0.2, 6)))}
    for k, (name, (v, f)) in enumerate(meshes.items()):
        screen = np.stack([turn(v, 0.37 + 0.9 * j, 0.21 * (j + 1)) for j in range(3)]).astype(np.float32)
        out[name] = (screen, f, vertex_colours(len(v), 100 + k), position_colours(v).astype(np.float32))
    return out
