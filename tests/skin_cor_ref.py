"""Float64 numpy restatement of centre-of-rotation skinning, written from the rule in
include/dsu_hip.h ("Centre-of-rotation skinning"), not from csrc/cor_blend.h: dense (V,J) weights,
np.exp, the triangles added in plain ascending order, the apply in the header's operand order, one
elementwise numpy operation per product and sum, so nothing is fused.  Helpers that draw the inputs
of the host and device tests and call the host entries live here too, so both use the same cases."""
import ctypes
import functools

import numpy as np

import corrective_ref as CR
import skin_dqs_ref as D
import skin_ref as R

EPS32 = 2.0 ** -24
same_bits = CR.same_bits


# ------------------------------------------------------------------ the rule
def canonical(influences, weights, n_joints):
    """Any (influences, weights) (V,K) -> the canonical table: dense float64 sums in k order, rounded
    to f32, the joints with a weight ascending, padding -1 / 0.  -> joints (V,K') i32, weights (V,K') f32,
    K' the longest row (at least 1)."""
    infl = np.asarray(influences, np.int64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    V, K = infl.shape
    dense = np.zeros((V, n_joints))
    for v in range(V):
        for k in range(K):
            j = infl[v, k]
            if 0 <= j < n_joints and w[v, k] > 0.0:
                dense[v, j] = dense[v, j] + w[v, k]
    d32 = dense.astype(np.float32)
    n = max(1, int((d32 > 0).sum(1).max()) if V else 1)
    joints = np.full((V, n), -1, np.int32)
    out = np.zeros((V, n), np.float32)
    for v in range(V):
        js = np.flatnonzero(d32[v] > 0)
        joints[v, :len(js)] = js
        out[v, :len(js)] = d32[v, js]
    return joints, out


def dense_weights(joints, weights, n_joints):
    """W (V,J) float64 of a canonical table (a row ends at its first joint outside [0, J))."""
    joints = np.asarray(joints, np.int64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    W = np.zeros((len(joints), n_joints))
    for v in range(len(joints)):
        for k in range(joints.shape[1]):
            j = joints[v, k]
            if not 0 <= j < n_joints:
                break
            W[v, j] = w[v, k]
    return W


def centres(rest, faces, joints, weights, n_joints, sigma):
    """-> centres (V,3) float64, valid (V,) uint8 from a canonical table."""
    x = np.asarray(rest, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, J = len(x), n_joints
    W = dense_weights(joints, weights, J)
    s2 = sigma * sigma
    den, num = np.zeros(V), np.zeros((V, 3))
    with np.errstate(all="ignore"):
        for t in range(len(f)):
            ia, ib, ic = f[t]
            if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= V:
                continue
            a, b, c = x[ia], x[ib], x[ic]
            u, w = b - a, c - a
            n = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])
            area = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) / 2.0
            if not (area > 0.0 and np.isfinite(area)):
                continue
            hat = ((W[ia] + W[ib]) + W[ic]) / 3.0
            cen = ((a + b) + c) / 3.0
            s = np.zeros(V)
            on = np.flatnonzero(hat != 0.0)
            for p, j in enumerate(on):
                for k in on[p + 1:]:
                    both = (W[:, j] != 0.0) & (W[:, k] != 0.0)
                    if not both.any():
                        continue
                    d = W[:, j] * hat[k] - W[:, k] * hat[j]
                    term = (((W[:, j] * W[:, k]) * hat[j]) * hat[k]) * np.exp(-(d * d) / s2)
                    s = np.where(both, s + term, s)
            sa = s * area
            den = den + sa
            num = num + sa[:, None] * cen[None, :]
        ok = (den > 0.0) & np.isfinite(den) & np.isfinite(num).all(1)
        out = np.where(ok[:, None], num / np.where(ok, den, 1.0)[:, None], 0.0)
    return out, ok.astype(np.uint8)


def centre_bound(rest, n_faces, sigma):
    """B = 2 (T + 1 / sigma^2 + 64) 2^-52 times the bounding-box diagonal of the finite vertices."""
    x = np.asarray(rest, np.float32).astype(np.float64)
    x = x[np.isfinite(x).all(1)]
    diag = float(np.linalg.norm(x.max(0) - x.min(0))) if len(x) else 0.0
    return 2.0 * (n_faces + 1.0 / (sigma * sigma) + 64.0) * 2.0 ** -52 * diag


def _linear(p, infl, w, use, mats, minus=False):
    """L(p) (F,V,3) for p (V,3); minus: M(p) = sum_k w_k (y_k - p) instead."""
    F, V = mats.shape[0], len(p)
    L = np.zeros((F, V, 3))
    for k in range(infl.shape[1]):
        m = mats[:, np.where(use[:, k], infl[:, k], 0)]                      # (F,V,3,4)
        y = np.stack([((m[..., c, 0] * p[:, 0] + m[..., c, 1] * p[:, 1]) + m[..., c, 2] * p[:, 2]) + m[..., c, 3]
                      for c in range(3)], -1)
        if minus:
            y = y - p[None]
        L = np.where(use[None, :, k, None], L + w[None, :, k, None] * y, L)
    return L


def skin_cor(rest, influences, weights, matrices, quats, centres, valid):
    """-> (out (F,V,3) float32: the rule's result after its one rounding, out64: the unrounded value)."""
    x = np.asarray(rest, np.float32).astype(np.float64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    infl = np.asarray(influences, np.int64)
    mats, q4 = np.asarray(matrices, np.float64), np.asarray(quats, np.float64)
    cen, val = np.asarray(centres, np.float64), np.asarray(valid).astype(bool)
    F, J = mats.shape[:2]
    V, K = infl.shape
    with np.errstate(all="ignore"):
        use = (infl >= 0) & (infl < J) & (w > 0.0)
        Lx, M = _linear(x, infl, w, use, mats), _linear(cen, infl, w, use, mats, minus=True)
        b = np.zeros((F, V, 4))
        pivot = np.zeros((F, V, 4))
        has = np.zeros(V, bool)
        for k in range(K):
            q = q4[:, np.where(use[:, k], infl[:, k], 0)]                    # (F,V,4)
            first = use[:, k] & ~has
            pivot[:, first] = q[:, first]
            has |= use[:, k]
            dot = ((q[..., 0] * pivot[..., 0] + q[..., 1] * pivot[..., 1]) + q[..., 2] * pivot[..., 2]) + \
                q[..., 3] * pivot[..., 3]
            sw = np.where(dot < 0.0, -w[:, k], w[:, k])
            b = np.where(use[None, :, k, None], b + sw[..., None] * q, b)
        n2 = ((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]) + b[..., 3] * b[..., 3]
        ok = val[None, :] & (n2 > 0.0) & np.isfinite(n2)
        n = np.sqrt(np.where(ok, n2, 1.0))
        rw, rx, ry, rz = (b[..., c] / n for c in range(4))
        d = x - cen
        dx, dy, dz = d[None, :, 0], d[None, :, 1], d[None, :, 2]
        ax, ay, az = ry * dz - rz * dy, rz * dx - rx * dz, rx * dy - ry * dx
        cx, cy, cz = ry * az - rz * ay, rz * ax - rx * az, rx * ay - ry * ax
        w2 = 2.0 * rw
        rot = np.stack([w2 * ax + 2.0 * cx, w2 * ay + 2.0 * cy, w2 * az + 2.0 * cz], -1)
        out64 = np.where(ok[..., None], x[None] + (M + rot), Lx)
        return out64.astype(np.float32), out64


# ------------------------------------------------------------------ the host entries
def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def host_centres(rest, faces, joints, weights, n_joints, sigma):
    """dsu_skin_cor_centres_host on a canonical table."""
    from drawingspinup_amd import _lib
    rest = np.ascontiguousarray(rest, np.float32)
    f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), np.int32)
    joints, w = np.ascontiguousarray(joints, np.int32), np.ascontiguousarray(weights, np.float32)
    V, K = joints.shape
    cen = np.full((V, 3), -7.0)
    val = np.full(V, 9, np.uint8)
    rc = _lib.lib().dsu_skin_cor_centres_host(_p(rest), _p(f), _p(joints), _p(w), V, len(f), K, n_joints, float(sigma),
                                              _p(cen), _p(val))
    assert rc == 0, rc
    return cen, val


def host_cor(rest, infl, w, mats, quats, cen, val):
    """dsu_skin_cor_host: the text the kernel compiles (csrc/cor_blend.h), run on host arrays."""
    from drawingspinup_amd import _lib
    rest, w = np.ascontiguousarray(rest, np.float32), np.ascontiguousarray(w, np.float32)
    infl = np.ascontiguousarray(infl, np.int32)
    mats, quats = np.ascontiguousarray(mats, np.float64), np.ascontiguousarray(quats, np.float64)
    cen, val = np.ascontiguousarray(cen, np.float64), np.ascontiguousarray(val, np.uint8)
    (V, K), (F, J) = infl.shape, mats.shape[:2]
    out = np.full((F, V, 3), -7.0, np.float32)
    rc = _lib.lib().dsu_skin_cor_host(_p(rest), _p(infl), _p(w), _p(mats), _p(quats), _p(cen), _p(val), V, K, F, J,
                                      _p(out))
    assert rc == 0, rc
    return out


def plan(V, T):
    """(parts, tiles per part, tile) of the device entry, restated from the header."""
    from drawingspinup_amd import _header
    d = _header.read().defines
    tile, cap = d["DSU_COR_TILE"], d["DSU_COR_MAX_PARTS"]
    nbx = max(-(-V // 256), 1)
    parts = min(cap, -(-1024 // nbx))
    tiles = -(-T // tile)
    return parts, max(-(-tiles // parts), 1), tile


# ------------------------------------------------------------------ inputs
def quats_of(mats):
    from drawingspinup_amd import animate
    return animate.rotation_quaternions(np.asarray(mats, np.float64)[..., :3])


def smooth_weights(verts, K, J, seed):
    """influences (V,K) i32 (distinct joints, any order), weights (V,K) f32 summing to 1: K of J
    anchors scattered through the mesh's box, each vertex on its K nearest with weights that fall
    off smoothly with the distance, so that neighbouring vertices resemble each other."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(0), v.max(0)
    anchors = rng.uniform(lo, hi, (J, 3))
    dist = np.linalg.norm(v[:, None] - anchors[None], axis=-1)
    near = np.argsort(dist, axis=1, kind="stable")[:, :K]
    near = np.take_along_axis(near, np.stack([rng.permutation(K) for _ in range(len(v))]), 1)
    w = 1.0 / (np.take_along_axis(dist, near, 1) ** 2 + 1e-3 * float(np.linalg.norm(hi - lo)) ** 2)
    w = w / w.sum(1, keepdims=True)
    return near.astype(np.int32), w.astype(np.float32)


MESHES = {"tube": CR.tube, "sphere": CR.icosphere}


@functools.lru_cache(maxsize=None)
def mesh_case(name, K, J=9, seed=5):
    """rest f32, faces, canonical joints / weights, the caller's influences / weights."""
    v, f = MESHES[name]()
    infl, w = smooth_weights(v, K, J, seed + K)
    joints, cw = canonical(infl, w, J)
    return v, f, joints, cw, infl, w


@functools.lru_cache(maxsize=None)
def character():
    """skin_ref.character_case() with weights on its K = 4 nearest bones' head joints."""
    v, f, segs = R.character_case()
    _, parents, off, ends = R.humanoid()
    heads, _ = R.bones_of(parents, off, ends)
    a, b = segs[:, 0].astype(np.float64), segs[:, 1].astype(np.float64)
    ab = b - a
    p = v.astype(np.float64)
    t = np.clip(((p[:, None] - a) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0, 1)
    dd = np.linalg.norm(a + t[..., None] * ab - p[:, None], axis=-1)
    near = np.argsort(dd, axis=1, kind="stable")[:, :4]
    w = 1.0 / (np.take_along_axis(dd, near, 1) ** 2 + 1e-4)
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    return v, f, heads[near].astype(np.int32), w, len(parents)


def apply_case(name, K, F, seed):
    """A mesh with smooth weights, its host centres (sigma 0.1) and F random rigid transforms of 9 joints."""
    v, f, joints, cw, infl, w = mesh_case(name, K)
    cen, val = _host_centres_cached(name, K)
    mats = D.random_transforms(np.random.default_rng(seed), F, 9)
    return v, infl, w, mats, quats_of(mats), cen, val


@functools.lru_cache(maxsize=None)
def _host_centres_cached(name, K):
    v, f, joints, cw, _, _ = mesh_case(name, K)
    return host_centres(v, f, joints, cw, 9, 0.1)


def edge_rows(seed=13):
    """Eight vertices at K = 4, J = 9, F = 2, one edge of the apply rule each -> rest, influences,
    weights, matrices, quats, centres, valid, the rows that must come out as the linear blend of x.
      0  influences -1 and 99 in front of two valid ones
      1  a zero weight in first place: the pivot is the second influence
      2  all weights zero                                                      -> linear (0)
      3  two influences whose quaternions are q and -q, half and half
      4  an influence whose quaternion is NaN                                  -> linear
      5  a negative weight and a NaN weight among valid ones: neither contributes
      6  a quaternion that is zero, alone                                      -> n2 = 0: linear
      7  not valid                                                             -> linear"""
    rng = np.random.default_rng(seed)
    F, J = 2, 9
    mats = D.random_transforms(rng, F, J)
    mats[:, 8] = mats[:, 7]
    quats = quats_of(mats)
    quats[:, 8] = -quats[:, 7]
    quats[:, 6] = np.nan
    quats[:, 5] = 0.0
    rest = rng.uniform(-0.6, 0.6, (8, 3)).astype(np.float32)
    infl = np.array([[-1, 99, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [7, 8, -1, -1], [1, 6, 2, 3], [0, 1, 2, 3],
                     [5, -1, 99, 5], [0, 1, 2, 3]], np.int32)
    w = np.array([[0.4, 0.3, 0.2, 0.1], [0.0, 0.5, 0.3, 0.2], [0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0],
                  [0.4, 0.3, 0.2, 0.1], [0.5, -0.25, np.nan, 0.5], [0.7, 0.1, 0.1, 0.3], [0.4, 0.3, 0.2, 0.1]],
                 np.float32)
    cen = rest.astype(np.float64) + rng.uniform(-0.1, 0.1, (8, 3))
    val = np.array([1, 1, 1, 1, 1, 1, 1, 0], np.uint8)
    return rest, infl, w, mats, quats, cen, val, np.array([2, 4, 6, 7])


# ------------------------------------------------------------------ the bend tube
TUBE_R, TUBE_SEGS, TUBE_RINGS = 0.1, 24, 41


def bend_tube():
    """Open tube along y in [-1, 1], radius 0.1, 24 x 41 vertices (vertex ring * 24 + segment), two
    joints: joint 1 sits at the origin, and the weight on it is a smoothstep across |y| <= 0.3.  The
    second half of every ring is the first half negated, so the f32 mesh keeps the half turn about
    its axis exactly and the centres lie on the axis (to the rounding of their sums).
    -> rest f32, faces, influences (V,2), weights (V,2) f32."""
    y = np.linspace(-1.0, 1.0, TUBE_RINGS)
    phi = 2 * np.pi * np.arange(TUBE_SEGS // 2) / TUBE_SEGS
    cs, sn = TUBE_R * np.cos(phi), TUBE_R * np.sin(phi)
    cs, sn = np.concatenate([cs, -cs]), np.concatenate([sn, -sn])
    v = np.stack([np.broadcast_to(cs, (TUBE_RINGS, TUBE_SEGS)), np.broadcast_to(y[:, None], (TUBE_RINGS, TUBE_SEGS)),
                  np.broadcast_to(sn, (TUBE_RINGS, TUBE_SEGS))], -1).reshape(-1, 3)
    at = lambda i, k: i * TUBE_SEGS + k % TUBE_SEGS
    f = []
    for i in range(TUBE_RINGS - 1):
        for k in range(TUBE_SEGS):
            f += [[at(i, k), at(i, k + 1), at(i + 1, k + 1)], [at(i, k), at(i + 1, k + 1), at(i + 1, k)]]
    u = np.clip((y + 0.3) / 0.6, 0.0, 1.0)
    w1 = np.repeat(u * u * (3.0 - 2.0 * u), TUBE_SEGS)
    infl = np.tile(np.array([[0, 1]], np.int32), (len(v), 1))
    return v.astype(np.float32), np.asarray(f, np.int64), infl, np.stack([1.0 - w1, w1], 1).astype(np.float32)


def two_joint_clip(axis, deg):
    """(1,2,3,4): joint 0 stays, joint 1 turns by deg about `axis` through the origin."""
    mats = np.zeros((1, 2, 3, 4))
    mats[0, 0, :, :3] = np.eye(3)
    mats[0, 1, :, :3] = R.rot(axis, deg)
    return mats


def axis_distance(p, mats):
    """Distance of points (N,3) from the bent axis: the segment from (0,-1,0) to the origin and the
    turned segment from the origin to R (0,1,0)."""
    def seg(a, b):
        ab = b - a
        t = np.clip(((p - a) * ab).sum(-1) / (ab * ab).sum(), 0.0, 1.0)
        return np.linalg.norm(a + t[:, None] * ab - p, axis=-1)
    o = np.zeros(3)
    return np.minimum(seg(np.array([0.0, -1.0, 0.0]), o), seg(o, mats[0, 1, :, :3] @ np.array([0.0, 1.0, 0.0])))
