"""Float64 numpy restatement of dual-quaternion skinning, written from the rule in include/dsu_hip.h
("Dual-quaternion skinning"), not from csrc/dqs_blend.h: the same operations in the same operand
order, one elementwise numpy operation per product and sum, so nothing is fused.  Helpers that draw
the inputs of the host and device tests live here too, so both use the same cases."""
import ctypes

import numpy as np

import skin_ref as R

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


def bound(ref64, scale):
    """The one final rounding to f32, plus float64 noise of the conversion and blend with room."""
    return EPS32 * np.abs(ref64) + 256.0 * EPS64 * scale


def skin_dqs(rest, influences, weights, dualquats):
    """-> (out (F,V,3) float32: the rule's result after its one rounding, out64 (F,V,3): the
    unrounded float64 value, scale (F,V,3): |R||x| + |t| of the blended transform, the magnitude the
    bounds are stated on).  Where the rule falls back to the rest position, out64 is the rest
    position and scale |x|."""
    x = np.asarray(rest, np.float32).astype(np.float64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    infl = np.asarray(influences, np.int64)
    dq = np.asarray(dualquats, np.float64)
    F, J = dq.shape[:2]
    V, K = infl.shape
    b = np.zeros((F, V, 8))
    pivot = np.zeros((F, V, 4))
    has = np.zeros(V, bool)
    with np.errstate(all="ignore"):
        for k in range(K):
            jn = infl[:, k]
            use = (jn >= 0) & (jn < J) & (w[:, k] > 0.0)
            q = dq[:, np.where(use, jn, 0)]                                    # (F,V,8)
            first = use & ~has
            pivot[:, first] = q[:, first, :4]
            has |= use
            dot = ((q[..., 0] * pivot[..., 0] + q[..., 1] * pivot[..., 1]) + q[..., 2] * pivot[..., 2]) + \
                q[..., 3] * pivot[..., 3]
            sw = np.where(dot < 0.0, -w[:, k], w[:, k])                        # (F,V)
            b = np.where(use[None, :, None], b + sw[..., None] * q, b)
        n2 = ((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]) + b[..., 3] * b[..., 3]
        ok = (n2 > 0.0) & np.isfinite(n2)
        n = np.sqrt(np.where(ok, n2, 1.0))
        r = b[..., :4] / n[..., None]
        d = b[..., 4:] / n[..., None]
        rw, rx, ry, rz = (r[..., c] for c in range(4))
        dw, dx, dy, dz = (d[..., c] for c in range(4))
        tx = 2.0 * ((rw * dx - dw * rx) + (ry * dz - rz * dy))
        ty = 2.0 * ((rw * dy - dw * ry) + (rz * dx - rx * dz))
        tz = 2.0 * ((rw * dz - dw * rz) + (rx * dy - ry * dx))
        X, Y, Z = x[None, :, 0], x[None, :, 1], x[None, :, 2]
        ax, ay, az = ry * Z - rz * Y, rz * X - rx * Z, rx * Y - ry * X
        cx, cy, cz = ry * az - rz * ay, rz * ax - rx * az, rx * ay - ry * ax
        w2 = 2.0 * rw
        out64 = np.stack([((X + w2 * ax) + 2.0 * cx) + tx, ((Y + w2 * ay) + 2.0 * cy) + ty,
                          ((Z + w2 * az) + 2.0 * cz) + tz], -1)
        # |R||x| + |t| with R the matrix of r
        Rm = np.empty((F, V, 3, 3))
        Rm[..., 0, 0] = 1.0 - 2.0 * (ry * ry + rz * rz); Rm[..., 0, 1] = 2.0 * (rx * ry - rw * rz)
        Rm[..., 0, 2] = 2.0 * (rx * rz + rw * ry); Rm[..., 1, 0] = 2.0 * (rx * ry + rw * rz)
        Rm[..., 1, 1] = 1.0 - 2.0 * (rx * rx + rz * rz); Rm[..., 1, 2] = 2.0 * (ry * rz - rw * rx)
        Rm[..., 2, 0] = 2.0 * (rx * rz - rw * ry); Rm[..., 2, 1] = 2.0 * (ry * rz + rw * rx)
        Rm[..., 2, 2] = 1.0 - 2.0 * (rx * rx + ry * ry)
        scale = np.einsum("fvab,vb->fva", np.abs(Rm), np.abs(x)) + np.abs(np.stack([tx, ty, tz], -1))
    rest_b = np.broadcast_to(x, out64.shape)
    out64 = np.where(ok[..., None], out64, rest_b)
    scale = np.where(ok[..., None], scale, np.abs(rest_b))
    with np.errstate(all="ignore"):
        return out64.astype(np.float32), out64, scale


def host_dqs(rest, infl, w, table):
    """dsu_skin_dqs_host: the text the kernel compiles (csrc/dqs_blend.h), run on host arrays."""
    from drawingspinup_amd import _lib
    rest, w = np.ascontiguousarray(rest, np.float32), np.ascontiguousarray(w, np.float32)
    infl, table = np.ascontiguousarray(infl, np.int32), np.ascontiguousarray(table, np.float64)
    (V, K), (F, J) = infl.shape, table.shape[:2]
    out = np.full((F, V, 3), -7.0, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert _lib.lib().dsu_skin_dqs_host(p(rest), p(infl), p(w), p(table), V, K, F, J, p(out)) == 0
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ inputs
def random_transforms(rng, F, J):
    """(F,J,3,4) float64: rotations over the full range, translations in +-0.5, drawn as _skin_inputs
    of tests/test_gpu_skin.py draws them."""
    mats = np.empty((F, J, 3, 4))
    for fr in range(F):
        for j in range(J):
            a = rng.uniform(-180, 180, 3)
            mats[fr, j, :, :3] = R.rot("Z", a[0]) @ R.rot("X", a[1]) @ R.rot("Y", a[2])
            mats[fr, j, :, 3] = rng.uniform(-0.5, 0.5, 3)
    return mats


def table_of(mats):
    """[R | t] (F,J,3,4) -> (F,J,8), restated apart from animate.dual_quaternions: the quaternion
    through the rotation's axis and angle (eigenvector of eigenvalue 1, angle from trace and the
    antisymmetric part), then d = 1/2 (0, t) (x) r."""
    m = np.asarray(mats, np.float64)
    out = np.empty(m.shape[:2] + (8,))
    for f in range(m.shape[0]):
        for j in range(m.shape[1]):
            Rm, t = m[f, j, :, :3], m[f, j, :, 3]
            vals, vecs = np.linalg.eig(Rm)
            a = np.real(vecs[:, np.argmin(np.abs(vals - 1.0))])
            a /= np.linalg.norm(a)
            skew = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
            ang = np.arctan2(0.5 * (skew @ a), 0.5 * (np.trace(Rm) - 1.0))
            r = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * a])
            if r[0] < 0:
                r = -r
            out[f, j, :4] = r
            out[f, j, 4] = -0.5 * (t @ r[1:])
            out[f, j, 5:] = 0.5 * (r[0] * t + np.cross(t, r[1:]))
    return out


def skin_inputs(V, K, F, J, seed):
    """rest (V,3) f32, influences (V,K) i32 (distinct joints per vertex), weights (V,K) f32 summing to
    1, transforms (F,J,3,4) f64."""
    rng = np.random.default_rng(seed)
    rest = rng.uniform(-0.6, 0.6, (V, 3)).astype(np.float32)
    infl = np.stack([rng.permutation(J)[:K] for _ in range(V)]).astype(np.int32)
    w = rng.random((V, K)) + 0.05
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    return rest, infl, w, random_transforms(rng, F, J)


def edge_rows(seed=11):
    """Seven vertices at K = 4, J = 9, F = 2, one edge of the rule each -> rest, influences, weights,
    table, the rows that must come out as the rest position.
      0  influences -1 and 99 in front of two valid ones
      1  a zero weight in first place: the pivot is the second influence
      2  all weights zero                                                      -> rest
      3  two influences with opposite rotations (joint 8 = -joint 7), half and half
      4  an influence whose table entry is NaN                                 -> rest
      5  a negative weight and a NaN weight among valid ones: neither contributes
      6  an entry whose rotation part is zero, alone                           -> n2 = 0, rest
    Row 3 cannot reach n2 = 0: the antipodal choice makes every contribution's rotation part have a
    non-negative dot product with the pivot's, so with unit quaternions b_r . r_pivot >= w_pivot > 0;
    q and -q add (the row comes out as joint 7's rigid transform).  n2 = 0 needs a table entry
    that is no unit quaternion: row 6."""
    rng = np.random.default_rng(seed)
    F, J = 2, 9
    table = table_of(random_transforms(rng, F, J))
    table[:, 8] = -table[:, 7]
    table[:, 6] = np.nan
    table[:, 5, :4] = 0.0
    rest = rng.uniform(-0.6, 0.6, (7, 3)).astype(np.float32)
    infl = np.array([[-1, 99, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [7, 8, -1, -1], [1, 6, 2, 3], [0, 1, 2, 3],
                     [5, -1, 99, 5]], np.int32)
    w = np.array([[0.4, 0.3, 0.2, 0.1], [0.0, 0.5, 0.3, 0.2], [0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0],
                  [0.4, 0.3, 0.2, 0.1], [0.5, -0.25, np.nan, 0.5], [0.7, 0.1, 0.1, 0.3]], np.float32)
    return rest, infl, w, table, np.array([2, 4, 6])
