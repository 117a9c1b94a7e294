"""Dense float64 numpy restatement of the thickness map's rule (include/dsu_hip.h, "Thickness map";
the shipped text is csrc/mesh_thickness.h): every triangle against every sample, the crossings of a
sample sorted by (z, face) and paired.  The operand order is the header's, numpy's elementwise float64
arithmetic fuses nothing, so the host entry is held to it bit for bit.  Also the meshes the thickness
and rig tests share."""
import numpy as np


def samples(v0, n, h):
    return np.float64(v0) + (np.arange(n, dtype=np.float64) + 0.5) * np.float64(h)


def _edge(px, py, qx, qy, sx, sy):
    dx, dy = qx - px, qy - py
    E = dx * (sy - py) - dy * (sx - px)
    return E, (E > 0.0) | ((E == 0.0) & ((dy < 0.0) | ((dy == 0.0) & (dx < 0.0))))


def crossings(verts, faces, x0, y0, h, W, H):
    """[(face, covered (H,W) bool, z (H,W) f64)] of the triangles the rule does not ignore."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    sx, sy = np.meshgrid(samples(x0, W, h), samples(y0, H, h))
    out = []
    for t, (ia, ib, ic) in enumerate(f):
        if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= len(v):
            continue
        a, b, c = v[ia], v[ib], v[ic]
        if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()):
            continue
        area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if area2 == 0.0:
            continue
        if area2 < 0.0:
            b, c, area2 = c, b, -area2
        eab, kab = _edge(a[0], a[1], b[0], b[1], sx, sy)
        ebc, kbc = _edge(b[0], b[1], c[0], c[1], sx, sy)
        eca, kca = _edge(c[0], c[1], a[0], a[1], sx, sy)
        z = ((ebc / area2) * a[2] + (eca / area2) * b[2]) + (eab / area2) * c[2]
        out.append((t, kab & kbc & kca, z))
    return out


def thickness(verts, faces, x0, y0, h, W, H):
    """-> (mid (H,W) f64, thickness (H,W) f64, count (H,W) i32)."""
    mid, thick = np.zeros((H, W)), np.zeros((H, W))
    count = np.zeros((H, W), np.int32)
    cr = crossings(verts, faces, x0, y0, h, W, H)
    for r in range(H):
        for c in range(W):
            hits = sorted((z[r, c], t) for t, k, z in cr if k[r, c])
            count[r, c] = len(hits)
            best = None
            for i in range(0, len(hits) - 1, 2):
                z0, z1 = hits[i][0], hits[i + 1][0]
                if best is None or z1 - z0 > best:
                    best, mid[r, c], thick[r, c] = z1 - z0, (z0 + z1) / 2.0, z1 - z0
    return mid, thick, count


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ meshes
_BOX_FACES = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7],      # z = lo, z = hi
                       [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6],      # y = lo, y = hi
                       [1, 2, 6], [1, 6, 5], [3, 0, 4], [3, 4, 7]])     # x = hi, x = lo


def box(lo, hi):
    """A closed box, 8 vertices and 12 outward faces; faces 0-1 are z = lo, 2-3 are z = hi."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0],
                  [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]], np.float32)
    return v, _BOX_FACES.astype(np.int32)


def join(parts):
    """Several (verts, faces) as one mesh of separate components."""
    vs, fs, n = [], [], 0
    for v, f in parts:
        vs.append(np.asarray(v, np.float32).reshape(-1, 3))
        fs.append(np.asarray(f, np.int32).reshape(-1, 3) + n)
        n += len(vs[-1])
    return np.concatenate(vs), np.concatenate(fs)


def rotated_box(centre, half, degrees):
    """A box turned about z through its centre (an arm raised by `degrees`)."""
    v, f = box(-np.asarray(half, np.float64), np.asarray(half, np.float64))
    a = np.radians(degrees)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return (v.astype(np.float64) @ R.T + np.asarray(centre, np.float64)).astype(np.float32), f


def icosphere(subdivisions):
    """Unit icosphere, 20 * 4^subdivisions faces, vertices on the sphere (f32)."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def slabs(n, rng):
    """n closed slabs over the unit square, stacked along z with gaps, of distinct depths: 12 n
    triangles over every sample inside, 2 n crossings.  -> (verts, faces, the largest depth, the mid
    z of that slab)."""
    depths = (1.0 + rng.permutation(n)) / 64.0
    parts, z, best = [], 0.0, None
    for d in depths:
        parts.append(box((0.0, 0.0, z), (1.0, 1.0, z + d)))
        if best is None or d > best[0]:
            best = (d, z + d / 2.0)
        z += d + 1.0 / 128.0
    v, f = join(parts)
    return v, f, best[0], best[1]


# ------------------------------------------------------------------ cases
def _open_box():
    v, f = box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    return v, f[2:]                     # without the two triangles of z = hi


def _two_boxes(d0, d1):
    return join([box((0.0, 0.0, 0.0), (1.0, 1.0, d0)), box((0.0, 0.0, 2.0), (1.0, 1.0, 2.0 + d1))])


def _broken():
    """A cube plus a face with an index out of range, a face with a negative index and a face on a NaN vertex."""
    v, f = box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    v = np.concatenate([v, np.array([[0.2, 0.2, np.nan], [0.9, 0.1, 5.0], [0.5, 0.9, 5.0]], np.float32)])
    f = np.concatenate([f, np.array([[0, 1, 11], [-1, 2, 3], [8, 9, 10], [9, 8, 10]], np.int32)])
    return v, f


def cases():
    """name -> (verts, faces, x0, y0, h, W, H): the cases of tests/test_mesh_thickness_host.py, which the
    GPU test runs again."""
    cube = box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    ico = icosphere(2)
    out = {
        "a_cube": (*cube, 0.0, 0.0, 0.25, 4, 4),
        "b_cube_rim": (*cube, -0.25, -0.25, 0.25, 6, 6),
        "c_boxes_03_05": (*_two_boxes(0.3, 0.5), 0.0, 0.0, 0.25, 4, 4),
        "c_boxes_05_03": (*_two_boxes(0.5, 0.3), 0.0, 0.0, 0.25, 4, 4),
        "c_boxes_equal": (*_two_boxes(0.5, 0.5), 0.0, 0.0, 0.25, 4, 4),
        "d_open_box": (*_open_box(), 0.0, 0.0, 0.25, 4, 4),
        "e_icosphere": (*ico, -1.03125, -1.03125, 0.0625, 33, 33),
        "g_no_faces": (cube[0], np.zeros((0, 3), np.int32), 0.0, 0.0, 0.25, 4, 4),
        "g_no_verts": (np.zeros((0, 3), np.float32), cube[1], 0.0, 0.0, 0.25, 4, 4),
        "g_one_column": (*cube, 0.4, 0.0, 0.125, 1, 8),
        "g_one_row": (*cube, 0.0, 0.4, 0.125, 8, 1),
        "g_broken": (*_broken(), 0.0, 0.0, 0.25, 4, 4),
    }
    for n in (21, 22, 23):
        v, f, _, _ = slabs(n, np.random.default_rng(n))
        out[f"f_slabs_{n}"] = (v, f, 0.0, 0.0, 0.125, 8, 8)
    return out
