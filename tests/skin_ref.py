"""Float64 restatement of the rigging rules (include/dsu_hip.h: dsu_bone_visibility, the bone-heat
system, dsu_skin_lbs) in numpy / scipy, with brute force over all triangles and a direct sparse
solve, plus the small meshes, skeletons and BVH text the tests use.  Test infrastructure only: it
shares no code with the product.
"""
import numpy as np

EPS_FRAGILE = 1e-9
NEAR = 1e-4
D_FLOOR = 1e-6


# ------------------------------------------------------------------ distance and visibility
def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _triple(x, y, z):
    return (x[..., 0] * (y[..., 1] * z[..., 2] - y[..., 2] * z[..., 1])
            + x[..., 1] * (y[..., 2] * z[..., 0] - y[..., 0] * z[..., 2])) \
        + x[..., 2] * (y[..., 0] * z[..., 1] - y[..., 1] * z[..., 0])


def _norm(a):
    return np.sqrt(_dot3(a, a))


def closest_points(verts, bones):
    """verts (V,3) f32, bones (B,2,3) f32 -> q (V,B,3), d (V,B), float64 in the header's order."""
    p = np.asarray(verts, np.float32).astype(np.float64)[:, None, :]
    bn = np.asarray(bones, np.float32).astype(np.float64)
    a, b = bn[None, :, 0, :], bn[None, :, 1, :]
    ab = b - a
    ap = p - a
    den = np.broadcast_to(_dot3(ab, ab), ap.shape[:2])
    num = _dot3(ap, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den > 0.0, num / den, 0.0)
    t = np.minimum(np.maximum(t, 0.0), 1.0)
    q = a + t[..., None] * ab
    e = q - p
    return q, np.sqrt(_dot3(e, e))


def visibility(verts, faces, bones, chunk=256):
    """Brute force over all triangles.  -> dist (V,B) f64, visible (V,B) bool, fragile (V,B) bool:
    a pair is fragile when no triangle blocks it with every deciding volume further than 1e-9
    (relative to the product of the three vectors' lengths) from zero, yet some triangle would
    block it with the volumes moved by that much."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    q, dist = closest_points(verts, bones)
    V, B = dist.shape
    vis = np.ones((V, B), bool)
    frag = np.zeros((V, B), bool)
    U, Vv, W = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]          # (1,M,3)
    for j in range(B):
        for i0 in range(0, V, chunk):
            i1 = min(i0 + chunk, V)
            p = v[i0:i1, None, :]
            qq = q[i0:i1, j, None, :]
            e = qq - p
            idx = np.arange(i0, i1)[:, None]
            free = (f[None, :, 0] != idx) & (f[None, :, 1] != idx) & (f[None, :, 2] != idx)
            A, Bv, C = U - p, Vv - p, W - p
            A2, B2, C2 = U - qq, Vv - qq, W - qq
            s1, s2 = _triple(A, Bv, C), _triple(A2, B2, C2)
            m1 = EPS_FRAGILE * _norm(A) * _norm(Bv) * _norm(C)
            m2 = EPS_FRAGILE * _norm(A2) * _norm(B2) * _norm(C2)
            exact = free & (((s1 > 0) & (s2 < 0)) | ((s1 < 0) & (s2 > 0)))
            maybe = free & (((s1 > -m1) & (s2 < m2)) | ((s1 < m1) & (s2 > -m2)))
            sure = free & (((s1 > m1) & (s2 < -m2)) | ((s1 < -m1) & (s2 > m2)))
            r, c = np.nonzero(maybe)
            if not len(r):
                continue
            ee = np.broadcast_to(e, A.shape)[r, c]
            a_, b_, c_ = A[r, c], Bv[r, c], C[r, c]
            t1, t2, t3 = _triple(ee, a_, b_), _triple(ee, b_, c_), _triple(ee, c_, a_)
            ne, na, nb, nc = _norm(ee), _norm(a_), _norm(b_), _norm(c_)
            g1, g2, g3 = EPS_FRAGILE * ne * na * nb, EPS_FRAGILE * ne * nb * nc, EPS_FRAGILE * ne * nc * na
            inside = ((t1 >= 0) & (t2 >= 0) & (t3 >= 0)) | ((t1 <= 0) & (t2 <= 0) & (t3 <= 0))
            inside_maybe = ((t1 >= -g1) & (t2 >= -g2) & (t3 >= -g3)) | ((t1 <= g1) & (t2 <= g2) & (t3 <= g3))
            inside_sure = ((t1 >= g1) & (t2 >= g2) & (t3 >= g3)) | ((t1 <= -g1) & (t2 <= -g2) & (t3 <= -g3))
            n = i1 - i0
            blocked = np.zeros(n, bool)
            blocked_sure = np.zeros(n, bool)
            blocked_maybe = np.zeros(n, bool)
            np.logical_or.at(blocked, r, exact[r, c] & inside)
            np.logical_or.at(blocked_sure, r, sure[r, c] & inside_sure)
            np.logical_or.at(blocked_maybe, r, inside_maybe)
            vis[i0:i1, j] = ~blocked
            frag[i0:i1, j] = blocked_maybe & ~blocked_sure
    finite = np.isfinite(dist)
    return dist, vis & finite, frag


# ------------------------------------------------------------------ the system
def components(n, f):
    label = np.arange(n)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    while True:
        lo = np.minimum(label[e[:, 0]], label[e[:, 1]])
        new = label.copy()
        np.minimum.at(new, e[:, 0], lo)
        np.minimum.at(new, e[:, 1], lo)
        new = new[new]
        if np.array_equal(new, label):
            return np.unique(label, return_inverse=True)[1]
        label = new


def heat_sources(dist, vis, labels, floor):
    """-> near (V,B) bool, n (V,), P (V,B), h (V,), the labels of the components that saw no bone."""
    vis = vis.copy()
    blind = [c for c in range(labels.max() + 1) if not vis[labels == c].any()]
    for c in blind:
        vis[labels == c] = True
    dmin = np.where(vis, dist, np.inf).min(1)
    near = vis & (dist <= (1.0 + NEAR) * dmin[:, None])
    n = near.sum(1)
    P = near / np.maximum(n, 1)[:, None]
    h = np.where(np.isfinite(dmin), 1.0 / np.maximum(dmin, floor) ** 2, 0.0)
    return near, n, P, h, blind


def stiffness_and_mass(v, f):
    """Cotangent stiffness (positive semi-definite, scipy csr) and the lumped barycentric mass."""
    import scipy.sparse as sp
    n = len(v)
    L = sp.csr_matrix((n, n))
    for k in range(3):
        i, j, o = f[:, (k + 1) % 3], f[:, (k + 2) % 3], f[:, k]
        a, b = v[i] - v[o], v[j] - v[o]
        cot = 0.5 * (a * b).sum(1) / np.linalg.norm(np.cross(a, b), axis=1)
        L = L + sp.coo_matrix((np.concatenate([-cot, -cot, cot, cot]),
                               (np.concatenate([i, j, i, j]), np.concatenate([j, i, i, j]))), shape=(n, n)).tocsr()
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    m = np.zeros(n)
    np.add.at(m, f.ravel(), np.repeat(area / 3.0, 3))
    return L, m


def heat_system(verts, faces, P, h):
    import scipy.sparse as sp
    v = np.asarray(verts, np.float32).astype(np.float64)
    L, m = stiffness_and_mass(v, np.asarray(faces, np.int64))
    A = (L + sp.diags(m * h)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A, (m * h)[:, None] * P


def solve_direct(A, rhs):
    from scipy.sparse.linalg import splu
    return splu(A.tocsc()).solve(rhs)


def bone_heat(verts, faces, bones, dist=None, vis=None):
    """The whole reference weighting: (V,B) float64 weights and the pieces."""
    f = np.asarray(faces, np.int64)
    if dist is None:
        dist, vis, _ = visibility(verts, f, bones)
    v = np.asarray(verts, np.float32).astype(np.float64)
    floor = D_FLOOR * float(np.linalg.norm(v.max(0) - v.min(0)))
    near, n, P, h, blind = heat_sources(dist, vis, components(len(v), f), floor)
    A, rhs = heat_system(verts, f, P, h)
    return solve_direct(A, rhs), {"A": A, "rhs": rhs, "P": P, "h": h, "n": n, "near": near, "blind": blind}


# ------------------------------------------------------------------ skinning
def skin_lbs(rest, influences, weights, matrices):
    """float64 from the f32 inputs: (F,V,3) and max over k of |R x| + |t| per (F,V,3) entry."""
    x = np.asarray(rest, np.float32).astype(np.float64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    m = np.asarray(matrices, np.float32).astype(np.float64)
    infl = np.asarray(influences, np.int64)
    F = m.shape[0]
    out = np.zeros((F,) + x.shape)
    mag = np.zeros((F,) + x.shape)
    for k in range(infl.shape[1]):
        mk = m[:, infl[:, k]]                                               # (F,V,3,4)
        out += w[None, :, k, None] * (np.einsum("fvab,vb->fva", mk[..., :3], x) + mk[..., 3])
        mag = np.maximum(mag, np.einsum("fvab,vb->fva", np.abs(mk[..., :3]), np.abs(x)) + np.abs(mk[..., 3]))
    return out, mag


# ------------------------------------------------------------------ meshes
def capsule(p0, p1, radius, n_around=12, n_along=6, n_cap=3):
    """Closed capsule around the segment p0 -> p1: rings of n_around vertices and two poles."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    axis = p1 - p0
    length = np.linalg.norm(axis)
    w = axis / length
    u = np.cross(w, [0.0, 0.0, 1.0] if abs(w[2]) < 0.9 else [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    t = np.cross(w, u)
    rings = [(-radius * np.cos(a), radius * np.sin(a)) for a in np.arange(1, n_cap + 1) * (np.pi / 2) / (n_cap + 0.5)]
    rings += [(s * length, radius) for s in np.arange(1, n_along) / n_along]
    rings += [(length + radius * np.cos(a), radius * np.sin(a))
              for a in np.arange(n_cap, 0, -1) * (np.pi / 2) / (n_cap + 0.5)]
    v = [p0 - radius * w]
    for z, r in rings:
        for k in range(n_around):
            a = 2 * np.pi * k / n_around
            v.append(p0 + z * w + r * (np.cos(a) * u + np.sin(a) * t))
    v.append(p1 + radius * w)
    nr, last = len(rings), len(v) - 1
    f = []
    ring = lambda i, k: 1 + i * n_around + k % n_around
    for k in range(n_around):
        f.append([0, ring(0, k + 1), ring(0, k)])
        f.append([last, ring(nr - 1, k), ring(nr - 1, k + 1)])
        for i in range(nr - 1):
            f += [[ring(i, k), ring(i, k + 1), ring(i + 1, k + 1)], [ring(i, k), ring(i + 1, k + 1), ring(i + 1, k)]]
    return np.asarray(v), np.asarray(f, np.int64)


def merge(*meshes):
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(v); fs.append(f + n); n += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def vertex_colours(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def jitter(v, amp, seed):
    return v + np.random.default_rng(seed).uniform(-amp, amp, v.shape)


HUMANOID = [  # name, parent, rest position
    ("hips", -1, (0.0, -0.05, 0.0)), ("spine", 0, (0.0, 0.12, 0.0)), ("chest", 1, (0.0, 0.28, 0.0)),
    ("neck", 2, (0.0, 0.38, 0.0)), ("head", 3, (0.0, 0.44, 0.0)),
    ("l_shoulder", 2, (0.13, 0.28, 0.0)), ("l_elbow", 5, (0.29, 0.28, 0.0)), ("l_wrist", 6, (0.42, 0.28, 0.0)),
    ("l_hand", 7, (0.46, 0.28, 0.0)),
    ("r_shoulder", 2, (-0.13, 0.28, 0.0)), ("r_elbow", 9, (-0.29, 0.28, 0.0)), ("r_wrist", 10, (-0.42, 0.28, 0.0)),
    ("r_hand", 11, (-0.46, 0.28, 0.0)),
    ("l_hip", 0, (0.06, -0.12, 0.0)), ("l_knee", 13, (0.06, -0.33, 0.0)), ("l_ankle", 14, (0.06, -0.53, 0.0)),
    ("r_hip", 0, (-0.06, -0.12, 0.0)), ("r_knee", 16, (-0.06, -0.33, 0.0)), ("r_ankle", 17, (-0.06, -0.53, 0.0)),
]
HUMANOID_ENDS = {4: (0.0, 0.06, 0.0), 8: (0.02, 0.0, 0.0), 12: (-0.02, 0.0, 0.0), 15: (0.0, -0.03, 0.0),
                 18: (0.0, -0.03, 0.0)}


def humanoid():
    """-> names, parents, offsets (J,3), end sites {joint: offset}: 19 joints, 23 bones."""
    names = [n for n, _, _ in HUMANOID]
    parents = np.asarray([p for _, p, _ in HUMANOID])
    pos = np.asarray([q for _, _, q in HUMANOID], np.float64)
    off = pos - np.where(parents[:, None] >= 0, pos[np.maximum(parents, 0)], 0.0)
    return names, parents, off, {j: np.asarray(o, np.float64) for j, o in HUMANOID_ENDS.items()}


def bones_of(parents, offsets, ends):
    """(heads, segments (B,2,3)): by head joint, its children in joint order, then its end site."""
    J = len(parents)
    pos = np.zeros((J, 3))
    for j in range(J):
        pos[j] = offsets[j] + (pos[parents[j]] if parents[j] >= 0 else 0.0)
    heads, segs = [], []
    for j in range(J):
        for c in range(j + 1, J):
            if parents[c] == j:
                heads.append(j); segs.append([pos[j], pos[c]])
        if j in ends:
            heads.append(j); segs.append([pos[j], pos[j] + ends[j]])
    return np.asarray(heads), np.asarray(segs)


def capsule_character(detail=1, seed=3):
    """Torso, head, two arms and two legs as closed capsules around the humanoid's bones (separate,
    overlapping components), every vertex moved a little so that nothing is aligned."""
    na, nl = 10 * detail, 5 * detail
    parts = [capsule((0, -0.05, 0), (0, 0.30, 0), 0.11, na + 4, nl + 1), capsule((0, 0.42, 0), (0, 0.47, 0), 0.07, na, 2),
             capsule((0.13, 0.28, 0), (0.46, 0.28, 0), 0.04, na, 2 * nl), capsule((-0.13, 0.28, 0), (-0.46, 0.28, 0), 0.04, na, 2 * nl),
             capsule((0.06, -0.12, 0), (0.06, -0.55, 0), 0.05, na, 2 * nl), capsule((-0.06, -0.12, 0), (-0.06, -0.55, 0), 0.05, na, 2 * nl)]
    v, f = merge(*parts)
    return jitter(v, 2e-3, seed).astype(np.float32), f


def torus_mesh(nu=40, nv=16, R=0.4, r=0.13, seed=4):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), r * np.sin(w), (R + r * np.cos(w)) * np.sin(u)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(nu) for j in range(nv)]
    f += [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(nu) for j in range(nv)]
    return jitter(v, 2e-3, seed).astype(np.float32), np.asarray(f, np.int64)


def torus_bones(R=0.4):
    """A chain inside the tube over three quarters of the ring, and one bone across the hole."""
    a = np.arange(7) * (1.5 * np.pi / 6) + 0.11
    pts = np.stack([R * np.cos(a), 0.013 * np.sin(3 * a), R * np.sin(a)], -1)
    segs = [[pts[k], pts[k + 1]] for k in range(6)] + [[[-0.12, 0.021, 0.05], [0.11, -0.017, -0.04]]]
    return np.asarray(segs, np.float32)


def sheet_mesh(n=24, seed=5):
    """An open, wavy sheet standing in the xy plane."""
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, n), np.linspace(-0.4, 0.4, n), indexing="ij")
    z = 0.08 * np.sin(5.1 * x + 0.3) * np.cos(4.3 * y - 0.2)
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    idx = lambda i, j: i * n + j
    f = [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(n - 1) for j in range(n - 1)]
    f += [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(n - 1) for j in range(n - 1)]
    return jitter(v, 2e-3, seed).astype(np.float32), np.asarray(f, np.int64)


def sheet_bones():
    """Three bones in front of the sheet and one behind it."""
    return np.asarray([[[-0.41, -0.29, 0.21], [-0.07, -0.23, 0.17]], [[-0.07, -0.23, 0.17], [0.33, 0.05, 0.24]],
                       [[0.33, 0.05, 0.24], [0.37, 0.31, 0.19]], [[-0.22, 0.12, -0.23], [0.19, 0.27, -0.18]]], np.float32)


def character_case():
    v, f = capsule_character()
    _, parents, off, ends = humanoid()
    heads, segs = bones_of(parents, off, ends)
    return v, f, segs.astype(np.float32)


def general_cases():
    """name -> (verts f32, faces, bones f32): the three meshes in general position."""
    return {"character": character_case(), "torus": torus_mesh() + (torus_bones(),),
            "sheet": sheet_mesh() + (sheet_bones(),)}


def lattice_case():
    """Axis-aligned boxes on a dyadic lattice and bones on lattice lines: every coordinate, product
    and volume is exact in float64, so the decisions have no rounding at all — touching (zero
    volumes) included."""
    def box(lo, hi):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        v = np.asarray([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1],
                        [x1, y1, z1], [x0, y1, z1]], np.float64)
        f = np.asarray([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5],
                        [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7]], np.int64)
        return v, f
    v, f = merge(box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), box((0.75, -0.25, -0.25), (1.25, 0.25, 0.25)),
                 box((-0.25, 0.75, -0.25), (0.25, 1.5, 0.25)))
    bones = np.asarray([[[-0.25, 0.0, 0.0], [0.25, 0.0, 0.0]], [[1.0, -0.125, 0.0], [1.0, 0.125, 0.0]],
                        [[0.0, 1.0, 0.0], [0.0, 1.25, 0.0]], [[0.5, 0.5, 0.5], [0.75, 0.25, 0.25]],
                        [[2.0, 0.0, 0.0], [2.0, 0.0, 0.0]]], np.float32)
    return v.astype(np.float32), f, bones


def cylinder_two_bones(n_around=16, n_half=6, radius=0.1, half=0.5):
    """A straight closed cylinder along x, symmetric about x = 0, with a ring on the joint plane;
    two collinear bones (-half, 0) and (0, half) on its axis."""
    xs = np.concatenate([-np.linspace(half, 0, n_half + 1)[:-1], np.linspace(0, half, n_half + 1)])
    v = [[-half, 0, 0]]
    for x in xs:
        for k in range(n_around):
            a = 2 * np.pi * (k + 0.5) / n_around
            v.append([x, radius * np.cos(a), radius * np.sin(a)])
    v.append([half, 0, 0])
    nr, last = len(xs), len(v) - 1
    ring = lambda i, k: 1 + i * n_around + k % n_around
    f = []
    for k in range(n_around):
        f.append([0, ring(0, k + 1), ring(0, k)])
        f.append([last, ring(nr - 1, k), ring(nr - 1, k + 1)])
        for i in range(nr - 1):
            # the diagonals mirror about the joint plane
            if i < n_half:
                f += [[ring(i, k), ring(i, k + 1), ring(i + 1, k + 1)], [ring(i, k), ring(i + 1, k + 1), ring(i + 1, k)]]
            else:
                f += [[ring(i, k), ring(i, k + 1), ring(i + 1, k)], [ring(i, k + 1), ring(i + 1, k + 1), ring(i + 1, k)]]
    bones = np.asarray([[[-half, 0, 0], [0, 0, 0]], [[0, 0, 0], [half, 0, 0]]], np.float32)
    return np.asarray(v, np.float32), np.asarray(f, np.int64), bones, n_half, n_around


# ------------------------------------------------------------------ BVH text
def bvh_text(names, parents, offsets, ends, channels, motion, frame_time=1.0 / 30.0):
    """channels: per joint a list such as ['Xposition', ..., 'Zrotation', 'Xrotation', 'Yrotation'];
    motion (F, total channels)."""
    J = len(names)
    kids = [[c for c in range(J) if parents[c] == j] for j in range(J)]
    out = ["HIERARCHY"]

    def emit(j, depth):
        pad = "  " * depth
        out.append(f"{pad}{'ROOT' if parents[j] < 0 else 'JOINT'} {names[j]}")
        out.append(pad + "{")
        out.append(f"{pad}  OFFSET " + " ".join(repr(float(x)) for x in offsets[j]))
        out.append(f"{pad}  CHANNELS {len(channels[j])} " + " ".join(channels[j]))
        for c in kids[j]:
            emit(c, depth + 1)
        if j in ends:
            out.append(f"{pad}  End Site")
            out.append(pad + "  {")
            out.append(f"{pad}    OFFSET " + " ".join(repr(float(x)) for x in ends[j]))
            out.append(pad + "  }")
        out.append(pad + "}")

    emit(0, 0)
    out += ["MOTION", f"Frames: {len(motion)}", f"Frame Time: {frame_time!r}"]
    out += [" ".join(repr(float(x)) for x in row) for row in motion]
    return "\n".join(out) + "\n"


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"X": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "Y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "Z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]
