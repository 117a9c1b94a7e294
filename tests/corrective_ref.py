"""Float64 numpy restatement of the corrective smoothing (delta mush), written from the rule in
include/dsu_hip.h ("Corrective smoothing"), not from csrc/corrective_smooth.h: the same operations
in the same operand order, one elementwise numpy operation per product and sum, so nothing is fused.
The loops run over the position in a row (all vertices and frames side by side), which keeps the
row order of every sum.  `rounded=False` keeps float64 buffers between the smoothing steps and does
not round the result: the "unrounded" truth the bounds are stated against.  The test meshes and the
wrappers of the host entries live here too, so the host and device tests use the same cases."""
import ctypes

import numpy as np

EPS32 = 2.0 ** -24
KEYS = ("rep", "faces", "nbr_rowptr", "nbr_cols", "cor_rowptr", "cor_faces")


# ------------------------------------------------------------------ the rule
def _rows(rowptr, cols):
    """CSR -> (table (V, longest row) of entries, 0 where a row has ended; lengths (V,))."""
    rowptr = np.asarray(rowptr, np.int64)
    n = np.diff(rowptr)
    width = int(n.max()) if len(n) else 0
    table = np.zeros((len(n), max(width, 1)), np.int64)
    for k in range(width):
        has = n > k
        table[has, k] = np.asarray(cols, np.int64)[rowptr[:-1][has] + k]
    return table, n


def smooth(q, topo, lam, iterations, rounded=True):
    """`iterations` smoothing steps on q (F,V,3) -> float64 (F,V,3), holding f32 values when rounded."""
    q = np.asarray(q, np.float32).astype(np.float64)
    nbr, deg = _rows(topo["nbr_rowptr"], topo["nbr_cols"])
    lam = float(lam)
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            total = np.zeros_like(q)
            for k in range(int(deg.max()) if len(deg) else 0):
                total = np.where((deg > k)[None, :, None], total + q[:, nbr[:, k]], total)
            m = total / np.maximum(deg, 1)[None, :, None].astype(np.float64)
            new = q + lam * (m - q)
            if rounded:
                new = new.astype(np.float32).astype(np.float64)
            q = np.where((deg > 0)[None, :, None], new, q)
    return q


def frames(s, topo):
    """The local frames of every vertex from the smoothed buffer s (F,V,3) float64 ->
    t, b, n (F,V,3) and ok (F,V): whether a frame exists."""
    nbr, deg = _rows(topo["nbr_rowptr"], topo["nbr_cols"])
    cor, ncor = _rows(topo["cor_rowptr"], topo["cor_faces"])
    G = np.asarray(topo["faces"], np.int64).reshape(-1, 3)
    F, V = s.shape[:2]
    N = np.zeros((F, V, 3))
    with np.errstate(all="ignore"):
        for k in range(int(ncor.max()) if len(ncor) and len(G) else 0):
            g = G[cor[:, k]]                                                   # (V,3)
            a, b, c = s[:, g[:, 0]], s[:, g[:, 1]], s[:, g[:, 2]]
            u, w = b - a, c - a
            cross = np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1],
                              u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                              u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)
            N = np.where((ncor > k)[None, :, None], N + cross, N)
        n2 = (N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2]
        ok = (n2 > 0.0) & np.isfinite(n2) & (deg > 0)[None] & (ncor > 0)[None]
        n = N / np.sqrt(np.where(ok, n2, 1.0))[..., None]
        e = s[:, nbr[:, 0]] - s
        en = (e[..., 0] * n[..., 0] + e[..., 1] * n[..., 1]) + e[..., 2] * n[..., 2]
        t = e - en[..., None] * n
        t2 = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
        ok = ok & (t2 > 0.0) & np.isfinite(t2)
        t = t / np.sqrt(np.where(ok, t2, 1.0))[..., None]
        b = np.stack([n[..., 1] * t[..., 2] - n[..., 2] * t[..., 1],
                      n[..., 2] * t[..., 0] - n[..., 0] * t[..., 2],
                      n[..., 0] * t[..., 1] - n[..., 1] * t[..., 0]], -1)
    return t, b, n, ok


def bind(rest, topo, lam, iterations, rounded=True):
    """-> delta (V,3) float64, valid (V,) uint8."""
    x = np.asarray(rest, np.float32).astype(np.float64)[None]
    s = smooth(x, topo, lam, iterations, rounded)
    t, b, n, ok = frames(s, topo)
    with np.errstate(all="ignore"):
        d = x - s
        dot = lambda a: (a[..., 0] * d[..., 0] + a[..., 1] * d[..., 1]) + a[..., 2] * d[..., 2]
        delta = np.stack([dot(t), dot(b), dot(n)], -1)[0]
    return np.where(ok[0][:, None], delta, 0.0), ok[0].astype(np.uint8)


def apply(skinned, topo, delta, valid, lam, iterations, rounded=True):
    """-> (F,V,3): float32 when rounded, else the unrounded float64 value."""
    x = np.asarray(skinned, np.float32)
    s = smooth(x, topo, lam, iterations, rounded)
    t, b, n, ok = frames(s, topo)
    rep = np.asarray(topo["rep"], np.int64)
    with np.errstate(all="ignore"):
        d = np.asarray(delta, np.float64)[None]
        moved = s + ((t * d[..., 0:1] + b * d[..., 1:2]) + n * d[..., 2:3])
        use = (ok & (np.asarray(valid) != 0)[None])[:, rep]
        if rounded:
            return np.where(use[..., None], moved.astype(np.float32)[:, rep], x)
        return np.where(use[..., None], moved[:, rep], x.astype(np.float64))


def corrective(skinned, rest, topo, lam, iterations, rounded=True):
    """Bind on the rest mesh, then apply to the skinned frames -> (out, delta, valid)."""
    delta, valid = bind(rest, topo, lam, iterations, rounded)
    return apply(skinned, topo, delta, valid, lam, iterations, rounded), delta, valid


def bound(ref64, iterations, scale, C):
    """The rounding of the result, plus one f32 rounding of a value of size `scale` per smoothing
    step, the input's and the result's: C (iterations + 2) 2^-24 scale."""
    return EPS32 * np.abs(ref64) + C * (iterations + 2) * EPS32 * scale


# ------------------------------------------------------------------ the host entries
def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _topo_args(topo):
    t = {k: np.ascontiguousarray(topo[k], np.int32) for k in KEYS}
    return t, (_p(t["nbr_rowptr"]), _p(t["nbr_cols"]), t["nbr_cols"].size, _p(t["cor_rowptr"]), _p(t["cor_faces"]),
               t["cor_faces"].size, _p(t["faces"]), len(t["faces"]))


def host_bind(rest, topo, lam, iterations):
    """dsu_corrective_bind_host: the text the kernels compile (csrc/corrective_smooth.h) on host arrays."""
    from drawingspinup_amd import _lib
    rest = np.ascontiguousarray(rest, np.float32)
    V = len(rest)
    t, args = _topo_args(topo)
    ws = np.full(2 * V * 3, -7.0, np.float32)
    delta, valid = np.full((V, 3), -7.0), np.full(V, 9, np.uint8)
    rc = _lib.lib().dsu_corrective_bind_host(_p(rest), *args, V, float(lam), int(iterations), _p(ws), ws.nbytes,
                                             _p(delta), _p(valid))
    assert rc == 0, rc
    return delta, valid


def host_smooth(skinned, topo, delta, valid, lam, iterations):
    """dsu_corrective_smooth_host on host arrays; the input is checked to be left as it was."""
    from drawingspinup_amd import _lib
    x = np.ascontiguousarray(skinned, np.float32)
    keep = x.copy()
    F, V = x.shape[:2]
    t, args = _topo_args(topo)
    delta, valid = np.ascontiguousarray(delta, np.float64), np.ascontiguousarray(valid, np.uint8)
    ws = np.full(2 * F * V * 3, -7.0, np.float32)
    out = np.full((F, V, 3), -7.0, np.float32)
    rc = _lib.lib().dsu_corrective_smooth_host(_p(x), _p(t["rep"]), *args, _p(delta), _p(valid), V, F, float(lam),
                                               int(iterations), _p(ws), ws.nbytes, _p(out))
    assert rc == 0, rc
    assert same_bits(x, keep)
    return out


def host_corrective(skinned, rest, topo, lam, iterations):
    delta, valid = host_bind(rest, topo, lam, iterations)
    return host_smooth(skinned, topo, delta, valid, lam, iterations), delta, valid


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    return np.array_equal(a.view(u), b.view(u))


# ------------------------------------------------------------------ meshes
RINGS, SEGS = 21, 16


def tube(rings=RINGS, segs=SEGS):
    """Open tube along z in [-1, 1], radius 0.1 (1 + 0.15 sin(21 z + 3 phi)): rings * segs vertices
    (336: one full block of 256 and a partial one), vertex ring * segs + segment, wound outward."""
    z = np.linspace(-1.0, 1.0, rings)[:, None]
    phi = (2 * np.pi * np.arange(segs) / segs)[None, :]
    r = 0.1 * (1 + 0.15 * np.sin(21 * z + 3 * phi))
    v = np.stack([r * np.cos(phi), r * np.sin(phi), np.broadcast_to(z, r.shape)], -1).reshape(-1, 3)
    at = lambda i, k: i * segs + k % segs
    f = []
    for i in range(rings - 1):
        for k in range(segs):
            f += [[at(i, k), at(i, k + 1), at(i + 1, k + 1)], [at(i, k), at(i + 1, k + 1), at(i + 1, k)]]
    return v.astype(np.float32), np.asarray(f, np.int64)


def split_tube():
    """The tube cut along the column of segment 0 (every vertex of that column once more, used by the
    faces on the far side of the cut: a uv seam) plus one isolated vertex at the end.
    -> verts, faces, origin (V,): the unsplit tube's vertex each vertex came from, -1 for the isolated one."""
    v, f = tube()
    n = len(v)
    dup = n + np.arange(RINGS)                                      # copy of vertex (ring, 0)
    f = f.copy()
    for m in range(len(f)):
        # the faces between segment SEGS - 1 and segment 0 take the copies
        if (f[m] % SEGS == SEGS - 1).any():
            f[m] = [dup[i // SEGS] if i % SEGS == 0 else i for i in f[m]]
    v2 = np.concatenate([v, v[np.arange(RINGS) * SEGS], [[0.3, 0.2, 0.1]]]).astype(np.float32)
    origin = np.concatenate([np.arange(n), np.arange(RINGS) * SEGS, [-1]])
    return v2, f, origin


def icosphere(level=3, radius=0.5):
    """Closed sphere, 10 4^level + 2 vertices (642 at level 3), wound outward."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (radius * np.asarray(v)).astype(np.float32), np.asarray(f, np.int64)


def edges_of(faces):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return np.unique(e, axis=0)


def stretch(p, rest, faces):
    """The largest |length / rest length - 1| over the edges of the mesh."""
    e = edges_of(faces)
    p, rest = np.asarray(p, np.float64), np.asarray(rest, np.float64)
    length = np.linalg.norm(p[e[:, 0]] - p[e[:, 1]], axis=1)
    rest_length = np.linalg.norm(rest[e[:, 0]] - rest[e[:, 1]], axis=1)
    return float(np.abs(length / rest_length - 1.0).max())


def rings_from(faces, start, n_verts):
    """Graph distance (in edges) of every vertex from `start`; -1 where unreachable."""
    e = edges_of(faces)
    dist = np.full(n_verts, -1, np.int64)
    dist[start] = 0
    d = 0
    while True:
        front = dist == d
        nxt = np.zeros(n_verts, bool)
        nxt[e[front[e[:, 0]], 1]] = True
        nxt[e[front[e[:, 1]], 0]] = True
        nxt &= dist < 0
        if not nxt.any():
            return dist
        d += 1
        dist[nxt] = d


def rotation(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"X": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "Y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "Z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def wobble(rest, F, seed, amp=0.05):
    """F skinned-like frames of a mesh: a rigid turn per frame plus a smooth, frame-dependent bend
    (so the frames are neither rigid nor equal) -> (F,V,3) f32."""
    rng = np.random.default_rng(seed)
    x = np.asarray(rest, np.float64)
    out = np.empty((F,) + x.shape)
    for k in range(F):
        a = rng.uniform(-180, 180, 3)
        Rm = rotation("Z", a[0]) @ rotation("X", a[1]) @ rotation("Y", a[2])
        y = x + amp * np.sin(3.0 * x[:, [1, 2, 0]] + rng.uniform(0, 6, 3))
        out[k] = y @ Rm.T + rng.uniform(-0.5, 0.5, 3)
    return out.astype(np.float32)
