"""Float64 numpy restatement of the UV-export rules (include/dsu_hip.h: dsu_uv_face_labels,
dsu_uv_components, dsu_uv_bake, dsu_uv_dilate), independent of csrc/mesh_uv.hip: brute-force
labels, union-find charts, a per-face rasteriser that visits the faces in index order, and the
dilation rounds.  RefBackend plugs them into drawingspinup_amd.nsr.uv (whose projection and
packing are host numpy in both paths).  Also the test meshes."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAGILE_REL = 1e-12          # an edge function within this of zero, relative to the face's uv area


# ------------------------------------------------------------------ rules
def face_labels(verts, faces):
    v = np.asarray(verts, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    M = len(faces)
    normal, label, area = np.zeros((M, 3)), np.full(M, -1, np.int64), np.zeros(M)
    for m in range(M):
        ia, ib, ic = faces[m]
        if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= len(v):
            continue
        e1, e2 = v[ib] - v[ia], v[ic] - v[ia]
        n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        mag = np.abs(n)
        if not np.all(np.isfinite(mag)) or not np.any(mag > 0):
            continue
        ax = 0
        if mag[1] > mag[ax]:
            ax = 1
        if mag[2] > mag[ax]:
            ax = 2
        normal[m], label[m], area[m] = n, 2 * ax + (1 if n[ax] < 0 else 0), 0.5 * mag[ax]
    return normal, label, area


def edge_faces(faces):
    """undirected edge -> the (face, edge slot) pairs that use it"""
    table = {}
    for m, f in enumerate(np.asarray(faces, np.int64)):
        for e in range(3):
            a, b = int(f[e]), int(f[(e + 1) % 3])
            table.setdefault((min(a, b), max(a, b)), []).append((m, e))
    return table


def adjacency(faces):
    adj = np.full((len(faces), 3), -1, np.int64)
    for users in edge_faces(faces).values():
        if len(users) == 2:
            (m0, e0), (m1, e1) = users
            adj[m0, e0], adj[m1, e1] = m1, m0
    return adj


def components(faces, label):
    """Union-find over manifold edges between faces of one label >= 0; id = smallest face index."""
    parent = list(range(len(faces)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for users in edge_faces(faces).values():
        if len(users) == 2:
            m0, m1 = users[0][0], users[1][0]
            if label[m0] >= 0 and label[m0] == label[m1]:
                r0, r1 = find(m0), find(m1)
                if r0 != r1:
                    parent[max(r0, r1)] = min(r0, r1)
    return np.asarray([find(m) for m in range(len(faces))], np.int64)


def synchronous_rounds(adj, label):
    """Rounds of the header's propagation when every face reads the previous round's values (the
    device's in-place rounds are never behind this); the last, changeless round counts."""
    M = len(label)
    chart = np.arange(M)
    ok = (adj >= 0) & (label[np.clip(adj, 0, None)] == label[:, None]) & (label[:, None] >= 0)
    rounds = 0
    while True:
        rounds += 1
        nb = np.where(ok, chart[np.clip(adj, 0, None)], M)
        c = np.minimum(chart, nb.min(1))
        c = np.minimum(c, chart[c])
        c = np.minimum(c, chart[c])
        if np.array_equal(c, chart):
            return chart, rounds
        chart = c


def _edges(t, px, py):
    ax, ay, bx, by, cx, cy = t
    w0 = (cx - bx) * (py - by) - (cy - by) * (px - bx)
    w1 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
    w2 = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    return w0, w1, w2


def bake(uvs, indices, colours, size, depth=None):
    """-> image (S,S,3) u8, face_id (S,S) i32, demote (M) u8 or None, fragile (S,S) bool: a sample
    with an edge function of some face within FRAGILE_REL of zero (and not exactly zero)."""
    S = int(size)
    uv = np.asarray(uvs, np.float32).astype(np.float64) * float(S)
    col = np.asarray(colours, np.float32).astype(np.float64)
    indices = np.asarray(indices, np.int64)
    M = len(indices)
    image = np.zeros((S, S, 3), np.uint8)
    face_id = np.full((S, S), -1, np.int32)
    fragile = np.zeros((S, S), bool)
    front = np.full((S, S), -1, np.int64)
    front_depth = np.zeros((S, S))
    demote = None if depth is None else np.zeros(M, np.uint8)
    for m in range(M):                                                  # index order: the lowest face wins
        ia, ib, ic = indices[m]
        if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= len(uv):
            continue
        t = (uv[ia, 0], uv[ia, 1], uv[ib, 0], uv[ib, 1], uv[ic, 0], uv[ic, 1])
        if not np.all(np.isfinite(t)):
            continue
        xs, ys = t[0::2], t[1::2]
        x0, x1 = max(int(np.floor(min(xs))) - 1, 0), min(int(np.ceil(max(xs))) + 1, S - 1)
        y0, y1 = max(int(np.floor(min(ys))) - 1, 0), min(int(np.ceil(max(ys))) + 1, S - 1)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.float64), np.arange(x0, x1 + 1, dtype=np.float64),
                             indexing="ij")
        w0, w1, w2 = _edges(t, px, py)
        area = (w0 + w1) + w2
        rows = S - 1 - np.arange(y0, y1 + 1)
        win = (slice(rows[-1], rows[0] + 1), slice(x0, x1 + 1))         # image rows run against y
        flip = lambda a: a[::-1]
        cover = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (area > 0)
        scale = np.abs(area) * FRAGILE_REL
        near = ((np.abs(w0) <= scale) & (w0 != 0)) | ((np.abs(w1) <= scale) & (w1 != 0)) | \
               ((np.abs(w2) <= scale) & (w2 != 0))
        fragile[win] |= flip(near)
        take = flip(cover) & (face_id[win] < 0)
        if take.any():
            with np.errstate(all="ignore"):
                b0, b1, b2 = w0 / area, w1 / area, w2 / area
                val = (b0[..., None] * col[ia] + b1[..., None] * col[ib]) + b2[..., None] * col[ic]
                val = val * 255.0
                q = np.where(np.isnan(val), 0.0, np.clip(val, 0.0, 255.0)).astype(np.uint8)
            sub_i, sub_f = image[win], face_id[win]
            sub_i[take] = flip(q)[take]
            sub_f[take] = m
        if demote is not None:
            strict = flip((w0 > 0) & (w1 > 0) & (w2 > 0) & (area > 0))
            if strict.any():
                fr, fd = front[win], front_depth[win]
                d = depth[m]
                empty = strict & (fr < 0)
                better = strict & (fr >= 0) & ((d > fd) | ((d == fd) & (m < fr)))
                worse = strict & (fr >= 0) & ~better
                demote[fr[better]] = 1
                if worse.any():
                    demote[m] = 1
                fr[empty | better] = m
                fd[empty | better] = d
    return image, face_id, demote, fragile


def dilate(image, covered, rounds):
    S = image.shape[0]
    img, cov = image.copy(), np.asarray(covered, bool).copy()
    for _ in range(int(rounds)):
        pi = np.zeros((S + 2, S + 2, 3), np.int64)
        pc = np.zeros((S + 2, S + 2), np.int64)
        pi[1:-1, 1:-1], pc[1:-1, 1:-1] = img * cov[..., None], cov
        total, n = np.zeros((S, S, 3), np.int64), np.zeros((S, S), np.int64)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if dr or dc:
                    total += pi[1 + dr:S + 1 + dr, 1 + dc:S + 1 + dc]
                    n += pc[1 + dr:S + 1 + dr, 1 + dc:S + 1 + dc]
        grow = ~cov & (n > 0)
        mean = (2 * total + n[..., None]) // np.maximum(2 * n[..., None], 1)
        img = np.where(cov[..., None], img, np.where(grow[..., None], mean, 0)).astype(np.uint8)
        cov = cov | grow
    return img, cov


class RefBackend:
    """The backend interface of drawingspinup_amd.nsr.uv over the functions above."""

    def labels(self, verts, faces):
        return face_labels(verts, faces)

    def components(self, faces, comp_label):
        return components(faces, comp_label), 0

    def bake(self, uvs, indices, colours, size, depth=None):
        return bake(uvs, indices, colours, size, depth)[:3]

    def dilate(self, image, covered, rounds):
        return dilate(image, covered, rounds)[0]

    @staticmethod
    def to_numpy(a):
        return a


def conflicts(uvs, indices, size):
    """Number of sample points strictly inside two faces — counted without any depth or chart."""
    S = int(size)
    uv = np.asarray(uvs, np.float32).astype(np.float64) * float(S)
    hits = np.zeros((S, S), np.int64)
    for ia, ib, ic in np.asarray(indices, np.int64):
        t = (uv[ia, 0], uv[ia, 1], uv[ib, 0], uv[ib, 1], uv[ic, 0], uv[ic, 1])
        xs, ys = t[0::2], t[1::2]
        x0, x1 = max(int(np.floor(min(xs))) - 1, 0), min(int(np.ceil(max(xs))) + 1, S - 1)
        y0, y1 = max(int(np.floor(min(ys))) - 1, 0), min(int(np.ceil(max(ys))) + 1, S - 1)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.float64), np.arange(x0, x1 + 1, dtype=np.float64),
                             indexing="ij")
        w0, w1, w2 = _edges(t, px, py)
        hits[y0:y1 + 1, x0:x1 + 1] += (w0 > 0) & (w1 > 0) & (w2 > 0)
    return int((hits > 1).sum())


# ------------------------------------------------------------------ meshes
def _grid_faces(ni, nj, idx):
    f = []
    for i in range(ni):
        for j in range(nj):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return np.asarray(f, np.int64)


def helicoid(nr=8, nt=48, r0=0.2, r1=0.5, pitch=0.05, turns=1.5):
    """x = r cos t, y = r sin t, z = pitch t: the normal (pitch sin t, -pitch cos t, r) keeps z as its
    dominant axis (r >= 0.2 > pitch), so the strip is ONE chart that covers itself over half a turn."""
    r, t = np.meshgrid(np.linspace(r0, r1, nr + 1), np.linspace(0.0, 2 * np.pi * turns, nt + 1), indexing="ij")
    v = np.stack([r * np.cos(t), r * np.sin(t), pitch * t], -1).reshape(-1, 3)
    return v.astype(np.float32), _grid_faces(nr, nt, lambda i, j: i * (nt + 1) + j)


def ribbon(n=2000, step=1.0 / 1024):
    """1 x n quads in the xy plane, faces numbered along its length: one chart of 2 n faces."""
    v = np.asarray([[i * step, j * step, 0.0] for i in range(n + 1) for j in range(2)], np.float32)
    return v, _grid_faces(n, 1, lambda i, j: i * 2 + j)


def lattice_cube(n=4):
    """The unit cube's six sides, n x n quads each, vertices on the lattice k / n (n a power of two):
    with a power-of-two scale every uv, edge function and depth is exact, and vertices and edges
    fall exactly on sample points."""
    verts, index, faces = [], {}, []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append([c / n for c in p])
        return index[p]
    for ax in range(3):
        u, w = (ax + 1) % 3, (ax + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def corner(di, dj):
                        p = [0, 0, 0]
                        p[ax], p[u], p[w] = side, i + di, j + dj
                        return vid(tuple(p))
                    q = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]
                    if side == 0:
                        q = q[::-1]                                        # outward normals
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.asarray(verts, np.float32), np.asarray(faces, np.int64)


def body_and_arm():
    z = np.load(os.path.join(GOLDEN, "mesh_color_reference.npz"))
    return z["verts"].astype(np.float32), z["faces"].astype(np.int64)


def meshes():
    import skin_ref
    out = {k: (v[0], np.asarray(v[1], np.int64)) for k, v in skin_ref.general_cases().items()}
    out["body_and_arm"] = body_and_arm()
    out["helicoid"] = helicoid()
    out["ribbon"] = ribbon()
    out["lattice"] = lattice_cube()
    return out


def vertex_colours(verts):
    """Smooth colours in [0,1] from the positions."""
    v = np.asarray(verts, np.float64)
    lo, ext = v.min(0), np.maximum(v.max(0) - v.min(0), 1e-9)
    return ((v - lo) / ext).astype(np.float32)


LATTICE_SCALE = 16.0


@functools.lru_cache(maxsize=None)
def reference(name, size, gutter=2):
    """parametrize + bake through RefBackend, computed once per (mesh, size, gutter)."""
    from drawingspinup_amd.nsr import uv as U
    verts, faces = meshes()[name]
    scale = LATTICE_SCALE if name == "lattice" else None
    vm, ind, uvs, info = U.parametrize(verts, faces, size, gutter, return_info=True, backend=RefBackend(), scale=scale)
    col = vertex_colours(verts)[vm]
    image, face_id, demote, fragile = bake(uvs, ind, col, size, U.face_depths(verts, faces, info["label"]))
    filled, _ = dilate(image, face_id >= 0, gutter)
    for a in (vm, ind, uvs, image, face_id, demote, fragile, filled):
        a.setflags(write=False)
    return {"verts": verts, "faces": faces, "vmapping": vm, "indices": ind, "uvs": uvs, "info": info,
            "colours": col, "image": image, "face_id": face_id, "demote": demote, "fragile": fragile,
            "filled": filled}
