"""Float64 / int64 numpy restatement of seam levelling (include/dsu_hip.h, UV export h. and i., and
the host step between them), independent of csrc/uv_seam.h and of nsr/uv.seam_offsets: the
per-group integer sums of the projected texels, the known offsets and their harmonic extension over
the welded mesh's edges (scipy's sparse LU), and the composed bytes.  RefBackend plugs the
restatement into drawingspinup_amd.nsr.uv.bake_drawings / uv_mapping on top of
tests/uv_field_ref.py's backend.  Also the cases, the synthetic `source` maps and the colours the
host and GPU tests share."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_field_ref as F  # noqa: E402
import uv_ref as R  # noqa: E402

ONE = 1 << 20                 # a barycentric of 1 in the gather's fixed point; also the known threshold
FRAGILE = 1e-6                # a levelled byte whose v + 0.5 lies this close to an integer may differ by one
FRAGILE_CAP = 0.005           # of the levelled texels
# The seam step (seam_step below) of seam_case("icosphere", 64, "z", "tone") — drawing = a smooth
# function of the surface point, fallback = rint(0.8 drawing + 10) — measured on this restatement:
# 15.66 levels with the hard composition, 2.88 levelled (112 texel pairs).  At 37^2: 15.54 -> 6.99.
STEP_BEFORE, STEP_AFTER = 15.657738095238095, 2.8839285714285716


# ------------------------------------------------------------------ the rule
def corners(uvs, indices, group, n_groups, face_id):
    """Per texel (row-major): sound (T) bool, the corners' groups (T,3) int64 (0 where not sound) and
    the barycentrics (T,3) of the sample point (c, S - 1 - r), whatever the arithmetic gave."""
    S = int(face_id.shape[0])
    uv = np.asarray(uvs, np.float32).astype(np.float64).reshape(-1, 2) * float(S)
    ind = np.asarray(indices, np.int64).reshape(-1, 3)
    grp = np.asarray(group, np.int64).reshape(-1)
    m = np.asarray(face_id, np.int64).reshape(-1)
    T, V, M = S * S, len(uv), len(ind)
    ok = (m >= 0) & (m < M)
    tri = ind[np.where(ok, m, 0)] if M else np.zeros((T, 3), np.int64)
    ok = ok & (tri.min(1) >= 0) & (tri.max(1) < V)
    tri = np.where(ok[:, None], tri, 0)
    if V == 0:
        uv, grp = np.zeros((1, 2)), np.zeros(1, np.int64)
    g = grp[tri]
    ok = ok & (g.min(1) >= 0) & (g.max(1) < int(n_groups))
    r = np.arange(T) // S
    c = np.arange(T) - r * S
    px, py = c.astype(np.float64), (S - 1 - r).astype(np.float64)
    ia, ib, ic = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(all="ignore"):
        w0, w1, w2 = R._edges((uv[ia, 0], uv[ia, 1], uv[ib, 0], uv[ib, 1], uv[ic, 0], uv[ic, 1]), px, py)
        area = (w0 + w1) + w2
        b = np.stack([w0 / area, w1 / area, w2 / area], -1)
    ok = ok & np.isfinite(area) & (area > 0)
    return ok, np.where(ok[:, None], g, 0), b


def gather(uvs, indices, group, n_groups, face_id, source, proj, fallback):
    """h. -> num (G,3) int64, den (G) int64."""
    G = int(n_groups)
    num, den = np.zeros((G, 3), np.int64), np.zeros(G, np.int64)
    if G == 0 or len(np.asarray(indices).reshape(-1, 3)) == 0:
        return num, den
    ok, g, b = corners(uvs, indices, group, G, face_id)
    use = ok & (np.asarray(source).reshape(-1) != 0)
    with np.errstate(all="ignore"):
        v = np.floor(b * float(ONE) + 0.5)
        q = np.where(v > 0, np.minimum(v, float(ONE)), 0.0)               # a NaN fails v > 0
    q = np.where(use[:, None], q, 0.0).astype(np.int64)
    diff = np.asarray(proj).reshape(-1, 3).astype(np.int64) - np.asarray(fallback).reshape(-1, 3).astype(np.int64)
    for i in range(3):
        np.add.at(den, g[:, i], q[:, i])
        np.add.at(num, g[:, i], q[:, i, None] * diff)
    return num, den


def apply(uvs, indices, group, face_id, source, proj, fallback, d, return_fragile=False):
    """i. -> image (S,S,3) u8 [, fragile (S,S) bool: a levelled texel with a channel whose v + 0.5 lies
    within FRAGILE of an integer]."""
    S = int(face_id.shape[0])
    d = np.asarray(d, np.float64).reshape(-1, 3)
    G = len(d)
    M = len(np.asarray(indices).reshape(-1, 3))
    if G == 0 or M == 0:
        ok = np.zeros(S * S, bool)
        g, b, d = np.zeros((S * S, 3), np.int64), np.zeros((S * S, 3)), np.zeros((1, 3))
    else:
        ok, g, b = corners(uvs, indices, group, G, face_id)
    fb = np.asarray(fallback).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = (b[:, 0, None] * d[g[:, 0]] + b[:, 1, None] * d[g[:, 1]]) + b[:, 2, None] * d[g[:, 2]]
        v = fb.astype(np.float64) + e
        finite = np.isfinite(v)
        lev = np.clip(np.floor(np.where(finite, v, 0.0) + 0.5), 0.0, 255.0).astype(np.uint8)
    levelled = np.where(finite, lev, fb)
    m = np.asarray(face_id, np.int64).reshape(-1)
    src = np.asarray(source).reshape(-1)
    out = np.where((src != 0)[:, None], np.asarray(proj).reshape(-1, 3), np.where(ok[:, None], levelled, fb))
    out = np.where((m < 0)[:, None], 0, out).astype(np.uint8).reshape(S, S, 3)
    if not return_fragile:
        return out
    with np.errstate(all="ignore"):
        near = np.abs((v + 0.5) - np.rint(v + 0.5)) <= FRAGILE
    fragile = (ok & (src == 0) & (m >= 0))[:, None] & finite & near
    return out, fragile.any(1).reshape(S, S)


def levelled_texels(uvs, indices, group, n_groups, face_id, source):
    """(S,S) bool: the texels i. levels (covered, not projected, on a sound face)."""
    ok = corners(uvs, indices, group, n_groups, face_id)[0].reshape(face_id.shape)
    return ok & (np.asarray(source) == 0) & (np.asarray(face_id) >= 0)


def offsets(num, den, group_faces):
    """The host step -> d (G,3) f64, known (G) bool: known groups num / den, the rest by the uniform
    Laplacian over the edges of group_faces (dense bookkeeping, scipy's spsolve per component set)."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    num, den = np.asarray(num, np.int64).reshape(-1, 3), np.asarray(den, np.int64).reshape(-1)
    G = len(den)
    known = den >= ONE
    d = np.zeros((G, 3))
    d[known] = num[known].astype(np.float64) / den[known].astype(np.float64)[:, None]
    nb = [set() for _ in range(G)]
    for a, b, c in np.asarray(group_faces, np.int64).reshape(-1, 3):
        if a == b or b == c or a == c:
            continue
        for p, q in ((a, b), (b, c), (c, a)):
            nb[p].add(int(q))
            nb[q].add(int(p))
    # flood the unknowns from the known groups: what is reached is solved, the rest keeps 0
    reached = np.zeros(G, bool)
    stack = [u for k in np.flatnonzero(known) for u in nb[k] if not known[u]]
    while stack:
        u = stack.pop()
        if reached[u]:
            continue
        reached[u] = True
        stack.extend(n for n in nb[u] if not known[n] and not reached[n])
    rows = np.flatnonzero(reached)
    if not len(rows):
        return d, known
    slot = np.full(G, -1, np.int64)
    slot[rows] = np.arange(len(rows))
    A = sp.lil_matrix((len(rows), len(rows)))
    rhs = np.zeros((len(rows), 3))
    for k, u in enumerate(rows):
        A[k, k] = float(len(nb[u]))
        for n in sorted(nb[u]):
            if known[n]:
                rhs[k] += d[n]
            else:
                A[k, slot[n]] = -1.0
    d[rows] = np.asarray(spsolve(A.tocsc(), rhs)).reshape(len(rows), 3)
    return d, known


class RefBackend(F.RefBackend):
    """uv_field_ref.RefBackend + the three seam steps."""

    def seam_gather(self, uvs, indices, group, n_groups, face_id, source, proj, fallback):
        return gather(uvs, indices, group, n_groups, face_id, source, proj, fallback)

    def seam_solve(self, A, rhs):
        from scipy.sparse.linalg import spsolve
        return np.asarray(spsolve(A.tocsc(), np.asarray(rhs, np.float64))).reshape(np.shape(rhs))

    def seam_apply(self, uvs, indices, group, face_id, source, proj, fallback, d):
        image, self.seam_fragile = apply(uvs, indices, group, face_id, source, proj, fallback, d, return_fragile=True)
        return image


def with_projection(backend, proj, source):
    """`backend` with its project() replaced by one that hands back the given proj / source: the seam
    tests feed bake_drawings a synthetic projection, so dsu_uv_project is not involved."""
    backend.project = lambda *a, **k: (proj, source)
    return backend


def bake_level(c, backend, gutter=0, convert=lambda a: a):
    """bake_drawings(seam="level") of a seam_case through `backend`, the case's proj / source standing
    in for the projection and its fallback for the field bake.  -> image (S,S,3) u8."""
    from drawingspinup_amd.nsr import uv as U
    be = with_projection(backend, convert(np.array(c["proj"])), convert(np.array(c["source"])))
    zeros = np.zeros((len(c["uvs"]), 3), np.float32)
    return U.bake_drawings(c["uvs"], c["indices"], c["positions"], None, None, None, zeros, c["size"], gutter,
                           backend=be, fallback_image=np.array(c["fallback"]), seam="level",
                           groups=c["group"], group_faces=c["group_faces"])


# ------------------------------------------------------------------ the library's host entries
def _lib():
    from drawingspinup_amd import _lib as L
    return L.lib()


_p = F._p


def _arrays(c):
    return (np.ascontiguousarray(c["uvs"], np.float32), np.ascontiguousarray(c["indices"], np.int32),
            np.ascontiguousarray(c["group"], np.int32), np.ascontiguousarray(c["face_id"], np.int32),
            np.ascontiguousarray(c["source"], np.uint8), np.ascontiguousarray(c["proj"], np.uint8),
            np.ascontiguousarray(c["fallback"], np.uint8))


def host_gather(c):
    """dsu_uv_seam_gather_host on a case -> num (G,3) i64, den (G) i64."""
    uvs, ind, grp, fid, src, proj, fb = _arrays(c)
    G = int(c["n_groups"])
    num, den = np.zeros((G, 3), np.int64), np.zeros(G, np.int64)
    rc = _lib().dsu_uv_seam_gather_host(_p(uvs), _p(ind), _p(grp), len(uvs), len(ind), G, c["size"], _p(fid), _p(src),
                                        _p(proj), _p(fb), _p(num), _p(den))
    assert rc == 0, rc
    return num, den


def host_apply(c, d):
    """dsu_uv_seam_apply_host on a case -> image (S,S,3) u8."""
    uvs, ind, grp, fid, src, proj, fb = _arrays(c)
    d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
    image = np.full((c["size"], c["size"], 3), 77, np.uint8)
    rc = _lib().dsu_uv_seam_apply_host(_p(uvs), _p(ind), _p(grp), len(uvs), len(ind), len(d), c["size"], _p(fid),
                                       _p(src), _p(proj), _p(fb), _p(d) if len(d) else None, _p(image))
    assert rc == 0, rc
    return image


# ------------------------------------------------------------------ cases
CASES = F.CASES
PATTERNS = ("z", "x")
# (case, size, source pattern, colours) on which bake_drawings(seam="level") is compared across backends
LEVEL_CASES = [("icosphere", 64, "z", "tone"), ("icosphere", 64, "x", "tone"), ("icosphere", 37, "z", "tone"),
               ("icosphere", 37, "x", "random"), ("icosphere", 64, "z", "constant"), ("lattice", None, "z", "tone")]


@functools.lru_cache(maxsize=None)
def atlas(name, size=None):
    """F.case + group / n_groups / group_faces, face_chart (M), the texels' surface points `point`
    (S,S,3) f64 (NaN where uncovered) and the vertex data behind the icosphere's atlas."""
    from drawingspinup_amd.nsr import uv as U
    c = dict(F.case(name, size))
    S = c["size"]
    if name == "icosphere":
        v, f = F.icosphere()
        vm, ind, uvs, info = U.parametrize(v, f, S, 2, return_info=True, backend=R.RefBackend())
        assert np.array_equal(uvs, c["uvs"]) and np.array_equal(ind, c["indices"])
        c["group"], c["group_faces"] = U.seam_groups(v, f, vm)
        c["face_chart"] = np.asarray(info["face_chart"], np.int64)
        c["verts"], c["faces"] = v, f
    else:
        c["group"] = np.arange(len(c["uvs"]), dtype=np.int32)
        c["group_faces"] = np.asarray(c["indices"], np.int64)
        c["face_chart"] = np.zeros(len(c["indices"]), np.int64)
    c["n_groups"] = int(c["group"].max()) + 1
    point = np.full((S * S, 3), np.nan)
    point[c["texels"]] = F.restated(name, size, 1)["p64"][:, 0]
    c["point"] = point.reshape(S, S, 3)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def source_map(c, pattern="z"):
    """The synthetic `source` of the tests.  "z": 1 where the texel's surface point has z > 0.2, 2 where
    z < -0.2, 0 between.  "x": the same bands along x at other places, 2 above 0.1 and 1 below -0.15."""
    p = c["point"]
    covered = c["face_id"] >= 0
    with np.errstate(invalid="ignore"):
        if pattern == "z":
            src = np.where(p[..., 2] > 0.2, 1, np.where(p[..., 2] < -0.2, 2, 0))
        else:
            src = np.where(p[..., 0] > 0.1, 2, np.where(p[..., 0] < -0.15, 1, 0))
    return np.where(covered, src, 0).astype(np.uint8)


def random_bytes(S, seed, lo=40, hi=200):
    """(S,S,3) u8 arbitrary bytes in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, (S, S, 3)).astype(np.uint8)


def smooth_bytes(c):
    """(S,S,3) u8: a smooth (affine) function of the texel's surface point, in [38, 230]; 0 where uncovered."""
    val = np.rint(F.affine(np.nan_to_num(c["point"])) * 255.0)
    return np.where((c["face_id"] >= 0)[..., None], val, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def seam_case(name, size=None, pattern="z", colours="random"):
    """A whole input set: atlas + source + proj + fallback.  colours: "random" = proj arbitrary bytes
    in [40, 200] and fallback other arbitrary bytes; "constant" = fallback = proj - (10, -7, 0);
    "tone" = proj smooth, fallback = rint(0.8 proj + 10) (the field's lighter, flatter tone)."""
    c = dict(atlas(name, size))
    S = c["size"]
    c["source"] = source_map(c, pattern)
    if colours == "random":
        c["proj"], c["fallback"] = random_bytes(S, 1), random_bytes(S, 2, 0, 255)
    elif colours == "constant":
        c["proj"] = random_bytes(S, 3)
        c["fallback"] = (c["proj"].astype(np.int64) - np.asarray([10, -7, 0])).astype(np.uint8)
    elif colours == "tone":
        c["proj"] = smooth_bytes(c)
        c["fallback"] = np.rint(0.8 * c["proj"].astype(np.float64) + 10.0).astype(np.uint8)
    else:
        raise KeyError(colours)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def restated(name, size=None, pattern="z", colours="random"):
    """num, den, d, known, image and fragile of a seam_case by the restatement, read-only."""
    c = seam_case(name, size, pattern, colours)
    num, den = gather(c["uvs"], c["indices"], c["group"], c["n_groups"], c["face_id"], c["source"], c["proj"],
                      c["fallback"])
    d, known = offsets(num, den, c["group_faces"])
    image, fragile = apply(c["uvs"], c["indices"], c["group"], c["face_id"], c["source"], c["proj"], c["fallback"], d,
                           return_fragile=True)
    out = {"num": num, "den": den, "d": d, "known": known, "image": image, "fragile": fragile,
           "levelled": levelled_texels(c["uvs"], c["indices"], c["group"], c["n_groups"], c["face_id"], c["source"])}
    for a in out.values():
        a.setflags(write=False)
    return out


def edge_cases():
    """name -> (case dict with its own arrays, d (G,3) or None = the restatement's own offsets): the rows
    of include/dsu_hip.h h. / i. that must add nothing / keep the fallback, on the icosphere at 37."""
    def fresh(**kw):
        c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in seam_case("icosphere", 37).items()}
        c.update(kw)
        return c
    base = seam_case("icosphere", 37)
    S, fid = 37, base["face_id"]
    covered = np.nonzero(fid.reshape(-1) >= 0)[0]
    # faces under projected texels only and faces under fallback texels only
    flat_src = base["source"].reshape(-1)[covered]
    faces = np.unique(fid.reshape(-1)[covered])
    on = np.isin(faces, fid.reshape(-1)[covered[flat_src != 0]])
    off = np.isin(faces, fid.reshape(-1)[covered[flat_src == 0]])
    lit, dark = faces[on & ~off], faces[off & ~on]
    pick = [lit[0], dark[0], lit[len(lit) // 2], dark[len(dark) // 2]]
    out = {}
    c = fresh()
    c["face_id"].reshape(-1)[covered[::11]] = len(c["indices"]) + 3
    out["face_id_out_of_range"] = (c, None)
    c = fresh()
    c["indices"][pick[0], 1], c["indices"][pick[1], 2] = len(c["uvs"]), -1
    out["vertex_index_out_of_range"] = (c, None)
    c = fresh()
    c["group"][c["indices"][pick[0], 0]], c["group"][c["indices"][pick[1], 1]] = c["n_groups"], -1
    out["group_out_of_range"] = (c, None)
    c = fresh()
    c["uvs"][c["indices"][pick[2], 0]] = np.nan
    c["uvs"][c["indices"][pick[3], 2]] = np.nan
    out["nan_uv"] = (c, None)
    c = fresh()
    for m in pick[:2]:
        c["uvs"][c["indices"][m, 1]] = c["uvs"][c["indices"][m, 0]]               # two corners on one point
    out["zero_area_face"] = (c, None)
    c = fresh()
    src = c["source"]
    src[(src == 1) & (np.arange(S)[None, :] % 2 == 0)] = 255
    out["source_1_2_255"] = (c, None)
    c = fresh(source=np.zeros((S, S), np.uint8))
    out["nothing_projected"] = (c, None)
    c = fresh(source=np.where(fid >= 0, 1, 0).astype(np.uint8))
    out["everything_projected"] = (c, None)
    c = fresh()
    d = np.array(restated("icosphere", 37)["d"])
    d[::5, 1] = np.nan
    d[3::7] = np.inf
    out["nan_in_d"] = (c, d)
    c = fresh()
    d = np.array(restated("icosphere", 37)["d"])
    d[::2] += 400.0
    d[1::2] -= 400.0
    out["past_0_and_255"] = (c, d)
    # one projected texel: its three groups get less than a whole texel's weight each
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in seam_case("triangle").items()}
    c["source"][:] = 0
    inner = np.nonzero(c["face_id"].reshape(-1) >= 0)[0]
    c["source"].reshape(-1)[inner[len(inner) // 2]] = 1
    out["slivers_only"] = (c, None)
    return out


# ------------------------------------------------------------------ the measure
def seam_step(image, source, face_id, face_chart):
    """The mean |a - b| over the 4-neighbour texel pairs (and channels) inside one chart of which one
    texel is projected (source != 0) and the other is not; also the number of pairs."""
    img = np.asarray(image).astype(np.float64)
    fid = np.asarray(face_id, np.int64)
    chart = np.where(fid >= 0, np.asarray(face_chart, np.int64)[np.where(fid >= 0, fid, 0)], -1)
    on = np.asarray(source) != 0
    total, n = 0.0, 0
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        pair = (chart[a] >= 0) & (chart[a] == chart[b]) & (on[a] != on[b])
        total += float(np.abs(img[a] - img[b])[pair].sum())
        n += int(pair.sum())
    return total / max(3 * n, 1), n
