"""Float64 numpy restatement of dsu_uv_project_area (include/dsu_hip.h, UV export j.), independent of
csrc/uv_project_area.h: every sub-sample's point from the atlas barycentrics (not clamped), the
view from the face, the mask at the nearest pixel, a brute-force occluder search over ALL triangles
behind a padded-box candidate filter (no grid, no grouping of the samples: the entry's answer must
not depend on either), the nearest or bilinear value, and the mean in ascending sample order.  The
operations and their order are the header's, so the library's host entry is held to EQUALITY in
every byte.  RefBackend plugs the restatement into nsr.uv.bake_drawings / uv_mapping.  Also: a numpy
z-grid for the host entry (the device's is built by ops.ZGrid), the host entry's ctypes call, and
the cases the host and GPU tests share."""
import ctypes
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_project_ref as P  # noqa: E402
import uv_ref as R  # noqa: E402
import uv_seam_ref as S  # noqa: E402

FILTERS = ("nearest", "bilinear")
BBOX_PAD = P.BBOX_PAD


# ------------------------------------------------------------------ the rule
def offsets(s):
    """o(i) = (2 i + 1 - s) / (2 s), i = 0 .. s - 1."""
    return (2.0 * np.arange(s) + 1.0 - s) / (2.0 * s)


def occluded(p, sign, own, P64, ind, valid, z_tolerance):
    """p (K,3) finite points, sign (K) +-1, own (K) the face each point lies on -> (K) bool: e.'s
    test against every valid triangle but the point's own."""
    out = np.zeros(len(p), bool)
    if not len(p):
        return out
    order = np.argsort(p[:, 0], kind="stable")
    sx = p[order, 0]
    qy, qz = p[:, 1], p[:, 2]
    for f in np.nonzero(valid)[0]:
        t = P64[ind[f]]
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = t
        if not np.all(np.isfinite(t[:, :2])):
            continue
        lo, hi = np.searchsorted(sx, [min(ax, bx, cx) - BBOX_PAD, max(ax, bx, cx) + BBOX_PAD])
        k = order[lo:hi]
        k = k[(qy[k] >= min(ay, by, cy) - BBOX_PAD) & (qy[k] <= max(ay, by, cy) + BBOX_PAD) & (own[k] != f)]
        if len(k) == 0:
            continue
        x, y = p[k, 0], qy[k]
        e0 = (x - bx) * (cy - by) - (y - by) * (cx - bx)
        e1 = (x - cx) * (ay - cy) - (y - cy) * (ax - cx)
        e2 = (x - ax) * (by - ay) - (y - ay) * (bx - ax)
        ar = (e0 + e1) + e2
        covers = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (ar != 0)
        with np.errstate(all="ignore"):
            d = (((e0 * az + e1 * bz) + e2 * cz) / ar - qz[k]) * sign[k]
        out[k[covers & (d > z_tolerance)]] = True
    return out


def values(colour, res, back, px, py, pixel_filter):
    """Step 5 for points (K) -> (K,3) f64."""
    span = float(res - 1)
    sx = np.where(back, -px, px)
    if pixel_filter == "nearest":
        X = np.clip(np.rint((sx + 0.5) * span), 0, span).astype(np.int64)
        Y = np.clip(np.rint((-py + 0.5) * span), 0, span).astype(np.int64)
        return colour[Y, X].astype(np.float64)
    fx, fy = np.clip((sx + 0.5) * span, 0, span), np.clip((-py + 0.5) * span, 0, span)
    x0 = np.minimum(np.floor(fx).astype(np.int64), max(res - 2, 0))
    y0 = np.minimum(np.floor(fy).astype(np.int64), max(res - 2, 0))
    x1, y1 = np.minimum(x0 + 1, res - 1), np.minimum(y0 + 1, res - 1)
    tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
    c00, c10 = colour[y0, x0].astype(np.float64), colour[y0, x1].astype(np.float64)
    c01, c11 = colour[y1, x0].astype(np.float64), colour[y1, x1].astype(np.float64)
    return ((1.0 - ty) * ((1.0 - tx) * c00 + tx * c10)) + (ty * ((1.0 - tx) * c01 + tx * c11))


def passing(uvs, indices, positions, face_id, mask_front, mask_back, z_tolerance, s):
    """Steps 1-4 and 6's extra sample, which do not depend on the filter: -> dict(rows, cols (N) of the
    texels with a face and a view, back (N) bool, p (N, s s + 1, 3) the points (the last one the
    texel's own), ok (N, s s + 1) bool)."""
    S_ = face_id.shape[0]
    uv = np.asarray(uvs, np.float32).astype(np.float64) * float(S_)
    P64 = np.asarray(positions, np.float32).astype(np.float64)
    ind = np.asarray(indices, np.int64).reshape(-1, 3)
    fid = np.asarray(face_id, np.int64)
    res = mask_front.shape[0]
    valid = np.zeros(len(ind), bool)
    if len(ind):
        valid = (ind.min(1) >= 0) & (ind.max(1) < len(P64))
    live = (fid >= 0) & (fid < len(ind))
    live[live] = valid[fid[live]]
    rows, cols = np.nonzero(live)
    m = fid[rows, cols]
    ia, ib, ic = ind[m, 0], ind[m, 1], ind[m, 2]
    with np.errstate(all="ignore"):
        Pa, Pb, Pc = P64[ia], P64[ib], P64[ic]
        nz = (Pb[:, 0] - Pa[:, 0]) * (Pc[:, 1] - Pa[:, 1]) - (Pb[:, 1] - Pa[:, 1]) * (Pc[:, 0] - Pa[:, 0])
        keep = (nz > 0) | (nz < 0)
        rows, cols, m, ia, ib, ic, Pa, Pb, Pc, nz = (a[keep] for a in (rows, cols, m, ia, ib, ic, Pa, Pb, Pc, nz))
        back = nz < 0
        o = offsets(s)
        ox = np.concatenate([np.tile(o, s), [0.0]])                        # j = jy s + jx, then the own point
        oy = np.concatenate([np.repeat(o, s), [0.0]])
        x = cols.astype(np.float64)[:, None] + ox[None]
        y = (S_ - 1 - rows).astype(np.float64)[:, None] + oy[None]
        t = tuple(a[:, None] for a in (uv[ia, 0], uv[ia, 1], uv[ib, 0], uv[ib, 1], uv[ic, 0], uv[ic, 1]))
        w0, w1, w2 = R._edges(t, x, y)
        area = (w0 + w1) + w2
        b0, b1, b2 = w0 / area, w1 / area, w2 / area
        p = (b0[..., None] * Pa[:, None] + b1[..., None] * Pb[:, None]) + b2[..., None] * Pc[:, None]
        finite = np.isfinite(p).all(-1)
        span = float(res - 1)
        sx = np.where(back[:, None], -p[..., 0], p[..., 0])
        X = np.clip(np.rint(np.where(finite, (sx + 0.5) * span, 0.0)), 0, span).astype(np.int64)
        Y = np.clip(np.rint(np.where(finite, (-p[..., 1] + 0.5) * span, 0.0)), 0, span).astype(np.int64)
    mask = np.where(back[:, None], np.asarray(mask_back)[Y, X], np.asarray(mask_front)[Y, X])
    cand = finite & (mask > 0)
    J = s * s + 1
    flat = np.nonzero(cand.reshape(-1))[0]
    texel = flat // J
    occ = occluded(p.reshape(-1, 3)[flat], np.where(back[texel], -1.0, 1.0), m[texel], P64, ind, valid,
                   float(z_tolerance))
    ok = cand.copy().reshape(-1)
    ok[flat[occ]] = False
    return {"rows": rows, "cols": cols, "back": back, "p": p, "ok": ok.reshape(-1, J)}


def resolve(g, size, color_front, color_back, s, pixel_filter):
    """Steps 5-7 from passing()'s result -> image (S,S,3) u8, source (S,S) u8, count (S,S) u8."""
    image = np.zeros((size, size, 3), np.uint8)
    source = np.zeros((size, size), np.uint8)
    count = np.zeros((size, size), np.uint8)
    rows, cols, back, p, ok = g["rows"], g["cols"], g["back"], g["p"], g["ok"]
    if not len(rows):
        return image, source, count
    res = color_front.shape[0]
    n = ok[:, :s * s].sum(1)
    total = np.zeros((len(rows), 3))
    for j in range(s * s):                                                   # ascending j
        use = ok[:, j]
        v = np.zeros((len(rows), 3))
        for view, colour in ((False, color_front), (True, color_back)):
            k = use & (back == view)
            v[k] = values(np.asarray(colour), res, view, p[k, j, 0], p[k, j, 1], pixel_filter)
        total = np.where(use[:, None], total + v, total)
    extra = (n == 0) & ok[:, s * s]
    for view, colour in ((False, color_front), (True, color_back)):
        k = extra & (back == view)
        total[k] = 0.0 + values(np.asarray(colour), res, view, p[k, s * s, 0], p[k, s * s, 1], pixel_filter)
    used = np.where(extra, 1, n)
    hit = used > 0
    with np.errstate(all="ignore"):
        byte = np.clip(np.floor(total / np.maximum(used, 1)[:, None] + 0.5), 0, 255).astype(np.uint8)
    image[rows[hit], cols[hit]] = byte[hit]
    source[rows[hit], cols[hit]] = np.where(back[hit], 2, 1)
    count[rows, cols] = n
    return image, source, count


def project_area(uvs, indices, positions, face_id, color_front, mask_front, color_back, mask_back, z_tolerance,
                 samples, pixel_filter="nearest"):
    g = passing(uvs, indices, positions, face_id, mask_front, mask_back, z_tolerance, int(samples))
    return resolve(g, face_id.shape[0], color_front, color_back, int(samples), pixel_filter)


class RefBackend(S.RefBackend):
    """uv_seam_ref.RefBackend (bake, project, field and seam steps) + project_area."""

    def project_area(self, uvs, indices, positions, face_id, color_front, mask_front, color_back, z_tolerance, erode,
                     samples, pixel_filter, cells_per_axis=None):
        host = lambda a: np.asarray(a.cpu() if hasattr(a, "cpu") else a)
        front, back = self.masks if self.masks is not None else \
            P.prepare_masks(positions, indices, host(mask_front), erode)
        return project_area(uvs, indices, positions, face_id, host(color_front), host(front), host(color_back),
                            host(back), z_tolerance, samples, pixel_filter)[:2]


# ------------------------------------------------------------------ the host entry
class HostGrid:
    """The z-parallel grid of dsu_zray_cast over tris (F,3,3) f32 as numpy arrays: cell_of in float32
    as csrc/mesh_geom.h has it, a triangle in every cell its box touches.  A triangle with a
    non-finite xy, or not listed in `faces`, is in no list (it can occlude nothing).  g = 1 is the
    one-cell grid: every listed face in one list."""

    def __init__(self, tris, g, faces=None):
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
        xy = tris[:, :, :2].astype(np.float32)
        use = np.isfinite(xy).all((1, 2))
        if faces is not None:
            sel = np.zeros(len(tris), bool)
            sel[faces] = True
            use &= sel
        pts = xy[use].reshape(-1, 2)
        lo = pts.min(0) if len(pts) else np.zeros(2, np.float32)
        hi = pts.max(0) if len(pts) else np.zeros(2, np.float32)
        span = max(float(hi[0] - lo[0]), float(hi[1] - lo[1]), 1e-9)
        self.g, self.cell = int(g), np.float32(span / g * (1.0 + 1e-6))
        self.x0, self.y0 = np.float32(lo[0]), np.float32(lo[1])
        inv = np.float32(1.0) / self.cell

        def cell_of(v, v0):
            c = np.floor((v.astype(np.float32) - v0) * inv)
            return np.clip(c, 0, self.g - 1).astype(np.int64)
        lists = [[] for _ in range(self.g * self.g)]
        for f in np.nonzero(use)[0]:
            cx = cell_of(np.array([xy[f, :, 0].min(), xy[f, :, 0].max()]), self.x0)
            cy = cell_of(np.array([xy[f, :, 1].min(), xy[f, :, 1].max()]), self.y0)
            for a in range(cy[0], cy[1] + 1):
                for b in range(cx[0], cx[1] + 1):
                    lists[a * self.g + b].append(f)
        self.offsets = np.zeros(self.g * self.g + 1, np.int32)
        self.offsets[1:] = np.cumsum([len(x) for x in lists])
        self.items = np.asarray([f for x in lists for f in x] + [0] * int(self.offsets[-1] == 0), np.int32)
        self.tris = tris


class DeviceGrid:
    """A HostGrid on the device, in the form ops.uv_project / uv_project_area take a ZGrid."""

    def __init__(self, grid, dev):
        import torch
        from drawingspinup_amd.ops import ptr
        self._ptr = ptr
        self.data = torch.from_numpy(grid.tris).to(dev).contiguous()
        self.offsets, self.items = torch.from_numpy(grid.offsets).to(dev), torch.from_numpy(grid.items).to(dev)
        self.x0, self.y0, self.cell, self.g = float(grid.x0), float(grid.y0), float(grid.cell), grid.g

    def args(self):
        return (self.x0, self.y0, self.cell, self.g, self._ptr(self.offsets), self._ptr(self.items))


def case_tris(c):
    """positions[indices] (F,3,3) f32, zeros for a face with an index out of range, and the faces whose
    indices are in range."""
    pos = np.asarray(c["positions"], np.float32)
    ind = np.asarray(c["indices"], np.int64).reshape(-1, 3)
    ok = np.zeros(len(ind), bool)
    if len(ind):
        ok = (ind.min(1) >= 0) & (ind.max(1) < len(pos))
    tris = np.zeros((len(ind), 3, 3), np.float32)
    tris[ok] = pos[ind[ok]]
    return tris, np.nonzero(ok)[0]


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def host_project_area(c, s, pixel_filter="nearest", grid=None, g=24, with_count=True, rc_only=False):
    """dsu_uv_project_area_host on a case dict -> image, source, count (None without with_count).
    grid: a HostGrid; None builds one with g cells per axis."""
    from drawingspinup_amd import _lib
    tris, ok = case_tris(c)
    if grid is None:
        grid = HostGrid(tris, g, ok)
    S_ = int(c["face_id"].shape[0])
    a = [np.ascontiguousarray(c["uvs"], np.float32), np.ascontiguousarray(c["indices"], np.int32),
         np.ascontiguousarray(c["positions"], np.float32), np.ascontiguousarray(c["face_id"], np.int32)]
    img = [np.ascontiguousarray(c[k], np.uint8) for k in ("color_front", "mask_front", "color_back", "mask_back")]
    image, source = np.full((S_, S_, 3), 77, np.uint8), np.full((S_, S_), 77, np.uint8)
    count = np.full((S_, S_), 77, np.uint8) if with_count else None
    F = len(a[1])
    rc = _lib.lib().dsu_uv_project_area_host(
        _p(a[0]), _p(a[1]), _p(a[2]), len(a[0]), F, S_, _p(a[3]), _p(grid.tris), float(grid.x0), float(grid.y0),
        float(grid.cell), grid.g, _p(grid.offsets), _p(grid.items), _p(img[0]), _p(img[1]), _p(img[2]), _p(img[3]),
        int(img[0].shape[0]), float(c["z_tolerance"]), int(s), FILTERS.index(pixel_filter), _p(image), _p(source),
        _p(count))
    if rc_only:
        return rc
    assert rc == 0, rc
    return image, source, count


# ------------------------------------------------------------------ cases
# (mesh, atlas size, masks): the arm in front of the body; several layers over one (x, y); an atlas
# that is no multiple of the tile, under the mesh's own eroded silhouette; exact arithmetic
GENERAL = [("body_and_arm", 64, "disc"), ("helicoid", 128, "disc"), ("character", 100, "silhouette"),
           ("lattice", 128, "disc")]
GPU_CASES = GENERAL[:3]


def case(name, size, masks="disc"):
    return P.case(name, size, P.Z_TOL, masks)


@functools.lru_cache(maxsize=None)
def restated(name, size, masks, s):
    """passing() of a case, computed once per s and shared by both filters."""
    c = case(name, size, masks)
    return passing(c["uvs"], c["indices"], c["positions"], c["face_id"], c["mask_front"], c["mask_back"],
                   c["z_tolerance"], s)


def want(name, size, masks, s, pixel_filter):
    c = case(name, size, masks)
    return resolve(restated(name, size, masks, s), size, c["color_front"], c["color_back"], s, pixel_filter)


ALIAS_RES, ALIAS_SIZE = 1025, 64


@functools.lru_cache(maxsize=None)
def aliasing_case():
    """One front-facing square, uv corners at texels 8 and 40 of a 64^2 atlas, x from 1201/2048 - 1/2,
    y from -1/16, 1/8 wide, z = 0, under a 1025^2 drawing of 255 (column & 1): four pixels per texel,
    a texel's own point on pixel coordinate k + 1/2, every sub-sample of s = 4 on an integer."""
    x0, y0, w = 1201.0 / 2048.0 - 0.5, -1.0 / 16.0, 0.125
    pos = np.asarray([[x0, y0, 0], [x0 + w, y0, 0], [x0 + w, y0 + w, 0], [x0, y0 + w, 0]], np.float32)
    assert np.array_equal(pos.astype(np.float64)[:, 0], [x0, x0 + w, x0 + w, x0])       # exact in float32
    uvs = np.asarray([[8, 8], [40, 8], [40, 40], [8, 40]], np.float32) / np.float32(ALIAS_SIZE)
    ind = np.asarray([[0, 1, 2], [0, 2, 3]], np.int64)
    fid = R.bake(uvs, ind, np.zeros((4, 3), np.float32), ALIAS_SIZE)[1]
    col = np.broadcast_to((255 * (np.arange(ALIAS_RES) & 1)).astype(np.uint8)[None, :, None],
                          (ALIAS_RES, ALIAS_RES, 3))
    col = np.ascontiguousarray(col)
    full = np.full((ALIAS_RES, ALIAS_RES), 255, np.uint8)
    out = {"uvs": uvs, "indices": ind, "positions": pos, "face_id": fid, "color_front": col, "color_back": col,
           "mask_front": full, "mask_back": full, "z_tolerance": P.Z_TOL, "size": ALIAS_SIZE}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def edge_rows():
    """name -> case dict: body_and_arm at 64 with one thing broken or degenerate each."""
    base = case("body_and_arm", 64)
    src = base["source"]

    def fresh(**kw):
        c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        c.update(kw)
        return c
    seen = np.unique(base["face_id"][src > 0])
    rows = {"uncovered_texel": fresh()}
    fid = np.array(base["face_id"])
    r, c_ = np.nonzero(src > 0)
    fid[r[::7], c_[::7]] = len(base["indices"]) + 5
    fid[r[3::7], c_[3::7]] = -7
    rows["face_id_out_of_range"] = fresh(face_id=fid)
    ind = np.array(base["indices"])
    ind[seen[len(seen) // 2], 1] = len(base["positions"]) + 3
    ind[seen[len(seen) // 3], 2] = -1
    rows["vertex_index_out_of_range"] = fresh(indices=ind)
    pos = np.array(base["positions"])
    pos[base["indices"][seen[len(seen) // 2], 0]] = np.nan
    rows["nan_vertex"] = fresh(positions=pos)
    zero = np.zeros_like(base["mask_front"])
    rows["all_zero_mask"] = fresh(mask_front=zero, mask_back=zero)
    one = np.full((1, 1), 255, np.uint8)
    rows["res_1"] = fresh(color_front=np.full((1, 1, 3), 201, np.uint8), color_back=np.full((1, 1, 3), 55, np.uint8),
                          mask_front=one, mask_back=one)
    return rows
