"""Float64 numpy restatement of dsu_uv_field_points / dsu_uv_field_resolve (include/dsu_hip.h, UV
export f. and g.), independent of csrc/uv_field.h: the sample points of the covered texels from the
atlas barycentrics (not clamped), and the mean of a texel's valid samples quantised as the bake
does.  RefBackend plugs the restatement into drawingspinup_amd.nsr.uv.bake_field / uv_mapping on
top of tests/uv_project_ref.py's backend (raster, gutter fill, drawings).  Also the cases and the
per-point callables the host and GPU tests share."""
import ctypes
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_project_ref as P  # noqa: E402
import uv_ref as R  # noqa: E402


# ------------------------------------------------------------------ the rule
def field_samples(uvs, indices, positions, face_id, texels, s):
    """-> dict(points (T, s s, 3) f32, valid (T, s s) u8, p64 (T, s s, 3) the point before its one
    rounding, b (T, s s, 3) the barycentrics, area (T, s s)); rows of invalid samples hold whatever
    the arithmetic gave (NaN included) in p64 / b / area and zeros in points."""
    S, s = int(face_id.shape[0]), int(s)
    uv = np.asarray(uvs, np.float32).astype(np.float64).reshape(-1, 2) * float(S)
    pos = np.asarray(positions, np.float32).astype(np.float64).reshape(-1, 3)
    ind = np.asarray(indices, np.int64).reshape(-1, 3)
    tex = np.asarray(texels, np.int64).reshape(-1)
    T, ss, V, M = len(tex), s * s, len(uv), len(ind)
    inside = (tex >= 0) & (tex < S * S)
    m = np.where(inside, np.asarray(face_id, np.int64).reshape(-1)[np.where(inside, tex, 0)], -1)
    ok = (m >= 0) & (m < M)
    tri = ind[np.where(ok, m, 0)] if M else np.zeros((T, 3), np.int64)
    ok &= (tri.min(1) >= 0) & (tri.max(1) < V) if T else ok
    ia, ib, ic = (np.where(ok, tri[:, k], 0) for k in range(3))
    if V == 0:
        uv, pos = np.zeros((1, 2)), np.zeros((1, 3))
    r = tex // S
    c = tex - r * S
    j = np.arange(ss)
    jy = j // s
    jx = j - jy * s
    off = lambda i: (2 * i + 1 - s).astype(np.float64) / float(2 * s)
    px = c.astype(np.float64)[:, None] + off(jx)[None, :]
    py = (S - 1 - r).astype(np.float64)[:, None] + off(jy)[None, :]
    col = lambda a: a[:, None]
    with np.errstate(all="ignore"):
        w0, w1, w2 = R._edges((col(uv[ia, 0]), col(uv[ia, 1]), col(uv[ib, 0]), col(uv[ib, 1]), col(uv[ic, 0]),
                               col(uv[ic, 1])), px, py)
        area = (w0 + w1) + w2
        b0, b1, b2 = w0 / area, w1 / area, w2 / area
        p64 = (b0[..., None] * pos[ia][:, None, :] + b1[..., None] * pos[ib][:, None, :]) + \
            b2[..., None] * pos[ic][:, None, :]
        p32 = p64.astype(np.float32)
    good = ok[:, None] & np.isfinite(area) & (area > 0) & np.isfinite(p32).all(-1)
    points = np.where(good[..., None], p32, np.float32(0.0)).astype(np.float32)
    return {"points": points, "valid": good.astype(np.uint8), "p64": p64, "b": np.stack([b0, b1, b2], -1),
            "area": area}


def field_points(uvs, indices, positions, face_id, texels, s):
    out = field_samples(uvs, indices, positions, face_id, texels, s)
    return out["points"], out["valid"]


def field_resolve(colours, valid, texels, image):
    """image (S,S,3) u8 is written in place at the listed texels that have a valid sample, and returned."""
    S = image.shape[0]
    tex = np.asarray(texels, np.int64).reshape(-1)
    col = np.asarray(colours, np.float32).reshape(len(tex), -1, 3)
    ok = np.asarray(valid).reshape(len(tex), -1) > 0
    total = np.zeros((len(tex), 3))
    for j in range(col.shape[1]):                                          # ascending j, one addition each
        with np.errstate(all="ignore"):
            total = np.where(ok[:, j, None], total + col[:, j].astype(np.float64), total)
    n = ok.sum(1)
    with np.errstate(all="ignore"):
        val = total / n[:, None].astype(np.float64) * 255.0
        q = np.where(np.isnan(val), 0.0, np.clip(val, 0.0, 255.0)).astype(np.uint8)
    write = (n > 0) & (tex >= 0) & (tex < S * S)
    image.reshape(-1, 3)[tex[write]] = q[write]
    return image


class RefBackend(P.RefBackend):
    """uv_project_ref.RefBackend + the field bake's two steps."""

    def field_points(self, uvs, indices, positions, face_id, texels, samples):
        return field_points(uvs, indices, positions, face_id, texels, samples)

    def field_resolve(self, colours, valid, texels, image):
        return field_resolve(colours, valid, texels, image)


# ------------------------------------------------------------------ the library's host entries
def _lib():
    from drawingspinup_amd import _lib as L
    return L


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def host_points(c, s, texels=None):
    """dsu_uv_field_points_host on a case -> points (T, s s, 3) f32, valid (T, s s) u8."""
    uvs, ind = np.ascontiguousarray(c["uvs"], np.float32), np.ascontiguousarray(c["indices"], np.int32)
    pos, fid = np.ascontiguousarray(c["positions"], np.float32), np.ascontiguousarray(c["face_id"], np.int32)
    tex = np.ascontiguousarray(c["texels"] if texels is None else texels, np.int32)
    points = np.full((len(tex), s * s, 3), 7.0, np.float32)
    valid = np.full((len(tex), s * s), 9, np.uint8)
    rc = _lib().lib().dsu_uv_field_points_host(_p(uvs), _p(ind), _p(pos), len(uvs), len(ind), c["size"], _p(fid),
                                             _p(tex), len(tex), s, _p(points), _p(valid))
    assert rc == 0, rc
    return points, valid


def host_resolve(colours, valid, texels, image, s):
    """dsu_uv_field_resolve_host: image (S,S,3) u8 is written in place, and returned."""
    colours, valid = np.ascontiguousarray(colours, np.float32), np.ascontiguousarray(valid, np.uint8)
    tex = np.ascontiguousarray(texels, np.int32)
    rc = _lib().lib().dsu_uv_field_resolve_host(_p(colours), _p(valid), _p(tex), len(tex), s, image.shape[0], _p(image))
    assert rc == 0, rc
    return image


# ------------------------------------------------------------------ per-point callables
def _f64(p):
    import torch
    return (p.double(), torch) if torch.is_tensor(p) else (np.asarray(p).astype(np.float64), np)


STRIPES_PER_UNIT = 40.0          # period 0.05: a third of the 0.15-long edges of the 320-face icosphere


def stripes(p):
    """(N,3) f32 points (numpy or torch) -> (N,3) colours: the parities of floor(40 x) per axis, in
    float64.  Products with 40 and 0.5, floor and differences of small integers: every operation
    is correctly rounded or exact on both sides, so numpy and the device give the same bits."""
    x, lib = _f64(p)
    k = lib.floor(x * STRIPES_PER_UNIT)
    par = k - 2.0 * lib.floor(k * 0.5)                                     # 0 or 1
    return lib.stack([par[:, 0], 0.25 + 0.5 * par[:, 1], 0.5 * (par[:, 0] + par[:, 2])], -1)


AFFINE_A = np.asarray([[0.6, 0.1, -0.2], [-0.15, 0.5, 0.2], [0.25, -0.3, 0.45]])
AFFINE_B = np.asarray([0.5, 0.45, 0.55])


def affine(p):
    """An affine map of position (numpy points), in float64: within [0.15, 0.9] on the ball of radius 0.5."""
    return np.asarray(p).astype(np.float64) @ AFFINE_A.T + AFFINE_B


# ------------------------------------------------------------------ cases
def _atlas(uvs, indices, positions, size):
    uvs, indices = np.asarray(uvs, np.float32), np.asarray(indices, np.int64)
    face_id = R.bake(uvs, indices, np.zeros((len(uvs), 3), np.float32), size)[1]
    return {"uvs": uvs, "indices": indices, "positions": np.asarray(positions, np.float32), "face_id": face_id,
            "size": size}


@functools.lru_cache(maxsize=None)
def icosphere(subdiv=2, radius=0.5):
    import frame_render_ref as F
    v, f = F.icosphere(subdiv)
    return (v * radius).astype(np.float32), f


@functools.lru_cache(maxsize=None)
def case(name, size=None):
    """uvs, indices, positions (in the field's frame), face_id, size and texels = the covered texels.
    triangle: one face in a 16^2 atlas, nothing special about its numbers.  lattice: a two-triangle
    square whose vertices sit on sample points, its positions a dyadic affine map of uv, so every
    quantity of the rule is exact.  icosphere: 320 faces of radius 0.5 through parametrize at the
    given size (64: several tiles; 37: no multiple of anything)."""
    from drawingspinup_amd.nsr import uv as U
    if name == "triangle":
        c = _atlas([[0.11, 0.07], [0.93, 0.21], [0.34, 0.88]], [[0, 1, 2]],
                   [[-0.31, 0.12, 0.4], [0.45, -0.2, 0.1], [0.05, 0.37, -0.33]], 16)
    elif name == "lattice":
        uv = np.asarray([[2, 2], [10, 2], [10, 10], [2, 10]], np.float64) / 16.0
        pos = np.stack([uv[:, 0] - 0.5, uv[:, 1] - 0.25, 0.25 * uv[:, 0] + 0.5 * uv[:, 1] - 0.125], -1)
        c = _atlas(uv, [[0, 1, 2], [0, 2, 3]], pos, 16)
    elif name == "icosphere":
        v, f = icosphere()
        vm, ind, uvs = U.parametrize(v, f, size, 2, backend=R.RefBackend())
        c = _atlas(uvs, ind, v[vm], size)
        c["vmapping"] = vm
    else:
        raise KeyError(name)
    c["texels"] = np.nonzero(c["face_id"].reshape(-1) >= 0)[0].astype(np.int32)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


CASES = [("triangle", None), ("lattice", None), ("icosphere", 64), ("icosphere", 37)]
SAMPLES = (1, 2, 4)


@functools.lru_cache(maxsize=None)
def restated(name, size, s):
    """field_samples of a case, read-only."""
    c = case(name, size)
    out = field_samples(c["uvs"], c["indices"], c["positions"], c["face_id"], c["texels"], s)
    for a in out.values():
        a.setflags(write=False)
    return out


def edge_rows():
    """The icosphere-at-37 case with rows that must come out invalid: an uncovered texel and indices
    outside the atlas in the list, a face id out of range, a face with a vertex index out of range,
    a NaN vertex.  -> (case dict with its own arrays, dict name -> rows of `texels`)."""
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in case("icosphere", 37).items()}
    S, fid = c["size"], c["face_id"]
    covered = c["texels"]
    uncovered = np.nonzero(fid.reshape(-1) < 0)[0][:3].astype(np.int32)
    pick = covered[[5, len(covered) // 3, len(covered) // 2, 2 * len(covered) // 3]]
    flat = fid.reshape(-1)
    faces = flat[pick].copy()
    flat[pick[0]] = len(c["indices"]) + 7                                  # a face id out of range
    c["indices"][faces[1], 1] = len(c["uvs"])                              # a vertex index out of range
    c["indices"][faces[2], 2] = -1
    c["positions"][c["indices"][faces[3], 0]] = np.nan                     # a NaN vertex
    rows = {"uncovered": uncovered, "outside": np.asarray([-1, S * S, S * S + 5], np.int32),
            "bad_face": np.nonzero(fid.reshape(-1) == flat[pick[0]])[0].astype(np.int32),
            "bad_index": np.nonzero(np.isin(fid.reshape(-1), faces[1:3]))[0].astype(np.int32),
            "nan_vertex": np.nonzero(np.isin(fid.reshape(-1),
                                             np.nonzero((c["indices"] == c["indices"][faces[3], 0]).any(1))[0]))[0]
            .astype(np.int32)}
    c["texels"] = np.concatenate([covered, rows["uncovered"], rows["outside"]]).astype(np.int32)
    return c, rows


def resolve_inputs(n_texels, s, seed=0):
    """colours (T, s s, 3) f32 with values below 0, above 1 and NaN among them, valid (T, s s) u8 with
    empty rows, for a resolve test."""
    rng = np.random.default_rng(seed)
    col = (rng.random((n_texels, s * s, 3)) * 1.4 - 0.2).astype(np.float32)
    col[rng.random(col.shape) < 0.02] = np.nan
    valid = (rng.random((n_texels, s * s)) < 0.7).astype(np.uint8)
    valid[::7] = 0
    return col, valid
