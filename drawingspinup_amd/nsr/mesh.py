"""Iso-surface extraction of the NSR export on the device:

    MarchingCubeHelper.forward            instant_nsr/models/geometry.py:50-69
        binary = (level <= 0) * (front_mask > 127)   ->  mcubes.smooth  ->  mcubes.marching_cubes
        ->  verts / (resolution - 1)
    BaseImplicitGeometry.isosurface(_)    geometry.py:83-117   (coarse box -> padded bbox of the
        coarse mesh's vertices -> fine pass with the front mask)
    save_mesh (axis convention, scale, OBJ)    instant_nsr/utils/mesh_utils.py:25-73

The reference does this on the host with PyMCubes 0.1.4 and OpenCV (both absent here, sources not
in the snapshot: PARITY UNPINNED for those two packages).  What is restated, and how:

  * `mcubes.smooth(binary)` -> `smooth_constrained` (the method PyMCubes picks for arrays of at most
    512^3 voxels): the constrained higher-order smoothing of Lempitsky, "Surface extraction from
    binary volumes with higher-order smoothness" (CVPR 2010), as PyMCubes implements it: signed
    Euclidean distance transform (+-0.5 at the boundary voxels), variables = the band |d| <= 4,
    energy |F x|^2 with F the stacked 1-D second differences along the three axes (a neighbour
    outside the band folds onto the diagonal), weighted-Jacobi iterations (weight 0.5) with the
    projection x >= lower, x <= upper where a voxel's bound on its own side is its INITIAL
    distance (`lower = where(x0 > 0, x0, -inf)`, `upper = where(x0 < 0, x0, inf)`), relaxed to 0
    for the voxels next to the surface (`|x0| < 1`): only those may move towards the zero level,
    every other voxel may only move away from it; energy test every 10 iterations (relative
    improvement), float64.
  * `mcubes.marching_cubes(volume, iso)`: x-major / y / z-minor sweep over the cubes, a corner is
    "below" when value <= iso (marchingcubes.h: `if(v[m] <= isovalue) cubeindex |= 1<<m`; the
    projection above leaves many voxels at exactly 0.0, so the rule matters), every grid edge owns ONE vertex (created by the first cube of the
    sweep that touches it: edges 6, 5, 10 of a cube, the remaining nine only on the low faces of
    the volume), vertices numbered in creation order, position by linear interpolation along the
    edge in float64, triangles cube by cube in table order.  The per-cube triangulation is the
    classic 256-configuration table PyMCubes compiles in (nsr/mc_table.py), so vertex AND face
    arrays are the ones `mcubes.marching_cubes` returns for the same volume.  `_build_tables`
    (a generator of a topologically equivalent table from first principles) is kept as a
    cross-check of that table only: tests compare the polygon loops of all 256 rows.
  * `cv2.resize(front_mask, (res, res), INTER_CUBIC)`: OpenCV's bicubic kernel (a = -0.75),
    half-pixel centres, replicated border, rounded and saturated to uint8.

Everything runs as tensor programs on the device (prefix sums over the sweep order instead of the
serial vertex list); the integer outputs are checked bit for bit against a serial restatement
(oracle/mcubes_ref.py).  `remesh` (geometry.py:63-64: quadric decimation of the fine mesh to
50 000 faces) is host code of the library (csrc/mesh_decimate.hip), as it is host code in the
reference; save_mesh's steps are further down and in nsr/mesh_post.py, nsr/thinning.py.
"""
import functools
import math
import os

import numpy as np
import torch

# cube corners (Bourke / PyMCubes numbering) and the two corners of each of the 12 edges
CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
# faces as cyclic corner lists
FACES = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5))
# creation order of a cube's vertices in the sweep and the condition under which THIS cube is the
# first to touch the edge (i, j, k = cube coordinates): edges 6, 5, 10 always, the others only on
# the low faces of the volume
CREATE_ORDER = (6, 5, 10, 0, 1, 2, 3, 4, 7, 8, 9, 11)
# edge -> (axis, (di, dj, dk) of the edge's low corner relative to the cube)
EDGE_AXIS_OFF = {0: (0, (0, 0, 0)), 2: (0, (0, 1, 0)), 4: (0, (0, 0, 1)), 6: (0, (0, 1, 1)),
                 3: (1, (0, 0, 0)), 1: (1, (1, 0, 0)), 7: (1, (0, 0, 1)), 5: (1, (1, 0, 1)),
                 8: (2, (0, 0, 0)), 9: (2, (1, 0, 0)), 11: (2, (0, 1, 0)), 10: (2, (1, 1, 0))}


def _edge_of(a, b):
    for e, (p, q) in enumerate(EDGES):
        if {p, q} == {a, b}:
            return e
    raise KeyError((a, b))


def _coplanar(e0, e1):
    """Do the two cube edges lie on a common cube face (a chord between them runs inside it)?"""
    s0, s1 = set(EDGES[e0]), set(EDGES[e1])
    return any(s0 <= set(f) and s1 <= set(f) for f in FACES)


def _triangulate(loop):
    """Triangles (same orientation as `loop`) of a polygon through cube edges.  Of all
    triangulations, in a fixed enumeration order, the first whose chords avoid the cube's faces:
    a chord inside a face of an ambiguous configuration could coincide with the chord the
    neighbouring cube draws there (an edge shared by four triangles)."""
    n = len(loop)
    best = None

    def rec(i, j):                       # triangulations of the sub-polygon loop[i..j]
        if j - i < 2:
            yield []
            return
        for k in range(i + 1, j):
            for left in rec(i, k):
                for right in rec(k, j):
                    yield left + [(i, k, j)] + right

    for tri in rec(0, n - 1):
        bad = 0
        for a, b, c in tri:
            for p, q in ((a, b), (b, c), (a, c)):
                if (q - p) % n not in (1, n - 1) and _coplanar(loop[p], loop[q]):
                    bad += 1
        if best is None or bad < best[0]:
            best = (bad, tri)
        if bad == 0:
            break
    out = []
    for a, b, c in best[1]:
        out += [loop[a], loop[b], loop[c]]
    return out


@functools.lru_cache(maxsize=None)
def _build_tables():
    """(edge_table (256,) int32 bit masks, tri_table (256, 3*T) int8 padded with -1).

    For every corner configuration (bit m set = corner m below the iso value) the surface inside the
    cube is the set of closed polygons through the crossed edges: each cube face contributes one
    segment between its two crossed edges, or — on a face whose diagonal corners are below — two
    segments that cut the two below-corners off separately (the choice depends on that face's four
    corner states only, so the two cubes sharing the face agree: no cracks).  Polygons are walked
    from their smallest edge, oriented so that the normal points to the below side, and
    triangulated by `_triangulate`."""
    pos = np.array(CORNERS, np.float64)
    mid = np.array([(pos[a] + pos[b]) / 2 for a, b in EDGES])
    edge_table = np.zeros(256, np.int32)
    tris = []
    for c in range(256):
        below = [(c >> m) & 1 for m in range(8)]
        mask = 0
        for e, (a, b) in enumerate(EDGES):
            if below[a] != below[b]:
                mask |= 1 << e
        edge_table[c] = mask
        adj = {e: [] for e in range(12) if mask >> e & 1}
        for f in FACES:
            fe = [_edge_of(f[i], f[(i + 1) % 4]) for i in range(4)]
            cross = [e for e in fe if mask >> e & 1]
            if len(cross) == 2:
                adj[cross[0]].append(cross[1]); adj[cross[1]].append(cross[0])
            elif len(cross) == 4:
                for i in range(4):
                    if below[f[i]]:                      # cut this below-corner off
                        e0, e1 = fe[i - 1], fe[i]        # its two face edges
                        adj[e0].append(e1); adj[e1].append(e0)
        seen, out = set(), []
        for start in sorted(adj):
            if start in seen:
                continue
            assert len(adj[start]) == 2
            loop, prev, cur = [start], start, min(adj[start])
            while cur != start:
                loop.append(cur)
                a, b = adj[cur]
                prev, cur = cur, (b if a == prev else a)
            seen.update(loop)
            p = mid[loop]
            normal = np.zeros(3)
            for i in range(len(loop)):                   # Newell
                a, b = p[i], p[(i + 1) % len(loop)]
                normal += np.cross(a, b)
            ref = np.zeros(3)
            for e in loop:
                a, b = EDGES[e]
                ref += (pos[a] - pos[b]) if below[a] else (pos[b] - pos[a])
            if normal @ ref < 0:
                loop = [loop[0]] + loop[:0:-1]
            out += _triangulate(loop)
        tris.append(out)
    width = max(len(t) for t in tris)
    tri_table = np.full((256, width), -1, np.int8)
    for c, t in enumerate(tris):
        tri_table[c, :len(t)] = t
    return edge_table, tri_table


@functools.lru_cache(maxsize=None)
def tables():
    """(edge_table (256,) int32, tri_table (256, 16) int8): the classic table (nsr/mc_table.py);
    the edge masks follow from the corner states."""
    from .mc_table import triangle_table
    return _build_tables()[0], triangle_table()


# ------------------------------------------------------------------------------------------------
# mcubes.marching_cubes
# ------------------------------------------------------------------------------------------------
@torch.no_grad()
def marching_cubes(volume, isovalue=0.0):
    """volume (X,Y,Z) float on the device -> (verts (N,3) float64 in index units, faces (M,3) int64).
    Vertex and face ORDER follow the serial x-major sweep (see the module docstring)."""
    dev = volume.device
    v = volume.to(torch.float64)
    X, Y, Z = v.shape
    assert min(X, Y, Z) >= 2
    et, tt = tables()
    edge_table = torch.from_numpy(et).to(dev)
    tri_table = torch.from_numpy(tt.astype(np.int64)).to(dev)
    if v.is_cuda:
        from .. import ops
        cube = ops.mc_cube_index(v.contiguous(), isovalue)         # one configuration byte per cube
    else:
        below = v <= isovalue                                      # marchingcubes.h: `<=`
        cube = torch.zeros((X - 1, Y - 1, Z - 1), dtype=torch.int64, device=dev)
        for m, (dx, dy, dz) in enumerate(CORNERS):
            cube += below[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].to(torch.int64) << m
    active = torch.nonzero((cube != 0) & (cube != 255))           # lexicographic = sweep order
    na = active.shape[0]
    if na == 0:
        return (torch.zeros((0, 3), dtype=torch.float64, device=dev),
                torch.zeros((0, 3), dtype=torch.int64, device=dev))
    ci, cj, ck = active[:, 0], active[:, 1], active[:, 2]
    cidx = cube[ci, cj, ck].to(torch.int64)
    emask = edge_table[cidx].to(torch.int64)
    # which of its 12 edges does each active cube CREATE (first cube of the sweep on that edge)?
    own = {6: None, 5: None, 10: None,
           0: (cj == 0) & (ck == 0), 1: ck == 0, 2: ck == 0, 3: (ci == 0) & (ck == 0),
           4: cj == 0, 7: ci == 0, 8: (ci == 0) & (cj == 0), 9: cj == 0, 11: ci == 0}
    created = torch.zeros((na, 12), dtype=torch.bool, device=dev)
    for e in range(12):
        flag = (emask >> e & 1).bool()
        created[:, e] = flag if own[e] is None else (flag & own[e])
    order = torch.tensor(CREATE_ORDER, device=dev)
    created_o = created[:, order]                                  # columns in creation order
    rank_o = torch.cumsum(created_o.to(torch.int64), 1) - created_o.to(torch.int64)
    n_created = created_o.sum(1)
    vbase = torch.cumsum(n_created, 0) - n_created
    vid_o = vbase[:, None] + rank_o                                # vertex id per (cube, slot)
    n_verts = int(n_created.sum())
    # vertex positions
    verts = torch.empty((n_verts, 3), dtype=torch.float64, device=dev)
    for slot, e in enumerate(CREATE_ORDER):
        sel = created_o[:, slot]
        if not bool(sel.any()):
            continue
        a, b = EDGES[e]
        base = active[sel]
        pa = base + torch.tensor(CORNERS[a], device=dev)
        pb = base + torch.tensor(CORNERS[b], device=dev)
        fa, fb = v[pa[:, 0], pa[:, 1], pa[:, 2]], v[pb[:, 0], pb[:, 1], pb[:, 2]]
        pa, pb = pa.to(torch.float64), pb.to(torch.float64)
        t = (isovalue - fa) / (fb - fa)
        p = (pb - pa) * t[:, None] + pa                            # (x2 - x1) * (iso - f1) / (f2 - f1) + x1
        p = torch.where((fa == fb)[:, None], (pa + pb) / 2, p)
        verts[vid_o[sel, slot]] = p
    # per grid edge: the id of its vertex (three dense id volumes, one per axis)
    eid = [torch.full((X, Y, Z), -1, dtype=torch.int32, device=dev) for _ in range(3)]
    for slot, e in enumerate(CREATE_ORDER):
        sel = created_o[:, slot]
        if not bool(sel.any()):
            continue
        axis, off = EDGE_AXIS_OFF[e]
        b = active[sel] + torch.tensor(off, device=dev)
        eid[axis][b[:, 0], b[:, 1], b[:, 2]] = vid_o[sel, slot].to(torch.int32)
    # triangles: cube by cube, table order
    tri = tri_table[cidx]                                          # (na, 3T), -1 padded
    ntri = (tri >= 0).sum(1) // 3
    fbase = torch.cumsum(ntri, 0) - ntri
    n_faces = int(ntri.sum())
    faces = torch.empty((n_faces, 3), dtype=torch.int64, device=dev)
    T = tri.shape[1] // 3
    cube_vid = torch.full((na, 12), -1, dtype=torch.int64, device=dev)
    for e in range(12):
        axis, off = EDGE_AXIS_OFF[e]
        b = active + torch.tensor(off, device=dev)
        cube_vid[:, e] = eid[axis][b[:, 0], b[:, 1], b[:, 2]].to(torch.int64)
    for t in range(T):
        sel = ntri > t
        if not bool(sel.any()):
            break
        e3 = tri[sel][:, 3 * t:3 * t + 3]
        faces[fbase[sel] + t] = torch.gather(cube_vid[sel], 1, e3)
    return verts, faces


# ------------------------------------------------------------------------------------------------
# mcubes.smooth (constrained)
# ------------------------------------------------------------------------------------------------
def _line_distance(other, axis, cap):
    """Per voxel, the distance ALONG `axis` to the nearest voxel where `other` is True (int32,
    capped at `cap`): two running-maximum sweeps over the index of the last such voxel."""
    n = other.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = n
    idx = torch.arange(n, device=other.device, dtype=torch.int32).view(shape)
    far = -(cap + n)
    last = torch.cummax(torch.where(other, idx, torch.full_like(idx, far).expand_as(other)), axis).values
    d_fwd = idx - last
    ridx = (n - 1) - idx
    nxt = torch.cummax(torch.where(other, ridx, torch.full_like(idx, far).expand_as(other)).flip(axis),
                       axis).values.flip(axis)
    d_bwd = ridx - nxt
    return torch.minimum(d_fwd, d_bwd).clamp(max=cap)


def _min_plus_pass(d2, axis, radius):
    """out[i] = min_{|s| <= radius} d2[i + s] + s^2 along `axis` (one sweep of the separable exact
    Euclidean transform, restricted to the radius that matters)."""
    out = d2.clone()
    n = d2.shape[axis]
    for s_ in range(1, radius + 1):
        if s_ >= n:
            break
        for sgn in (1, -1):
            sh = sgn * s_
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            if sh > 0:
                src[axis], dst[axis] = slice(sh, n), slice(0, n - sh)
            else:
                src[axis], dst[axis] = slice(0, n + sh), slice(-sh, n)
            tgt = out[tuple(dst)]
            tgt.copy_(torch.minimum(tgt, d2[tuple(src)] + s_ * s_))
    return out


def _band_tables(radius, band_radius):
    """Host tables over d2 = min(squared distance to the nearest voxel of the other class, (R+1)^2)
    for csrc/mesh_volume.hip: the float64 values signed_distance_band's last lines produce (sqrt,
    far-field value, half-voxel shift, sign; row 0 = inside voxels) and |value| <= band_radius."""
    R = int(math.ceil(radius))
    k = np.arange((R + 1) * (R + 1) + 1, dtype=np.float64)
    d = np.sqrt(k)
    d = np.where(d > radius, float(radius) + 1.0, d)
    inside = d - 0.5
    table = np.stack([inside, -(d - 0.5)])
    band = (np.abs(inside) <= band_radius).astype(np.uint8) if band_radius is not None else np.zeros(k.shape, np.uint8)
    return R, table, band


@torch.no_grad()
def signed_distance_band_device(binary, radius=5.0, band_radius=None):
    """signed_distance_band on the library's kernels (dsu_volume_band_distance): the same integers
    through three passes over two bytes per voxel, then the values through the host's table.
    Returns (dist f64, band bool = |dist| <= band_radius, or None)."""
    from .. import ops
    R, table, band = _band_tables(radius, band_radius)
    dev = binary.device
    dist, bm = ops.volume_band_distance(binary.bool(), R, torch.from_numpy(table).to(dev),
                                        torch.from_numpy(band).to(dev))
    return dist, (bm if band_radius is not None else None)


@torch.no_grad()
def signed_distance_band(binary, radius=5.0):
    """scipy.ndimage.distance_transform_edt on both classes, exact wherever the other class is
    within `radius` voxels: d = +(distance to the nearest False voxel) - 0.5 inside,
    -(distance to the nearest True voxel) + 0.5 outside; farther voxels get +-(radius + 0.5).
    Separable squared-distance transform in integers: nearest other-class voxel along z, then
    min-plus sweeps over |dy| <= R and |dx| <= R (a nearest voxel within R has every coordinate
    offset within R).  Device volumes: csrc/mesh_volume.hip (bit-identical values); this tensor
    program is the host form and the tests' comparison (`signed_distance_band_tensor_program`)."""
    if binary.is_cuda and math.ceil(radius) <= 8 and binary.shape[2] <= 4096:
        return signed_distance_band_device(binary, radius)[0]
    return signed_distance_band_tensor_program(binary, radius)


@torch.no_grad()
def signed_distance_band_tensor_program(binary, radius=5.0):
    b = binary.bool()
    R = int(math.ceil(radius))
    cap2 = (R + 1) * (R + 1)

    def dist2_to(other):
        dz = _line_distance(other, 2, R + 1)
        d2 = (dz * dz).clamp(max=cap2)
        d2 = _min_plus_pass(d2, 1, R).clamp(max=cap2)
        return _min_plus_pass(d2, 0, R).clamp(max=cap2)

    d_in = torch.sqrt(dist2_to(~b).to(torch.float64))          # True voxels: nearest False
    d_out = torch.sqrt(dist2_to(b).to(torch.float64))          # False voxels: nearest True
    big = float(radius) + 1.0
    d_in = torch.where(d_in > radius, torch.full_like(d_in, big), d_in)
    d_out = torch.where(d_out > radius, torch.full_like(d_out, big), d_out)
    return torch.where(b, d_in - 0.5, -(d_out - 0.5))


# default bounds of the brick layout when the distinct distances are known up front: "coded" (one
# byte per voxel into a table) or "stored" (the distance as a double); tools/smooth_probe.py measures both
BRICK_BOUNDS = "coded"


@torch.no_grad()
def smooth_constrained(binary, max_iters=250, rel_tol=1e-6, band_radius=4.0, weight=0.5, layout=None):
    """mcubes.smooth for volumes of at most 512^3 voxels (see the module docstring).  Returns the
    float64 volume PyMCubes returns — the signed distance with the band replaced by the solution —
    except that distances beyond the band are capped at +-(band_radius + 1.5): they never reach the
    zero level set, and an exact far-field transform of 2 x 512^3 voxels would cost more than
    everything else in the export.

    The unknowns are the band voxels only (a few million of the 134 M).  layout: "bricks" (the
    default on a device tensor: the band compacted in 8^3 bricks, csrc/mesh_smooth.hip) or "slots"
    (compacted voxel by voxel in x-major order with six neighbour-slot arrays; F and F^T are
    gathers over them: host tensors, and the comparison of the brick layout's tests)."""
    b = binary.bool()
    values = None
    if b.is_cuda and math.ceil(band_radius + 1.0) <= 8 and b.shape[2] <= 4096:
        dist, band = signed_distance_band_device(b, band_radius + 1.0, band_radius)
        # every distance the transform can produce: the byte-coded bounds need no pass to find them
        values = torch.from_numpy(np.unique(_band_tables(band_radius + 1.0, band_radius)[1]))
    else:
        dist = signed_distance_band(b, band_radius + 1.0)
        band = dist.abs() <= band_radius
    return smooth_band(dist, band, max_iters, rel_tol, weight, layout, values)[0]


def _slot_layout(dist, band):
    """The band compacted voxel by voxel: (flat, nbr_slots, x, lower, upper), or None when the band
    is empty.  flat: x-major linear index of the band voxels; nbr_slots: six (nv,) int32 tensors;
    x: the band's distances; lower / upper: PyMCubes' bounds."""
    pos = torch.nonzero(band)
    nv = pos.shape[0]
    if nv == 0:
        return None
    shp = dist.shape
    dev = dist.device
    # x-major linear index of the band voxels (the order nonzero / mask indexing walk them in)
    flat = (pos[:, 0] * shp[1] + pos[:, 1]) * shp[2] + pos[:, 2]
    slot = torch.full(shp, -1, dtype=torch.int32, device=dev)
    slot.view(-1)[flat] = torch.arange(nv, device=dev, dtype=torch.int32)
    shape = torch.tensor(shp, device=dev)
    nbr_slots = []                          # -x, +x, -y, +y, -z, +z : slot or -1
    for a in range(3):
        for sgn in (-1, 1):
            q = pos.clone()
            q[:, a] += sgn
            ok = (q[:, a] >= 0) & (q[:, a] < shape[a])
            q[:, a].clamp_(0, int(shape[a]) - 1)
            n = slot[q[:, 0], q[:, 1], q[:, 2]]
            nbr_slots.append(torch.where(ok, n, torch.full_like(n, -1)))
    del slot
    x = dist.reshape(-1)[flat]
    # PyMCubes' bounds: own-side bound = the initial distance, 0 next to the surface
    ninf, pinf = float("-inf"), float("inf")
    lower = torch.where(x > 0, x, torch.full_like(x, ninf))
    upper = torch.where(x < 0, x, torch.full_like(x, pinf))
    lower = torch.where(lower.abs() < 1, torch.zeros_like(x), lower)
    upper = torch.where(upper.abs() < 1, torch.zeros_like(x), upper)
    return flat, nbr_slots, x, lower, upper


def _bricks_supported(shape):
    return len(shape) == 3 and min(shape) >= 1 and \
        -(-shape[0] // 8) * -(-shape[1] // 8) * -(-shape[2] // 8) < 2 ** 22


@torch.no_grad()
def smooth_band(dist, band, max_iters=250, rel_tol=1e-6, weight=0.5, layout=None, values=None,
                bounds=None, direct=False):
    """The iteration of smooth_constrained on the voxels `band` (bool) of `dist` (f64, written in
    place).  Returns (dist, iterations run).  values: the distinct distances of the band when the
    caller knows them (ascending f64); bounds "coded" / "stored" and direct: the brick layout's
    measured alternatives (ops.smooth_bricks_build, ops.smooth_bricks_iterate)."""
    dev = dist.device
    if layout is None:
        layout = "bricks" if dist.is_cuda and _bricks_supported(dist.shape) else "slots"
    if layout not in ("bricks", "slots"):
        raise ValueError(f"layout {layout!r}: 'bricks' or 'slots'")
    check_each = 10
    cum_rel_tol = 1 - (1 - rel_tol) ** check_each

    def run(energy, iterate):
        energy_now = float(energy())
        done = 0
        while done < max_iters:
            step = min(check_each, max_iters - done)
            iterate(step)
            done += step
            if step == check_each:
                energy_before = energy_now
                energy_now = float(energy())
                if energy_before <= 0 or (energy_before - energy_now) / energy_before < cum_rel_tol:
                    break
        return done

    if layout == "bricks":
        from .. import ops
        if not dist.is_cuda or not _bricks_supported(dist.shape):
            raise ValueError("the brick layout needs a device volume of fewer than 2^22 bricks")
        if bounds is None:
            bounds = BRICK_BOUNDS if values is not None else "stored"
        if bounds == "coded" and values is None:
            values = torch.unique(dist[band])
        bricks = ops.smooth_bricks_build(band, dist, values if bounds == "coded" else None)
        if bricks is None:
            return dist, 0
        done = run(lambda: ops.smooth_bricks_energy(bricks),
                   lambda step: ops.smooth_bricks_iterate(bricks, weight, step, direct))
        ops.smooth_bricks_scatter(bricks, dist)     # (dist is the caller's own volume: written in place)
        return dist, done
    slots = _slot_layout(dist, band)
    if slots is None:
        return dist, 0
    flat, nbr_slots, x, lower, upper = slots
    nv = x.shape[0]
    if dist.is_cuda:
        # the iteration itself: csrc/mesh_smooth.hip (one pass over the band per iteration)
        from .. import ops
        nbr_t = torch.stack(nbr_slots).contiguous()
        lower, upper = lower.contiguous(), upper.contiguous()
        x = x.contiguous()
        ybuf = torch.empty(3 * nv, dtype=torch.float64, device=dev)
        done = run(lambda: ops.smooth_energy(nbr_t, x, ybuf),
                   lambda step: ops.smooth_iterate(nbr_t, lower, upper, x, ybuf, weight, step))
        dist.view(-1)[flat] = x             # (dist is this call's own volume: written in place)
        return dist, done
    # host tensors (CPU tests of the restatement): the same iteration as tensor programs
    nbr = [[nbr_slots[2 * a + k].clamp(min=0).long() for k in range(2)] for a in range(3)]
    has = [[(nbr_slots[2 * a + k] >= 0).to(torch.float64) for k in range(2)] for a in range(3)]
    cdiag = [-2.0 + (1 - has[a][0]) + (1 - has[a][1]) for a in range(3)]

    def apply_q(v):
        out = torch.zeros_like(v)
        for a in range(3):
            y = cdiag[a] * v + v[nbr[a][0]] * has[a][0] + v[nbr[a][1]] * has[a][1]        # F rows
            out += cdiag[a] * y + y[nbr[a][0]] * has[a][0] + y[nbr[a][1]] * has[a][1]    # F^T
        return out

    diag = torch.zeros_like(x)
    for a in range(3):
        diag += cdiag[a] ** 2 + has[a][0] + has[a][1]
    inv_d = 1.0 / diag
    energy_now = float((x * apply_q(x)).sum()) / 2
    done = 0
    for i in range(max_iters):
        done = i + 1
        x1 = -inv_d * (apply_q(x) - diag * x)               # -D^-1 R x
        x = weight * x1 + (1 - weight) * x
        x = torch.minimum(torch.maximum(x, lower), upper)
        if (i + 1) % check_each == 0:
            energy_before = energy_now
            energy_now = float((x * apply_q(x)).sum()) / 2
            if energy_before <= 0 or (energy_before - energy_now) / energy_before < cum_rel_tol:
                break
    out = dist.clone()
    out[band] = x
    return out, done


# ------------------------------------------------------------------------------------------------
# cv2.resize(..., interpolation=cv2.INTER_CUBIC) for a uint8 single-channel image
# ------------------------------------------------------------------------------------------------
def resize_cubic_u8(img, out_hw):
    """OpenCV bicubic (A = -0.75): source coordinate (dst + 0.5) * scale - 0.5, 4 taps per axis,
    replicated border, result rounded and saturated to uint8.  img (H,W) uint8 tensor."""
    A = -0.75

    def weights(t):
        w0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
        w1 = ((A + 2) * t - (A + 3)) * t * t + 1
        w2 = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1
        return torch.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], -1)

    def axis_tables(n_in, n_out, dev):
        s = n_in / n_out
        f = (torch.arange(n_out, dtype=torch.float64, device=dev) + 0.5) * s - 0.5
        i0 = torch.floor(f)
        idx = (i0[:, None] + torch.arange(-1, 3, device=dev)).clamp(0, n_in - 1).long()
        return idx, weights(f - i0)

    x = img.to(torch.float64)
    H, W = x.shape
    oh, ow = out_hw
    iy, wy = axis_tables(H, oh, x.device)
    ix, wx = axis_tables(W, ow, x.device)
    rows = (x[iy] * wy[:, :, None]).sum(1)                    # (oh, W)
    out = (rows[:, ix] * wx[None]).sum(-1)                    # (oh, ow)
    return torch.floor(out + 0.5).clamp(0, 255).to(torch.uint8)


# ------------------------------------------------------------------------------------------------
# MarchingCubeHelper / isosurface / export
# ------------------------------------------------------------------------------------------------
def _remesh_host(v, f, face_count, boundary_weight, keep_manifold, quadrics=None):
    import ctypes as C
    from .. import _lib, ops
    ov, of = np.empty_like(v), np.empty_like(f)
    nv, nf = C.c_int64(0), C.c_int64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    flags = 0 if keep_manifold else 1
    if quadrics is None:
        ops.check(_lib.lib().dsu_mesh_decimate_quadric(
            p(v), v.shape[0], p(f), f.shape[0], int(face_count), float(boundary_weight), flags,
            p(ov), C.byref(nv), p(of), C.byref(nf)), "dsu_mesh_decimate_quadric")
    else:
        ops.check(_lib.lib().dsu_mesh_decimate_quadric_q(
            p(v), v.shape[0], p(f), f.shape[0], int(face_count), float(boundary_weight), flags,
            p(quadrics), p(ov), C.byref(nv), p(of), C.byref(nf)), "dsu_mesh_decimate_quadric_q")
    return ov[:nv.value].copy(), of[:nf.value].astype(np.int64)


# the device rounds stop at PARALLEL_STOP x face_count and never go below PARALLEL_FLOOR x
# face_count; the serial queue (seeded with the accumulated quadrics) takes the last stretch and
# lands on the exact count
PARALLEL_STOP, PARALLEL_FLOOR, PARALLEL_MIN_FACES = 1.25, 1.0, 20000
last_remesh_stats = {}


def _decimate_parallel(verts, faces, stop_faces, floor_faces, boundary_weight, keep_manifold, max_rounds, workspace):
    import ctypes as C
    from .. import _lib, ops
    dev = verts.device
    v = verts.detach().to(torch.float64).contiguous().clone()
    f = faces.detach().to(dev, torch.int32).contiguous().clone()
    nv, n_faces = v.shape[0], int(f.shape[0])
    lib = _lib.lib()
    ws_bytes = int(lib.dsu_mesh_decimate_parallel_workspace_bytes(nv, n_faces))
    if ws_bytes < 0:
        raise ops.DsuError("dsu_mesh_decimate_parallel_workspace_bytes: unsupported size")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if workspace is None else workspace
    assert ws.dtype == torch.uint8 and ws.device == dev and ws.dim() == 1 and ws.is_contiguous(), \
        "workspace: a contiguous 1-D uint8 tensor on the device of verts"
    quad = torch.empty(nv, 10, dtype=torch.float64, device=dev)
    out_nf = C.c_int64(0)
    stats = (C.c_int32 * 3)()
    ops.check(lib.dsu_mesh_decimate_parallel(
        v.data_ptr(), nv, f.data_ptr(), n_faces, int(stop_faces), int(floor_faces), float(boundary_weight),
        0 if keep_manifold else 1, int(max_rounds), quad.data_ptr(), C.byref(out_nf), stats, ws.data_ptr(),
        int(ws.numel()), torch.cuda.current_stream(dev).cuda_stream), "dsu_mesh_decimate_parallel")
    return v, f[:out_nf.value], quad, list(stats)


def decimate_parallel(verts, faces, stop_faces, floor_faces, boundary_weight=1.0, keep_manifold=True,
                      max_rounds=200, workspace=None):
    """The device rounds alone (`dsu_mesh_decimate_parallel`) on device tensors of any size:
    -> (verts (n_verts,3) float64, live faces (m,3) int32, quadrics (n_verts,10) float64, stats
    (3,) int32 = rounds, collapses, rejected), device tensors over all n_verts in the C ABI's
    indexing (collapsed vertices keep their rows; no live face names them).  The inputs are not
    modified.  `workspace`: a uint8 device tensor to use instead of a fresh allocation."""
    v, f, quad, stats = _decimate_parallel(verts, faces, stop_faces, floor_faces, boundary_weight, keep_manifold,
                                           max_rounds, workspace)
    return v, f, quad, torch.tensor(stats, dtype=torch.int32, device=v.device)


def remesh(verts, faces, face_count, boundary_weight=1.0, keep_manifold=True):
    """mesh_utils.py:10-22 (`trimesh.simplify_quadratic_decimation(face_count)` -> Open3D's quadric
    decimation): (N,3) float verts, (M,3) int faces -> (verts float64, faces int64) numpy arrays,
    collapsed until the face count is <= face_count (or no admissible collapse is left).
    Device tensors (the export path: 1-3 M triangles from the 512^3 marching cubes): rounds of
    independent collapses on the GPU down to 1.25 x face_count (`decimate_parallel`), then
    the serial queue for the last stretch.  Host arrays: the serial queue alone
    (`dsu_mesh_decimate_quadric`; restated from the published method — trimesh / Open3D are absent:
    unpinned, see the kernel files' headers for what is kept and what is added)."""
    on_device = torch.is_tensor(verts) and verts.is_cuda
    n_faces = int(faces.shape[0])
    if not on_device or n_faces <= max(PARALLEL_MIN_FACES, PARALLEL_STOP * face_count):
        v = np.ascontiguousarray(np.asarray(verts.detach().cpu() if torch.is_tensor(verts) else verts,
                                            dtype=np.float64))
        f = np.ascontiguousarray(np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces)
                                 .astype(np.int32))
        return _remesh_host(v, f, face_count, boundary_weight, keep_manifold)
    v, f, quad, stats = _decimate_parallel(verts, faces, int(PARALLEL_STOP * face_count),
                                           int(PARALLEL_FLOOR * face_count), boundary_weight, keep_manifold, 200, None)
    # only the vertices still in use travel to the host
    used, inv = torch.unique(f.reshape(-1).long(), return_inverse=True)
    last_remesh_stats.update(input_faces=n_faces, device_faces=int(f.shape[0]), rounds=int(stats[0]),
                             collapses=int(stats[1]), rejected=int(stats[2]))
    hv = np.ascontiguousarray(v[used].cpu().numpy())
    hq = np.ascontiguousarray(quad[used].cpu().numpy())
    hf = np.ascontiguousarray(inv.reshape(-1, 3).to(torch.int32).cpu().numpy())
    return _remesh_host(hv, hf, face_count, boundary_weight, keep_manifold, quadrics=hq)


class MarchingCubeHelper:
    """geometry.py:33-69; `face_count` switches the fine stage's `remesh` on (geometry.py:63-64)."""

    def __init__(self, resolution, face_count=None):
        self.resolution = int(resolution)
        self.face_count = face_count

    @torch.no_grad()
    def __call__(self, level, threshold=0.0, front_mask=None, fine_stage=False):
        res = self.resolution
        level = level.float().view(res, res, res)
        binary = level <= 0
        if front_mask is not None:
            fm = resize_cubic_u8(front_mask.to(level.device), (res, res))
            binary = binary & (fm[:, None, :].expand(res, res, res) > 127)       # np.tile(front_mask[:, None, :])
        value = smooth_constrained(binary)
        verts, faces = marching_cubes(value, threshold)
        verts = verts / (res - 1.0)
        if fine_stage and self.face_count and faces.shape[0] > int(self.face_count):
            v, f = remesh(verts, faces, int(self.face_count))
            verts = torch.from_numpy(v).to(verts.device)
            faces = torch.from_numpy(f).to(faces.device)
        return {"verts": verts, "faces": faces, "binary": binary}


def scale_anything(x, src, dst):                    # instant_nsr/models/utils.py:101-106
    return (x - src[0]) / (src[1] - src[0]) * (dst[1] - dst[0]) + dst[0]


def crop_front_mask(front_mask, vmin, vmax):
    """geometry.py:93-98: the fine pass crops the (rotated) front mask to the fine box in x and z."""
    size = front_mask.shape[0] / 2
    x_min, x_max = int(math.floor(vmin[0] * size + size)), int(math.ceil(vmax[0] * size + size))
    z_min, z_max = int(math.floor(vmin[2] * size + size)), int(math.ceil(vmax[2] * size + size))
    return front_mask[x_min:x_max, z_min:z_max]


@torch.no_grad()
def isosurface(model, front_mask=None, resolution=None, face_count=None):
    """BaseImplicitGeometry.isosurface (geometry.py:108-117) on the device: coarse pass over the
    whole box, bounding box of the coarse MESH's vertices padded by 10 % and clamped, fine pass in
    it with the front mask (and, with `face_count`, the fine stage's remesh).  Returns the fine
    mesh {verts (N,3) f64 world, faces (M,3) i64} plus the two level volumes."""
    r = float(model.config.radius)
    res = resolution or model.config.geometry.isosurface.resolution
    thr = float(model.config.geometry.isosurface.threshold)
    helper = MarchingCubeHelper(res, face_count)

    def one(vmin, vmax, fm, fine_stage=False):
        level = model.isosurface_levels(vmin, vmax, res)
        mesh = helper(level, thr, fm, fine_stage)
        v = mesh["verts"]
        mesh["verts"] = torch.stack([scale_anything(v[:, a], (0, 1), (vmin[a], vmax[a])) for a in range(3)], -1)
        mesh["level"] = level
        return mesh

    coarse = one((-r, -r, -r), (r, r, r), None)
    if coarse["verts"].shape[0] == 0:
        return coarse, coarse
    vmin, vmax = coarse["verts"].amin(0), coarse["verts"].amax(0)
    vmin_ = (vmin - (vmax - vmin) * 0.1).clamp(-r, r).tolist()
    vmax_ = (vmax + (vmax - vmin) * 0.1).clamp(-r, r).tolist()
    fm = None if front_mask is None else crop_front_mask(front_mask, vmin_, vmax_)
    fine = one(vmin_, vmax_, fm, True)
    fine["vmin"], fine["vmax"] = vmin_, vmax_
    return fine, coarse


@torch.no_grad()
def vertex_colors(model, verts, chunk=2097152):
    """NeuSModel.export's colour pass (neus.py:222-236): texture(feature, -normal, normal)."""
    import torch.nn.functional as F
    out = []
    for i in range(0, verts.shape[0], chunk):
        p = verts[i:i + chunk].float()
        _, grad, feat = model.geometry(p, with_grad=True, with_feature=True)
        normal = F.normalize(grad, p=2, dim=-1)
        out.append(model.texture(feat, -normal, normal))
    return torch.cat(out, 0) if out else torch.zeros((0, 3), device=verts.device)


def field_colours(model):
    """The texture field as a function of position, for nsr/uv.bake_field: (N,3) device points ->
    (N,3) colours, evaluated as vertex_colors evaluates the vertices."""
    return lambda p: vertex_colors(model, p)


# ------------------------------------------------------------------------------------------------
# save_mesh's host-side geometry steps that need no ray caster (mesh_utils.py:25-93)
# ------------------------------------------------------------------------------------------------
def laplacian_smooth_implicit(verts, faces, lamb=2.0, iterations=5, volume_constraint=True):
    """trimesh.smoothing.filter_laplacian(mesh, lamb, iterations, implicit_time_integration=True)
    as save_mesh calls it (mesh_utils.py:44-45), restated from trimesh's published algorithm
    (trimesh is absent here: unpinned): umbrella operator L with equal weights (row i = 1/deg(i) on
    the neighbours of i), every iteration solves (I + lamb (I - L)) V' = V (sparse LU, factorised
    once), then rescales V' so that the enclosed volume stays what it was before the filter.
    verts (N,3) float64, faces (M,3) int -> (N,3) float64."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    v = np.array(verts, np.float64)
    f = np.asarray(faces, np.int64)
    n = v.shape[0]
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = np.unique(np.concatenate([e, e[:, ::-1]], 0), axis=0)              # undirected, unique
    deg = np.bincount(e[:, 0], minlength=n).astype(np.float64)
    w = 1.0 / deg[e[:, 0]]
    L = sp.coo_matrix((w, (e[:, 0], e[:, 1])), shape=(n, n)).tocsc()
    A = (sp.identity(n, format="csc") + lamb * (sp.identity(n, format="csc") - L)).tocsc()
    lu = splu(A)

    def volume(p):
        a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)

    vol0 = volume(v) if volume_constraint else 0.0
    for _ in range(int(iterations)):
        v = lu.solve(v)
        if volume_constraint:
            vol = volume(v)
            if vol != 0.0 and vol0 / vol > 0.0:
                v *= (vol0 / vol) ** (1.0 / 3.0)
    return v


def laplacian_smooth_implicit_device(verts, faces, lamb=2.0, iterations=5, volume_constraint=True,
                                     sweeps=96):
    """The same filter on DEVICE tensors (verts (N,3) float64, faces (M,3) int64): neighbour lists
    by a sort of the directed edges, every implicit step by Jacobi sweeps of the library
    (`dsu_umbrella_implicit_solve`: the matrix is diagonally dominant, 96 sweeps contract the error
    by (2/3)^96 = 1e-17), volume rescaling with device reductions.  Returns (N,3) float64."""
    from .. import _lib, ops
    dev = verts.device
    v = verts.to(torch.float64).contiguous().clone()
    f = faces.to(torch.int64)
    n = v.shape[0]
    if n == 0 or f.shape[0] == 0:
        return v
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = torch.cat([e, e.flip(1)], 0)
    key = torch.unique(e[:, 0] * n + e[:, 1])                          # sorted: row-major, columns ascending
    rows = torch.div(key, n, rounding_mode="floor")
    cols = (key - rows * n).to(torch.int32).contiguous()
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    off = off.to(torch.int32).contiguous()
    tmp = torch.empty_like(v)

    def volume(p):
        a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        return (a * torch.linalg.cross(b, c)).sum() / 6.0

    vol0 = volume(v) if volume_constraint else None
    lib = _lib.lib()
    for _ in range(int(iterations)):
        rhs = v.clone()
        ops.check(lib.dsu_umbrella_implicit_solve(off.data_ptr(), cols.data_ptr(), n, float(lamb),
                                                  rhs.data_ptr(), v.data_ptr(), tmp.data_ptr(), int(sweeps),
                                                  torch.cuda.current_stream(dev).cuda_stream),
                  "dsu_umbrella_implicit_solve")
        if volume_constraint:
            vol = volume(v)
            ratio = vol0 / vol
            # (vol0 / vol) ** (1/3) where the ratio is positive and finite, 1 otherwise: no host read
            scale = torch.where(torch.isfinite(ratio) & (ratio > 0), ratio.abs() ** (1.0 / 3.0),
                                torch.ones_like(ratio))
            v = v * scale
    return v


def shear_transformation_device(v):
    """shear_transformation on a device tensor (N,3) float64 (the 2x2 SVD on the host: four numbers)."""
    d = v[:, 1:3]
    nd = d - d.mean(0)
    H = (nd.T @ nd).cpu().numpy()
    vec, val, _ = np.linalg.svd(H)
    vec = vec[:, val.argsort()[::-1]]
    a = -vec[1, 0] / vec[0, 0]
    out = v.clone()
    out[:, 2] += a * v[:, 1]
    return out


def shear_transformation(v):
    """mesh_utils.py:76-93: principal axis of the (y, z) coordinates by SVD of their scatter matrix,
    then z += a * y with a = -v[1,0] / v[0,0] (the figure is sheared upright).  In place on a copy."""
    v = np.array(v, np.float64)
    d = v[:, 1:3]
    nd = d - d.mean(0)
    H = nd.T @ nd
    vec, val, _ = np.linalg.svd(H)
    vec = vec[:, val.argsort()[::-1]]
    a = -vec[1, 0] / vec[0, 0]
    v[:, 2] += a * v[:, 1]
    return v


def nearest_vertex_colors(old_verts, new_verts, colors):
    """mesh_utils.py:50-53 (no colour back-projection): colour of the nearest vertex of the mesh
    before smoothing, for every vertex after it."""
    from scipy.spatial import cKDTree
    _, idx = cKDTree(np.asarray(old_verts, np.float64)).query(np.asarray(new_verts, np.float64), k=1)
    return np.asarray(colors)[idx]


def post_process_mesh(verts, faces, colors=None, ortho_scale=1.35, smoothing=False, shearing=False,
                      color_back_projection=None, thinning=None, return_projection_frame=False):
    """save_mesh (mesh_utils.py:25-73) up to the file write: halve, swap to the front-facing
    convention (x right, y up, z front), [thinning], [Laplacian smoothing], [colour back-projection
    | nearest-vertex colour transfer], [shear], ortho_scale.  Returns (verts (N,3) f64, faces (M,3)
    i64 0-based, colors (N,3) f32 or None) as numpy arrays.  The bracketed steps follow the
    reference's export.* switches (all on in its YAML).  color_back_projection: dict(color_front,
    mask_front, color_back) of (res,res[,3]) uint8 device tensors — the LANCZOS-resized <uid>/mv
    PNGs — runs nsr/mesh_post.color_projection (coloring_utils.py:91-138) on the device instead of
    the nearest-vertex transfer (mesh_utils.py:48-53).  thinning: dict(mask=(res,res) uint8
    character mask, type='double' | 'front' | 'back') runs nsr/thinning.thinning_processing
    (mesh_utils.py:38-39) first; the nearest-vertex colour transfer then reads the thinned
    vertices, as the reference's does.  return_projection_frame: a fourth value, the vertices
    (N,3) f64 as color_projection sees them — after thinning and smoothing, before shear and
    ortho_scale (what nsr/uv.bake_drawings projects the drawings from)."""
    if torch.is_tensor(verts) and verts.is_cuda and thinning is None and \
            (colors is None or color_back_projection is not None):
        # everything stays on the device (the export path: smoothing by Jacobi sweeps, colour
        # back-projection, shear); host arrays only at the very end, for the OBJ writer
        vd = verts.detach().to(torch.float64) * 0.5
        out = torch.stack([vd[:, 0], vd[:, 2], -vd[:, 1]], -1)
        fd = faces.detach().to(verts.device, torch.int64)
        c = None
        if smoothing and fd.shape[0]:
            out = laplacian_smooth_implicit_device(out, fd, lamb=2.0, iterations=5)
        if color_back_projection is not None and fd.shape[0]:
            from .mesh_post import color_projection
            cbp = color_back_projection
            c = color_projection(out.contiguous(), fd, cbp["color_front"], cbp["mask_front"],
                                 cbp["color_back"], res=cbp["color_front"].shape[0]).float().cpu().numpy()
        frame = out
        if shearing and out.shape[0]:
            out = shear_transformation_device(out)
        res = ((out * ortho_scale).cpu().numpy(), fd.cpu().numpy(), c)
        return res + (frame.cpu().numpy(),) if return_projection_frame else res
    v = verts.detach().cpu().numpy().astype(np.float64) * 0.5
    old = np.zeros_like(v)
    old[:, 0], old[:, 1], old[:, 2] = v[:, 0], v[:, 2], -v[:, 1]
    fz = faces.detach().cpu().numpy().astype(np.int64)
    c = None if colors is None else colors.detach().float().cpu().numpy()
    if thinning is not None and len(fz):
        from .thinning import thinning_processing
        mask = thinning["mask"]
        mask = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
        old = thinning_processing(old, fz, mask, thinning.get("type", "double"),
                                  device=thinning.get("device", verts.device if verts.is_cuda else None))
    out = old
    if smoothing and len(fz):
        out = laplacian_smooth_implicit(old, fz, lamb=2.0, iterations=5)
        if c is not None and color_back_projection is None:
            c = nearest_vertex_colors(old, out, c)
    if color_back_projection is not None and len(fz):
        from .mesh_post import color_projection
        cbp = color_back_projection
        dev = cbp["color_front"].device
        c = color_projection(torch.from_numpy(np.ascontiguousarray(out)).to(dev),
                             torch.from_numpy(fz).to(dev), cbp["color_front"], cbp["mask_front"],
                             cbp["color_back"], res=cbp["color_front"].shape[0]).float().cpu().numpy()
    frame = out
    if shearing and len(out):
        out = shear_transformation(out)
    res = (out * ortho_scale, fz, c)
    return res + (np.asarray(frame, np.float64),) if return_projection_frame else res


def write_obj(path, verts, faces, colors=None):
    """trimesh's OBJ export of a mesh with `vertex_colors` (mesh_utils.py:60-73): `v x y z r g b`,
    faces 1-based."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    lines = []
    if colors is not None:
        for p, q in zip(verts, colors):
            lines.append("v %.8f %.8f %.8f %.6f %.6f %.6f\n" % (p[0], p[1], p[2], q[0], q[1], q[2]))
    else:
        for p in verts:
            lines.append("v %.8f %.8f %.8f\n" % (p[0], p[1], p[2]))
    for t in faces + 1:
        lines.append("f %d %d %d\n" % (t[0], t[1], t[2]))
    with open(path, "w") as fh:
        fh.writelines(lines)
    return path


def write_obj_textured(path, verts, faces, uvs, image, name):
    """The OBJ + MTL + PNG triple of a UV-mapped mesh (coloring_utils.uv_mapping + trimesh's export):
    `<name>.obj` beside `path` with mtllib / usemtl, `v`, `vt` and `f a/a b/b c/c` (one uv per
    vertex), `<name>.mtl` with SimpleMaterial's values (diffuse, ambient, specular 1, glossiness 0)
    and map_Kd, `<name>.png`.  Returns the OBJ's path."""
    from PIL import Image
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    obj = os.path.join(folder, name + ".obj")
    lines = ["mtllib %s.mtl\n" % name, "usemtl %s\n" % name]
    for p in verts:
        lines.append("v %.8f %.8f %.8f\n" % (p[0], p[1], p[2]))
    for t in np.asarray(uvs, np.float64):
        lines.append("vt %.9f %.9f\n" % (t[0], t[1]))
    for t in np.asarray(faces) + 1:
        lines.append("f %d/%d %d/%d %d/%d\n" % (t[0], t[0], t[1], t[1], t[2], t[2]))
    with open(obj, "w") as fh:
        fh.writelines(lines)
    with open(os.path.join(folder, name + ".mtl"), "w") as fh:
        fh.write("newmtl %s\nKa 1.00000000 1.00000000 1.00000000\nKd 1.00000000 1.00000000 1.00000000\n"
                 "Ks 1.00000000 1.00000000 1.00000000\nNs 0.00000000\nmap_Kd %s.png\n" % (name, name))
    Image.fromarray(np.ascontiguousarray(image, np.uint8)).save(os.path.join(folder, name + ".png"))
    return obj


def save_obj(path, verts, faces, colors=None, ortho_scale=1.35, smoothing=False, shearing=False,
             color_back_projection=None, thinning=None, export_uv=False, texture_size=1024,
             texture_source="vertex", texture_field=None, texture_samples=2, texture_seam="none",
             texture_drawing_samples=1, texture_drawing_filter="nearest"):
    """save_mesh (mesh_utils.py:25-73) = post_process_mesh + write_obj, or with export_uv
    (mesh_utils.py:65-67) + uv_mapping and the textured triple named after the file.
    texture_source: "vertex" bakes the vertex colours (the reference's texture); "drawings" (an
    extension, needs export_uv and color_back_projection) projects the front / back drawings of
    color_back_projection into the atlas texel by texel, the vertex colours filling what neither
    drawing sees (nsr/uv.bake_drawings); "field" (an extension, needs export_uv and texture_field)
    evaluates texture_field — a callable from (N,3) f32 points in the frame of `verts` to (N,3)
    colours, field_colours(model) — at texture_samples^2 points per texel (nsr/uv.bake_field), the
    vertex colours staying where nothing can be evaluated.  "drawings" with a texture_field uses the
    field bake as its fallback; "vertex" ignores it.
    texture_seam: "level" (needs texture_source="drawings") levels the fallback texels to the
    drawings where the two meet (nsr/uv.bake_drawings, seam="level"); "none" composes them as they
    are.
    texture_drawing_samples, texture_drawing_filter (other than 1 and "nearest" they need
    texture_source="drawings"): the drawings are read at that many points per texel side (1..8),
    each at its "nearest" pixel or "bilinear", and averaged (nsr/uv.bake_drawings, samples and
    pixel_filter); texture_samples stays the field's alone."""
    if texture_source not in ("vertex", "drawings", "field"):
        raise ValueError("texture_source must be 'vertex', 'drawings' or 'field'")
    if texture_seam not in ("none", "level"):
        raise ValueError("texture_seam must be 'none' or 'level'")
    drawings = texture_source == "drawings"
    if texture_seam == "level" and not drawings:
        raise ValueError("texture_seam='level' needs texture_source='drawings'")
    if isinstance(texture_drawing_samples, bool) or not isinstance(texture_drawing_samples, int) or \
            not 1 <= texture_drawing_samples <= 8:
        raise ValueError("texture_drawing_samples must be an integer 1..8")
    if texture_drawing_filter not in ("nearest", "bilinear"):
        raise ValueError("texture_drawing_filter must be 'nearest' or 'bilinear'")
    if (texture_drawing_samples != 1 or texture_drawing_filter != "nearest") and not drawings:
        raise ValueError("texture_drawing_samples / texture_drawing_filter need texture_source='drawings'")
    if drawings and not (export_uv and color_back_projection is not None):
        raise ValueError("texture_source='drawings' needs export_uv=True and the color_back_projection images")
    if texture_source == "field" and not (export_uv and callable(texture_field)):
        raise ValueError("texture_source='field' needs export_uv=True and a callable texture_field")
    if texture_source != "vertex" and texture_field is not None and not callable(texture_field):
        raise ValueError("texture_field must be callable")
    out, fz, c, *frame = post_process_mesh(verts, faces, colors, ortho_scale, smoothing, shearing,
                                           color_back_projection, thinning, return_projection_frame=drawings)
    if export_uv:
        if c is None:
            raise ValueError("export_uv needs vertex colours")
        from .uv import uv_mapping
        name = os.path.splitext(os.path.basename(path))[0]
        projection = dict(color_back_projection, positions=frame[0], seam=texture_seam,
                          samples=texture_drawing_samples, filter=texture_drawing_filter) if drawings else None
        field = None
        if texture_source != "vertex" and texture_field is not None:
            field = {"positions": verts.detach().float().cpu().numpy(), "eval_colours": texture_field,
                     "samples": int(texture_samples)}
        m = uv_mapping(out, fz, c, name, size=int(texture_size),
                       device=verts.device if verts.is_cuda else None, projection=projection, field=field)
        return write_obj_textured(path, m["verts"], m["faces"], m["uvs"], m["image"], name)
    return write_obj(path, out, fz, c)
