"""GPU: the counting-sort protocol of csrc/bin_sort.h (COUNT, the caller's prefix sum, FILL) as each
of its five sources runs it: the three staged entry points (dsu_mesh_render_ortho, dsu_uv_bake,
dsu_bone_visibility) through their plans, and the z-grid / point bins of mesh_post.hip through
ops.ZGrid.  The enumeration of every source (which bins an item touches) is restated below in
float64 numpy with the device's operation order, and EQUALITY is asserted: the per-bin counts, the
offsets, every bin's id list as a set (the order within a bin comes from atomics and is free), no
id twice in a bin, nothing at all from an invalid item, and the n_items guard of FILL.

The inputs are the smallest that reach every branch of an enumeration: a face over every bin, faces
off every side of the frame, a NaN and an infinite vertex, an index == V and a negative one, faces
across one and across both tile boundaries, a face inside the last (partial) tile, a face clipped by
the frame, a degenerate face, and a face outside the frame but inside the margin of the range."""
import math

import numpy as np
import pytest
import torch

from drawingspinup_amd import ops
from drawingspinup_amd._lib import lib, ptr, stream

pytestmark = pytest.mark.gpu

SENTINEL = -7
NAN, INF = float("nan"), float("inf")


def _t(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _box(x0, x1, y0, y1):
    """Three 2-D vertices whose bounding box is [x0, x1] x [y0, y1]."""
    return [(x0, y0), (x1, y0), (x0, y1)]


# ---------------------------------------------------------------- the shared checks
def check_counts(counts, want):
    assert counts.tolist() == [len(w) for w in want]


def check_fill(counts, offsets, items, want):
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert len(items) == offsets[-1]
    for b, w in enumerate(want):
        got = items[offsets[b]:offsets[b + 1]].tolist()
        assert sorted(got) == sorted(w), b
        assert len(set(got)) == len(got), b


def check_staged(plan, fill_stage, want, invalid):
    """Checks 1-4 on a plan of a staged entry point.  want[b] = the ids of bin b."""
    nb = plan.bins
    assert nb == len(want)
    plan.count()
    counts = plan.workspace[:nb].cpu().numpy()
    check_counts(counts, want)
    total = plan.scan()
    plan.fill(total)
    offsets = plan.workspace[nb:2 * nb + 1].cpu().numpy()
    items = plan.items.cpu().numpy()
    check_fill(counts, offsets, items, want)
    assert invalid and not set(items.tolist()) & set(invalid)
    assert not any(set(w) & set(invalid) for w in want)          # the restatement agrees on what is invalid
    # the guard: FILL told of half the items, on a full-length buffer
    half = total // 2
    assert 0 < half < total
    full = torch.full((total,), SENTINEL, dtype=torch.int32, device=plan.workspace.device)
    plan.items = full[:half]
    plan._stage(fill_stage)
    got = full.cpu().numpy()
    assert (got[half:] == SENTINEL).all()
    bin_of = np.searchsorted(offsets, np.arange(total), side="right") - 1
    written = 0
    for at in range(half):
        if got[at] != SENTINEL:
            assert got[at] in want[bin_of[at]], at
            written += 1
    assert written > 0


# ---------------------------------------------------------------- render: (frame, triangle) -> 16x16-pixel tiles
R_SIZE, R_SS, R_CX, R_CY, R_SPAN = 20, 2, 0.1, -0.05, 2.0      # G = 2 (the second tile is partial), N = 40


def render_case():
    """Sample pitch 0.05; x in [-0.9, 1.1], y in [-1.05, 0.95]; the tile boundary (sample 32) at
    x = 0.7 and y = -0.65."""
    boxes = [
        (-5.0, 5.0, -5.0, 5.0),        # 0  the whole frame
        (3.0, 4.0, 0.0, 0.5),          # 1  outside (right; left in the mirrored frame)
        (-4.0, -3.0, 0.0, 0.5),        # 2  outside (left)
        (0.0, 0.5, 3.0, 4.0),          # 3  outside (above)
        (0.0, 0.5, -4.0, -3.0),        # 4  outside (below)
        (0.0, 0.3, 0.0, 0.3),          # 5  a NaN vertex (set below)
        (0.0, 0.3, 0.0, 0.3),          # 6  an infinite vertex
        (0.0, 0.3, 0.0, 0.3),          # 7  an index == V
        (0.0, 0.3, 0.0, 0.3),          # 8  a negative index
        (0.5, 0.9, 0.2, 0.4),          # 9  across the tile boundary in x
        (0.6, 0.8, -0.75, -0.55),      # 10 across both boundaries: four tiles
        (0.85, 1.0, -1.0, -0.8),       # 11 inside the last, partial tile
        (0.9, 2.0, 0.5, 1.5),          # 12 clipped by the frame
        (-0.5, -0.5, 0.5, 0.5),        # 13 degenerate (a point): binned like any other
        (1.11, 1.5, 0.0, 0.2),         # 14 outside the frame, inside the range's margin: binned
    ]
    xy = np.array([p for b in boxes for p in _box(*b)], np.float64)
    v0 = np.concatenate([xy, np.linspace(-1.0, 1.0, len(xy))[:, None]], 1)
    v1 = v0 * np.array([-1.0, 1.0, 1.0]) + np.array([0.2, 0.1, 0.0])          # frame 1: mirrored and shifted
    screen = np.stack([v0, v1]).astype(np.float32)
    screen[:, 3 * 5 + 1, 0] = NAN
    screen[:, 3 * 6 + 2, 1] = INF
    faces = np.arange(3 * len(boxes), dtype=np.int32).reshape(-1, 3)
    faces[7, 2] = screen.shape[1]
    faces[8, 0] = -1
    return screen, faces, [1, 2, 3, 4, 5, 6, 7, 8]


def render_bins(screen, faces):
    """mesh_render.hip: face_indices, sample_range, then the tile range per frame."""
    F, V = screen.shape[:2]
    N, G, T = R_SIZE * R_SS, (R_SIZE + 15) // 16, 16 * R_SS
    n, lim = float(N), float(N) + 4.0
    want = [[] for _ in range(F * G * G)]
    for f in range(F):
        for m, (ia, ib, ic) in enumerate(faces):
            if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= V:
                continue
            p = screen[f, [ia, ib, ic], :2].astype(np.float64)
            if not np.isfinite(p).all():
                continue
            xmin, xmax, ymin, ymax = p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max()
            tc0, tc1 = ((xmin - R_CX) / R_SPAN + 0.5) * n - 0.5, ((xmax - R_CX) / R_SPAN + 0.5) * n - 0.5
            tr0, tr1 = (0.5 - (ymax - R_CY) / R_SPAN) * n - 0.5, (0.5 - (ymin - R_CY) / R_SPAN) * n - 0.5
            c0, c1 = math.floor(min(max(tc0, -4.0), lim)), math.ceil(min(max(tc1, -4.0), lim))
            r0, r1 = math.floor(min(max(tr0, -4.0), lim)), math.ceil(min(max(tr1, -4.0), lim))
            if c1 < 0 or r1 < 0 or c0 > N - 1 or r0 > N - 1:
                continue
            c0, r0, c1, r1 = max(c0, 0), max(r0, 0), min(c1, N - 1), min(r1, N - 1)
            for ty in range(r0 // T, r1 // T + 1):
                for tx in range(c0 // T, c1 // T + 1):
                    want[(f * G + ty) * G + tx].append(m)
    return want


def test_render_bins(dev):
    screen, faces, invalid = render_case()
    want = render_bins(screen, faces)
    # the case reaches what it is meant to: one, two and four tiles, both frames differ
    sizes = {m: sum(m in w for w in want[:4]) for m in range(len(faces))}
    assert sizes[0] == 4 and sizes[9] == 2 and sizes[10] == 4 and sizes[11] == 1 and sizes[14] == 1
    assert want[:4] != want[4:]
    plan = ops.MeshRenderPlan(_t(screen, np.float32, dev), _t(faces, np.int32, dev), R_CX, R_CY, R_SPAN,
                              R_SIZE, R_SS)
    check_staged(plan, ops.RENDER_FILL, want, invalid)


# ---------------------------------------------------------------- uv: face -> 16x16-texel tiles
UV_SIZE = 20                                                    # G = 2; the tile boundary (texel 16) at 0.8


def uv_case():
    boxes = [
        (-1.0, 3.0, -1.0, 3.0),        # 0  the whole atlas
        (1.5, 1.8, 0.1, 0.2),          # 1  outside (right)
        (-0.9, -0.5, 0.1, 0.2),        # 2  outside (left)
        (0.1, 0.2, 1.5, 1.8),          # 3  outside (above)
        (0.1, 0.2, -0.9, -0.5),        # 4  outside (below)
        (0.1, 0.3, 0.1, 0.3),          # 5  a NaN vertex
        (0.1, 0.3, 0.1, 0.3),          # 6  an infinite vertex
        (0.1, 0.3, 0.1, 0.3),          # 7  an index == V
        (0.1, 0.3, 0.1, 0.3),          # 8  a negative index
        (0.7, 0.9, 0.1, 0.2),          # 9  across the tile boundary in u
        (0.75, 0.85, 0.75, 0.85),      # 10 across both: four tiles
        (0.85, 0.95, 0.9, 0.95),       # 11 inside the last, partial tile
        (0.9, 1.6, 0.3, 0.4),          # 12 clipped by the atlas
        (0.25, 0.25, 0.25, 0.25),      # 13 degenerate
        (-0.04, -0.01, 0.1, 0.2),      # 14 left of the atlas, inside the margin of the range: binned
    ]
    uvs = np.array([p for b in boxes for p in _box(*b)], np.float32)
    uvs[3 * 5 + 1, 0] = NAN
    uvs[3 * 6 + 2, 1] = -INF
    faces = np.arange(3 * len(boxes), dtype=np.int32).reshape(-1, 3)
    faces[7, 1] = len(uvs)
    faces[8, 2] = -3
    return uvs, faces, [1, 2, 3, 4, 5, 6, 7, 8]


def uv_bins(uvs, faces):
    """mesh_uv.hip: face_indices, uv_tri, uv_range, then the tile range."""
    S, G, V = UV_SIZE, (UV_SIZE + 15) // 16, len(uvs)
    lim = float(S) + 4.0
    want = [[] for _ in range(G * G)]
    for m, (ia, ib, ic) in enumerate(faces):
        if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= V:
            continue
        p = uvs[[ia, ib, ic]].astype(np.float64) * float(S)
        if not np.isfinite(p).all():
            continue
        xmin, xmax, ymin, ymax = p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max()
        x0, x1 = math.floor(min(max(xmin, -4.0), lim)), math.ceil(min(max(xmax, -4.0), lim))
        y0, y1 = math.floor(min(max(ymin, -4.0), lim)), math.ceil(min(max(ymax, -4.0), lim))
        if x1 < 0 or y1 < 0 or x0 > S - 1 or y0 > S - 1:
            continue
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, S - 1), min(y1, S - 1)
        for ty in range(y0 // 16, y1 // 16 + 1):
            for tx in range(x0 // 16, x1 // 16 + 1):
                want[ty * G + tx].append(m)
    return want


def test_uv_bins(dev):
    uvs, faces, invalid = uv_case()
    want = uv_bins(uvs, faces)
    sizes = {m: sum(m in w for w in want) for m in range(len(faces))}
    assert sizes[0] == 4 and sizes[9] == 2 and sizes[10] == 4 and sizes[11] == 1 and sizes[14] == 1
    plan = ops.UvBakePlan(_t(uvs, np.float32, dev), _t(faces, np.int32, dev), UV_SIZE)
    check_staged(plan, ops.UV_FILL, want, invalid)


# ---------------------------------------------------------------- skin: triangle -> cells of its 3-D box
def skin_case():
    """Boxes (x0, x1, y0, y1, z0, z1) in a 3 x 2 x 2 grid of unit cells over [0,3] x [0,2] x [0,2]
    (the two bones span it).  The grid clamps, so there is no off-grid kind: a triangle pushed
    outside after the plan chose its grid lands in the border cells."""
    boxes = [
        (0.2, 2.7, 0.3, 1.6, 0.4, 1.5),    # 0  several cells in every axis: all twelve
        (0.1, 0.4, 0.1, 0.4, 0.1, 0.4),    # 1  one cell
        (0.6, 1.4, 1.2, 1.4, 1.2, 1.4),    # 2  two cells along x
        (1.2, 1.4, 0.6, 1.4, 0.2, 0.4),    # 3  two cells along y
        (2.2, 2.4, 0.2, 0.4, 0.6, 1.4),    # 4  two cells along z
        (1.1, 1.3, 1.1, 1.3, 1.1, 1.3),    # 5  a NaN vertex (set after the plan is built)
        (1.1, 1.3, 1.1, 1.3, 1.1, 1.3),    # 6  an infinite vertex (likewise)
        (1.1, 1.3, 1.1, 1.3, 1.1, 1.3),    # 7  an index == V
        (1.1, 1.3, 1.1, 1.3, 1.1, 1.3),    # 8  a negative index
        (1.5, 1.6, 0.5, 0.6, 1.5, 1.6),    # 9  moved to x in [-5, 10] after the plan is built: clamped
    ]
    verts = np.array([p for (x0, x1, y0, y1, z0, z1) in boxes
                      for p in [(x0, y0, z0), (x1, y1, z0), (x0, y0, z1)]], np.float32)
    faces = np.arange(3 * len(boxes), dtype=np.int32).reshape(-1, 3)
    faces[7, 0] = len(verts)
    faces[8, 1] = -1
    bones = np.array([[[0.0, 0.0, 0.0], [3.0, 2.0, 2.0]], [[0.0, 2.0, 0.0], [3.0, 0.0, 2.0]]], np.float32)
    late = {3 * 5: (NAN, 1.1, 1.1), 3 * 6 + 1: (1.3, INF, 1.1), 3 * 9: (-5.0, 0.5, 1.5), 3 * 9 + 1: (10.0, 0.6, 1.5)}
    return verts, faces, bones, late, [5, 6, 7, 8]


def skin_bins(verts, faces, lo, cell, g):
    """mesh_skin.hip: face_indices, finite vertices, cell_of per axis (clamped), then the cell box."""
    want = [[] for _ in range(g[0] * g[1] * g[2])]
    for m, (ia, ib, ic) in enumerate(faces):
        if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= len(verts):
            continue
        p = verts[[ia, ib, ic]].astype(np.float64)
        if not np.isfinite(p).all():
            continue
        c0 = [int(min(max(math.floor((p[:, a].min() - lo[a]) / cell), 0.0), g[a] - 1.0)) for a in range(3)]
        c1 = [int(min(max(math.floor((p[:, a].max() - lo[a]) / cell), 0.0), g[a] - 1.0)) for a in range(3)]
        for cz in range(c0[2], c1[2] + 1):
            for cy in range(c0[1], c1[1] + 1):
                for cx in range(c0[0], c1[0] + 1):
                    want[(cz * g[1] + cy) * g[0] + cx].append(m)
    return want


def test_skin_bins(dev):
    verts, faces, bones, late, invalid = skin_case()
    tv = _t(verts, np.float32, dev)
    plan = ops.BoneVisibilityPlan(tv, _t(faces, np.int32, dev), _t(bones, np.float32, dev), cells_per_axis=3)
    assert plan.g == [3, 2, 2] and plan.cells == plan.bins == 12 and plan.verts is tv
    for k, p in late.items():                                     # the grid is chosen; now move the vertices
        verts[k] = p
        tv[k] = torch.tensor(p, dtype=torch.float32, device=dev)
    want = skin_bins(verts, faces, plan.lo, plan.cell, plan.g)
    sizes = {m: sum(m in w for w in want) for m in range(len(faces))}
    assert sizes[0] == 12 and sizes[1] == 1 and sizes[2] == sizes[3] == sizes[4] == 2 and sizes[9] == 3
    check_staged(plan, ops.SKIN_FILL, want, invalid)


# ---------------------------------------------------------------- z-grid and point bins (mesh_post.hip)
def zgrid_cell(v, v0, cell, g):
    """cell_of of mesh_post.hip.  The device works in float32; every coordinate below is at least a
    tenth of a cell away from a cell boundary, so float64 gives the same cell."""
    return int(min(max(math.floor((v - v0) * (1.0 / cell)), 0), g - 1))


def check_zgrid(dev, data, points, want):
    g, lo, hi = 3, (0.0, 0.0), (3.0, 3.0)
    d = _t(data, np.float32, dev)
    grid = ops.ZGrid(d, lo, hi, points=points, cells_per_axis=g)
    assert grid.g == g and (grid.x0, grid.y0) == lo
    counts = torch.zeros(g * g, dtype=torch.int32, device=dev)
    fn = lib().dsu_point_bin_count if points else lib().dsu_zgrid_count
    assert fn(ptr(d, torch.float32), len(data), grid.x0, grid.y0, grid.cell, g, ptr(counts), stream()) == 0
    counts = counts.cpu().numpy()
    check_counts(counts, want(grid))
    check_fill(counts, grid.offsets.cpu().numpy(), grid.items.cpu().numpy(), want(grid))


def test_zgrid_triangle_bins(dev):
    boxes = [(0.2, 0.4, 0.2, 0.4),         # one cell
             (0.5, 1.5, 0.3, 2.6),         # 2 x 3 cells
             (0.1, 2.9, 0.1, 2.9),         # every cell
             (2.3, 2.6, 1.2, 1.7),         # one cell, last column
             (2.5, 7.0, -4.0, 0.5)]        # reaches outside: clamped to the border cells
    tris = np.array([[(x, y, 0.5) for x, y in _box(*b)] for b in boxes], np.float32)

    def want(grid):
        out = [[] for _ in range(9)]
        for f, t in enumerate(tris.astype(np.float64)):
            cx0, cx1 = (zgrid_cell(v, grid.x0, grid.cell, 3) for v in (t[:, 0].min(), t[:, 0].max()))
            cy0, cy1 = (zgrid_cell(v, grid.y0, grid.cell, 3) for v in (t[:, 1].min(), t[:, 1].max()))
            for cy in range(cy0, cy1 + 1):
                for cx in range(cx0, cx1 + 1):
                    out[cy * 3 + cx].append(f)
        assert [sum(f in o for o in out) for f in range(5)] == [1, 6, 9, 1, 1]
        return out
    check_zgrid(dev, tris, False, want)


def test_zgrid_point_bins(dev):
    pts = np.array([(0.5, 0.5), (0.6, 0.4), (1.5, 2.5), (2.5, 0.3), (2.7, 0.2), (9.0, -1.0), (1.4, 1.6)], np.float32)

    def want(grid):
        out = [[] for _ in range(9)]
        for i, (x, y) in enumerate(pts.astype(np.float64)):
            out[zgrid_cell(y, grid.y0, grid.cell, 3) * 3 + zgrid_cell(x, grid.x0, grid.cell, 3)].append(i)
        assert out[0] == [0, 1] and out[2] == [3, 4, 5] and out[7] == [2] and out[4] == [6]
        return out
    check_zgrid(dev, pts, True, want)
