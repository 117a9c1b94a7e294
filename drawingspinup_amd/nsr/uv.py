"""The export_uv branch of save_mesh (mesh_utils.py:65-67, coloring_utils.py:140-167) without
xatlas: axis-projection charts, shelf packing, and the reference's compute_interpolation_map as a
rasteriser of the mesh's own triangles.

    parametrize(verts, faces)            -> (vmapping, indices, uvs), as xatlas.parametrize
    bake_vertex_colours(uvs, indices, c) -> (size, size, 3) uint8, as compute_interpolation_map
    bake_drawings(uvs, indices, p, ...)  -> the same atlas with the input drawings projected into
                                            it texel by texel (an extension, see below)
    bake_field(uvs, indices, p, eval)    -> the same atlas with the optimised texture field evaluated
                                            texel by texel (an extension, see below)
    uv_mapping(v, faces, colours, name)  -> the textured mesh, as coloring_utils.uv_mapping

Labels, charts, the atlas raster and the gutter fill run on the device (csrc/mesh_uv.hip, rules in
include/dsu_hip.h); projection and packing are numpy on the host.

Charts.  A face's label is its normal's dominant axis and sign; a chart is a connected component
of faces that share a manifold edge and a label, its id the smallest face index in it.  No label
relaxation is shipped, so every face keeps |n_axis| >= |n| / sqrt(3): MIN_COS.  A chart is
projected along its axis, the two other axes ordered so that its faces are counter-clockwise in
uv; one scale (texels per unit length) serves all charts.  A chart that overlaps itself in
projection is split: the atlas is rasterised, of the faces strictly containing one sample point
all but the front-most (largest coordinate sum along the viewing side of the axis; lowest index on
a tie) are demoted to label + 6, and charts, packing and raster are redone — the check therefore
always runs at the layout that is returned.  After SPLIT_ROUNDS demotions a face still in conflict
becomes a chart of its own.

Texel convention: the reference's, image row r / column c samples uv * size = (c, size - 1 - r).
That is half a texel away from the texel-centre convention most viewers assume; the gutter fill
around every chart is what makes the difference harmless (a bilinear fetch near a chart's border
reads filled texels, never the empty atlas).

Drawings.  The vertex-colour bake holds no more detail than the vertices do.  bake_drawings asks,
per texel, which pixel of the front or back drawing the texel's surface point sees — the question
nsr/mesh_post.color_projection asks per vertex (same frame, same masks, same nearest-pixel read) —
and keeps the vertex-colour bake where neither view sees it (dsu_uv_project in include/dsu_hip.h
has the rule in full).  What remains visible of the composition: a seam where projected and
fallback texels meet (unless it is levelled, below), nearest-pixel sampling by default (samples > 1
or pixel_filter="bilinear" reads samples x samples points per texel and averages them:
dsu_uv_project_area), and a fallback band along the silhouette as wide as the erosion of the masks
(19 pixels of the 2048^2 drawings).

Field.  bake_field asks the network the export has just optimised instead: every covered texel's
surface point (samples x samples of them, a texel wide) goes back to the field's own frame through
the atlas barycentrics and is evaluated by the caller's `eval_colours` (nsr/mesh.field_colours:
the kernels vertex_colors runs); the mean of a texel's samples is its colour
(dsu_uv_field_points / dsu_uv_field_resolve in include/dsu_hip.h).  The points lie on the
triangles, not on the zero level set (no snapping), and a sub-sample that falls outside its face is
evaluated on the face's plane.  With the drawings as well, the field takes the vertex bake's place
as their fallback; the seam between the two stays unless it is levelled.

Seam.  bake_drawings(seam="level") (projection["seam"], save_obj's texture_seam; off by default)
levels the fallback to the drawings (Lempitsky & Ivanov 2007): the drawing texels keep their bytes,
the fallback texels get a smooth colour offset.  dsu_uv_seam_gather sums drawing - fallback of the
projected texels per welded vertex group (seam_groups: the chart copies of a vertex are one
unknown, so the offset is continuous across chart borders); seam_offsets makes a group with a whole
texel's weight known and extends the known offsets harmonically over the welded mesh's edges
(uniform weights: an M-matrix, so no offset leaves the range of the known ones; solved by
dsu_spd_cg_block); dsu_uv_seam_apply adds the offset interpolated within each face and rounds.  What
stays of the seam: the high-frequency mismatch (sharp ink beside a smooth field), which an offset
that is smooth over the mesh does not touch.
"""
import math

import numpy as np
import torch

MIN_COS = 1.0 / math.sqrt(3.0)
SPLIT_ROUNDS = 8
SHRINK = 0.9            # the scale's factor per packing retry
FILL_TARGET = 0.6       # first scale: the charts' projected area over the atlas area
# Occluders closer than this in front of a texel's point are ignored (projection frame units, the
# mesh inside [-0.5, 0.5]).  Lower bound: z is float32, one rounding is ~6e-8 here, and a neighbour
# across a shared edge or a fold meets the point at a depth difference of that order, which must
# not count as cover.  Upper bound: two layers of the surface that really hide one another are at
# least one voxel of the marching-cubes lattice apart, ~1e-3 at resolution 512; a tolerance near
# that would let the rear layer read the drawing through the front one.  1e-4 is a tenth of a voxel
# and three decades above the rounding.  The choice rests on that reasoning: on the smooth
# ~50 000-face probe mesh the sweep of tools/uv_project_probe.py (`tolerance_sweep` in
# profiles/uv_project_probe.json) moves 3 of 334 085 covered texels between 0 and 1e-5 and none
# between 1e-5, 1e-4 and 1e-3, so that mesh does not tell the candidates apart; a marching-cubes
# mesh with thin folds has not been swept.
Z_TOLERANCE = 1e-4
# Seam levelling: a group's offset is known when the projected texels around it weigh at least one
# whole texel (the gather's fixed point: a barycentric of 1 is 2^20); slivers do not pin an offset.
SEAM_MIN_WEIGHT = 1 << 20
SEAM_TOL = 1e-10
SEAM_MAX_ITERS = 20000
PIXEL_FILTERS = ("nearest", "bilinear")     # how bake_drawings reads a drawing at a sample point


# ------------------------------------------------------------------ host parts
def shelf_pack(wh, ids, size, gutter):
    """Boxes (C,2) whole texels (w, h), sorted by (h descending, id), placed left to right on
    shelves from the bottom: boxes `gutter` apart and `gutter` from the border.  -> (C,2) int64
    origins (x0, y0) in the input's order, or None when they do not fit."""
    wh = np.asarray(wh, np.int64).reshape(-1, 2)
    ids = np.asarray(ids, np.int64)
    out = np.zeros_like(wh)
    x = y = int(gutter)
    shelf = 0
    for k in np.lexsort((ids, -wh[:, 1])):
        w, h = int(wh[k, 0]), int(wh[k, 1])
        if w + 2 * gutter > size:
            return None
        if x + w + gutter > size:
            y += shelf + gutter
            x, shelf = int(gutter), 0
        if y + h + gutter > size:
            return None
        out[k] = (x, y)
        x += w + gutter
        shelf = max(shelf, h)
    return out


def _axes(label):
    """(axis, u axis, v axis, viewing sign) per base label 0..5; a degenerate face (-1) uses axis 0."""
    lab = np.where(label < 0, 0, label)
    a = lab // 2
    neg = (lab % 2) == 1
    ua, va = (a + 1) % 3, (a + 2) % 3
    return a, np.where(neg, va, ua), np.where(neg, ua, va), np.where(neg, -1.0, 1.0)


def face_depths(verts, faces, label):
    """Per face: the sum of its three coordinates along its axis, (a + b) + c in float64, times the
    viewing sign — larger is nearer the side the chart is seen from."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    a, _, _, sg = _axes(label)
    rows = np.arange(len(faces))
    p = v[faces][rows, :, a]                                           # (M,3)
    return sg * ((p[:, 0] + p[:, 1]) + p[:, 2])


def layout(verts, faces, label, chart, size, gutter, scale=None):
    """Projection + packing for given labels and chart ids -> (vmapping, indices, uvs, info)."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    M = len(faces)
    ids, face_slot = np.unique(chart, return_inverse=True)
    Cn = len(ids)
    first = np.zeros(Cn, np.int64)
    first[face_slot[::-1]] = np.arange(M)[::-1]                        # any face of the chart: the lowest
    clabel = label[first]
    # one new vertex per (old vertex, chart), ordered by (old vertex, chart id)
    corner_v = faces.reshape(-1)
    corner_c = np.repeat(chart, 3)
    key, inv = np.unique(corner_v * np.int64(max(M, 1)) + corner_c, return_inverse=True)
    vmapping = key // max(M, 1)
    vchart = key - vmapping * max(M, 1)
    indices = inv.reshape(M, 3).astype(np.int64)
    vslot = np.searchsorted(ids, vchart)
    _, ua, va, _ = _axes(clabel)
    flat = clabel < 0                                                  # degenerate: a point
    pu = np.where(flat[vslot], 0.0, v[vmapping, ua[vslot]])
    pv = np.where(flat[vslot], 0.0, v[vmapping, va[vslot]])
    lo_u, lo_v = np.full(Cn, np.inf), np.full(Cn, np.inf)
    hi_u, hi_v = np.full(Cn, -np.inf), np.full(Cn, -np.inf)
    np.minimum.at(lo_u, vslot, pu); np.minimum.at(lo_v, vslot, pv)
    np.maximum.at(hi_u, vslot, pu); np.maximum.at(hi_v, vslot, pv)
    ext = np.stack([hi_u - lo_u, hi_v - lo_v], 1) if Cn else np.zeros((0, 2))
    if scale is None:
        e1, e2 = v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
        n = np.cross(e1, e2)
        a, _, _, _ = _axes(label)
        total = 0.5 * float(np.abs(n[np.arange(M), a])[label >= 0].sum()) if M else 0.0
        scale = math.sqrt(FILL_TARGET * size * size / total) if total > 0 else 1.0
    retries = 0
    while True:
        wh = np.ceil(ext * scale).astype(np.int64) + 1                 # samples x0 .. x0 + ceil(extent s)
        origin = shelf_pack(wh, ids, size, gutter)
        if origin is not None:
            break
        scale *= SHRINK
        retries += 1
        if retries > 400:
            raise ValueError(f"{Cn} charts do not fit a {size}x{size} atlas with gutter {gutter}")
    U = (pu - lo_u[vslot]) * scale + origin[vslot, 0]
    W = (pv - lo_v[vslot]) * scale + origin[vslot, 1]
    uvs = (np.stack([U, W], 1) / float(size)).astype(np.float32)
    a, _, _, _ = _axes(clabel)
    info = {"face_chart": chart.astype(np.int64), "chart_ids": ids, "chart_axis": a,
            "chart_sign": np.where(clabel < 0, 0, clabel % 2), "chart_rect": np.concatenate([origin, wh], 1),
            "scale": float(scale), "min_cos": MIN_COS, "pack_retries": retries}
    return vmapping, indices, uvs, info


# ------------------------------------------------------------------ device parts
class DeviceBackend:
    """The kernels behind the interface parametrize / bake_vertex_colours / bake_drawings use
    (tests/uv_ref.py, tests/uv_project_ref.py, tests/uv_field_ref.py and tests/uv_seam_ref.py have the
    float64 numpy one)."""

    def __init__(self, device=None):
        self.dev = torch.device(device if device is not None else "cuda")

    def labels(self, verts, faces):
        from .. import ops
        self.faces = torch.from_numpy(np.ascontiguousarray(faces)).to(self.dev)
        n, lab, ar = ops.uv_face_labels(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(self.dev),
                                        self.faces)
        self.adjacency = ops.face_adjacency(self.faces)
        return n.cpu().numpy(), lab.cpu().numpy().astype(np.int64), ar.cpu().numpy()

    def components(self, faces, comp_label):
        from .. import ops
        chart, rounds = ops.uv_components(self.adjacency, torch.from_numpy(comp_label.astype(np.int32)).to(self.dev))
        return chart.cpu().numpy().astype(np.int64), rounds

    def bake(self, uvs, indices, colours, size, depth=None):
        from .. import ops
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.dev)
        img, fid, dem = ops.uv_bake(t(uvs, np.float32), t(indices, np.int32), t(colours, np.float32), size,
                                    None if depth is None else t(depth, np.float64))
        return img, fid, (None if dem is None else dem.cpu().numpy())

    def dilate(self, image, covered, rounds):
        from .. import ops
        return ops.uv_dilate(image, covered, rounds)[0]

    def _projection_inputs(self, uvs, indices, positions, color_front, mask_front, color_back, erode):
        """-> (uvs, indices, positions) and (color_front, mask_front, color_back, mask_back) on the
        device, the masks prepared as color_projection prepares them: what ops.uv_project takes before
        and after face_id."""
        from .mesh_post import projection_masks
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(_host(a), dt)).to(self.dev)
        pos, ind = t(positions, np.float32), t(indices, np.int64)
        cf, mf, cb = (torch.as_tensor(a).to(self.dev, torch.uint8).contiguous()
                      for a in (color_front, mask_front, color_back))
        front, back = projection_masks(pos, ind, mf, res=cf.shape[0], ksize=int(erode))
        return (t(uvs, np.float32), ind, pos), (cf, front, cb, back)

    def project(self, uvs, indices, positions, face_id, color_front, mask_front, color_back, z_tolerance,
                erode, cells_per_axis=None):
        """Mask preparation as color_projection's + dsu_uv_project -> image (S,S,3) u8, source (S,S) u8."""
        from .. import ops
        atlas, images = self._projection_inputs(uvs, indices, positions, color_front, mask_front, color_back, erode)
        return ops.uv_project(*atlas, face_id, *images, z_tolerance, cells_per_axis=cells_per_axis)

    def project_area(self, uvs, indices, positions, face_id, color_front, mask_front, color_back, z_tolerance,
                     erode, samples, pixel_filter, cells_per_axis=None):
        """project with dsu_uv_project_area in dsu_uv_project's place -> image (S,S,3) u8, source (S,S) u8."""
        from .. import ops
        atlas, images = self._projection_inputs(uvs, indices, positions, color_front, mask_front, color_back, erode)
        return ops.uv_project_area(*atlas, face_id, *images, z_tolerance, samples, pixel_filter,
                                   cells_per_axis=cells_per_axis)[:2]

    def field_points(self, uvs, indices, positions, face_id, texels, samples):
        from .. import ops
        t = lambda a, dt: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.dev)
        return ops.uv_field_points(t(uvs, np.float32), t(indices, np.int32), t(positions, np.float32), face_id,
                                   texels, samples)

    def field_resolve(self, colours, valid, texels, image):
        from .. import ops
        return ops.uv_field_resolve(colours, valid, texels, image)

    def _seam_atlas(self, uvs, indices, group):
        t = lambda a, dt: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.dev)
        return t(uvs, np.float32), t(indices, np.int32), t(group, np.int32)

    def seam_gather(self, uvs, indices, group, n_groups, face_id, source, proj, fallback):
        from .. import ops
        return ops.uv_seam_gather(*self._seam_atlas(uvs, indices, group), face_id, source, proj, fallback, n_groups)

    def seam_solve(self, A, rhs):
        """A (n,n) scipy csr with sorted indices, symmetric positive definite, rhs (n,3) -> x (n,3)
        f64 (numpy) by dsu_spd_cg_block; .seam_iterations holds the iteration count."""
        from .. import ops
        x, iters, res = ops.spd_cg_block(torch.from_numpy(A.indptr.astype(np.int32)).to(self.dev),
                                         torch.from_numpy(A.indices.astype(np.int32)).to(self.dev),
                                         torch.from_numpy(A.data.astype(np.float64)).to(self.dev),
                                         torch.from_numpy(np.ascontiguousarray(rhs, np.float64)).to(self.dev),
                                         tol=SEAM_TOL, max_iters=SEAM_MAX_ITERS)
        if iters >= SEAM_MAX_ITERS and not (res <= SEAM_TOL).all():
            raise RuntimeError(f"seam solve did not converge in {SEAM_MAX_ITERS} iterations "
                               f"(residual {res.max():.3e})")
        self.seam_iterations = iters
        return x.cpu().numpy()

    def seam_apply(self, uvs, indices, group, face_id, source, proj, fallback, d):
        from .. import ops
        return ops.uv_seam_apply(*self._seam_atlas(uvs, indices, group), face_id, source, proj, fallback,
                                 torch.from_numpy(np.ascontiguousarray(d, np.float64)).to(self.dev))

    @staticmethod
    def to_numpy(a):
        return a.cpu().numpy()


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def parametrize(verts, faces, size=1024, gutter=2, return_info=False, device=None, scale=None, backend=None):
    """xatlas.parametrize's contract: vmapping (V',) int64 — new vertex k is old vertex vmapping[k];
    indices (M,3) int64 with vmapping[indices] == faces; uvs (V',2) float32 in [0,1].  `scale`
    (texels per unit length) overrides the first scale tried.  With return_info also the dict
    described in the module's header (face_chart, chart_ids / _axis / _sign / _rect (x0, y0, w, h
    in uv texels, y up), scale, min_cos, split_rounds, isolated_faces, component_rounds)."""
    verts = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    faces = np.ascontiguousarray(np.asarray(faces, np.int64).reshape(-1, 3))
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError("face index out of range")
    be = backend if backend is not None else DeviceBackend(device)
    normal, base, area = be.labels(verts, faces)
    comp = base.copy()
    depth = face_depths(verts, faces, base)
    split_rounds = isolated = 0
    comp_rounds = []
    zeros = None
    for _ in range(SPLIT_ROUNDS + len(faces) + 2):
        chart, rounds = be.components(faces, comp)
        comp_rounds.append(int(rounds))
        vmapping, indices, uvs, info = layout(verts, faces, base, chart, size, gutter, scale)
        if zeros is None or len(zeros) != len(vmapping):
            zeros = np.zeros((len(vmapping), 3), np.float32)
        demote = be.bake(uvs, indices, zeros, size, depth)[2]
        hit = np.nonzero(demote)[0] if len(faces) else np.zeros(0, np.int64)
        if len(hit) == 0:
            break
        if split_rounds < SPLIT_ROUNDS:
            comp[hit] += 6
            split_rounds += 1
        else:
            comp[hit] = -2                                             # joins nothing: a chart of its own
            isolated += len(hit)
    else:
        raise RuntimeError("uv charts still overlap after the split loop")
    info.update(split_rounds=split_rounds, isolated_faces=isolated, component_rounds=comp_rounds,
                label=base, normal=normal, area=area)
    return (vmapping, indices, uvs, info) if return_info else (vmapping, indices, uvs)


def bake_vertex_colours(uvs, indices, colours, size=1024, gutter=2, device=None, backend=None,
                        return_maps=False):
    """compute_interpolation_map on the mesh's own triangles: (size, size, 3) uint8, `gutter` rounds
    of fill around the charts, 0 where nothing reaches.  return_maps: also face_id (size, size)
    int32 before the fill, -1 where no face covers the sample."""
    be = backend if backend is not None else DeviceBackend(device)
    img, fid, _ = be.bake(np.asarray(uvs, np.float32), np.asarray(indices, np.int64),
                          np.asarray(colours, np.float32).reshape(-1, 3), int(size))
    out = be.dilate(img, fid >= 0, int(gutter)) if gutter > 0 else img
    out = be.to_numpy(out)
    return (out, be.to_numpy(fid)) if return_maps else out


def seam_groups(verts, faces, vmapping):
    """The unknowns of seam levelling: verts (V,3) and faces (M,3) of the mesh before the charts,
    vmapping (V') as parametrize returns it.  -> group (V') int32, the welded class of every atlas
    vertex (nsr/thinning._weld's representative of vmapping[k], compacted to [0, G)): the chart
    copies of one vertex and coincident vertices are one unknown; group_faces (F,3) int64, the faces
    over the groups without those whose three groups are not distinct (the graph's triangles)."""
    from .thinning import _weld
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    vmapping = np.asarray(vmapping, np.int64).reshape(-1)
    rep, _ = _weld(np.asarray(verts, np.float64).reshape(-1, 3), faces)
    reps, group = np.unique(rep[vmapping], return_inverse=True)
    g = np.searchsorted(reps, rep[faces]) if len(faces) else np.zeros((0, 3), np.int64)
    distinct = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    return group.reshape(-1).astype(np.int32), g[distinct].astype(np.int64)


def seam_offsets(num, den, group_faces, backend):
    """The host step of seam levelling (include/dsu_hip.h, between h. and i.): num (G,3) and den (G)
    int64 from seam_gather -> d (G,3) f64, known (G) bool.  A group with den >= SEAM_MIN_WEIGHT is
    known, d = num / den.  The others solve the uniform Laplacian over the edges of group_faces,
    deg(u) d_u - sum of unknown neighbours = sum of known neighbours, through backend.seam_solve
    (three columns at once); a connected set of unknowns without a known neighbour keeps 0."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    num = np.asarray(_host(num), np.int64).reshape(-1, 3)
    den = np.asarray(_host(den), np.int64).reshape(-1)
    G = len(den)
    known = den >= SEAM_MIN_WEIGHT
    d = np.zeros((G, 3), np.float64)
    d[known] = num[known].astype(np.float64) / den[known].astype(np.float64)[:, None]
    gf = np.asarray(group_faces, np.int64).reshape(-1, 3)
    if G == 0 or not len(gf) or known.all() or not known.any():
        return d, known
    e = np.concatenate([gf[:, [0, 1]], gf[:, [1, 2]], gf[:, [2, 0]]], 0)
    e = np.unique(np.sort(e, 1), axis=0)                               # every undirected edge once
    A = sp.csr_matrix((np.ones(2 * len(e)), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))),
                      shape=(G, G))
    deg = np.asarray(A.sum(1)).reshape(-1)
    unknown = np.flatnonzero(~known)
    Auu, Auk = A[unknown][:, unknown], A[unknown][:, np.flatnonzero(known)]
    _, comp = connected_components(Auu, directed=False)
    touches = np.asarray(Auk.sum(1)).reshape(-1) > 0
    fed = np.zeros(comp.max() + 1, bool)
    fed[comp[touches]] = True
    keep = np.flatnonzero(fed[comp])                                   # rows of `unknown` that are solved
    if not len(keep):
        return d, known
    L = (sp.diags(deg[unknown[keep]]) - Auu[keep][:, keep]).tocsr()
    L.sum_duplicates()
    L.sort_indices()
    rhs = Auk[keep] @ d[known]
    d[unknown[keep]] = np.asarray(backend.seam_solve(L, np.ascontiguousarray(rhs, np.float64)), np.float64)
    return d, known


def bake_drawings(uvs, indices, positions, color_front_u8, mask_front_u8, color_back_u8, fallback_colours,
                  size=1024, gutter=2, z_tolerance=Z_TOLERANCE, erode=19, device=None, backend=None,
                  return_maps=False, fallback_image=None, seam="none", groups=None, group_faces=None, samples=1,
                  pixel_filter="nearest"):
    """The atlas with the drawings projected into it: positions (V',3) are the atlas vertices in
    color_projection's frame (x right, y up, z front, inside [-0.5, 0.5]: after thinning and
    smoothing, before shear and ortho_scale), color_*_u8 (res,res,3) and mask_front_u8 (res,res) the
    images color_projection takes (arrays or tensors).  The masks are prepared as there (cut to the
    mesh's silhouette, eroded with the `erode` ellipse, mirrored for the back view); a texel that
    neither view sees keeps the vertex-colour bake of fallback_colours (V',3); the gutter fill runs
    over the composition.  return_maps: also face_id (size,size) i32 and source (size,size) u8
    (0 fallback, 1 front, 2 back).  fallback_image (size,size,3) u8 without gutter fill (bake_field's,
    gutter=0) takes the place of the vertex-colour bake.
    seam: "none" composes with a hard where(source > 0, drawing, fallback); "level" leaves the
    drawing texels alone and adds to the fallback texels a smooth offset that meets the drawing at
    the border (dsu_uv_seam_gather, seam_offsets, dsu_uv_seam_apply); it needs groups (V') and
    group_faces (F,3) from seam_groups.
    samples, pixel_filter: the drawings read at samples x samples points per texel (1..8), each at its
    "nearest" pixel or "bilinear", and averaged (dsu_uv_project_area); 1 and "nearest" are
    dsu_uv_project, one nearest pixel per texel."""
    if seam not in ("none", "level"):
        raise ValueError("seam must be 'none' or 'level'")
    if not 1 <= int(samples) <= 8:
        raise ValueError("samples must be 1..8")
    if pixel_filter not in PIXEL_FILTERS:
        raise ValueError("pixel_filter must be 'nearest' or 'bilinear'")
    if seam == "level" and (groups is None or group_faces is None):
        raise ValueError("seam='level' needs groups and group_faces (seam_groups)")
    be = backend if backend is not None else DeviceBackend(device)
    uvs, indices = np.asarray(uvs, np.float32), np.asarray(indices, np.int64)
    img, fid, _ = be.bake(uvs, indices, np.asarray(fallback_colours, np.float32).reshape(-1, 3), int(size))
    pos = np.asarray(_host(positions), np.float32).reshape(-1, 3)
    if int(samples) > 1 or pixel_filter != "nearest":
        proj, src = be.project_area(uvs, indices, pos, fid, color_front_u8, mask_front_u8, color_back_u8,
                                    float(z_tolerance), int(erode), int(samples), pixel_filter)
    else:
        proj, src = be.project(uvs, indices, pos, fid, color_front_u8, mask_front_u8, color_back_u8,
                               float(z_tolerance), int(erode))
    if fallback_image is not None:
        img = torch.as_tensor(_host(fallback_image)).to(src.device) if torch.is_tensor(src) else _host(fallback_image)
        if tuple(img.shape) != tuple(proj.shape):
            raise ValueError("fallback_image must be (size,size,3) uint8")
    if seam == "level":
        groups = np.ascontiguousarray(groups, np.int32).reshape(-1)
        if len(groups) != len(uvs):
            raise ValueError("groups must hold one class per atlas vertex")
        n_groups = int(groups.max()) + 1 if len(groups) else 0
        num, den = be.seam_gather(uvs, indices, groups, n_groups, fid, src, proj, img)
        d, _ = seam_offsets(be.to_numpy(num), be.to_numpy(den), group_faces, be)
        out = be.seam_apply(uvs, indices, groups, fid, src, proj, img, d)
    else:
        where = torch.where if torch.is_tensor(src) else np.where
        out = where((src > 0)[..., None], proj, img)
    if gutter > 0:
        out = be.dilate(out, fid >= 0, int(gutter))
    out = be.to_numpy(out)
    return (out, be.to_numpy(fid), be.to_numpy(src)) if return_maps else out


def bake_field(uvs, indices, field_positions, eval_colours, fallback_colours=None, size=1024, gutter=2,
               samples=2, chunk=1 << 21, device=None, backend=None, return_maps=False):
    """The atlas with the texture field evaluated texel by texel: field_positions (V',3) are the
    atlas vertices in the field's frame (the vertices the export received, in the atlas's vertex
    order), eval_colours a callable taking (N,3) f32 points (on the device, with the device
    backend) and returning (N,3) colours in [0,1].  The vertex bake of fallback_colours (V',3;
    zeros when None) gives face_id and what stays where a texel has no valid sample; the covered
    texels are then walked in pieces of at most chunk // samples^2 texels — points, eval_colours on
    all points of the piece, the mean into the image — so that no more than `chunk` points exist at
    a time; the gutter fill runs over the result.  samples: sub-samples per axis, 1..8.
    return_maps: also face_id (size,size) i32 and evaluated (size,size) u8, 1 where at least one
    sample was valid."""
    be = backend if backend is not None else DeviceBackend(device)
    s, S = int(samples), int(size)
    if not 1 <= s <= 8:
        raise ValueError("samples must be 1..8")
    if not callable(eval_colours):
        raise ValueError("eval_colours must be callable")
    uvs, indices = np.asarray(uvs, np.float32), np.asarray(indices, np.int64)
    pos = np.ascontiguousarray(np.asarray(_host(field_positions), np.float32).reshape(-1, 3))
    if len(pos) != len(uvs):
        raise ValueError("field_positions must hold one row per atlas vertex")
    fallback = np.zeros((len(uvs), 3), np.float32) if fallback_colours is None else \
        np.asarray(fallback_colours, np.float32).reshape(-1, 3)
    img, fid, _ = be.bake(uvs, indices, fallback, S)
    on_device = torch.is_tensor(fid)
    if on_device:
        texels = torch.nonzero(fid.reshape(-1) >= 0).reshape(-1).to(torch.int32)
        evaluated = torch.zeros(S * S, dtype=torch.uint8, device=fid.device)
        # uploaded once, not once per piece
        put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(fid.device)
        uvs_b, ind_b, pos_b = put(uvs, np.float32), put(indices, np.int32), put(pos, np.float32)
    else:
        texels = np.nonzero(np.asarray(fid).reshape(-1) >= 0)[0].astype(np.int32)
        evaluated = np.zeros(S * S, np.uint8)
        uvs_b, ind_b, pos_b = uvs, indices, pos
    piece = max(1, int(chunk) // (s * s))
    for at in range(0, len(texels), piece):
        part = texels[at:at + piece]
        points, valid = be.field_points(uvs_b, ind_b, pos_b, fid, part, s)
        colours = eval_colours(points.reshape(-1, 3))
        if tuple(colours.shape) != (len(part) * s * s, 3):
            raise ValueError("eval_colours must return one (r, g, b) per point")
        colours = colours.detach().float() if on_device else np.asarray(colours, np.float32)
        img = be.field_resolve(colours.reshape(len(part), s * s, 3), valid, part, img)
        hit = valid.reshape(len(part), s * s)
        evaluated[part.long() if on_device else part] = hit.amax(1) if on_device else hit.max(1)
    out = be.dilate(img, fid >= 0, int(gutter)) if gutter > 0 else img
    out = be.to_numpy(out)
    return (out, be.to_numpy(fid), be.to_numpy(evaluated.reshape(S, S))) if return_maps else out


def uv_mapping(v_np, faces, vert_colors, save_name, size=1024, gutter=2, device=None, backend=None,
               projection=None, field=None):
    """coloring_utils.uv_mapping: parametrise, duplicate the vertices per chart, bake the colours.
    Returns the textured mesh as a dict (verts (V',3) f64, faces (M,3) i64, uvs (V',2) f32, image
    (size,size,3) u8, name) — what trimesh.Trimesh + TextureVisuals hold in the reference.
    projection: dict(positions (V,3) in the order of v_np and in color_projection's frame,
    color_front, mask_front, color_back[, z_tolerance, erode, seam, samples, filter]) bakes with
    bake_drawings, the vertex colours being the fallback (seam "level": the fallback texels levelled
    to the drawings, the groups built from v_np, faces and vmapping; samples / filter: bake_drawings'
    samples / pixel_filter); None = the vertex colours alone.
    field: dict(positions (V,3) in the order of v_np and in the field's frame, eval_colours[,
    samples, chunk]) bakes with bake_field, the vertex colours staying where no sample is valid; with
    `projection` as well the drawings are composed over the field bake instead of the vertex bake."""
    v_np = np.asarray(v_np, np.float64).reshape(-1, 3)
    vmapping, indices, uvs = parametrize(v_np, faces, size, gutter, device=device, backend=backend)
    colours = np.asarray(vert_colors, np.float32)[vmapping]
    fallback_image = None
    if field is not None:
        fallback_image = bake_field(uvs, indices, _host(field["positions"]).reshape(-1, 3)[vmapping],
                                    field["eval_colours"], colours, size, gutter if projection is None else 0,
                                    samples=field.get("samples", 2), chunk=field.get("chunk", 1 << 21),
                                    device=device, backend=backend)
    if projection is None and field is not None:
        image = fallback_image
    elif projection is None:
        image = bake_vertex_colours(uvs, indices, colours, size, gutter, device=device, backend=backend)
    else:
        pr = projection
        seam = pr.get("seam", "none")
        groups, group_faces = seam_groups(v_np, faces, vmapping) if seam == "level" else (None, None)
        image = bake_drawings(uvs, indices, _host(pr["positions"]).reshape(-1, 3)[vmapping], pr["color_front"],
                              pr["mask_front"], pr["color_back"], colours, size, gutter,
                              z_tolerance=pr.get("z_tolerance", Z_TOLERANCE), erode=pr.get("erode", 19),
                              device=device, backend=backend, fallback_image=fallback_image, seam=seam,
                              groups=groups, group_faces=group_faces, samples=pr.get("samples", 1),
                              pixel_filter=pr.get("filter", "nearest"))
    return {"verts": v_np[vmapping], "faces": indices, "uvs": uvs, "image": image, "name": save_name}
