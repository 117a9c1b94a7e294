"""Automatic skinning weights (bone heat) and the skinned render: skeleton + clip -> (F,V,3) on the
device -> the frames of render_frames.

The weighting follows the published bone-heat form (Baran & Popovic 2007), not Blender's source
(blender_animation.py:38-44 calls paint.weight_from_bones(type='AUTOMATIC')): for every vertex the
nearest visible bones are its heat sources, and the weights W solve (L + M H) W = M H P with the
cotangent stiffness L, the lumped mass M, h_i = 1 / d_i^2 and p_ij = 1 / n_i on the n_i nearest
visible bones.  Distances and visibility (ops.bone_visibility) and the solve (ops.spd_cg_block) run
on the device; the system is assembled here, once per character.
"""
import numpy as np
import torch

from .. import ops
from ..nsr.thinning import _weld, cotmatrix
from .corrective import check_parameters, smoothing_topology
from .render import _pixel_filter_args, _texture_args, _vertex_colours, frame_window, position_colours
from .skeleton import dual_quaternions, rotation_quaternions, skinning_matrices

SKINNING = ("linear", "dual_quaternion", "centre_of_rotation")
COR_SIGMA = 0.1      # width of the weight similarity of the centres of rotation (Le & Hodgins 2016)
NEAR = 1e-4          # bones within (1 + NEAR) of the nearest visible one share a vertex's heat
D_FLOOR = 1e-6       # d_i is taken no smaller than this fraction of the bounding-box diagonal


def lumped_mass(v, f):
    """A third of the incident triangle area per vertex (barycentric lumping)."""
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    m = np.zeros(len(v))
    np.add.at(m, f.ravel(), np.repeat(area / 3.0, 3))
    return m


def components(n, f):
    """Connected-component label per vertex of the mesh graph."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    return connected_components(g, directed=False)[1]


def heat_sources(dist, visible, labels, floor):
    """-> (P (n,B), h (n,), fallback component labels).  A component in which no vertex sees any bone
    ignores visibility (its block of the system would be singular otherwise)."""
    vis = np.asarray(visible).astype(bool).copy()
    sees = np.zeros(labels.max() + 1, bool)
    np.logical_or.at(sees, labels, vis.any(1))
    blind = np.flatnonzero(~sees)
    vis[np.isin(labels, blind)] = True
    d = np.where(vis, dist, np.inf)
    dmin = d.min(1)
    has = np.isfinite(dmin)
    near = vis & (dist <= (1.0 + NEAR) * dmin[:, None])
    n = near.sum(1)
    P = near / np.maximum(n, 1)[:, None]
    h = np.zeros(len(dist))
    h[has] = 1.0 / np.maximum(dmin[has], floor) ** 2
    return P, h, blind


def heat_system(v, f, P, h):
    """(A csr with sorted indices, rhs (n,B)) of (L + M H) W = M H P."""
    import scipy.sparse as sp
    L = -cotmatrix(v, f)
    mh = lumped_mass(v, f) * h
    A = (L + sp.diags(mh)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A, mh[:, None] * P


def finish_weights(W, heads, K=4):
    """Clamp negative weights to 0, keep the K largest per vertex (None: all; ties go to the lower
    bone index), renormalise to sum 1, and hand each bone's weight to the joint at its head.
    -> influences (V,K) int32, weights (V,K) float32."""
    W = np.maximum(np.asarray(W, np.float64), 0.0)
    B = W.shape[1]
    K = B if K is None else int(min(max(K, 1), B))
    top = np.argsort(-W, axis=1, kind="stable")[:, :K]
    w = np.take_along_axis(W, top, 1)
    s = w.sum(1, keepdims=True)
    w = np.where(s > 0, w / np.where(s > 0, s, 1.0), np.eye(1, K))       # nothing left: all on the first
    return np.asarray(heads, np.int64)[top].astype(np.int32), w.astype(np.float32)


@torch.no_grad()
def bone_heat_weights(verts, faces, skeleton, K=4, device="cuda", tol=1e-10, max_iters=20000,
                      return_info=False):
    """Bone-heat skinning weights of a mesh for a skeleton placed inside it (fit_to_mesh scales and
    centres one; it does not place joints inside limbs).  verts (V,3), faces (M,3) 0-based.
    -> influences (V,K) int32 joint indices, weights (V,K) float32 summing to 1 per vertex
    (numpy).  return_info adds a dict: the full (V,B) float64 weights, iterations, residuals, the
    distances and visibility, the bone heads."""
    dev = torch.device(device)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    heads, segs = skeleton.bones()
    if not len(heads):
        raise ValueError("the skeleton has no bone")
    # coincident vertices are solved as one, zero-area triangles left out (nsr/thinning._weld)
    rep, g = _weld(v, f)
    used = np.zeros(len(v), bool)
    used[g.ravel()] = True
    idx = np.flatnonzero(used)
    new = np.full(len(v), -1, np.int64)
    new[idx] = np.arange(len(idx))
    vc, fc = v[idx], new[g]
    if not len(fc):
        raise ValueError("the mesh has no triangle with an area")
    dist, vis = ops.bone_visibility(torch.from_numpy(vc.astype(np.float32)).to(dev),
                                    torch.from_numpy(fc.astype(np.int32)).to(dev),
                                    torch.from_numpy(segs.astype(np.float32)).to(dev))
    dist, vis = dist.cpu().numpy(), vis.cpu().numpy()
    floor = D_FLOOR * float(np.linalg.norm(vc.max(0) - vc.min(0)))
    P, h, blind = heat_sources(dist, vis, components(len(vc), fc), floor)
    A, rhs = heat_system(vc.astype(np.float32).astype(np.float64), fc, P, h)
    W, iters, res = ops.spd_cg_block(torch.from_numpy(A.indptr.astype(np.int32)).to(dev),
                                     torch.from_numpy(A.indices.astype(np.int32)).to(dev),
                                     torch.from_numpy(A.data).to(dev), torch.from_numpy(rhs).to(dev),
                                     x0=torch.from_numpy(P).to(dev), tol=tol, max_iters=max_iters)
    if iters >= max_iters and not (res <= tol).all():
        raise RuntimeError(f"bone-heat solve did not converge in {max_iters} iterations (residual {res.max():.3e})")
    Wc = W.cpu().numpy()
    Wfull = np.zeros((len(v), len(heads)))
    has = new[rep] >= 0
    Wfull[has] = Wc[new[rep[has]]]
    if not has.all():
        # a vertex without any triangle: everything on the nearest bone
        lone = np.flatnonzero(~has)
        a, b = segs[:, 0], segs[:, 1]
        ab = b - a
        t = np.clip(((v[lone, None] - a) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0, 1)
        dd = np.linalg.norm(a + t[..., None] * ab - v[lone, None], axis=-1)
        Wfull[lone, dd.argmin(1)] = 1.0
    infl, w = finish_weights(Wfull, heads, K)
    if return_info:
        return infl, w, {"W": Wfull, "iterations": iters, "residuals": res, "dist": dist, "visible": vis,
                         "heads": heads, "fallback_components": blind, "compact": idx}
    return infl, w


@torch.no_grad()
def cor_centres(verts, faces, weights, n_joints, device="cuda", sigma=COR_SIGMA):
    """The centres of rotation of a rigged mesh (ops.skin_cor_centres; Le & Hodgins, "Real-time
    skeletal skinning with optimized centers of rotation", 2016), once per character: for every
    vertex the area-weighted mean of the centroids of the triangles whose weights resemble its own,
    a sum over all (vertex, triangle) pairs on the device.  verts (V,3), faces (T,3) 0-based, weights
    = (influences, weights) as bone_heat_weights returns them, n_joints of the skeleton.
    -> (centres (V,3) float64, valid (V,) uint8) on the device; a vertex on one joint alone has none
    (valid 0) and is blended linearly.  They depend on the rest mesh and the weights only, so one
    result serves every clip: animate_mesh(centres=...)."""
    dev = torch.device(device)
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    v = to_np(verts).astype(np.float32).reshape(-1, 3)
    f = to_np(faces).astype(np.int32).reshape(-1, 3)
    infl, w = (to_np(a) for a in weights)
    return ops.skin_cor_centres(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), infl, w, int(n_joints),
                                sigma=float(sigma))


@torch.no_grad()
def animate_mesh(verts, faces, colours, skeleton, clip, weights=None, ss=4, device="cuda", K=4, want=(),
                 texture=None, uvs=None, texture_filter="bilinear", mip_coverage="faces", skinning="linear",
                 corrective_iterations=0, corrective_factor=0.5, pixel_filter=None, filter_width=None,
                 centres=None, cor_sigma=COR_SIGMA, max_anisotropy=None):
    """Render a skinned animation of one mesh: weights (bone heat unless given as (influences,
    weights)), skinning on the device, then the rasteriser of render_frames.  skinning: "linear"
    blends the joints' matrices (ops.skin_lbs, Blender's default), "dual_quaternion" their unit dual
    quaternions (ops.skin_dqs, Blender's "Preserve Volume": a twisted or bent limb keeps its
    radius), "centre_of_rotation" the joints' rotation quaternions about a centre of rotation per
    vertex that itself moves by the linear blend (ops.skin_cor, Le & Hodgins 2016: the radius is kept
    and the outside of a sharp bend does not bulge); the weights are the same for all three.
    centres: the (centres, valid) of cor_centres for this mesh and these weights; None computes them
    with cor_sigma (once per call), and the result carries them as `cor_centres` for the next clip.
    The other blends ignore both.  Under a rest clip a vertex with a centre returns its rest position
    bit for bit; one without (a single joint, or joints no triangle shares) takes the linear blend.
    The skinned vertices never leave the device; the
    window is frame_window's rule on their bounding box over all frames (Blender uses the object's
    bound_box).  texture, uvs, texture_filter, max_anisotropy, mip_coverage, pixel_filter, filter_width: as in
    render_frames (colours may be None with a texture).
    corrective_iterations N > 0 runs the corrective smoothing (delta mush,
    ops.corrective_smooth: N smoothing steps of strength corrective_factor, then the rest mesh's
    detail put back) on the skinned vertices of either blend: it repairs the creases that wrong or
    abruptly changing weights leave at a joint; the topology and the bind are computed once per call
    from the rest mesh, and window and `vertices` are taken from the corrected tensor.  0 (default)
    is off.

    Returns the dictionary of render_frames plus `vertices`, the (F,V,3) device tensor (and
    `cor_centres` with skinning="centre_of_rotation")."""
    if skinning not in SKINNING:
        raise ValueError(f"skinning {skinning!r}: one of {SKINNING}")
    check_parameters(corrective_iterations, corrective_factor)
    dev = torch.device(device)
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    v = to_np(verts).astype(np.float64).reshape(-1, 3)
    f = to_np(faces).astype(np.int64).reshape(-1, 3)
    tex = _texture_args(texture, uvs, texture_filter, len(v), dev, f, mip_coverage, max_anisotropy)
    tex.update(_pixel_filter_args(pixel_filter, filter_width, ss))
    c = _vertex_colours(colours, len(v), texture is not None)
    if weights is None:
        weights = bone_heat_weights(v, f, skeleton, K=K, device=device)
    infl, w = (to_np(a) for a in weights)
    rest, ti, tw = (torch.from_numpy(a).to(dev) for a in (v.astype(np.float32), infl.astype(np.int32),
                                                          w.astype(np.float32)))
    if skinning == "linear":
        mats = skinning_matrices(skeleton, clip).astype(np.float32)
        screen = ops.skin_lbs(rest, ti, tw, torch.from_numpy(mats).to(dev))
    elif skinning == "dual_quaternion":
        screen = ops.skin_dqs(rest, ti, tw, torch.from_numpy(dual_quaternions(skinning_matrices(skeleton, clip))).to(dev))
    else:
        mats = skinning_matrices(skeleton, clip)
        if centres is None:
            centres = cor_centres(v, f, (infl, w), mats.shape[1], device=dev, sigma=cor_sigma)
        centres = tuple(a.to(dev) for a in centres)
        screen = ops.skin_cor(rest, ti, tw, torch.from_numpy(mats).to(dev),
                              torch.from_numpy(rotation_quaternions(mats[..., :3])).to(dev), *centres)
    if corrective_iterations:
        topology = ops.corrective_topology(smoothing_topology(v, f), dev)
        delta, valid = ops.corrective_bind(rest, topology, corrective_factor, corrective_iterations)
        screen = ops.corrective_smooth(screen, topology, delta, valid, corrective_factor, corrective_iterations)
    box = torch.stack([screen.amin((0, 1)), screen.amax((0, 1))]).cpu().numpy()
    cx, cy, size, span = frame_window(box)
    pos = torch.from_numpy(position_colours(v).astype(np.float32)).to(dev)
    out = ops.mesh_render_ortho(screen, torch.from_numpy(f).to(dev), None if c is None else torch.from_numpy(c).to(dev),
                                pos, cx, cy, span, size, ss, want=("color_u8", "pos_u8", "frames", *want), **tex)
    res = {"color": out["color_u8"], "pos": out["pos_u8"], "edge": ops.pos_edge_u8(out["pos_u8"]),
           "frames": out["frames"], "size": int(size), "span": float(span), "centre": (cx, cy),
           "vertices": screen}
    if skinning == "centre_of_rotation":
        res["cor_centres"] = centres
    res.update({k: out[k] for k in want})
    return res
