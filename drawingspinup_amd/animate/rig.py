"""A rig from 2-D joint marks (host, float64, around one device query): the marks of a front drawing
(AnimatedDrawings' `char_cfg.yaml`) are lifted into the mesh at the middle of its thickness under each
mark, and any BVH clip is retargeted to the lifted skeleton by the world directions of its bones.

The reference has no such step: its characters come rigged from Mixamo (blender_animation.py imports
an FBX already fitted to the character).  Placement without marks is not attempted: local fits of a
skeleton to a mesh move joints out of the limbs while they lower their energy.

    read_marks       names, parents and pixel coordinates of the marks
    pixels_to_mesh   pixel coordinates of a `<uid>/mv` front image -> xy in the exported OBJ's frame
    lift_marks       marks in the mesh's xy -> a Skeleton inside the mesh (ops.mesh_thickness)
    retarget_clip    a clip of another skeleton -> a clip of this one

Unpinned: neither Blender nor Mixamo is here to compare against; the tests hold the geometry (joints
inside the limbs, bone directions equal to the source's), not a likeness to Mixamo's rigs.
"""
import math

import numpy as np

from .skeleton import Clip, Skeleton


# ------------------------------------------------------------------ marks
def read_marks(source):
    """The joint marks of a drawing -> (names (J), parents (J,) int64 with -1 for the root, xy (J,2)
    float64 pixel coordinates, image origin top-left, x right, y down).

    `source`: the path of a file in AnimatedDrawings' `char_cfg.yaml` layout, or the dict it holds:
    `width`, `height`, `skeleton: [{name, parent, loc: [x, y]}]`, the root with `parent: null`.  The
    joints are reordered parent before child, otherwise in the file's order.  A cycle, a parent that is
    not a joint, a second root and a name given twice are refused with the joint's name."""
    cfg = _marks_dict(source)
    rows = cfg.get("skeleton")
    if not isinstance(rows, (list, tuple)) or not rows:
        raise ValueError("marks: `skeleton` must be a list of joints")
    names, parent_names, locs = [], [], []
    for row in rows:
        if not isinstance(row, dict) or "name" not in row or "loc" not in row:
            raise ValueError(f"marks: a joint needs `name`, `parent` and `loc`, found {row!r}")
        name = str(row["name"])
        if name in names:
            raise ValueError(f"marks: joint {name!r} is given twice")
        loc = np.asarray(row["loc"], np.float64).reshape(-1)
        if loc.shape != (2,) or not np.isfinite(loc).all():
            raise ValueError(f"marks: joint {name!r} needs `loc: [x, y]`")
        names.append(name)
        parent_names.append(None if row.get("parent") is None else str(row["parent"]))
        locs.append(loc)
    roots = [n for n, p in zip(names, parent_names) if p is None]
    if not roots:
        raise ValueError(f"marks: no root (a joint with `parent: null`); joint {names[0]!r} is on a cycle")
    if len(roots) > 1:
        raise ValueError(f"marks: joint {roots[1]!r} is a second root ({roots[0]!r} is the first)")
    for n, p in zip(names, parent_names):
        if p is not None and p not in names:
            raise ValueError(f"marks: joint {n!r} names the parent {p!r}, which is not a joint")
    order, placed = [], set()
    while len(order) < len(names):
        ready = [i for i, (n, p) in enumerate(zip(names, parent_names))
                 if n not in placed and (p is None or p in placed)]
        if not ready:
            left = next(n for n in names if n not in placed)
            raise ValueError(f"marks: joint {left!r} is on a cycle of parents")
        for i in ready:                       # one generation per round, in the file's order
            order.append(i)
            placed.add(names[i])
    new_index = {names[i]: k for k, i in enumerate(order)}
    out_names = [names[i] for i in order]
    parents = np.asarray([-1 if parent_names[i] is None else new_index[parent_names[i]] for i in order], np.int64)
    return out_names, parents, np.asarray([locs[i] for i in order], np.float64).reshape(-1, 2)


def marks_size(source):
    """(width, height) of the image the marks were made on (None where the file does not say)."""
    cfg = _marks_dict(source)
    return tuple(None if cfg.get(k) is None else int(cfg[k]) for k in ("width", "height"))


def _marks_dict(source):
    if isinstance(source, dict):
        return source
    import yaml
    with open(source) as fh:
        cfg = yaml.safe_load(fh)
    if not isinstance(cfg, dict):
        raise ValueError(f"{source}: a mapping with `skeleton` expected")
    return cfg


def pixels_to_mesh(xy_px, res, ortho_scale=1.35, shearing=False):
    """Pixel coordinates on a `<uid>/mv` front image of side `res` -> (n,2) float64 xy in the frame of
    the exported OBJ.

    The inverse of the pixel rule of nsr/mesh_post.get_color_from_image, pixel = ((x, -y) + 1/2)
    (res - 1), followed by what nsr/mesh.post_process_mesh applies after the colour projection: the
    shear (`shearing`: z += a y, which leaves x and y as they are, so the flag changes nothing here and
    is taken only to mirror the export's switches) and the factor `ortho_scale`.  Marks made on another
    image (AnimatedDrawings' own crop, say) are in that image's pixels: mapping them to the `<uid>/mv`
    front image first is the caller's job."""
    res = int(res)
    if res < 2:
        raise ValueError("res must be at least 2")
    del shearing
    p = np.asarray(xy_px, np.float64).reshape(-1, 2)
    out = np.empty_like(p)
    out[:, 0] = p[:, 0] / (res - 1) - 0.5
    out[:, 1] = -(p[:, 1] / (res - 1) - 0.5)
    return out * float(ortho_scale)


# ------------------------------------------------------------------ lifting
MAX_LATTICE = 4094          # + the rim of one sample on both sides = DSU_THICKNESS_MAX_SIDE
END_SITE_HALVINGS = 8


def thickness_lattice(verts, lattice=512):
    """(x0, y0, h, W, H) of the lattice lift_marks lays over a mesh: its xy bounding box grown by one
    sample on every side, h = the longer side / lattice."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    lattice = int(lattice)
    if not 1 <= lattice <= MAX_LATTICE:
        raise ValueError(f"lattice must be in 1 .. {MAX_LATTICE}")
    if not len(v) or not np.isfinite(v[:, :2]).all():
        raise ValueError("the mesh needs vertices with finite x and y")
    lo, hi = v[:, :2].min(0), v[:, :2].max(0)
    h = float(max(hi - lo)) / lattice
    if not h > 0.0:
        raise ValueError("the mesh has no extent in x and y")
    W, H = (int(math.ceil((hi[k] - lo[k]) / h)) + 2 for k in (0, 1))
    return float(lo[0] - h), float(lo[1] - h), h, min(W, lattice + 2), min(H, lattice + 2)


def lift_marks(names, parents, xy, verts, faces, lattice=512, snap=0.05, end_sites=True, device="cuda",
               backend="device"):
    """Marks in the mesh's xy (pixels_to_mesh) -> a Skeleton whose joints lie inside the mesh.

    One thickness map of the mesh along z (ops.mesh_thickness, on `device`; `backend="host"` runs the
    host entry of the same text, without a device) on thickness_lattice(verts, lattice).  A mark whose
    sample (row floor((y - y0) / h), column floor((x - x0) / h)) has thickness > 0 becomes the joint
    (x, y, mid of that sample).  Another mark moves to the centre of the nearest sample with thickness
    > 0 within `snap` times the bounding box's height (ties: smaller distance^2, then row, then
    column); with no such sample a ValueError names the joint.

    `end_sites`: a leaf joint gets an end site along its parent bone's direction in xy, half that
    bone's xy length long, halved up to 8 times until the tip's sample has thickness > 0 (none
    otherwise); the tip's z is that sample's mid.

    names, parents: as read_marks returns them (parent before child)."""
    names = list(names)
    parents = np.asarray(parents, np.int64).reshape(-1)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    if len(parents) != len(names) or len(xy) != len(names):
        raise ValueError("names, parents and xy must have one entry per joint")
    v32 = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    f32 = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3).astype(np.int32))
    x0, y0, h, W, H = thickness_lattice(v32, lattice)
    mid, thick, _ = _thickness(v32, f32, x0, y0, h, W, H, device, backend)
    height = float(v32[:, 1].astype(np.float64).max() - v32[:, 1].astype(np.float64).min())

    def sample_of(p):
        r, c = int(math.floor((p[1] - y0) / h)), int(math.floor((p[0] - x0) / h))
        return (r, c) if 0 <= r < H and 0 <= c < W and thick[r, c] > 0.0 else None

    inside = np.argwhere(thick > 0.0)                                   # (n, 2) rows, columns
    centres = np.stack([x0 + (inside[:, 1] + 0.5) * h, y0 + (inside[:, 0] + 0.5) * h], 1)
    pos = np.empty((len(names), 3))
    for j, p in enumerate(xy):
        rc = sample_of(p)
        if rc is not None:
            pos[j] = (p[0], p[1], mid[rc])
            continue
        d2 = ((centres - p) ** 2).sum(1)
        near = np.flatnonzero(d2 <= (float(snap) * height) ** 2)
        if not len(near):
            raise ValueError(f"joint {names[j]!r}: its mark is outside the mesh and no sample inside the mesh "
                             f"lies within snap = {snap} of the height")
        k = near[np.lexsort((inside[near, 1], inside[near, 0], d2[near]))[0]]
        pos[j] = (centres[k, 0], centres[k, 1], mid[inside[k, 0], inside[k, 1]])
    ends = {}
    if end_sites:
        leaves = [j for j in range(len(names)) if parents[j] >= 0 and not (parents == j).any()]
        for j in leaves:
            step = (pos[j, :2] - pos[parents[j], :2]) * 0.5
            for _ in range(END_SITE_HALVINGS + 1):
                tip = pos[j, :2] + step
                rc = sample_of(tip)
                if rc is not None and (step != 0.0).any():
                    ends[j] = np.array([tip[0], tip[1], mid[rc]]) - pos[j]
                    break
                step = step * 0.5
    offsets = pos.copy()
    offsets[1:] = pos[1:] - pos[parents[1:]]
    return Skeleton(names, parents, offsets, ends)


def _thickness(v32, f32, x0, y0, h, W, H, device, backend):
    from .. import ops
    if backend == "host":
        return ops.mesh_thickness_host(v32, f32, x0, y0, h, W, H)
    if backend != "device":
        raise ValueError(f"backend {backend!r}: 'device' or 'host'")
    import torch
    out = ops.mesh_thickness(torch.from_numpy(v32).to(device), torch.from_numpy(f32).to(device), x0, y0, h, W, H)
    return tuple(t.cpu().numpy() for t in out)


# ------------------------------------------------------------------ retargeting
HALF_TURN_BELOW = -1.0 + 1e-12


def minimal_rotation(a, b):
    """(...,3) unit vectors a, b -> (...,3,3): the rotation about a x b that takes a to b,
    I + [v]x + [v]x^2 / (1 + c) with v = a x b, c = a . b.  For c < -1 + 1e-12 (opposite vectors): the
    half turn about a x e normalised, e the coordinate axis with the smallest |a . e|."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    v = np.cross(a, b)
    c = (a * b).sum(-1)
    K = np.zeros(a.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -v[..., 2], v[..., 1]
    K[..., 1, 0], K[..., 1, 2] = v[..., 2], -v[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -v[..., 1], v[..., 0]
    half = c < HALF_TURN_BELOW
    R = np.eye(3) + K + (K @ K) / np.where(half, 1.0, 1.0 + c)[..., None, None]
    if half.any():
        e = np.eye(3)[np.abs(a).argmin(-1)]
        ax = np.cross(a, e)
        ax = ax / np.sqrt((ax * ax).sum(-1, keepdims=True))
        R = np.where(half[..., None, None], 2.0 * ax[..., :, None] * ax[..., None, :] - np.eye(3), R)
    return R


def _forward(skeleton, clip):
    """World rotations (F,J,3,3) and positions (F,J,3) of the joints in every frame."""
    J, F = skeleton.n_joints, clip.n_frames
    if clip.rotations.shape[1] != J:
        raise ValueError("the clip has another number of joints than its skeleton")
    Rw, X = np.empty((F, J, 3, 3)), np.empty((F, J, 3))
    for j in range(J):
        p = skeleton.parents[j]
        if p < 0:
            Rw[:, j], X[:, j] = clip.rotations[:, j], clip.translations
        else:
            Rw[:, j] = Rw[:, p] @ clip.rotations[:, j]
            X[:, j] = X[:, p] + Rw[:, p] @ skeleton.offsets[j]
    return Rw, X


def _unit(v):
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    return v / n, n[..., 0]


def _root_height(skeleton):
    return float(skeleton.rest_positions()[0, 1] - skeleton.rest_points()[:, 1].min())


def retarget_clip(source_skeleton, clip, target_skeleton, joint_map=None):
    """A clip of `source_skeleton` -> a Clip of `target_skeleton` in which every mapped bone points, in
    every frame, where the source's chain points in the world.

    `joint_map`: {target joint name: source joint name}; by default the names that are equal ignoring
    case.  A name that is not in its skeleton is an error, and the target's root must be mapped.

    For a mapped target joint j with source joint s, let c be j's first child (in joint order) that is
    mapped to a descendant s_c of s and lies apart from j; u_t and u_s the unit rest directions j -> c
    and s -> s_c, d_f the unit direction s -> s_c in frame f (forward kinematics of the source).  The
    target's world rotation is Q_f,j = M_f Rw_S,f[s] A_j with A_j the minimal rotation u_t -> u_s
    (minimal_rotation) and M_f the minimal rotation Rw_S,f[s] u_s -> d_f, the identity when s_c is s's
    own child (joints between s and s_c that the map skips bend the chain; M_f follows its chord).  A
    mapped joint without such a child takes its parent's A and M = I; an unmapped joint follows its
    parent (local identity).  Local rotations are Q_parent^T Q_j.  The root translation is P_T[root] +
    k (X_S,f[s_root] - P_S[s_root]), k = the target root's height above its lowest rest point (end
    sites included) over the source's, 1 where the source's is not > 0.

    A_j is not the identity where the character was drawn in another pose than the source's rest
    pose: the skinned mesh therefore deforms already at the source's rest frame.  That is the point —
    the drawn arm comes down to where the clip's arm is — and not an error of the bind.  Bone lengths
    are the target's; nothing scales a bone."""
    S, T = source_skeleton, target_skeleton
    s_index = {n: i for i, n in enumerate(S.names)}
    t_index = {n: i for i, n in enumerate(T.names)}
    if joint_map is None:
        lower = {}
        for i, n in enumerate(S.names):
            lower.setdefault(n.lower(), i)
        src = np.asarray([lower.get(n.lower(), -1) for n in T.names], np.int64)
    else:
        src = np.full(T.n_joints, -1, np.int64)
        for tn, sn in joint_map.items():
            if tn not in t_index:
                raise ValueError(f"joint_map: {tn!r} is not a joint of the target skeleton")
            if sn not in s_index:
                raise ValueError(f"joint_map: {tn!r} is mapped to {sn!r}, which is not a joint of the source skeleton")
            src[t_index[tn]] = s_index[sn]
    if src[0] < 0:
        raise ValueError(f"the target's root {T.names[0]!r} is not mapped to a source joint")
    Rw, X = _forward(S, clip)
    F = clip.n_frames
    PS, PT = S.rest_positions(), T.rest_positions()

    def descends(a, b):                      # source joint a strictly below b
        a = S.parents[a]
        while a >= 0:
            if a == b:
                return True
            a = S.parents[a]
        return False

    A = np.empty((T.n_joints, 3, 3))
    Q = np.empty((F, T.n_joints, 3, 3))
    for j in range(T.n_joints):
        p, s = T.parents[j], src[j]
        A[j] = A[p] if p >= 0 else np.eye(3)
        if s < 0:
            Q[:, j] = Q[:, p]
            continue
        M = None
        for c in np.flatnonzero(T.parents == j):
            sc = src[c]
            if sc < 0 or not descends(sc, s):
                continue
            u_t, len_t = _unit(PT[c] - PT[j])
            u_s, len_s = _unit(PS[sc] - PS[s])
            if not (len_t > 0.0 and len_s > 0.0):
                continue
            A[j] = minimal_rotation(u_t, u_s)
            if S.parents[sc] != s:
                d, len_d = _unit(X[:, sc] - X[:, s])
                if (len_d > 0.0).all():
                    M = minimal_rotation(Rw[:, s] @ u_s, d)
            break
        Q[:, j] = Rw[:, s] @ A[j] if M is None else M @ Rw[:, s] @ A[j]
    rot = np.empty_like(Q)
    for j in range(T.n_joints):
        p = T.parents[j]
        rot[:, j] = Q[:, j] if p < 0 else np.swapaxes(Q[:, p], -1, -2) @ Q[:, j]
    hs = _root_height(S)
    k = _root_height(T) / hs if hs > 0.0 else 1.0
    tr = PT[0] + k * (X[:, src[0]] - PS[src[0]])
    return Clip(tr, rot, clip.frame_time)
