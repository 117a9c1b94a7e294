"""Skeleton and motion clip of a rigged animation (host, float64): a BVH reader, the fit of a
skeleton to a mesh's bounding box and the per-frame skinning matrices.

The reference binds a Mixamo FBX armature inside Blender (blender_animation.py:10-44) and has no
reader of its own; FBX is a binary, proprietary format and stays out.  BVH is plain text: a
HIERARCHY of ROOT / JOINT / End Site blocks with OFFSET and CHANNELS, then MOTION with one line of
channel values per frame.
"""
import math
import os

import numpy as np


class Skeleton:
    """names (J), parents (J, -1 for the root, parent before child), offsets (J,3) from the parent
    (the root's: its rest position).  end_sites: {joint: offset} of the End Site of a leaf joint.

    A bone is the segment joint -> child joint; an end site gives a leaf joint a bone; a joint with
    neither a child nor an end site has none."""

    def __init__(self, names, parents, offsets, end_sites=None):
        self.names = list(names)
        self.parents = np.asarray(parents, np.int64).reshape(-1)
        self.offsets = np.asarray(offsets, np.float64).reshape(-1, 3).copy()
        self.end_sites = {int(j): np.asarray(o, np.float64).reshape(3).copy() for j, o in (end_sites or {}).items()}
        J = len(self.names)
        if len(self.parents) != J or len(self.offsets) != J or J < 1:
            raise ValueError("names, parents and offsets must have one entry per joint")
        if self.parents[0] != -1 or any(not (0 <= self.parents[j] < j) for j in range(1, J)):
            raise ValueError("joints must come parent before child, the root first")
        if any(not (0 <= j < J) for j in self.end_sites):
            raise ValueError("end site on a joint that does not exist")

    @property
    def n_joints(self):
        return len(self.names)

    def rest_positions(self):
        """(J,3) world positions of the joints in the rest pose."""
        pos = np.zeros((self.n_joints, 3))
        for j in range(self.n_joints):
            pos[j] = self.offsets[j] + (pos[self.parents[j]] if self.parents[j] >= 0 else 0.0)
        return pos

    def rest_points(self):
        """Joint positions followed by the end-site tips (in joint order)."""
        pos = self.rest_positions()
        tips = [pos[j] + self.end_sites[j] for j in sorted(self.end_sites)]
        return np.concatenate([pos, np.asarray(tips).reshape(-1, 3)])

    def bones(self):
        """(heads (B,) joint at the head of each bone, segments (B,2,3) head and tail in the rest
        pose).  Order: by head joint; its children in joint order, then its end site."""
        pos = self.rest_positions()
        heads, segs = [], []
        for j in range(self.n_joints):
            for c in range(j + 1, self.n_joints):
                if self.parents[c] == j:
                    heads.append(j); segs.append([pos[j], pos[c]])
            if j in self.end_sites:
                heads.append(j); segs.append([pos[j], pos[j] + self.end_sites[j]])
        return np.asarray(heads, np.int64), np.asarray(segs, np.float64).reshape(-1, 2, 3)


class Clip:
    """translations (F,3): the root's position per frame; rotations (F,J,3,3): every joint's local
    rotation; float64.  frame_time in seconds."""

    def __init__(self, translations, rotations, frame_time=1.0 / 30.0):
        self.translations = np.asarray(translations, np.float64).reshape(-1, 3).copy()
        self.rotations = np.asarray(rotations, np.float64).copy()
        self.frame_time = float(frame_time)
        if self.rotations.ndim != 4 or self.rotations.shape[2:] != (3, 3) or \
                self.rotations.shape[0] != len(self.translations):
            raise ValueError("translations (F,3) and rotations (F,J,3,3) expected")

    @property
    def n_frames(self):
        return len(self.translations)

    def resample(self, frame_time):
        """This clip at another frame time (resample_clip)."""
        return resample_clip(self, frame_time)


def rest_clip(skeleton, n_frames=1):
    """The clip that leaves the skeleton in its rest pose."""
    rot = np.broadcast_to(np.eye(3), (n_frames, skeleton.n_joints, 3, 3))
    return Clip(np.broadcast_to(skeleton.offsets[0], (n_frames, 3)), rot)


def axis_rotation(axis, degrees):
    """Right-handed rotation about 'X' | 'Y' | 'Z' by an angle in degrees."""
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    if axis == "X":
        return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    if axis == "Y":
        return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    if axis == "Z":
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    raise ValueError(f"axis {axis!r}")


def read_bvh(path):
    """-> (Skeleton, Clip).  HIERARCHY with ROOT / JOINT / End Site, OFFSET, CHANNELS with 3 or 6
    channels in any rotation order (the rotations compose in channel order: `Zrotation Xrotation
    Yrotation` is Rz Rx Ry, angles in degrees); MOTION with `Frames:` and `Frame Time:`.  The position
    channels of the root are its translation; a joint without them keeps its OFFSET, and position
    channels of other joints are read and ignored."""
    with open(path) as fh:
        tok = fh.read().split()
    pos = 0

    def take():
        nonlocal pos
        if pos >= len(tok):
            raise ValueError(f"{path}: unexpected end of file")
        pos += 1
        return tok[pos - 1]

    def expect(word):
        t = take()
        if t.upper() != word.upper():
            raise ValueError(f"{path}: expected {word!r}, found {t!r}")

    names, parents, offsets, channels, ends = [], [], [], [], {}

    def joint(parent):
        j = len(names)
        names.append(take()); parents.append(parent); offsets.append(None); channels.append([])
        expect("{")
        while True:
            t = take()
            u = t.upper()
            if u == "OFFSET":
                offsets[j] = [float(take()) for _ in range(3)]
            elif u == "CHANNELS":
                n = int(take())
                if n not in (3, 6):
                    raise ValueError(f"{path}: joint {names[j]} has {n} channels (3 or 6 expected)")
                channels[j] = [take() for _ in range(n)]
            elif u == "JOINT":
                joint(j)
            elif u == "END":
                expect("Site"); expect("{"); expect("OFFSET")
                ends[j] = [float(take()) for _ in range(3)]
                expect("}")
            elif u == "}":
                break
            else:
                raise ValueError(f"{path}: unexpected {t!r} in joint {names[j]}")
        if offsets[j] is None:
            raise ValueError(f"{path}: joint {names[j]} has no OFFSET")

    expect("HIERARCHY"); expect("ROOT")
    joint(-1)
    expect("MOTION"); expect("Frames:")
    F = int(take())
    expect("Frame"); expect("Time:")
    dt = float(take())
    width = sum(len(c) for c in channels)
    vals = np.asarray([float(x) for x in tok[pos:pos + F * width]], np.float64)
    if len(vals) != F * width:
        raise ValueError(f"{path}: {len(vals)} motion values, {F} frames of {width} expected")
    vals = vals.reshape(F, width)
    skel = Skeleton(names, parents, offsets, ends)
    J = len(names)
    tr = np.broadcast_to(skel.offsets[0], (F, 3)).copy()
    rot = np.broadcast_to(np.eye(3), (F, J, 3, 3)).copy()
    col = 0
    for j in range(J):
        for ch in channels[j]:
            kind, axis = ch[1:].lower(), ch[0].upper()
            if axis not in "XYZ" or kind not in ("position", "rotation"):
                raise ValueError(f"{path}: channel {ch!r}")
            if kind == "position":
                if j == 0:
                    tr[:, "XYZ".index(axis)] = vals[:, col]
            else:
                for f in range(F):
                    rot[f, j] = rot[f, j] @ axis_rotation(axis, vals[f, col])
            col += 1
    skel.channels = channels
    return skel, Clip(tr, rot, dt)


def fit_to_mesh(skeleton, clip, verts):
    """One uniform scale and one translation of the skeleton (joints and end-site tips) and of the
    clip's root translations, so that the rest skeleton's height equals the mesh's y extent, it is
    centred in x and z on the mesh's bounding box and its lowest point sits at the mesh's lowest y.

    A convenience, not an auto-rigger: it does not move joints relative to each other.  Placing the
    joints inside the limbs of the character remains the caller's job."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    pts = skeleton.rest_points()
    plo, phi = pts.min(0), pts.max(0)
    height = phi[1] - plo[1]
    if not height > 0:
        raise ValueError("the skeleton has no height")
    s = (hi[1] - lo[1]) / height
    shift = np.array([(lo[0] + hi[0]) / 2 - s * (plo[0] + phi[0]) / 2, lo[1] - s * plo[1],
                      (lo[2] + hi[2]) / 2 - s * (plo[2] + phi[2]) / 2])
    off = skeleton.offsets * s
    off[0] = off[0] + shift
    fitted = Skeleton(skeleton.names, skeleton.parents, off, {j: o * s for j, o in skeleton.end_sites.items()})
    return fitted, Clip(clip.translations * s + shift, clip.rotations, clip.frame_time)


def skinning_matrices(skeleton, clip):
    """(F,J,3,4) float64: the world transform of every joint in every frame times the inverse of its
    rest transform — what takes a rest-pose point bound to the joint to its place in the frame."""
    J, F = skeleton.n_joints, clip.n_frames
    if clip.rotations.shape[1] != J:
        raise ValueError("the clip has another number of joints than the skeleton")
    rest = skeleton.rest_positions()
    Rw = np.empty((F, J, 3, 3))
    tw = np.empty((F, J, 3))
    for j in range(J):
        p = skeleton.parents[j]
        if p < 0:
            Rw[:, j] = clip.rotations[:, j]
            tw[:, j] = clip.translations
        else:
            Rw[:, j] = Rw[:, p] @ clip.rotations[:, j]
            tw[:, j] = tw[:, p] + Rw[:, p] @ skeleton.offsets[j]
    out = np.empty((F, J, 3, 4))
    out[..., :3] = Rw
    out[..., 3] = tw - np.einsum("fjab,jb->fja", Rw, rest)
    return out


def rotation_quaternions(R):
    """(...,3,3) rotations -> (...,4) unit quaternions (w, x, y, z) with w >= 0 (w = 0: the first
    non-zero component positive).  The branch is chosen by the largest of the trace and the diagonal
    entries (Shepperd), so that a rotation near 180 degrees keeps its digits."""
    R = np.asarray(R, np.float64)
    if R.shape[-2:] != (3, 3):
        raise ValueError("rotations (...,3,3) expected")
    m = R.reshape(-1, 3, 3)
    d0, d1, d2 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    branch = np.stack([d0 + d1 + d2, d0, d1, d2], 1).argmax(1)
    q = np.empty((len(m), 4))
    for b in range(4):
        i = np.flatnonzero(branch == b)
        if not len(i):
            continue
        a = m[i]
        if b == 0:
            s = 2.0 * np.sqrt(np.maximum(1.0 + a[:, 0, 0] + a[:, 1, 1] + a[:, 2, 2], 0.0))          # 4 w
            q[i] = np.stack([s / 4.0, (a[:, 2, 1] - a[:, 1, 2]) / s, (a[:, 0, 2] - a[:, 2, 0]) / s,
                             (a[:, 1, 0] - a[:, 0, 1]) / s], 1)
        elif b == 1:
            s = 2.0 * np.sqrt(np.maximum(1.0 + a[:, 0, 0] - a[:, 1, 1] - a[:, 2, 2], 0.0))          # 4 x
            q[i] = np.stack([(a[:, 2, 1] - a[:, 1, 2]) / s, s / 4.0, (a[:, 0, 1] + a[:, 1, 0]) / s,
                             (a[:, 0, 2] + a[:, 2, 0]) / s], 1)
        elif b == 2:
            s = 2.0 * np.sqrt(np.maximum(1.0 + a[:, 1, 1] - a[:, 0, 0] - a[:, 2, 2], 0.0))          # 4 y
            q[i] = np.stack([(a[:, 0, 2] - a[:, 2, 0]) / s, (a[:, 0, 1] + a[:, 1, 0]) / s, s / 4.0,
                             (a[:, 1, 2] + a[:, 2, 1]) / s], 1)
        else:
            s = 2.0 * np.sqrt(np.maximum(1.0 + a[:, 2, 2] - a[:, 0, 0] - a[:, 1, 1], 0.0))          # 4 z
            q[i] = np.stack([(a[:, 1, 0] - a[:, 0, 1]) / s, (a[:, 0, 2] + a[:, 2, 0]) / s,
                             (a[:, 1, 2] + a[:, 2, 1]) / s, s / 4.0], 1)
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    q = q + 0.0                                                      # -0 -> +0
    lead = np.take_along_axis(q, (q != 0.0).argmax(1)[:, None], 1)   # the first non-zero component
    return np.where(lead < 0.0, -q, q).reshape(R.shape[:-2] + (4,)) + 0.0


def quaternion_rotations(q):
    """(...,4) unit quaternions (w, x, y, z) -> (...,3,3) rotations; the inverse of
    rotation_quaternions."""
    q = np.asarray(q, np.float64)
    if q.shape[-1] != 4:
        raise ValueError("quaternions (...,4) expected")
    w, x, y, z = (q[..., c] for c in range(4))
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1.0 - 2.0 * (y * y + z * z)
    R[..., 0, 1] = 2.0 * (x * y - w * z)
    R[..., 0, 2] = 2.0 * (x * z + w * y)
    R[..., 1, 0] = 2.0 * (x * y + w * z)
    R[..., 1, 1] = 1.0 - 2.0 * (x * x + z * z)
    R[..., 1, 2] = 2.0 * (y * z - w * x)
    R[..., 2, 0] = 2.0 * (x * z - w * y)
    R[..., 2, 1] = 2.0 * (y * z + w * x)
    R[..., 2, 2] = 1.0 - 2.0 * (x * x + y * y)
    return R


def dual_quaternions(matrices):
    """(F,J,3,4) rigid transforms [R | t] -> (F,J,8) float64 [r_w r_x r_y r_z | d_w d_x d_y d_z]: the
    unit rotation quaternion r of R and the dual part d = 1/2 (0, t) (x) r — the table of
    ops.skin_dqs.  ValueError when a matrix is not rigid (|R^T R - I| above 1e-9, or det < 0):
    skinning_matrices is rigid by construction, so this guards matrices made elsewhere."""
    m = np.asarray(matrices, np.float64)
    if m.ndim != 4 or m.shape[2:] != (3, 4):
        raise ValueError("matrices (F,J,3,4) expected")
    R, t = m[..., :3], m[..., 3]
    if m.size:
        err = np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max()
        if not err <= 1e-9 or not (np.linalg.det(R) > 0.0).all():
            raise ValueError(f"dual quaternions need rigid transforms (|R^T R - I| = {err:.3e}, "
                             f"smallest determinant {np.linalg.det(R).min():.3f})")
    r = rotation_quaternions(R)
    w, v = r[..., :1], r[..., 1:]
    out = np.empty(m.shape[:2] + (8,))
    out[..., :4] = r
    out[..., 4] = -0.5 * (t * v).sum(-1)
    out[..., 5:] = 0.5 * (w * t + np.cross(t, v))
    return out + 0.0                                                 # -0 -> +0


SLERP_LINEAR_BELOW = 1e-8       # radians: below this angle two quaternions are lerped and normalised


def resample_clip(clip, frame_time):
    """The clip at the times k frame_time, k = 0 .. floor(T / frame_time), T = (F - 1)
    clip.frame_time.  The root translations are interpolated linearly; every joint's local rotation
    by slerp between the two neighbouring frames, along the shorter arc (the quaternions' signs are
    aligned first; below an angle of 1e-8 they are lerped and normalised).  A time that coincides
    with a source frame (its quotient by clip.frame_time is an integer in float64) copies that
    frame unchanged, so the clip's own frame_time returns equal arrays.  A one-frame clip is
    returned as it is."""
    ft = float(frame_time)
    if not (ft > 0.0 and math.isfinite(ft)):
        raise ValueError("frame_time must be positive")
    F = clip.n_frames
    if F <= 1:
        return clip
    # in units of the clip's frames: time k ft is frame k ratio, and T / ft = (F - 1) / ratio.  The own
    # rate (ratio 1) and whole multiples of it give whole frames exactly
    ratio = ft / clip.frame_time
    n = int(math.floor((F - 1) / ratio)) + 1
    u = np.arange(n) * ratio
    i0 = np.minimum(np.floor(u).astype(np.int64), F - 1)
    i1 = np.minimum(i0 + 1, F - 1)
    a = u - i0
    exact = a == 0.0
    tr = (1.0 - a)[:, None] * clip.translations[i0] + a[:, None] * clip.translations[i1]
    q0, q1 = rotation_quaternions(clip.rotations[i0]), rotation_quaternions(clip.rotations[i1])
    dot = (q0 * q1).sum(-1, keepdims=True)
    q1 = np.where(dot < 0.0, -q1, q1)
    theta = np.arccos(np.clip(np.abs(dot), 0.0, 1.0))
    al = a[:, None, None]
    small = theta < SLERP_LINEAR_BELOW
    st = np.where(small, 1.0, np.sin(theta))
    k0 = np.where(small, 1.0 - al, np.sin((1.0 - al) * theta) / st)
    k1 = np.where(small, al, np.sin(al * theta) / st)
    q = k0 * q0 + k1 * q1
    rot = quaternion_rotations(q / np.sqrt((q * q).sum(-1, keepdims=True)))
    tr[exact] = clip.translations[i0[exact]]
    rot[exact] = clip.rotations[i0[exact]]
    return Clip(tr, rot, ft)


def bvh_files(folder):
    """Sorted *.bvh under a folder ([] when it does not exist)."""
    if not os.path.isdir(folder):
        return []
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(".bvh"))
