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


def bvh_files(folder):
    """Sorted *.bvh under a folder ([] when it does not exist)."""
    if not os.path.isdir(folder):
        return []
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(".bvh"))
