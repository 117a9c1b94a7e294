"""A rig from marks without a GPU (drawingspinup_amd/animate/rig.py, the thickness map through
backend="host"): the marks reader, the pixel rule's inverse, the lift of 16 marks into a tube character
of boxes, and retargeting.

Retargeting is held to 1e-12 throughout: a chain of at most 50 float64 3x3 products at 4 ulp each is
about 4e-14, and the bound is 25 times that.  (`run_render --marks` needs the device for its frames:
tests/test_gpu_mesh_thickness.py runs it.)"""
import numpy as np
import pytest
import torch

import rig_cases as RC
from drawingspinup_amd import animate, ops
from drawingspinup_amd.animate import Skeleton, rig

BOUND = 1e-12


# ------------------------------------------------------------------ marks
def _cfg(rows, width=400, height=400):
    return {"width": width, "height": height, "skeleton": [dict(name=n, parent=p, loc=list(l)) for n, p, l in rows]}


def _rows():
    xy = np.arange(32, dtype=np.float64).reshape(16, 2) * 7.0 + 3.0
    return [(n, None if p < 0 else RC.NAMES[p], xy[i]) for i, (n, p) in enumerate(zip(RC.NAMES, RC.PARENTS))]


def test_read_marks_orders_parent_before_child(tmp_path):
    import yaml
    rows = _rows()
    shuffled = [rows[i] for i in (6, 5, 4, 15, 3, 2, 1, 0, 9, 8, 7, 12, 11, 10, 14, 13)]      # children first
    path = tmp_path / "char_cfg.yaml"
    path.write_text(yaml.safe_dump(_cfg([(n, p, [float(v) for v in l]) for n, p, l in shuffled])))
    names, parents, xy = animate.read_marks(str(path))
    assert sorted(names) == sorted(RC.NAMES) and names[0] == "root" and parents[0] == -1
    assert parents.dtype == np.int64 and xy.shape == (16, 2) and xy.dtype == np.float64
    want_parent = {n: (None if p < 0 else RC.NAMES[p]) for n, p in zip(RC.NAMES, RC.PARENTS)}
    want_xy = {n: l for n, _, l in rows}
    for j, n in enumerate(names):
        assert (want_parent[n] is None) == (parents[j] < 0)
        if parents[j] >= 0:
            assert parents[j] < j and names[parents[j]] == want_parent[n]
        assert (xy[j] == want_xy[n]).all()
    # a generation at a time, each in the file's order
    assert names[:4] == ["root", "hip", "right_hip", "left_hip"]
    Skeleton(names, parents, np.zeros((16, 3)))                         # the order a Skeleton asks for
    again = animate.read_marks(_cfg(shuffled))                          # a plain dict
    assert again[0] == names and (again[1] == parents).all() and (again[2] == xy).all()
    assert rig.marks_size(str(path)) == (400, 400)


def test_read_marks_refuses_what_is_no_tree():
    rows = _rows()
    cyc = [(n, ("left_foot" if n == "left_hip" else p), l) for n, p, l in rows]
    with pytest.raises(ValueError, match="left_(hip|knee|foot).*cycle"):
        animate.read_marks(_cfg(cyc))
    with pytest.raises(ValueError, match="'neck'.*'spine9'"):
        animate.read_marks(_cfg([(n, ("spine9" if n == "neck" else p), l) for n, p, l in rows]))
    with pytest.raises(ValueError, match="'torso'.*second root"):
        animate.read_marks(_cfg([(n, (None if n == "torso" else p), l) for n, p, l in rows]))
    with pytest.raises(ValueError, match="'hip'.*twice"):
        animate.read_marks(_cfg(rows + [("hip", "root", (1.0, 2.0))]))
    with pytest.raises(ValueError, match="no root.*'root'"):
        animate.read_marks(_cfg([(n, ("left_foot" if n == "root" else p), l) for n, p, l in rows]))


def test_pixels_to_mesh_inverts_the_export():
    """Vertices through the export (post_process_mesh: its projection frame, then shear and
    ortho_scale) and through the pixel rule of get_color_from_image before its rounding; from the
    pixels pixels_to_mesh must land on the exported x and y.  8 ulp of the largest coordinate."""
    from drawingspinup_amd.nsr.mesh import post_process_mesh
    rng = np.random.default_rng(2)
    v = torch.from_numpy(rng.uniform(-0.95, 0.95, size=(200, 3)))
    f = torch.from_numpy(rng.integers(0, 200, size=(50, 3)))
    for res, scale in ((2048, 1.35), (1024, 1.0)):
        out, _, _, frame = post_process_mesh(v, f, ortho_scale=scale, shearing=True, return_projection_frame=True)
        px = (np.stack([frame[:, 0], -frame[:, 1]], 1) + 0.5) * (res - 1)
        got = animate.pixels_to_mesh(px, res, ortho_scale=scale, shearing=True)
        assert got.shape == (200, 2) and np.abs(got - out[:, :2]).max() <= 8 * 2.0 ** -52 * np.abs(out).max()
    centre = animate.pixels_to_mesh([[1023.5, 1023.5], [0.0, 0.0]], 2048)
    assert (centre[0] == 0.0).all() and (centre[1] == [-0.5 * 1.35, 0.5 * 1.35]).all()       # origin top-left
    with pytest.raises(ValueError):
        animate.pixels_to_mesh([[0.0, 0.0]], 1)


# ------------------------------------------------------------------ lifting
_LIFT = {}


def lifted():
    if "s" not in _LIFT:
        v, f = RC.character()
        _LIFT["s"] = animate.lift_marks(RC.NAMES, RC.PARENTS, RC.marks(), v, f, lattice=RC.LATTICE, backend="host")
        lat = rig.thickness_lattice(v, RC.LATTICE)
        _LIFT["lattice"], _LIFT["map"] = lat, ops.mesh_thickness_host(v, f, *lat)
    return _LIFT["s"]


def test_lattice_covers_the_box_grown_by_a_sample():
    v, _ = RC.character()
    x0, y0, h, W, H = rig.thickness_lattice(v, RC.LATTICE)
    lo, hi = v[:, :2].astype(np.float64).min(0), v[:, :2].astype(np.float64).max(0)
    assert h == max(hi - lo) / RC.LATTICE and x0 == lo[0] - h and y0 == lo[1] - h
    assert x0 + W * h >= hi[0] + h * (1 - 1e-9) and y0 + H * h >= hi[1] + h * (1 - 1e-9) and max(W, H) == RC.LATTICE + 2
    for bad in (0, 4095):
        with pytest.raises(ValueError):
            rig.thickness_lattice(v, bad)


def test_lifted_joints_and_tips_lie_inside_the_boxes():
    s = lifted()
    x0, y0, h, W, H = _LIFT["lattice"]
    mid, thick, count = _LIFT["map"]
    assert s.names == RC.NAMES and (s.parents == RC.PARENTS).all()
    pos, marks = s.rest_positions(), RC.marks()
    want = ["torso"] * 4 + ["right_arm"] * 3 + ["left_arm"] * 3 + ["right_leg"] * 3 + ["left_leg"] * 3
    for j, name in enumerate(RC.NAMES):
        assert RC.box_of(pos[j]) == want[j], name
        assert (pos[j, :2] == marks[j]).all() and pos[j, 2] == 0.0, name     # the box's mid-depth, exactly
        r, c = int(np.floor((pos[j, 1] - y0) / h)), int(np.floor((pos[j, 0] - x0) / h))
        assert count[r, c] == 2 and thick[r, c] > 0.07 and mid[r, c] == 0.0, name      # a pair, not the default
    leaves = [j for j in range(16) if not (RC.PARENTS == j).any()]
    assert sorted(s.end_sites) == leaves == [3, 6, 9, 12, 15]
    tip_box = {3: "head", 6: "right_arm", 9: "left_arm", 12: "right_leg", 15: "left_leg"}
    for j in leaves:
        tip, bone = pos[j] + s.end_sites[j], pos[j] - pos[RC.PARENTS[j]]
        assert RC.box_of(tip) == tip_box[j] and tip[2] == 0.0, RC.NAMES[j]
        e = s.end_sites[j]
        k = np.log2(0.5 * np.linalg.norm(bone[:2]) / np.linalg.norm(e[:2]))      # halvings taken
        assert abs(k - round(k)) < 1e-9 and 0 <= round(k) <= 8, RC.NAMES[j]
        assert abs(e[0] * bone[1] - e[1] * bone[0]) < 1e-15 and e[:2] @ bone[:2] > 0.0      # along the bone
    # the neck's tip reaches the head at once; a hand's needs halvings (the arm ends 0.03 past the hand)
    assert np.allclose(s.end_sites[3][:2], (pos[3] - pos[2])[:2] * 0.5, rtol=0, atol=1e-16)
    assert np.linalg.norm(s.end_sites[6][:2]) < 0.03 < np.linalg.norm((pos[6] - pos[5])[:2]) * 0.5
    without = animate.lift_marks(RC.NAMES, RC.PARENTS, marks, *RC.character(), lattice=RC.LATTICE, end_sites=False,
                                 backend="host")
    assert without.end_sites == {} and (without.offsets == s.offsets).all()


def test_a_mark_outside_snaps_to_the_nearest_inside_sample():
    v, f = RC.character()
    lifted()
    x0, y0, h, W, H = _LIFT["lattice"]
    thick = _LIFT["map"][1]
    marks = RC.marks()
    marks[5] = RC.arm_point(1.0, 0.2, RC.ARM_HALF + 2.0 * h)             # two samples above the right arm
    r0, c0 = int(np.floor((marks[5, 1] - y0) / h)), int(np.floor((marks[5, 0] - x0) / h))
    assert thick[r0, c0] == 0.0
    s = animate.lift_marks(RC.NAMES, RC.PARENTS, marks, v, f, lattice=RC.LATTICE, backend="host")
    # the rule again, by a plain search over every sample
    cand = []
    for r in range(H):
        for c in range(W):
            if thick[r, c] > 0.0:
                cx, cy = x0 + (c + 0.5) * h, y0 + (r + 0.5) * h
                cand.append(((cx - marks[5, 0]) ** 2 + (cy - marks[5, 1]) ** 2, r, c, cx, cy))
    d2, r, c, cx, cy = min(cand)
    p = s.rest_positions()[5]
    assert (p[:2] == (cx, cy)).all() and p[2] == 0.0 and RC.box_of(p) == "right_arm"
    assert 1.0 * h < np.sqrt(d2) < 3.5 * h
    others = [j for j in range(16) if j != 5]
    assert (s.rest_positions()[others] == lifted().rest_positions()[others]).all()


def test_a_mark_outside_snap_raises_with_the_joints_name():
    v, f = RC.character()
    marks = RC.marks()
    marks[11] = (0.6, -0.3)
    with pytest.raises(ValueError, match="right_knee"):
        animate.lift_marks(RC.NAMES, RC.PARENTS, marks, v, f, lattice=RC.LATTICE, backend="host")
    marks[11] = (0.085 + 0.055 + 0.03, -0.25)           # 0.03 beside the leg: inside snap = 0.05 x 1.3, outside 0.01
    animate.lift_marks(RC.NAMES, RC.PARENTS, marks, v, f, lattice=RC.LATTICE, backend="host")
    with pytest.raises(ValueError, match="right_knee"):
        animate.lift_marks(RC.NAMES, RC.PARENTS, marks, v, f, lattice=RC.LATTICE, snap=0.01, backend="host")
    with pytest.raises(ValueError, match="backend"):
        animate.lift_marks(RC.NAMES, RC.PARENTS, marks, v, f, lattice=RC.LATTICE, backend="numpy")


# ------------------------------------------------------------------ retargeting
def _check_rotations(clip):
    R_ = clip.rotations
    err = np.abs(np.swapaxes(R_, -1, -2) @ R_ - np.eye(3)).max()
    assert err <= BOUND and (np.linalg.det(R_) > 0.0).all(), err


def _first_child_bones(T, S, src):
    """(j, c, s, s_c) of the rule: c the first child of j mapped below s."""
    out = []
    for j in range(T.n_joints):
        if src[j] < 0:
            continue
        for c in np.flatnonzero(T.parents == j):
            a = src[c]
            below = False
            while a >= 0 and src[c] >= 0:
                a = S.parents[a]
                below = below or a == src[j]
            if below:
                out.append((j, int(c), int(src[j]), int(src[c])))
                break
    return out


def _by_name(T, S):
    low = [n.lower() for n in S.names]
    return np.array([low.index(n.lower()) if n.lower() in low else -1 for n in T.names])


def _directions_match(T, out, S, clip, bones):
    _, XS = RC.forward(S, clip)
    _, XT = RC.forward(T, out)
    worst = 0.0
    for j, c, s, sc in bones:
        worst = max(worst, np.abs(RC.unit(XT[:, c] - XT[:, j]) - RC.unit(XS[:, sc] - XS[:, s])).max())
    return worst


def test_retarget_to_the_source_itself_returns_the_clip():
    S = RC.source_skeleton()
    clip = RC.random_clip(S, 6, seed=1)
    out = animate.retarget_clip(S, clip, S)
    assert out.frame_time == clip.frame_time and out.rotations.shape == clip.rotations.shape
    assert np.abs(out.rotations - clip.rotations).max() <= BOUND
    assert np.abs(out.translations - clip.translations).max() <= BOUND * np.abs(clip.translations).max()
    _check_rotations(out)


def test_a_scaled_source_gives_the_same_rotations_and_scaled_translations():
    S, big = RC.source_skeleton(), RC.source_skeleton(scale=2.5)
    clip = RC.random_clip(S, 6, seed=2)
    clip_big = animate.Clip(clip.translations * 2.5, clip.rotations, clip.frame_time)
    T = lifted()
    a, b = animate.retarget_clip(S, clip, T), animate.retarget_clip(big, clip_big, T)
    assert np.abs(a.rotations - b.rotations).max() <= BOUND
    assert np.abs(a.translations - b.translations).max() <= BOUND
    # and onto the small skeleton itself: the root's path shrinks by 1 / 2.5 about the root
    back = animate.retarget_clip(big, clip_big, S)
    assert np.abs(back.rotations - clip.rotations).max() <= BOUND
    want = S.offsets[0] + (clip_big.translations - big.offsets[0]) / 2.5
    assert np.abs(back.translations - want).max() <= BOUND * np.abs(want).max()
    _check_rotations(a)
    _check_rotations(back)


def _turned_arms(S, how):
    """The source with the offsets and end sites below both shoulders turned about z: by +-40 degrees,
    or by a half turn (negated exactly)."""
    off, ends = S.offsets.copy(), {j: e.copy() for j, e in S.end_sites.items()}
    for first, sign in ((4, 1.0), (7, -1.0)):
        if how == 180:
            M = np.diag([-1.0, -1.0, 1.0])
        else:
            a = np.radians(sign * how)
            M = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        for j in (first + 1, first + 2):
            off[j] = M @ off[j]
        ends[first + 2] = M @ ends[first + 2]
    return Skeleton([n.lower() for n in S.names], S.parents, off, ends)


@pytest.mark.parametrize("how", [40, 180])
def test_turned_arm_rest_directions_follow_the_source_in_every_frame(how):
    S = RC.source_skeleton()
    T = _turned_arms(S, how)
    clip = RC.random_clip(S, 8, seed=3 + how)
    out = animate.retarget_clip(S, clip, T)
    _check_rotations(out)
    bones = _first_child_bones(T, S, _by_name(T, S))
    assert {(4, 5), (5, 6), (7, 8), (8, 9)} <= {(j, c) for j, c, _, _ in bones} and len(bones) == 11
    worst = _directions_match(T, out, S, clip, bones)
    print(f"[retarget] arms turned by {how}: largest direction error {worst:.2e}")
    assert worst <= BOUND
    if how == 180:                          # the half-turn branch was taken, and is a half turn
        u = RC.unit(T.rest_positions()[5] - T.rest_positions()[4])
        A = animate.minimal_rotation(u, -u)
        assert np.abs(A @ u + u).max() <= 1e-15 and np.abs(A @ A - np.eye(3)).max() <= 1e-15
    # the legs and the spine have the source's rest directions: their local rotations are the clip's
    same = [0, 1, 2, 3, 10, 11, 12, 13, 14, 15]
    assert np.abs(out.rotations[:, same] - clip.rotations[:, same]).max() <= BOUND


def test_the_lifted_character_follows_the_source_whatever_pose_it_was_drawn_in():
    S, T = RC.source_skeleton(), lifted()
    clip = RC.random_clip(S, 8, seed=9)
    out = animate.retarget_clip(S, clip, T)
    _check_rotations(out)
    bones = _first_child_bones(T, S, _by_name(T, S))
    assert len(bones) == 11 and _directions_match(T, out, S, clip, bones) <= BOUND
    # drawn with raised arms, driven from a T-pose: the rest frame of the source already bends the arms
    rest = animate.retarget_clip(S, animate.rest_clip(S), T)
    assert np.abs(rest.rotations[0, 4] - np.eye(3)).max() > 0.1
    k = (T.rest_positions()[0, 1] - T.rest_points()[:, 1].min()) / (S.rest_positions()[0, 1] - S.rest_points()[:, 1].min())
    assert np.abs(out.translations - (T.offsets[0] + k * (clip.translations - S.offsets[0]))).max() <= BOUND


def test_an_unmapped_spine_joint_of_the_source_bends_the_chord():
    S = RC.source_skeleton(spine_joint=True)
    T = _turned_arms(RC.source_skeleton(), 40)
    assert "spine1" in S.names and "spine1" not in T.names
    clip = RC.random_clip(S, 8, seed=11)
    out = animate.retarget_clip(S, clip, T)
    _check_rotations(out)
    src = _by_name(T, S)
    bones = _first_child_bones(T, S, src)
    hip = [b for b in bones if b[0] == 1][0]
    assert S.parents[hip[3]] != hip[2] and S.names[S.parents[hip[3]]] == "spine1"       # the chord hip -> torso
    worst = _directions_match(T, out, S, clip, bones)
    print(f"[retarget] unmapped spine joint: largest direction error {worst:.2e}")
    assert worst <= BOUND
    # without M_f the hip's bone would point along the source hip's own frame instead
    Rw, XS = RC.forward(S, clip)
    u_s = RC.unit(S.rest_positions()[hip[3]] - S.rest_positions()[hip[2]])
    assert np.abs(Rw[:, hip[2]] @ u_s - RC.unit(XS[:, hip[3]] - XS[:, hip[2]])).max() > 1e-3


def test_joint_maps():
    S, T = RC.source_skeleton(), lifted()
    clip = RC.random_clip(S, 3, seed=4)
    full = {t: s for t, s in zip(T.names, S.names)}
    a, b = animate.retarget_clip(S, clip, T), animate.retarget_clip(S, clip, T, joint_map=full)
    assert (a.rotations == b.rotations).all() and (a.translations == b.translations).all()
    with pytest.raises(ValueError, match="'Spine9'.*source"):
        animate.retarget_clip(S, clip, T, joint_map={**full, "torso": "Spine9"})
    with pytest.raises(ValueError, match="'tail'.*target"):
        animate.retarget_clip(S, clip, T, joint_map={**full, "tail": "Hip"})
    with pytest.raises(ValueError, match="root"):
        animate.retarget_clip(S, clip, T, joint_map={t: s for t, s in full.items() if t != "root"})
    # an unmapped joint follows its parent; a mapped leaf takes its parent's A
    part = {t: s for t, s in full.items() if t not in ("right_elbow",)}
    out = animate.retarget_clip(S, clip, T, joint_map=part)
    assert np.abs(out.rotations[:, 5] - np.eye(3)).max() <= BOUND
    _check_rotations(out)
