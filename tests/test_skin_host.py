"""CPU: the host side of the rigging — BVH reader, skeleton fit, skinning matrices, the argument
level of run_render — and the properties of the reference weighting itself (tests/skin_ref.py)."""
import itertools

import numpy as np
import pytest

import skin_ref as R
from drawingspinup_amd import animate
from drawingspinup_amd.animate import skeleton as S
from drawingspinup_amd.animate import skin
from drawingspinup_amd.entry import run_render


def _humanoid_bvh(tmp_path, n_frames=3, seed=0, order="ZXY"):
    names, parents, off, ends = R.humanoid()
    chans = [(["Xposition", "Yposition", "Zposition"] if j == 0 else []) + [a + "rotation" for a in order]
             for j in range(len(names))]
    rng = np.random.default_rng(seed)
    motion = rng.uniform(-40, 40, (n_frames, sum(len(c) for c in chans)))
    p = tmp_path / "walk.bvh"
    p.write_text(R.bvh_text(names, parents, off, ends, chans, motion))
    return p, names, parents, off, ends, chans, motion


def test_bvh_round_trip_of_a_19_joint_humanoid(tmp_path):
    p, names, parents, off, ends, chans, motion = _humanoid_bvh(tmp_path)
    sk, clip = animate.read_bvh(str(p))
    assert sk.names == names and len(names) == 19
    assert np.array_equal(sk.parents, parents)
    assert np.array_equal(sk.offsets, off)                     # repr() round-trips float64
    assert set(sk.end_sites) == set(ends) and all(np.array_equal(sk.end_sites[j], ends[j]) for j in ends)
    assert sk.channels == chans
    assert clip.n_frames == 3 and clip.frame_time == 1.0 / 30.0
    assert clip.translations.dtype == np.float64 and clip.rotations.shape == (3, 19, 3, 3)
    assert np.array_equal(clip.translations, motion[:, :3])
    heads, segs = sk.bones()
    rh, rs = R.bones_of(parents, off, ends)
    assert len(heads) == 23 and np.array_equal(heads, rh) and np.abs(segs - rs).max() <= 1e-15


@pytest.mark.parametrize("order", ["".join(p) for p in itertools.permutations("XYZ")])
def test_every_rotation_order_against_hand_composed_matrices(tmp_path, order):
    p, names, parents, off, ends, chans, motion = _humanoid_bvh(tmp_path, n_frames=2, seed=7, order=order)
    _, clip = animate.read_bvh(str(p))
    col = 0
    for j in range(len(names)):
        col += 3 if j == 0 else 0
        for f in range(2):
            a = motion[f, col:col + 3]
            want = R.rot(order[0], a[0]) @ R.rot(order[1], a[1]) @ R.rot(order[2], a[2])
            assert np.abs(clip.rotations[f, j] - want).max() <= 1e-12
        col += 3


def test_three_channel_root_and_malformed_files(tmp_path):
    names, parents, off, ends = ["a", "b"], np.array([-1, 0]), np.array([[0.5, 1.0, 0.0], [0.0, 1.0, 0.0]]), {1: np.array([0, 0.5, 0])}
    chans = [["Yrotation", "Xrotation", "Zrotation"]] * 2
    p = tmp_path / "t.bvh"
    p.write_text(R.bvh_text(names, parents, off, ends, chans, np.zeros((2, 6))))
    sk, clip = animate.read_bvh(str(p))
    assert np.array_equal(clip.translations, [[0.5, 1.0, 0.0]] * 2)        # no position channels: the OFFSET
    assert len(sk.bones()[0]) == 2
    p.write_text(R.bvh_text(names, parents, off, ends, chans, np.zeros((2, 6)))[:-8])
    with pytest.raises(ValueError):
        animate.read_bvh(str(p))
    with pytest.raises(ValueError):
        animate.Skeleton(["a", "b"], [-1, 1], np.zeros((2, 3)))


def test_skinning_matrices_of_the_rest_clip_are_the_identity(tmp_path):
    names, parents, off, ends = R.humanoid()
    sk = animate.Skeleton(names, parents, off, ends)
    m = animate.skinning_matrices(sk, animate.rest_clip(sk, 2))
    assert m.shape == (2, 19, 3, 4) and m.dtype == np.float64
    assert np.abs(m - np.concatenate([np.eye(3), np.zeros((3, 1))], 1)).max() <= 1e-12
    # and a rotation of one joint moves its descendants rigidly about it
    clip = animate.rest_clip(sk, 1)
    clip.rotations[0, 6] = R.rot("Z", 90.0)                                  # left elbow
    m = animate.skinning_matrices(sk, clip)
    pos = sk.rest_positions()
    wrist = m[0, 7, :, :3] @ pos[7] + m[0, 7, :, 3]
    assert np.abs(wrist - (pos[6] + [0.0, pos[7][0] - pos[6][0], 0.0])).max() <= 1e-12
    assert np.abs(m[0, 5] - np.concatenate([np.eye(3), np.zeros((3, 1))], 1)).max() <= 1e-12


def test_fit_to_mesh_meets_its_three_conditions():
    names, parents, off, ends = R.humanoid()
    sk = animate.Skeleton(names, parents, off * 37.0, {j: o * 37.0 for j, o in ends.items()})
    clip = animate.rest_clip(sk, 2)
    clip.translations[1] += [3.0, 1.0, -2.0]
    rng = np.random.default_rng(1)
    verts = rng.uniform([-0.31, -0.62, -0.05], [0.43, 0.51, 0.17], (500, 3))
    fit, fclip = animate.fit_to_mesh(sk, clip, verts)
    pts, lo, hi = fit.rest_points(), verts.min(0), verts.max(0)
    assert abs((pts[:, 1].max() - pts[:, 1].min()) - (hi[1] - lo[1])) <= 1e-12
    assert abs((pts[:, 0].max() + pts[:, 0].min()) / 2 - (hi[0] + lo[0]) / 2) <= 1e-12
    assert abs((pts[:, 2].max() + pts[:, 2].min()) / 2 - (hi[2] + lo[2]) / 2) <= 1e-12
    assert abs(pts[:, 1].min() - lo[1]) <= 1e-12
    s = (hi[1] - lo[1]) / (sk.rest_points()[:, 1].max() - sk.rest_points()[:, 1].min())
    assert np.abs((fclip.translations[1] - fclip.translations[0]) - s * np.array([3.0, 1.0, -2.0])).max() <= 1e-12
    assert np.abs(animate.skinning_matrices(fit, fclip)[0] - np.concatenate([np.eye(3), np.zeros((3, 1))], 1)).max() <= 1e-12
    assert "not an auto-rigger" in animate.fit_to_mesh.__doc__


def test_reference_weights_are_a_partition_of_unity():
    v, f, bones = R.character_case()
    W, parts = R.bone_heat(v, f, bones)
    assert np.abs(W.sum(1) - 1.0).max() <= 1e-9
    assert W.min() >= -1e-9 and W.max() <= 1.0 + 1e-9
    assert not parts["blind"]


def test_reference_cylinder_with_two_collinear_bones_is_mirrored():
    v, f, bones, n_half, n_around = R.cylinder_two_bones()
    W, _ = R.bone_heat(v, f, bones)
    assert np.abs(W.sum(1) - 1.0).max() <= 1e-9
    mirror = np.empty(len(v), np.int64)                      # vertex with x negated
    key = {tuple(np.round(p, 6)): i for i, p in enumerate(v.astype(np.float64))}
    for i, p in enumerate(v.astype(np.float64)):
        mirror[i] = key[tuple(np.round(p * [-1, 1, 1], 6))]
    assert np.abs(W[:, 0] - W[mirror, 1]).max() <= 1e-9
    joint_ring = 1 + n_half * n_around + np.arange(n_around)
    assert np.abs(v[joint_ring, 0]).max() == 0.0
    assert np.abs(W[joint_ring] - 0.5).max() <= 1e-9
    assert W[0, 0] > 0.9 and W[-1, 1] > 0.9


def test_reference_single_bone_gives_all_ones():
    v, f, bones, _, _ = R.cylinder_two_bones()
    W, _ = R.bone_heat(v, f, bones[:1])
    assert np.abs(W - 1.0).max() <= 1e-9


def test_general_position_cases_have_few_fragile_pairs():
    """The condition the device comparison rests on: at most 0.5 % of the (vertex, bone) pairs of each
    mesh have a deciding volume within 1e-9 (relative) of zero in the reference."""
    for name, (v, f, bones) in R.general_cases().items():
        _, vis, frag = R.visibility(v, f, bones)
        assert frag.mean() <= 0.005, (name, frag.mean())
        assert 0.02 < vis.mean() < 0.98, (name, vis.mean())             # both answers occur


def test_finish_weights_keeps_the_largest_and_breaks_ties_downwards():
    W = np.array([[0.25, 0.25, 0.25, -0.1, 0.25, 0.1], [0.0, 0.0, 0.7, 0.3, 0.0, 0.0], [0.0] * 6])
    heads = np.array([0, 0, 1, 2, 3, 4])
    infl, w = skin.finish_weights(W, heads, K=4)
    assert infl.dtype == np.int32 and w.dtype == np.float32 and infl.shape == (3, 4)
    assert infl[0].tolist() == [0, 0, 1, 3] and np.allclose(w[0], 0.25)
    assert infl[1, :2].tolist() == [1, 2] and np.allclose(w[1], [0.7, 0.3, 0, 0])
    assert np.allclose(w.sum(1), 1.0)
    infl, w = skin.finish_weights(W, heads, K=None)
    assert infl.shape == (3, 6) and np.allclose(w[0].sum(), 1.0) and w[0].min() == 0.0
    infl, w = skin.finish_weights(W, heads, K=1)
    assert infl[:2, 0].tolist() == [0, 1] and np.array_equal(w[:2, 0], [1.0, 1.0])


def test_product_system_matches_the_reference_system():
    v, f, bones = R.sheet_mesh() + (R.sheet_bones(),)
    dist, vis, _ = R.visibility(v, f, bones)
    floor = 1e-6 * float(np.linalg.norm(v.astype(np.float64).max(0) - v.astype(np.float64).min(0)))
    near, n, P, h, blind = R.heat_sources(dist, vis, R.components(len(v), f), floor)
    P2, h2, blind2 = skin.heat_sources(dist, vis, skin.components(len(v), f), floor)
    assert np.array_equal(P, P2) and np.array_equal(h, h2) and list(blind) == list(blind2)
    A, rhs = R.heat_system(v, f, P, h)
    A2, rhs2 = skin.heat_system(v.astype(np.float64), f, P2, h2)
    assert np.array_equal(A.indptr, A2.indptr) and np.array_equal(A.indices, A2.indices)
    assert np.abs(A.data - A2.data).max() <= 1e-12 * np.abs(A.data).max()
    assert np.abs(rhs - rhs2).max() <= 1e-12 * np.abs(rhs).max()


def test_run_render_actions_at_the_argument_level(tmp_path):
    mesh = tmp_path / "mesh"
    mesh.mkdir()
    assert run_render.plan_actions(str(mesh), test=True) == [("rest_rotate", None)]
    assert run_render.plan_actions(str(mesh), test=False) == [("rest_pose", None)]
    (mesh / "bvh_files").mkdir()
    assert run_render.plan_actions(str(mesh), test=True) == [("rest_rotate", None)]      # empty folder
    (mesh / "bvh_files" / "wave.bvh").write_text("")
    (mesh / "bvh_files" / "jump.bvh").write_text("")
    (mesh / "bvh_files" / "notes.txt").write_text("")
    got = run_render.plan_actions(str(mesh), test=True)
    assert [a for a, _ in got] == ["jump", "wave"] and all(p.endswith(a + ".bvh") for a, p in got)
    assert run_render.plan_actions(str(mesh), test=False) == [("rest_pose", None)]     # training: unchanged


def test_new_entry_points_validate_before_launching():
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    assert lib.dsu_bone_visibility_workspace_bytes(4, 5, 6) == (3 * 120 + 1) * 4
    assert lib.dsu_bone_visibility_workspace_bytes(0, 5, 6) == -1
    assert lib.dsu_bone_visibility_workspace_bytes(256, 256, 256) == -1
    assert lib.dsu_bone_visibility(0, None, None, None, 10, 10, 2, None, 0.0, 0.0, 0.0, 0.1, 4, 4, 4, None, 0,
                                   None, 0, None, None, None) == -1
    n = lib.dsu_spd_cg_block_workspace_bytes(1000, 25)
    assert n >= (3 * 1000 * 25 + 1000) * 8 and lib.dsu_spd_cg_block_workspace_bytes(1000, 257) == -1
    assert lib.dsu_spd_cg_block(None, None, None, 10, 10, 2, None, None, 1e-10, 5, None, 0, None, None, None) == -1
    assert lib.dsu_skin_lbs(None, None, None, None, 10, 4, 1, 3, None, None) == -1
    assert lib.dsu_skin_lbs(None, None, None, None, 0, 4, 1, 3, None, None) == 0
    with pytest.raises(_lib.DsuError):
        import torch
        from drawingspinup_amd import ops
        ops.skin_lbs(torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int32), torch.ones(4, 1), torch.zeros(1, 1, 3, 4))
