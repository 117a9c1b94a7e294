"""Dual-quaternion skinning without a GPU: the blend the kernel compiles (csrc/dqs_blend.h through
dsu_skin_dqs_host) against the numpy restatement (tests/skin_dqs_ref.py) bit for bit, its identity,
antipodal, rigid and volume properties, the rotation <-> quaternion conversions, the resampling of a
clip, and the argument checks of the new entry points and keywords.

Bound of the rigid and device comparisons: 2^-24 |ref| + 256 2^-53 scale, scale = |R||x| + |t| — the
one final rounding to f32, plus float64 noise of the conversion and blend with room (about 3e-14,
far below the first term)."""
import ctypes
import itertools

import numpy as np
import pytest

import skin_dqs_ref as D
import skin_ref as R
from drawingspinup_amd import animate

P = ctypes.c_void_p


def _lib():
    from drawingspinup_amd import _lib
    return _lib.lib()


def _ptr(a):
    return P(a.ctypes.data)


host_dqs, _same_bits = D.host_dqs, D.same_bits


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("K,F", [(1, 1), (4, 1), (9, 1), (1, 7), (4, 7), (9, 7)])
def test_host_entry_equals_the_restatement_bit_for_bit(K, F):
    rest, infl, w, mats = D.skin_inputs(777, K, F, 9, seed=K * 1000 + F)
    table = animate.dual_quaternions(mats)
    got = host_dqs(rest, infl, w, table)
    ref, _, _ = D.skin_dqs(rest, infl, w, table)
    n = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"[dqs] K {K} F {F}: {n} of {got.size} coordinates differ from the restatement")
    assert _same_bits(got, ref)
    assert np.abs(got - rest[None]).max() > 0.1                       # it moved


def test_edge_rows():
    rest, infl, w, table, at_rest = D.edge_rows()
    got = host_dqs(rest, infl, w, table)
    ref, ref64, scale = D.skin_dqs(rest, infl, w, table)
    assert _same_bits(got, ref)
    for row in at_rest:
        assert _same_bits(got[:, row], np.broadcast_to(rest[row], (2, 3)).copy()), row
    moved = np.setdiff1d(np.arange(len(rest)), at_rest)
    assert np.isfinite(got[:, moved]).all() and (np.abs(got[:, moved] - rest[moved]).max((0, 2)) > 1e-3).all()
    # row 0: the invalid influences contribute nothing — the same bytes as with them and their weights removed
    assert _same_bits(got[:, 0], host_dqs(rest[:1], infl[:1, 2:], w[:1, 2:], table)[:, 0])
    # row 1: the zero weight in first place is skipped, the second influence is the pivot
    assert _same_bits(got[:, 1], host_dqs(rest[1:2], infl[1:2, 1:], w[1:2, 1:], table)[:, 0])
    # row 5: the negative and the NaN weight contribute nothing
    assert _same_bits(got[:, 5], host_dqs(rest[5:6], infl[5:6, [0, 3]], w[5:6, [0, 3]], table)[:, 0])
    # row 3: q and -q are the same transform and add: joint 7's rigid transform
    m = _matrices_of(table[:, 7])
    x = rest[3].astype(np.float64)
    rigid = m[..., :3] @ x + m[..., 3]
    sc = np.abs(m[..., :3]) @ np.abs(x) + np.abs(m[..., 3])
    assert (np.abs(got[:, 3] - rigid) <= D.bound(rigid, sc)).all()


def _matrices_of(table):
    """(...,8) -> (...,3,4): back through animate.quaternion_rotations and t = 2 d r*."""
    r, d = table[..., :4], table[..., 4:]
    t = 2.0 * (r[..., :1] * d[..., 1:] - d[..., :1] * r[..., 1:] + np.cross(r[..., 1:], d[..., 1:]))
    return np.concatenate([animate.quaternion_rotations(r), t[..., None]], -1)


@pytest.mark.parametrize("K", [4, 9])
def test_identity_table_gives_the_rest_mesh_byte_for_byte(K):
    rest, infl, w, mats = D.skin_inputs(777, K, 3, 9, seed=40 + K)
    mats[:] = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    w = np.random.default_rng(K).uniform(0.01, 3.0, w.shape).astype(np.float32)      # positive, any sum
    got = host_dqs(rest, infl, w, animate.dual_quaternions(mats))
    assert _same_bits(got, np.broadcast_to(rest, got.shape).copy())


def test_negating_table_entries_changes_no_bit():
    J = 4
    rest, infl, w, mats = D.skin_inputs(300, 4, 2, J, seed=77)
    table = animate.dual_quaternions(mats)
    want = host_dqs(rest, infl, w, table)
    for n in range(J + 1):
        for subset in itertools.combinations(range(J), n):                    # all 16, the pivots' included
            t = table.copy()
            t[:, list(subset)] *= -1.0
            assert _same_bits(host_dqs(rest, infl, w, t), want), subset
    t = table.copy()
    t[0, 1] *= -1.0                                                            # one frame of one joint
    assert _same_bits(host_dqs(rest, infl, w, t), want)


@pytest.mark.parametrize("K", [1, 4, 9])
def test_influences_with_one_transform_give_that_rigid_transform(K):
    rest, infl, w, mats = D.skin_inputs(500, K, 5, 9, seed=90 + K)
    mats[:] = mats[:, :1]                                                      # every joint: joint 0's transform
    w = np.random.default_rng(K).uniform(0.01, 3.0, w.shape).astype(np.float32)
    got = host_dqs(rest, infl, w, animate.dual_quaternions(mats)).astype(np.float64)
    x = rest.astype(np.float64)
    rigid = np.einsum("fab,vb->fva", mats[:, 0, :, :3], x) + mats[:, None, 0, :, 3]
    scale = np.einsum("fab,vb->fva", np.abs(mats[:, 0, :, :3]), np.abs(x)) + np.abs(mats[:, None, 0, :, 3])
    excess = np.abs(got - rigid) - D.bound(rigid, scale)
    print(f"[dqs] K {K}: largest |got - rigid| / bound {float((np.abs(got - rigid) / D.bound(rigid, scale)).max()):.3f}")
    assert excess.max() <= 0.0


@pytest.mark.parametrize("theta", [60.0, 120.0, 179.0])
def test_a_twisted_ring_keeps_its_radius(theta):
    rho, n = 0.1, 64
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([rho * np.cos(a), np.full(n, 0.03), rho * np.sin(a)], 1).astype(np.float32)
    rho32 = np.hypot(ring[:, 0].astype(np.float64), ring[:, 2].astype(np.float64))     # the f32 ring's own radii
    mats = np.zeros((1, 2, 3, 4))
    mats[0, 0, :, :3] = np.eye(3)
    mats[0, 1, :, :3] = R.rot("Y", theta)
    infl = np.tile(np.array([[0, 1]], np.int32), (n, 1))
    w = np.full((n, 2), 0.5, np.float32)
    got = host_dqs(ring, infl, w, animate.dual_quaternions(mats))[0].astype(np.float64)
    radius = np.hypot(got[:, 0], got[:, 2])
    assert np.abs(radius - rho).max() <= 1e-6 * rho and np.abs(radius - rho32).max() <= 1e-6 * rho
    assert np.array_equal(got[:, 1], ring[:, 1].astype(np.float64))
    # the linear blend of the same inputs loses it: rho cos(theta / 2)
    lbs, _ = R.skin_lbs(ring, infl, w, mats.astype(np.float32))
    lin = np.hypot(lbs[0, :, 0], lbs[0, :, 2])
    want = rho * np.cos(np.radians(theta) / 2)
    print(f"[dqs] theta {theta}: dual-quaternion radius {radius.mean():.5f}, linear {lin.mean():.5f} (rho cos = {want:.5f})")
    assert np.abs(lin - want).max() <= 1e-6 * rho
    assert want < 0.87 * rho and np.abs(radius - lin).min() > 0.13 * rho


# ------------------------------------------------------------------ conversions
def _random_rotations(n, seed):
    q = np.random.default_rng(seed).normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return animate.quaternion_rotations(q), q


def _half_turn(axis):
    a = np.asarray(axis, np.float64)
    return 2.0 * np.outer(a, a) / (a @ a) - np.eye(3)


def test_rotation_quaternion_round_trip_and_sign():
    Rm, q = _random_rotations(10000, 1)
    got = animate.rotation_quaternions(Rm)
    assert got.shape == (10000, 4) and (got[:, 0] >= 0.0).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 4e-16
    assert np.abs(animate.quaternion_rotations(got) - Rm).max() <= 1e-14
    assert np.abs(got - np.where(q[:, :1] < 0, -q, q)).max() <= 1e-14
    # every branch was taken
    assert all(((np.stack([np.trace(Rm, axis1=1, axis2=2), Rm[:, 0, 0], Rm[:, 1, 1], Rm[:, 2, 2]], 1)).argmax(1) == b).any()
               for b in range(4))
    # leading dimensions are kept
    assert animate.rotation_quaternions(Rm.reshape(100, 100, 3, 3)).shape == (100, 100, 4)
    assert np.array_equal(animate.rotation_quaternions(np.eye(3)), [1.0, 0.0, 0.0, 0.0])


@pytest.mark.parametrize("axis,want", [((1, 0, 0), (0, 1, 0, 0)), ((0, 1, 0), (0, 0, 1, 0)), ((0, 0, 1), (0, 0, 0, 1)),
                                       ((1, 1, 0), (0, 0.5 ** 0.5, 0.5 ** 0.5, 0)),
                                       ((-1, 0, 0), (0, 1, 0, 0)), ((0, 1, -1), (0, 0, 0.5 ** 0.5, -0.5 ** 0.5))])
def test_exact_half_turns(axis, want):
    Rm = _half_turn(axis)
    q = animate.rotation_quaternions(Rm)
    assert q[0] == 0.0 and q[np.flatnonzero(q)[0]] > 0.0                       # w = 0: first non-zero positive
    assert not np.signbit(q).any() or (q[np.signbit(q)] != 0.0).all()          # no -0
    assert np.abs(q - np.asarray(want)).max() <= 1e-15
    assert np.abs(animate.quaternion_rotations(q) - Rm).max() <= 1e-14


def test_rotations_next_to_a_half_turn_keep_their_digits():
    rng = np.random.default_rng(3)
    axes = rng.normal(size=(200, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    ang = np.pi - rng.uniform(0, 1e-7, 200)
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axes], 1)
    Rm = animate.quaternion_rotations(q)
    assert np.abs(animate.quaternion_rotations(animate.rotation_quaternions(Rm)) - Rm).max() <= 1e-14


def test_dual_quaternions_round_trip_and_refusals():
    rng = np.random.default_rng(4)
    mats = D.random_transforms(rng, 6, 9)
    table = animate.dual_quaternions(mats)
    assert table.shape == (6, 9, 8) and table.dtype == np.float64
    assert np.abs(_matrices_of(table) - mats).max() <= 1e-14
    assert np.abs((table[..., :4] * table[..., 4:]).sum(-1)).max() <= 1e-15     # d orthogonal to r
    assert np.abs(table - D.table_of(mats)).max() <= 1e-13                     # the independent construction
    ident = animate.dual_quaternions(np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None, None])
    assert np.array_equal(ident[0, 0], [1.0, 0, 0, 0, 0, 0, 0, 0]) and not np.signbit(ident).any()
    scaled = mats.copy()
    scaled[2, 3, :, :3] *= 1.0 + 1e-6
    with pytest.raises(ValueError):
        animate.dual_quaternions(scaled)
    mirrored = mats.copy()
    mirrored[1, 0, :, 0] *= -1.0
    with pytest.raises(ValueError):
        animate.dual_quaternions(mirrored)
    nan = mats.copy()
    nan[0, 0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        animate.dual_quaternions(nan)
    with pytest.raises(ValueError):
        animate.dual_quaternions(mats[0])
    assert animate.dual_quaternions(np.zeros((0, 3, 3, 4))).shape == (0, 3, 8)


# ------------------------------------------------------------------ resampling
def _clip(F, J, dt, seed):
    rng = np.random.default_rng(seed)
    rot = np.empty((F, J, 3, 3))
    for f in range(F):
        for j in range(J):
            a = rng.uniform(-180, 180, 3)
            rot[f, j] = R.rot("Z", a[0]) @ R.rot("X", a[1]) @ R.rot("Y", a[2])
    return animate.Clip(rng.uniform(-1, 1, (F, 3)), rot, dt)


@pytest.mark.parametrize("dt", [1.0 / 30.0, 1.0 / 120.0, 0.041])
def test_resampling_to_the_own_rate_and_to_half_of_it_copies_frames(dt):
    clip = _clip(11, 4, dt, 5)
    same = animate.resample_clip(clip, clip.frame_time)
    assert np.array_equal(same.translations, clip.translations) and np.array_equal(same.rotations, clip.rotations)
    assert same.frame_time == clip.frame_time
    half = clip.resample(2.0 * clip.frame_time)
    assert half.n_frames == 6 and half.frame_time == 2.0 * clip.frame_time
    assert np.array_equal(half.translations, clip.translations[::2])
    assert np.array_equal(half.rotations, clip.rotations[::2])


def test_constant_angular_velocity_is_reproduced():
    F, dt, rate = 9, 0.3125, 40.0                                              # degrees per second: 12.5 per frame
    axis = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    base = R.rot("X", 25.0) @ R.rot("Y", -50.0)

    def turn(deg):
        a = np.radians(deg)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)

    clip = animate.rest_clip(animate.Skeleton(["a", "b"], [-1, 0], np.zeros((2, 3))), F)
    clip.frame_time = dt
    for k in range(F):
        clip.rotations[k, 1] = base @ turn(rate * k * dt)
        clip.translations[k] = [0.1 * k, -0.2 * k, 0.05 * k]
    fine = animate.resample_clip(clip, dt / 2.5)
    assert fine.n_frames == 21                                                 # floor(8 * 2.5) + 1
    for k in range(fine.n_frames):
        t = k * dt / 2.5
        assert np.abs(fine.rotations[k, 1] - base @ turn(rate * t)).max() <= 1e-12, k
        assert np.abs(fine.rotations[k, 0] - np.eye(3)).max() <= 1e-15
        assert np.abs(fine.translations[k] - np.array([0.1, -0.2, 0.05]) * (t / dt)).max() <= 1e-12
    assert np.array_equal(fine.rotations[::5], clip.rotations[::2])            # the times that coincide


def test_slerp_takes_the_shorter_arc():
    clip = animate.Clip(np.zeros((2, 3)), np.stack([R.rot("Y", 350.0), R.rot("Y", 10.0)])[:, None], 0.1)
    mid = animate.resample_clip(clip, 0.05)
    assert mid.n_frames == 3
    assert np.abs(mid.rotations[1, 0] - np.eye(3)).max() <= 1e-14              # through 0, not through 180
    quarter = animate.resample_clip(clip, 0.025)
    assert np.abs(quarter.rotations[1, 0] - R.rot("Y", -5.0)).max() <= 1e-14
    # two frames a hair apart: lerped and normalised, still a rotation
    near = animate.Clip(np.zeros((2, 3)), np.stack([R.rot("Z", 30.0), R.rot("Z", 30.0 + 1e-10)])[:, None], 0.1)
    got = animate.resample_clip(near, 0.05).rotations[1, 0]
    assert np.abs(got - R.rot("Z", 30.0)).max() <= 1e-11 and np.abs(got.T @ got - np.eye(3)).max() <= 1e-15


@pytest.mark.parametrize("F,dt,new,want", [(10, 0.1, 0.25, 4), (10, 0.1, 1.0, 1), (5, 1.0 / 120, 1.0 / 30, 2),
                                           (121, 1.0 / 120, 1.0 / 30, 31), (4, 0.5, 0.4, 4)])
def test_frame_count_follows_the_formula(F, dt, new, want):
    clip = _clip(F, 2, dt, 6)
    got = animate.resample_clip(clip, new)
    assert got.n_frames == int(np.floor((F - 1) * dt / new)) + 1 == want
    assert np.array_equal(got.rotations[0], clip.rotations[0]) and np.array_equal(got.translations[0], clip.translations[0])
    q = animate.rotation_quaternions(got.rotations)
    assert np.abs(animate.quaternion_rotations(q) - got.rotations).max() <= 1e-14        # rotations still


def test_one_frame_clip_and_bad_frame_times():
    one = _clip(1, 3, 0.1, 7)
    assert animate.resample_clip(one, 0.01) is one
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            animate.resample_clip(_clip(3, 2, 0.1, 8), bad)


# ------------------------------------------------------------------ arguments
def test_entry_points_validate_without_a_gpu():
    lib = _lib()
    rest, infl, w, mats = D.skin_inputs(5, 2, 1, 3, seed=9)
    table = animate.dual_quaternions(mats)
    out = np.zeros((1, 5, 3), np.float32)
    a = (_ptr(rest), _ptr(infl), _ptr(w), _ptr(table))
    assert lib.dsu_skin_dqs_host(*a, 5, 2, 1, 3, _ptr(out)) == 0
    for i in range(4):                                                         # each null pointer
        b = list(a)
        b[i] = None
        assert lib.dsu_skin_dqs_host(*b, 5, 2, 1, 3, _ptr(out)) == -1
        assert lib.dsu_skin_dqs(*b, 5, 2, 1, 3, _ptr(out), None) == -1
    assert lib.dsu_skin_dqs_host(*a, 5, 2, 1, 3, None) == -1
    assert lib.dsu_skin_dqs(*a, 5, 2, 1, 3, None, None) == -1
    for V, K, F, J in ((-1, 2, 1, 3), (5, 0, 1, 3), (5, 4097, 1, 3), (5, 2, 0, 3), (5, 2, 65536, 3), (5, 2, 1, 0),
                       (1 << 30, 2, 4, 3)):
        assert lib.dsu_skin_dqs_host(*a, V, K, F, J, _ptr(out)) == -1, (V, K, F, J)
        assert lib.dsu_skin_dqs(*a, V, K, F, J, _ptr(out), None) == -1, (V, K, F, J)
    # an empty problem: nothing to do, no pointer needed, no launch
    assert lib.dsu_skin_dqs_host(None, None, None, None, 0, 2, 1, 3, None) == 0
    assert lib.dsu_skin_dqs(None, None, None, None, 0, 2, 1, 3, None, None) == 0


def test_ops_skin_dqs_refuses_host_tensors_and_bad_shapes():
    import torch
    from drawingspinup_amd import _lib, ops
    rest, infl, w, mats = D.skin_inputs(5, 2, 1, 3, seed=9)
    t = [torch.from_numpy(a) for a in (rest, infl, w, animate.dual_quaternions(mats))]
    with pytest.raises(_lib.DsuError):
        ops.skin_dqs(*t)                                                       # no CPU fallback
    with pytest.raises(ValueError):
        ops.skin_dqs(t[0], t[1], t[2], torch.from_numpy(mats))                 # matrices are not a table


def test_animate_mesh_refuses_an_unknown_skinning():
    v, f = R.capsule((0, 0, 0), (0, 0.3, 0), 0.05)
    sk = animate.Skeleton(["a", "b"], [-1, 0], [[0, 0, 0], [0, 0.3, 0]])
    with pytest.raises(ValueError, match="cubic"):
        animate.animate_mesh(v, f, R.vertex_colours(len(v), 1), sk, animate.rest_clip(sk), skinning="cubic",
                             device="cuda:0")


def test_run_render_parser_knows_the_new_flags(tmp_path, capsys):
    from drawingspinup_amd.entry import run_render
    for bad in (["--skinning", "cubic"], ["--fps", "0"], ["--fps", "-3"], ["--fps", "fast"]):
        with pytest.raises(SystemExit) as e:
            run_render.run(["--data_dir", str(tmp_path), "--uid", "none", "--test", *bad])
        assert e.value.code == 2
    capsys.readouterr()
    # accepted values get as far as looking for the mesh
    with pytest.raises(FileNotFoundError):
        run_render.run(["--data_dir", str(tmp_path), "--uid", "none", "--test", "--skinning", "dual_quaternion",
                        "--fps", "15"])
