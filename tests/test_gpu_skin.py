"""GPU: the rigging kernels (csrc/mesh_skin.hip) against the float64 restatement of their rules
(tests/skin_ref.py: brute force over all triangles, scipy's sparse LU), and the skinned render end
to end.

Measured bars (one MI355X; the figures are also in profiles/skin_probe.json, accuracy_vs_reference):
  * dist: the device runs the reference's float64 operations; only sqrt and the division may round
    differently.  Largest relative difference measured on the three meshes: 0 (character 0, torus 0,
    sheet 0: both are correctly rounded on the device); asserted: four times that, i.e. equality.
  * true residual |b - A x| / |b| after a solve to tol = 1e-10: measured 6.656e-11 (character, 54
    iterations), 8.178e-11 (torus, 82), 7.069e-11 (sheet, 139), each equal to the recurrence's own
    residual to five digits (no drift); asserted: twice the largest, 1.636e-10.
  * max |W - W_splu| at tol = 1e-10: measured 4.488e-11 (character), 6.968e-12 (torus), 6.121e-12
    (sheet); asserted: four times the largest, 1.796e-10 (below 1e-6, which is all the f32 weights
    need).
"""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import skin_ref as R
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu

DIST_REL_MEASURED = 0.0          # bit-equal on all three meshes
RESID_MEASURED = 8.178e-11
W_DIFF_MEASURED = 4.489e-11
TOL = 1e-10
MAX_ITERS = 20000


@functools.lru_cache(maxsize=None)
def _case(name):
    v, f, bones = R.lattice_case() if name == "lattice" else R.general_cases()[name]
    dist, vis, frag = R.visibility(v, f, bones)
    return v, f, bones, dist, vis, frag


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _device_visibility(dev, v, f, bones, **kw):
    dist, vis = ops.bone_visibility(_t(v, dev), _t(f, dev, torch.int32), _t(bones, dev), **kw)
    return dist.cpu().numpy(), vis.cpu().numpy().astype(bool)


GENERAL = ["character", "torus", "sheet"]


# ------------------------------------------------------------------ 2. distances and visibility
@pytest.mark.parametrize("name", GENERAL)
def test_distance_matches_the_reference(dev, name):
    v, f, bones, dist, vis, frag = _case(name)
    got, _ = _device_visibility(dev, v, f, bones)
    assert got.dtype == np.float64 and got.shape == dist.shape
    rel = float((np.abs(got - dist) / dist).max())
    print(f"[skin] {name}: dist max relative difference {rel:.3e}")
    assert rel <= 4.0 * DIST_REL_MEASURED


@pytest.mark.parametrize("name", GENERAL)
def test_visibility_equals_the_reference_outside_its_fragile_pairs(dev, name):
    v, f, bones, dist, vis, frag = _case(name)
    assert frag.mean() <= 0.005                                    # the condition the comparison rests on
    assert 0.02 < vis.mean() < 0.98
    _, got = _device_visibility(dev, v, f, bones)
    differ = got != vis
    print(f"[skin] {name}: fragile {frag.mean():.5f}, visible {vis.mean():.3f}, "
          f"differing pairs {int(differ.sum())} (outside fragile {int((differ & ~frag).sum())})")
    assert not (differ & ~frag).any()
    # the answer depends neither on the grid nor on the vertex order
    _, coarse = _device_visibility(dev, v, f, bones, cells_per_axis=3)
    _, fine = _device_visibility(dev, v, f, bones, cells_per_axis=40)
    assert np.array_equal(coarse, got) and np.array_equal(fine, got)


def test_lattice_case_has_no_exclusions(dev):
    v, f, bones, dist, vis, frag = _case("lattice")
    got_d, got = _device_visibility(dev, v, f, bones)
    assert np.array_equal(got, vis)
    assert vis.any() and not vis.all()
    assert np.array_equal(got_d, dist)             # dyadic coordinates: every operation is exact or correctly rounded
    for cells in (1, 2, 7):
        assert np.array_equal(_device_visibility(dev, v, f, bones, cells_per_axis=cells)[1], vis)


@pytest.mark.parametrize("name", GENERAL)
def test_closest_sets_equal_the_reference(dev, name):
    v, f, bones, dist, vis, frag = _case(name)
    got_d, got = _device_visibility(dev, v, f, bones)
    labels = R.components(len(v), f)
    floor = R.D_FLOOR * float(np.linalg.norm(v.astype(np.float64).max(0) - v.astype(np.float64).min(0)))
    near, n, P, h, _ = R.heat_sources(dist, vis, labels, floor)
    from drawingspinup_amd.animate import skin
    P2, h2, _ = skin.heat_sources(got_d, got, skin.components(len(v), f), floor)
    keep = ~frag.any(1)                                           # the same exclusion, per vertex
    assert keep.mean() > 0.9
    assert np.array_equal((P2 > 0)[keep], near[keep])
    assert np.array_equal((P2 > 0).sum(1)[keep], n[keep])
    assert np.array_equal(P2[keep], P[keep])


# ------------------------------------------------------------------ 3. the solve
def _system(name):
    v, f, bones, dist, vis, frag = _case(name)
    W, parts = R.bone_heat(v, f, bones, dist, vis)
    return parts["A"], parts["rhs"], parts["P"], W


def _cg(dev, A, rhs, x0, tol=TOL, max_iters=MAX_ITERS):
    x, iters, res = ops.spd_cg_block(_t(A.indptr.astype(np.int32), dev), _t(A.indices.astype(np.int32), dev),
                                     _t(A.data, dev), _t(rhs, dev), x0=_t(x0, dev), tol=tol, max_iters=max_iters)
    return x.cpu().numpy(), iters, res


@pytest.mark.parametrize("name", GENERAL)
def test_block_cg_against_the_direct_solve(dev, name):
    A, rhs, P, W = _system(name)
    x, iters, res = _cg(dev, A, rhs, P)
    true = float((np.linalg.norm(rhs - A @ x, axis=0) / np.linalg.norm(rhs, axis=0)).max())
    diff = float(np.abs(x - W).max())
    print(f"[skin] {name}: n {A.shape[0]} iterations {iters}, recurrence residual {res.max():.3e}, "
          f"true residual {true:.3e}, max |W - W_splu| {diff:.3e}")
    assert 0 < iters < MAX_ITERS and (res <= TOL).all()
    assert true <= 2.0 * RESID_MEASURED
    assert diff <= 4.0 * W_DIFF_MEASURED and 4.0 * W_DIFF_MEASURED < 1e-6
    x2, iters2, res2 = _cg(dev, A, rhs, P)
    assert iters2 == iters and np.array_equal(x2, x) and np.array_equal(res2, res)      # the same bits
    # the iteration limit is honoured and reported
    x3, iters3, res3 = _cg(dev, A, rhs, P, max_iters=5)
    assert iters3 == 5 and (res3 > TOL).any()


def test_block_cg_shapes(dev):
    """One column, many columns, a matrix smaller than a workgroup, a zero right-hand side."""
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    for n, B in ((5, 1), (300, 3), (1000, 64), (700, 200)):
        G = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=n, format="csr")
        A = (G @ G.T + sp.diags(rng.uniform(0.5, 2.0, n))).tocsr()
        A.sort_indices()
        rhs = rng.normal(size=(n, B))
        rhs[:, B // 2] = 0.0
        x, iters, res = _cg(dev, A, rhs, np.zeros((n, B)))
        want = R.solve_direct(A, rhs)
        assert (res <= TOL).all() and iters < MAX_ITERS
        assert np.abs(x - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
        assert not x[:, B // 2].any()


def _nested():
    """A closed capsule around the bone and a second one around the first: no vertex of the outer
    component sees the bone."""
    inner = R.capsule((-0.2, 0.0, 0.0), (0.2, 0.0, 0.0), 0.08, 10, 4, 2)
    outer = R.capsule((-0.25, 0.0, 0.0), (0.25, 0.0, 0.0), 0.2, 10, 4, 2)
    v, f = R.merge(inner, outer)
    names, parents = ["a", "b", "c"], np.array([-1, 0, 1])
    off = np.array([[-0.18, 0.003, 0.002], [0.17, 0.004, -0.003], [0.18, -0.002, 0.004]])
    return R.jitter(v, 1e-3, 9).astype(np.float32), f, len(inner[0]), names, parents, off


def test_component_that_sees_no_bone_takes_the_fallback(dev):
    v, f, n_inner, names, parents, off = _nested()
    sk = animate.Skeleton(names, parents, off)
    infl, w, info = animate.bone_heat_weights(v, f, sk, K=None, device=dev, return_info=True)
    assert not info["visible"][n_inner:].any() and info["visible"][:n_inner].any()
    assert len(info["fallback_components"]) == 1
    assert info["iterations"] < MAX_ITERS
    assert np.abs(info["W"].sum(1) - 1.0).max() <= 1e-8
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 4 * 2.0 ** -24
    heads, segs = R.bones_of(parents, off, {})
    W, parts = R.bone_heat(v, f, segs.astype(np.float32))
    assert len(parts["blind"]) == 1
    # not one of the three measured meshes: 1e-8 is two orders above the solve's bars and still
    # below half an ulp of an f32 weight (2^-25 = 3e-8)
    assert np.abs(info["W"] - W).max() <= 1e-8
    assert info["W"][n_inner:].min() > 0.0                         # the outer shell is shared by both bones


# ------------------------------------------------------------------ 4. skinning
def _skin_inputs(V, K, F, J, seed):
    rng = np.random.default_rng(seed)
    rest = rng.uniform(-0.6, 0.6, (V, 3)).astype(np.float32)
    infl = np.stack([rng.permutation(J)[:K] for _ in range(V)]).astype(np.int32)
    w = rng.random((V, K)) + 0.05
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    mats = np.empty((F, J, 3, 4))
    for fr in range(F):
        for j in range(J):
            a = rng.uniform(-180, 180, 3)
            mats[fr, j, :, :3] = R.rot("Z", a[0]) @ R.rot("X", a[1]) @ R.rot("Y", a[2])
            mats[fr, j, :, 3] = rng.uniform(-0.5, 0.5, 3)
    return rest, infl, w, mats.astype(np.float32)


def _lbs(dev, rest, infl, w, mats):
    out = ops.skin_lbs(_t(rest, dev), _t(infl, dev), _t(w, dev), _t(mats, dev))
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.mark.parametrize("K,F", [(1, 1), (4, 1), (4, 120), (9, 1), (9, 120), (1, 120)])
def test_skinning_within_the_derived_bound(dev, K, F):
    """Per coordinate (2 K + 4) 2^-24 max(|R x| + |t|): each influence is three products, three sums
    (<= 4 roundings on a magnitude <= |R x| + |t|, weighted by w_k <= 1: with sum w ~ 1 they add up
    to 4), then one product and one sum per influence on the accumulator (2 K)."""
    J = 9
    rest, infl, w, mats = _skin_inputs(777, K, F, J, seed=K * 1000 + F)
    got = _lbs(dev, rest, infl, w, mats)
    ref, mag = R.skin_lbs(rest, infl, w, mats)
    assert got.shape == (F, 777, 3)
    excess = np.abs(got - ref) - (2 * K + 4) * 2.0 ** -24 * mag
    assert excess.max() <= 0.0


def test_identity_pose_reproduces_the_rest_mesh(dev):
    rest, infl, w, mats = _skin_inputs(500, 4, 2, 6, seed=5)
    mats[:] = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    got = _lbs(dev, rest, infl, w, mats)
    assert (np.abs(got - rest[None]) <= (2 * 4 + 4) * 2.0 ** -24 * np.abs(rest[None])).all()
    w1 = np.zeros_like(w)
    w1[:, 0] = 1.0
    assert np.array_equal(_lbs(dev, rest, infl, w1, mats), np.broadcast_to(rest, (2,) + rest.shape))


def test_single_influence_vertex_follows_its_joint(dev):
    rest, infl, w, mats = _skin_inputs(400, 4, 3, 6, seed=6)
    w[:] = 0.0
    w[:, 2] = 1.0                                                  # one influence, not the first
    got = _lbs(dev, rest, infl, w, mats).astype(np.float64)
    m = mats.astype(np.float64)[:, infl[:, 2]]
    x = rest.astype(np.float64)
    rigid = np.einsum("fvab,vb->fva", m[..., :3], x) + m[..., 3]
    scale = np.einsum("fvab,vb->fva", np.abs(m[..., :3]), np.abs(x)) + np.abs(m[..., 3])
    assert (np.abs(got - rigid) <= 4 * 2.0 ** -24 * scale).all()
    # an influence outside [0, J) contributes nothing
    bad = infl.copy()
    bad[:, 0] = 99
    bad[:, 1] = -1
    assert np.array_equal(_lbs(dev, rest, bad, w, mats), got.astype(np.float32))


# ------------------------------------------------------------------ 5. end to end
@functools.lru_cache(maxsize=None)
def _character():
    v, f = R.capsule_character()
    names, parents, off, ends = R.humanoid()
    return v, f, R.vertex_colours(len(v), 8), animate.Skeleton(names, parents, off, ends)


_WEIGHTS = {}


def _weights(dev):
    if "w" not in _WEIGHTS:
        v, f, c, sk = _character()
        _WEIGHTS["w"] = animate.bone_heat_weights(v, f, sk, device=dev, return_info=True)
    return _WEIGHTS["w"]


def _swing(sk, n=30):
    """Left forearm and right shin swing: the left elbow turns about z, the right knee about x.  Their
    bones lie outside the torso capsule, so no torso vertex has them as a heat source."""
    clip = animate.rest_clip(sk, n)
    for k in range(n):
        a = 40.0 * np.sin(2 * np.pi * k / n)
        clip.rotations[k, 6] = R.rot("Z", a)
        clip.rotations[k, 17] = R.rot("X", 0.7 * a)
    return clip


def test_bone_heat_weights_match_the_reference_on_the_character(dev):
    v, f, c, sk = _character()
    infl, w, info = _weights(dev)
    _, _, bones, _, _, _ = _case("character")
    # the reference system and direct solve on the device's own distances and visibility
    W, _ = R.bone_heat(v, f, bones, info["dist"], info["visible"].astype(bool))
    d = float(np.abs(info["W"] - W).max())
    print(f"[skin] character: bone_heat_weights vs reference max |dW| {d:.3e}, iterations {info['iterations']}")
    assert d <= 4.0 * W_DIFF_MEASURED
    assert infl.shape == (len(v), 4) and infl.dtype == np.int32 and w.dtype == np.float32
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 4 * 2.0 ** -24 and w.min() >= 0.0
    assert (np.diff(w, axis=1) <= 0).all()                         # the largest first


def test_rest_clip_renders_as_rest_pose(dev):
    """Byte equality needs the skinned rest mesh to BE the rest mesh.  dsu_skin_lbs forms
    sum_k w_k x in f32, which is x itself only when one weight is 1 (K = 1: 0 + 1 * x); with K = 4
    it is x within (2 K + 4) 2^-24 |x|, and a vertex moved by 1e-7 flips the few sub-samples that sit
    that close to an edge.  So: K = 1 equal byte for byte; K = 4 vertices within the bound and the
    number of differing pixels printed (measured: see profiles/skin_probe.json, rest_clip_k4)."""
    v, f, c, sk = _character()
    infl, w, _ = _weights(dev)
    one = (infl[:, :1].copy(), np.ones((len(v), 1), np.float32))
    got = animate.animate_mesh(v, f, c, sk, animate.rest_clip(sk, 1), weights=one, device=dev)
    window = (*got["centre"], got["size"], got["span"])
    assert window == animate.frame_window(got["vertices"].cpu().numpy())
    ref = animate.render_frames(v, f, c, "rest_pose", device=dev, window=window)
    assert np.array_equal(got["vertices"][0].cpu().numpy(), v)
    for k in ("color", "pos", "edge", "frames"):
        assert torch.equal(got[k], ref[k]), k
    assert got["vertices"].is_cuda and got["vertices"].shape == (1, len(v), 3)
    got4 = animate.animate_mesh(v, f, c, sk, animate.rest_clip(sk, 1), weights=(infl, w), device=dev)
    moved = np.abs(got4["vertices"][0].cpu().numpy().astype(np.float64) - v.astype(np.float64))
    assert (moved <= 12 * 2.0 ** -24 * np.abs(v.astype(np.float64))).all()
    ref4 = animate.render_frames(v, f, c, "rest_pose", device=dev,
                                 window=(*got4["centre"], got4["size"], got4["span"]))
    n_diff = int((got4["color"] != ref4["color"]).any(-1).sum())
    print(f"[skin] rest clip at K = 4: {n_diff} of {got4['size'] ** 2} colour pixels differ from rest_pose, "
          f"largest vertex move {moved.max():.3e}")


def test_swing_renders_every_frame_and_leaves_the_torso_alone(dev):
    v, f, c, sk = _character()
    infl, w, _ = _weights(dev)
    clip = _swing(sk)
    got = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev)
    assert got["color"].shape[0] == 30 and got["frames"].shape == (30, 6, got["size"], got["size"])
    assert (got["color"][..., 3].reshape(30, -1).amax(1) == 255).all()             # every frame non-empty
    window = (*got["centre"], got["size"], got["span"])
    assert window == animate.frame_window(got["vertices"].cpu().numpy())
    # a moved limb against the rest pose in the same window: frame 8 is near the top of the swing
    one = animate.Clip(clip.translations[8:9], clip.rotations[8:9])
    moved = animate.skinning_matrices(sk, one)[0]
    still = np.abs(moved - np.concatenate([np.eye(3), np.zeros((3, 1))], 1)).max((1, 2)) == 0.0
    assert not still[[6, 7, 8, 17, 18]].any() and still[[0, 1, 2, 3, 4, 5, 9, 13, 16]].all()
    a = ops.mesh_render_ortho(got["vertices"][8:9], _t(f, dev), _t(c, dev),
                              _t(animate.position_colours(v).astype(np.float32), dev), *got["centre"], got["span"],
                              got["size"], 4, want=("color_u8",))["color_u8"][0].cpu().numpy()
    b = animate.render_frames(v, f, c, "rest_pose", device=dev, window=window)["color"][0].cpu().numpy()
    assert np.array_equal(a, got["color"][8].cpu().numpy())
    S, span, (cx, cy) = got["size"], got["span"], got["centre"]
    col = lambda x: int(round(((x - cx) / span + 0.5) * S))
    row = lambda y: int(round((0.5 - (y - cy) / span) * S))
    # the torso's core: every vertex that can show there carries weight 1 on unmoved joints
    x0, x1, y0, y1 = -0.06, 0.04, 0.0, 0.2
    inside = (v[:, 0] > x0 - 0.02) & (v[:, 0] < x1 + 0.02) & (v[:, 1] > y0 - 0.02) & (v[:, 1] < y1 + 0.02)
    assert inside.sum() > 20
    assert (w[inside] * ~still[infl[inside]]).sum() == 0.0
    torso = (slice(row(y1), row(y0)), slice(col(x0), col(x1)))
    assert (b[torso][..., 3] == 255).all()
    assert np.array_equal(a[torso], b[torso])
    # the left forearm was at y = 0.28: its pixels changed
    arm = (slice(row(0.31), row(0.25)), slice(col(0.34), col(0.44)))
    assert (b[arm][..., 3] == 255).any() and not np.array_equal(a[arm], b[arm])
    assert (a[..., 3] != b[..., 3]).any()


def test_run_render_with_a_bvh_folder(dev, tmp_path):
    from drawingspinup_amd.entry import run_render
    from drawingspinup_amd.nsr.mesh import write_obj
    root, uid = str(tmp_path), "uid0"
    v, f, c, sk = _character()
    mesh_dir = os.path.join(root, uid, "mesh")
    obj = os.path.join(mesh_dir, "it3000-mc512-f50000_c_r_s_cbp.obj")
    write_obj(obj, v.astype(np.float64), f, c)
    names, parents, off, ends = R.humanoid()
    chans = [(["Xposition", "Yposition", "Zposition"] if j == 0 else []) + ["Zrotation", "Xrotation", "Yrotation"]
             for j in range(len(names))]
    motion = np.zeros((4, 3 + 3 * len(names)))
    motion[:, :3] = off[0]
    motion[:, 3 + 3 * 5] = [0.0, 15.0, 30.0, 45.0]                    # left shoulder, Z rotation
    os.makedirs(os.path.join(mesh_dir, "bvh_files"))
    with open(os.path.join(mesh_dir, "bvh_files", "wave.bvh"), "w") as fh:
        fh.write(R.bvh_text(names, parents, off * 100.0, {j: o * 100.0 for j, o in ends.items()}, chans,
                            motion * np.r_[[100.0] * 3, [1.0] * (3 * len(names))]))
    out_dir, rendered = run_render.run(["--data_dir", root, "--uid", uid, "--test", "--device", str(dev)])
    assert out_dir == os.path.join(mesh_dir, "blender_render", "wave")
    assert not os.path.exists(os.path.join(mesh_dir, "blender_render", "rest_rotate"))
    with np.load(os.path.join(mesh_dir, "skin_weights.npz")) as z:
        infl, w = z["influences"], z["weights"]
        assert list(z["joints"]) == names
    # the same in memory, from the cached weights
    ov, of, oc = animate.read_obj(obj)
    fsk, fclip = animate.fit_to_mesh(*animate.read_bvh(os.path.join(mesh_dir, "bvh_files", "wave.bvh")), ov)
    mem = animate.animate_mesh(ov, of, oc, fsk, fclip, weights=(infl, w), device=dev)
    for sub, key in (("color", "color"), ("pos", "pos"), ("edge", "edge")):
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["%04d.png" % (i + 1) for i in range(4)]
        for i in range(4):
            png = np.asarray(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
            assert np.array_equal(png, mem[key][i].cpu().numpy()), (sub, i)
            assert np.array_equal(png, rendered[key][i].cpu().numpy())
    assert not torch.equal(mem["color"][0], mem["color"][3])
    # a second run reads the cache instead of solving again
    stamp = os.path.getmtime(os.path.join(mesh_dir, "skin_weights.npz"))
    run_render.run(["--data_dir", root, "--uid", uid, "--test", "--device", str(dev)])
    assert os.path.getmtime(os.path.join(mesh_dir, "skin_weights.npz")) == stamp
