"""GPU: dual-quaternion skinning (skin_dqs_kernel of csrc/mesh_skin.hip) against the float64
restatement of its rule (tests/skin_dqs_ref.py) and against the host entry that compiles the same
text, then through animate_mesh and run_render.

Bound per coordinate against the restatement's unrounded float64 value: 2^-24 |ref64| + 256 2^-53
scale, scale = |R||x| + |t| — "the same f32 or its neighbour across a rounding tie".  Expected number
of coordinates that differ from dsu_skin_dqs_host: 0 (the same text and flags, IEEE float64 division
and square root on both sides); the tests print the count and assert it."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import skin_dqs_ref as D
import skin_ref as R
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _dqs(dev, rest, infl, w, table):
    out = ops.skin_dqs(_t(rest, dev), _t(infl, dev), _t(w, dev), _t(table, dev))
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(K, F):
    rest, infl, w, mats = D.skin_inputs(777, K, F, 9, seed=K * 1000 + F)
    table = animate.dual_quaternions(mats)
    _, ref64, scale = D.skin_dqs(rest, infl, w, table)
    return rest, infl, w, table, ref64, scale, D.host_dqs(rest, infl, w, table)


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("K,F", [(1, 1), (4, 1), (4, 120), (9, 120)])
def test_device_within_the_bound_and_equal_to_the_host_entry(dev, K, F):
    """F = 120 puts the frame index in the upper grid blocks; K = 9 exceeds the four influences the
    pipeline keeps."""
    rest, infl, w, table, ref64, scale, host = _case(K, F)
    got = _dqs(dev, rest, infl, w, table)
    assert got.shape == (F, 777, 3)
    ratio = float((np.abs(got.astype(np.float64) - ref64) / D.bound(ref64, scale)).max())
    n = int((got.view(np.uint32) != host.view(np.uint32)).sum())
    print(f"[dqs] K {K} F {F}: largest |device - ref64| / bound {ratio:.3f}; {n} of {got.size} coordinates "
          f"differ from dsu_skin_dqs_host")
    assert (np.abs(got.astype(np.float64) - ref64) <= D.bound(ref64, scale)).all()
    assert D.same_bits(got, host)


def test_edge_rows_give_the_host_entry_s_bytes(dev):
    rest, infl, w, table, at_rest = D.edge_rows()
    got = _dqs(dev, rest, infl, w, table)
    assert D.same_bits(got, D.host_dqs(rest, infl, w, table))
    for row in at_rest:
        assert D.same_bits(got[:, row], np.broadcast_to(rest[row], (2, 3)).copy()), row


def test_identity_table_gives_the_rest_mesh_byte_for_byte(dev):
    rest, infl, w, mats = D.skin_inputs(777, 4, 3, 9, seed=44)
    mats[:] = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    got = _dqs(dev, rest, infl, w, animate.dual_quaternions(mats))
    assert D.same_bits(got, np.broadcast_to(rest, got.shape).copy())


def test_two_runs_and_a_side_stream_give_the_same_bits(dev):
    rest, infl, w, table, _, _, host = _case(4, 120)
    a = [_t(x, dev) for x in (rest, infl, w, table)]
    first = ops.skin_dqs(*a)
    second = ops.skin_dqs(*a)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = ops.skin_dqs(*a)
    side.synchronize()
    assert torch.equal(first, second) and torch.equal(first, third)
    assert D.same_bits(third.cpu().numpy(), host)


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _character():
    v, f = R.capsule_character()
    names, parents, off, ends = R.humanoid()
    return v, f, R.vertex_colours(len(v), 8), animate.Skeleton(names, parents, off, ends)


_WEIGHTS = {}


def _weights(dev):
    if "w" not in _WEIGHTS:
        v, f, c, sk = _character()
        _WEIGHTS["w"] = animate.bone_heat_weights(v, f, sk, device=dev)
    return _WEIGHTS["w"]


def _swing(sk, n=30):
    """The swing of tests/test_gpu_skin.py: the left elbow turns about z, the right knee about x, by
    at most 40 degrees, so it fits the window."""
    clip = animate.rest_clip(sk, n)
    for k in range(n):
        a = 40.0 * np.sin(2 * np.pi * k / n)
        clip.rotations[k, 6] = R.rot("Z", a)
        clip.rotations[k, 17] = R.rot("X", 0.7 * a)
    return clip


def test_animate_mesh_with_dual_quaternions(dev):
    v, f, c, sk = _character()
    infl, w = _weights(dev)
    # bone-heat weights are rarely exactly 1 in f32: every third vertex is bound to its first influence alone
    w = w.copy()
    w[::3] = [1.0, 0.0, 0.0, 0.0]
    clip = _swing(sk)
    got = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning="dual_quaternion")
    mats = animate.skinning_matrices(sk, clip)
    direct = ops.skin_dqs(_t(v, dev), _t(infl, dev), _t(w, dev), _t(animate.dual_quaternions(mats), dev))
    assert got["vertices"].is_cuda and got["vertices"].shape == (30, len(v), 3)
    assert torch.equal(got["vertices"], direct)
    # a vertex bound to one joint follows that joint rigidly
    single = np.flatnonzero(w[:, 0] == 1.0)
    assert len(single) >= len(v) // 3 and not w[single, 1:].any()
    m = mats[:, infl[single, 0]]                                               # (F,n,3,4)
    x = v[single].astype(np.float64)
    rigid = np.einsum("fvab,vb->fva", m[..., :3], x) + m[..., 3]
    scale = np.einsum("fvab,vb->fva", np.abs(m[..., :3]), np.abs(x)) + np.abs(m[..., 3])
    verts = got["vertices"].cpu().numpy().astype(np.float64)
    assert (np.abs(verts[:, single] - rigid) <= D.bound(rigid, scale)).all()
    moved_joints = np.unique(infl[single, 0][np.abs(rigid - x).max((0, 2)) > 1e-3])
    assert len(moved_joints) >= 2                                              # forearm and shin among them
    # the same outputs, in the same shapes, as the linear call
    lin = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning="linear")
    assert set(got) == set(lin)
    window = (*got["centre"], got["size"], got["span"])
    assert window == animate.frame_window(got["vertices"].cpu().numpy())
    for k in ("color", "pos", "edge", "frames", "vertices"):
        assert got[k].shape == lin[k].shape and got[k].dtype == lin[k].dtype, k
    assert (got["color"][..., 3].reshape(30, -1).amax(1) == 255).all()         # every frame non-empty
    assert not torch.equal(got["vertices"], lin["vertices"])                   # and it is another blend
    assert torch.equal(lin["vertices"], animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w),
                                                             device=dev)["vertices"])   # the default is linear


def test_rest_clip_at_four_influences_renders_as_rest_pose(dev):
    """What the linear blend shows only at K = 1 (test_rest_clip_renders_as_rest_pose): with four
    influences per vertex the skinned rest mesh IS the rest mesh, so every frame is byte-equal."""
    v, f, c, sk = _character()
    infl, w = _weights(dev)
    assert infl.shape[1] == 4 and (w[:, 1] > 0).any()
    got = animate.animate_mesh(v, f, c, sk, animate.rest_clip(sk, 1), weights=(infl, w), device=dev,
                               skinning="dual_quaternion")
    assert D.same_bits(got["vertices"][0].cpu().numpy(), v)
    window = (*got["centre"], got["size"], got["span"])
    ref = animate.render_frames(v, f, c, "rest_pose", device=dev, window=window)
    for k in ("color", "pos", "edge", "frames"):
        assert torch.equal(got[k], ref[k]), k


def test_run_render_with_dual_quaternions_and_a_frame_rate(dev, tmp_path):
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
    motion = np.zeros((7, 3 + 3 * len(names)))
    motion[:, :3] = off[0]
    motion[:, 3 + 3 * 5] = np.arange(7) * 9.0                          # left shoulder, Z rotation
    motion[:, 3 + 3 * 6 + 1] = np.arange(7) * 20.0                     # left elbow, X rotation: a twist about its bone
    os.makedirs(os.path.join(mesh_dir, "bvh_files"))
    bvh = os.path.join(mesh_dir, "bvh_files", "wave.bvh")
    with open(bvh, "w") as fh:
        fh.write(R.bvh_text(names, parents, off * 100.0, {j: o * 100.0 for j, o in ends.items()}, chans,
                            motion * np.r_[[100.0] * 3, [1.0] * (3 * len(names))], frame_time=0.04))
    args = ["--data_dir", root, "--uid", uid, "--test", "--device", str(dev)]
    out_dir, rendered = run_render.run(args + ["--skinning", "dual_quaternion", "--fps", "15"])
    assert out_dir == os.path.join(mesh_dir, "blender_render", "wave")
    with np.load(os.path.join(mesh_dir, "skin_weights.npz")) as z:
        infl, w = z["influences"], z["weights"]
    stamp = os.path.getmtime(os.path.join(mesh_dir, "skin_weights.npz"))
    ov, of, oc = animate.read_obj(obj)
    fsk, fclip = animate.fit_to_mesh(*animate.read_bvh(bvh), ov)
    assert fclip.n_frames == 7 and fclip.frame_time == 0.04
    slow = animate.resample_clip(fclip, 1.0 / 15.0)
    assert slow.n_frames == 4                                          # 0.24 s at 15 frames / s: 0, 1/15, 2/15, 3/15
    mem = animate.animate_mesh(ov, of, oc, fsk, slow, weights=(infl, w), device=dev, skinning="dual_quaternion")

    def same_as_folder(mem, n):
        for sub in ("color", "pos", "edge"):
            assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["%04d.png" % (i + 1) for i in range(n)]
            for i in range(n):
                png = np.asarray(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
                assert np.array_equal(png, mem[sub][i].cpu().numpy()), (sub, i)

    same_as_folder(mem, 4)
    assert torch.equal(rendered["vertices"], mem["vertices"])
    # without the two flags: the linear blend of every frame of the clip, from the same cached weights
    for sub in ("color", "pos", "edge"):
        for name in os.listdir(os.path.join(out_dir, sub)):
            os.remove(os.path.join(out_dir, sub, name))
    _, plain = run_render.run(args)
    assert os.path.getmtime(os.path.join(mesh_dir, "skin_weights.npz")) == stamp
    lin = animate.animate_mesh(ov, of, oc, fsk, fclip, weights=(infl, w), device=dev, skinning="linear")
    same_as_folder(lin, 7)
    assert torch.equal(plain["vertices"], lin["vertices"]) and plain["vertices"].shape[0] == 7
