"""GPU: corrective smoothing (corrective_smooth_kernel, corrective_bind_kernel and
corrective_apply_kernel of csrc/mesh_corrective.hip) against the host entries that compile the same
text and against the unrounded float64 restatement (tests/corrective_ref.py), then through
animate_mesh and run_render.

Expected number of coordinates that differ from the host entries: 0 (the same text and flags, IEEE
float64 division and square root on both sides); the tests print the count and assert it.  Against
the unrounded restatement the bound is the one of tests/test_corrective_host.py:
2^-24 |ref64| + C (iterations + 2) 2^-24 max|x| with C = 4 x 0.6237."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import corrective_ref as CR
import skin_ref as R
from drawingspinup_amd import animate, ops
from drawingspinup_amd.animate.corrective import smoothing_topology

pytestmark = pytest.mark.gpu

C_RIGID = 4 * 0.6237
LAM = 0.5


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    v, f = {"tube": CR.tube, "icosphere": CR.icosphere}[name]()
    return v, f, smoothing_topology(v, f)


@functools.lru_cache(maxsize=None)
def _case(name, F, iterations):
    v, f, topo = _mesh(name)
    x = CR.wobble(v, F, seed=F)
    host, hdelta, hvalid = CR.host_corrective(x, v, topo, LAM, iterations)
    ref64, _, _ = CR.corrective(x, v, topo, LAM, iterations, rounded=False)
    return v, topo, x, host, hdelta, hvalid, ref64


def _device(dev, x, rest, topo, lam, iterations):
    t = ops.corrective_topology(topo, dev)
    delta, valid = ops.corrective_bind(_t(rest, dev), t, lam, iterations)
    xs = _t(x, dev)
    keep = xs.clone()
    out = ops.corrective_smooth(xs, t, delta, valid, lam, iterations)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == xs.shape
    assert delta.dtype == torch.float64 and valid.dtype == torch.uint8
    assert torch.equal(xs.view(torch.int32), keep.view(torch.int32))           # the input is never written
    return out.cpu().numpy(), delta.cpu().numpy(), valid.cpu().numpy()


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("name,F,iterations", [("tube", 1, 1), ("tube", 7, 2), ("icosphere", 120, 5), ("tube", 120, 10)])
def test_device_equal_to_the_host_entries_and_within_the_bound(dev, name, F, iterations):
    """336 and 642 vertices leave a partial block of 256; F = 120 puts the frame in blockIdx.y; 1, 2, 5
    and 10 iterations end in either half of the workspace."""
    v, topo, x, host, hdelta, hvalid, ref64 = _case(name, F, iterations)
    got, delta, valid = _device(dev, x, v, topo, LAM, iterations)
    n = int((got.view(np.uint32) != host.view(np.uint32)).sum())
    nd = int((delta.view(np.uint64) != hdelta.view(np.uint64)).sum())
    err = np.abs(got.astype(np.float64) - ref64)
    scale = float(np.abs(x).max())
    ratio = float((err / CR.bound(ref64, iterations, scale, C_RIGID)).max())
    print(f"[corrective] {name} F {F} iterations {iterations}: {n} of {got.size} coordinates differ from "
          f"dsu_corrective_smooth_host, {nd} of {delta.size} offsets from dsu_corrective_bind_host; largest "
          f"|device - ref64| / bound {ratio:.3f}")
    assert CR.same_bits(valid, hvalid) and CR.same_bits(delta, hdelta)
    assert CR.same_bits(got, host)
    assert (err <= CR.bound(ref64, iterations, scale, C_RIGID)).all()


def test_edge_rows_give_the_host_entries_bytes(dev):
    # the seam-split tube with an isolated vertex; frame 1 has displaced duplicates, frame 2 is one point
    v, f, origin = CR.split_tube()
    topo = smoothing_topology(v, f)
    wv = CR.tube()[0]
    n = len(wv)
    x = np.concatenate([CR.wobble(wv, 4, seed=21)[:, origin[:-1]], np.full((4, 1, 3), 0.25, np.float32)], 1)
    x[1, n:n + CR.RINGS] += 0.125
    x[2] = np.float32([0.3, -0.7, 0.11])
    x[3, 10 * CR.SEGS + 3, 1] = np.nan
    for lam, iterations in ((0.5, 2), (0.0, 3), (1.0, 5)):
        host, hdelta, hvalid = CR.host_corrective(x, v, topo, lam, iterations)
        got, delta, valid = _device(dev, x, v, topo, lam, iterations)
        assert CR.same_bits(delta, hdelta) and CR.same_bits(valid, hvalid)
        assert CR.same_bits(got, host), (lam, iterations)
        assert CR.same_bits(got[:, -1], x[:, -1]) and CR.same_bits(got[2], x[2])
        assert CR.same_bits(got[:, n:n + CR.RINGS], got[:, np.arange(CR.RINGS) * CR.SEGS])
        near = np.append(CR.rings_from(CR.tube()[1], 10 * CR.SEGS + 3, n) <= iterations + 1, [False] * (CR.RINGS + 1))
        assert CR.same_bits(got[3, near], x[3, near])
        assert np.isfinite(got[3, :n][~near[:n]]).all()


def test_two_runs_and_a_side_stream_give_the_same_bits(dev):
    v, topo, x, host, hdelta, hvalid, _ = _case("tube", 120, 10)
    t = ops.corrective_topology(topo, dev)
    rest, xs = _t(v, dev), _t(x, dev)
    run = lambda: ops.corrective_smooth(xs, t, *ops.corrective_bind(rest, t, LAM, 10), LAM, 10)
    first = run()
    second = run()
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert torch.equal(first, second) and torch.equal(first, third)
    assert CR.same_bits(third.cpu().numpy(), host)


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
    """The left elbow turns about z, the right knee about x, by at most 40 degrees, so it fits the window."""
    clip = animate.rest_clip(sk, n)
    for k in range(n):
        a = 40.0 * np.sin(2 * np.pi * k / n)
        clip.rotations[k, 6] = R.rot("Z", a)
        clip.rotations[k, 17] = R.rot("X", 0.7 * a)
    return clip


@pytest.mark.parametrize("skinning", ["linear", "dual_quaternion"])
def test_animate_mesh_with_corrective_smoothing(dev, skinning):
    v, f, c, sk = _character()
    infl, w = _weights(dev)
    clip = _swing(sk)
    plain = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning=skinning)
    got = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning=skinning,
                               corrective_iterations=10)
    mats = animate.skinning_matrices(sk, clip)
    if skinning == "linear":
        skinned = ops.skin_lbs(_t(v, dev), _t(infl, dev), _t(w, dev), _t(mats.astype(np.float32), dev))
    else:
        skinned = ops.skin_dqs(_t(v, dev), _t(infl, dev), _t(w, dev), _t(animate.dual_quaternions(mats), dev))
    assert torch.equal(skinned, plain["vertices"])
    topo = smoothing_topology(v, f)
    delta, valid = ops.corrective_bind(_t(v, dev), topo, 0.5, 10)
    direct = ops.corrective_smooth(skinned, topo, delta, valid, 0.5, 10)
    assert got["vertices"].is_cuda and torch.equal(got["vertices"], direct)
    assert not torch.equal(got["vertices"], plain["vertices"])
    assert set(got) == set(plain)
    for k in ("color", "pos", "edge", "frames", "vertices"):
        assert got[k].shape == plain[k].shape and got[k].dtype == plain[k].dtype, k
    window = (*got["centre"], got["size"], got["span"])
    assert window == animate.frame_window(got["vertices"].cpu().numpy())
    assert (got["color"][..., 3].reshape(30, -1).amax(1) == 255).all()         # every frame non-empty
    # 0 is off: every byte is the one written without the keyword
    off = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning=skinning,
                               corrective_iterations=0, corrective_factor=0.9)
    assert set(off) == set(plain)
    for k in ("color", "pos", "edge", "frames", "vertices"):
        assert torch.equal(off[k], plain[k]), k
    assert (off["size"], off["span"], off["centre"]) == (plain["size"], plain["span"], plain["centre"])


def test_rest_clip_stays_within_the_rest_pose_bound(dev):
    """Dual-quaternion skinning of a rest clip gives the rest mesh byte for byte, so the input is the
    identity case of the rigid-invariance bound."""
    v, f, c, sk = _character()
    infl, w = _weights(dev)
    got = animate.animate_mesh(v, f, c, sk, animate.rest_clip(sk, 2), weights=(infl, w), device=dev,
                               skinning="dual_quaternion", corrective_iterations=10)
    ref = np.broadcast_to(v.astype(np.float64), (2,) + v.shape)
    err = np.abs(got["vertices"].cpu().numpy().astype(np.float64) - ref)
    print(f"[corrective] rest clip, 10 iterations: largest |vertices - rest| {err.max():.3e}")
    assert (err <= CR.bound(ref, 10, float(np.abs(v).max()), C_RIGID)).all()


def test_run_render_with_corrective_smoothing(dev, tmp_path):
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
    motion = np.zeros((5, 3 + 3 * len(names)))
    motion[:, :3] = off[0]
    motion[:, 3 + 3 * 5] = np.arange(5) * 9.0                          # left shoulder, Z rotation
    motion[:, 3 + 3 * 6] = np.arange(5) * 15.0                         # left elbow, Z rotation: a bend
    os.makedirs(os.path.join(mesh_dir, "bvh_files"))
    bvh = os.path.join(mesh_dir, "bvh_files", "wave.bvh")
    with open(bvh, "w") as fh:
        fh.write(R.bvh_text(names, parents, off * 100.0, {j: o * 100.0 for j, o in ends.items()}, chans,
                            motion * np.r_[[100.0] * 3, [1.0] * (3 * len(names))], frame_time=0.04))
    args = ["--data_dir", root, "--uid", uid, "--test", "--device", str(dev)]
    out_dir, rendered = run_render.run(args + ["--corrective_smooth", "10"])
    assert out_dir == os.path.join(mesh_dir, "blender_render", "wave")
    npz = os.path.join(mesh_dir, "skin_weights.npz")
    with np.load(npz) as z:
        assert sorted(z.files) == ["influences", "joints", "weights"]
        infl, w = z["influences"], z["weights"]
    stamp = os.path.getmtime(npz)
    ov, of, oc = animate.read_obj(obj)
    fsk, fclip = animate.fit_to_mesh(*animate.read_bvh(bvh), ov)

    def same_as_folder(mem, n):
        for sub in ("color", "pos", "edge"):
            assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["%04d.png" % (i + 1) for i in range(n)]
            for i in range(n):
                png = np.asarray(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
                assert np.array_equal(png, mem[sub][i].cpu().numpy()), (sub, i)

    mem = animate.animate_mesh(ov, of, oc, fsk, fclip, weights=(infl, w), device=dev, corrective_iterations=10)
    same_as_folder(mem, 5)
    assert torch.equal(rendered["vertices"], mem["vertices"])
    # without the flag: the bytes of the plain call, from the same cached weights
    _, plain = run_render.run(args)
    assert os.path.getmtime(npz) == stamp
    lin = animate.animate_mesh(ov, of, oc, fsk, fclip, weights=(infl, w), device=dev)
    same_as_folder(lin, 5)
    assert torch.equal(plain["vertices"], lin["vertices"])
    assert not torch.equal(plain["vertices"], mem["vertices"])
    # the flag again: the weights are still the cached ones
    run_render.run(args + ["--corrective_smooth", "10", "--corrective_factor", "0.5"])
    assert os.path.getmtime(npz) == stamp
    same_as_folder(mem, 5)
