"""The thickness map on the device (csrc/mesh_thickness.hip): dsu_mesh_thickness_ortho byte-equal to
dsu_mesh_thickness_ortho_host (the same text, csrc/mesh_thickness.h; tests/test_mesh_thickness_host.py
holds that one to the float64 restatement) in all three outputs, on that file's cases and on the
icosphere at a lattice of several workgroups; two runs and a run on a side stream give the same
bits; then the way up: lift_marks on the device against the host backend, animate_mesh with the lifted
skeleton and a retargeted clip, and run_render --marks."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import mesh_thickness_ref as R
import rig_cases as RC
import skin_ref
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu

CASES = R.cases()
CASES["e_icosphere_257x129"] = (*R.icosphere(2), -1.05, -1.02, 2.1 / 257.0, 257, 129)
NAMES = ("mid", "thickness", "count")


def _device(dev, case):
    v, f = case[:2]
    out = ops.mesh_thickness(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), *case[2:])
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_is_byte_equal_to_the_host_entry(dev, name):
    case = CASES[name]
    got, want = _device(dev, case), ops.mesh_thickness_host(*case)
    diff = {k: int((g != w).sum()) if g.shape == w.shape else -1 for k, g, w in zip(NAMES, got, want)}
    print(f"[thickness] {name}: samples that differ from the host entry {diff}; largest count {int(want[2].max(initial=0))}")
    for k, g, w in zip(NAMES, got, want):
        assert R.same_bits(g, w), (name, k)


def test_runs_and_streams_give_the_same_bits(dev):
    case = CASES["e_icosphere_257x129"]
    first = _device(dev, case)
    assert int(first[2].max()) == 2 and (first[1] > 0).sum() > 10000
    again = _device(dev, case)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = _device(dev, case)
    torch.cuda.current_stream(dev).wait_stream(side)
    for k, a, b, c in zip(NAMES, first, again, on_side):
        assert R.same_bits(a, b) and R.same_bits(a, c), k


def test_any_grid_gives_the_same_map(dev):
    """The result does not depend on the grid the triangles come through: the wrapper's cells of 16 x 16
    samples against a coarse and a fine grid of ZGrid's own choosing, called at the C level."""
    from drawingspinup_amd._lib import check, lib, ptr, stream
    v, f, x0, y0, h, W, H = CASES["e_icosphere_257x129"]
    want = ops.mesh_thickness_host(v, f, x0, y0, h, W, H)
    vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    tris = vd[fd.long()].contiguous()
    for g in (3, 40):
        grid = ops.ZGrid(tris, (-1.2, -1.2), (1.2, 1.2), cells_per_axis=g)
        mid = torch.full((H, W), -1.0, dtype=torch.float64, device=dev)
        thick, count = torch.full_like(mid, -1.0), torch.full((H, W), -1, dtype=torch.int32, device=dev)
        gx0, gy0, cell, gg, off, items = grid.args()
        check(lib().dsu_mesh_thickness_ortho(ptr(vd), len(v), ptr(fd), len(f), gx0, gy0, cell, gg, off, items,
                                             grid.items.shape[0], x0, y0, h, W, H, ptr(mid), ptr(thick), ptr(count),
                                             stream()), "dsu_mesh_thickness_ortho")
        for k, g_, w in zip(NAMES, (mid, thick, count), want):
            assert R.same_bits(g_.cpu().numpy(), w), (g, k)


# ------------------------------------------------------------------ the rig on the device
def _lifted(dev=None):
    v, f = RC.character()
    kw = dict(backend="host") if dev is None else dict(device=dev)
    return animate.lift_marks(RC.NAMES, RC.PARENTS, RC.marks(), v, f, lattice=RC.LATTICE, **kw)


def test_lift_marks_on_the_device_equals_the_host_backend(dev):
    a, b = _lifted(dev), _lifted()
    assert a.names == b.names and (a.parents == b.parents).all()
    assert R.same_bits(a.offsets, b.offsets) and sorted(a.end_sites) == sorted(b.end_sites) == [3, 6, 9, 12, 15]
    for j in a.end_sites:
        assert R.same_bits(a.end_sites[j], b.end_sites[j])
    v, f = RC.character()                                  # the default lattice of 512 as well
    a = animate.lift_marks(RC.NAMES, RC.PARENTS, RC.marks(), v, f, device=dev)
    b = animate.lift_marks(RC.NAMES, RC.PARENTS, RC.marks(), v, f, backend="host")
    assert R.same_bits(a.offsets, b.offsets) and all(R.same_bits(a.end_sites[j], b.end_sites[j]) for j in b.end_sites)


def _two_frame_clip(S):
    clip = RC.random_clip(S, 2, seed=21, max_degrees=35.0)
    clip.rotations[0] = np.eye(3)                          # frame 0: the source's rest pose
    clip.translations[0] = S.offsets[0]
    return clip


def test_animate_mesh_with_the_lifted_skeleton_and_a_retargeted_clip(dev):
    v, f = RC.character()
    colours = np.full((len(v), 3), 0.6, np.float32)
    sk, S = _lifted(dev), RC.source_skeleton()
    clip = animate.retarget_clip(S, _two_frame_clip(S), sk)
    weights = animate.bone_heat_weights(v, f, sk, device=dev)
    a = animate.animate_mesh(v, f, colours, sk, clip, weights=weights, device=dev, ss=2)
    b = animate.animate_mesh(v, f, colours, sk, clip, weights=weights, device=dev, ss=2)
    for k in ("color", "pos", "edge", "vertices"):
        assert torch.equal(a[k], b[k]), k
    assert a["color"].shape[0] == 2 and (a["color"][..., 3].reshape(2, -1).amax(1) == 255).all()
    # drawn with raised arms, driven from a T-pose: frame 0, the source's rest pose, already brings the arms down
    moved = (a["vertices"][0].cpu().numpy().astype(np.float64) - v).reshape(6, 8, 3)
    assert moved[4, :, 1].min() < -0.05 and moved[5, :, 1].min() < -0.05


def test_run_render_with_marks(dev, tmp_path):
    import yaml
    from drawingspinup_amd.entry import run_render
    from drawingspinup_amd.nsr.mesh import write_obj
    root, uid, res = str(tmp_path), "uid0", 512
    v, f = RC.character()
    mesh_dir = os.path.join(root, uid, "mesh")
    obj = os.path.join(mesh_dir, "it3000-mc512-f50000_c_r_s_cbp.obj")
    write_obj(obj, v.astype(np.float64), f, np.full((len(v), 3), 0.6, np.float32))
    # the marks in pixels of a front image of side 512: the inverse of pixels_to_mesh
    xy = RC.marks() / 1.35
    px = np.stack([(xy[:, 0] + 0.5) * (res - 1), (0.5 - xy[:, 1]) * (res - 1)], 1)
    order = [3, 2, 1, 0] + list(range(4, 16))                      # children before parents in the file
    marks = os.path.join(root, uid, "char_cfg.yaml")
    with open(marks, "w") as fh:
        yaml.safe_dump({"width": res, "height": res, "skeleton": [
            dict(name=RC.NAMES[j].upper(), parent=None if RC.PARENTS[j] < 0 else RC.NAMES[RC.PARENTS[j]].upper(),
                 loc=[float(px[j, 0]), float(px[j, 1])]) for j in order]}, fh)
    S = RC.source_skeleton()
    chans = [(["Xposition", "Yposition", "Zposition"] if j == 0 else []) + ["Zrotation", "Xrotation", "Yrotation"]
             for j in range(S.n_joints)]
    motion = np.zeros((2, 3 + 3 * S.n_joints))
    motion[:, :3] = S.offsets[0]
    motion[1, 3 + 3 * 4] = 30.0                                    # right shoulder about z
    motion[1, 3 + 3 * 11 + 1] = -40.0                              # right knee about x
    os.makedirs(os.path.join(mesh_dir, "bvh_files"))
    bvh = os.path.join(mesh_dir, "bvh_files", "wave.bvh")
    with open(bvh, "w") as fh:
        fh.write(skin_ref.bvh_text(S.names, S.parents, S.offsets, S.end_sites, chans, motion, frame_time=0.04))
    jm = {n.upper(): s for n, s in zip(RC.NAMES, S.names)}
    args = ["--data_dir", root, "--uid", uid, "--test", "--device", str(dev), "--ss", "2"]
    out_dir, rendered = run_render.run(args + ["--marks", marks, "--joint_map", json.dumps(jm)])
    assert out_dir == os.path.join(mesh_dir, "blender_render", "wave")
    assert not os.path.exists(os.path.join(mesh_dir, "skin_weights.npz"))
    npz = os.path.join(mesh_dir, "skin_weights_marks.npz")
    with np.load(npz) as z:
        assert sorted(z.files) == ["influences", "joints", "points", "weights"]
        assert sorted(z["joints"]) == sorted(n.upper() for n in RC.NAMES) and z["joints"][0] == "ROOT"
        infl, w, points, joints = z["influences"], z["weights"], z["points"], [str(n) for n in z["joints"]]
    stamp = os.path.getmtime(npz)
    # the same through the functions: marks -> mesh frame -> lifted skeleton -> retargeted clip
    ov, of, oc = animate.read_obj(obj)
    names, parents, mxy = animate.read_marks(marks)
    sk = animate.lift_marks(names, parents, animate.pixels_to_mesh(mxy, res), ov, of, device=dev)
    assert names == joints and R.same_bits(sk.rest_points(), points)
    pos, drawn = sk.rest_positions(), RC.marks()[[RC.NAMES.index(n.lower()) for n in names]]
    assert np.abs(pos[:, :2] - drawn).max() < 1e-12 and all(RC.box_of(p) is not None for p in pos)
    rclip = animate.retarget_clip(*animate.read_bvh(bvh), sk, jm)
    mem = animate.animate_mesh(ov, of, oc, sk, rclip, weights=(infl, w), device=dev, ss=2)
    assert torch.equal(rendered["vertices"], mem["vertices"])
    for sub in ("color", "pos", "edge"):
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["0001.png", "0002.png"]
        for i in range(2):
            png = np.asarray(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
            assert np.array_equal(png, mem[sub][i].cpu().numpy()), (sub, i)
    # again: the cached weights are read, not rewritten; the other flags compose
    _, again = run_render.run(args + ["--marks", marks, "--joint_map", json.dumps(jm), "--marks_res", str(res)])
    assert os.path.getmtime(npz) == stamp and torch.equal(again["vertices"], rendered["vertices"])
    _, dqs = run_render.run(args + ["--marks", marks, "--joint_map", json.dumps(jm), "--skinning", "dual_quaternion",
                                    "--corrective_smooth", "2"])
    assert os.path.getmtime(npz) == stamp and dqs["vertices"].shape == rendered["vertices"].shape
    # skin_weights.npz and skin_cor.npz belong to the runs without --marks: neither is written here
    run_render.run(args + ["--marks", marks, "--joint_map", json.dumps(jm), "--skinning", "centre_of_rotation"])
    assert not {"skin_weights.npz", "skin_cor.npz"} & set(os.listdir(mesh_dir))
    assert os.path.getmtime(npz) == stamp
    with pytest.raises(SystemExit):
        run_render.run(args + ["--joint_map", "{}"])
