"""GPU: centre-of-rotation skinning (cor_rows_kernel, cor_centres_kernel, cor_centres_wide_kernel,
cor_reduce_kernel and skin_cor_kernel of csrc/mesh_skin.hip) against the host entries that compile the
same text (csrc/cor_blend.h), then through animate_mesh and run_render.

Centres: the device partitions the triangle range and has its own exp, so it is held to the host
entry within B = 2 (T + 1 / sigma^2 + 64) 2^-52 times the bounding-box diagonal per coordinate, with
`valid` equal; the tests print the largest error / B.  Apply: byte-equal to dsu_skin_cor_host on the
device's own centres (the same text and flags, IEEE float64 division and square root on both sides);
the tests print the number of coordinates that differ and assert 0."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import corrective_ref as CR
import skin_cor_ref as C
import skin_dqs_ref as D
import skin_ref as R
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _centres(dev, rest, faces, infl, w, J, sigma=0.1):
    cen, val = ops.skin_cor_centres(_t(rest, dev), _t(np.asarray(faces, np.int32).reshape(-1, 3), dev), infl, w, J,
                                    sigma=sigma)
    assert cen.is_cuda and cen.dtype == torch.float64 and val.dtype == torch.uint8
    return cen, val


def _against_host(tag, dev, rest, faces, joints, cw, J, sigma=0.1):
    cen, val = _centres(dev, rest, faces, joints, cw, J, sigma)
    got, gv = cen.cpu().numpy(), val.cpu().numpy()
    host, hv = C.host_centres(rest, faces, joints, cw, J, sigma)
    T = len(np.asarray(faces).reshape(-1, 3))
    B = C.centre_bound(rest, T, sigma)
    err = float(np.abs(got - host).max())
    parts, per, tile = C.plan(len(rest), T)
    used = -(-(-(-T // tile)) // per)
    print(f"[cor] {tag}: V {len(rest)} T {T} K {joints.shape[1]} J {J}: {int(gv.sum())} valid; {used} of {parts} "
          f"partitions hold triangles; largest |device - host| / B = {err / B if B else 0.0:.4f}")
    assert np.array_equal(gv, hv)
    assert err <= B
    return got, gv


# ------------------------------------------------------------------ centres
@pytest.mark.parametrize("name,K,J,sigma", [("tube", 1, 9, 0.1), ("tube", 4, 9, 0.1), ("sphere", 4, 9, 0.05),
                                            ("sphere", 9, 9, 0.1), ("tube", 2, 2, 0.1), ("sphere", 4, 19, 0.1)])
def test_device_centres_within_the_bound_of_the_host_entry(dev, name, K, J, sigma):
    """K = 9 takes the kernel that reads both rows from memory; J = 2 has rows shorter than 3K, J = 19
    rows of the full 3K; the sphere's 1280 faces are 20 tiles for 16 partitions: two each, the last six
    empty."""
    v, f, joints, cw, _, _ = C.mesh_case(name, K, J)
    got, gv = _against_host(f"{name} sigma {sigma}", dev, v, f, joints, cw, J, sigma)
    assert gv.all() == (K > 1) and gv.any() == (K > 1)


@pytest.mark.parametrize("K", [4, 9])
@pytest.mark.parametrize("T", [0, 1, 63, 64, 65, 1024, 1025])
def test_face_counts_around_the_tile_and_the_partitions(dev, K, T):
    """The first T faces of the sphere (V = 642: 16 partitions).  1, 63, 64, 65: one tile less one, one
    tile, one tile and one triangle, all in partition 0 or 0 and 1; 1024: one tile in each partition;
    1025: 17 tiles, two per partition, the last seven partitions empty."""
    v, f, joints, cw, _, _ = C.mesh_case("sphere", K)
    parts, per, tile = C.plan(len(v), T)
    assert (parts, tile) == (16, 64) and per == (2 if T == 1025 else 1)
    _against_host("first faces", dev, v, f[:T], joints, cw, 9)


@pytest.mark.parametrize("T", [1, 63, 65, 1025])
@pytest.mark.parametrize("K,J", [(4, 19), (2, 2)])
def test_odd_face_counts_with_an_even_row_width(dev, K, J, T):
    """T (1 + min(3K, J)) odd — rows of 12 (K 4, J 19) or 2 (J 2) pairs and an odd face count: the int32
    part of the workspace is an odd number of words, and the size is whole doubles all the same."""
    from drawingspinup_amd import _lib
    v, f, joints, cw, _, _ = C.mesh_case("sphere", K, J)
    rw = min(3 * joints.shape[1], J)
    assert rw % 2 == 0 and (T * (1 + rw)) % 2 == 1
    nbytes = _lib.lib().dsu_skin_cor_centres_workspace_bytes(len(v), T, joints.shape[1], J)
    parts, per, tile = C.plan(len(v), T)
    assert nbytes % 8 == 0 and nbytes >= (parts * len(v) * 4 + T * 4 + T * rw) * 8 + (T + T * rw) * 4
    _against_host("odd faces, even rows", dev, v, f[:T], joints, cw, J)


@pytest.mark.parametrize("V", [1, 255, 256, 257])
def test_vertex_counts_around_the_workgroup(dev, V):
    """The first V vertices of the tube with all its faces: those that reach past V are skipped."""
    v, f, joints, cw, _, _ = C.mesh_case("tube", 4)
    got, gv = _against_host("first vertices", dev, v[:V], f, joints[:V], cw[:V], 9)
    assert gv.any() == (V > 1)


def test_edge_rows_and_the_character(dev):
    v, f, infl, w, J = C.character()
    joints, cw = C.canonical(infl, w, J)
    _against_host("character", dev, v, f, joints, cw, J)
    # faces out of range, of zero area and at a NaN vertex; the wrapper's table from a caller's
    v, f, _, _, infl, w = C.mesh_case("tube", 4)
    V0 = len(v)
    v = np.concatenate([v, [[0.3, 0.2, 0.1], [np.nan, 0.0, 0.0]]]).astype(np.float32)
    f = np.concatenate([f, [[0, 1, V0 + 2], [-1, 2, 3], [7, 7, 8], [0, 1, V0 + 1]]])
    infl = np.concatenate([infl, [[7, 8, -1, -1], [0, 1, 2, 3]]]).astype(np.int32)
    w = np.concatenate([w, [[0.5, 0.5, 0, 0], [0.25] * 4]]).astype(np.float32)
    infl[infl >= 7] = 6
    infl[V0] = [7, 8, -1, -1]
    infl[0, 0], w[1, 0], w[2, 1], w[3, 2] = 99, 0.0, -0.25, np.nan
    infl[4, 1] = infl[4, 0]
    joints, cw = C.canonical(infl, w, 9)
    got, gv = _against_host("edge rows", dev, v, f, joints, cw, 9)
    assert gv[V0] == 0 and np.isfinite(got).all()
    # the wrapper makes the same table from the caller's
    cen, val = _centres(dev, v, f, infl, w, 9)
    assert C.same_bits(cen.cpu().numpy(), got) and np.array_equal(val.cpu().numpy(), gv)
    # a table made elsewhere with weights of 0 inside rows, straight to the C entry (the wrapper would
    # drop them): zero factors contribute nothing on the device as on the host
    zw = cw.copy()
    zw[10, 1], zw[11, 0] = 0.0, 0.0
    zw[12, 1:] = 0.0
    rest, faces = _t(v, dev), _t(f.astype(np.int32), dev)
    tj, tw = _t(joints, dev), _t(zw, dev)
    from drawingspinup_amd import _lib
    lib, ptr = _lib.lib(), _lib.ptr
    nbytes = lib.dsu_skin_cor_centres_workspace_bytes(len(v), len(f), joints.shape[1], 9)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    zc = torch.zeros((len(v), 3), dtype=torch.float64, device=dev)
    zv = torch.zeros(len(v), dtype=torch.uint8, device=dev)
    assert lib.dsu_skin_cor_centres(ptr(rest), ptr(faces), ptr(tj), ptr(tw), len(v), len(f), joints.shape[1], 9, 0.1,
                                    ptr(ws), nbytes, ptr(zc), ptr(zv), _lib.stream()) == 0
    hc, hv = C.host_centres(v, f, joints, zw, 9, 0.1)
    assert np.array_equal(zv.cpu().numpy(), hv) and hv[12] == 0
    assert np.abs(zc.cpu().numpy() - hc).max() <= C.centre_bound(v, len(f), 0.1)


def test_centres_two_runs_and_a_side_stream_give_the_same_bits(dev):
    for K in (4, 9):
        v, f, joints, cw, _, _ = C.mesh_case("sphere", K)
        first = _centres(dev, v, f, joints, cw, 9)
        second = _centres(dev, v, f, joints, cw, 9)
        torch.cuda.synchronize(dev)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            third = _centres(dev, v, f, joints, cw, 9)
        side.synchronize()
        for a, b in zip(first, second):
            assert torch.equal(a, b)
        for a, b in zip(first, third):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ apply
@functools.lru_cache(maxsize=None)
def _apply_inputs(K, F):
    name = "tube" if F == 1 else "sphere"
    v, f, joints, cw, infl, w = C.mesh_case(name, K)
    mats = D.random_transforms(np.random.default_rng(K * 1000 + F), F, 9)
    return v, f, infl, w, mats, C.quats_of(mats)


def _cor(dev, rest, infl, w, mats, quats, cen, val):
    out = ops.skin_cor(_t(rest, dev), _t(infl, dev), _t(w, dev), _t(mats, dev), _t(quats, dev), cen, val)
    assert out.is_cuda and out.dtype == torch.float32
    return out


@pytest.mark.parametrize("K,F", [(1, 1), (4, 1), (4, 120), (9, 120)])
def test_device_apply_equals_the_host_entry_byte_for_byte(dev, K, F):
    v, f, infl, w, mats, quats = _apply_inputs(K, F)
    cen, val = _centres(dev, v, f, infl, w, 9)
    got = _cor(dev, v, infl, w, mats, quats, cen, val).cpu().numpy()
    host = C.host_cor(v, infl, w, mats, quats, cen.cpu().numpy(), val.cpu().numpy())
    n = int((got.view(np.uint32) != host.view(np.uint32)).sum())
    print(f"[cor] apply K {K} F {F}: {n} of {got.size} coordinates differ from dsu_skin_cor_host; "
          f"{int(val.sum())} of {len(v)} centres valid")
    assert got.shape == (F, len(v), 3)
    assert C.same_bits(got, host)
    assert bool(val.any()) == (K > 1)


def test_apply_edge_rows_give_the_host_entry_s_bytes(dev):
    rest, infl, w, mats, quats, cen, val, linear_rows = C.edge_rows()
    got = _cor(dev, rest, infl, w, mats, quats, _t(cen, dev), _t(val, dev)).cpu().numpy()
    assert C.same_bits(got, C.host_cor(rest, infl, w, mats, quats, cen, val))
    lin = _cor(dev, rest, infl, w, mats, quats, _t(cen, dev), _t(np.zeros_like(val), dev)).cpu().numpy()
    for row in linear_rows:
        assert C.same_bits(got[:, row], lin[:, row]), row


def test_apply_two_runs_and_a_side_stream_give_the_same_bits(dev):
    v, f, infl, w, mats, quats = _apply_inputs(4, 120)
    cen, val = _centres(dev, v, f, infl, w, 9)
    a = [_t(x, dev) for x in (v, infl, w, mats, quats)] + [cen, val]
    first = ops.skin_cor(*a)
    second = ops.skin_cor(*a)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = ops.skin_cor(*a)
    side.synchronize()
    assert torch.equal(first, second) and torch.equal(first, third)


# ------------------------------------------------------------------ through the layers
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


def _swing(sk, n=12):
    """The swing of tests/test_gpu_skin.py: the left elbow turns about z, the right knee about x."""
    clip = animate.rest_clip(sk, n)
    for k in range(n):
        a = 40.0 * np.sin(2 * np.pi * k / n)
        clip.rotations[k, 6] = R.rot("Z", a)
        clip.rotations[k, 17] = R.rot("X", 0.7 * a)
    return clip


def test_animate_mesh_with_centres_of_rotation(dev):
    v, f, c, sk = _character()
    infl, w = _weights(dev)
    w = w.copy()
    w[::3] = [1.0, 0.0, 0.0, 0.0]                     # every third vertex on its first influence alone
    clip = _swing(sk)
    got = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning="centre_of_rotation")
    mats = animate.skinning_matrices(sk, clip)
    cen, val = ops.skin_cor_centres(_t(v, dev), _t(f.astype(np.int32), dev), infl, w, len(sk.names))
    direct = ops.skin_cor(_t(v, dev), _t(infl, dev), _t(w, dev), _t(mats, dev),
                          _t(animate.rotation_quaternions(mats[..., :3]), dev), cen, val)
    assert got["vertices"].is_cuda and got["vertices"].shape == (12, len(v), 3)
    assert torch.equal(got["vertices"], direct)
    assert torch.equal(got["cor_centres"][0], cen) and torch.equal(got["cor_centres"][1], val)
    assert 0 < int(val.sum()) < len(v)
    # animate.cor_centres is the same call, and handing the centres back gives the same frames
    again = animate.cor_centres(v, f, (infl, w), len(sk.names), device=dev)
    assert torch.equal(again[0], cen) and torch.equal(again[1], val)
    reuse = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning="centre_of_rotation",
                                 centres=got["cor_centres"])
    for k in ("vertices", "color", "pos", "edge", "frames"):
        assert torch.equal(reuse[k], got[k]), k
    # a vertex bound to one joint has no centre and follows that joint within the linear blend's bound
    single = np.flatnonzero(w[:, 0] == 1.0)
    assert len(single) >= len(v) // 3 and not val.cpu().numpy()[single].any()
    m = mats[:, infl[single, 0]]
    x = v[single].astype(np.float64)
    rigid = np.einsum("fvab,vb->fva", m[..., :3], x) + m[..., 3]
    scale = np.einsum("fvab,vb->fva", np.abs(m[..., :3]), np.abs(x)) + np.abs(m[..., 3])
    verts = got["vertices"].cpu().numpy().astype(np.float64)
    assert (np.abs(verts[:, single] - rigid) <= (2 * 4 + 4) * C.EPS32 * scale).all()
    # the same outputs, in the same shapes, as the other blends, and another blend than both
    lin = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning="linear")
    dqs = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning="dual_quaternion")
    assert set(got) == set(lin) | {"cor_centres"} and "cor_centres" not in dqs
    for k in ("color", "pos", "edge", "frames", "vertices"):
        assert got[k].shape == lin[k].shape and got[k].dtype == lin[k].dtype, k
    assert not torch.equal(got["vertices"], lin["vertices"]) and not torch.equal(got["vertices"], dqs["vertices"])
    assert (got["color"][..., 3].reshape(12, -1).amax(1) == 255).all()
    # corrective smoothing composes with it unchanged
    smooth = animate.animate_mesh(v, f, c, sk, clip, weights=(infl, w), device=dev, skinning="centre_of_rotation",
                                  centres=got["cor_centres"], corrective_iterations=2)
    topo = ops.corrective_topology(animate.smoothing_topology(v.astype(np.float64), f), dev)
    delta, ok = ops.corrective_bind(_t(v, dev), topo, 0.5, 2)
    assert torch.equal(smooth["vertices"], ops.corrective_smooth(direct, topo, delta, ok, 0.5, 2))


def test_run_render_with_centres_of_rotation(dev, tmp_path):
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
    motion[:, 3 + 3 * 5] = np.arange(4) * 12.0                         # left shoulder, Z rotation
    motion[:, 3 + 3 * 6] = np.arange(4) * 30.0                         # left elbow, Z rotation: a bend
    os.makedirs(os.path.join(mesh_dir, "bvh_files"))
    bvh = os.path.join(mesh_dir, "bvh_files", "wave.bvh")
    with open(bvh, "w") as fh:
        fh.write(R.bvh_text(names, parents, off * 100.0, {j: o * 100.0 for j, o in ends.items()}, chans,
                            motion * np.r_[[100.0] * 3, [1.0] * (3 * len(names))], frame_time=0.04))
    args = ["--data_dir", root, "--uid", uid, "--test", "--device", str(dev)]
    # without the flag: the linear call, and no skin_cor.npz
    out_dir, plain = run_render.run(args)
    cache, wpath = os.path.join(mesh_dir, "skin_cor.npz"), os.path.join(mesh_dir, "skin_weights.npz")
    assert not os.path.exists(cache)
    with np.load(wpath) as z:
        infl, w = z["influences"], z["weights"]
    with open(wpath, "rb") as fh:
        weight_bytes = fh.read()
    stamp = os.path.getmtime(wpath)
    ov, of, oc = animate.read_obj(obj)
    fsk, fclip = animate.fit_to_mesh(*animate.read_bvh(bvh), ov)

    def folder():
        return {sub: [np.asarray(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1)))) for i in range(4)]
                for sub in ("color", "pos", "edge")}

    def same_as_folder(mem):
        pngs = folder()
        for sub in pngs:
            assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["%04d.png" % (i + 1) for i in range(4)]
            for i in range(4):
                assert np.array_equal(pngs[sub][i], mem[sub][i].cpu().numpy()), (sub, i)
        return pngs

    lin = animate.animate_mesh(ov, of, oc, fsk, fclip, weights=(infl, w), device=dev)
    same_as_folder(lin)
    assert torch.equal(plain["vertices"], lin["vertices"])
    # with it: the in-memory frames, and the centres are stored
    _, rendered = run_render.run(args + ["--skinning", "centre_of_rotation"])
    mem = animate.animate_mesh(ov, of, oc, fsk, fclip, weights=(infl, w), device=dev, skinning="centre_of_rotation")
    first = same_as_folder(mem)
    assert torch.equal(rendered["vertices"], mem["vertices"]) and not torch.equal(mem["vertices"], lin["vertices"])
    with np.load(cache) as z:
        assert list(z["joints"]) == list(fsk.names) and int(z["n_faces"]) == len(of) and float(z["sigma"]) == 0.1
        assert C.same_bits(z["centres"], mem["cor_centres"][0].cpu().numpy())
        assert np.array_equal(z["valid"], mem["cor_centres"][1].cpu().numpy())
    # a second run reads the stored centres (the file is not rewritten) and writes the same bytes
    cstamp = os.path.getmtime(cache)
    _, second = run_render.run(args + ["--skinning", "centre_of_rotation"])
    assert os.path.getmtime(cache) == cstamp and torch.equal(second["vertices"], mem["vertices"])
    again = folder()
    assert all(np.array_equal(a, b) for sub in first for a, b in zip(first[sub], again[sub]))
    assert os.path.getmtime(wpath) == stamp
    with open(wpath, "rb") as fh:
        assert fh.read() == weight_bytes
