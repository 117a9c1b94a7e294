"""GPU: mip-mapped frames — the atlas pyramid (csrc/mesh_mip.hip, dsu_mip_pyramid_build) and the
trilinear read of it in the resolve of the frame rasteriser (csrc/mesh_render.hip,
DSU_TEX_TRILINEAR) against known answers and the restatement of the rule
(tests/frame_render_mip_ref.py), and the way through animate and run_render."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import frame_render_mip_ref as MR
import frame_render_ref as R
import test_gpu_frame_render_tex as TX
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu

WANT = TX.WANT
GENERAL = TX.GENERAL


def _rgba(T, seed):
    return TX._random_texture(T, seed, 4)


def _masks(T, seed):
    rng = np.random.default_rng(seed)
    one = np.zeros((T, T), bool)
    one[rng.integers(T), rng.integers(T)] = True
    return {"no mask": None, "random 60 %": rng.random((T, T)) < 0.6, "all uncovered": np.zeros((T, T), bool),
            "one texel": one}


# ------------------------------------------------------------------ 1. the pyramid
@pytest.mark.parametrize("T", [1, 2, 5, 37, 64])
def test_pyramid_bytes_equal_the_restatement(dev, T):
    image = _rgba(T, 40 + T)                                 # a random alpha byte too: level 0 keeps it
    tex = TX._t(dev, image, np.uint8)
    for label, mask in _masks(T, T).items():
        cov = None if mask is None else torch.from_numpy(mask).to(dev)
        for gutter in (0, 2):
            want = MR.pyramid(image, mask, gutter)
            pyr = ops.mip_pyramid(tex, cov, gutter)
            assert (pyr.T, pyr.L) == (T, len(want)) and pyr.buffer.shape == (MR.level_offsets(T)[-1], 4)
            assert np.array_equal(pyr.buffer.cpu().numpy(), MR.flatten(want)), (label, gutter)
            assert np.array_equal(pyr.level(0).cpu().numpy(), image)
            for k in range(pyr.L):
                assert np.array_equal(pyr.level(k).cpu().numpy(), want[k]), (label, gutter, k)
            again = ops.mip_pyramid(tex, cov, gutter)
            assert torch.equal(again.buffer, pyr.buffer), (label, gutter)
    # three channels: an opaque alpha is added to level 0
    rgb = ops.mip_pyramid(tex[..., :3].contiguous())
    assert torch.equal(rgb.level(0)[..., :3], tex[..., :3]) and bool((rgb.level(0)[..., 3] == 255).all())
    assert torch.equal(rgb.buffer[T * T:], ops.mip_pyramid(tex).buffer[T * T:])


# ------------------------------------------------------------------ 2. known answers
def _uv_quad():
    """The quad [-0.25, 0.25]^2 carrying uv [0, 1]^2."""
    v, f = R.quad(-0.25, -0.25, 0.25, 0.25, 0.0)
    uv = ((v[:, :2] + 0.25) * 2.0).astype(np.float32)
    return v.astype(np.float32)[None], f, uv, np.clip(v + 0.5, 0, 1).astype(np.float32)


def test_the_aliasing_case(dev):
    """A checkerboard of 1-texel squares under a lattice of every other texel: rho = 2 exactly, so
    k = 1, t = 0 and trilinear reads the level of 128s; bilinear lands on odd texel coordinates only
    and returns one of the two colours everywhere."""
    T = 64
    yy, xx = np.mgrid[:T, :T]
    tex = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, -1)
    screen, f, uv, pos = _uv_quad()
    assert MR.footprint(*(screen[0][f[:, i]].astype(np.float64) for i in range(3)),
                        *(uv[f[:, i]].astype(np.float64) for i in range(3)), T, 1.0 / 64).tolist() == [2.0, 2.0]
    tri = TX._gpu(dev, screen, f, None, pos, 0.0, 0.0, 1.0, 64, 1, uv=uv, texture=tex, filter="trilinear")
    bil = TX._gpu(dev, screen, f, None, pos, 0.0, 0.0, 1.0, 64, 1, uv=uv, texture=tex, filter="bilinear")
    inside = (slice(0, 1), slice(17, 47), slice(17, 47))
    assert (tri["face_id"][inside] >= 0).all()
    assert (tri["color_u8"][inside][..., :3] == 128).all() and (tri["color_u8"][inside][..., 3] == 255).all()
    seen = np.unique(bil["color_u8"][inside][..., :3])
    print("bilinear on the checkerboard:", seen.tolist())
    assert len(seen) == 1 and seen[0] in (0, 255)
    for k in ("pos_u8", "face_id", "depth"):
        assert np.array_equal(tri[k], bil[k]), k


def test_magnification_is_the_bilinear_call(dev):
    screen, f, uv, pos = _uv_quad()
    tex = TX._random_texture(8, 3)
    args = (dev, screen, f, None, pos, 0.0, 0.0, 1.0, 64, 4)                 # rho = 2 * 8 / 256 < 1
    tri = TX._gpu(*args, uv=uv, texture=tex, filter="trilinear")
    bil = TX._gpu(*args, uv=uv, texture=tex, filter="bilinear")
    assert (tri["face_id"] >= 0).sum() > 10000
    for k in WANT:
        assert np.array_equal(tri[k], bil[k]), k


def test_the_pyramid_enters_through_the_colour_channels_only(dev):
    screen, f, col, pos = GENERAL["two_blobs"]
    uv = TX._general_uv(pos)
    for span, S, ss in ((1.35, 64, 2), (5.4, 32, 1)):
        args = (dev, screen, f, col, pos, 0.0, 0.0, span, S, ss)
        plain = TX._gpu(*args)
        for tex in (TX._random_texture(37, 5), _rgba(64, 6)):
            got = TX._gpu(*args, uv=uv, texture=tex, filter="trilinear")
            for k in ("pos_u8", "face_id", "depth"):
                assert np.array_equal(got[k], plain[k]), k
            assert np.array_equal(got["color_u8"][..., 3], plain["color_u8"][..., 3])
            assert np.array_equal(got["frames"][:, 3:], plain["frames"][:, 3:])
            assert np.array_equal(got["pixels"][..., 3:], plain["pixels"][..., 3:])
            assert not np.array_equal(got["color_u8"], plain["color_u8"])
        # a constant texture, every texel covered: that constant whatever rho
        k = np.array([201, 7, 98], np.uint8)
        flat = TX._gpu(dev, screen, f, np.broadcast_to(k.astype(np.float32) / np.float32(255.0), col.shape), pos,
                       0.0, 0.0, span, S, ss)
        got = TX._gpu(*args, uv=uv, texture=np.broadcast_to(k, (37, 37, 3)), filter="trilinear")
        assert np.array_equal(got["color_u8"], flat["color_u8"])
        assert np.array_equal(got["frames"], flat["frames"])


# ------------------------------------------------------------------ 3. general position
SIZE = 64
SPANS = {1: (1.35,), 2: (1.35, 5.4), 4: (1.35, 21.6)}         # the mesh at full size and 4 / 16 samples per old one
TEXTURES = (64, 37)                                           # 37: no power of two anywhere


@functools.lru_cache(maxsize=None)
def _base(name, ss, span):
    screen, f, col, pos = GENERAL[name]
    return R.render(screen, f, col, pos, 0.0, 0.0, span, SIZE, ss)


@functools.lru_cache(maxsize=None)
def _levels(T):
    rng = np.random.default_rng(70 + T)
    image = _rgba(T, 20 + T)
    covered = rng.random((T, T)) < 0.8
    return image, covered, MR.pyramid(image, covered)


def _restated(name, ss, span, T):
    screen, f, col, pos = GENERAL[name]
    return MR.render(screen, f, TX._general_uv(pos), _levels(T)[2], pos, 0.0, 0.0, span, SIZE, ss,
                     base=_base(name, ss, span))


def test_the_case_list_spans_the_levels_and_few_samples_are_fragile():
    """On the restatement alone: the faces of the cases below sit at k = 0, 1, 2 and at the top
    level, and the samples left out of the comparison (fragile visibility) stay under 4.5e-5 of the
    covered ones."""
    covered = fragile = 0
    seen = {T: set() for T in TEXTURES}
    for name in sorted(GENERAL):
        for ss, spans in SPANS.items():
            for span in spans:
                base = _base(name, ss, span)
                cov = base["face_id"] >= 0
                covered += int(cov.sum())
                fragile += int((base["fragile"] & cov).sum())
                for T in TEXTURES:
                    k = _restated(name, ss, span, T)["lod_k"][cov]
                    seen[T] |= set(np.unique(k).tolist())
    print(f"covered {covered}, fragile {fragile}, levels {seen}")
    for T in TEXTURES:
        assert {0, 1, 2, len(MR.level_sizes(T)) - 1} <= seen[T]
    assert covered > 250000 and fragile <= 4.5e-5 * covered


@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(GENERAL))
def test_general_position_against_the_restatement(dev, name, ss):
    screen, f, col, pos = GENERAL[name]
    uv = TX._general_uv(pos)
    for span in SPANS[ss]:
        base = _base(name, ss, span)
        for T in TEXTURES:
            image, covered, levels = _levels(T)
            ref = _restated(name, ss, span, T)
            pyr = ops.mip_pyramid(TX._t(dev, image, np.uint8), torch.from_numpy(covered).to(dev))
            out = ops.mesh_render_ortho(TX._t(dev, screen, np.float32), TX._t(dev, f, np.int64), None,
                                        TX._t(dev, pos, np.float32), 0.0, 0.0, span, SIZE, ss, WANT,
                                        uv=TX._t(dev, uv, np.float32), texture=TX._t(dev, image, np.uint8),
                                        filter="trilinear", pyramid=pyr)
            got = {k: v.cpu().numpy() for k, v in out.items()}
            k = ref["lod_k"][base["face_id"] >= 0]
            print(f"{name} ss={ss} span={span} T={T}: levels {np.bincount(k, minlength=len(levels)).tolist()}")
            TX._compare_with_restatement(got, ref, SIZE, ss, f"span={span} T={T}")
            ok = got["face_id"] == ref["face_id"]
            assert np.array_equal(got["depth"][ok], ref["depth"][ok])


# ------------------------------------------------------------------ 4. animation
def test_the_level_follows_the_animation(dev):
    """A clip that scales the mesh by 1, 1/2, 1/4: the footprint doubles from frame to frame, so every
    face climbs one level per frame."""
    v, f = R.noisy_icosphere(2, 0.45, 0.2, 4)
    pos = animate.position_colours(v).astype(np.float32)
    uv = TX._general_uv(pos)
    motion = np.stack([v, v * 0.5, v * 0.25])
    image, covered, _ = _levels(64)
    window, ss = (0.0, 0.0, SIZE, 2.0), 1
    levels = MR.pyramid(image)                                # render_frames: mip_coverage "all" below
    ref = MR.render(motion.astype(np.float32), f, uv, levels, pos, 0.0, 0.0, 2.0, SIZE, ss)
    med = [int(np.median(ref["lod_k"][i][ref["lod_k"][i] >= 0])) for i in range(3)]
    print("median level per frame:", med)
    assert med[1] == med[0] + 1 and med[2] == med[0] + 2
    kw = dict(ss=ss, device=dev, window=window, want=("face_id", "pixels"), texture=image, uvs=uv,
              texture_filter="trilinear", mip_coverage="all")
    a = animate.render_frames(v, f, None, motion, **kw)
    got = {"face_id": a["face_id"].cpu().numpy(), "pixels": a["pixels"].cpu().numpy(),
           "color_u8": a["color"].cpu().numpy(), "pos_u8": a["pos"].cpu().numpy(), "frames": a["frames"].cpu().numpy()}
    TX._compare_with_restatement(got, ref, SIZE, ss, "clip")
    # every frame differs from the bilinear one where the level is above 0, and the frames differ among themselves
    b = animate.render_frames(v, f, None, motion, **{**kw, "texture_filter": "bilinear"})
    assert torch.equal(a["pos"], b["pos"]) and not torch.equal(a["color"][1], b["color"][1])
    # two runs, and a run on a side stream
    again = animate.render_frames(v, f, None, motion, **kw)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        aside = animate.render_frames(v, f, None, motion, **kw)
    side.synchronize()
    for k in ("color", "pos", "edge", "frames", "face_id", "pixels"):
        assert torch.equal(a[k], again[k]) and torch.equal(a[k], aside[k]), k


def test_mip_coverage_faces_keeps_the_background_out(dev):
    """Charts over a background of another colour: with the faces' own coverage the coarse levels hold
    the charts' colour alone; with every texel covered the background bleeds in."""
    v, f = R.quad(-0.25, -0.25, 0.25, 0.25, 0.0)
    uv = (0.25 + (v[:, :2] + 0.25)).astype(np.float32)        # the chart fills the middle quarter of the atlas
    T = 64
    tex = np.zeros((T, T, 3), np.uint8)                       # black background
    cov = ops.uv_bake(TX._t(dev, uv, np.float32), TX._t(dev, f, np.int64), torch.zeros(4, 3, device=dev), T)[1] >= 0
    tex[cov.cpu().numpy()] = (200, 100, 50)
    assert 0.2 < float(cov.float().mean()) < 0.3
    kw = dict(ss=1, device=dev, window=(0.0, 0.0, 32, 4.0), texture=tex, uvs=uv, texture_filter="trilinear")
    faces = animate.render_frames(v, f, None, "rest_pose", **kw)             # rho = 4: level 2
    every = animate.render_frames(v, f, None, "rest_pose", mip_coverage="all", **kw)
    seen = faces["color"][..., 3] == 255
    assert int(seen.sum()) >= 9 and torch.equal(faces["color"][..., 3], every["color"][..., 3])
    assert bool((faces["color"][seen][:, :3] == torch.tensor([200, 100, 50], dtype=torch.uint8, device=dev)).all())
    assert bool((every["color"][seen][:, 0] < 200).any())


# ------------------------------------------------------------------ 5. files and the skinned route
def test_run_render_with_the_trilinear_filter(dev, tmp_path):
    from drawingspinup_amd.entry import run_render
    from drawingspinup_amd.nsr import mesh as M
    root, uid = str(tmp_path), "uid0"
    v, f = R.noisy_icosphere(2, 0.45, 0.3, 2)
    world = (v * [0.7, 1.2, 0.5] / 1.35 * 2.0).astype(np.float32)          # save_obj scales by ortho_scale / 2
    path = M.save_obj(os.path.join(root, uid, "mesh", "m.obj"), torch.from_numpy(world).to(dev),
                      torch.from_numpy(f).to(dev), torch.from_numpy(R.vertex_colours(len(v), 3)).to(dev),
                      export_uv=True, texture_size=1024)
    verts, faces, uvs, image = animate.read_obj_textured(path)
    common = ["--data_dir", root, "--uid", uid, "--ss", "1", "--texture", "atlas", "--device", str(dev)]
    for action, extra, n in (("rest_rotate", ["--test", "--frames", "2"], 2), ("rest_pose", [], 1)):
        for coverage in ("faces", "all"):
            out_dir, rendered = run_render.run(common + extra + ["--texture_filter", "trilinear",
                                                                 "--mip_coverage", coverage])
            assert out_dir == os.path.join(root, uid, "mesh", "blender_render", action)
            mem = animate.render_frames(verts, faces, None, action, ss=1, n_frames=2, device=dev, texture=image,
                                        uvs=uvs, texture_filter="trilinear", mip_coverage=coverage)
            assert 0.05 < float((mem["color"][..., 3] == 255).float().mean()) < 0.9
            for sub in ("color", "pos", "edge"):
                assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["%04d.png" % (i + 1) for i in range(n)]
                for i in range(n):
                    png = np.array(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
                    assert np.array_equal(png, mem[sub][i].cpu().numpy()), (action, coverage, sub, i)
            assert torch.equal(rendered["frames"], mem["frames"])
        # the filter shows: at ss 1 a 1024^2 atlas is finer than the lattice of most faces
        bil = animate.render_frames(verts, faces, None, action, ss=1, n_frames=2, device=dev, texture=image, uvs=uvs)
        assert torch.equal(bil["pos"], mem["pos"]) and not torch.equal(bil["color"], mem["color"])
    # a BVH clip: the action is named by the file; the weights come from the cache (one joint, weight 1)
    import skin_ref as SK
    names, parents, off, ends = SK.humanoid()
    chans = [(["Xposition", "Yposition", "Zposition"] if j == 0 else []) + ["Zrotation", "Xrotation", "Yrotation"]
             for j in range(len(names))]
    motion = np.zeros((2, 3 + 3 * len(names)))
    motion[:, :3] = off[0]
    motion[:, 5] = [0.0, 40.0]                                           # the root, turned about y
    mesh_dir = os.path.join(root, uid, "mesh")
    os.makedirs(os.path.join(mesh_dir, "bvh_files"))
    with open(os.path.join(mesh_dir, "bvh_files", "wave.bvh"), "w") as fh:
        fh.write(SK.bvh_text(names, parents, off, ends, chans, motion))
    one = (np.zeros((len(verts), 1), np.int32), np.ones((len(verts), 1), np.float32))
    np.savez(os.path.join(mesh_dir, "skin_weights.npz"), influences=one[0], weights=one[1], joints=np.asarray(names))
    out_dir, rendered = run_render.run(common + ["--test", "--texture_filter", "trilinear"])
    assert out_dir == os.path.join(mesh_dir, "blender_render", "wave")
    sk, clip = animate.fit_to_mesh(*animate.read_bvh(os.path.join(mesh_dir, "bvh_files", "wave.bvh")), verts)
    mem = animate.animate_mesh(verts, faces, None, sk, clip, weights=one, ss=1, device=dev, texture=image, uvs=uvs,
                               texture_filter="trilinear")
    assert not torch.equal(mem["color"][0], mem["color"][1])
    for sub in ("color", "pos", "edge"):
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["0001.png", "0002.png"]
        for i in range(2):
            png = np.array(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
            assert np.array_equal(png, mem[sub][i].cpu().numpy()), ("wave", sub, i)
            assert np.array_equal(png, rendered[sub][i].cpu().numpy())


def test_animate_mesh_rest_clip_with_the_trilinear_filter_is_rest_pose(dev):
    import skin_ref as SK
    from drawingspinup_amd.nsr import uv as U
    v, f = SK.capsule_character()
    names, parents, off, ends = SK.humanoid()
    sk = animate.Skeleton(names, parents, off, ends)
    m = U.uv_mapping(v, f, SK.vertex_colours(len(v), 8), "c", size=128, device=dev)
    v, f = m["verts"].astype(np.float32), m["faces"]
    image = TX._random_texture(128, 4)
    one = (np.zeros((len(v), 1), np.int32), np.ones((len(v), 1), np.float32))
    for coverage in ("faces", "all"):
        tex = dict(texture=image, uvs=m["uvs"], texture_filter="trilinear", mip_coverage=coverage)
        got = animate.animate_mesh(v, f, None, sk, animate.rest_clip(sk, 1), weights=one, ss=1, device=dev, **tex)
        window = (*got["centre"], got["size"], got["span"])
        ref = animate.render_frames(v, f, None, "rest_pose", ss=1, device=dev, window=window, **tex)
        for k in ("color", "pos", "edge", "frames"):
            assert torch.equal(got[k], ref[k]), (coverage, k)
        assert int((got["color"][..., 3] == 255).sum()) > 1000
