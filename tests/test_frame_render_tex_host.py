"""CPU: the host side of the textured frames — the textured OBJ reader, the float64 restatement of
the sampling rule (tests/frame_render_tex_ref.py) on hand-computed answers, the argument checks of the
entry point with a tex (listed in test_frame_render_host.render_entry_refusals) and run_render's
refusal of an untextured OBJ."""
import os

import numpy as np
import pytest

import frame_render_ref as R
import frame_render_tex_ref as TR
from drawingspinup_amd import animate
from drawingspinup_amd.nsr.mesh import write_obj, write_obj_textured


# ------------------------------------------------------------------ read_obj_textured
def test_read_obj_textured_inverts_write_obj_textured(tmp_path):
    rng = np.random.default_rng(0)
    v = rng.normal(size=(41, 3))
    f = rng.integers(0, 41, size=(60, 3))                   # not every vertex first used in file order
    uvs = rng.random((41, 2)).astype(np.float32)
    image = rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)
    path = write_obj_textured(str(tmp_path / "m" / "a.obj"), v, f, uvs, image, "a")
    v2, f2, uv2, im2 = animate.read_obj_textured(path)
    assert v2.dtype == np.float64 and f2.dtype == np.int64 and uv2.dtype == np.float32 and im2.dtype == np.uint8
    assert np.array_equal(f2, f)
    assert np.array_equal(im2, image)
    assert np.array_equal(v2, np.array([[float("%.8f" % x) for x in row] for row in v]))
    # the file's 9 decimals, then f32
    printed = np.array([[float("%.9f" % x) for x in row] for row in uvs.astype(np.float64)])
    assert np.array_equal(uv2, printed.astype(np.float32))
    assert np.abs(uv2.astype(np.float64) - uvs).max() <= 0.5e-9 + 2.0 ** -24
    # read_obj itself is what it was: one nearest texel per vertex
    v3, f3, c3 = animate.read_obj(path)
    assert np.array_equal(f3, f) and c3.shape == (41, 3)


def test_read_obj_textured_splits_a_vertex_used_with_two_uvs(tmp_path):
    image = np.arange(2 * 2 * 3, dtype=np.uint8).reshape(2, 2, 3)
    write_obj_textured(str(tmp_path / "t.obj"), np.zeros((3, 3)), np.array([[0, 1, 2]]), np.zeros((3, 2)), image, "t")
    p = tmp_path / "t.obj"
    p.write_text("mtllib t.mtl\nusemtl t\n"
                 "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\n"
                 "vt 0.1 0.1\nvt 0.2 0.2\nvt 0.3 0.3\nvt 0.4 0.4\n"
                 "f 1/3 2/1 3/2\n"
                 "f 1/3 3/4 4/4\n")                         # vertex 3 comes with vt 2 and with vt 4
    v, f, uv, im = animate.read_obj_textured(str(p))
    # first-use order of the (v, vt) pairs: (1,3) (2,1) (3,2) (3,4) (4,4)
    assert f.tolist() == [[0, 1, 2], [0, 3, 4]]
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 0], [0, 1, 0]]
    assert np.array_equal(uv, np.array([[0.3, 0.3], [0.1, 0.1], [0.2, 0.2], [0.4, 0.4], [0.4, 0.4]], np.float32))
    assert np.array_equal(im, image)


def test_read_obj_textured_says_why_it_refuses(tmp_path):
    rng = np.random.default_rng(1)
    v, f = rng.normal(size=(5, 3)), np.array([[0, 1, 2], [2, 3, 4]])
    plain = write_obj(str(tmp_path / "plain.obj"), v, f, rng.random((5, 3)))
    with pytest.raises(ValueError, match="vt"):
        animate.read_obj_textured(plain)
    # a vt index out of range
    image = np.zeros((4, 4, 3), np.uint8)
    path = write_obj_textured(str(tmp_path / "a.obj"), v, f, rng.random((5, 2)), image, "a")
    txt = open(path).read()
    open(path, "w").write(txt.replace("f 3/3 4/4 5/5", "f 3/3 4/4 5/6"))
    with pytest.raises(ValueError, match="vt index out of range"):
        animate.read_obj_textured(path)
    open(path, "w").write(txt)
    assert animate.read_obj_textured(path)[1].tolist() == f.tolist()
    # the texture: not square, then missing
    from PIL import Image
    Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(str(tmp_path / "a.png"))
    with pytest.raises(ValueError, match="square"):
        animate.read_obj_textured(path)
    os.remove(str(tmp_path / "a.png"))
    with pytest.raises(ValueError, match="map_Kd"):
        animate.read_obj_textured(path)
    os.remove(str(tmp_path / "a.mtl"))
    with pytest.raises(ValueError, match="map_Kd"):
        animate.read_obj_textured(path)


# ------------------------------------------------------------------ the restatement's two filters
# rows top to bottom; row r, column c holds uv T = (c, 1 - r)
TEX2 = np.array([[[10, 20, 30], [50, 60, 70]],
                 [[90, 100, 110], [200, 220, 240]]], np.uint8)


def _sample(uvs, filter):
    uvs = np.asarray(uvs, np.float64)
    tx, ty = TR.texel_coordinates(uvs[:, 0], uvs[:, 1], 2)
    return TR.sample(TEX2, tx, ty, filter)


def test_restatement_on_a_two_by_two_texture():
    f32 = lambda a: (np.asarray(a, np.float32) / np.float32(255.0)).astype(np.float64)
    # texel centres: uv T = (0,0) bottom-left = row 1, (1,0), (0,1) = row 0, (1,1)
    centres = [[0.0, 0.0], [0.5, 0.0], [0.0, 0.5], [0.5, 0.5]]
    want = f32([TEX2[1, 0], TEX2[1, 1], TEX2[0, 0], TEX2[0, 1]])
    for flt in (TR.NEAREST, TR.BILINEAR):
        assert np.array_equal(_sample(centres, flt), want), flt
    # nearest is sample_texture per sample
    rng = np.random.default_rng(2)
    uvs = rng.uniform(-0.3, 1.3, (200, 2))
    assert np.array_equal(_sample(uvs, TR.NEAREST), animate.render.sample_texture(TEX2, uvs).astype(np.float64))
    # the half-texel point uv T = (0.5, 0.5): the mean of the four texels
    mid = _sample([[0.25, 0.25]], TR.BILINEAR)[0]
    mean = TEX2.astype(np.float64).reshape(4, 3).sum(0) * 0.25 / 255.0
    assert np.array_equal(mid, mean.astype(np.float32).astype(np.float64))
    assert mid.tolist() == [float(np.float32(x / 255.0)) for x in (87.5, 100.0, 112.5)]
    # a quarter of the way from the left column, on the bottom row: 0.75 left + 0.25 right
    q = _sample([[0.125, 0.0]], TR.BILINEAR)[0]
    assert q.tolist() == [float(np.float32((0.75 * a + 0.25 * b) / 255.0)) for a, b in zip(TEX2[1, 0], TEX2[1, 1])]
    # uv outside [0, 1]: clamped to the border texels, both filters
    outside = [[-3.0, -2.0], [7.0, -0.1], [-0.5, 9.0], [1.0, 1.0], [1e300, 1e300]]
    want = f32([TEX2[1, 0], TEX2[1, 1], TEX2[0, 0], TEX2[0, 1], TEX2[0, 1]])
    for flt in (TR.NEAREST, TR.BILINEAR):
        assert np.array_equal(_sample(outside, flt), want), flt
    # non-finite texel coordinates are taken as 0
    for flt in (TR.NEAREST, TR.BILINEAR):
        got = _sample([[np.nan, 0.5], [0.5, np.inf], [np.nan, np.nan]], flt)
        assert np.array_equal(got, f32([TEX2[0, 0], TEX2[1, 1], TEX2[1, 0]])), flt
    # T = 1
    one = np.array([[[7, 8, 9]]], np.uint8)
    for flt in (TR.NEAREST, TR.BILINEAR):
        tx, ty = TR.texel_coordinates([0.3, 5.0], [0.9, -2.0], 1)
        assert np.array_equal(TR.sample(one, tx, ty, flt), f32([[7, 8, 9]] * 2)), flt


def test_restatement_renders_the_texture_and_keeps_everything_else():
    v, f = R.quad(-0.5, -0.5, 0.5, 0.5, 0.0)
    uv = (v[:, :2] + 0.5 - 1.0 / 16.0).astype(np.float32)
    tex = np.random.default_rng(3).integers(0, 256, (8, 8, 3)).astype(np.uint8)
    pos = animate.position_colours(v).astype(np.float32)
    base = R.render_frame(v.astype(np.float32), f, np.zeros((4, 3), np.float32), pos, 0.0, 0.0, 1.0, 8, 1)
    for flt in (TR.NEAREST, TR.BILINEAR):
        out = TR.render_frame(v.astype(np.float32), f, uv, tex, pos, 0.0, 0.0, 1.0, 8, 1, flt)
        assert np.array_equal(out["color_u8"][..., :3], tex) and (out["color_u8"][..., 3] == 255).all()
        for k in ("face_id", "depth", "pos_u8", "fragile"):
            assert np.array_equal(out[k], base[k]), k
        assert np.array_equal(out["pixels"][..., 3:], base["pixels"][..., 3:])
    # every sample sits on a texel centre: all of them are half a texel from a nearest boundary
    assert not TR.render_frame(v.astype(np.float32), f, uv, tex, pos, 0, 0, 1.0, 8, 1, TR.NEAREST)["tex_fragile"].any()
    edge_uv = (v[:, :2] + 0.5).astype(np.float32)            # samples on texel boundaries: tx + 0.5 integer
    assert TR.render_frame(v.astype(np.float32), f, edge_uv, tex, pos, 0, 0, 1.0, 8, 1, TR.NEAREST)["tex_fragile"].all()
    assert not TR.render_frame(v.astype(np.float32), f, edge_uv, tex, pos, 0, 0, 1.0, 8, 1, TR.BILINEAR)["tex_fragile"].any()


# ------------------------------------------------------------------ argument checks
def test_textured_entry_point_validates_before_launching():
    from test_frame_render_host import render_entry_refusals
    for flt in (0, 1):                                      # DSU_TEX_NEAREST, DSU_TEX_BILINEAR
        render_entry_refusals(flt)


def test_textured_render_needs_the_device_and_both_arguments():
    import torch
    from drawingspinup_amd import ops
    with pytest.raises(ValueError):
        ops.texture_rgba(torch.zeros(4, 5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.texture_rgba(torch.zeros(4, 4, 3))
    assert ops.texture_rgba(torch.zeros(4, 4, 3, dtype=torch.uint8))[..., 3].eq(255).all()
    v = np.zeros((3, 3))
    with pytest.raises(ValueError, match="together"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", texture=np.zeros((2, 2, 3), np.uint8), device="cpu")
    with pytest.raises(ValueError, match="together"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", uvs=np.zeros((3, 2)), device="cpu")
    with pytest.raises(ValueError, match="texture_filter"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", texture=np.zeros((2, 2, 3), np.uint8),
                              uvs=np.zeros((3, 2)), texture_filter="cubic", device="cpu")
    with pytest.raises(ValueError):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", device="cpu")     # neither colours nor a texture


def test_run_render_atlas_refuses_a_vertex_coloured_obj(tmp_path, monkeypatch):
    from drawingspinup_amd.entry import run_render
    v, f = R.icosphere(1)
    write_obj(str(tmp_path / "uid0" / "mesh" / "m.obj"), v * 0.4, f, R.vertex_colours(len(v), 0))

    def no_render(*a, **k):
        raise AssertionError("rendering started")

    monkeypatch.setattr(animate, "render_frames", no_render)
    monkeypatch.setattr(animate, "animate_mesh", no_render)
    with pytest.raises(ValueError, match="vt"):
        run_render.run(["--data_dir", str(tmp_path), "--uid", "uid0", "--texture", "atlas"])
    with pytest.raises(SystemExit):
        run_render.run(["--data_dir", str(tmp_path), "--uid", "uid0", "--texture", "mipmap"])
