"""CPU: the host side of the frame rendering (drawingspinup_amd.animate), the float64 reference
rasteriser itself on analytic cases, the ISA budget of the raster / resolve kernel and the argument
checks of the new C entry points (no launch happens here: there is no GPU)."""
import ctypes
import importlib.util
import os
import shutil

import numpy as np
import pytest

import frame_render_ref as R
from drawingspinup_amd import animate
from drawingspinup_amd.nsr.mesh import write_obj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ OBJ, position colours
def test_read_obj_inverts_write_obj(tmp_path):
    rng = np.random.default_rng(0)
    v = rng.normal(size=(37, 3))
    c = rng.random((37, 3)).astype(np.float32)
    f = rng.integers(0, 37, size=(50, 3))
    path = write_obj(str(tmp_path / "m" / "a.obj"), v, f, c)
    v2, f2, c2 = animate.read_obj(path)
    assert v2.dtype == np.float64 and f2.dtype == np.int64 and c2.dtype == np.float32
    assert np.array_equal(f2, f)
    assert np.abs(v2 - v).max() <= 0.5e-8 + 1e-15          # %.8f
    assert np.abs(c2 - c).max() <= 0.5e-6 + 1e-7           # %.6f, then f32
    # the printed values themselves come back exactly
    assert np.array_equal(v2, np.array([[float("%.8f" % x) for x in row] for row in v]))
    path = write_obj(str(tmp_path / "b.obj"), v, f)
    assert animate.read_obj(path)[2] is None


def test_read_obj_rejects_what_it_cannot_render(tmp_path):
    p = tmp_path / "q.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    with pytest.raises(ValueError):
        animate.read_obj(str(p))
    p.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError):
        animate.read_obj(str(p))
    p.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nf 1/1/1 2/2/2 3/3/3\n")
    assert animate.read_obj(str(p))[1].tolist() == [[0, 1, 2]]


def test_position_colours_of_a_box():
    v = np.array([[-1.0, 2.0, 10.0], [3.0, 2.5, 10.0], [1.0, 4.0, 14.0], [0.0, 3.0, 11.0]])
    p = animate.position_colours(v)
    assert np.array_equal(p, [[0, 0, 0], [1, 0.25, 0], [0.5, 1, 1], [0.25, 0.5, 0.25]])
    flat = animate.position_colours(np.array([[0.0, 0, 5], [1, 2, 5]]))
    assert np.array_equal(flat, [[0, 0, 0], [1, 1, 0]])    # an axis without extent: 0, not nan


# ------------------------------------------------------------------ the view rule
def _box(w, h, cx=0.0, cy=0.0):
    return np.array([[[cx - w / 2, cy - h / 2, -0.3], [cx + w / 2, cy + h / 2, 0.4]]])


def test_frame_window_threshold():
    assert animate.frame_window(_box(1.0, 1.35)) == (0.0, 0.0, 512, 1.35)
    assert animate.frame_window(_box(0.4, 0.9))[2:] == (512, 1.35)
    # ratio 1.36: 512 / 1.35 * 1.36 = 515.79 -> 515 -> 516
    w = 1.36
    assert int(512 / 1.35 * w) == 515
    cx, cy, size, span = animate.frame_window(_box(w, 0.5))
    assert size == 516 and span == 1.35 * (516 / 512)
    # height decides as well as width
    assert animate.frame_window(_box(0.5, w))[2] == 516
    # a ratio whose size lands on a multiple of 4 stays there: 2.0 -> int(758.5) = 758 -> 760;
    # 1.35 * 520 / 512 + a hair -> 520
    assert int(512 / 1.35 * 2.0) == 758 and animate.frame_window(_box(2.0, 1.0))[2] == 760
    r = 1.35 * 520 / 512 + 1e-9
    assert int(512 / 1.35 * r) == 520 and animate.frame_window(_box(r, 1.0))[2:] == (520, 1.35 * (520 / 512))
    with pytest.raises(ValueError):
        animate.frame_window(_box(6.0, 1.0))               # beyond the 2048 px the rasteriser takes


def test_frame_window_centre_is_the_box_centre_over_all_frames():
    frames = np.array([[[-0.5, 0.0, 0.0], [0.1, 0.2, 0.0]],
                       [[0.3, -0.4, 0.0], [0.7, 0.6, 0.0]]])
    cx, cy, size, span = animate.frame_window(frames)
    assert (cx, cy) == ((0.7 - 0.5) / 2, (0.6 - 0.4) / 2) and size == 512
    frames[1, 1, 0] = 1.5                                   # width 2.0
    cx, cy, size, span = animate.frame_window(frames)
    assert cx == 0.5 and size == 760 and span == 1.35 * (760 / 512)


# ------------------------------------------------------------------ motions
def test_rest_rotate():
    rng = np.random.default_rng(1)
    v = rng.normal(size=(20, 3))
    fr = animate.rest_rotate(v, 24)
    assert fr.shape == (24, 20, 3)
    assert np.array_equal(fr[0], v)
    assert np.array_equal(fr[12], v * [-1, 1, -1])          # the half turn, exactly
    assert np.array_equal(fr[6], np.stack([v[:, 2], v[:, 1], -v[:, 0]], 1))   # +x went to the back
    assert np.array_equal(fr[:, :, 1], np.broadcast_to(v[:, 1], (24, 20)))
    norms = np.hypot(fr[:, :, 0], fr[:, :, 2])
    assert np.abs(norms - np.hypot(v[:, 0], v[:, 2])).max() < 1e-14
    # consecutive frames are the same turn
    a = np.arctan2(fr[1, :, 2], fr[1, :, 0]) - np.arctan2(v[:, 2], v[:, 0])
    assert np.abs(np.angle(np.exp(1j * (a + 2 * np.pi / 24)))).max() < 1e-12
    assert np.array_equal(animate.rest_pose(v), v[None])
    assert animate.motion_frames(v, fr[:3]).shape == (3, 20, 3)
    with pytest.raises(ValueError):
        animate.motion_frames(v, fr[:, :5])
    with pytest.raises(ValueError):
        animate.motion_frames(v, "walk")


# ------------------------------------------------------------------ the reference rasteriser
RED, BLUE = [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]


def _render(v, f, col, S, ss, span=1.0):
    v = np.asarray(v, np.float64)
    return R.render_frame(v.astype(np.float32), f, np.asarray(col, np.float32),
                          animate.position_colours(v).astype(np.float32), 0.0, 0.0, span, S, ss)


def test_reference_pixel_aligned_square():
    # S = 8 over span 1: pixel edges at multiples of 1/8; the square covers pixels [2,6) x [2,6)
    v, f = R.quad(-0.25, -0.25, 0.25, 0.25, 0.0)
    for ss in (1, 2, 4):
        out = _render(v, f, [RED] * 4, 8, ss)
        a = out["pixels"][..., 3]
        want = np.zeros((8, 8)); want[2:6, 2:6] = 1
        assert np.array_equal(a, want)
        assert np.array_equal(out["color_u8"][..., 3], want * 255)
        assert np.array_equal(out["color_u8"][2:6, 2:6, :3].reshape(-1, 3), [[255, 0, 0]] * 16)
        assert not out["color_u8"][want == 0].any()          # rgb = 0 where nothing is covered
        assert (out["face_id"] >= 0).sum() == 16 * ss * ss


def test_reference_half_covered_column():
    # right edge at x = 1/16: half of pixel column 4 (x in [0, 1/8)) at ss = 4
    v, f = R.quad(-0.25, -0.25, 0.0625, 0.25, 0.0)
    out = _render(v, f, [BLUE] * 4, 8, 4)
    a = out["pixels"][..., 3]
    assert np.array_equal(a[2:6, 4], [0.5] * 4) and np.array_equal(a[2:6, 2:4], np.ones((4, 2)))
    assert not a[:, 5:].any()
    assert np.array_equal(out["color_u8"][3, 4], [0, 0, 255, 128])      # straight alpha: full colour


def test_reference_nearer_quad_wins():
    v0, f0 = R.quad(-0.25, -0.25, 0.25, 0.25, -0.5)
    v1, f1 = R.quad(-0.125, -0.125, 0.375, 0.375, 0.25, first=4)
    out = _render(np.concatenate([v0, v1]), np.concatenate([f0, f1]), [RED] * 4 + [BLUE] * 4, 8, 2)
    c = out["color_u8"]
    assert c[4, 4].tolist() == [0, 0, 255, 255]              # overlap: the nearer (larger z) one
    assert c[5, 2].tolist() == [255, 0, 0, 255]              # only the far one
    assert np.array_equal(out["depth"][8, 8], np.float32(0.25))
    # the same with the face order swapped: the result does not depend on it
    out2 = _render(np.concatenate([v1, v0]), np.concatenate([f1 - 4, f0 + 4]), [BLUE] * 4 + [RED] * 4, 8, 2)
    assert np.array_equal(out2["color_u8"], c)


def test_reference_shared_edge_on_sample_centres_goes_to_the_lower_face():
    # ss = 1, S = 8: sample centres at odd multiples of 1/16.  Two coplanar quads share the edge
    # x = 1/16, which runs through the centres of column 4.
    v0, f0 = R.quad(-0.3125, -0.3125, 0.0625, 0.3125, 0.0)
    v1, f1 = R.quad(0.0625, -0.3125, 0.3125, 0.3125, 0.0, first=4)
    out = _render(np.concatenate([v0, v1]), np.concatenate([f0, f1]), [RED] * 4 + [BLUE] * 4, 8, 1)
    fid = out["face_id"]
    assert set(fid[2:6, 4].tolist()) <= {0, 1} and (fid[2:6, 5] >= 2).all()
    # inside one quad the diagonal a-c runs through sample centres too: face 0 before face 1
    assert fid[3, 3] in (0, 1) and (fid[fid >= 0] >= 0).all()
    v, f = R.quad(-0.3125, -0.3125, 0.3125, 0.3125, 0.0)
    d = _render(v, f, [RED] * 4, 8, 1)["face_id"]
    assert [d[7 - k, k] for k in range(2, 6)] == [0, 0, 0, 0]   # on the diagonal: the lower id
    assert d[5, 4] == 0 and d[2, 3] == 1                        # below / above it


def test_reference_edge_map():
    pos = np.zeros((8, 8, 4), np.uint8)
    pos[2:6, 2:6] = [100, 120, 140, 255]
    e = R.pos_edge(pos)
    # background is 2, inside is < 1: every pixel next to the silhouette boundary is an edge
    assert (e[1:7, 1:7][[0, -1]] == 0).all() and e[3, 3] == 255 and e[0, 0] == 255 and e[4, 4] == 255
    assert e[2, 2] == 0 and e[1, 1] == 0
    flat = np.full((6, 6, 4), 255, np.uint8)
    assert (R.pos_edge(flat) == 255).all()                  # reflect-101: no edge at the border


# ------------------------------------------------------------------ ISA budget
def _isa():
    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    return isa


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and not shutil.which("hipcc"),
                    reason="hipcc not available")
def test_raster_kernel_has_no_scratch_and_two_workgroups_of_lds_per_cu():
    isa = _isa()
    txt = isa.compile_asm(os.path.join(isa.CSRC, "mesh_render.hip"))
    md = isa.metadata(txt)
    seen = {}
    for name, body in isa.bodies(txt):
        short = isa.demangle_short(name)
        ops = [ln.split()[0] for ln in body if ln[:1] in " \t" and ln.split()]
        seen[short] = (md[name], ops)
    assert {f"mesh_raster_resolve_kernel<{s}>" for s in (1, 2, 4)} <= set(seen), sorted(seen)
    for short, (m, ops) in seen.items():
        assert m["scratch"] == 0 and m["vspill"] == 0 and m["sspill"] == 0, (short, m)
        assert sum(o.startswith("scratch_") for o in ops) == 0, short
        assert m["lds"] <= 64 * 1024, (short, m)
    m4, ops4 = seen["mesh_raster_resolve_kernel<4>"]
    assert m4["lds"] >= 64 * 64 * 8                         # the tile's keys live in LDS
    assert any(o.startswith("ds_max") and o.endswith("u64") for o in ops4), "visibility is an LDS 64-bit max"
    assert not any(o.startswith(("global_atomic", "buffer_atomic", "flat_atomic")) for o in ops4)
    assert m4["vgpr"] <= 128                                # four waves per SIMD by registers


# ------------------------------------------------------------------ argument checks
def render_entry_refusals(flt):
    """Every refusal of dsu_mesh_render_ortho for one colour source: flt None = tex NULL (vertex colours),
    else the DSU_TEX_* of a tex.  No call here may get as far as a launch with faces: the pointers are
    host memory.  Shared with the textured and the mip host tests."""
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    P = ctypes.c_void_p
    buf = np.zeros(4096, np.int32)                          # host memory standing in: nothing may touch it
    ws, fake = P(buf.ctypes.data), P(buf.ctypes.data)

    def call(stage=0, screen=fake, faces=fake, colour=fake if flt is None else None, pos=fake, uv=fake,
             texels=fake, T=8, flt=flt, F=1, V=3, M=1, span=1.35, S=16, ss=4, workspace=ws, wbytes=4096 * 4,
             items=fake, n_items=1):
        tex = None if flt is None else ctypes.byref(_lib.RenderTexture(uv, texels, T, flt))
        return lib.dsu_mesh_render_ortho(stage, screen, faces, colour, pos, tex, F, V, M, 0.0, 0.0, span, S, ss,
                                         workspace, wbytes, items, n_items, None, None, None, None,
                                         None, None, None)

    for stage in (0, 2):
        assert call(stage, ss=3) == -1
        assert call(stage, S=18) == -1 and call(stage, S=0) == -1 and call(stage, S=2052) == -1
        assert call(stage, workspace=None) == -1 and call(stage, wbytes=8) == -1
        assert call(stage, screen=None) == -1 and call(stage, faces=None) == -1
        assert call(stage, span=0.0) == -1 and call(stage, span=float("nan")) == -1
        assert call(stage, F=0) == -1 and call(stage, M=-1) == -1
    assert call(stage=1, items=None) == -1 and call(stage=3) == -1 and call(stage=-1) == -1
    assert call(stage=2, pos=None) == -1 and call(stage=2, items=None) == -1
    if flt is None:
        assert call(stage=2, colour=None) == -1
    else:                                                   # every call here has colour=None: it is not asked for
        assert call(stage=2, uv=None) == -1 and call(stage=2, texels=None) == -1
        assert call(stage=2, T=0) == -1 and call(stage=2, T=8193) == -1 and call(stage=2, T=-4) == -1
        assert call(stage=2, flt=3) == -1 and call(stage=2, flt=-1) == -1
        assert call(stage=2, texels=P(buf.ctypes.data + 2)) == -1       # a texel is one aligned 32-bit word
        # COUNT and FILL do not look at tex: with no faces (nothing is launched) a tex that RASTER refuses
        # field by field gets as far as tex = NULL does, past the argument checks
        for stage in (0, 1):
            plain = call(stage, M=0, flt=None, colour=fake)
            assert plain != -1 and call(stage, M=0, uv=None, texels=P(buf.ctypes.data + 2), T=-4, flt=99) == plain
    assert not buf.any()


def test_render_entry_points_validate_before_launching():
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    assert lib.dsu_mesh_render_ortho_workspace_bytes(24, 512) == (3 * 24 * 32 * 32 + 1) * 4
    assert lib.dsu_mesh_render_ortho_workspace_bytes(1, 20) == (3 * 4 + 1) * 4      # partial tiles count
    assert lib.dsu_mesh_render_ortho_workspace_bytes(1, 510) == -1
    assert lib.dsu_mesh_render_ortho_workspace_bytes(1, 2052) == -1
    assert lib.dsu_mesh_render_ortho_workspace_bytes(0, 512) == -1
    render_entry_refusals(None)
    fake = ctypes.c_void_p(np.zeros(64, np.int32).ctypes.data)
    assert lib.dsu_pos_edge_u8(None, 1, 8, 8, fake, None) == -1
    assert lib.dsu_pos_edge_u8(fake, 1, 8, 8, None, None) == -1
    assert lib.dsu_pos_edge_u8(fake, 0, 8, 8, fake, None) == -1
    assert lib.dsu_pos_edge_u8(fake, 1, 1, 8, fake, None) == -1


def test_render_needs_the_device():
    """No CPU fallback: host tensors are refused."""
    import torch
    from drawingspinup_amd import _lib, ops
    with pytest.raises(_lib.DsuError):
        ops.pos_edge_u8(torch.zeros(1, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(_lib.DsuError):
        ops.mesh_render_ortho(torch.zeros(1, 3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(3, 3),
                              torch.zeros(3, 3), 0, 0, 1.35, 16)


def test_pipeline_switch_is_validated():
    from drawingspinup_amd.drawing import DrawingPipeline
    with pytest.raises(ValueError):
        DrawingPipeline(frames="blender")
