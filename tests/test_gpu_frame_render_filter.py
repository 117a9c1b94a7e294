"""GPU: the pixel filter of the frame rasteriser (dsu_mesh_render_ortho_filtered, csrc/mesh_render.hip
and csrc/film_filter.h) — against the unfiltered entry where the two must agree, against known answers,
against the float64 restatement (tests/frame_render_filter_ref.py) in general position, against the
host entry on the device's own samples, and the way through animate, run_render and the pipeline.

Sizes: S = 40 (tiles of 16 pixels: a partial tile exists), F <= 3, ss 1 / 2 / 4."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import frame_render_filter_ref as FR
import frame_render_ref as R
import frame_render_tex_ref as TR
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu

WANT = ("color_u8", "pos_u8", "face_id", "depth", "frames", "pixels")
S = 40
SPAN = 1.35
GENERAL = R.general_cases()


def _t(dev, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _gpu(dev, screen, faces, colour, pos, cx, cy, span, size, ss, want=WANT, pixel_filter=None, uv=None,
         texture=None, filter="bilinear"):
    kw = {} if texture is None else dict(uv=_t(dev, uv, np.float32), texture=_t(dev, texture, np.uint8), filter=filter)
    out = ops.mesh_render_ortho(_t(dev, screen, np.float32), _t(dev, faces, np.int64),
                                None if colour is None else _t(dev, colour, np.float32), _t(dev, pos, np.float32),
                                cx, cy, span, size, ss, want, pixel_filter=pixel_filter, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bh(width, ss):
    return animate.pixel_filter("blackman_harris", width, ss)


def _general_uv(pos):
    return (0.05 + 0.9 * pos[:, :2].astype(np.float64)).astype(np.float32)


def _random_texture(T, seed):
    return np.random.default_rng(seed).integers(0, 256, (T, T, 3)).astype(np.uint8)


# ------------------------------------------------------------------ 1. where the two entry points must agree
@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("source", ["vertex", "nearest", "bilinear", "trilinear"])
def test_ones_without_a_halo_equal_the_unfiltered_entry(dev, source, ss):
    screen, f, col, pos = GENERAL["two_blobs"]
    tex = {} if source == "vertex" else dict(uv=_general_uv(pos), texture=_random_texture(37, 3), filter=source)
    args = (screen, f, None if tex else col, pos, 0.03, -0.02, SPAN, S, ss)
    plain = _gpu(dev, *args, **tex)
    got = _gpu(dev, *args, pixel_filter=(np.ones(ss), 0), **tex)
    assert (plain["face_id"] >= 0).sum() > 300 and 0 < (plain["color_u8"][..., 3] == 255).mean() < 1
    for k in WANT:
        assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k
    box = _gpu(dev, *args, pixel_filter=animate.pixel_filter("box", None, ss), **tex)
    for k in WANT:
        assert np.array_equal(box[k].view(np.uint8), plain[k].view(np.uint8)), k


@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("width", [1.5, 3.0])
def test_face_id_and_depth_do_not_depend_on_the_filter(dev, width, ss):
    for name, (screen, f, col, pos) in GENERAL.items():
        args = (screen, f, col, pos, 0.0, 0.0, SPAN, S, ss)
        plain = _gpu(dev, *args, want=("face_id", "depth", "pos_u8"))
        got = _gpu(dev, *args, want=("face_id", "depth", "pos_u8"), pixel_filter=_bh(width, ss))
        assert np.array_equal(got["face_id"], plain["face_id"]), name
        assert np.array_equal(got["depth"].view(np.uint32), plain["depth"].view(np.uint32)), name
        # and the filter does something (width 1.5 has equal central taps and none beyond them at ss 1 and 2)
        assert width == 1.5 or not np.array_equal(got["pos_u8"], plain["pos_u8"]), name


# ------------------------------------------------------------------ 2. known answers
# span 1.25 over 40 pixels: a pixel is 1/32 wide and a sample 1/128 at ss 4, pixel (r, c) spans
# x in -0.625 + [c, c + 1] / 32, y in 0.625 - [r, r + 1] / 32
ALIGNED_SPAN = 1.25


@pytest.mark.parametrize("width", [1.5, 3.0, 5.0])
@pytest.mark.parametrize("ss", [1, 2, 4])
def test_lattice_aligned_constant_square(dev, ss, width):
    taps, halo = _bh(width, ss)
    # pixels rows 9 .. 26, columns 13 .. 33 and a quarter (ss 4: one sample column more): across both tile seams
    r0, r1, c0, c1 = 9 * ss, 27 * ss, 13 * ss, 34 * ss + (ss == 4)
    N = S * ss
    v, f = R.quad(-0.625 + c0 * 1.25 / N, 0.625 - r1 * 1.25 / N, -0.625 + c1 * 1.25 / N, 0.625 - r0 * 1.25 / N, 0.125)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    # attributes that interpolate exactly: (w0 c + w1 c + w2 c) / (w0 + w1 + w2) is c for c a power of two
    col, pos = np.tile(np.float32([0.25, 1.0, 0.5]), (4, 1)), np.tile(np.float32([0.5, 0.125, 1.0]), (4, 1))
    screen = v.astype(np.float32)[None]
    got = _gpu(dev, screen, f, col, pos, 0.0, 0.0, ALIGNED_SPAN, S, ss, pixel_filter=(taps, halo))
    want_cov = np.zeros((N, N), bool)
    want_cov[r0:r1, c0:c1] = True
    assert np.array_equal(got["face_id"][0] >= 0, want_cov)
    seen = got["pixels"][0, :, :, 3] > 0
    assert (got["color_u8"][0][seen][:, :3] == [64, 255, 128]).all() and (got["pos_u8"][0][seen][:, :3] == [128, 32, 255]).all()
    assert (got["color_u8"][0][~seen] == 0).all()

    def ratio(lo, hi):                                                      # 1-D: covered tap sum / existing tap sum
        a = np.zeros(S)
        for i in range(S):
            q = np.arange(-halo, ss + halo)
            at = i * ss + q
            exists = (at >= 0) & (at < N)
            a[i] = taps[exists & (at >= lo) & (at < hi)].sum() / taps[exists].sum()
        return a
    alpha = ratio(r0, r1)[:, None] * ratio(c0, c1)[None, :]
    assert np.abs(got["pixels"][0, :, :, 3].astype(np.float64) - alpha).max() <= 1e-7       # f32 storage
    ref = FR.render(screen, f, col, pos, 0.0, 0.0, ALIGNED_SPAN, S, ss, taps, halo)
    assert np.abs(ref["pixels"][0, :, :, 3] - alpha).max() <= 1e-12
    assert np.array_equal(got["pixels"], ref["pixels"].astype(np.float32))
    assert np.array_equal(got["color_u8"], ref["color_u8"]) and np.array_equal(got["pos_u8"], ref["pos_u8"])
    assert np.array_equal(got["frames"], R.frames_tensor(ref["color_u8"], ref["pos_u8"]))


def _cell_triangle(r, c, first):
    """A triangle inside pixel (r, c) of the aligned window that holds the pixel's centre."""
    x0, top, e = -0.625 + c / 32.0, 0.625 - r / 32.0, 1.0 / 1024
    v = np.array([[x0 + e, top - 1 / 32.0 + e, 0.0], [x0 + 1 / 32.0 - e, top - 1 / 32.0 + e, 0.0],
                  [x0 + 1 / 64.0, top - e, 0.0]])
    return v, np.array([[0, 1, 2]], np.int64) + first


@pytest.mark.parametrize("ss", [1, 2, 4])
def test_the_halo_reaches_across_tile_seams(dev, ss):
    """Triangles inside the first pixel of a tile: the pixels of the tile before it see them only if the
    (frame, triangle) pair is listed in that tile too.  Across a tile column, a tile row and a corner.
    Width 3.0 reaches one pixel (halo = ss), width 5.0 two (halo = 2 ss): column 15, and columns 14 and 15."""
    cells = [(5, 16), (16, 5), (16, 16)]
    v, f = R.merge(*[_cell_triangle(r, c, 0) for r, c in cells])
    col, pos = np.ones((9, 3), np.float32), np.full((9, 3), 0.5, np.float32)
    screen = v.astype(np.float32)[None]
    for width, reach in ((3.0, 1), (5.0, 2)):
        taps, halo = _bh(width, ss)
        assert -(-halo // ss) == reach
        got = _gpu(dev, screen, f, col, pos, 0.0, 0.0, ALIGNED_SPAN, S, ss, pixel_filter=(taps, halo))
        covered = got["face_id"][0] >= 0
        own = np.zeros((S, S), bool)
        for r, c in cells:
            own[r, c] = True
        assert np.array_equal(covered.reshape(S, ss, S, ss).any((1, 3)), own)       # the samples lie in those pixels only
        alpha = got["pixels"][0, :, :, 3]
        want = np.zeros((S, S), bool)
        for r, c in cells:
            want[r - reach:r + reach + 1, c - reach:c + reach + 1] = True
        assert np.array_equal(alpha > 0, want), width
        assert (alpha[5, 16 - reach:16] > 0).all() and (alpha[16 - reach:16, 5] > 0).all()      # tile 0 from tile 1, 0 from 3
        assert all(alpha[16 - k, 16 - k] > 0 for k in range(1, reach + 1))                      # and across the corner
        ref = FR.render(screen, f, col, pos, 0.0, 0.0, ALIGNED_SPAN, S, ss, taps, halo)
        assert np.array_equal(got["face_id"], ref["face_id"])
        assert np.abs(got["pixels"].astype(np.float64) - ref["pixels"]).max() <= 1e-7


@pytest.mark.parametrize("ss", [1, 2, 4])
def test_weights_are_renormalised_at_the_image_border(dev, ss):
    v, f = R.quad(-2.0, -2.0, 2.0, 2.0, 0.0)                              # larger than the window
    col, pos = np.tile(np.float32([1.0, 0.5, 0.25]), (4, 1)), np.tile(np.float32([0.5, 1.0, 0.125]), (4, 1))
    for width in (1.5, 3.0, 5.0):
        got = _gpu(dev, v.astype(np.float32)[None], f, col, pos, 0.0, 0.0, ALIGNED_SPAN, S, ss,
                   pixel_filter=_bh(width, ss))
        assert (got["pixels"][..., 3] == 1.0).all()
        assert (got["color_u8"] == [255, 128, 64, 255]).all() and (got["pos_u8"] == [128, 255, 32, 255]).all()
        assert (got["frames"][:, 3] == 1.0).all()


# ------------------------------------------------------------------ 3. general position
@functools.lru_cache(maxsize=None)
def _samples(name, ss):
    """The restatement's ss = 1 render on the N x N lattice: vertex colours, and the bilinear atlas (T 37)."""
    screen, f, col, pos = GENERAL[name]
    base = R.render(screen, f, col, pos, 0.0, 0.0, SPAN, S * ss, 1)
    tex = _random_texture(37, 57)
    textured = TR.render(screen, f, _general_uv(pos), tex, pos, 0.0, 0.0, SPAN, S * ss, 1, TR.BILINEAR, base=base)
    assert not textured["tex_fragile"].any()
    return base, textured, tex


@functools.lru_cache(maxsize=None)
def _unfiltered_face_id(dev, name, ss):
    screen, f, col, pos = GENERAL[name]
    return _gpu(dev, screen, f, col, pos, 0.0, 0.0, SPAN, S, ss, want=("face_id",))["face_id"]


@pytest.mark.parametrize("width", [1.5, 3.0])
@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(GENERAL))
def test_general_position_against_the_float64_restatement(dev, name, ss, width):
    """The bars of the unfiltered test: pixels to 1e-5, uint8 within one level and only within 1e-4 of a
    rounding boundary.  Excused are exactly the pixels whose footprint holds a sample whose face_id differs
    from the restatement's; every such sample must be fragile, and their set is the unfiltered call's."""
    screen, f, col, pos = GENERAL[name]
    taps, halo = _bh(width, ss)
    hp = -(-halo // ss)
    base, textured, tex = _samples(name, ss)
    covered, fragile = base["face_id"] >= 0, base["fragile"]
    assert covered.sum() > 300
    for label, samples, kw in (("vertex", base, dict(colour=col)),
                               ("bilinear", textured, dict(colour=None, uv=_general_uv(pos), texture=tex))):
        ref = FR.from_samples(samples, taps, halo, ss)
        got = _gpu(dev, screen, f, kw.pop("colour"), pos, 0.0, 0.0, SPAN, S, ss, pixel_filter=(taps, halo), **kw)
        assert np.array_equal(got["face_id"], _unfiltered_face_id(dev, name, ss))
        bad = got["face_id"] != ref["face_id"]
        assert not (bad & ~fragile).any()
        excused = FR.footprint_any(bad, halo, ss)
        assert excused.sum() <= (2 * hp + 1) ** 2 * bad.sum()
        err = np.abs(got["pixels"].astype(np.float64) - ref["pixels"])
        err[excused] = 0
        print(f"{name} ss={ss} width={width} {label}: covered {int(covered.sum())}, face_id mismatches {int(bad.sum())}, "
              f"excused pixels {int(excused.sum())}, max |pixel - restatement| {err.max():.3e}")
        assert err.max() <= 1e-5
        for key, sl in (("color_u8", slice(0, 4)), ("pos_u8", slice(4, 8))):
            d = np.abs(got[key].astype(np.int16) - ref[key].astype(np.int16))
            d[excused] = 0
            v255 = ref["pixels"][..., sl] * 255.0 + 0.5
            to_boundary = np.abs(v255 - np.round(v255)) / 255.0
            print(f"  {key}: {int((d > 0).sum())} values off by one level, max diff {int(d.max())}")
            assert d.max() <= 1
            assert (to_boundary[d > 0] <= 1e-4).all()
        assert np.array_equal(got["frames"], R.frames_tensor(got["color_u8"], got["pos_u8"]))
        ok = ~bad
        assert np.array_equal(got["depth"][ok], ref["depth"][ok])
        a = got["pixels"][..., 3]
        assert (a == 0).any() and (a == 1).any()


# ------------------------------------------------------------------ 4. determinism
def test_two_runs_and_a_side_stream_are_bit_identical(dev):
    screen, f, col, pos = GENERAL["torus"]
    args = (_t(dev, screen, np.float32), _t(dev, f, np.int64), _t(dev, col, np.float32), _t(dev, pos, np.float32),
            0.0, 0.0, SPAN, S, 4)
    flt = _bh(3.0, 4)
    a = ops.mesh_render_ortho(*args, want=WANT, pixel_filter=flt)
    b = ops.mesh_render_ortho(*args, want=WANT, pixel_filter=flt)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        c = ops.mesh_render_ortho(*args, want=WANT, pixel_filter=flt)
    side.synchronize()
    x = torch.randn(1024, 1024, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for _ in range(10):
            x = torch.tanh(x @ x * 1e-3)
    d = ops.mesh_render_ortho(*args, want=WANT, pixel_filter=flt)
    torch.cuda.synchronize(dev)
    for k in WANT:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and torch.equal(a[k], d[k]), k


# ------------------------------------------------------------------ 5. the kernel against the host entry
@pytest.mark.parametrize("source", ["vertex", "bilinear", "trilinear"])
@pytest.mark.parametrize("ss", [2, 4])
def test_kernel_equals_the_host_entry_on_the_devices_own_samples(dev, ss, source):
    """An ss = 1 render at N x N gives the device's per-sample values (its `pixels`): the same lattice, the
    same winners.  The host entry (the text the kernel compiles) resolves them; the filtered kernel at
    S = 40 must give the same bytes."""
    import ctypes
    from drawingspinup_amd import _lib
    screen, f, col, pos = GENERAL["icosphere"]
    tex = {} if source == "vertex" else dict(uv=_general_uv(pos), texture=_random_texture(37, 8), filter=source)
    colour = None if tex else col
    N = S * ss
    fine = _gpu(dev, screen, f, colour, pos, 0.0, 0.0, SPAN, N, 1, want=("pixels", "face_id"), **tex)
    covered = np.ascontiguousarray(fine["face_id"] >= 0, np.uint8)
    assert np.array_equal(covered, fine["pixels"][..., 3] == 1.0)
    s_col, s_pos = np.ascontiguousarray(fine["pixels"][..., 0:3]), np.ascontiguousarray(fine["pixels"][..., 4:7])
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    for width in (1.5, 3.0):
        taps, halo = _bh(width, ss)
        got = _gpu(dev, screen, f, colour, pos, 0.0, 0.0, SPAN, S, ss, pixel_filter=(taps, halo), **tex)
        assert np.array_equal(got["face_id"], fine["face_id"])
        host = {"pixels": np.empty((3, S, S, 8), np.float32), "color_u8": np.empty((3, S, S, 4), np.uint8),
                "pos_u8": np.empty((3, S, S, 4), np.uint8)}
        assert _lib.lib().dsu_pixel_filter_resolve_host(ptr(s_col), ptr(s_pos), ptr(covered), 3, S, ss, ptr(taps), halo,
                                                        *[ptr(host[k]) for k in host]) == 0
        for k in host:
            assert np.array_equal(got[k].view(np.uint8), host[k].view(np.uint8)), (k, width)


# ------------------------------------------------------------------ 6. plans, files, the pipeline
def test_a_plan_binned_with_one_halo_refuses_a_raster_with_another(dev):
    screen, f, col, pos = GENERAL["two_blobs"]
    args = (_t(dev, screen, np.float32), _t(dev, f, np.int64), 0.0, 0.0, SPAN, S, 4)
    tc, tp = _t(dev, col, np.float32), _t(dev, pos, np.float32)
    wide, narrow = _bh(3.0, 4), _bh(1.5, 4)
    plan = ops.MeshRenderPlan(*args, halo=wide[1]).bin()
    with pytest.raises(ValueError, match="halo"):
        plan.raster(tc, tp, taps=narrow[0])
    with pytest.raises(ValueError, match="halo"):
        plan.raster(tc, tp)
    plain = ops.MeshRenderPlan(*args).bin()
    with pytest.raises(ValueError, match="halo"):
        plain.raster(tc, tp, taps=wide[0])
    assert plan.items.numel() > plain.items.numel()                        # grown tiles list more pairs
    a = plan.raster(tc, tp, taps=wide[0])
    b = ops.mesh_render_ortho(args[0], args[1], tc, tp, *args[2:], pixel_filter=wide)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(Exception):
        ops.mesh_render_ortho(args[0], args[1], tc, tp, *args[2:], pixel_filter=(np.ones(4 + 18), 9))


def _png_bytes(out_dir):
    return {sub: [open(os.path.join(out_dir, sub, n), "rb").read() for n in sorted(os.listdir(os.path.join(out_dir, sub)))]
            for sub in ("color", "pos", "edge")}


def test_run_render_with_the_pixel_filter(dev, tmp_path, monkeypatch):
    from drawingspinup_amd.entry import run_render
    from drawingspinup_amd.nsr.mesh import write_obj
    root, uid = str(tmp_path), "uid0"
    v, f = R.noisy_icosphere(2, 0.45, 0.3, 2)
    v = v * [0.7, 1.2, 0.5]
    colours = R.vertex_colours(len(v), 3)
    write_obj(os.path.join(root, uid, "mesh", "m.obj"), v, f, colours)
    verts, faces, cols = animate.read_obj(os.path.join(root, uid, "mesh", "m.obj"))
    common = ["--data_dir", root, "--uid", uid, "--test", "--frames", "2", "--ss", "2", "--device", str(dev)]
    out_dir, rendered = run_render.run(common + ["--pixel_filter", "eevee"])
    mem = animate.render_frames(verts, faces, cols, "rest_rotate", ss=2, n_frames=2, device=dev, pixel_filter="eevee")
    for sub in ("color", "pos", "edge"):
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["0001.png", "0002.png"]
        for i in range(2):
            png = np.array(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
            assert np.array_equal(png, mem[sub][i].cpu().numpy()), (sub, i)
    assert torch.equal(rendered["frames"], mem["frames"])
    assert torch.equal(mem["edge"], ops.pos_edge_u8(mem["pos"]))
    explicit = animate.render_frames(verts, faces, cols, "rest_rotate", ss=2, n_frames=2, device=dev,
                                     pixel_filter="blackman_harris", filter_width=3.0)
    assert torch.equal(explicit["color"], mem["color"]) and torch.equal(explicit["pos"], mem["pos"])
    filtered = _png_bytes(out_dir)
    # no flags: the call as it was — the unfiltered entry point, and its bytes
    stages = []
    original = ops.MeshRenderPlan._stage

    def recording(self, stage, colour=None, pos=None, tex=None, outs=(None,) * 6, taps=None):
        stages.append((stage, self.halo, taps))
        return original(self, stage, colour, pos, tex, outs, taps)
    monkeypatch.setattr(ops.MeshRenderPlan, "_stage", recording)
    run_render.run(common)
    monkeypatch.undo()
    assert stages == [(0, 0, None), (1, 0, None), (2, 0, None)]
    plain = animate.render_frames(verts, faces, cols, "rest_rotate", ss=2, n_frames=2, device=dev)
    direct = ops.mesh_render_ortho(_t(dev, animate.rest_rotate(verts, 2), np.float32), _t(dev, faces, np.int64),
                                   _t(dev, cols, np.float32), _t(dev, animate.position_colours(verts), np.float32),
                                   *plain["centre"], plain["span"], plain["size"], 2)
    assert torch.equal(direct["color_u8"], plain["color"]) and torch.equal(direct["pos_u8"], plain["pos"])
    for sub in ("color", "pos", "edge"):
        for i in range(2):
            png = np.array(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
            assert np.array_equal(png, plain[sub][i].cpu().numpy()), (sub, i)
    unflagged = _png_bytes(out_dir)
    assert unflagged["color"] != filtered["color"] and unflagged["pos"] != filtered["pos"]
    # softer silhouettes: more partially covered pixels
    partial = lambda c: int(((c[..., 3] > 0) & (c[..., 3] < 255)).sum())
    assert partial(mem["color"]) > partial(plain["color"])


def test_animate_mesh_and_the_pipeline_pass_the_filter_on(dev):
    import skin_ref as SK
    from drawingspinup_amd.drawing import DrawingPipeline
    v, f = SK.capsule_character()
    names, parents, off, ends = SK.humanoid()
    sk = animate.Skeleton(names, parents, off, ends)
    v = v.astype(np.float32)
    col = SK.vertex_colours(len(v), 8)
    one = (np.zeros((len(v), 1), np.int32), np.ones((len(v), 1), np.float32))
    got = animate.animate_mesh(v, f, col, sk, animate.rest_clip(sk, 1), weights=one, device=dev, pixel_filter="cycles")
    window = (*got["centre"], got["size"], got["span"])
    ref = animate.render_frames(v, f, col, "rest_pose", device=dev, window=window, pixel_filter="cycles")
    plain = animate.render_frames(v, f, col, "rest_pose", device=dev, window=window)
    for k in ("color", "pos", "edge", "frames"):
        assert torch.equal(got[k], ref[k]), k
    assert not torch.equal(plain["color"], ref["color"])
    pipe = DrawingPipeline.__new__(DrawingPipeline)                        # render_mesh reads these four only
    pipe.render_ss, pipe.n_frames, pipe.device, pipe.render_filter = 2, 2, dev, "eevee"
    mesh = {"verts": v, "faces": f, "colors": col}
    frames, edge = pipe.render_mesh(mesh)
    want = animate.render_frames(v, f, col, "rest_rotate", ss=2, n_frames=2, device=dev, pixel_filter="eevee")
    assert torch.equal(frames, want["frames"]) and torch.equal(edge, want["edge"])
    pipe.render_filter = None
    frames0, _ = pipe.render_mesh(mesh)
    assert torch.equal(frames0, animate.render_frames(v, f, col, "rest_rotate", ss=2, n_frames=2, device=dev)["frames"])
    assert not torch.equal(frames0, frames)
