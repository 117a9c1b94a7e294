"""GPU: anisotropic frames — DSU_TEX_ANISOTROPIC in the resolve of the frame rasteriser
(csrc/mesh_render.hip, csrc/mip_sample.h) against known answers, the restatement of the rule
(tests/frame_render_aniso_ref.py) and the host entry that compiles the kernel's text, and the way
through ops, animate and run_render."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import frame_render_aniso_ref as AR
import frame_render_filter_ref as FR
import frame_render_mip_ref as MR
import frame_render_ref as R
import test_gpu_frame_render_mip as TM
import test_gpu_frame_render_tex as TX
import uv_ref
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu

WANT = TX.WANT
GENERAL = TX.GENERAL
SIZE, SPANS, TEXTURES = TM.SIZE, TM.SPANS, TM.TEXTURES        # the cases of the mip test, its references shared
CAPS = (2, 8)


def _gpu(dev, screen, faces, pos, cx, cy, span, S, ss, uv, texture, cap=None, filter="anisotropic", want=WANT,
         pixel_filter=None, pyramid=None):
    kw = {} if cap is None else {"max_anisotropy": cap}
    out = ops.mesh_render_ortho(TX._t(dev, screen, np.float32), TX._t(dev, faces, np.int64), None,
                                TX._t(dev, pos, np.float32), cx, cy, span, S, ss, want, uv=TX._t(dev, uv, np.float32),
                                texture=TX._t(dev, texture, np.uint8), filter=filter, pyramid=pyramid,
                                pixel_filter=pixel_filter, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. the stripe case
def _stripe_quad():
    """Two triangles, 8 samples wide and 64 tall in a 64-sample window of span 1, whose uvs put sample
    (R, C), C = 28 .. 35, on the texel point tx = 8 (C - 28) + 4, ty = 63 - R of a 64^2 atlas: u is
    compressed by 8, v by 1, every number dyadic."""
    v, f = R.quad(-0.0625, -0.5, 0.0625, 0.5, 0.0)
    uv = np.stack([(v[:, 0] + 0.0625) * 8.0, v[:, 1] + 0.5 - 1.0 / 128], 1)
    assert np.array_equal(uv.astype(np.float32).astype(np.float64), uv)
    return v.astype(np.float32)[None], f, uv.astype(np.float32), np.clip(v + 0.5, 0, 1).astype(np.float32)


def _stripes(along_rows):
    band = ((np.arange(64) // 4) % 2 * 255).astype(np.uint8)
    grey = np.broadcast_to(band[:, None] if along_rows else band[None, :], (64, 64))
    return np.ascontiguousarray(np.repeat(grey[..., None], 3, -1))


@pytest.mark.parametrize("pixel_filter", [None, "cycles"])
@pytest.mark.parametrize("ss", [1, 2])
def test_stripes_survive_along_the_axis_that_is_not_compressed(dev, ss, pixel_filter):
    screen, f, uv, pos = _stripe_quad()
    S, N = 64 // ss, 64
    flt = None if pixel_filter is None else animate.pixel_filter(pixel_filter, None, ss)
    for along_rows in (True, False):
        tex = _stripes(along_rows)
        levels = MR.pyramid(np.concatenate([tex, np.full((64, 64, 1), 255, np.uint8)], -1))
        fine = AR.render(screen, f, uv, levels, pos, 0.0, 0.0, 1.0, N, 1, 8)
        inside = fine["face_id"][0] >= 0
        assert inside.sum() == 8 * 64 and (fine["probes"][0][inside] == 8).all() and (fine["lod_k"][0][inside] == 0).all()
        ref = AR.render(screen, f, uv, levels, pos, 0.0, 0.0, 1.0, S, ss, 8) if flt is None else \
            FR.from_samples(fine, flt[0], flt[1], ss)
        got = _gpu(dev, screen, f, pos, 0.0, 0.0, 1.0, S, ss, uv, tex, 8, pixel_filter=flt)
        tri = _gpu(dev, screen, f, pos, 0.0, 0.0, 1.0, S, ss, uv, tex, filter="trilinear", pixel_filter=flt)
        assert np.array_equal(got["face_id"], fine["face_id"]) and np.array_equal(tri["face_id"], fine["face_id"])
        assert np.array_equal(got["color_u8"], ref["color_u8"])
        if flt is None:
            assert np.array_equal(got["pixels"], ref["pixels"].astype(np.float32))
        # per sample (the restatement at ss 1): exactly the band's 0 / 255 under the anisotropic rule
        # (bands along the compressed axis: column 35 is left out, its probes reach the atlas's clamped edge)
        rgb = fine["color_u8"][0][inside][:, :3]
        if along_rows:
            rows = np.nonzero(inside)[0]
            assert np.array_equal(rgb, np.repeat(((rows // 4) % 2 * 255)[:, None], 3, 1))
        else:
            assert np.isin(rgb[np.nonzero(inside)[1] < 35], (127, 128)).all()
        if flt is None:                                       # per pixel, well inside the quad
            cols = slice(28 // ss, 36 // ss if along_rows else 34 // ss)
            a, t = got["color_u8"][0, :, cols, :3], tri["color_u8"][0, :, cols, :3]
            assert np.isin(t, (127, 128)).all()
            if along_rows:
                want = np.repeat((((np.arange(S) * ss) // 4) % 2 * 255)[:, None, None], 3, 2)
                assert np.array_equal(a, np.broadcast_to(want, a.shape))
            else:
                assert np.isin(a, (127, 128)).all()


# ------------------------------------------------------------------ 2. general position
@functools.lru_cache(maxsize=None)
def _restated(name, ss, span, T, cap):
    screen, f, col, pos = GENERAL[name]
    return AR.render(screen, f, TX._general_uv(pos), TM._levels(T)[2], pos, 0.0, 0.0, span, SIZE, ss, cap,
                     base=TM._base(name, ss, span))


def test_the_case_list_spans_levels_and_probe_counts_and_few_samples_are_fragile():
    """On the restatement alone: the faces of the cases below sit on several levels and on every N from
    1 to the cap, and the samples left out of the comparison (fragile visibility) stay under 4.5e-5 of
    the covered ones."""
    covered = fragile = 0
    levels = {T: set() for T in TEXTURES}
    probes = {cap: set() for cap in CAPS}
    for name in sorted(GENERAL):
        for ss, spans in SPANS.items():
            for span in spans:
                base = TM._base(name, ss, span)
                cov = base["face_id"] >= 0
                covered += int(cov.sum())
                fragile += int((base["fragile"] & cov).sum())
                for T in TEXTURES:
                    for cap in CAPS:
                        ref = _restated(name, ss, span, T, cap)
                        levels[T] |= set(np.unique(ref["lod_k"][cov]).tolist())
                        probes[cap] |= set(np.unique(ref["probes"][cov]).tolist())
    print(f"covered {covered}, fragile {fragile}, levels {levels}, probes {probes}")
    for T in TEXTURES:
        assert {0, 1, 2} <= levels[T]
    for cap in CAPS:
        assert probes[cap] == set(range(1, cap + 1))
    assert covered > 250000 and fragile <= 4.5e-5 * covered


@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(GENERAL))
def test_general_position_against_the_restatement(dev, name, ss):
    screen, f, col, pos = GENERAL[name]
    uv = TX._general_uv(pos)
    for span in SPANS[ss]:
        base = TM._base(name, ss, span)
        for T in TEXTURES:
            image, covered, levels = TM._levels(T)
            pyr = ops.mip_pyramid(TX._t(dev, image, np.uint8), torch.from_numpy(covered).to(dev))
            for cap in CAPS:
                ref = _restated(name, ss, span, T, cap)
                got = _gpu(dev, screen, f, pos, 0.0, 0.0, span, SIZE, ss, uv, image, cap, pyramid=pyr)
                n = ref["probes"][base["face_id"] >= 0]
                print(f"{name} ss={ss} span={span} T={T} cap={cap}: probes {np.bincount(n, minlength=cap + 1).tolist()}")
                TX._compare_with_restatement(got, ref, SIZE, ss, f"span={span} T={T} cap={cap}")
                ok = got["face_id"] == ref["face_id"]
                assert np.array_equal(got["depth"][ok], ref["depth"][ok])


# ------------------------------------------------------------------ 3. the kernel against the host entry
def _host_on_device_samples(screen, f, uv, flat, T, span, N, cap, face_id):
    """dsu_aniso_sample_host on the device's own winners: face_id (F,N,N) of an ss = 1 render on the N
    lattice -> rgb (F,N,N,3) f32, 0 where empty."""
    from drawingspinup_amd import _lib
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    xs, ys = R.lattice(N, 0.0, 0.0, span)
    out = np.zeros(face_id.shape + (3,), np.float32)
    for i in range(face_id.shape[0]):
        Rr, Cc = np.nonzero(face_id[i] >= 0)
        fc = np.asarray(f)[face_id[i][Rr, Cc]]
        sv, t = screen[i].astype(np.float64), uv.astype(np.float64)
        a, b, c = sv[fc[:, 0]], sv[fc[:, 1]], sv[fc[:, 2]]
        w0, w1, w2 = R._edge(xs[Cc], ys[Rr], a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1])
        area = w0 + w1 + w2
        ta, tb, tc = t[fc[:, 0]], t[fc[:, 1]], t[fc[:, 2]]
        tx = np.ascontiguousarray((w0 * ta[:, 0] + w1 * tb[:, 0] + w2 * tc[:, 0]) / area * float(T))
        ty = np.ascontiguousarray((w0 * ta[:, 1] + w1 * tb[:, 1] + w2 * tc[:, 1]) / area * float(T))
        tri = np.ascontiguousarray(np.concatenate([a[:, :2], b[:, :2], c[:, :2]], 1))
        uv6 = np.ascontiguousarray(np.concatenate([uv[fc[:, 0]], uv[fc[:, 1]], uv[fc[:, 2]]], 1), np.float32)
        rgb = np.zeros((len(Rr), 3), np.float32)
        assert _lib.lib().dsu_aniso_sample_host(ptr(flat), T, ptr(tri), ptr(uv6), float(span) / N, ptr(tx), ptr(ty), cap,
                                                len(Rr), ptr(rgb), None, None, None) == 0
        out[i][Rr, Cc] = rgb
    return out


@pytest.mark.parametrize("cap", CAPS)
def test_kernel_equals_the_host_entry_on_the_devices_own_samples(dev, cap):
    """ss = 1: a pixel is a sample, `pixels` holds the kernel's per-sample value.  The host entry compiles
    the same text (csrc/mip_sample.h); fed the device's winners and the lattice's coordinates it must give
    the same bytes.  Then the filtered kernel at ss 2 against dsu_pixel_filter_resolve_host on those samples."""
    from drawingspinup_amd import _lib
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    screen, f, col, pos = GENERAL["icosphere"]
    uv, T, span, N = TX._general_uv(pos), 37, 2.7, 80
    image, covered, levels = TM._levels(T)
    flat = np.ascontiguousarray(MR.flatten(levels))
    pyr = ops.mip_pyramid(TX._t(dev, image, np.uint8), torch.from_numpy(covered).to(dev))
    assert np.array_equal(pyr.buffer.cpu().numpy(), flat)
    fine = _gpu(dev, screen, f, pos, 0.0, 0.0, span, N, 1, uv, image, cap, want=("pixels", "face_id"), pyramid=pyr)
    host = _host_on_device_samples(screen, f, uv, flat, T, span, N, cap, fine["face_id"])
    seen = fine["face_id"] >= 0
    assert seen.sum() > 1500
    assert np.array_equal(np.ascontiguousarray(fine["pixels"][..., :3]).view(np.uint32), host.view(np.uint32))
    ss, S = 2, N // 2
    s_col, s_pos = np.ascontiguousarray(fine["pixels"][..., 0:3]), np.ascontiguousarray(fine["pixels"][..., 4:7])
    cov8 = np.ascontiguousarray(seen, np.uint8)
    for width in (1.5, 3.0):
        taps, halo = animate.pixel_filter("blackman_harris", width, ss)
        got = _gpu(dev, screen, f, pos, 0.0, 0.0, span, S, ss, uv, image, cap, pixel_filter=(taps, halo), pyramid=pyr)
        assert np.array_equal(got["face_id"], fine["face_id"])
        res = {"pixels": np.empty((3, S, S, 8), np.float32), "color_u8": np.empty((3, S, S, 4), np.uint8),
               "pos_u8": np.empty((3, S, S, 4), np.uint8)}
        assert _lib.lib().dsu_pixel_filter_resolve_host(ptr(s_col), ptr(s_pos), ptr(cov8), 3, S, ss, ptr(taps), halo,
                                                        *[ptr(res[k]) for k in res]) == 0
        for k in res:
            assert np.array_equal(got[k].view(np.uint8), res[k].view(np.uint8)), (k, width)


# ------------------------------------------------------------------ 4. what the filter may and may not touch
def test_the_filter_enters_through_the_colour_channels_only(dev):
    screen, f, col, pos = GENERAL["two_blobs"]
    uv = TX._general_uv(pos)
    for span, S, ss in ((1.35, 64, 2), (5.4, 32, 1)):
        plain = TX._gpu(dev, screen, f, col, pos, 0.0, 0.0, span, S, ss)
        for tex in (TX._random_texture(37, 5), TX._random_texture(64, 6, 4)):
            got = _gpu(dev, screen, f, pos, 0.0, 0.0, span, S, ss, uv, tex, 8)
            for k in ("pos_u8", "face_id", "depth"):
                assert np.array_equal(got[k], plain[k]), k
            assert np.array_equal(got["color_u8"][..., 3], plain["color_u8"][..., 3])
            assert np.array_equal(got["frames"][:, 3:], plain["frames"][:, 3:])
            assert np.array_equal(got["pixels"][..., 3:], plain["pixels"][..., 3:])
            assert not np.array_equal(got["color_u8"], plain["color_u8"])
            tri = _gpu(dev, screen, f, pos, 0.0, 0.0, span, S, ss, uv, tex, filter="trilinear")
            assert not np.array_equal(got["color_u8"], tri["color_u8"])
        # a constant texture, every texel covered: that constant whatever the footprint
        k = np.array([201, 7, 98], np.uint8)
        flat = TX._gpu(dev, screen, f, np.broadcast_to(k.astype(np.float32) / np.float32(255.0), col.shape), pos,
                       0.0, 0.0, span, S, ss)
        for cap in (1, 8, 16):
            got = _gpu(dev, screen, f, pos, 0.0, 0.0, span, S, ss, uv, np.broadcast_to(k, (37, 37, 3)), cap)
            assert np.array_equal(got["color_u8"], flat["color_u8"]), cap
            assert np.array_equal(got["frames"], flat["frames"]), cap


def test_footprints_up_to_one_texel_are_the_bilinear_call(dev):
    """A window so fine that every face has s1 <= 1 (a sheared, anisotropic map of the frame's own screen
    coordinates, 0.82 texels per sample along its long axis): one probe at level 0 — the bilinear read
    of the same texels, in every output and under the pixel filter too."""
    screen, f, col, pos = GENERAL["torus"]
    screen = screen[:1]
    x, y = screen[0, :, 0].astype(np.float64), screen[0, :, 1].astype(np.float64)
    uv, T = np.stack([0.5 + 0.6 * x + 0.1 * y, 0.5 + 0.07 * y], 1).astype(np.float32), 256
    tex = TX._random_texture(T, 3)
    h = 1.35 / 256
    sv, t = screen.astype(np.float64), uv.astype(np.float64)
    fp = AR.footprint(sv[0][f[:, 0]], sv[0][f[:, 1]], sv[0][f[:, 2]], t[f[:, 0]], t[f[:, 1]], t[f[:, 2]], T, h, 16, 9)
    assert (fp["s1"] <= 1.0).all() and (fp["s1"] > 0.8).all() and (fp["s1"] / (np.abs(fp["rho"]) + 1e-300) == 1).all()
    for flt in (None, animate.pixel_filter("cycles", None, 4)):
        ani = _gpu(dev, screen, f, pos, 0.0, 0.0, 1.35, 64, 4, uv, tex, 16, pixel_filter=flt)
        bil = _gpu(dev, screen, f, pos, 0.0, 0.0, 1.35, 64, 4, uv, tex, filter="bilinear", pixel_filter=flt)
        assert (ani["face_id"] >= 0).sum() > 10000
        for k in WANT:
            assert np.array_equal(ani[k].view(np.uint8), bil[k].view(np.uint8)), k


def test_two_runs_and_a_side_stream_are_bit_identical(dev):
    screen, f, col, pos = GENERAL["torus"]
    image, covered, _ = TM._levels(64)
    args = (TX._t(dev, screen, np.float32), TX._t(dev, f, np.int64), None, TX._t(dev, pos, np.float32),
            0.0, 0.0, 5.4, SIZE, 2)
    kw = dict(want=WANT, uv=TX._t(dev, TX._general_uv(pos), np.float32), texture=TX._t(dev, image, np.uint8),
              filter="anisotropic", max_anisotropy=8)
    for flt in (None, animate.pixel_filter("eevee", None, 2)):
        a = ops.mesh_render_ortho(*args, pixel_filter=flt, **kw)
        b = ops.mesh_render_ortho(*args, pixel_filter=flt, **kw)
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            c = ops.mesh_render_ortho(*args, pixel_filter=flt, **kw)
        side.synchronize()
        for k in WANT:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


# ------------------------------------------------------------------ 5. the smallest sizes that can still go wrong
def _squashed_triangle(F):
    """One triangle that covers most of the window — its footprint crosses every tile border of a 32-pixel
    frame —, seen more and more edge-on from frame to frame (x scaled by 1, 1/3, 1/9)."""
    v = np.array([[-0.9, -0.8, 0.0], [0.95, -0.6, 0.1], [-0.2, 0.9, 0.2]])
    screen = np.stack([v * [3.0 ** -j, 1.0, 1.0] for j in range(F)]).astype(np.float32)
    uv = np.array([[0.1, 0.15], [0.9, 0.2], [0.35, 0.85]], np.float32)
    return screen, np.array([[0, 1, 2]]), uv, np.clip(v * 0.5 + 0.5, 0, 1).astype(np.float32)


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("S", [16, 32])
def test_one_tile_and_four_one_frame_and_three(dev, S, F):
    screen, f, uv, pos = _squashed_triangle(F)
    for T in (1, 37):
        image = TX._random_texture(T, 90 + T, 4)
        levels = MR.pyramid(image)
        for ss in (1, 2, 4):
            base = R.render(screen, f, np.zeros((3, 3), np.float32), pos, 0.0, 0.0, 2.0, S, ss)
            for cap in (2, 16):
                ref = AR.render(screen, f, uv, levels, pos, 0.0, 0.0, 2.0, S, ss, cap, base=base)
                got = _gpu(dev, screen, f, pos, 0.0, 0.0, 2.0, S, ss, uv, image, cap)
                seen = ref["face_id"] >= 0
                assert seen[0].sum() > 0.2 * seen[0].size
                if T > 1 and F == 3:                          # the last frame's ratio is about 10
                    assert ref["probes"][seen].max() == min(cap, 10)
                TX._compare_with_restatement(got, ref, S, ss, f"S={S} F={F} T={T} ss={ss} cap={cap}")


# ------------------------------------------------------------------ 6. ops and animate
def test_plan_keywords(dev):
    screen, f, col, pos = GENERAL["icosphere"]
    plan = ops.MeshRenderPlan(TX._t(dev, screen, np.float32), TX._t(dev, f, np.int64), 0.0, 0.0, 1.35, 32, 1).bin()
    p, uv = TX._t(dev, pos, np.float32), TX._t(dev, TX._general_uv(pos), np.float32)
    tex = TX._t(dev, TX._random_texture(16, 1), np.uint8)
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match="max_anisotropy"):
            plan.raster(None, p, uv=uv, texture=tex, filter="anisotropic", max_anisotropy=bad)
    with pytest.raises(ValueError, match="max_anisotropy"):
        plan.raster(None, p, uv=uv, texture=tex, filter="bilinear", max_anisotropy=4)
    with pytest.raises(ValueError, match="pyramid"):
        plan.raster(None, p, uv=uv, texture=tex, filter="anisotropic", pyramid=ops.mip_pyramid(tex[:8, :8].contiguous()))
    with pytest.raises(ValueError, match="needs both"):
        plan.raster(TX._t(dev, col, np.float32), p, filter="anisotropic")
    # the default cap is 8, and a pyramid built by the call is the one built beforehand with its gutter
    a = plan.raster(None, p, WANT, uv=uv, texture=tex, filter="anisotropic")
    b = plan.raster(None, p, WANT, uv=uv, texture=tex, filter="anisotropic", max_anisotropy=8,
                    pyramid=ops.mip_pyramid(tex, gutter=8))
    for k in WANT:
        assert torch.equal(a[k], b[k]), k


def test_render_frames_builds_the_gutter_the_probes_can_reach(dev):
    """mip_coverage "faces": level 0 dilated by max(2, cap) rounds with covered texels keeping their bytes,
    the levels above built from it with as many gutter rounds; "all": nothing is dilated."""
    v, f = R.quad(-0.25, -0.25, 0.25, 0.25, 0.0)
    uv = (0.25 + (v[:, :2] + 0.25)).astype(np.float32)        # the chart fills the middle quarter of the atlas
    T = 32
    image = TX._random_texture(T, 12)
    cov = (ops.uv_bake(TX._t(dev, uv, np.float32), TX._t(dev, f, np.int64), torch.zeros(4, 3, device=dev), T)[1] >= 0)
    cov = cov.cpu().numpy()
    assert 0.2 < cov.mean() < 0.3
    for cap, rounds in ((1, 2), (5, 5)):
        tex = animate.render._texture_args(image, uv, "anisotropic", 4, dev, f, "faces", cap)
        assert tex["max_anisotropy"] == cap and tex["filter"] == "anisotropic"
        img_d, cov_d = uv_ref.dilate(image, cov, rounds)
        assert np.array_equal(img_d[cov], image[cov]) and cov_d.sum() > cov.sum()
        rgba = np.concatenate([img_d, np.full((T, T, 1), 255, np.uint8)], -1)
        want = MR.pyramid(rgba, cov_d, rounds)
        assert np.array_equal(tex["pyramid"].buffer.cpu().numpy(), MR.flatten(want)), cap
        every = animate.render._texture_args(image, uv, "anisotropic", 4, dev, f, "all", cap)
        rgba0 = np.concatenate([image, np.full((T, T, 1), 255, np.uint8)], -1)
        assert np.array_equal(every["pyramid"].buffer.cpu().numpy(), MR.flatten(MR.pyramid(rgba0, None, rounds))), cap
    # through render_frames: the frame equals the call on that pyramid
    kw = dict(ss=1, device=dev, window=(0.0, 0.0, 32, 4.0), texture=image, uvs=uv, texture_filter="anisotropic")
    a = animate.render_frames(v, f, None, "rest_pose", max_anisotropy=5, **kw)
    b = _gpu(dev, v.astype(np.float32)[None], f, animate.position_colours(v), 0.0, 0.0, 4.0, 32, 1, uv,
             tex["texture"].cpu().numpy(), 5, pyramid=tex["pyramid"])
    assert np.array_equal(a["color"].cpu().numpy(), b["color_u8"]) and int((a["color"][..., 3] == 255).sum()) >= 9


# ------------------------------------------------------------------ 7. files and the skinned route
def test_run_render_with_the_anisotropic_filter(dev, tmp_path):
    from drawingspinup_amd.entry import run_render
    from drawingspinup_amd.nsr import mesh as M
    root, uid = str(tmp_path), "uid0"
    v, f = R.noisy_icosphere(2, 0.45, 0.3, 2)
    world = (v * [0.7, 1.2, 0.5] / 1.35 * 2.0).astype(np.float32)          # save_obj scales by ortho_scale / 2
    path = M.save_obj(os.path.join(root, uid, "mesh", "m.obj"), torch.from_numpy(world).to(dev),
                      torch.from_numpy(f).to(dev), torch.from_numpy(R.vertex_colours(len(v), 3)).to(dev),
                      export_uv=True, texture_size=1024)
    verts, faces, uvs, image = animate.read_obj_textured(path)
    common = ["--data_dir", root, "--uid", uid, "--ss", "1", "--texture", "atlas", "--device", str(dev),
              "--texture_filter", "anisotropic"]
    for action, extra, n, flags, kw in (
            ("rest_rotate", ["--test", "--frames", "2"], 2, ["--max_anisotropy", "4"], dict(max_anisotropy=4)),
            ("rest_pose", [], 1, ["--mip_coverage", "all", "--pixel_filter", "cycles"],
             dict(mip_coverage="all", pixel_filter="cycles"))):
        out_dir, rendered = run_render.run(common + extra + flags)
        assert out_dir == os.path.join(root, uid, "mesh", "blender_render", action)
        mem = animate.render_frames(verts, faces, None, action, ss=1, n_frames=2, device=dev, texture=image,
                                    uvs=uvs, texture_filter="anisotropic", **kw)
        assert 0.05 < float((mem["color"][..., 3] == 255).float().mean()) < 0.9
        for sub in ("color", "pos", "edge"):
            assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["%04d.png" % (i + 1) for i in range(n)]
            for i in range(n):
                png = np.array(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
                assert np.array_equal(png, mem[sub][i].cpu().numpy()), (action, sub, i)
        assert torch.equal(rendered["frames"], mem["frames"])
        # the filter shows against the trilinear frames, in the colour and nowhere else
        tri = animate.render_frames(verts, faces, None, action, ss=1, n_frames=2, device=dev, texture=image,
                                    uvs=uvs, texture_filter="trilinear", **{k: w for k, w in kw.items()
                                                                            if k != "max_anisotropy"})
        assert torch.equal(tri["pos"], mem["pos"]) and not torch.equal(tri["color"], mem["color"])
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
    out_dir, rendered = run_render.run(common + ["--test", "--max_anisotropy", "16", "--skinning", "dual_quaternion",
                                                 "--corrective_smooth", "2"])
    assert out_dir == os.path.join(mesh_dir, "blender_render", "wave")
    sk, clip = animate.fit_to_mesh(*animate.read_bvh(os.path.join(mesh_dir, "bvh_files", "wave.bvh")), verts)
    mem = animate.animate_mesh(verts, faces, None, sk, clip, weights=one, ss=1, device=dev, texture=image, uvs=uvs,
                               texture_filter="anisotropic", max_anisotropy=16, skinning="dual_quaternion",
                               corrective_iterations=2)
    assert not torch.equal(mem["color"][0], mem["color"][1])
    for sub in ("color", "pos", "edge"):
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["0001.png", "0002.png"]
        for i in range(2):
            png = np.array(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
            assert np.array_equal(png, mem[sub][i].cpu().numpy()), ("wave", sub, i)
            assert np.array_equal(png, rendered[sub][i].cpu().numpy())


def test_animate_mesh_rest_clip_with_the_anisotropic_filter_is_rest_pose(dev):
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
        tex = dict(texture=image, uvs=m["uvs"], texture_filter="anisotropic", max_anisotropy=4, mip_coverage=coverage)
        got = animate.animate_mesh(v, f, None, sk, animate.rest_clip(sk, 1), weights=one, ss=1, device=dev, **tex)
        window = (*got["centre"], got["size"], got["span"])
        ref = animate.render_frames(v, f, None, "rest_pose", ss=1, device=dev, window=window, **tex)
        for k in ("color", "pos", "edge", "frames"):
            assert torch.equal(got[k], ref[k]), (coverage, k)
        assert int((got["color"][..., 3] == 255).sum()) > 1000
