"""GPU: textured frames — the UV atlas sampled inside the resolve of the frame rasteriser
(csrc/mesh_render.hip, dsu_mesh_render_ortho with a tex) against known answers and the float64
restatement of its rule (tests/frame_render_tex_ref.py), its self-consistency at production size
and the way through animate and run_render."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import frame_render_ref as R
import frame_render_tex_ref as TR
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu

WANT = ("color_u8", "pos_u8", "face_id", "depth", "frames", "pixels")
FILTERS = (TR.NEAREST, TR.BILINEAR)


def _t(dev, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _gpu(dev, screen, faces, colour, pos, cx, cy, span, S, ss, want=WANT, uv=None, texture=None, filter="bilinear"):
    kw = {} if texture is None else dict(uv=_t(dev, uv, np.float32), texture=_t(dev, texture, np.uint8), filter=filter)
    out = ops.mesh_render_ortho(_t(dev, screen, np.float32), _t(dev, faces, np.int64),
                                None if colour is None else _t(dev, colour, np.float32), _t(dev, pos, np.float32),
                                cx, cy, span, S, ss, want, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _random_texture(T, seed, channels=3):
    return np.random.default_rng(seed).integers(0, 256, (T, T, channels)).astype(np.uint8)


# ------------------------------------------------------------------ 1. identity mapping
def _identity_quad(T):
    """The quad over [-0.5, 0.5]^2 whose uvs put sample (R, C) of a T-sample lattice over span 1 on the
    centre of texel uv T = (C, T - 1 - R): image row R, column C."""
    v, f = R.quad(-0.5, -0.5, 0.5, 0.5, 0.0)
    uv = v[:, :2] + 0.5 - 1.0 / (2 * T)
    assert np.array_equal(uv.astype(np.float32).astype(np.float64), uv)          # dyadic
    return v, f, uv.astype(np.float32), np.clip(v * 0.5 + 0.5, 0, 1).astype(np.float32)


@pytest.mark.parametrize("flt", FILTERS)
def test_identity_mapping_returns_the_texture(dev, flt):
    v, f, uv, pos = _identity_quad(8)
    tex = _random_texture(8, 1)
    got = _gpu(dev, v.astype(np.float32)[None], f, None, pos, 0.0, 0.0, 1.0, 8, 1, uv=uv, texture=tex, filter=flt)
    assert np.array_equal(got["color_u8"][0, :, :, :3], tex)
    assert (got["color_u8"][0, :, :, 3] == 255).all()
    # a four-channel texture: the fourth byte is not read
    rgba = np.concatenate([tex, _random_texture(8, 2, 1)], -1)
    again = _gpu(dev, v.astype(np.float32)[None], f, None, pos, 0.0, 0.0, 1.0, 8, 1, uv=uv, texture=rgba, filter=flt)
    for k in WANT:
        assert np.array_equal(again[k], got[k]), k


@pytest.mark.parametrize("flt", FILTERS)
@pytest.mark.parametrize("ss", [2, 4])
def test_identity_mapping_box_mean(dev, ss, flt):
    T = 8 * ss
    v, f, uv, pos = _identity_quad(T)
    tex = _random_texture(T, 10 + ss)
    got = _gpu(dev, v.astype(np.float32)[None], f, None, pos, 0.0, 0.0, 1.0, 8, ss, uv=uv, texture=tex, filter=flt)
    mean = tex.astype(np.float64).reshape(8, ss, 8, ss, 3).sum((1, 3)) / float(ss * ss)    # exact: levels
    want = np.floor(mean + 0.5)
    d = np.abs(got["color_u8"][0, :, :, :3].astype(np.float64) - want)
    to_boundary = np.abs(mean + 0.5 - np.round(mean + 0.5)) / 255.0
    print(f"ss={ss} {flt}: {int((d > 0).sum())} of {d.size} values off by one level")
    assert d.max() <= 1 and (to_boundary[d > 0] <= 1e-4).all()
    assert (got["color_u8"][0, :, :, 3] == 255).all()
    # before quantisation: the mean of the f32 texel values
    px = got["pixels"][0, :, :, :3].astype(np.float64)
    assert np.abs(px - mean / 255.0).max() <= 2.0 ** -23


def _grid_cases():
    cases = []
    for ss in (1, 2, 4):
        N = 32 * ss
        x0 = (2 * 3 + 1) / (2.0 * N) - 0.5
        v, f = R.grid_mesh(5 * ss, x0, x0, 4.0 / N, z_of=lambda i, j: ((i * 3 + j * 5) % 7 - 3) / 8.0)
        uv = v[:, :2] + 0.5 - 1.0 / (2 * N)              # affine in (x, y): sample (R, C) -> uv N = (C, N - 1 - R)
        for T in (N, N // 2):                            # on texel centres; on centres and half-way points
            for flt in FILTERS:
                cases.append((f"grid_ss{ss}-T{T}-{flt}", v, f, uv, T, ss, flt))
    return cases


@pytest.mark.parametrize("case", _grid_cases(), ids=lambda c: c[0])
def test_lattice_aligned_grid_equals_the_restatement(dev, case):
    name, v, f, uv, T, ss, flt = case
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert np.array_equal(uv.astype(np.float32).astype(np.float64), uv)
    pos = np.clip(v * 0.5 + 0.5, 0, 1).astype(np.float32)
    screen = v.astype(np.float32)[None]
    tex = _random_texture(T, T + ss)
    ref = TR.render(screen, f, uv, tex, pos, 0.0, 0.0, 1.0, 32, ss, flt)
    assert (ref["face_id"] >= 0).any()
    assert T != 32 * ss or not ref["tex_fragile"].any()      # texel centres; at T = N / 2 everything is dyadic instead
    got = _gpu(dev, screen, f, None, pos, 0.0, 0.0, 1.0, 32, ss, uv=uv, texture=tex, filter=flt)
    assert np.array_equal(got["face_id"], ref["face_id"])
    assert np.array_equal(got["depth"], ref["depth"])
    assert np.array_equal(got["color_u8"], ref["color_u8"])
    assert np.array_equal(got["pos_u8"], ref["pos_u8"])
    assert np.abs(got["pixels"].astype(np.float64) - ref["pixels"]).max() <= 2.0 ** -24
    assert np.array_equal(got["frames"], R.frames_tensor(ref["color_u8"], ref["pos_u8"]))


# ------------------------------------------------------------------ 2. texture independence
GENERAL = R.general_cases()


def _general_uv(pos):
    return (0.05 + 0.9 * pos[:, :2].astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("flt", FILTERS)
def test_the_texture_enters_through_the_colour_channels_only(dev, flt):
    screen, f, col, pos = GENERAL["two_blobs"]
    uv = _general_uv(pos)
    args = (screen, f, col, pos, 0.0, 0.0, 1.35, 128, 2)
    plain = _gpu(dev, *args)
    for tex in (_random_texture(37, 5), _random_texture(64, 6, 4)):
        got = _gpu(dev, *args, uv=uv, texture=tex, filter=flt)
        for k in ("pos_u8", "face_id", "depth"):
            assert np.array_equal(got[k], plain[k]), k
        assert np.array_equal(got["color_u8"][..., 3], plain["color_u8"][..., 3])
        assert np.array_equal(got["frames"][:, 3:], plain["frames"][:, 3:])
        assert np.array_equal(got["pixels"][..., 3:], plain["pixels"][..., 3:])
        assert not np.array_equal(got["color_u8"], plain["color_u8"])
    # one constant colour k: the untextured render with vertex colours k / 255
    k = np.array([201, 7, 98], np.uint8)
    const = np.broadcast_to(k, (16, 16, 3))
    flat = _gpu(dev, screen, f, np.broadcast_to(k.astype(np.float32) / np.float32(255.0), col.shape), pos,
                0.0, 0.0, 1.35, 128, 2)
    got = _gpu(dev, *args, uv=uv, texture=const, filter=flt)
    assert np.array_equal(got["color_u8"], flat["color_u8"])
    assert np.array_equal(got["frames"], flat["frames"])


# ------------------------------------------------------------------ 3. general position
@functools.lru_cache(maxsize=None)
def _general_base(name, ss):
    screen, f, col, pos = GENERAL[name]
    return R.render(screen, f, col, pos, 0.0, 0.0, 1.35, 128, ss)


def _compare_with_restatement(got, ref, S, ss, label):
    """The bars of the general-position test: face ids equal outside geometrically fragile samples;
    outside pixels that hold a fragile sample of either kind the colour equals the restatement to
    1e-5 in `pixels` and to one level in uint8, and differs only within 1e-4 of a rounding boundary."""
    F = ref["face_id"].shape[0]
    fragile = ref["fragile"]
    bad = got["face_id"] != ref["face_id"]
    assert not (bad & ~fragile).any(), label
    excused = (bad | fragile | ref["tex_fragile"]).reshape(F, S, ss, S, ss).any((2, 4))
    err = np.abs(got["pixels"].astype(np.float64) - ref["pixels"])
    err[excused] = 0
    d = np.abs(got["color_u8"].astype(np.int16) - ref["color_u8"].astype(np.int16))
    d[excused] = 0
    v255 = ref["pixels"][..., :4] * 255.0 + 0.5
    to_boundary = np.abs(v255 - np.round(v255)) / 255.0
    print(f"  {label}: excused pixels {int(excused.sum())}, max |pixel - restatement| {err.max():.3e}, "
          f"{int((d > 0).sum())} values off by one level (max {int(d.max())})")
    assert err.max() <= 1e-5, label
    assert d.max() <= 1 and (to_boundary[d > 0] <= 1e-4).all(), label
    assert np.array_equal(got["frames"], R.frames_tensor(got["color_u8"], got["pos_u8"])), label
    return excused


@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(GENERAL))
def test_general_position_against_the_float64_restatement(dev, name, ss):
    screen, f, col, pos = GENERAL[name]
    uv = _general_uv(pos)
    S, span = 128, 1.35
    base = _general_base(name, ss)
    covered = base["face_id"] >= 0
    refs = {}
    for T in (64, 37):                                       # 37: no power of two anywhere
        tex = _random_texture(T, 20 + T)
        for flt in FILTERS:
            ref = TR.render(screen, f, uv, tex, pos, 0.0, 0.0, span, S, ss, flt, base=base)
            n_geo, n_tex = int((ref["fragile"] & covered).sum()), int(ref["tex_fragile"].sum())
            print(f"{name} ss={ss} T={T} {flt}: covered {int(covered.sum())}, fragile {n_geo} geometric, {n_tex} texture")
            assert flt == TR.NEAREST or n_tex == 0
            assert covered.sum() > 5000 and n_geo + n_tex <= 1e-4 * covered.sum()     # on the restatement alone
            refs[T, flt] = (tex, ref)
    for (T, flt), (tex, ref) in refs.items():
        got = _gpu(dev, screen, f, None, pos, 0.0, 0.0, span, S, ss, uv=uv, texture=tex, filter=flt)
        _compare_with_restatement(got, ref, S, ss, f"T={T} {flt}")
        ok = got["face_id"] == ref["face_id"]
        assert np.array_equal(got["depth"][ok], ref["depth"][ok])


@pytest.mark.parametrize("flt", FILTERS)
def test_a_nan_uv_reads_texel_coordinate_zero(dev, flt):
    screen, f, col, pos = GENERAL["icosphere"]
    S, span, ss = 128, 1.35, 2
    base = _general_base("icosphere", ss)
    # a vertex of a face that is seen in the first frame
    vertex = int(f[base["face_id"][0][base["face_id"][0] >= 0][len(f) // 3]][0])
    uv = _general_uv(pos)
    uv[vertex] = np.nan
    tex = _random_texture(37, 9)
    ref = TR.render(screen, f, uv, tex, pos, 0.0, 0.0, span, S, ss, flt, base=base)
    got = _gpu(dev, screen, f, None, pos, 0.0, 0.0, span, S, ss, uv=uv, texture=tex, filter=flt)
    clean = _gpu(dev, screen, f, None, pos, 0.0, 0.0, span, S, ss, uv=_general_uv(pos), texture=tex, filter=flt)
    for k in ("face_id", "depth", "pos_u8"):
        assert np.array_equal(got[k], clean[k]), k           # its faces stay covered
    assert np.array_equal(got["color_u8"][..., 3], clean["color_u8"][..., 3])
    assert np.isfinite(got["pixels"]).all() and np.isfinite(got["frames"]).all()
    _compare_with_restatement(got, ref, S, ss, f"nan uv {flt}")
    # the faces around that vertex show the texel of uv T = (0, 0): the image's bottom-left corner
    touched = np.isin(got["face_id"], np.nonzero((f == vertex).any(1))[0])
    assert touched.any()
    inside = touched.reshape(3, S, ss, S, ss).all((2, 4))
    assert inside.any() and (got["color_u8"][inside][:, :3] == tex[36, 0]).all()


# ------------------------------------------------------------------ 4. production size
@pytest.fixture(scope="module")
def production(dev):
    from drawingspinup_amd.nsr import uv as U
    v, f = R.torus(200, 128, 0.38, 0.18)                      # 51 200 faces
    v = R.turn(v * (1.0 + 0.08 * np.sin(7.0 * v[:, :1] + 3.0 * v[:, 1:2])), 0.3, 0.9)
    m = U.uv_mapping(v, f, R.vertex_colours(len(v), 7), "torus", size=1024, device=dev)
    v, f = m["verts"], m["faces"]
    pos = animate.position_colours(v).astype(np.float32)
    xyz = animate.rest_rotate(v, 24)
    cx, cy, size, span = animate.frame_window(xyz)
    assert size == 512 and len(f) == 51200 and m["image"].shape == (1024, 1024, 3)
    # a high-frequency texture: the bake with every other texel inverted
    yy, xx = np.mgrid[:1024, :1024]
    image = np.where(((yy + xx) % 2 == 0)[..., None], m["image"], 255 - m["image"]).astype(np.uint8)
    col = animate.render.sample_texture(image, m["uvs"])     # what read_obj makes of the same file
    return dict(screen=_t(dev, xyz, np.float32), faces=_t(dev, f, np.int64), col=_t(dev, col, np.float32),
                pos=_t(dev, pos, np.float32), uv=_t(dev, m["uvs"], np.float32),
                texture=ops.texture_rgba(_t(dev, image, np.uint8)), cx=cx, cy=cy, span=span)


@pytest.mark.parametrize("flt", FILTERS)
def test_production_size_is_self_consistent(dev, production, flt):
    p = production
    args = (p["screen"], p["faces"], None, p["pos"], p["cx"], p["cy"], p["span"])
    tex = dict(uv=p["uv"], texture=p["texture"], filter=flt)
    want = ("color_u8", "pos_u8", "face_id", "frames")
    a = ops.mesh_render_ortho(*args, 512, 4, want=want, **tex)
    assert a["face_id"].shape == (24, 2048, 2048) and 0.1 < float((a["face_id"] >= 0).float().mean()) < 0.9
    # the same lattice at S = 2048, ss = 1, then the box filter with torch, in the kernel's order
    b = ops.mesh_render_ortho(*args, 2048, 1, want=("face_id", "pixels"), **tex)
    assert torch.equal(a["face_id"], b["face_id"])
    for f in range(24):
        pix = b["pixels"][f].view(512, 4, 512, 4, 8)
        acc = torch.zeros(512, 512, 3, dtype=torch.float64, device=dev)
        cnt = torch.zeros(512, 512, dtype=torch.float64, device=dev)
        for sy in range(4):
            for sx in range(4):
                s = pix[:, sy, :, sx]
                cov = s[..., 3] == 1.0
                acc += torch.where(cov[..., None], s[..., :3].double(), 0.0)
                cnt += cov
        v = torch.where(cnt[..., None] > 0, acc / cnt.clamp(min=1)[..., None], 0.0)
        q = torch.floor(v * 255.0 + 0.5).to(torch.uint8)
        a8 = torch.floor(cnt / 16.0 * 255.0 + 0.5).to(torch.uint8)
        assert torch.equal(a["color_u8"][f], torch.cat([q, a8[..., None]], -1)), f
    del b, pix
    # two runs are bit-identical
    c = ops.mesh_render_ortho(*args, 512, 4, want=want, **tex)
    for k in a:
        assert torch.equal(a[k], c[k]), k
    # a run on a side stream
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        d = ops.mesh_render_ortho(*args, 512, 4, want=want, **tex)
    side.synchronize()
    for k in a:
        assert torch.equal(a[k], d[k]), k
    # and a run beside a second stream doing other work
    x = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for _ in range(40):
            x = torch.tanh(x @ x * 1e-3)
    e = ops.mesh_render_ortho(*args, 512, 4, want=want, **tex)
    torch.cuda.synchronize(dev)
    for k in a:
        assert torch.equal(a[k], e[k]), k
    # the texture shows: the vertex-sampled render of the same mesh has the same geometry and
    # other colours
    plain = ops.mesh_render_ortho(p["screen"], p["faces"], p["col"], p["pos"], p["cx"], p["cy"], p["span"], 512, 4,
                                  want=("color_u8", "pos_u8"))
    assert torch.equal(plain["pos_u8"], a["pos_u8"])
    assert torch.equal(ops.pos_edge_u8(plain["pos_u8"]), ops.pos_edge_u8(a["pos_u8"]))
    assert torch.equal(plain["color_u8"][..., 3], a["color_u8"][..., 3])
    seen = a["color_u8"][..., 3] == 255
    differ = (plain["color_u8"][..., :3] != a["color_u8"][..., :3]).any(-1) & seen
    print(f"{flt}: {int(differ.sum())} of {int(seen.sum())} fully covered pixels differ from the vertex-sampled render")
    assert differ.sum() > 0.5 * seen.sum()


# ------------------------------------------------------------------ 5. files
def test_run_render_with_the_atlas(dev, tmp_path):
    from drawingspinup_amd.entry import run_render
    from drawingspinup_amd.nsr import mesh as M
    root, uid = str(tmp_path), "uid0"
    v, f = R.noisy_icosphere(3, 0.45, 0.3, 2)
    world = (v * [0.7, 1.2, 0.5] / 1.35 * 2.0).astype(np.float32)          # save_obj scales by ortho_scale / 2: it fits the frame
    path = M.save_obj(os.path.join(root, uid, "mesh", "m.obj"), torch.from_numpy(world).to(dev),
                      torch.from_numpy(f).to(dev), torch.from_numpy(R.vertex_colours(len(v), 3)).to(dev),
                      export_uv=True, texture_size=128)
    verts, faces, uvs, image = animate.read_obj_textured(path)
    assert image.shape == (128, 128, 3) and len(uvs) == len(verts) >= len(v) and len(faces) == len(f)
    for flt in FILTERS:
        out_dir, rendered = run_render.run(["--data_dir", root, "--uid", uid, "--test", "--frames", "3", "--ss", "2",
                                            "--texture", "atlas", "--texture_filter", flt, "--device", str(dev)])
        assert out_dir == os.path.join(root, uid, "mesh", "blender_render", "rest_rotate")
        mem = animate.render_frames(verts, faces, None, "rest_rotate", ss=2, n_frames=3, device=dev, texture=image,
                                    uvs=uvs, texture_filter=flt)
        assert 0.05 < float((mem["color"][..., 3] == 255).float().mean()) < 0.9
        for sub in ("color", "pos", "edge"):
            assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["0001.png", "0002.png", "0003.png"]
            for i in range(3):
                png = np.array(Image.open(os.path.join(out_dir, sub, "%04d.png" % (i + 1))))
                assert np.array_equal(png, mem[sub][i].cpu().numpy()), (flt, sub, i)
        assert torch.equal(rendered["frames"], mem["frames"])
    atlas = {sub: [open(os.path.join(out_dir, sub, n), "rb").read() for n in sorted(os.listdir(os.path.join(out_dir, sub)))]
             for sub in ("color", "pos", "edge")}
    # --texture vertex is the call without the flag: the bytes it wrote before
    common = ["--data_dir", root, "--uid", uid, "--test", "--frames", "3", "--ss", "2", "--device", str(dev)]
    run_render.run(common + ["--texture", "vertex"])
    flagged = {sub: [open(os.path.join(out_dir, sub, n), "rb").read() for n in sorted(os.listdir(os.path.join(out_dir, sub)))]
               for sub in ("color", "pos", "edge")}
    run_render.run(common)
    for sub in ("color", "pos", "edge"):
        now = [open(os.path.join(out_dir, sub, n), "rb").read() for n in sorted(os.listdir(os.path.join(out_dir, sub)))]
        assert now == flagged[sub], sub
    assert flagged["pos"] == atlas["pos"] and flagged["edge"] == atlas["edge"] and flagged["color"] != atlas["color"]


def test_animate_mesh_rest_clip_with_a_texture_is_rest_pose(dev):
    import skin_ref as SK
    from drawingspinup_amd.nsr import uv as U
    v, f = SK.capsule_character()
    names, parents, off, ends = SK.humanoid()
    sk = animate.Skeleton(names, parents, off, ends)
    m = U.uv_mapping(v, f, SK.vertex_colours(len(v), 8), "c", size=128, device=dev)
    v, f = m["verts"].astype(np.float32), m["faces"]
    image = _random_texture(128, 4)
    # one influence of weight 1: the skinned rest mesh is the rest mesh, bit for bit
    one = (np.zeros((len(v), 1), np.int32), np.ones((len(v), 1), np.float32))
    for flt in FILTERS:
        tex = dict(texture=image, uvs=m["uvs"], texture_filter=flt)
        got = animate.animate_mesh(v, f, None, sk, animate.rest_clip(sk, 1), weights=one, device=dev, **tex)
        assert np.array_equal(got["vertices"][0].cpu().numpy(), v)
        window = (*got["centre"], got["size"], got["span"])
        ref = animate.render_frames(v, f, None, "rest_pose", device=dev, window=window, **tex)
        for k in ("color", "pos", "edge", "frames"):
            assert torch.equal(got[k], ref[k]), (flt, k)
        assert int((got["color"][..., 3] == 255).sum()) > 1000
        plain = animate.render_frames(v, f, np.zeros((len(v), 3), np.float32), "rest_pose", device=dev, window=window)
        assert torch.equal(plain["pos"], got["pos"]) and not torch.equal(plain["color"], got["color"])
