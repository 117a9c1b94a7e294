"""GPU: the orthographic frame renderer (csrc/mesh_render.hip) against the float64 restatement of
its rule (tests/frame_render_ref.py), its self-consistency at production size, the edge kernel,
the PNG hand-off to the stylisation entry points and the pipeline switch."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import frame_render_ref as R
from drawingspinup_amd import animate, ops

pytestmark = pytest.mark.gpu

WANT = ("color_u8", "pos_u8", "face_id", "depth", "frames", "pixels")


def _gpu(dev, screen, faces, colour, pos, cx, cy, span, S, ss, want=WANT):
    out = ops.mesh_render_ortho(torch.from_numpy(np.asarray(screen, np.float32)).to(dev),
                                torch.from_numpy(np.asarray(faces, np.int64)).to(dev),
                                torch.from_numpy(np.asarray(colour, np.float32)).to(dev),
                                torch.from_numpy(np.asarray(pos, np.float32)).to(dev), cx, cy, span, S, ss, want)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. lattice-aligned cases
def _dyadic_colours(n, seed):
    return np.random.default_rng(seed).integers(0, 9, (n, 3)).astype(np.float32) / 8.0


def _aligned_cases():
    red, blue = [[1.0, 0.0, 0.0]] * 4, [[0.0, 0.0, 1.0]] * 4
    cases = []
    v, f = R.quad(-0.25, -0.25, 0.25, 0.25, 0.0)
    cases += [("square", v, f, red, 8, ss) for ss in (1, 2, 4)]
    v, f = R.quad(-0.25, -0.25, 0.0625, 0.25, 0.0)
    cases.append(("half_column", v, f, blue, 8, 4))
    v0, f0 = R.quad(-0.25, -0.25, 0.25, 0.25, -0.5)
    v1, f1 = R.quad(-0.125, -0.125, 0.375, 0.375, 0.25, first=4)
    cases += [("stacked", np.concatenate([v0, v1]), np.concatenate([f0, f1]), red + blue, 8, ss) for ss in (1, 2, 4)]
    cases.append(("stacked_swapped", np.concatenate([v1, v0]), np.concatenate([f1 - 4, f0 + 4]), blue + red, 8, 2))
    v0, f0 = R.quad(-0.3125, -0.3125, 0.0625, 0.3125, 0.0)
    v1, f1 = R.quad(0.0625, -0.3125, 0.3125, 0.3125, 0.0, first=4)
    cases.append(("shared_edge", np.concatenate([v0, v1]), np.concatenate([f0, f1]), red + blue, 8, 1))
    # grid meshes with every vertex on a sample centre: S = 32 over span 1, vertices every 4 samples
    # (doubled areas are powers of two, every product and quotient is exact); depth folds over
    for ss in (1, 2, 4):
        N = 32 * ss
        x0 = (2 * 3 + 1) / (2.0 * N) - 0.5
        v, f = R.grid_mesh(5 * ss, x0, x0, 4.0 / N, z_of=lambda i, j: ((i * 3 + j * 5) % 7 - 3) / 8.0)
        cases.append((f"grid_ss{ss}", v, f, _dyadic_colours(len(v), ss), 32, ss))
    return cases


@pytest.mark.parametrize("case", _aligned_cases(), ids=lambda c: f"{c[0]}-ss{c[5]}")
def test_lattice_aligned_cases_equal_the_reference(dev, case):
    name, v, f, col, S, ss = case
    v = np.asarray(v, np.float64)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)            # dyadic: f32 holds them
    pos = np.clip(v * 0.5 + 0.5, 0, 1).astype(np.float32)                          # dyadic attributes
    screen = v.astype(np.float32)[None]
    ref = R.render(screen, f, col, pos, 0.0, 0.0, 1.0, S, ss)
    got = _gpu(dev, screen, f, col, pos, 0.0, 0.0, 1.0, S, ss)
    assert (ref["face_id"] >= 0).any()
    assert np.array_equal(got["face_id"], ref["face_id"])
    assert np.array_equal(got["depth"], ref["depth"])
    assert np.array_equal(got["color_u8"], ref["color_u8"])
    assert np.array_equal(got["pos_u8"], ref["pos_u8"])
    assert np.abs(got["pixels"].astype(np.float64) - ref["pixels"]).max() <= 2.0 ** -24     # its f32 rounding
    assert np.array_equal(got["frames"], R.frames_tensor(ref["color_u8"], ref["pos_u8"]))


def test_analytic_alpha_on_the_device(dev):
    v, f = R.quad(-0.25, -0.25, 0.0625, 0.25, 0.0)
    got = _gpu(dev, v.astype(np.float32)[None], f, [[0, 0, 1.0]] * 4, [[0.5, 0.5, 0.5]] * 4, 0, 0, 1.0, 8, 4)
    a = got["pixels"][0, :, :, 3]
    assert np.array_equal(a[2:6, 4], [0.5] * 4) and np.array_equal(a[2:6, 2:4], np.ones((4, 2)))
    assert a.sum() == 4 * 2 + 4 * 0.5
    assert got["color_u8"][0, 3, 4].tolist() == [0, 0, 255, 128]


# ------------------------------------------------------------------ 2. general position
GENERAL = R.general_cases()


@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(GENERAL))
def test_general_position_against_the_float64_reference(dev, name, ss):
    screen, f, col, pos = GENERAL[name]
    assert len(f) <= 5000 and screen.shape[0] == 3
    S, span = 128, 1.35
    ref = R.render(screen, f, col, pos, 0.0, 0.0, span, S, ss)
    covered = ref["face_id"] >= 0
    fragile = ref["fragile"]
    n_frag = int((fragile & covered).sum())
    print(f"{name} ss={ss}: covered {int(covered.sum())}, fragile {n_frag}")
    assert covered.sum() > 5000 and n_frag <= 1e-4 * covered.sum()               # on the reference alone
    got = _gpu(dev, screen, f, col, pos, 0.0, 0.0, span, S, ss)
    bad = got["face_id"] != ref["face_id"]
    print(f"  face_id mismatches {int(bad.sum())} (all of them fragile: {bool((~bad | fragile).all())})")
    assert not (bad & ~fragile).any()
    # pixels that hold a mismatching (fragile) sample are excused below, no others
    excused = bad.reshape(3, S, ss, S, ss).any((2, 4))
    err = np.abs(got["pixels"].astype(np.float64) - ref["pixels"])
    err[excused] = 0
    print(f"  max |pixel - reference| {err.max():.3e}")
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


# ------------------------------------------------------------------ 3. production size
@pytest.fixture(scope="module")
def production(dev):
    v, f = R.torus(200, 128, 0.38, 0.18)                      # 51 200 faces
    v = R.turn(v * (1.0 + 0.08 * np.sin(7.0 * v[:, :1] + 3.0 * v[:, 1:2])), 0.3, 0.9)
    col = R.vertex_colours(len(v), 7)
    pos = animate.position_colours(v).astype(np.float32)
    xyz = animate.rest_rotate(v, 24)
    cx, cy, size, span = animate.frame_window(xyz)
    assert size == 512
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(dev)
    return dict(screen=t(xyz, np.float32), faces=t(f, np.int64), col=t(col, np.float32), pos=t(pos, np.float32),
                cx=cx, cy=cy, span=span)


def test_production_size_is_self_consistent(dev, production):
    p = production
    args = (p["screen"], p["faces"], p["col"], p["pos"], p["cx"], p["cy"], p["span"])
    a = ops.mesh_render_ortho(*args, 512, 4, want=("color_u8", "pos_u8", "face_id", "frames"))
    assert len(p["faces"]) > 45000 and a["face_id"].shape == (24, 2048, 2048)
    assert 0.1 < float((a["face_id"] >= 0).float().mean()) < 0.9
    # the same lattice at S = 2048, ss = 1: the same winners
    b = ops.mesh_render_ortho(*args, 2048, 1, want=("face_id", "pixels"))
    assert torch.equal(a["face_id"], b["face_id"])
    # the box filter of that call's per-sample attributes, with torch, in the kernel's order
    for f in range(24):
        pix = b["pixels"][f].view(512, 4, 512, 4, 8)
        acc = torch.zeros(512, 512, 6, dtype=torch.float64, device=dev)
        cnt = torch.zeros(512, 512, dtype=torch.float64, device=dev)
        for sy in range(4):
            for sx in range(4):
                s = pix[:, sy, :, sx]
                cov = s[..., 3] == 1.0
                acc += torch.where(cov[..., None], s[..., [0, 1, 2, 4, 5, 6]].double(), 0.0)
                cnt += cov
        v = torch.where(cnt[..., None] > 0, acc / cnt.clamp(min=1)[..., None], 0.0)
        q = torch.floor(v * 255.0 + 0.5).to(torch.uint8)
        a8 = torch.floor(cnt / 16.0 * 255.0 + 0.5).to(torch.uint8)
        assert torch.equal(a["color_u8"][f], torch.cat([q[..., :3], a8[..., None]], -1)), f
        assert torch.equal(a["pos_u8"][f], torch.cat([q[..., 3:], a8[..., None]], -1)), f
    del b
    # two runs are bit-identical (the bin lists come out in a different order every time)
    c = ops.mesh_render_ortho(*args, 512, 4, want=("color_u8", "pos_u8", "face_id", "frames"))
    for k in a:
        assert torch.equal(a[k], c[k]), k
    # and so is a run beside a second stream doing other work
    side = torch.cuda.Stream(dev)
    x = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for _ in range(40):
            x = torch.tanh(x @ x * 1e-3)
    d = ops.mesh_render_ortho(*args, 512, 4, want=("color_u8", "pos_u8", "face_id", "frames"))
    torch.cuda.synchronize(dev)
    for k in a:
        assert torch.equal(a[k], d[k]), k


# ------------------------------------------------------------------ 4. edges
def _edges_equal(dev, pos_u8):
    got = ops.pos_edge_u8(torch.from_numpy(pos_u8).to(dev)).cpu().numpy()
    ref = np.stack([R.pos_edge(p) for p in pos_u8])
    assert np.array_equal(got, ref)
    return ref


def test_edge_kernel_equals_the_reference(dev):
    for name, (screen, f, col, pos) in GENERAL.items():
        pos_u8 = _gpu(dev, screen, f, col, pos, 0.0, 0.0, 1.35, 128, 4, want=("pos_u8",))["pos_u8"]
        e = _edges_equal(dev, pos_u8)
        assert 0.005 < (e == 0).mean() < 0.5, name            # silhouettes and folds, not everything
        # a one-pixel hole inside the character
        holed = pos_u8.copy()
        yy, xx = np.argwhere(holed[0, :, :, 3] == 255)[len(np.argwhere(holed[0, :, :, 3] == 255)) // 2]
        holed[0, yy, xx, 3] = 0
        eh = _edges_equal(dev, holed)
        assert (eh[0, yy - 1:yy + 2, xx - 1:xx + 2] == 0).sum() >= 8
        # the character touching the border: the window moved off-centre cuts it
        cut = _gpu(dev, screen, f, col, pos, 0.45, -0.5, 1.35, 128, 2, want=("pos_u8",))["pos_u8"]
        assert (cut[:, 0, :, 3] == 255).any() or (cut[:, -1, :, 3] == 255).any() or (cut[:, :, 0, 3] == 255).any()
        _edges_equal(dev, cut)
    # a non-square map and full-frame coverage (reflect-101 on every side)
    g = np.random.default_rng(3)
    _edges_equal(dev, g.integers(0, 256, (2, 20, 36, 4)).astype(np.uint8))
    full = g.integers(0, 256, (1, 16, 16, 4)).astype(np.uint8)
    full[..., 3] = 255
    _edges_equal(dev, full)


# ------------------------------------------------------------------ 5. hand-off through PNG files
def test_run_render_hands_over_to_the_stylisation_entry_point(dev, tmp_path):
    from drawingspinup_amd.entry import _test_stage, data as D, run_render
    from drawingspinup_amd.nsr.mesh import write_obj
    root, uid = str(tmp_path), "uid0"
    v, f = R.noisy_icosphere(3, 0.45, 0.3, 2)
    v = v * [0.7, 1.2, 0.5]
    write_obj(os.path.join(root, uid, "mesh", "it3000-mc512-f50000_c_r_s_cbp.obj"), v, f, R.vertex_colours(len(v), 3))
    out_dir, rendered = run_render.run(["--data_dir", root, "--uid", uid, "--test", "--frames", "3", "--ss", "2"])
    assert out_dir == os.path.join(root, uid, "mesh", "blender_render", "rest_rotate")
    size = rendered["size"]
    for sub, mode in (("color", "RGBA"), ("pos", "RGBA"), ("edge", "L")):
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == ["0001.png", "0002.png", "0003.png"]
        im = Image.open(os.path.join(out_dir, sub, "0001.png"))
        assert im.mode == mode and im.size == (size, size)
    ds = D.DatasetFullImages(out_dir, "color", True, True, True)
    assert len(ds) == 3
    frames, edge = rendered["frames"].cpu(), rendered["edge"].cpu()
    for i in range(3):
        b = ds[i]
        assert np.array_equal(np.array(Image.open(os.path.join(out_dir, "edge", b["file_name"]))), edge[i].numpy())
        want = frames[i].clone()
        want[0:3, edge[i] < 255] = -1.0                       # overlap_edge_on_img: black, then normalised
        assert torch.equal(b["pre"], want)
        assert torch.equal(b["pre_mask"], frames[i, 3:4])
    assert 0.05 < float(frames[:, 3].mean()) < 0.9 and (edge < 255).any()
    # rest_pose: one frame, the default window
    out_dir0, r0 = run_render.run(["--data_dir", root, "--uid", uid, "--ss", "1"])
    assert sorted(os.listdir(os.path.join(out_dir0, "color"))) == ["0001.png"] and r0["size"] == 512
    assert r0["span"] == 1.35
    os.rename(out_dir0, os.path.join(root, "rest_pose_aside"))          # keep stage 1 to the three frames
    _test_stage.run(1, ["--uid", uid, "--root_dir", root, "--random_init"])
    res = os.path.join(out_dir, "res_stage1_mask_pos")
    assert sorted(os.listdir(res)) == ["0001.png", "0002.png", "0003.png"]
    s1 = Image.open(os.path.join(res, "0002.png"))
    assert s1.mode == "RGBA" and s1.size == (size, size)
    assert np.array_equal(np.array(s1)[..., 3], rendered["color"][1, :, :, 3].cpu().numpy())


# ------------------------------------------------------------------ 6. the pipeline switch
def _stand_in_views(drawing, seed):
    """Six 256^2 'predicted' views made from the drawing itself (the diffusion stage is not what this
    test is about): colours = the drawing on white (mirrored for the back), normals = a dome."""
    import torch.nn.functional as F
    small = F.interpolate(drawing[None], size=(256, 256), mode="bilinear", align_corners=False)[0]
    rgb = small[:3] * small[3:4] + (1 - small[3:4])
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 256, device=drawing.device),
                            torch.linspace(-1, 1, 256, device=drawing.device), indexing="ij")
    nz = (1 - (xx ** 2 + yy ** 2).clamp(max=0.99)).sqrt()
    nrm = torch.stack([xx, -yy, nz]) * 0.5 + 0.5
    colors = torch.stack([rgb, rgb, rgb, rgb.flip(2), rgb, rgb])
    return nrm[None].expand(6, -1, -1, -1).contiguous(), colors


def test_pipeline_renders_the_reconstructed_mesh(dev):
    from drawingspinup_amd.drawing import DrawingPipeline, synthetic_edges, synthetic_frames
    pipe = DrawingPipeline(dev, seed=0, nsr_steps=40, n_frames=4, export_resolution=128, with_mv=False,
                           with_contour=False, frames="rendered")
    pipe.multiview = _stand_in_views
    outs = [pipe.run(seed) for seed in (1, 2)]
    for o in outs:
        assert o["frame_source"] == "rendered"
        n, _, S, _ = o["rendered"].shape
        assert n == 4 and o["frames"].shape == (4, 4, S, S) and o["frames"].dtype == torch.uint8
        # alpha of the stylised frames = the rendered coverage
        assert torch.equal(o["frames"][:, 3], (o["rendered"][:, 3] * 255).to(torch.uint8))
        assert 0.02 < float(o["rendered"][:, 3].mean()) < 0.9
    assert not torch.equal(outs[0]["rendered"], outs[1]["rendered"])
    assert not torch.equal(outs[0]["frames"][:, :3], outs[1]["frames"][:, :3])
    # the default is what it was: synthetic frames, the same three keys, the same values
    pipe.frames = "synthetic"
    o = pipe.run(1)
    assert sorted(o) == ["frames", "inside_voxels", "views"]
    fr = synthetic_frames(1, 4, device=dev)
    assert torch.equal(o["frames"], pipe.stylize(fr, synthetic_edges(fr)))
    assert DrawingPipeline.__init__.__defaults__[-1] == "synthetic"
