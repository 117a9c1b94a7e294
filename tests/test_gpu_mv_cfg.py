"""Classifier-free guidance in the multi-view pipeline on the GPU: the two HIP kernels around the
UNet call (csrc/mv_guidance.hip) against their rules, the guided pipeline against the REFERENCE's
own guided pipeline (tests/golden/mv_cfg_reference.npz, make_mv_cfg_golden.py), and the properties
the guided branch must keep: affine in guidance_scale after one step, the guidance_scale == 1 output
untouched by guided calls on the same object (eager and captured), full width from the YAML key
and DrawingPipeline down."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_cfg_ref as R  # noqa: E402
from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.mv.pipeline import DDIMScheduler, MVDiffusionImagePipeline  # noqa: E402
from drawingspinup_amd.mv.unet import UNetMV2DConditionModel  # noqa: E402
from oracle import mv_weights  # noqa: E402
from oracle.mv_pipeline_aux import (LinearClip, LinearVAE, aux_state, camera_embeddings,  # noqa: E402
                                    det_noise, input_image)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _f16(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half()


# ------------------------------------------------------------------------------------ kernels
# (B, C, h, w).  The issue's three (C = 4: odd h*w -> 8-byte vectors, 16-byte vectors over several
# blocks, one 4-element row) and a row of 9 elements, which only the single-element path can take.
@pytest.mark.parametrize("shape", [(6, 4, 5, 7), (12, 4, 32, 32), (1, 4, 1, 1), (3, 1, 3, 3)])
def test_cfg_model_input_is_the_torch_cat(dev, shape):
    lat, img = _f16(shape, 1).to(dev), _f16(shape, 2).to(dev)
    want = torch.cat([torch.cat([lat] * 2), torch.cat([torch.zeros_like(img), img])], dim=1)
    got = ops.cfg_model_input(lat, img)
    assert got.shape == want.shape and got.dtype == torch.float16
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_cfg_model_input_on_pointers_aligned_to_8_bytes_only(dev):
    """A row of 4096 elements would take 16-byte vectors; inputs that start 8 bytes into an
    allocation must not."""
    shape, n = (2, 4, 32, 32), 2 * 4 * 32 * 32
    lat = _f16(n + 4, 3).to(dev)[4:].view(shape)
    img = _f16(n + 4, 4).to(dev)[4:].view(shape)
    assert lat.data_ptr() % 16 == 8 and lat.is_contiguous()
    want = torch.cat([torch.cat([lat] * 2), torch.cat([torch.zeros_like(img), img])], dim=1)
    assert torch.equal(ops.cfg_model_input(lat, img).view(torch.int16), want.view(torch.int16))


def _step_scalars(which, eta):
    s = DDIMScheduler()
    s.set_timesteps(75)
    return s.step_scalars(s.timesteps_host[{"mid": 37, "last": -1}[which]], eta)


@pytest.mark.parametrize("case", ["mid-noise", "mid-std0", "last-noise"])
@pytest.mark.parametrize("g", [1.0, 3.0, 0.0])
@pytest.mark.parametrize("shape", [(6, 4, 5, 7), (12, 4, 32, 32), (3, 1, 3, 3)])
def test_ddim_cfg_step_within_one_f16_spacing_of_the_rule(dev, shape, g, case):
    """Every output element within one f16 spacing (at the float64 value) of the rule of
    include/dsu_hip.h evaluated in float64 from the same f16 inputs and f32 scalars, so only the
    final rounding can differ.  (That needs the kernel's arithmetic in double: where the two terms
    of `prev` cancel, f32 roundings of them reach 2.7 spacings of the small result on these very
    inputs.)  `last`: the 75-step schedule's last timestep, a_prev = alphas_cumprod[0]; `std0`:
    eta = 0, no noise.  Two calls give the same bits."""
    which, noise = case.split("-")
    sc = _step_scalars(which, 1.0 if noise == "noise" else 0.0)
    assert (sc[3] > 0) == (noise == "noise")
    B = shape[0]
    pred, lat = _f16((2 * B,) + shape[1:], 5), _f16(shape, 6)
    vn = _f16(shape, 7) if noise == "noise" else None
    got = ops.ddim_cfg_step(pred.to(dev), lat.to(dev), None if vn is None else vn.to(dev), g, *sc)
    again = ops.ddim_cfg_step(pred.to(dev), lat.to(dev), None if vn is None else vn.to(dev), g, *sc)
    assert got.shape == shape and got.dtype == torch.float16
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))
    want = R.cfg_step_rule(pred.numpy(), lat.numpy(), None if vn is None else vn.numpy(), g, *sc)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want) / R.f16_spacing(want)
    print(f"ddim_cfg_step {shape} g={g} {case}: max error {err.max():.3f} f16 spacings")
    assert err.max() <= 1.0


def test_ddim_cfg_step_refuses_what_it_cannot_compute(dev):
    from drawingspinup_amd._lib import DsuError
    pred, lat = _f16((2, 4, 2, 2), 8).to(dev), _f16((1, 4, 2, 2), 9).to(dev)
    with pytest.raises(DsuError):
        ops.ddim_cfg_step(pred, lat, None, 3.0, 0.0, 1.0, 0.9, 0.0)          # sqrt(a_t) = 0
    with pytest.raises(DsuError):
        ops.ddim_cfg_step(pred, lat, None, 3.0, 0.5, 0.8, 0.9, 0.9)          # 1 - a_prev - std^2 < 0


# ------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def small(dev):
    """The reduced-width pipeline of test_pipeline_vs_reference_pipeline_fixture (the reference
    fixtures' UNet config and name-derived parameters, linear stand-ins for CLIP and the VAE) and
    the injected draws, shared by the tests below."""
    zp = np.load(os.path.join(GOLDEN, "mv_pipeline_reference.npz"))
    cfg = json.loads(str(zp["cfg_json"]))
    names_shapes = [(str(n), tuple(int(v) for v in str(s).split(",")) if str(s) else ())
                    for n, s in zip(zp["names"], zp["shapes"])]
    unet = UNetMV2DConditionModel(
        sample_size=cfg["sample_size"], in_channels=cfg["in_channels"],
        out_channels=cfg["out_channels"], block_out_channels=tuple(cfg["block_out_channels"]),
        layers_per_block=cfg["layers_per_block"], cross_attention_dim=cfg["cross_attention_dim"],
        attention_head_dim=cfg["attention_head_dim"], norm_num_groups=cfg["norm_num_groups"],
        projection_class_embeddings_input_dim=cfg["projection_class_embeddings_input_dim"],
        num_views=cfg["num_views"], cd_attention_mid=cfg["cd_attention_mid"],
        down_block_types=tuple(cfg["down_block_types"]), up_block_types=tuple(cfg["up_block_types"]))
    unet.load_state_dict({k: v.float() for k, v in mv_weights.synth_state_dict(names_shapes).items()},
                         strict=True)
    unet = unet.half().to(dev).eval()
    vae = aux_state(LinearVAE().double().eval(), "aux.vae.").half().to(dev)
    clip = aux_state(LinearClip().double().eval(), "aux.clip.").half().to(dev)
    return {"pipe": MVDiffusionImagePipeline(unet, vae, clip),
            "imgs": input_image()[None].expand(12, -1, -1, -1).contiguous().to(dev),
            "cam": camera_embeddings().to(dev),
            "lat0": det_noise("draw.0", (12, 4, 32, 32)).half(),
            "noise": torch.stack([det_noise("draw.%d" % (i + 1), (12, 4, 32, 32)) for i in range(3)]).half()}


def _run(small, guidance_scale, steps=3, output_type="latent", callback=None, imgs=None):
    return small["pipe"](small["imgs"] if imgs is None else imgs, small["cam"], num_inference_steps=steps,
                         guidance_scale=guidance_scale, eta=1.0, latents=small["lat0"].clone(),
                         step_noise=small["noise"], output_type=output_type, callback=callback)


def test_guided_pipeline_vs_reference_pipeline_fixture(small):
    """The HIP pipeline at guidance_scale 3 against the reference's own guided pipeline in float64:
    same f16 input batch, camera embeddings, injected initial latents and per-step noise; 3 DDIM
    steps with eta = 1, decode, denormalise.  Bounds = the guidance-1 test's
    (test_pipeline_vs_reference_pipeline_fixture: latents rel-L2 5e-3, image mean 3e-3, max 8e-2)
    times 5: the guided prediction is (1 - g) u + g c, which amplifies the UNet's f16 error by at
    most |1 - g| + g = 5 at g = 3.  Latents after each step rel-L2 < 2.5e-2; images mean |d| <
    1.5e-2, max |d| < 4e-1.  (Measured values: PARITY.md, M7.)"""
    z = np.load(os.path.join(GOLDEN, "mv_cfg_reference.npz"))
    steps = int(z["steps"])
    got = []
    out = _run(small, float(z["guidance_scale"]), steps, "pt",
               callback=lambda i, t, lat: got.append(lat.float().cpu().double()))
    assert [int(t) for t in small["pipe"].scheduler.timesteps] == z["timesteps"].tolist()
    assert out.shape == (12, 3, 256, 256) and len(got) == steps
    rels = []
    for i, lat in enumerate(got):
        assert lat.shape == (12, 4, 32, 32)
        want = torch.from_numpy(z["lat_%d" % (i + 1)]).double()
        rels.append(float((lat - want).norm() / want.norm()))
    d = (out.float().cpu()[z["keep"]] - torch.from_numpy(z["out"].astype(np.float32))).abs()
    print("guided pipeline vs reference pipeline: latents rel-L2", ["%.2e" % r for r in rels],
          "image max|d| %.2e mean|d| %.2e" % (float(d.max()), float(d.mean())))
    assert max(rels) < 2.5e-2
    assert float(d.mean()) < 1.5e-2 and float(d.max()) < 4e-1


class _Stop(Exception):
    pass


def test_one_step_is_affine_in_the_guidance_scale(small):
    """The first UNet evaluation does not depend on g, and the step is affine in the guided
    prediction u + g (c - u): after ONE step (the first of the 3-step schedule, t = 667; the
    callback ends the run there) lat(3) = (lat(2) + lat(4)) / 2 up to the three roundings to f16 —
    half a spacing for lat(3), and half of (half + half) for the mean, each at its own magnitude,
    so one spacing at the largest of the three magnitudes bounds it (the kernel's arithmetic is
    double: its error is far below that)."""
    first = {}

    def keep_and_stop(g):
        def callback(i, t, lat):
            first[g] = lat.cpu().numpy().astype(np.float64)
            raise _Stop
        return callback

    for g in (2.0, 3.0, 4.0):
        with pytest.raises(_Stop):
            _run(small, g, callback=keep_and_stop(g))
    dev_ = np.abs(first[3.0] - (first[2.0] + first[4.0]) / 2)
    spacing = R.f16_spacing(np.maximum(np.maximum(np.abs(first[2.0]), np.abs(first[4.0])), np.abs(first[3.0])))
    print("affinity in g after one step: max deviation %.3f f16 spacings" % float((dev_ / spacing).max()))
    assert np.abs(first[4.0] - first[2.0]).max() > 0.1                 # guidance moves the latents at all
    assert (dev_ <= spacing).all()


def _churn(dev, sizes):
    """Device allocations of the given element counts (int64 zeros) on the current stream and on
    every stream of torch's pool, then released: a block that a capture still points at but nobody
    owns any more would be handed out here and overwritten (with zeros: a dangling gather index
    then reads row 0 and changes the output instead of leaving the buffer)."""
    keep = []
    for _ in range(33):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            keep += [torch.zeros(n, dtype=torch.int64, device=dev) for n in sizes]
    keep += [torch.zeros(n, dtype=torch.int64, device=dev) for n in sizes]
    torch.cuda.synchronize()


@pytest.mark.parametrize("use_graph", [False, True])
def test_guidance_1_is_untouched_by_guided_calls(dev, small, use_graph):
    """guidance_scale == 1 gives the same bytes before and after a guided call on the same pipeline
    object; with `use_graph` the B-row and the 2B-row shapes each keep their own capture, and going
    back and forth replays them — with device allocations in between, and every tensor the UNet
    caches per batch size (the captures point at them) still the one it was at capture time."""
    pipe = small["pipe"]
    pipe.use_graph = use_graph
    pipe.drop_graphs()
    try:
        before = _run(small, 1.0, 2)
        plain = pipe._graph
        guided = _run(small, 3.0, 2)
        idx = dict(pipe.unet.__dict__["_dsu_tproj_idx"])
        assert sorted(k[0] for k in idx) == [12, 24]
        sizes = sorted({t.numel() for t in idx.values()} | {4096, 1 << 16})
        _churn(dev, sizes)
        after = _run(small, 1.0, 2)
        _churn(dev, sizes)
        guided_again = _run(small, 3.0, 2)
        now = pipe.unet.__dict__["_dsu_tproj_idx"]
        assert all(now[k] is t and now[k].data_ptr() == t.data_ptr() for k, t in idx.items())
        if use_graph:
            assert len(pipe._graphs) == 2 and pipe._graphs[plain["key"]] is plain
            assert sorted(k[0][0] for k in pipe._graphs) == [12, 24]
            assert all(g["graph"] is not None for g in pipe._graphs.values())
            assert pipe._graph["key"][0][0] == 24                       # the one replayed last
            pipe._graph = None                                          # drops every capture
            assert not pipe._graphs and pipe._graph is None
        else:
            assert pipe._graph is None and not pipe._graphs
    finally:
        pipe.use_graph = False
        pipe.drop_graphs()
    assert torch.isfinite(before.float()).all() and torch.isfinite(guided.float()).all()
    assert torch.equal(before.view(torch.int16), after.view(torch.int16))
    assert torch.equal(guided.view(torch.int16), guided_again.view(torch.int16))
    assert not torch.equal(before, guided)


@pytest.mark.parametrize("guidance_scale", [1.0, 3.0])
def test_graph_replay_matches_eager_on_the_next_image_too(small, guidance_scale):
    """The capture is made on one image and replayed on another: everything that depends on the
    image (the UNet's cached cross-attention term included) must be inside it, without guidance
    and with it."""
    pipe = small["pipe"]
    other = small["imgs"].flip(-1).contiguous()
    eager, eager_other = _run(small, guidance_scale, 2), _run(small, guidance_scale, 2, imgs=other)
    pipe.use_graph = True
    pipe.drop_graphs()
    try:
        replayed = _run(small, guidance_scale, 2)
        replayed_other = _run(small, guidance_scale, 2, imgs=other)
        assert len(pipe._graphs) == 1
    finally:
        pipe.use_graph = False
        pipe.drop_graphs()
    assert not torch.equal(eager, eager_other)
    assert torch.equal(eager.view(torch.int16), replayed.view(torch.int16))
    assert torch.equal(eager_other.view(torch.int16), replayed_other.view(torch.int16))


# ------------------------------------------------------------------------------------ full width
@pytest.fixture(scope="module")
def drawing_pipeline(dev):
    from drawingspinup_amd.drawing import DrawingPipeline
    return DrawingPipeline(dev, seed=0, guidance_scale=3.0, mv_steps=2, nsr_steps=2, n_frames=1,
                           with_contour=False, with_matting=False)


def test_full_width_guided_batch(dev, drawing_pipeline):
    """The shipped architecture at B = 24 rows of 32x32 latents (4 multi-view groups of 6, joint
    pairs i / i + 12), 2 steps at g = 3."""
    from drawingspinup_amd.drawing import synthetic_drawing
    img = synthetic_drawing(7, size=256, device=dev)
    imgs = (img[:3] * img[3:4] + (1 - img[3:4]))[None].expand(12, -1, -1, -1).contiguous()
    gen = torch.Generator(device=dev).manual_seed(0)
    out = drawing_pipeline.mv(imgs.half(), generator=gen, guidance_scale=3.0, eta=1.0,
                              num_inference_steps=2, output_type="latent")
    assert out.shape == (12, 4, 32, 32) and out.dtype == torch.float16
    assert torch.isfinite(out.float()).all()


def test_drawing_pipeline_passes_guidance_scale_through(dev, drawing_pipeline):
    from drawingspinup_amd.drawing import synthetic_drawing
    dp = drawing_pipeline
    assert dp.guidance_scale == 3.0
    drawing = synthetic_drawing(7, device=dev)
    seen = []
    unet_forward = dp.mv.unet.forward
    dp.mv.unet.forward = lambda x, *a: seen.append(x.shape[0]) or unet_forward(x, *a)
    try:
        guided = dp.multiview(drawing, 5)
        dp.guidance_scale = 1.0
        plain = dp.multiview(drawing, 5)
    finally:
        dp.guidance_scale = 3.0
        del dp.mv.unet.forward
    assert seen == [24, 24, 12, 12]
    assert len(guided) == len(plain) == 2
    for a, b in zip(guided, plain):
        assert a.shape == b.shape == (6, 3, 256, 256) and a.dtype == b.dtype
        assert torch.isfinite(a.float()).all() and 0 <= float(a.min()) and float(a.max()) <= 1


def test_entry_mv_runs_a_yaml_with_guidance_scale_3(dev, drawing_pipeline, tmp_path, monkeypatch):
    """`guidance_scale: 3.0` in the YAML's pipe_validation_kwargs reaches the pipeline through
    entry/mv.py and the run ends in its PNGs (the shared full-width pipeline stands in for the one
    `--random_init` would build: same constructor, minutes of host time saved)."""
    import yaml
    from PIL import Image
    from drawingspinup_amd.drawing import synthetic_drawing
    from drawingspinup_amd.entry import config as C
    from drawingspinup_amd.entry import mv
    conf = C._plain(C.BUILTIN["mvdiffusion-joint-ortho-6views"])
    conf["pipe_validation_kwargs"]["guidance_scale"] = 3.0
    path = os.path.join(str(tmp_path), "mvdiffusion-guided.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(conf, f)
    root, uid = str(tmp_path), "uid0"
    os.makedirs(os.path.join(root, uid, "char"))
    rgba = (synthetic_drawing(7, device="cpu").permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()
    Image.fromarray(rgba, "RGBA").save(os.path.join(root, uid, "char", "ffc_resnet_inpainted.png"))
    rows = []
    pipe = drawing_pipeline.mv
    monkeypatch.setattr(mv, "build_random_pipeline", lambda device, seed=0: pipe)
    unet_forward = pipe.unet.forward
    pipe.unet.forward = lambda x, *a: rows.append(x.shape[0]) or unet_forward(x, *a)
    try:
        mv.main(["--config", path, "--uid", uid, "--data_root", root, "--num_inference_steps", "2",
                 "--random_init"])
    finally:
        del pipe.unet.forward
    assert rows == [24, 24]
    for sub in ("color", "normal", "mask"):
        files = sorted(os.listdir(os.path.join(root, uid, "mv", sub)))
        assert files == sorted(f"{v}.png" for v in ("front", "front_right", "right", "back", "left", "front_left"))
    assert Image.open(os.path.join(root, uid, "mv", "normal", "left.png")).size == (1024, 1024)
