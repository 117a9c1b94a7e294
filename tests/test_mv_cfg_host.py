"""Classifier-free guidance of the multi-view pipeline, CPU side.  tests/golden/mv_cfg_reference.npz
= the REFERENCE's own MVDiffusionImagePipeline.__call__ at guidance_scale 3 driving its own UNet
(float64, CPU, 3 steps, eta 1; tests/golden/make_mv_cfg_golden.py — the recipe of
mv_pipeline_reference.npz, whose UNet config / parameter names it shares):
  * mv.pipeline.cfg_conditioning reproduces the 24-row embeddings, image latents and camera
    embedding the reference handed its UNet;
  * the float64 guided loop of tests/mv_cfg_ref.py (which the GPU pipeline test's bounds lean on)
    reproduces the reference's latents after every step;
  * the attention tables at B = 24: joint attention pairs row i with i % 12 + 12 (the reference's
    chunk(2) quirk, reproduced), multi-view attention forms 4 groups of 6.
The HIP kernels and the guided pipeline are held to the same fixture in tests/test_gpu_mv_cfg.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_cfg_ref as R  # noqa: E402
from drawingspinup_amd.mv import preprocess as PP  # noqa: E402
from oracle import mv_ref as mr  # noqa: E402
from oracle import mv_weights  # noqa: E402
from oracle.mv_pipeline_aux import (LinearClip, LinearVAE, aux_state, camera_embeddings,  # noqa: E402
                                    det_noise, input_image)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "mv_cfg_reference.npz"))


def test_cfg_conditioning_matches_the_reference_pipeline(z):
    from drawingspinup_amd.mv.pipeline import cfg_conditioning
    u8 = PP.to_pil_u8(input_image()[None])
    clip = aux_state(LinearClip().double().eval(), "aux.clip.")
    vae = aux_state(LinearVAE().double().eval(), "aux.vae.")
    cam = camera_embeddings().double()
    with torch.no_grad():
        emb = clip(pixel_values=PP.clip_pixel_values(u8).double()).image_embeds.unsqueeze(1)
        lat = vae.encode_mode(PP.vae_input(u8, torch.float64)) * vae.scaling_factor
    emb, lat = emb.expand(12, -1, -1), lat.expand(12, -1, -1, -1)           # mv.py:70: 12 copies of one image
    emb2, lat2, cam2 = cfg_conditioning(emb, lat, torch.cat([torch.sin(cam), torch.cos(cam)], -1))
    assert emb2.shape == (24, 1, 768) and lat2.shape == (24, 4, 32, 32) and cam2.shape == (24, 10)
    np.testing.assert_allclose(emb2.numpy(), z["image_embeddings"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(lat2.numpy(), z["image_latents"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(cam2.numpy(), z["camera"], rtol=0, atol=2e-6)
    # the unconditional half really is zero in the reference, and its camera rows are the conditional ones
    assert not z["image_embeddings"][:12].any() and not z["image_latents"][:12].any()
    assert np.array_equal(z["camera"][:12], z["camera"][12:])
    # dtype and device follow the inputs (the pipeline hands it f16 device tensors)
    h = cfg_conditioning(emb.half(), lat.half(), cam2[:12].half())
    assert all(t.dtype == torch.float16 for t in h)


def test_float64_guided_loop_matches_the_reference_pipeline(z):
    zp = np.load(os.path.join(GOLDEN, "mv_pipeline_reference.npz"))         # same UNet: config and names
    cfg = json.loads(str(zp["cfg_json"]))
    names_shapes = [(str(n), tuple(int(v) for v in str(s).split(",")) if str(s) else ())
                    for n, s in zip(zp["names"], zp["shapes"])]
    ref = mr.UNetRef(mv_weights.synth_state_dict(names_shapes), tuple(cfg["block_out_channels"]),
                     tuple(cfg["down_block_types"]), tuple(cfg["up_block_types"]),
                     layers_per_block=cfg["layers_per_block"], heads=cfg["attention_head_dim"],
                     groups=cfg["norm_num_groups"], temb_dtype=torch.float32)
    steps = int(z["steps"])
    assert mr.ddim_timesteps(steps) == z["timesteps"].tolist()
    noise = [det_noise("draw.%d" % (i + 1), (12, 4, 32, 32)) for i in range(steps)]
    lats = R.guided_denoise_loop(ref, det_noise("draw.0", (12, 4, 32, 32)),
                                 torch.from_numpy(z["image_latents"]).double(),
                                 torch.from_numpy(z["image_embeddings"]).double(),
                                 torch.from_numpy(z["camera"]).double(), float(z["guidance_scale"]),
                                 steps, noise, eta=1.0)
    assert len(lats) == steps
    for i, lat in enumerate(lats):
        want = torch.from_numpy(z["lat_%d" % (i + 1)]).double()
        assert lat.shape == (12, 4, 32, 32)
        # inputs above went through the fixture's float32 storage
        assert float((lat - want).abs().max()) < 5e-6 * max(1.0, float(want.abs().max())), i


def test_attention_tables_at_the_guided_batch():
    from drawingspinup_amd.mv.unet import _seg_table
    joint = _seg_table("joint", 24, 0, "cpu").tolist()
    assert joint == [[i % 12, i % 12 + 12] for i in range(24)]
    mv = _seg_table("mv", 24, 6, "cpu").tolist()
    assert mv == [[i // 6 * 6 + s for s in range(6)] for i in range(24)]
    assert len({tuple(r) for r in mv}) == 4


def test_step_scalars_are_the_scheduler_steps_own():
    """DDIMScheduler.step_scalars feeds ops.ddim_cfg_step: the same f32 values `step` forms, at the
    first step, a middle one and the last (a_prev = alphas_cumprod[0])."""
    from drawingspinup_amd.mv.pipeline import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(75)
    acp = s.alphas_cumprod
    for t in (s.timesteps_host[0], s.timesteps_host[37], s.timesteps_host[-1]):
        prev_t = t - 1000 // 75
        a_t, a_prev = acp[t], acp[prev_t] if prev_t >= 0 else acp[0]
        var = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
        for eta in (0.0, 1.0):
            got = s.step_scalars(t, eta)
            want = (a_t ** 0.5, (1 - a_t) ** 0.5, a_prev ** 0.5, eta * var ** 0.5)
            assert got == tuple(float(w) for w in want)
            assert all(float(np.float32(v)) == v for v in got)
            assert 1.0 - got[2] ** 2 - got[3] ** 2 > 0
    assert s.timesteps_host[-1] == 1 and s.step_scalars(1, 1.0)[2] == float(acp[0] ** 0.5)
