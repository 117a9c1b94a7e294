"""Generate tests/golden/mv_cfg_reference.npz: the recipe of make_mv_pipeline_golden.py (the
REFERENCE's own MVDiffusionImagePipeline.__call__ and UNetMV2DConditionModel, UNMODIFIED, float64,
CPU, reduced width, sample_size 32, the same stand-ins and the same deterministic draws) run WITH
classifier-free guidance: 3 steps, eta = 1, guidance_scale = 3.

    python tests/golden/make_mv_cfg_golden.py          # needs /root/reference

What the guided branch adds to the pinned glue (pipeline_mvdiffusion_image.py): the zero
"negative" image embedding and the zero image latents stacked IN FRONT of the conditional ones
(:164-180), the camera embedding duplicated (:290-294), `cat([latents] * 2)` (:465), the 24-row UNet
call — whose joint attention chunks the batch in two and therefore pairs row i with row
i % 12 + 12, unconditional with conditional (transformer_mv2d.py:878-883) — and
`uncond + guidance_scale * (cond - uncond)` (:476-477) ahead of the scheduler step.  Initial latents,
per-step noise and the callback's latents keep 12 rows.

The UNet config, parameter names and the input image are those of mv_pipeline_reference.npz (not
stored twice); recorded here: the 24-row image_embeddings / image_latents / camera the reference
handed its UNet, the timesteps, the latents after every step and out[KEEP] as f16.
"""
import os
import sys

import numpy as np
import torch

from transformers import CLIPImageProcessor  # the REAL one; imported before the stand-ins below
CLIPImageProcessor()                             # (transformers probes `torchvision` lazily)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/2_charactor_reconstructor"
sys.path.insert(0, os.path.join(ROOT, "oracle", "stubs"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import mv_weights  # noqa: E402
from oracle.mv_pipeline_aux import (LinearVAE, LinearClip, aux_state, input_image,  # noqa: E402
                                    camera_embeddings, det_noise)
from diffusers.schedulers import DDIMScheduler  # noqa: E402  (stub)
import diffusers.schedulers as stub_sched  # noqa: E402
from mvdiffusion.models.unet_mv2d_condition import UNetMV2DConditionModel  # noqa: E402
from mvdiffusion.pipelines import pipeline_mvdiffusion_image as ref_pipe  # noqa: E402

from make_mv_reference_golden import CFG as UNET_CFG  # noqa: E402  (same directory)

STEPS = 3
GUIDANCE_SCALE = 3.0
KEEP = [0, 5, 6, 11]


def main():
    torch.set_grad_enabled(False)
    cfg = dict(UNET_CFG, sample_size=32)
    unet = UNetMV2DConditionModel(**cfg).double().eval()
    names_shapes = [(k, tuple(v.shape)) for k, v in unet.state_dict().items()]
    unet.load_state_dict(mv_weights.synth_state_dict(names_shapes), strict=True)
    unet.enable_xformers_memory_efficient_attention()
    vae = aux_state(LinearVAE().double().eval(), "aux.vae.")
    clip = aux_state(LinearClip().double().eval(), "aux.clip.")

    draws = []

    def fake_randn(shape, generator=None, device=None, dtype=None, layout=None):
        draws.append(tuple(shape))
        return det_noise("draw.%d" % (len(draws) - 1), tuple(shape)).to(dtype)

    ref_pipe.randn_tensor = fake_randn            # prepare_latents (pipeline :266)
    stub_sched.randn_tensor = fake_randn          # DDIMScheduler.step variance noise

    pipe = ref_pipe.MVDiffusionImagePipeline(
        vae=vae, image_encoder=clip, unet=unet, scheduler=DDIMScheduler(), safety_checker=None,
        feature_extractor=CLIPImageProcessor(), requires_safety_checker=False, num_views=6)
    pipe.set_progress_bar_config(disable=True)

    rec = {}
    enc = pipe._encode_image

    def spy_encode(image_pil, *a, **k):
        e, l = enc(image_pil, *a, **k)
        rec["image_embeddings"], rec["image_latents"] = e.clone(), l.clone()
        return e, l
    pipe._encode_image = spy_encode
    cam_fn = pipe.prepare_camera_embedding

    def spy_cam(*a, **k):
        rec["camera"] = cam_fn(*a, **k).clone()
        return rec["camera"]
    pipe.prepare_camera_embedding = spy_cam
    steps = []

    img = input_image()
    imgs_in = img[None].expand(12, -1, -1, -1).contiguous()               # mv.py:70 (f16 batch)
    out = pipe(imgs_in, camera_embeddings(), generator=None, output_type="pt",
               num_images_per_prompt=1, num_inference_steps=STEPS, guidance_scale=GUIDANCE_SCALE,
               eta=1.0, callback=lambda i, t, lat: steps.append((int(t), lat.clone()))).images
    assert out.shape == (12, 3, 256, 256) and len(steps) == STEPS and len(draws) == STEPS + 1
    assert all(d == (12, 4, 32, 32) for d in draws)                       # the draws keep 12 rows
    assert rec["image_embeddings"].shape == (24, 1, 768) and rec["image_latents"].shape == (24, 4, 32, 32)
    assert rec["camera"].shape == (24, 10)
    print("timesteps", [t for t, _ in steps], "draws", draws)
    print("out rms", float(out.pow(2).mean().sqrt()), "min/max", float(out.min()), float(out.max()))
    arrays = {
        "steps": np.int64(STEPS), "guidance_scale": np.float64(GUIDANCE_SCALE),
        "timesteps": np.array([t for t, _ in steps]), "keep": np.array(KEEP),
        "image_embeddings": rec["image_embeddings"].numpy().astype(np.float32),
        "image_latents": rec["image_latents"].numpy().astype(np.float32),
        "camera": rec["camera"].numpy().astype(np.float32),
        "out": out[KEEP].numpy().astype(np.float16),
    }
    for i, (_, lat) in enumerate(steps):
        arrays["lat_%d" % (i + 1)] = lat.numpy().astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "mv_cfg_reference.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
