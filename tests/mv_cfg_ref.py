"""Float64 restatement of the multi-view pipeline's classifier-free-guidance branch
(2_charactor_reconstructor/mvdiffusion/pipelines/pipeline_mvdiffusion_image.py:164-180, 290-294,
463-486 with do_classifier_free_guidance) on oracle.mv_ref's UNet and DDIM step.  TEST
INFRASTRUCTURE ONLY; pinned to the reference's own pipeline by tests/test_mv_cfg_host.py
(tests/golden/mv_cfg_reference.npz)."""
import numpy as np
import torch

from oracle import mv_ref as mr


def conditioning(image_embeddings, image_latents, camera):
    """B rows -> 2B rows, unconditional half first: zero embedding, zero image latents, the camera
    embedding twice."""
    return (torch.cat([torch.zeros_like(image_embeddings), image_embeddings]),
            torch.cat([torch.zeros_like(image_latents), image_latents]),
            torch.cat([camera, camera]))


def guided_denoise_loop(unet, latents, image_latents2, image_embeddings2, camera2, guidance_scale,
                        num_inference_steps, step_noise, eta=1.0, run_steps=None):
    """`image_latents2` / `image_embeddings2` / `camera2` are the 2B-row tensors of `conditioning`;
    latents and step_noise keep B rows.  Returns the latents after each step."""
    acp = mr.ddim_alphas_cumprod()
    out = []
    lat = latents.double()
    for i, t in enumerate(mr.ddim_timesteps(num_inference_steps)[:run_steps]):
        model_in = torch.cat([torch.cat([lat] * 2), image_latents2.double()], 1)
        uncond, cond = unet(model_in, torch.tensor([t]), image_embeddings2, camera2).chunk(2)
        eps = uncond + guidance_scale * (cond - uncond)
        lat = mr.ddim_step(eps, t, lat, num_inference_steps, eta, step_noise[i], acp)
        out.append(lat)
    return out


def cfg_step_rule(noise_pred, latents, variance_noise, g, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, std):
    """The rule of dsu_ddim_cfg_step (include/dsu_hip.h) in float64 numpy, from the f16 tensors and
    the four f32 scalars the kernel is handed."""
    sa, sb, sp, sd = (float(np.float32(v)) for v in (sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, std))
    u, c = np.split(noise_pred.astype(np.float64), 2)
    n = u + float(np.float32(g)) * (c - u)
    x0 = (latents.astype(np.float64) - sb * n) / sa
    prev = sp * x0 + np.sqrt(max(1.0 - sp * sp - sd * sd, 0.0)) * n
    if variance_noise is not None:
        prev = prev + sd * variance_noise.astype(np.float64)
    return prev


def f16_spacing(v):
    """Distance between adjacent f16 values at |v| (float64 array): 2^(e-10) in the binade
    [2^e, 2^(e+1)), 2^-24 below the smallest normal 2^-14."""
    m, e = np.frexp(np.abs(v))                        # |v| = m 2^e, m in [0.5, 1); (0, 0) at zero
    return np.ldexp(1.0, np.maximum(np.where(m > 0, e - 1, -14), -14) - 10)
