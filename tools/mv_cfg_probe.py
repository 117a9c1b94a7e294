"""Time classifier-free guidance in the multi-view stage on the full-width model (random weights,
12 views of 32x32 latents): the denoising loop per step at guidance_scale 1 (12-row UNet) and 3
(24-row UNet plus the two kernels of csrc/mv_guidance.hip), and the two kernels beside the chain of
torch ops they replace (zeros_like + three cats; chunk + three elementwise ops + the f32 scheduler
step).  Device events, median of --runs after warm-up.

    python tools/mv_cfg_probe.py [--steps 10] [--runs 5] [--out profiles/mv_cfg_probe.json]

Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.mv.pipeline import build_random_pipeline  # noqa: E402


def timed(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv_cfg_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mv_cfg_probe: needs a GPU")
    dev = torch.device("cuda:0")
    pipe = build_random_pipeline(dev, seed=0, with_clip=False)
    g = torch.Generator().manual_seed(0)
    B, shape = 12, (12, 4, 32, 32)
    emb = torch.randn(B, 1, 768, generator=g).half().to(dev)
    img_lat = torch.randn(shape, generator=g).half().to(dev)
    pipe._encode_image = lambda images: (emb, img_lat)      # the loop alone: CLIP / VAE encode are not in it
    images = torch.zeros(B, 3, 256, 256, device=dev, dtype=torch.float16)
    lat0 = torch.randn(shape, generator=g).half().to(dev)
    noise = torch.randn((args.steps,) + shape, generator=g).half().to(dev)

    def loop(scale):
        return lambda: pipe(images, num_inference_steps=args.steps, guidance_scale=scale, eta=1.0,
                            latents=lat0, step_noise=noise, output_type="latent")

    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "runs": args.runs,
           "latents": list(shape)}
    for name, scale in (("g1", 1.0), ("g3", 3.0)):
        res["loop_ms_per_step_" + name] = timed(loop(scale), args.runs) / args.steps
    res["g3_over_g1"] = res["loop_ms_per_step_g3"] / res["loop_ms_per_step_g1"]

    # the kernels beside the torch ops of the same step, 200 calls per timing
    pipe.scheduler.set_timesteps(75)
    t = pipe.scheduler.timesteps_host[37]
    sc = pipe.scheduler.step_scalars(t, 1.0)
    pred = torch.randn((2 * B,) + shape[1:], generator=g).half().to(dev)
    img_lat2 = torch.cat([torch.zeros_like(img_lat), img_lat])
    reps = 200

    def many(fn):
        def run():
            for _ in range(reps):
                fn()
        return run

    def torch_input():
        return torch.cat([torch.cat([lat0] * 2), torch.cat([torch.zeros_like(img_lat), img_lat])], dim=1)

    def torch_input_hoisted():                               # the zero half assembled once per call, as the v_prediction path does
        return torch.cat([torch.cat([lat0] * 2), img_lat2], dim=1)

    def torch_step():
        u, c = pred.chunk(2)
        return pipe.scheduler.step(u + 3.0 * (c - u), t, lat0, eta=1.0, variance_noise=noise[0])

    res["us_per_call"] = {
        "dsu_cfg_model_input": 1e3 * timed(many(lambda: ops.cfg_model_input(lat0, img_lat)), args.runs) / reps,
        "torch_model_input": 1e3 * timed(many(torch_input), args.runs) / reps,
        "torch_model_input_zero_half_hoisted": 1e3 * timed(many(torch_input_hoisted), args.runs) / reps,
        "dsu_ddim_cfg_step": 1e3 * timed(many(lambda: ops.ddim_cfg_step(pred, lat0, noise[0], 3.0, *sc)),
                                         args.runs) / reps,
        "torch_guidance_and_step": 1e3 * timed(many(torch_step), args.runs) / reps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
