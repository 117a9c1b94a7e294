"""Share of the texture backward's 32-sample halves that carry no colour gradient (d_rgb all zero:
samples behind the front surface, where the f32 transmittance has underflowed to 0), per step of a
whole fit.  Read from the liveness bitmap the compositing backward fills in the library's step
(dsu_nsr_driver_live_halves): no extra launch in the step, one popcount per step here.

    python tools/texture_dead_halves.py sphere [steps]     the synthetic-sphere fit of nsr_native_vs_fused.py
    python tools/texture_dead_halves.py drawing [steps]    the NSR fit of bench.py's first timed drawing
                                                           (contour removal and multi-view diffusion first)

Prints every 100th step (samples, halves, dead halves, share, inv_s) and the mean over all steps."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
from drawingspinup_amd import _lib, ops                                      # noqa: E402
from drawingspinup_amd.nsr.system import OrthoData, OrthoNeuSSystem          # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "sphere"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
dev = torch.device("cuda:0")
POP = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=dev)


def probed_fit(sysm, dataset, max_steps):
    """OrthoNeuSSystem.fit with the bitmap of every step counted (on the device, no synchronisation)."""
    sysm.dataset = dataset
    live = torch.zeros(max_steps, dtype=torch.int64, device=dev)
    halves, samples, inv_s = [], [], {}
    for s in range(max_steps):
        step = sysm.global_step
        r = sysm.training_step()
        drv = sysm._native
        assert drv is not None, "the probe reads the library-sequenced step"
        n = int(r["n_samples"])
        h = (n + 31) // 32
        p = int(_lib.lib().dsu_nsr_driver_live_halves(drv.handle, step))
        off = p - drv.workspace.data_ptr()
        words = drv.workspace[off:off + 4 * ((h + 31) // 32)]
        live[s] = POP[words.long()].sum()
        halves.append(h)
        samples.append(n)
        if s % 100 == 0 or s == max_steps - 1:
            inv_s[s] = float(sysm.model.variance.inv_s)
    if sysm.table_opt is not None:
        sysm.table_opt.finalize()
    live = live.cpu().tolist()
    shares = []
    for s in range(max_steps):
        dead = halves[s] - live[s]
        assert 0 <= dead <= halves[s], (s, halves[s], live[s])
        shares.append(dead / max(halves[s], 1))
        if s in inv_s:
            print(f"{what} step {s:5d}  samples {samples[s]:7d}  halves {halves[s]:6d}  dead {dead:6d}  "
                  f"share {shares[-1]:.3f}  inv_s {inv_s[s]:.1f}", flush=True)
    print(f"{what}: mean dead-half share over {max_steps} steps {sum(shares) / len(shares):.4f}  "
          f"(last 1000: {sum(shares[-1000:]) / len(shares[-1000:]):.4f}); "
          f"dead halves / halves over the fit {1 - sum(live) / sum(halves):.4f}", flush=True)


if what == "sphere":
    ds = OrthoData.synthetic_sphere(512, device=dev)
    sysm = OrthoNeuSSystem(device=dev, seed=3)
    sysm.step_mode = "native"
    torch.manual_seed(3)
    probed_fit(sysm, ds, steps)
else:
    import bench
    from drawingspinup_amd.drawing import DrawingPipeline, synthetic_drawing
    args = bench.parse(["--gpus", "1"])
    pipe = DrawingPipeline(dev, seed=0, mv_steps=args.mv_steps, nsr_steps=steps, n_frames=args.frames)
    class FitDone(Exception):
        pass

    def fit(self, dataset, max_steps=None, log_every=0):
        probed_fit(self, dataset, max_steps)
        raise FitDone()                                        # the export is not what is measured

    OrthoNeuSSystem.fit = fit
    drawing = synthetic_drawing(0, device=dev)                 # bench.py: seed rank * 100 + s of the timed drawings
    cleaned = pipe.remove_contour(drawing)
    normals, colors = pipe.multiview(cleaned, 123456)
    try:
        pipe.reconstruct(normals, colors, cleaned, 123456)
    except FitDone:
        pass
    torch.cuda.synchronize()
