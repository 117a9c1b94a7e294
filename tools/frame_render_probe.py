"""Time the frame renderer (csrc/mesh_render.hip) at production size: 24 frames of a ~50 000-face
mesh at 512^2 with 4x4 sub-samples, binning / raster + resolve / edges separately (median of 20
runs after warm-up, device events), beside the 24-frame stylisation of the same frames.

    python tools/frame_render_probe.py [--obj mesh.obj] [--frames 24] [--size 512] [--ss 4] [--runs 20]

Without --obj a seeded ~51 000-face blob stands in for the exported character.  Writes
profiles/frame_render_probe.json (or --out).  Needs a GPU: there is no fallback.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from drawingspinup_amd import animate, ops  # noqa: E402


def blob(nu=200, nv=128, seed=0):
    """A closed, bumpy, character-sized surface of 2 nu nv triangles (a thick ring, tilted)."""
    rng = np.random.default_rng(seed)
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    r = 0.18 * (1.0 + 0.15 * np.sin(3 * u + rng.uniform(0, 6)) * np.cos(2 * w))
    v = np.stack([(0.38 + r * np.cos(w)) * np.cos(u), 1.5 * r * np.sin(w) + 0.3 * np.sin(u),
                  (0.38 + r * np.cos(w)) * np.sin(u)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(nu) for j in range(nv)] + \
        [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(nu) for j in range(nv)]
    return v, np.asarray(f, np.int64), rng.random((len(v), 3)).astype(np.float32)


def edge_tests(xyz, faces, cx, cy, span, N):
    """(triangle, sample) pairs the raster stage evaluates: the bounding boxes of the kernel's
    sample_range (floor / ceil of the bounds, clipped to the frame), summed over frames and triangles."""
    total = 0
    for fr in xyz.astype(np.float32).astype(np.float64):
        t = fr[faces]
        lo, hi = t[..., :2].min(1), t[..., :2].max(1)
        c0 = np.floor(((lo[:, 0] - cx) / span + 0.5) * N - 0.5)
        c1 = np.ceil(((hi[:, 0] - cx) / span + 0.5) * N - 0.5)
        r0 = np.floor((0.5 - (hi[:, 1] - cy) / span) * N - 0.5)
        r1 = np.ceil((0.5 - (lo[:, 1] - cy) / span) * N - 0.5)
        w = np.clip(c1, 0, N - 1) - np.clip(c0, 0, N - 1) + 1
        h = np.clip(r1, 0, N - 1) - np.clip(r0, 0, N - 1) + 1
        seen = (c1 >= 0) & (r1 >= 0) & (c0 <= N - 1) & (r0 <= N - 1)
        total += int((w * h)[seen].sum())
    return total


def timed(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def kernel_resources(ss):
    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    try:
        txt = isa.compile_asm(os.path.join(isa.CSRC, "mesh_render.hip"))
    except (SystemExit, OSError) as e:
        return {"unavailable": str(e)[:200]}
    md = isa.metadata(txt)
    for name, _ in isa.bodies(txt):
        if isa.demangle_short(name) == f"mesh_raster_resolve_kernel<{ss}>":
            m = md[name]
            return {"lds_bytes": m["lds"], "vgpr": m["vgpr"], "sgpr": m["sgpr"], "scratch_bytes": m["scratch"],
                    "threads": 256}
    return {"unavailable": "kernel not found in the assembly"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", default=None)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ss", type=int, default=4)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-style", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_render_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_render_probe needs a GPU")
    dev = torch.device("cuda:0")
    if a.obj:
        v, f, col = animate.read_obj(a.obj)
    else:
        v, f, col = blob()
    xyz = animate.rest_rotate(v, a.frames)
    cx, cy, size, span = animate.frame_window(xyz)
    size = a.size
    screen = torch.from_numpy(xyz.astype(np.float32)).to(dev)
    faces = torch.from_numpy(f).to(dev)
    colour = torch.from_numpy(col).to(dev)
    pos = torch.from_numpy(animate.position_colours(v).astype(np.float32)).to(dev)
    plan = ops.MeshRenderPlan(screen, faces, cx, cy, span, size, a.ss)
    t_bin = timed(lambda: plan.bin(), a.runs)
    n_items = plan.items.numel()
    # raster writes color, pos and frames: what render_frames asks for
    F, S = a.frames, size
    outs = {"color_u8": torch.empty(F, S, S, 4, dtype=torch.uint8, device=dev),
            "pos_u8": torch.empty(F, S, S, 4, dtype=torch.uint8, device=dev),
            "frames": torch.empty(F, 6, S, S, device=dev)}
    order = ("color_u8", "pos_u8", "face_id", "depth", "frames", "pixels")
    t_raster = timed(lambda: plan._stage(ops.RENDER_RASTER, colour, pos, outs=[outs.get(k) for k in order]), a.runs)
    t_edge = timed(lambda: ops.pos_edge_u8(outs["pos_u8"]), a.runs)
    t_all = timed(lambda: animate.render_frames(v, f, col, xyz, ss=a.ss, device=dev, window=(cx, cy, size, span)),
                  max(3, a.runs // 4))
    tests = edge_tests(xyz, f, cx, cy, span, size * a.ss)
    coverage = float((outs["color_u8"][..., 3] > 0).float().mean())
    res = {"mesh": a.obj or "seeded blob", "faces": int(len(f)), "verts": int(len(v)), "frames": F, "size": S,
           "ss": a.ss, "span": span, "bins": plan.bins, "bin_items": int(n_items), "coverage": coverage,
           "runs": a.runs,
           "binning_ms": {"median": t_bin[0], "min": t_bin[1], "max": t_bin[2],
                          "note": "count + prefix sum (torch, one read-back) + fill"},
           "raster_resolve_ms": {"median": t_raster[0], "min": t_raster[1], "max": t_raster[2]},
           "edges_ms": {"median": t_edge[0], "min": t_edge[1], "max": t_edge[2]},
           "render_frames_ms": {"median": t_all[0], "min": t_all[1], "max": t_all[2],
                                "note": "host arrays in, device tensors out: uploads included"},
           "edge_function_tests": tests,
           "subsamples_tested_per_s": tests / (t_raster[0] * 1e-3),
           "lattice_samples_per_s": F * (S * a.ss) ** 2 / (t_raster[0] * 1e-3),
           "raster_kernel": kernel_resources(a.ss),
           "device": torch.cuda.get_device_name(0)}
    if not a.no_style:
        from drawingspinup_amd.drawing import DrawingPipeline
        pipe = DrawingPipeline(dev, seed=0, n_frames=F, with_mv=False, with_contour=False)
        edges = ops.pos_edge_u8(outs["pos_u8"])
        t_style = timed(lambda: pipe.stylize(outs["frames"], edges), 5, warmup=2)
        res["stylisation_ms"] = {"median": t_style[0], "min": t_style[1], "max": t_style[2], "frames": F}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
