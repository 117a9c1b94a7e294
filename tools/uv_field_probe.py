"""Measure the field bake (dsu_uv_field_points / dsu_uv_field_resolve, csrc/mesh_uv.hip;
nsr/uv.bake_field) at production size: the 51 200-face probe mesh of tools/uv_probe.py, a 1024^2
atlas, a sphere-initialised NeuSModel as the field, 1, 2 and 4 sub-samples per axis.  Records
  * `kernel_us`: per bake, the time of the two new kernels, of the evaluation kernels (the SDF /
    finite-difference and texture kernels vertex_colors launches: names holding `sdf_` or
    `texture_`), of the other atlas kernels (`uv_`, the bake's binning) and of everything else
    (torch's: nonzero, normalize, casts, copies), from a `rocprofv3 --kernel-trace --stats` run of
    `--trace-samples S --trace-launches N` — one run per S, and one with N = 0 (DIR/s0: the set-up
    alone — parametrize, the network's initialisation — which is subtracted), read back with
    --kernel-stats,
  * `call_ms`: the whole bake_field call beside bake_vertex_colours in the same run, a host clock
    around the call and a device synchronise, median / min / max of --runs after warm-up; and
    `evaluation_ms`, device events around the calls of eval_colours inside it (the network's
    kernels AND the tensor operations of vertex_colors around them), summed per bake,
  * the number of points evaluated.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/s0 -- \
        python tools/uv_field_probe.py --trace-samples 1 --trace-launches 0
    for s in 1 2 4; do rocprofv3 --kernel-trace --stats --output-format csv -d DIR/s$s -- \
        python tools/uv_field_probe.py --trace-samples $s --trace-launches 3; done
    python tools/uv_field_probe.py [--size 1024] [--kernel-stats DIR] [--out profiles/uv_field_probe.json]

Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from drawingspinup_amd.nsr import uv as U  # noqa: E402
from drawingspinup_amd.nsr.mesh import field_colours  # noqa: E402
from drawingspinup_amd.nsr.model import NeuSModel  # noqa: E402
from uv_probe import character  # noqa: E402

SAMPLES = (1, 2, 4)


CLASSES = ("uv_field_points_kernel", "uv_field_resolve_kernel", "evaluation", "atlas", "other")


def class_totals(folder):
    """rocprofv3's kernel statistics under `folder` summed per class -> (microseconds, calls)."""
    import csv
    import glob
    paths = sorted(glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True))
    if not paths:
        raise SystemExit(f"--kernel-stats: no *kernel_stats.csv under {folder}")
    us, calls = dict.fromkeys(CLASSES, 0.0), dict.fromkeys(CLASSES, 0)
    for path in paths:
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            key = next((k for k in CLASSES[:2] if k in name), None) or \
                ("evaluation" if ("sdf_" in name or "texture_" in name) else
                 "atlas" if ("uv_" in name or "bin_" in name) else "other")
            us[key] += float(row["TotalDurationNs"]) / 1e3
            calls[key] += int(row["Calls"])
    return us, calls


def kernel_stats(folder, setup_folder, launches):
    """Microseconds per bake and class: the traced run's totals less the set-up run's, over `launches`."""
    us, calls = class_totals(folder)
    base, _ = class_totals(setup_folder)
    if not (calls["uv_field_points_kernel"] and calls["uv_field_resolve_kernel"]):
        raise SystemExit(f"--kernel-stats {folder}: the field kernels are not in the statistics")
    res = {k: (us[k] - base[k]) / launches for k in CLASSES}
    total = sum(res.values())
    res.update(total=total, evaluation_share=res["evaluation"] / total,
               field_kernels_share=(res["uv_field_points_kernel"] + res["uv_field_resolve_kernel"]) / total,
               launches_of_each_field_kernel_per_bake=calls["uv_field_points_kernel"] / launches)
    return res


class Timed:
    """A callable with device events around every call."""

    def __init__(self, fn):
        self.fn, self.pairs = fn, []

    def __call__(self, p):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = self.fn(p)
        b.record()
        self.pairs.append((a, b))
        return out

    def take_ms(self):
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in self.pairs)
        self.pairs.clear()
        return ms


def wall_ms(fn, runs, warmup=2, timed=None):
    """-> (median, min, max) of the call; with `timed`, also the same of its events' sum per call."""
    for _ in range(warmup):
        fn()
    ms, inner = [], []
    for _ in range(runs):
        if timed is not None:
            timed.take_ms()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if timed is not None:
            inner.append(timed.take_ms())
    three = lambda v: (statistics.median(v), min(v), max(v))
    return (three(ms), three(inner)) if timed is not None else three(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--gutter", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--trace-samples", type=int, default=0,
                    help="only bake with this many sub-samples per axis, --trace-launches times, and exit "
                         "(the run rocprofv3 traces)")
    ap.add_argument("--trace-launches", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None, help="folder with s0/ s1/ s2/ s4/ of those rocprofv3 runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_field_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    verts, faces, colours = character()
    S = args.size
    vm, ind, uvs = U.parametrize(verts, faces, S, args.gutter, device=dev)
    torch.manual_seed(0)
    model = NeuSModel().to(dev).eval()
    model.update_step(0, 0)
    field = Timed(field_colours(model))
    pos, fallback = verts[vm], colours[vm]
    bake = lambda s, **kw: U.bake_field(uvs, ind, pos, field, fallback, S, args.gutter, samples=s, device=dev, **kw)
    vertex = lambda: U.bake_vertex_colours(uvs, ind, fallback, S, args.gutter, device=dev)
    if args.trace_samples:
        for _ in range(args.trace_launches):
            bake(args.trace_samples)
        torch.cuda.synchronize()
        return
    per_s = {}
    for s in SAMPLES:
        img, fid, ev = bake(s, return_maps=True)
        n = int((fid >= 0).sum())
        call_ms, evaluation_ms = wall_ms(lambda: bake(s), args.runs, timed=field)
        per_s[str(s)] = {
            "covered_texels": n, "evaluated_texels": int((ev > 0).sum()), "points": n * s * s,
            "pieces": -(-n // max(1, (1 << 21) // (s * s))),
            "differs_from_vertex_bake_texels": int((img != vertex()).any(-1).sum()),
            "repeat_is_bit_identical": bool(np.array_equal(img, bake(s))),
            "call_ms": call_ms, "evaluation_ms": evaluation_ms,
            "kernel_us": kernel_stats(os.path.join(args.kernel_stats, f"s{s}"), os.path.join(args.kernel_stats, "s0"),
                                      args.trace_launches) if args.kernel_stats else None}
    res = {"device": torch.cuda.get_device_name(0), "faces": int(len(faces)), "new_vertices": int(len(vm)),
           "size": S, "gutter": args.gutter, "field": "NeuSModel(), sphere-initialised, step 0",
           "samples": per_s, "call_ms_bake_vertex_colours": wall_ms(vertex, args.runs),
           "call_ms_is": "host clock around one call (host arrays in, host image out) ending in a device "
                         "synchronise: median, min, max of `runs` after 2 warm-up calls",
           "evaluation_ms_is": "device events around the calls of eval_colours inside that call, summed per call",
           "kernel_us_is": "rocprofv3 --kernel-trace --stats over --trace-launches bakes, a run per sample count, "
                           "less a run of the set-up alone: microseconds per bake by class of kernel "
                           "(evaluation: names with sdf_ / texture_; other: torch's; null: not collected)",
           "runs": args.runs, "trace_launches": args.trace_launches}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
