"""Kernel time of the textured frame rasteriser (csrc/mesh_render.hip) at production size: the
51 200-face torus of the tests, a 1024^2 atlas from uv_mapping, 24 frames at 512^2 with 4x4
sub-samples.  Each arm is one `rocprofv3 --kernel-trace --stats` run (no counters) of a worker
process that launches every kernel --launches times; the per-dispatch durations of the trace give
the median and the range.

    python tools/render_tex_probe.py [--parent-root DIR] [--launches 30] [--out profiles/render_tex_probe.json]

--parent-root: a checkout of the parent commit with its library built.  Its untextured kernel is
then measured twice, alternating with this tree's (parent, this, parent, this): the difference
between the parent's own two runs is the spread the comparison is read against.  Without it only
this tree is measured (twice).  Needs a GPU and rocprofv3: there is no fallback.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))

# label -> how the ss = 4 instantiation is spelt in a trace, demangled (blanks removed) or mangled
KERNELS = {"untextured": ("mesh_raster_resolve_kernel<4>", "mesh_raster_resolve_kernelILi4EE"),
           "nearest": ("mesh_raster_resolve_textured_kernel<4,0>", "mesh_raster_resolve_textured_kernelILi4ELi0EE"),
           "bilinear": ("mesh_raster_resolve_textured_kernel<4,1>", "mesh_raster_resolve_textured_kernelILi4ELi1EE")}


def worker(root, launches):
    """Build the production case with the package under `root` and launch the raster kernels."""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import frame_render_ref as R
    from drawingspinup_amd import animate, ops
    from drawingspinup_amd.nsr import uv as U
    dev = torch.device("cuda:0")
    v, f = R.torus(200, 128, 0.38, 0.18)
    v = R.turn(v * (1.0 + 0.08 * np.sin(7.0 * v[:, :1] + 3.0 * v[:, 1:2])), 0.3, 0.9)
    m = U.uv_mapping(v, f, R.vertex_colours(len(v), 7), "torus", size=1024, device=dev)
    v, f = m["verts"], m["faces"]
    xyz = animate.rest_rotate(v, 24)
    cx, cy, size, span = animate.frame_window(xyz)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    screen, faces = t(xyz, np.float32), t(f, np.int64)
    pos = t(animate.position_colours(v), np.float32)
    colour = t(animate.render.sample_texture(m["image"], m["uvs"]), np.float32)
    plan = ops.MeshRenderPlan(screen, faces, cx, cy, span, size, 4).bin()
    want = ("color_u8", "pos_u8", "frames")
    textured = hasattr(ops, "texture_rgba")
    if textured:
        uv, tex = t(m["uvs"], np.float32), ops.texture_rgba(t(m["image"], np.uint8))
    for _ in range(launches):
        out = plan.raster(colour, pos, want)
    torch.cuda.synchronize()
    info = {"faces": int(len(f)), "verts": int(len(v)), "frames": 24, "size": int(size), "ss": 4,
            "texture": 1024, "bin_items": int(plan.items.numel()),
            "coverage": float((out["color_u8"][..., 3] > 0).float().mean()), "device": torch.cuda.get_device_name(0)}
    if textured:
        for flt in ("nearest", "bilinear"):
            for _ in range(launches):
                plan.raster(None, pos, want, uv=uv, texture=tex, filter=flt)
            torch.cuda.synchronize()
    print("PROBE_INFO " + json.dumps(info))


def durations(trace_dir):
    """kernel label -> per-dispatch durations in microseconds, from the kernel trace of one run."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    out = {k: [] for k in KERNELS}
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"].replace(" ", "")
                for label, needles in KERNELS.items():
                    if any(n in name for n in needles):
                        out[label].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return out


def summary(us):
    return {"launches": len(us), "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def run_arm(root, launches, keep):
    trace = tempfile.mkdtemp(prefix="render_tex_probe_", dir=keep)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    cmd = [rocprof, "--kernel-trace", "--stats", "-f", "csv", "-d", trace, "--", sys.executable,
           os.path.abspath(__file__), "--worker", "--root", root, "--launches", str(launches)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"the profiled worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    info = [json.loads(ln[len("PROBE_INFO "):]) for ln in r.stdout.splitlines() if ln.startswith("PROBE_INFO ")]
    res = {k: summary(v) for k, v in durations(trace).items() if v}
    shutil.rmtree(trace, ignore_errors=True)
    return res, info[0]


def resources():
    sys.path.insert(0, HERE)
    import isa_stats as isa
    txt = isa.compile_asm(os.path.join(isa.CSRC, "mesh_render.hip"))
    md = isa.metadata(txt)
    out = {}
    for name, _ in isa.bodies(txt):
        short = isa.demangle_short(name)
        if short.startswith("mesh_raster_resolve"):
            m = md[name]
            out[short] = {"vgpr": m["vgpr"], "sgpr": m["sgpr"], "scratch_bytes": m["scratch"], "lds_bytes": m["lds"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_tex_probe.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.root), a.launches)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = os.path.dirname(os.path.abspath(a.out))
    arms = [("parent", os.path.abspath(a.parent_root))] if a.parent_root else []
    order = (arms + [("this", ROOT)]) * 2
    runs, info = [], None
    for label, root in order:
        res, info = run_arm(root, a.launches, keep)
        runs.append({"tree": label, **res})
        print(label, json.dumps(res), flush=True)
    med = lambda tree, k: [r[k]["median_us"] for r in runs if r["tree"] == tree and k in r]
    this = med("this", "untextured")
    out = {"case": info, "launches_per_kernel": a.launches, "runs": runs,
           "untextured_this_median_us": this, "untextured_this_spread_us": max(this) - min(this),
           "textured_over_untextured": {k: statistics.mean(med("this", k)) / statistics.mean(this)
                                        for k in ("nearest", "bilinear")}}
    if a.parent_root:
        parent = med("parent", "untextured")
        out.update(untextured_parent_median_us=parent, untextured_parent_spread_us=max(parent) - min(parent),
                   untextured_this_minus_parent_us=statistics.mean(this) - statistics.mean(parent))
    try:
        out["kernel_resources"] = resources()
    except (SystemExit, OSError) as e:
        out["kernel_resources"] = {"unavailable": str(e)[:200]}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
