"""Kernel time of the mip-mapped frame rasteriser (csrc/mesh_render.hip, csrc/mesh_mip.hip) at
production size: the 51 200-face torus of the tests, 24 frames at 512^2, in two cases —
    ss4_T1024   4x4 sub-samples, a 1024^2 atlas (the default: a sub-sample is about a texel)
    ss1_T2048   one sample per pixel, a 2048^2 atlas (the aliasing case the filter is for)
Each arm is one `rocprofv3 --kernel-trace --stats` run (no counters) of a worker process that
launches the bilinear and the trilinear resolve --launches times each and builds the pyramid
--builds times; the per-dispatch durations of the trace give the median and the range, and the
pyramid's kernels (one reduction and `gutter` dilations per level) are summed per build.

    python tools/render_mip_probe.py [--parent-root DIR] [--launches 30] [--out profiles/render_mip_probe.json]

--parent-root: a checkout of the parent commit with its library built.  Its bilinear kernel is then
measured twice, alternating with this tree's (parent, this, parent, this): the difference between
the parent's own two runs is the spread the comparison is read against.  Without it only this tree
is measured (twice).  Needs a GPU and rocprofv3: there is no fallback.
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

CASES = {"ss4_T1024": (4, 1024), "ss1_T2048": (1, 2048)}
GUTTER = 2


def _needles(ss, flt):
    return (f"mesh_raster_resolve_textured_kernel<{ss},{flt}>", f"mesh_raster_resolve_textured_kernelILi{ss}ELi{flt}EE")


# label -> how the instantiation is spelt in a trace, demangled (blanks removed) or mangled
KERNELS = {f"{case}/{name}": _needles(ss, flt) for case, (ss, _) in CASES.items()
           for name, flt in (("bilinear", 1), ("trilinear", 2))}
PYRAMID = ("mip_reduce_kernel", "mip_dilate_kernel")


def levels(T):
    L = 1
    while T > 1:
        T, L = (T + 1) // 2, L + 1
    return L


def worker(root, launches, builds):
    """Build the production cases with the package under `root` and launch the kernels."""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import frame_render_ref as R
    from drawingspinup_amd import animate, ops
    from drawingspinup_amd.nsr import uv as U
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    v0, f0 = R.torus(200, 128, 0.38, 0.18)
    v0 = R.turn(v0 * (1.0 + 0.08 * np.sin(7.0 * v0[:, :1] + 3.0 * v0[:, 1:2])), 0.3, 0.9)
    mip = hasattr(ops, "mip_pyramid")
    info = {"device": torch.cuda.get_device_name(0), "frames": 24, "gutter": GUTTER, "cases": {}}
    for case, (ss, T) in CASES.items():                       # the pyramid kernels are told apart by this order
        m = U.uv_mapping(v0, f0, R.vertex_colours(len(v0), 7), "torus", size=T, device=dev)
        v, f = m["verts"], m["faces"]
        xyz = animate.rest_rotate(v, 24)
        cx, cy, size, span = animate.frame_window(xyz)
        screen, faces = t(xyz, np.float32), t(f, np.int64)
        pos, uv = t(animate.position_colours(v), np.float32), t(m["uvs"], np.float32)
        # a high-frequency texture: the bake with every other texel inverted
        yy, xx = np.mgrid[:T, :T]
        image = np.where(((yy + xx) % 2 == 0)[..., None], m["image"], 255 - m["image"]).astype(np.uint8)
        tex = ops.texture_rgba(t(image, np.uint8))
        plan = ops.MeshRenderPlan(screen, faces, cx, cy, span, size, ss).bin()
        want = ("color_u8", "pos_u8", "frames")
        for _ in range(launches):
            out = plan.raster(None, pos, want, uv=uv, texture=tex, filter="bilinear")
        torch.cuda.synchronize()
        info["cases"][case] = {"faces": int(len(f)), "verts": int(len(v)), "size": int(size), "ss": ss, "texture": T,
                               "bin_items": int(plan.items.numel()),
                               "coverage": float((out["color_u8"][..., 3] > 0).float().mean())}
        if not mip:
            continue
        covered = ops.uv_bake(uv, faces, torch.zeros(len(v), 3, device=dev), T)[1] >= 0
        for _ in range(builds):
            pyr = ops.mip_pyramid(tex, covered, GUTTER)
        torch.cuda.synchronize()
        for _ in range(launches):
            tri = plan.raster(None, pos, want, uv=uv, texture=tex, filter="trilinear", pyramid=pyr)
        torch.cuda.synchronize()
        seen = out["color_u8"][..., 3] == 255
        info["cases"][case].update(
            atlas_fill=float(covered.float().mean()), pyramid_bytes=int(pyr.buffer.numel()),
            pyramid_workspace_bytes=int(ops.lib().dsu_mip_workspace_bytes(T)),
            pixels_differing_from_bilinear=float(((tri["color_u8"] != out["color_u8"]).any(-1) & seen).sum() / seen.sum()))
    print("PROBE_INFO " + json.dumps(info))


def durations(trace_dir, builds):
    """kernel label -> per-dispatch durations in microseconds; `<case>/pyramid_build` -> the summed
    kernel time of each build."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    out = {k: [] for k in KERNELS}
    pyramid = []
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"].replace(" ", "")
                us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                for label, needles in KERNELS.items():
                    if any(n in name for n in needles):
                        out[label].append(us)
                if any(n in name for n in PYRAMID):
                    pyramid.append((int(row["Start_Timestamp"]), us))
    pyramid = [us for _, us in sorted(pyramid)]
    at = 0
    for case, (_, T) in CASES.items():
        per = (levels(T) - 1) * (1 + GUTTER)                  # kernels of one build
        if len(pyramid) >= at + per * builds:
            out[f"{case}/pyramid_build"] = [sum(pyramid[at + i * per:at + (i + 1) * per]) for i in range(builds)]
        at += per * builds
    return out


def summary(us):
    return {"launches": len(us), "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def run_arm(root, launches, builds, keep):
    trace = tempfile.mkdtemp(prefix="render_mip_probe_", dir=keep)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    cmd = [rocprof, "--kernel-trace", "--stats", "-f", "csv", "-d", trace, "--", sys.executable,
           os.path.abspath(__file__), "--worker", "--root", root, "--launches", str(launches), "--builds", str(builds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise SystemExit(f"the profiled worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    info = [json.loads(ln[len("PROBE_INFO "):]) for ln in r.stdout.splitlines() if ln.startswith("PROBE_INFO ")]
    res = {k: summary(v) for k, v in durations(trace, builds).items() if v}
    shutil.rmtree(trace, ignore_errors=True)
    return res, info[0]


def resources():
    sys.path.insert(0, HERE)
    import isa_stats as isa
    out = {}
    for src, prefix in (("mesh_render.hip", "mesh_raster_resolve"), ("mesh_mip.hip", "mip_")):
        txt = isa.compile_asm(os.path.join(isa.CSRC, src))
        md = isa.metadata(txt)
        for name, _ in isa.bodies(txt):
            short = isa.demangle_short(name)
            if short.startswith(prefix):
                m = md[name]
                out[short] = {"vgpr": m["vgpr"], "sgpr": m["sgpr"], "scratch_bytes": m["scratch"], "lds_bytes": m["lds"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--builds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_mip_probe.json"))
    ap.add_argument("--no-resources", action="store_true", help="leave the compiler's resource figures out")
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.root), a.launches, a.builds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = os.path.dirname(os.path.abspath(a.out))
    arms = [("parent", os.path.abspath(a.parent_root))] if a.parent_root else []
    order = (arms + [("this", ROOT)]) * 2
    runs, info = [], None
    for label, root in order:
        res, arm_info = run_arm(root, a.launches, a.builds, keep)
        if label == "this":
            info = arm_info
        runs.append({"tree": label, **res})
        print(label, json.dumps(res), flush=True)
    med = lambda tree, k: [r[k]["median_us"] for r in runs if r["tree"] == tree and k in r]
    out = {"case": info, "launches_per_kernel": a.launches, "builds": a.builds, "runs": runs, "cases": {}}
    for case in CASES:
        bil, tri = med("this", f"{case}/bilinear"), med("this", f"{case}/trilinear")
        c = {"bilinear_this_median_us": bil, "trilinear_this_median_us": tri,
             "trilinear_over_bilinear_same_run": [t / b for t, b in zip(tri, bil)],
             "pyramid_build_kernel_sum_median_us": med("this", f"{case}/pyramid_build")}
        if a.parent_root:
            parent = med("parent", f"{case}/bilinear")
            c.update(bilinear_parent_median_us=parent, bilinear_parent_spread_us=max(parent) - min(parent),
                     bilinear_this_minus_parent_us=statistics.mean(bil) - statistics.mean(parent),
                     trilinear_over_parent_bilinear=statistics.mean(tri) / statistics.mean(parent))
        out["cases"][case] = c
    if not a.no_resources:
        try:
            out["kernel_resources"] = resources()
        except (SystemExit, OSError) as e:
            out["kernel_resources"] = {"unavailable": str(e)[:200]}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
