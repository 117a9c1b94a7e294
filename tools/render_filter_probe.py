"""Kernel time of the frame rasteriser's pixel filter (csrc/mesh_render.hip, csrc/film_filter.h) at
production size: the 51 200-face torus of the tests, 24 frames at 512^2 with 4x4 sub-samples, with
vertex colours and with a 1024^2 bilinear atlas.  Per colour source: the box kernel of the unfiltered
entry point, the filtered kernel at width 1.5 (cycles) and 3.0 (eevee), and the COUNT / FILL kernels
of the binning at hp = 0 / 1 / 2 pixels of tile growth (hp 2 is width 5.0, the widest accepted).
Each arm is one `rocprofv3 --kernel-trace --stats` run (no counters) of a worker process; the worker
logs the label of every launch in order, and the trace's dispatches of the rasteriser's kernels,
sorted by start time, are read against that log.

    python tools/render_filter_probe.py [--parent-root DIR] [--launches 30] [--out profiles/render_filter_probe.json]

--parent-root: a checkout of the parent commit with its library built.  Its box kernel is then
measured twice, alternating with this tree's (parent, this, parent, this): the difference between
the parent's own two runs is the spread this tree's box kernel is read against.  Without it only this
tree is measured (twice).  Also recorded, not asserted: the edge pixels (pos2edge) of the first frame
under the box, width 1.5 and width 3.0.  Needs a GPU and rocprofv3: there is no fallback.
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

SS, ATLAS = 4, 1024
WIDTHS = {"width_1.5": 1.5, "width_3.0": 3.0}
GROWTH = {"hp0": None, "hp1": 3.0, "hp2": 5.0}           # tile growth in pixels -> a width that has it at ss 4
TRACED = ("mesh_raster_resolve", "FrameTriangle")         # the kernels the log speaks of: resolves, binning


def worker(root, launches):
    """Build the production case with the package under `root`, launch the kernels, log the order."""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inspect
    import numpy as np
    import torch
    import frame_render_ref as R
    from drawingspinup_amd import animate, ops
    from drawingspinup_amd.nsr import uv as U
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    filtered = "pixel_filter" in inspect.signature(ops.mesh_render_ortho).parameters
    v0, f0 = R.torus(200, 128, 0.38, 0.18)
    v0 = R.turn(v0 * (1.0 + 0.08 * np.sin(7.0 * v0[:, :1] + 3.0 * v0[:, 1:2])), 0.3, 0.9)
    m = U.uv_mapping(v0, f0, R.vertex_colours(len(v0), 7), "torus", size=ATLAS, device=dev)
    v, f = m["verts"], m["faces"]
    xyz = animate.rest_rotate(v, 24)
    cx, cy, size, span = animate.frame_window(xyz)
    screen, faces = t(xyz, np.float32), t(f, np.int64)
    pos, uv = t(animate.position_colours(v), np.float32), t(m["uvs"], np.float32)
    col = t(animate.render.sample_texture(m["image"], m["uvs"]), np.float32)
    tex = ops.texture_rgba(t(m["image"], np.uint8))
    sources = {"vertex": dict(colour=col), "bilinear": dict(colour=None, uv=uv, texture=tex, filter="bilinear")}
    want = ("color_u8", "pos_u8", "frames")
    log = []                                                 # one label per traced kernel launch, in order
    info = {"device": torch.cuda.get_device_name(0), "frames": 24, "faces": int(len(f)), "verts": int(len(v)),
            "size": int(size), "ss": SS, "texture": ATLAS, "filtered": filtered, "bin_items": {}, "edge_pixels_frame0": {},
            "partial_pixels_frame0": {}}

    def note(name, out):
        info["edge_pixels_frame0"][name] = int((ops.pos_edge_u8(out["pos_u8"][:1]) == 0).sum())
        a = out["pos_u8"][0, :, :, 3]
        info["partial_pixels_frame0"][name] = int(((a > 0) & (a < 255)).sum())

    torch.cuda.synchronize()
    plan = ops.MeshRenderPlan(screen, faces, cx, cy, span, size, SS).bin()
    log += ["hp0/count", "hp0/fill"]
    info["bin_items"]["hp0"] = int(plan.items.numel())
    for name, kw in sources.items():
        kw = dict(kw)
        for _ in range(launches):
            out = plan.raster(kw.get("colour"), pos, want, **{k: kw[k] for k in kw if k != "colour"})
        log += [f"{name}/box"] * launches
        if name == "vertex":
            note("box", out)
    torch.cuda.synchronize()
    if filtered:
        for label, width in WIDTHS.items():
            taps, halo = animate.pixel_filter("blackman_harris", width, SS)
            fplan = ops.MeshRenderPlan(screen, faces, cx, cy, span, size, SS, halo).bin()
            log += [f"hp{-(-halo // SS)}/count", f"hp{-(-halo // SS)}/fill"]
            for name, kw in sources.items():
                kw = dict(kw)
                for _ in range(launches):
                    out = fplan.raster(kw.get("colour"), pos, want, taps=taps, **{k: kw[k] for k in kw if k != "colour"})
                log += [f"{name}/{label}"] * launches
                if name == "vertex":
                    note(label, out)
            torch.cuda.synchronize()
        for label, width in GROWTH.items():                  # the binning alone, `launches` times per growth
            halo = 0 if width is None else animate.pixel_filter("blackman_harris", width, SS)[1]
            bplan = ops.MeshRenderPlan(screen, faces, cx, cy, span, size, SS, halo)
            for _ in range(launches):
                bplan.count()
                bplan.fill(bplan.scan())
                log += [f"{label}/count", f"{label}/fill"]
            info["bin_items"][label] = int(bplan.items.numel())
        torch.cuda.synchronize()
    info["log"] = log
    print("PROBE_INFO " + json.dumps(info))


def durations(trace_dir, log):
    """label -> per-dispatch durations in microseconds: the traced kernels by start time, against the log."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    rows = []
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                if any(n in row["Kernel_Name"] for n in TRACED):
                    rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3,
                                 row["Kernel_Name"]))
    rows.sort()
    if len(rows) != len(log):
        raise SystemExit(f"{len(rows)} traced dispatches for {len(log)} logged launches")
    out = {}
    for (_, us, name), label in zip(rows, log):
        binning = label.endswith(("/count", "/fill"))
        if ("bin_kernel" in name) != binning or (not binning and ("filtered" in name) == label.endswith("/box")):
            raise SystemExit(f"launch {label!r} does not match dispatch {name!r}")
        out.setdefault(label, []).append(us)
    return out


def summary(us):
    return {"launches": len(us), "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def run_arm(root, launches, keep):
    trace = tempfile.mkdtemp(prefix="render_filter_probe_", dir=keep)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    cmd = [rocprof, "--kernel-trace", "--stats", "-f", "csv", "-d", trace, "--", sys.executable,
           os.path.abspath(__file__), "--worker", "--root", root, "--launches", str(launches)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise SystemExit(f"the profiled worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    info = [json.loads(ln[len("PROBE_INFO "):]) for ln in r.stdout.splitlines() if ln.startswith("PROBE_INFO ")][0]
    res = {k: summary(v) for k, v in durations(trace, info.pop("log")).items()}
    shutil.rmtree(trace, ignore_errors=True)
    return res, info


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_filter_probe.json"))
    ap.add_argument("--no-resources", action="store_true", help="leave the compiler's resource figures out")
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.root), a.launches)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = os.path.dirname(os.path.abspath(a.out))
    arms = [("parent", os.path.abspath(a.parent_root))] if a.parent_root else []
    runs, info = [], None
    for label, root in (arms + [("this", ROOT)]) * 2:
        res, arm_info = run_arm(root, a.launches, keep)
        if label == "this":
            info = arm_info
        runs.append({"tree": label, **res})
        print(label, json.dumps(res), flush=True)
    med = lambda tree, k: [r[k]["median_us"] for r in runs if r["tree"] == tree and k in r]
    out = {"case": info, "launches_per_kernel": a.launches, "runs": runs, "sources": {}, "binning": {}}
    for name in ("vertex", "bilinear"):
        box = med("this", f"{name}/box")
        c = {"box_this_median_us": box}
        for label in WIDTHS:
            flt = med("this", f"{name}/{label}")
            c[f"{label}_median_us"] = flt
            c[f"{label}_over_box_same_run"] = [x / b for x, b in zip(flt, box)]
        if a.parent_root:
            parent = med("parent", f"{name}/box")
            diff = statistics.mean(box) - statistics.mean(parent)
            c.update(box_parent_median_us=parent, box_parent_spread_us=max(parent) - min(parent),
                     box_this_minus_parent_us=diff, box_within_parent_spread=abs(diff) <= max(parent) - min(parent))
        out["sources"][name] = c
    for label in GROWTH:
        out["binning"][label] = {"count_median_us": med("this", f"{label}/count"), "fill_median_us": med("this", f"{label}/fill")}
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
