"""Kernel time of the anisotropic frame rasteriser (csrc/mesh_render.hip, DSU_TEX_ANISOTROPIC) at
production size: the 51 200-face torus of the tests, the 24-frame turntable at 512^2, in two cases —
    ss4_T1024   4x4 sub-samples, a 1024^2 atlas
    ss1_T2048   one sample per pixel, a 2048^2 atlas
and the caps 2, 8 and 16.  Each arm is one `rocprofv3 --kernel-trace --stats` run (no counters) of a
worker process that launches the trilinear resolve and the anisotropic resolve at every cap
--launches times each, and builds the pyramid with the gutter each of them uses --builds times; the
per-dispatch durations of the trace give the median and the range.  The anisotropic launches of one
case are one kernel: they are told apart by their order in the trace (cap 2, 8, 16).

    python tools/render_aniso_probe.py [--parent-root DIR] [--launches 30] [--out profiles/render_aniso_probe.json]

--parent-root: a checkout of the parent commit with its library built.  Its trilinear kernel is then
measured twice, alternating with this tree's (parent, this, parent, this): the difference between
the parent's own two runs is the spread this tree's trilinear kernel is read against.  Without it
only this tree is measured (twice).  Needs a GPU and rocprofv3: there is no fallback.
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
CAPS = (2, 8, 16)
GUTTERS = (2,) + tuple(max(2, c) for c in CAPS)               # the trilinear build, then one per cap
PYRAMID = ("mip_reduce_kernel", "mip_dilate_kernel")


def _needles(ss, flt):
    return (f"mesh_raster_resolve_textured_kernel<{ss},{flt}>", f"mesh_raster_resolve_textured_kernelILi{ss}ELi{flt}EE")


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
    aniso = hasattr(ops, "ANISOTROPIC")
    info = {"device": torch.cuda.get_device_name(0), "frames": 24, "caps": list(CAPS), "cases": {}}
    for case, (ss, T) in CASES.items():                       # the kernels are told apart by this order
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
        covered = ops.uv_bake(uv, faces, torch.zeros(len(v), 3, device=dev), T)[1] >= 0
        for _ in range(builds):
            pyr = ops.mip_pyramid(tex, covered, GUTTERS[0])
        torch.cuda.synchronize()
        for _ in range(launches):
            tri = plan.raster(None, pos, want, uv=uv, texture=tex, filter="trilinear", pyramid=pyr)
        torch.cuda.synchronize()
        seen = tri["color_u8"][..., 3] == 255
        c = {"faces": int(len(f)), "verts": int(len(v)), "size": int(size), "ss": ss, "texture": T,
             "bin_items": int(plan.items.numel()), "fully_covered_pixels": int(seen.sum()),
             "atlas_fill": float(covered.float().mean())}
        info["cases"][case] = c
        if not aniso:
            continue
        # the pyramids as animate.render_frames builds them (mip_coverage "faces"): level 0 dilated by the
        # gutter, then the build with as many rounds; the dilation is not part of the timed build
        pyramids = {}
        for cap in CAPS:
            g = max(2, cap)
            rgb, cov = ops.uv_dilate(tex[..., :3].contiguous(), covered, g)
            level0 = torch.cat([rgb, tex[..., 3:]], -1).contiguous()
            torch.cuda.synchronize()
            for _ in range(builds):
                pyramids[cap] = (level0, ops.mip_pyramid(level0, cov, g))
            torch.cuda.synchronize()
        differing = {}
        for cap in CAPS:
            level0, p = pyramids[cap]
            for _ in range(launches):
                out = plan.raster(None, pos, want, uv=uv, texture=level0, filter="anisotropic", pyramid=p,
                                  max_anisotropy=cap)
            torch.cuda.synchronize()
            differing[str(cap)] = float(((out["color_u8"] != tri["color_u8"]).any(-1) & seen).sum() / seen.sum())
        # N over the (frame, face) pairs: the restatement's footprint on the same f32 inputs
        import frame_render_aniso_ref as AR
        sv, tt, fi = xyz.astype(np.float32).astype(np.float64), m["uvs"].astype(np.float32).astype(np.float64), f
        hist = {str(cap): np.zeros(cap + 1, np.int64) for cap in CAPS}
        for i in range(len(sv)):
            for cap in CAPS:
                fp = AR.footprint(sv[i][fi[:, 0]], sv[i][fi[:, 1]], sv[i][fi[:, 2]], tt[fi[:, 0]], tt[fi[:, 1]],
                                  tt[fi[:, 2]], T, float(span) / float(size * ss), cap, levels(T))
                hist[str(cap)] += np.bincount(fp["N"], minlength=cap + 1)
        c.update(pixels_differing_from_trilinear=differing,
                 probes_histogram_over_frame_face_pairs={k: h[1:].tolist() for k, h in hist.items()})
    print("PROBE_INFO " + json.dumps(info))


def durations(trace_dir, launches, builds, aniso):
    """label -> per-dispatch durations in microseconds; `<case>/pyramid_build_gutter<g>` -> the summed
    kernel time of each build."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    rows = []
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"].replace(" ", ""),
                             (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows.sort()
    out = {}
    pyramid = [us for _, name, us in rows if any(n in name for n in PYRAMID)]
    at = 0
    for case, (ss, T) in CASES.items():
        out[f"{case}/trilinear"] = [us for _, name, us in rows if any(n in name for n in _needles(ss, 2))]
        ani = [us for _, name, us in rows if any(n in name for n in _needles(ss, 3))]
        for j, cap in enumerate(CAPS):
            out[f"{case}/anisotropic_cap{cap}"] = ani[j * launches:(j + 1) * launches]
        for j, g in enumerate(GUTTERS if aniso else GUTTERS[:1]):
            per = (levels(T) - 1) * (1 + g)                   # kernels of one build
            if len(pyramid) >= at + per * builds:
                label = f"{case}/pyramid_build_gutter{g}" + ("_trilinear" if j == 0 else f"_cap{CAPS[j - 1]}")
                out[label] = [sum(pyramid[at + i * per:at + (i + 1) * per]) for i in range(builds)]
            at += per * builds
    return out


def summary(us):
    return {"launches": len(us), "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def run_arm(root, launches, builds, keep):
    trace = tempfile.mkdtemp(prefix="render_aniso_probe_", dir=keep)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    cmd = [rocprof, "--kernel-trace", "--stats", "-f", "csv", "-d", trace, "--", sys.executable,
           os.path.abspath(__file__), "--worker", "--root", root, "--launches", str(launches), "--builds", str(builds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise SystemExit(f"the profiled worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    info = [json.loads(ln[len("PROBE_INFO "):]) for ln in r.stdout.splitlines() if ln.startswith("PROBE_INFO ")]
    aniso = "probes_histogram_over_frame_face_pairs" in next(iter(info[0]["cases"].values()))
    res = {k: summary(v) for k, v in durations(trace, launches, builds, aniso).items() if v}
    shutil.rmtree(trace, ignore_errors=True)
    return res, info[0]


def resources():
    sys.path.insert(0, HERE)
    import isa_stats as isa
    out = {}
    txt = isa.compile_asm(os.path.join(isa.CSRC, "mesh_render.hip"))
    md = isa.metadata(txt)
    for name, _ in isa.bodies(txt):
        short = isa.demangle_short(name)
        if short.startswith("mesh_raster_resolve"):
            m = md[name]
            out[short] = {"vgpr": m["vgpr"], "sgpr": m["sgpr"], "scratch_bytes": m["scratch"], "lds_bytes": m["lds"],
                          "vgpr_spills": m["vspill"], "sgpr_spills": m["sspill"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_aniso_probe.json"))
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
        tri = med("this", f"{case}/trilinear")
        c = {"trilinear_this_median_us": tri}
        for cap in CAPS:
            ani = med("this", f"{case}/anisotropic_cap{cap}")
            c[f"anisotropic_cap{cap}_this_median_us"] = ani
            c[f"anisotropic_cap{cap}_over_trilinear_same_run"] = [x / y for x, y in zip(ani, tri)]
        for k in sorted({k for r in runs for k in r if k.startswith(f"{case}/pyramid_build")}):
            c[k.split("/")[1] + "_kernel_sum_median_us"] = med("this", k)
        if a.parent_root:
            parent = med("parent", f"{case}/trilinear")
            c.update(trilinear_parent_median_us=parent, trilinear_parent_spread_us=max(parent) - min(parent),
                     trilinear_this_minus_parent_us=statistics.mean(tri) - statistics.mean(parent),
                     trilinear_this_inside_parent_spread=bool(min(parent) <= statistics.mean(tri) <= max(parent)))
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
