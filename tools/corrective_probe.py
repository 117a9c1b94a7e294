"""Time the corrective smoothing (csrc/mesh_corrective.hip) on the probe character of
tools/skin_probe.py (25 092 vertices, 120 frames).  A worker process runs twice, one after the other:
once under `rocprofv3 --kernel-trace --stats`, which gives the per-launch time of
corrective_smooth_kernel, corrective_bind_kernel and corrective_apply_kernel beside skin_lbs_kernel
and skin_dqs_kernel, and once plain, which gives the wall time of animate_mesh with
corrective_iterations 0 and 10 and of the ops (host clock around a call that ends in a synchronise;
the tracer slows the host, so these are not taken under it).  A smoothing launch
is compared with its compulsory traffic, 24 F V bytes (every vertex of every frame read and
written once as 3 f32), at the HBM rates of the MI355X.  The compiler's register / LDS / spill
figures of the three kernels come from tools/isa_stats.py.

    python tools/corrective_probe.py [--runs 10] [--frames 120] [--out profiles/corrective_probe.json]

This process starts the tracer with the worker after `--` and never opens the GPU itself.  The probe
needs a GPU: there is no fallback.
"""
import argparse
import csv
import importlib.util
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

KERNELS = ("corrective_smooth_kernel", "corrective_bind_kernel", "corrective_apply_kernel", "skin_lbs_kernel",
           "skin_dqs_kernel")
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29          # peak of the part; measured float4 copy


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_resources():
    isa = _tool("isa_stats")
    try:
        txt = isa.compile_asm(os.path.join(isa.CSRC, "mesh_corrective.hip"))
    except (SystemExit, OSError) as e:
        return {"unavailable": str(e)[:200]}
    md, out = isa.metadata(txt), {}
    for name, _ in isa.bodies(txt):
        short = isa.demangle_short(name)
        if short in KERNELS:
            m = md[name]
            out[short] = {"vgpr": m["vgpr"], "agpr": m["agpr"], "sgpr": m["sgpr"], "lds_bytes": m["lds"],
                          "scratch_bytes": m["scratch"], "vgpr_spills": m["vspill"], "sgpr_spills": m["sspill"],
                          "threads": 256}
    return out


def worker(a):
    import numpy as np
    import torch
    from drawingspinup_amd import animate, ops
    if not torch.cuda.is_available():
        raise SystemExit("corrective_probe needs a GPU")
    probe = _tool("skin_probe")
    dev = torch.device("cuda:0")
    v, f, sk = probe.character()
    clip = probe.swing(sk, a.frames)
    col = np.random.default_rng(1).random((len(v), 3)).astype(np.float32)
    infl, w = animate.bone_heat_weights(v, f, sk, device=dev)
    t0 = time.perf_counter()
    topo = animate.smoothing_topology(v, f)
    t_topo = (time.perf_counter() - t0) * 1e3
    tv = torch.from_numpy(v.astype(np.float32)).to(dev)
    ti, tw = torch.from_numpy(infl).to(dev), torch.from_numpy(w).to(dev)
    m64 = animate.skinning_matrices(sk, clip)
    mats = torch.from_numpy(m64.astype(np.float32)).to(dev)
    dq = torch.from_numpy(animate.dual_quaternions(m64)).to(dev)
    tt = ops.corrective_topology(topo, dev)
    t_lbs = probe.timed(lambda: ops.skin_lbs(tv, ti, tw, mats), a.runs)
    t_dqs = probe.timed(lambda: ops.skin_dqs(tv, ti, tw, dq), a.runs)
    skinned = ops.skin_lbs(tv, ti, tw, mats)
    t_bind = probe.timed(lambda: ops.corrective_bind(tv, tt, a.factor, a.iterations), a.runs)
    delta, valid = ops.corrective_bind(tv, tt, a.factor, a.iterations)
    t_smooth = probe.timed(lambda: ops.corrective_smooth(skinned, tt, delta, valid, a.factor, a.iterations), a.runs)
    out = ops.corrective_smooth(skinned, tt, delta, valid, a.factor, a.iterations)
    moved = (out - skinned).norm(dim=-1)
    n_all = max(2, a.runs // 3)
    t_off = probe.timed(lambda: animate.animate_mesh(v, f, col, sk, clip, weights=(infl, w), device=dev), n_all, warmup=1)
    t_on = probe.timed(lambda: animate.animate_mesh(v, f, col, sk, clip, weights=(infl, w), device=dev,
                                                    corrective_iterations=a.iterations, corrective_factor=a.factor),
                       n_all, warmup=1)
    res = {"mesh": "seeded tube character of tools/skin_probe.py", "verts": int(len(v)), "faces": int(len(f)),
           "frames": a.frames, "runs": a.runs, "iterations": a.iterations, "factor": a.factor,
           "representatives": int((topo["rep"] == np.arange(len(v))).sum()), "welded_faces": int(len(topo["faces"])),
           "neighbour_entries": int(topo["nbr_cols"].size), "corner_entries": int(topo["cor_faces"].size),
           "vertices_with_a_frame_at_bind": int(valid.sum().item()),
           "topology_host_ms": t_topo,
           "skin_lbs_ms": t_lbs, "skin_dqs_ms": t_dqs,
           "corrective_bind_ms": dict(t_bind, note="iterations smoothing launches on one frame + the bind launch"),
           "corrective_smooth_ms": dict(t_smooth, note="iterations smoothing launches + one apply, workspace allocation included"),
           "largest_displacement": float(moved.max().item()), "mean_displacement": float(moved.mean().item()),
           "animate_mesh_ms": {"corrective_iterations_0": t_off, "corrective_iterations_%d" % a.iterations: t_on,
                               "note": "weights given; host arrays in, uploads, topology and bind included"},
           "device": torch.cuda.get_device_name(0)}
    with open(a.worker, "w") as fh:
        json.dump(res, fh)


def read_trace(folder):
    ns = {k: [] for k in KERNELS}
    for dp, _, fs in os.walk(folder):
        for name in fs:
            if not name.endswith("kernel_trace.csv"):
                continue
            with open(os.path.join(dp, name), newline="") as fh:
                for row in csv.DictReader(fh):
                    for k in ns:
                        if k in row.get("Kernel_Name", ""):
                            ns[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]),
                                          int(row.get("Grid_Size_Y", row.get("Grid_Size", 0)) or 0)))
    missing = [k for k, x in ns.items() if not x]
    if missing:
        raise SystemExit(f"no launches of {missing} in the traces under {folder}")
    return ns


def summarise(ns, res):
    """Per-launch figures; the corrective kernels run on 1 frame (bind) and on all frames (smooth):
    only the launches over all frames are counted for the smoothing and apply kernels."""
    F, V = res["frames"], res["verts"]
    out = {}
    for k, rows in ns.items():
        if k in ("corrective_smooth_kernel", "corrective_apply_kernel"):
            # grid.y is the frame count (blockDim.y = 1); a trace without that column: by duration
            full = [r for r in rows if r[2] == F]
            longest = max(e - s for s, e, _ in rows)
            rows = full or [r for r in rows if (r[1] - r[0]) * 4 >= longest]
        d = [e - s for s, e, _ in rows]
        out[k] = {"median_us": statistics.median(d) / 1e3, "min_us": min(d) / 1e3, "max_us": max(d) / 1e3, "launches": len(d)}
    nbytes = 24 * F * V
    us = out["corrective_smooth_kernel"]["median_us"]
    out["smoothing_launch_vs_compulsory_traffic"] = {
        "bytes_per_launch": nbytes, "definition": "24 F V: 3 f32 read and 3 f32 written per (frame, vertex)",
        "us_at_hbm_copy_rate_%.2f_TBs" % HBM_COPY_TBS: nbytes / (HBM_COPY_TBS * 1e6),
        "us_at_hbm_spec_rate_%.1f_TBs" % HBM_SPEC_TBS: nbytes / (HBM_SPEC_TBS * 1e6),
        "measured_over_copy_rate_time": us / (nbytes / (HBM_COPY_TBS * 1e6)),
        "measured_over_spec_rate_time": us / (nbytes / (HBM_SPEC_TBS * 1e6)),
        "achieved_TBs_of_compulsory_bytes": nbytes / (us * 1e6)}
    out["note"] = "rocprofv3 --kernel-trace --stats of a worker run of its own; the other figures are from a plain run"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--factor", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corrective_probe.json"))
    ap.add_argument("--keep-trace", metavar="DIR", help="keep the tracer's output under DIR")
    ap.add_argument("--worker", metavar="JSON", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        raise SystemExit("rocprofv3 not found")
    tmp = a.keep_trace or tempfile.mkdtemp(prefix="corrective_probe_")
    os.makedirs(tmp, exist_ok=True)
    part = os.path.join(tmp, "worker.json")
    cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
           sys.executable, os.path.abspath(__file__), "--worker", part, "--frames", str(a.frames), "--runs", str(a.runs),
           "--iterations", str(a.iterations), "--factor", str(a.factor)]
    r = subprocess.run(cmd, cwd=ROOT)
    if r.returncode != 0 or not os.path.exists(part):
        raise SystemExit(f"the traced worker failed (exit {r.returncode})")
    # the wall times: the same worker without the tracer (this overwrites the traced run's figures)
    r = subprocess.run(cmd[cmd.index("--") + 1:], cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the plain worker failed (exit {r.returncode})")
    with open(part) as fh:
        res = json.load(fh)
    res["kernel_trace"] = summarise(read_trace(os.path.join(tmp, "trace")), res)
    res["kernels"] = kernel_resources()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not a.keep_trace:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
