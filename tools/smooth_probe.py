"""Kernel time of the export smoothing (csrc/mesh_smooth.hip) on the band of a 512^3 volume: the
band compacted voxel by voxel (`layout="slots"`: smooth_fused_kernel) against the band compacted in
8^3 bricks (smooth_brick_kernel), from `rocprofv3 --kernel-trace --stats` runs of a worker process.

    python tools/smooth_probe.py [--n 512] [--iters 30] [--out profiles/smooth_bricks_probe.json]

Arms alternate slots, bricks, slots, bricks: one profiled worker process each.  A brick arm runs the
iteration three ways on the same band — staged in LDS with byte-coded bounds, staged in LDS with the
distances stored as doubles, and with direct loads — so that each comparison is within one process;
the comparison of the layouts is between neighbouring arms of one invocation.  Recorded: band voxels,
active bricks, fill; median / min / max per kernel; the energy pass; the set-up of each layout
(device events around the build, and the summed time of the brick build kernels).  Needs a GPU and
rocprofv3: there is no fallback.
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
ROOT = os.path.dirname(HERE)

KERNELS = {
    "slots/iterate": ["smooth_fused_kernel"],
    "slots/energy_rows": ["smooth_rows_kernel"],
    "slots/energy_sum": ["smooth_energy_kernel"],
    "bricks/iterate_lds_coded": ["smooth_brick_kernel<true,false,"],
    "bricks/iterate_lds_stored": ["smooth_brick_kernel<false,false,"],
    "bricks/iterate_direct_coded": ["smooth_brick_kernel<true,true,"],
    "bricks/iterate_direct_stored": ["smooth_brick_kernel<false,true,"],
    "bricks/energy": ["smooth_brick_energy_kernel"],
    "bricks/build_flags": ["brick_flag_kernel"],
    "bricks/build_gather": ["brick_gather_kernel"],
    "bricks/write_back": ["brick_scatter_kernel"],
}


def volume(n, dev):
    """The solid of tests/test_gpu_mesh.py::_shape at n^3, formed on the device."""
    import torch
    c = torch.linspace(-1, 1, n, device=dev)
    x, y, z = c.view(n, 1, 1), c.view(1, n, 1), c.view(1, 1, n)
    return ((x / 0.7) ** 2 + (y / 0.5) ** 2 + (z / 0.6) ** 2 <= 1.0) | \
        ((x - 0.3).abs() + y.abs() + z.abs() < 0.35)


def worker(arm, n, iters):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from drawingspinup_amd import ops
    from drawingspinup_amd.nsr import mesh as M
    if not torch.cuda.is_available():
        raise SystemExit("smooth_probe needs a GPU")
    dev = torch.device("cuda:0")
    dist, band = M.signed_distance_band_device(volume(n, dev), 5.0, 4.0)
    values = torch.from_numpy(np.unique(M._band_tables(5.0, 4.0)[1]))
    info = {"arm": arm, "n": n, "iters": iters, "band_voxels": int(band.sum())}

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    if arm == "slots":
        def build():
            flat, nbr_slots, x, lower, upper = M._slot_layout(dist, band)
            nv = x.shape[0]
            return (flat, torch.stack(nbr_slots).contiguous(), x.contiguous(), lower.contiguous(),
                    upper.contiguous(), torch.empty(3 * nv, dtype=torch.float64, device=dev))
        build()                                                     # warm the allocator and torch's kernels
        (flat, nbr_t, x, lower, upper, ybuf), info["setup_ms"] = timed(build)
        ops.smooth_iterate(nbr_t, lower, upper, x, ybuf, 0.5, 2)
        _, ms = timed(lambda: ops.smooth_iterate(nbr_t, lower, upper, x, ybuf, 0.5, iters))
        info["iterate_event_ms_per_iteration"] = ms / iters
        info["energy"] = [float(ops.smooth_energy(nbr_t, x, ybuf)) for _ in range(3)][-1]
        _, info["write_back_ms"] = timed(lambda: dist.view(-1).__setitem__(flat, x))
    else:
        ops.smooth_bricks_build(band, dist, values)                 # warm
        coded, info["setup_coded_ms"] = timed(lambda: ops.smooth_bricks_build(band, dist, values))
        stored, info["setup_stored_ms"] = timed(lambda: ops.smooth_bricks_build(band, dist, None))
        assert coded.code is not None and stored.x0 is not None
        info.update(active_bricks=coded.nb, brick_voxels=coded.nb * 512,
                    fill=info["band_voxels"] / (coded.nb * 512))
        for label, s, direct in (("lds_coded", coded, False), ("lds_stored", stored, False),
                                 ("direct_coded", coded, True)):
            ops.smooth_bricks_iterate(s, 0.5, 2, direct)
            _, ms = timed(lambda: ops.smooth_bricks_iterate(s, 0.5, iters, direct))
            info[f"iterate_{label}_event_ms_per_iteration"] = ms / iters
        info["energy"] = [float(ops.smooth_bricks_energy(stored)) for _ in range(3)][-1]
        _, info["write_back_ms"] = timed(lambda: ops.smooth_bricks_scatter(stored, dist))
    print("PROBE_INFO " + json.dumps(info))


def durations(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    out = {k: [] for k in KERNELS}
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"].replace(" ", "")
                us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                for label, needles in KERNELS.items():
                    if any(nd in name for nd in needles):
                        out[label].append(us)
    return out


def summary(us):
    return {"launches": len(us), "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def run_arm(arm, n, iters, keep):
    trace = tempfile.mkdtemp(prefix="smooth_probe_", dir=keep)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    cmd = [rocprof, "--kernel-trace", "--stats", "-f", "csv", "-d", trace, "--", sys.executable,
           os.path.abspath(__file__), "--worker", arm, "--n", str(n), "--iters", str(iters)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"the profiled worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    info = [json.loads(ln[len("PROBE_INFO "):]) for ln in r.stdout.splitlines() if ln.startswith("PROBE_INFO ")]
    res = {k: summary(v) for k, v in durations(trace).items() if v}
    shutil.rmtree(trace, ignore_errors=True)
    return {"arm": arm, "info": info[0], "kernels": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, choices=["slots", "bricks"])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bricks_probe.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.n, a.iters)
    keep = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(keep, exist_ok=True)
    runs = []
    for arm in ("slots", "bricks", "slots", "bricks"):
        runs.append(run_arm(arm, a.n, a.iters, keep))
        print(json.dumps(runs[-1]), flush=True)
    med = lambda arm, k: [r["kernels"][k]["median_us"] for r in runs if r["arm"] == arm and k in r["kernels"]]
    slots, bricks = med("slots", "slots/iterate"), med("bricks", "bricks/iterate_lds_coded")
    b = [r["info"] for r in runs if r["arm"] == "bricks"]
    out = {"volume": f"_shape({a.n})", "iterations_per_variant": a.iters,
           "band_voxels": b[0]["band_voxels"], "active_bricks": b[0]["active_bricks"], "fill": b[0]["fill"],
           "iterate_median_us": {"slots": slots, "bricks_lds_coded": bricks,
                                 "bricks_lds_stored": med("bricks", "bricks/iterate_lds_stored"),
                                 "bricks_direct_coded": med("bricks", "bricks/iterate_direct_coded")},
           "slots_over_bricks_neighbouring_arms": [s / k for s, k in zip(slots, bricks)],
           "energy_pass_median_us": {
               "slots": [x + y for x, y in zip(med("slots", "slots/energy_rows"), med("slots", "slots/energy_sum"))],
               "bricks": med("bricks", "bricks/energy")},
           "setup_event_ms": {"slots": [r["info"]["setup_ms"] for r in runs if r["arm"] == "slots"],
                              "bricks_coded": [i["setup_coded_ms"] for i in b],
                              "bricks_stored": [i["setup_stored_ms"] for i in b]},
           "write_back_event_ms": {"slots": [r["info"]["write_back_ms"] for r in runs if r["arm"] == "slots"],
                                   "bricks": [i["write_back_ms"] for i in b]},
           "runs": runs}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))


if __name__ == "__main__":
    main()
