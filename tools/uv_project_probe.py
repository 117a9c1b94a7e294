"""Measure the per-texel projection of the drawings into the atlas (dsu_uv_project,
csrc/uv_project_area.hip; nsr/uv.bake_drawings) at production size: the ~50 000-face probe mesh of tools/uv_probe.py, a
1024^2 atlas, 2048^2 drawings.  Records
  * the time of dsu_uv_project beside dsu_uv_bake's raster from the same run, two ways:
    `kernel_us` = the kernels' own durations from a `rocprofv3 --kernel-trace --stats` run of
    `--trace-launches N` (a run of its own, read back with --kernel-stats), and `call_ms` = device
    events around `--batch` back-to-back calls through the ops wrappers, per call, median of --runs
    after warm-up: that one includes the wrapper's allocations and Python and is an UPPER BOUND on
    the kernel time,
  * the front / back / fallback shares of the covered texels,
  * how many texels change class between the tolerances 0, 1e-5, 1e-4, 1e-3,
  * device against tests/uv_project_ref.py on the tests' cases: differing texels, fragile texels.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/uv_project_probe.py --trace-launches 30
    python tools/uv_project_probe.py [--size 1024] [--res 2048] [--kernel-stats DIR]
                                     [--out profiles/uv_project_probe.json]

Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402
from drawingspinup_amd.nsr.mesh_post import projection_masks  # noqa: E402
from uv_probe import character  # noqa: E402

TOLERANCES = (0.0, 1e-5, 1e-4, 1e-3)
PROJECT_KERNEL = "uv_project_area_kernel<true>"         # what dsu_uv_project launches


def timed_batch(fn, runs, batch, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / batch)
    return statistics.median(ms), min(ms), max(ms)


def kernel_stats(folder):
    """The rows of dsu_uv_project's kernel (the one-point instantiation of uv_project_area_kernel) and of
    uv_raster_kernel in rocprofv3's kernel statistics under `folder`, microseconds."""
    import csv
    import glob
    out = {}
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(path)):
            for key in (PROJECT_KERNEL, "uv_raster_kernel"):
                if key in row.get("Name", ""):
                    out[key] = {"calls": int(row["Calls"]), "mean": float(row["AverageNs"]) / 1e3,
                                "min": float(row["MinNs"]) / 1e3, "max": float(row["MaxNs"]) / 1e3}
    if len(out) != 2:
        raise SystemExit(f"--kernel-stats {folder}: no *kernel_stats.csv there with Name / Calls / AverageNs / MinNs / "
                         f"MaxNs rows of both kernels (found {sorted(out)})")
    return out


def accuracy(dev):
    import uv_project_ref as P
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    out = {}
    for name, size, tol in [c + (P.Z_TOL,) for c in P.CASES] + [("torus", 256, 0.0)]:
        c = P.case(name, size, tol)
        img, src = ops.uv_project(t(c["uvs"], np.float32), t(c["indices"], np.int32), t(c["positions"], np.float32),
                                  t(c["face_id"], np.int32), t(c["color_front"]), t(c["mask_front"]),
                                  t(c["color_back"]), t(c["mask_back"]), tol)
        img, src = img.cpu().numpy(), src.cpu().numpy()
        out[f"{name}_{size}_tol{tol:g}"] = {
            "source_differ": int((src != c["source"]).sum()),
            "image_texels_differ": int((img != c["image"]).any(-1).sum()),
            "fragile_texels": int(c["fragile"].sum()), "texels": size * size,
            "front": int((c["source"] == 1).sum()), "back": int((c["source"] == 2).sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--gutter", type=int, default=2)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--trace-launches", type=int, default=0,
                    help="only launch the two kernels this often and exit (the run rocprofv3 traces)")
    ap.add_argument("--kernel-stats", default=None, help="folder of that rocprofv3 run's csv output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_project_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    verts, faces, colours = character()
    S, res = args.size, args.res
    # the probe mesh inside the projection frame; its faces wound outward (the facing test reads the winding)
    v = verts.astype(np.float64)
    v = (v - 0.5 * (v.min(0) + v.max(0))) * (0.9 / (v.max(0) - v.min(0)).max())
    tri = v[faces]
    if np.einsum("ij,ij->", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])) < 0:
        v = v * np.array([1.0, 1.0, -1.0])
    frame = v.astype(np.float32)
    vm, ind, uvs = U.parametrize(frame, faces, S, args.gutter, device=dev)

    duv, dind = torch.from_numpy(uvs).to(dev), torch.from_numpy(ind.astype(np.int32)).to(dev)
    dpos = torch.from_numpy(frame[vm]).to(dev)
    dcol = torch.from_numpy(colours[vm]).to(dev)
    plan = ops.UvBakePlan(duv, dind, S).bin()
    _, fid, _ = plan.raster(dcol)
    rng = np.random.default_rng(0)
    cf = torch.from_numpy(rng.integers(0, 256, (res, res, 3), dtype=np.uint8)).to(dev)
    cb = torch.from_numpy(rng.integers(0, 256, (res, res, 3), dtype=np.uint8)).to(dev)
    full = torch.full((res, res), 255, dtype=torch.uint8, device=dev)
    front, back = projection_masks(dpos, dind.long(), full, res=res, ksize=19)
    tris = dpos[dind.long()].contiguous()
    xy = tris[..., :2].reshape(-1, 2)
    grid = ops.ZGrid(tris, xy.amin(0).tolist(), xy.amax(0).tolist())
    cells = (grid.offsets[1:] - grid.offsets[:-1]).float()

    project = lambda tol=U.Z_TOLERANCE: ops.uv_project(duv, dind, dpos, fid, cf, front, cb, back, tol, grid=grid)
    if args.trace_launches:
        for _ in range(args.trace_launches):
            project()
            plan.raster(dcol)
        torch.cuda.synchronize()
        return
    covered = (fid >= 0)
    n_cov = int(covered.sum())
    classes = {tol: project(tol)[1] for tol in TOLERANCES}
    src = classes[U.Z_TOLERANCE]
    sweep = {}
    for a, b in zip(TOLERANCES[:-1], TOLERANCES[1:]):
        sweep[f"{a:g}->{b:g}"] = {"changed": int((classes[a] != classes[b]).sum()),
                                 "gained": int(((classes[a] == 0) & (classes[b] > 0)).sum()),
                                 "lost": int(((classes[a] > 0) & (classes[b] == 0)).sum())}
    again = project()
    ms_project = timed_batch(project, args.runs, args.batch)
    ms_raster = timed_batch(lambda: plan.raster(dcol), args.runs, args.batch)
    res_json = {
        "device": torch.cuda.get_device_name(0), "faces": int(len(faces)), "new_vertices": int(len(vm)),
        "size": S, "drawing_res": res, "z_tolerance": U.Z_TOLERANCE, "erode": 19,
        "covered_texels": n_cov, "atlas_fill": n_cov / float(S * S),
        "grid_cells_per_axis": int(grid.g), "triangles_per_cell_mean": float(cells.mean()),
        "triangles_per_cell_max": int(cells.max()),
        "kernel_us": kernel_stats(args.kernel_stats) if args.kernel_stats else None,
        "kernel_us_source": "rocprofv3 --kernel-trace --stats over a run of --trace-launches (null: not collected)",
        "call_ms": {"uv_project": ms_project, "uv_bake_raster": ms_raster},
        "call_ms_is": "device events around `batch` back-to-back calls of the ops wrapper, per call: median, min, "
                      "max of `runs`; includes allocation and Python per call: an upper bound on the kernel time",
        "runs": args.runs, "batch": args.batch,
        "shares_of_covered": {"front": float((src == 1).sum()) / max(n_cov, 1),
                              "back": float((src == 2).sum()) / max(n_cov, 1),
                              "fallback": float(((src == 0) & covered).sum()) / max(n_cov, 1)},
        "tolerance_sweep": sweep,
        "repeat_is_bit_identical": bool(torch.equal(again[0], project()[0]) and torch.equal(again[1], src)),
        "accuracy": accuracy(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res_json, fh, indent=1)
    print(json.dumps(res_json))


if __name__ == "__main__":
    main()
