"""Measure the thickness map (dsu_mesh_thickness_ortho, csrc/mesh_thickness.hip) at production size:
the 51 200-face probe mesh of tools/uv_probe.py on the 512^2 lattice animate.lift_marks lays over it.
Records
  * the kernel's time beside that of dsu_uv_project's kernel (tools/uv_project_probe.py's setting: 1024^2
    atlas, 2048^2 drawings) from ONE `rocprofv3 --kernel-trace --stats` run of `--trace-launches N`, no
    counters, read back with --kernel-stats,
  * the histogram of crossings per sample, the triangles per grid cell, the share of samples inside,
  * device against the host entry: samples that differ (0 expected),
  * the wall time of animate.lift_marks for 16 marks (median of --runs after a warm-up; it includes
    the binning, the copy back and the host part).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/thickness_probe.py --trace-launches 30
    python tools/thickness_probe.py [--kernel-stats DIR] [--out profiles/thickness_probe.json]

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

from drawingspinup_amd import animate, ops  # noqa: E402
from drawingspinup_amd.animate import rig  # noqa: E402
from uv_probe import character  # noqa: E402

KERNELS = ("mesh_thickness_kernel", "uv_project_area_kernel<true>")   # the latter: what dsu_uv_project launches


def kernel_stats(folder):
    """The rows of the two kernels in rocprofv3's kernel statistics under `folder`, microseconds."""
    import csv
    import glob
    out = {}
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(path)):
            for key in KERNELS:
                if key in row.get("Name", ""):
                    out[key] = {"calls": int(row["Calls"]), "mean": float(row["AverageNs"]) / 1e3,
                                "min": float(row["MinNs"]) / 1e3, "max": float(row["MaxNs"]) / 1e3}
    if len(out) != len(KERNELS):
        raise SystemExit(f"--kernel-stats {folder}: no *kernel_stats.csv there with rows of {KERNELS} (found {sorted(out)})")
    return out


def uv_project_call(dev, verts, faces, colours, size=1024, res=2048):
    """dsu_uv_project as tools/uv_project_probe.py sets it up, as a callable."""
    from drawingspinup_amd.nsr import uv as U
    from drawingspinup_amd.nsr.mesh_post import projection_masks
    v = verts.astype(np.float64)
    v = (v - 0.5 * (v.min(0) + v.max(0))) * (0.9 / (v.max(0) - v.min(0)).max())
    tri = v[faces]
    if np.einsum("ij,ij->", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])) < 0:
        v = v * np.array([1.0, 1.0, -1.0])
    frame = v.astype(np.float32)
    vm, ind, uvs = U.parametrize(frame, faces, size, 2, device=dev)
    duv, dind = torch.from_numpy(uvs).to(dev), torch.from_numpy(ind.astype(np.int32)).to(dev)
    dpos, dcol = torch.from_numpy(frame[vm]).to(dev), torch.from_numpy(colours[vm]).to(dev)
    _, fid, _ = ops.UvBakePlan(duv, dind, size).bin().raster(dcol)
    rng = np.random.default_rng(0)
    cf = torch.from_numpy(rng.integers(0, 256, (res, res, 3), dtype=np.uint8)).to(dev)
    cb = torch.from_numpy(rng.integers(0, 256, (res, res, 3), dtype=np.uint8)).to(dev)
    full = torch.full((res, res), 255, dtype=torch.uint8, device=dev)
    front, back = projection_masks(dpos, dind.long(), full, res=res, ksize=19)
    tris = dpos[dind.long()].contiguous()
    xy = tris[..., :2].reshape(-1, 2)
    grid = ops.ZGrid(tris, xy.amin(0).tolist(), xy.amax(0).tolist())
    return lambda: ops.uv_project(duv, dind, dpos, fid, cf, front, cb, back, U.Z_TOLERANCE, grid=grid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--trace-launches", type=int, default=0,
                    help="only launch the two kernels this often and exit (the run rocprofv3 traces)")
    ap.add_argument("--kernel-stats", default=None, help="folder of that rocprofv3 run's csv output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thickness_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    verts, faces, colours = character()
    lat = rig.thickness_lattice(verts, args.lattice)
    dv, df = torch.from_numpy(verts).to(dev), torch.from_numpy(faces.astype(np.int32)).to(dev)
    thickness = lambda: ops.mesh_thickness(dv, df, *lat)
    if args.trace_launches:
        project = uv_project_call(dev, verts, faces, colours)
        for _ in range(args.trace_launches):
            thickness()
            project()
        torch.cuda.synchronize()
        return
    mid, thick, count = (t.cpu().numpy() for t in thickness())
    again = thickness()
    host = ops.mesh_thickness_host(verts, faces, *lat)
    differ = {k: int((a != b).sum()) for k, a, b in zip(("mid", "thickness", "count"), (mid, thick, count), host)}
    # the grid the wrapper bins on: cells of 16 x 16 samples
    x0, y0, h, W, H = lat
    g = -(-max(W, H) // ops.THICKNESS_TILE)
    span = g * ops.THICKNESS_TILE * h
    grid = ops.ZGrid(dv[df.long()].contiguous(), (x0, y0), (x0 + span, y0 + span), cells_per_axis=g)
    cells = (grid.offsets[1:] - grid.offsets[:-1]).float()
    # 16 marks on samples inside the mesh, spread over them; a chain of joints
    inside = np.argwhere(thick > 0.0)
    pick = inside[np.linspace(0, len(inside) - 1, 16).astype(np.int64)]
    marks = np.stack([x0 + (pick[:, 1] + 0.5) * h, y0 + (pick[:, 0] + 0.5) * h], 1)
    names, parents = [f"j{i}" for i in range(16)], np.arange(-1, 15)
    lift = lambda: animate.lift_marks(names, parents, marks, verts, faces, lattice=args.lattice, device=dev)
    lift()
    wall = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lift()
        wall.append((time.perf_counter() - t0) * 1e3)
    values, n = np.unique(count, return_counts=True)
    res_json = {
        "device": torch.cuda.get_device_name(0), "faces": int(len(faces)), "vertices": int(len(verts)),
        "lattice": [int(W), int(H)], "h": h,
        "kernel_us": kernel_stats(args.kernel_stats) if args.kernel_stats else None,
        "kernel_us_source": "one rocprofv3 --kernel-trace --stats run of --trace-launches, no counters (null: not collected)",
        "crossings_histogram": {int(k): int(c) for k, c in zip(values, n)},
        "samples_inside": int((thick > 0.0).sum()), "samples": int(W * H),
        "grid_cells_per_axis": int(g), "triangles_per_cell_mean": float(cells.mean()),
        "triangles_per_cell_max": int(cells.max()),
        "samples_that_differ_from_the_host_entry": differ,
        "repeat_is_bit_identical": bool(all(torch.equal(a, torch.from_numpy(b).to(dev))
                                            for a, b in zip(again, (mid, thick, count)))),
        "lift_marks_16_wall_ms": {"median": statistics.median(wall), "min": min(wall), "max": max(wall),
                                  "runs": args.runs},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res_json, fh, indent=1)
    print(json.dumps(res_json))


if __name__ == "__main__":
    main()
