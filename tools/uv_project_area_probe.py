"""Measure the area-sampled projection of the drawings (dsu_uv_project_area,
csrc/uv_project_area.hip; nsr/uv.bake_drawings(samples=, pixel_filter=)) at production size: mesh,
atlas and drawings as tools/uv_project_probe.py has them (the ~50 000-face probe mesh, a 1024^2
atlas, 2048^2 drawings).  Records
  * `kernel_us`: the kernel's own durations from ONE `rocprofv3 --kernel-trace --stats` run of
    `--trace-launches N` (no counters): ops.uv_project, the yardstick, on the grid it builds for
    itself, and ops.uv_project_area at s = 1, 2, 4 under both filters on the finer grid it builds
    (--cells overrides it).  All are instantiations of uv_project_area_kernel (s = 1 the one-point
    one, which is also what ops.uv_project launches), so the dispatches are told apart by their
    order in the kernel trace (N of each, ops.uv_project first, then in the order of CONFIGS), and
    `ratio_to_uv_project` = mean / ops.uv_project's mean of the same run,
  * per configuration: count / s^2 over the projected texels, texels gained over s = 1,
  * the standard deviation of the projected texels' blue channel at s = 1, 2, 4 for drawings whose
    blue channel is a one-pixel checker (what aliasing leaves of a pattern a texel cannot hold),
  * the wall time of bake_drawings at s = 1 and s = 4 (bilinear), median of --runs.
Nothing here is asserted.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/uv_project_area_probe.py --trace-launches 30
    python tools/uv_project_area_probe.py [--kernel-trace DIR] [--out profiles/uv_project_area_probe.json]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402
from drawingspinup_amd.nsr.mesh_post import projection_masks  # noqa: E402
from uv_probe import character  # noqa: E402

CONFIGS = [(s, f) for s in (1, 2, 4) for f in ("nearest", "bilinear")]


def kernel_trace(folder, launches):
    """Durations (us) from the kernel trace under `folder`: the dispatches of uv_project_area_kernel in
    start order, `launches` of ops.uv_project on the grid it builds for itself, then `launches` per
    configuration."""
    import csv
    import glob
    found = []
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)):
        for row in csv.DictReader(open(path)):
            if "uv_project_area_kernel" in row.get("Kernel_Name", ""):
                t0, t1 = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                found.append((t0, (t1 - t0) / 1e3))
    if len(found) != launches * (1 + len(CONFIGS)):
        raise SystemExit(f"--kernel-trace {folder}: expected {launches * (1 + len(CONFIGS))} dispatches of "
                         f"uv_project_area_kernel, found {len(found)}")
    row = lambda d: {"calls": len(d), "mean": statistics.mean(d), "min": min(d), "max": max(d)}
    found = [d for _, d in sorted(found)]
    out = {"uv_project": row(found[:launches])}
    for k, (s, f) in enumerate(CONFIGS):
        r = row(found[(k + 1) * launches:(k + 2) * launches])
        r["ratio_to_uv_project"] = r["mean"] / out["uv_project"]["mean"]
        out[f"uv_project_area s={s} {f}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--gutter", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace-launches", type=int, default=0,
                    help="only launch the kernels this often each and exit (the run rocprofv3 traces)")
    ap.add_argument("--kernel-trace", default=None, help="folder of that rocprofv3 run's csv output")
    ap.add_argument("--traced-launches", type=int, default=30, help="the --trace-launches of the traced run")
    ap.add_argument("--cells", type=int, default=None,
                    help="cells per axis of the z-grid (default: what ops.uv_project_area builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_project_area_probe.json"))
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
    _, fid, _ = ops.UvBakePlan(duv, dind, S).bin().raster(dcol)
    # r = column, g = row, b = a one-pixel checker (tests/uv_project_ref.drawings at this resolution)
    row, col = torch.meshgrid(torch.arange(res, device=dev), torch.arange(res, device=dev), indexing="ij")
    cf = torch.stack([col % 256, row % 256, 255 * ((row + col) & 1)], -1).to(torch.uint8).contiguous()
    cb = cf[..., [2, 0, 1]].contiguous()
    full = torch.full((res, res), 255, dtype=torch.uint8, device=dev)
    front, back = projection_masks(dpos, dind.long(), full, res=res, ksize=19)
    tris = dpos[dind.long()].contiguous()
    xy = tris[..., :2].reshape(-1, 2)
    grid = ops.ZGrid(tris, xy.amin(0).tolist(), xy.amax(0).tolist(),
                     cells_per_axis=args.cells or ops.uv_area_cells(len(faces)))

    own = ops.ZGrid(tris, xy.amin(0).tolist(), xy.amax(0).tolist())          # what ops.uv_project builds
    one = lambda: ops.uv_project(duv, dind, dpos, fid, cf, front, cb, back, U.Z_TOLERANCE, grid=own)
    area = lambda s, f: ops.uv_project_area(duv, dind, dpos, fid, cf, front, cb, back, U.Z_TOLERANCE, s, f, grid=grid)
    if args.trace_launches:
        for _ in range(args.trace_launches):
            one()
        for s, f in CONFIGS:
            for _ in range(args.trace_launches):
                area(s, f)
        torch.cuda.synchronize()
        return
    covered = fid >= 0
    base_src = one()[1]
    quality = {}
    for s, f in CONFIGS:
        img, src, cnt = area(s, f)
        on = src > 0
        blue = img[..., 2][on].double()
        # the back drawing carries the checker in its red channel (the channels are permuted)
        chk = torch.where(src == 1, img[..., 2], img[..., 0])[on].double()
        quality[f"s={s} {f}"] = {
            "projected_texels": int(on.sum()),
            "gained_over_s1": int((on & (base_src == 0)).sum()),
            "lost_against_s1": int(((base_src > 0) & ~on).sum()),
            "mean_count_over_s2": float(cnt[on].double().mean()) / (s * s),
            "own_point_texels": int((on & (cnt == 0)).sum()),
            "blue_std_projected": float(blue.std()),
            "checker_channel_std_projected": float(chk.std())}
    fallback = colours[vm]

    def bake(s, f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        U.bake_drawings(uvs, ind, frame[vm], cf, full, cb, fallback, S, args.gutter, device=dev, samples=s, pixel_filter=f)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    wall = {}
    for s, f in ((1, "nearest"), (4, "bilinear")):
        bake(s, f)
        ms = [bake(s, f) for _ in range(args.runs)]
        wall[f"s={s} {f}"] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
    res_json = {
        "device": torch.cuda.get_device_name(0), "faces": int(len(faces)), "size": S, "drawing_res": res,
        "z_tolerance": U.Z_TOLERANCE, "erode": 19, "covered_texels": int(covered.sum()),
        "grid_cells_per_axis": int(grid.g), "uv_project_grid_cells_per_axis": int(own.g),
        "kernel_us": kernel_trace(args.kernel_trace, args.traced_launches) if args.kernel_trace else None,
        "kernel_us_source": "one rocprofv3 --kernel-trace --stats run of --trace-launches, no counters; the "
                            "kernel's dispatches split by start order (null: not collected)",
        "quality": quality,
        "bake_drawings_wall_ms": wall,
        "bake_drawings_wall_ms_is": "perf_counter around one bake_drawings call (mask preparation, uploads, raster, "
                                    "projection, gutter fill, download), synchronised; median, min, max of `runs`",
        "runs": args.runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res_json, fh, indent=1)
    print(json.dumps(res_json))


if __name__ == "__main__":
    main()
