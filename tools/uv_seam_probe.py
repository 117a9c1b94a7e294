"""Measure seam levelling in the atlas (dsu_uv_seam_gather / dsu_uv_seam_apply, csrc/mesh_uv.hip;
nsr/uv.bake_drawings(seam="level")) at production size: the ~50 000-face probe mesh of
tools/uv_project_probe.py, a 1024^2 atlas, 2048^2 drawings.  The drawings are a smooth function of
the surface point (the same one in both views); the fallback is the vertex bake of that function
scaled by 0.8 and shifted by 10 levels: the tone difference levelling is for.  Records
  * `kernel_us`: the two kernels' own durations beside dsu_uv_project's kernel from one
    `rocprofv3 --kernel-trace --stats` run of `--trace-launches N` (read back with --kernel-stats),
  * the CG iteration count and the counts of known and unknown groups,
  * the wall time of bake_drawings with and without levelling (host clock around the whole call,
    synchronised; median of --runs),
  * the seam step — the mean |a - b| over 4-neighbour texel pairs inside one chart, one projected and
    the other not — before and after.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/uv_seam_probe.py --trace-launches 30
    python tools/uv_seam_probe.py [--size 1024] [--res 2048] [--kernel-stats DIR]
                                  [--out profiles/uv_seam_probe.json]

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

from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402
from uv_probe import character  # noqa: E402

KERNELS = ("uv_seam_gather_kernel", "uv_seam_apply_kernel", "uv_project_area_kernel<true>")   # dsu_uv_project's
# tools/isa_stats.py drawingspinup_amd/csrc/mesh_uv.hip --filter uv_seam (static, from the code object's metadata)
ISA = {"uv_seam_gather_kernel": {"vgpr": 40, "scratch": 0, "lds": 37120},
       "uv_seam_apply_kernel": {"vgpr": 48, "scratch": 0, "lds": 0}}


def tone(x, y):
    """(...,3) in [0.05, 0.95]: the drawings' colour at the frame point (x, y), smooth."""
    return np.stack([0.5 + 0.25 * np.sin(6.0 * x) + 0.2 * np.cos(5.0 * y),
                     0.5 + 0.3 * np.sin(4.0 * y + 1.0) * np.cos(3.0 * x),
                     0.5 + 0.45 * np.sin(2.0 * x + 3.0 * y)], -1)


def kernel_stats(folder):
    """The rows of the three kernels in rocprofv3's kernel statistics under `folder`, microseconds."""
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
        raise SystemExit(f"--kernel-stats {folder}: no *kernel_stats.csv there with rows of all of {KERNELS} "
                         f"(found {sorted(out)})")
    return out


def seam_step(image, source, face_id, face_chart):
    img = np.asarray(image).astype(np.float64)
    fid = np.asarray(face_id, np.int64)
    chart = np.where(fid >= 0, np.asarray(face_chart, np.int64)[np.where(fid >= 0, fid, 0)], -1)
    on = np.asarray(source) != 0
    total, n = 0.0, 0
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        pair = (chart[a] >= 0) & (chart[a] == chart[b]) & (on[a] != on[b])
        total += float(np.abs(img[a] - img[b])[pair].sum())
        n += int(pair.sum())
    return total / max(3 * n, 1), n


def wall(fn, runs):
    fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--gutter", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace-launches", type=int, default=0,
                    help="only launch the three kernels this often and exit (the run rocprofv3 traces)")
    ap.add_argument("--kernel-stats", default=None, help="folder of that rocprofv3 run's csv output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_seam_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    verts, faces, _ = character()
    S, res = args.size, args.res
    # the probe mesh inside the projection frame; its faces wound outward (the facing test reads the winding)
    v = verts.astype(np.float64)
    v = (v - 0.5 * (v.min(0) + v.max(0))) * (0.9 / (v.max(0) - v.min(0)).max())
    tri = v[faces]
    if np.einsum("ij,ij->", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])) < 0:
        v = v * np.array([1.0, 1.0, -1.0])
    frame = v.astype(np.float32)
    vm, ind, uvs, info = U.parametrize(frame, faces, S, args.gutter, device=dev, return_info=True)
    groups, group_faces = U.seam_groups(frame, faces, vm)

    # front pixel (X, Y) shows the frame point (X / span - 1/2, 1/2 - Y / span); the back view is mirrored in x
    span = float(res - 1)
    Y, X = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    front = np.rint(tone(X / span - 0.5, 0.5 - Y / span) * 255.0).astype(np.uint8)
    cf = torch.from_numpy(front).to(dev)
    cb = torch.from_numpy(np.ascontiguousarray(front[:, ::-1])).to(dev)
    full = torch.full((res, res), 255, dtype=torch.uint8, device=dev)
    fallback_colours = (0.8 * tone(frame[vm, 0].astype(np.float64), frame[vm, 1].astype(np.float64)) + 10.0 / 255.0)
    fallback_colours = fallback_colours.astype(np.float32)

    be = U.DeviceBackend(dev)
    fallback, fid, _ = be.bake(uvs, ind, fallback_colours, S)
    proj, src = be.project(uvs, ind, frame[vm], fid, cf, full, cb, U.Z_TOLERANCE, 19)
    G = int(groups.max()) + 1
    duv, dind, dgrp = be._seam_atlas(uvs, ind, groups)
    gather = lambda: ops.uv_seam_gather(duv, dind, dgrp, fid, src, proj, fallback, G)
    num, den = gather()
    d, known = U.seam_offsets(num, den, group_faces, be)
    dd = torch.from_numpy(d).to(dev)
    apply = lambda: ops.uv_seam_apply(duv, dind, dgrp, fid, src, proj, fallback, dd)
    if args.trace_launches:
        tris = torch.from_numpy(frame[vm]).to(dev)[dind.long()].contiguous()
        xy = tris[..., :2].reshape(-1, 2)
        grid = ops.ZGrid(tris, xy.amin(0).tolist(), xy.amax(0).tolist())
        from drawingspinup_amd.nsr.mesh_post import projection_masks
        dpos = torch.from_numpy(frame[vm]).to(dev)
        mf, mb = projection_masks(dpos, dind.long(), full, res=res, ksize=19)
        for _ in range(args.trace_launches):
            ops.uv_project(duv, dind, dpos, fid, cf, mf, cb, mb, U.Z_TOLERANCE, grid=grid)
            gather()
            apply()
        torch.cuda.synchronize()
        return
    levelled = apply()
    again = gather()
    covered = fid >= 0
    hard = torch.where((src > 0)[..., None], proj, fallback)
    chart = info["face_chart"]
    to = lambda a: a.cpu().numpy()
    before = seam_step(to(hard), to(src), to(fid), chart)
    after = seam_step(to(levelled), to(src), to(fid), chart)
    bake = lambda seam: U.bake_drawings(uvs, ind, frame[vm], cf, full, cb, fallback_colours, S, args.gutter, device=dev,
                                        seam=seam, groups=groups, group_faces=group_faces)
    n_cov = int(covered.sum())
    res_json = {
        "device": torch.cuda.get_device_name(0), "faces": int(len(faces)), "new_vertices": int(len(vm)),
        "size": S, "drawing_res": res, "erode": 19, "covered_texels": n_cov,
        "projected_share_of_covered": float(((src > 0) & covered).sum()) / max(n_cov, 1),
        "groups": G, "known_groups": int(known.sum()), "unknown_groups": int((~known).sum()),
        "groups_with_sliver_weight": int(((to(den) > 0) & (to(den) < U.SEAM_MIN_WEIGHT)).sum()),
        "cg_iterations": int(getattr(be, "seam_iterations", 0)), "cg_tol": U.SEAM_TOL,
        "offset_range": [float(d.min()), float(d.max())],
        "kernel_us": kernel_stats(args.kernel_stats) if args.kernel_stats else None,
        "kernel_us_source": "rocprofv3 --kernel-trace --stats over a run of --trace-launches (null: not collected)",
        "isa": ISA,
        "bake_drawings_wall_ms": {"none": wall(lambda: bake("none"), args.runs),
                                  "level": wall(lambda: bake("level"), args.runs)},
        "bake_drawings_wall_ms_is": "host clock around the whole call (uploads, raster, mask preparation, projection, "
                                    "composition, gutter fill, download), synchronised: median, min, max of `runs`",
        "runs": args.runs,
        "seam_step": {"before": before[0], "after": after[0], "pairs": before[1]},
        "projected_texels_untouched": bool(torch.equal(levelled[src > 0], proj[src > 0])),
        "repeat_is_bit_identical": bool(torch.equal(again[0], num) and torch.equal(again[1], den)
                                        and torch.equal(apply(), levelled))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res_json, fh, indent=1)
    print(json.dumps(res_json))


if __name__ == "__main__":
    main()
