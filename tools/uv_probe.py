"""Time the UV export (csrc/mesh_uv.hip, nsr/uv.py) at production size: a ~50 000-face character
into a 1024^2 atlas — labels, chart components (per round), binning, raster, gutter fill (median of
--runs after warm-up, device events) and the host's projection + packing; chart count, split
rounds, atlas fill, and the accuracy figures the tests quote (device against tests/uv_ref.py on
the tests' meshes: differing labels / chart ids / face ids / demote flags / image bytes, fragile
samples).

    python tools/uv_probe.py [--size 1024] [--runs 20] [--out profiles/uv_probe.json]

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

from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402


def character(nu=200, nv=128, seed=0):
    """A closed, bumpy, flat-ish surface of 2 nu nv triangles: a thick ring squeezed along z."""
    rng = np.random.default_rng(seed)
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    r = 0.18 * (1.0 + 0.15 * np.sin(3 * u + rng.uniform(0, 6)) * np.cos(2 * w))
    v = np.stack([(0.38 + r * np.cos(w)) * np.cos(u), (0.38 + r * np.cos(w)) * np.sin(u), 0.35 * r * np.sin(w)],
                 -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(nu) for j in range(nv)] + \
        [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(nu) for j in range(nv)]
    return v.astype(np.float32), np.asarray(f, np.int64), rng.random((len(v), 3)).astype(np.float32)


def timed(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def accuracy(dev):
    import uv_ref as R
    out = {}
    for name, size in (("body_and_arm", 64), ("character", 128), ("helicoid", 128), ("lattice", 128)):
        r = R.reference(name, size)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        n, lab, ar = ops.uv_face_labels(t(r["verts"], np.float32), t(r["faces"], np.int64))
        rn, rl, ra = R.face_labels(r["verts"], r["faces"])
        chart, rounds = ops.uv_components(ops.face_adjacency(t(r["faces"], np.int64)), lab)
        depth = U.face_depths(r["verts"], r["faces"], r["info"]["label"])
        img, fid, dem = ops.uv_bake(t(r["uvs"], np.float32), t(r["indices"], np.int32), t(r["colours"], np.float32),
                                    size, t(depth, np.float64))
        out[f"{name}_{size}"] = {
            "labels_differ": int((lab.cpu().numpy() != rl).sum()),
            "normals_differ": int((n.cpu().numpy() != rn).any(1).sum()),
            "chart_ids_differ": int((chart.cpu().numpy() != R.components(r["faces"], rl)).sum()),
            "component_rounds": rounds,
            "face_id_differ": int((fid.cpu().numpy() != r["face_id"]).sum()),
            "image_texels_differ": int((img.cpu().numpy() != r["image"]).any(-1).sum()),
            "demote_differ": int((dem.cpu().numpy() != r["demote"]).sum()),
            "fragile_samples": int(r["fragile"].sum()), "samples": size * size}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--gutter", type=int, default=2)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    verts, faces, colours = character()
    S = args.size
    t0 = time.perf_counter()
    vm, ind, uvs, info = U.parametrize(verts, faces, S, args.gutter, return_info=True, device=dev)
    torch.cuda.synchronize()
    t_param = time.perf_counter() - t0
    t0 = time.perf_counter()
    U.layout(verts, faces, info["label"], info["face_chart"], S, args.gutter)
    t_host = time.perf_counter() - t0

    dv, df = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    adj = ops.face_adjacency(df)
    _, lab, _ = ops.uv_face_labels(dv, df)
    _, rounds = ops.uv_components(adj, lab)
    duv, dind = torch.from_numpy(uvs).to(dev), torch.from_numpy(ind.astype(np.int32)).to(dev)
    dcol = torch.from_numpy(colours[vm]).to(dev)
    ddepth = torch.from_numpy(U.face_depths(verts, faces, info["label"])).to(dev)
    plan = ops.UvBakePlan(duv, dind, S).bin()
    img, fid, _ = plan.raster(dcol, ddepth)
    cov = (fid >= 0).to(torch.uint8)
    ms_comp = timed(lambda: ops.uv_components(adj, lab), args.runs)
    res = {
        "device": torch.cuda.get_device_name(0), "faces": int(len(faces)), "new_vertices": int(len(vm)),
        "size": S, "gutter": args.gutter, "charts": int(len(info["chart_ids"])),
        "split_rounds": int(info["split_rounds"]), "isolated_faces": int(info["isolated_faces"]),
        "pack_retries": int(info["pack_retries"]), "scale_texels_per_unit": info["scale"],
        "atlas_fill": float(cov.float().mean()), "faces_per_tile_max": int(plan.workspace[:plan.bins].max()),
        "ms": {"labels": timed(lambda: ops.uv_face_labels(dv, df), args.runs),
               "adjacency_torch": timed(lambda: ops.face_adjacency(df), args.runs),
               "components_total": ms_comp, "components_rounds": rounds, "components_per_round": ms_comp / max(rounds, 1),
               "bin": timed(lambda: ops.UvBakePlan(duv, dind, S).bin(), args.runs),
               "raster": timed(lambda: plan.raster(dcol, ddepth), args.runs),
               "dilate_all_rounds": timed(lambda: ops.uv_dilate(img, cov, args.gutter), args.runs),
               "host_projection_and_packing": t_host * 1e3, "parametrize_whole_loop": t_param * 1e3},
        "accuracy": accuracy(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
