"""Time the rigging steps (csrc/mesh_skin.hip) on a synthetic ~50 000-face character with 25 bones
and 120 frames: triangle binning, distances + visibility, the bone-heat solve (with its iteration
count), skinning (linear-blend and dual-quaternion), and the render of the same 120 frames; plus the compiler's register / LDS / spill
figures of the three kernels and, with --accuracy, the differences from the float64 reference
(tests/skin_ref.py) on the three test meshes that the GPU tests' bars are set from.

    python tools/skin_probe.py [--runs 10] [--frames 120] [--accuracy] [--out profiles/skin_probe.json]

Kernel times of the two skinning kernels come from a trace of the same run, taken from outside and
merged afterwards (the second command needs no GPU):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/skin_probe.py ...
    python tools/skin_probe.py --merge-trace DIR [--out profiles/skin_probe.json]

The probe itself needs a GPU: there is no fallback.
"""
import argparse
import csv
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from drawingspinup_amd import animate, ops  # noqa: E402
from drawingspinup_amd.animate import skin  # noqa: E402


def tube(p0, p1, radius, n_around, n_along, rng):
    """Closed bumpy tube around p0 -> p1 (two pole vertices)."""
    p0, p1 = np.asarray(p0, float), np.asarray(p1, float)
    w = (p1 - p0) / np.linalg.norm(p1 - p0)
    u = np.cross(w, [0, 0, 1.0] if abs(w[2]) < 0.9 else [1.0, 0, 0])
    u /= np.linalg.norm(u)
    t = np.cross(w, u)
    s = (np.arange(n_along) + 0.5) / n_along
    r = radius * np.sqrt(np.maximum(1 - (2 * s - 1) ** 8, 0.02)) * (1 + 0.05 * np.sin(9 * s + rng.uniform(0, 6)))
    a = 2 * np.pi * np.arange(n_around) / n_around
    ring = p0[None, None] + s[:, None, None] * (p1 - p0)[None, None] + \
        r[:, None, None] * (np.cos(a)[None, :, None] * u + np.sin(a)[None, :, None] * t)
    v = np.concatenate([[p0], ring.reshape(-1, 3), [p1]])
    idx = lambda i, k: 1 + i * n_around + k % n_around
    f = []
    for k in range(n_around):
        f += [[0, idx(0, k + 1), idx(0, k)], [len(v) - 1, idx(n_along - 1, k), idx(n_along - 1, k + 1)]]
        for i in range(n_along - 1):
            f += [[idx(i, k), idx(i, k + 1), idx(i + 1, k + 1)], [idx(i, k), idx(i + 1, k + 1), idx(i + 1, k)]]
    return v, np.asarray(f, np.int64)


def character(scale=1.0, seed=0):
    """(verts, faces, Skeleton): torso, head, arms and legs as tubes, 21 joints / 25 bones."""
    rng = np.random.default_rng(seed)
    J = [("hips", -1, (0, -0.05, 0)), ("spine", 0, (0, 0.1, 0)), ("chest", 1, (0, 0.25, 0)), ("neck", 2, (0, 0.38, 0)),
         ("head", 3, (0, 0.45, 0)),
         ("l_shoulder", 2, (0.13, 0.28, 0)), ("l_elbow", 5, (0.28, 0.28, 0)), ("l_wrist", 6, (0.41, 0.28, 0)),
         ("l_hand", 7, (0.45, 0.28, 0)),
         ("r_shoulder", 2, (-0.13, 0.28, 0)), ("r_elbow", 9, (-0.28, 0.28, 0)), ("r_wrist", 10, (-0.41, 0.28, 0)),
         ("r_hand", 11, (-0.45, 0.28, 0)),
         ("l_hip", 0, (0.06, -0.12, 0)), ("l_knee", 13, (0.06, -0.33, 0)), ("l_ankle", 14, (0.06, -0.52, 0)),
         ("l_toe", 15, (0.06, -0.55, 0.05)),
         ("r_hip", 0, (-0.06, -0.12, 0)), ("r_knee", 17, (-0.06, -0.33, 0)), ("r_ankle", 18, (-0.06, -0.52, 0)),
         ("r_toe", 19, (-0.06, -0.55, 0.05))]
    ends = {4: (0, 0.06, 0), 8: (0.02, 0, 0), 12: (-0.02, 0, 0), 16: (0, 0, 0.03), 20: (0, 0, 0.03)}
    pos = np.asarray([p for _, _, p in J], float)
    par = np.asarray([p for _, p, _ in J])
    off = pos - np.where(par[:, None] >= 0, pos[np.maximum(par, 0)], 0.0)
    sk = animate.Skeleton([n for n, _, _ in J], par, off, ends)
    n = lambda x: max(8, int(round(x * scale)))
    parts = [tube((0, -0.18, 0), (0, 0.42, 0), 0.12, n(110), n(100), rng), tube((0, 0.36, 0), (0, 0.56, 0), 0.08, n(64), n(32), rng),
             tube((0.09, 0.28, 0), (0.5, 0.28, 0), 0.04, n(40), n(64), rng), tube((-0.09, 0.28, 0), (-0.5, 0.28, 0), 0.04, n(40), n(64), rng),
             tube((0.06, -0.08, 0), (0.06, -0.6, 0), 0.055, n(48), n(72), rng), tube((-0.06, -0.08, 0), (-0.06, -0.6, 0), 0.055, n(48), n(72), rng)]
    vs, fs, k = [], [], 0
    for v, f in parts:
        vs.append(v); fs.append(f + k); k += len(v)
    v = np.concatenate(vs) + rng.uniform(-2e-4, 2e-4, (k, 3))
    return v, np.concatenate(fs), sk


def swing(sk, n):
    clip = animate.rest_clip(sk, n)
    rot = animate.skeleton.axis_rotation
    for k in range(n):
        a = 45.0 * np.sin(2 * np.pi * k / n)
        clip.rotations[k, 5], clip.rotations[k, 9] = rot("Z", a), rot("Z", a)
        clip.rotations[k, 6] = rot("Z", 0.5 * a + 20)
        clip.rotations[k, 13], clip.rotations[k, 17] = rot("X", 0.6 * a), rot("X", -0.6 * a)
        clip.rotations[k, 14] = rot("X", 15 - 0.3 * a)
        clip.rotations[k, 0] = rot("Y", 0.2 * a)
    return clip


def timed(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def kernel_resources():
    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    try:
        txt = isa.compile_asm(os.path.join(isa.CSRC, "mesh_skin.hip"))
    except (SystemExit, OSError) as e:
        return {"unavailable": str(e)[:200]}
    md, out = isa.metadata(txt), {}
    for name, _ in isa.bodies(txt):
        short = isa.demangle_short(name)
        if short in ("bone_visibility_kernel", "cg_spmv_kernel", "cg_update_kernel", "cg_direction_kernel", "skin_lbs_kernel",
                     "skin_dqs_kernel"):
            m = md[name]
            out[short] = {"vgpr": m["vgpr"], "sgpr": m["sgpr"], "lds_bytes": m["lds"], "scratch_bytes": m["scratch"],
                          "vgpr_spills": m["vspill"], "sgpr_spills": m["sspill"], "threads": 256}
    return out


def accuracy(dev):
    """Device against tests/skin_ref.py on the three test meshes: the figures the tests' bars come from."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import skin_ref as R
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dt is None else \
        torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    out = {}
    for name, (v, f, bones) in R.general_cases().items():
        dist, vis, frag = R.visibility(v, f, bones)
        gd, gv = ops.bone_visibility(t(v), t(f, torch.int32), t(bones))
        gd, gv = gd.cpu().numpy(), gv.cpu().numpy().astype(bool)
        W, parts = R.bone_heat(v, f, bones, dist, vis)
        A, rhs = parts["A"], parts["rhs"]
        x, iters, res = ops.spd_cg_block(t(A.indptr.astype(np.int32)), t(A.indices.astype(np.int32)), t(A.data), t(rhs),
                                         x0=t(parts["P"]), tol=1e-10, max_iters=20000)
        x = x.cpu().numpy()
        out[name] = {"verts": int(len(v)), "faces": int(len(f)), "bones": int(len(bones)),
                     "dist_max_relative_difference": float((np.abs(gd - dist) / dist).max()),
                     "fragile_fraction": float(frag.mean()), "visible_fraction": float(vis.mean()),
                     "visibility_differs": int((gv != vis).sum()),
                     "visibility_differs_outside_fragile": int(((gv != vis) & ~frag).sum()),
                     "cg_iterations": iters, "cg_recurrence_residual": float(res.max()),
                     "cg_true_residual": float((np.linalg.norm(rhs - A @ x, axis=0) / np.linalg.norm(rhs, axis=0)).max()),
                     "max_abs_W_minus_splu": float(np.abs(x - W).max())}
    return out


def merge_trace(folder, out):
    """Median duration of skin_lbs_kernel and skin_dqs_kernel in the *kernel_trace.csv files under
    `folder` (one traced run of this probe), and their ratio, into the probe's JSON."""
    ns = {"skin_lbs_kernel": [], "skin_dqs_kernel": []}
    for dp, _, fs in os.walk(folder):
        for name in fs:
            if not name.endswith("kernel_trace.csv"):
                continue
            with open(os.path.join(dp, name), newline="") as fh:
                for row in csv.DictReader(fh):
                    for k in ns:
                        if k in row.get("Kernel_Name", ""):
                            ns[k].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    if not all(ns.values()):
        raise SystemExit(f"no launches of {[k for k, v in ns.items() if not v]} in the traces under {folder}")
    with open(out) as fh:
        res = json.load(fh)
    us = {k: {"median_us": statistics.median(v) / 1e3, "min_us": min(v) / 1e3, "max_us": max(v) / 1e3, "launches": len(v)}
          for k, v in ns.items()}
    res["skinning_kernel_trace"] = dict(us, dqs_over_lbs=us["skin_dqs_kernel"]["median_us"] / us["skin_lbs_kernel"]["median_us"],
                                        bytes_written_per_launch=12 * res["frames"] * res["verts"],
                                        note="rocprofv3 --kernel-trace of the run that wrote this file")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["skinning_kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-trace", metavar="DIR", help="read a kernel trace of an earlier run into --out; no GPU needed")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="mesh resolution factor (1.0: ~50 000 faces)")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skin_probe.json"))
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("skin_probe needs a GPU")
    dev = torch.device("cuda:0")
    v, f, sk = character(a.scale)
    heads, segs = sk.bones()
    clip = swing(sk, a.frames)
    col = np.random.default_rng(1).random((len(v), 3)).astype(np.float32)
    tv, tf = torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)
    tb = torch.from_numpy(segs.astype(np.float32)).to(dev)
    plan = ops.BoneVisibilityPlan(tv, tf, tb)
    t_bin = timed(lambda: plan.bin(), a.runs)
    t_vis = timed(lambda: plan.run(), a.runs)
    dist, vis = (x.cpu().numpy() for x in plan.run())
    t0 = time.perf_counter()
    floor = skin.D_FLOOR * float(np.linalg.norm(v.max(0) - v.min(0)))
    P, h, blind = skin.heat_sources(dist, vis, skin.components(len(v), f), floor)
    A, rhs = skin.heat_system(v.astype(np.float32).astype(np.float64), f, P, h)
    t_assemble = (time.perf_counter() - t0) * 1e3
    csr = [torch.from_numpy(x).to(dev) for x in (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, rhs, P)]
    solve = lambda: ops.spd_cg_block(csr[0], csr[1], csr[2], csr[3], x0=csr[4], tol=1e-10, max_iters=20000)
    t_solve = timed(solve, max(2, a.runs // 3), warmup=1)
    W, iters, res = solve()
    W = W.cpu().numpy()
    true = float((np.linalg.norm(rhs - A @ W, axis=0) / np.maximum(np.linalg.norm(rhs, axis=0), 1e-300)).max())
    infl, w = skin.finish_weights(W, heads, 4)
    mats = torch.from_numpy(animate.skinning_matrices(sk, clip).astype(np.float32)).to(dev)
    ti, tw = torch.from_numpy(infl).to(dev), torch.from_numpy(w).to(dev)
    t_skin = timed(lambda: ops.skin_lbs(tv, ti, tw, mats), a.runs)
    dq = torch.from_numpy(animate.dual_quaternions(animate.skinning_matrices(sk, clip))).to(dev)
    t_dqs = timed(lambda: ops.skin_dqs(tv, ti, tw, dq), a.runs)
    apart = (ops.skin_dqs(tv, ti, tw, dq) - ops.skin_lbs(tv, ti, tw, mats)).norm(dim=-1)
    screen = ops.skin_lbs(tv, ti, tw, mats)
    box = torch.stack([screen.amin((0, 1)), screen.amax((0, 1))]).cpu().numpy()
    cx, cy, size, span = animate.frame_window(box)
    pos = torch.from_numpy(animate.position_colours(v).astype(np.float32)).to(dev)
    tc, tf64 = torch.from_numpy(col).to(dev), torch.from_numpy(f).to(dev)
    t_render = timed(lambda: ops.pos_edge_u8(ops.mesh_render_ortho(screen, tf64, tc, pos, cx, cy, span, size, 4)["pos_u8"]),
                     max(2, a.runs // 2))
    t_all = timed(lambda: animate.animate_mesh(v, f, col, sk, clip, weights=(infl, w), device=dev), max(2, a.runs // 3), warmup=1)
    res_json = {"mesh": "seeded tube character", "verts": int(len(v)), "faces": int(len(f)), "bones": int(len(heads)),
                "joints": sk.n_joints, "frames": a.frames, "runs": a.runs,
                "grid": plan.g, "grid_items": int(plan.items.numel()),
                "binning_ms": dict(t_bin, note="count + prefix sum (torch, one read-back) + fill"),
                "visibility_ms": t_vis, "pairs": int(len(v) * len(heads)),
                "brute_force_tests": int(len(v)) * int(len(heads)) * int(len(f)),
                "visible_fraction": float(vis.mean()), "fallback_components": int(len(blind)),
                "assemble_host_ms": t_assemble,
                "solve_ms": dict(t_solve, iterations=iters, recurrence_residual=float(res.max()), true_residual=true,
                                 tol=1e-10, nnz=int(A.nnz)),
                "skinning_ms": t_skin,
                "skinning_dqs_ms": dict(t_dqs, largest_distance_from_linear=float(apart.max()),
                                        note="dual-quaternion blend of the same frames; host clock around one launch"),
                "render_ms": dict(t_render, size=int(size), span=float(span), ss=4,
                                                         note="bin + raster + resolve + edges of the skinned frames"),
                "animate_mesh_ms": dict(t_all, note="weights given; host arrays in, uploads included"),
                "kernels": kernel_resources(), "device": torch.cuda.get_device_name(0)}
    ref = os.path.join(ROOT, "profiles", "frame_render_probe.json")
    if os.path.exists(ref):
        with open(ref) as fh:
            r = json.load(fh)
        res_json["for_scale_frame_render_probe"] = {k: r[k] for k in ("frames", "faces", "binning_ms", "raster_resolve_ms", "edges_ms") if k in r}
    if a.accuracy:
        res_json["accuracy_vs_reference"] = accuracy(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res_json, fh, indent=1)
    print(json.dumps(res_json))


if __name__ == "__main__":
    main()
