"""Time centre-of-rotation skinning (csrc/mesh_skin.hip, csrc/cor_blend.h) on the probe character of
tools/skin_probe.py (25 092 vertices, 120 frames).  A worker process runs twice, one after the other:
once under `rocprofv3 --kernel-trace --stats` (no counters), which gives the per-launch time of the
centres kernels (cor_rows_kernel, cor_centres_kernel, cor_reduce_kernel; one build) and of
skin_cor_kernel beside skin_lbs_kernel and skin_dqs_kernel, and once plain, which gives the wall time
of animate.cor_centres and of animate_mesh with each blend (host clock around a call that ends in a
synchronise; the tracer slows the host, so these are not taken under it).  Also recorded: the share of
vertices with a valid centre, the largest distance between this blend and the other two on the
probe's swing, and the bend-tube measures of the float64 restatement (tests/skin_cor_ref.py; CPU).
Nothing is asserted: the apply kernel is to be read against skin_dqs_kernel of the same run, the
centres against the bone-heat solve they sit beside (profiles/skin_probe.json), once per character.

    python tools/skin_cor_probe.py [--runs 10] [--frames 120] [--out profiles/skin_cor_probe.json]

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

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

KERNELS = ("cor_rows_kernel", "cor_centres_kernel", "cor_reduce_kernel", "skin_cor_kernel", "skin_lbs_kernel",
           "skin_dqs_kernel")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_resources():
    isa = _tool("isa_stats")
    try:
        txt = isa.compile_asm(os.path.join(isa.CSRC, "mesh_skin.hip"))
    except (SystemExit, OSError) as e:
        return {"unavailable": str(e)[:200]}
    md, out = isa.metadata(txt), {}
    for name, _ in isa.bodies(txt):
        short = isa.demangle_short(name)
        if short in KERNELS or short == "cor_centres_wide_kernel":
            m = md[name]
            out[short] = {"vgpr": m["vgpr"], "agpr": m["agpr"], "sgpr": m["sgpr"], "lds_bytes": m["lds"],
                          "scratch_bytes": m["scratch"], "vgpr_spills": m["vspill"], "sgpr_spills": m["sspill"],
                          "threads": 256}
    return out


def bend_tube_measures():
    """The measures of docs/NEXT_ROWS.md from the float64 restatements of the three blends (numpy)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import skin_cor_ref as C
    import skin_dqs_ref as D
    import skin_ref as R
    from drawingspinup_amd import animate
    v, f, infl, w = C.bend_tube()
    joints, cw = C.canonical(infl, w, 2)
    cen, val = C.centres(v, f, joints, cw, 2, 0.1)
    out = {"tube": "24 x 41 vertices, radius 0.1, length 2, smoothstep weights across |y| <= 0.3, sigma 0.1",
           "valid_rings": int(val.reshape(C.TUBE_RINGS, C.TUBE_SEGS).all(1).sum())}

    def blends(mats):
        _, cor = C.skin_cor(v, infl, w, mats, C.quats_of(mats), cen, val)
        _, dqs, _ = D.skin_dqs(v, infl, w, animate.dual_quaternions(mats))
        lbs, _ = R.skin_lbs(v, infl, w, mats.astype(np.float32))
        return {"linear": lbs[0], "dual_quaternion": dqs[0], "centre_of_rotation": cor[0]}

    def ring_radius(p):
        r = p.reshape(C.TUBE_RINGS, C.TUBE_SEGS, 3)
        return float(np.linalg.norm(r - r.mean(1, keepdims=True), axis=-1).min()) / C.TUBE_R

    for deg in (90.0, 120.0):
        mats = C.two_joint_clip("Z", deg)
        out["bend_%d" % deg] = {k: {"smallest_ring_radius_over_r": ring_radius(p),
                                    "largest_axis_distance_over_r": float(C.axis_distance(p, mats).max()) / C.TUBE_R,
                                    "smallest_axis_distance_over_r": float(C.axis_distance(p, mats).min()) / C.TUBE_R}
                                for k, p in blends(mats).items()}
    for deg in (120.0, 178.0):
        out["twist_%d" % deg] = {k: {"smallest_ring_radius_over_r": float(np.hypot(p[:, 0], p[:, 2]).min()) / C.TUBE_R}
                                 for k, p in blends(C.two_joint_clip("Y", deg)).items()}
    return out


def worker(a):
    import numpy as np
    import torch
    from drawingspinup_amd import animate, ops
    if not torch.cuda.is_available():
        raise SystemExit("skin_cor_probe needs a GPU")
    probe = _tool("skin_probe")
    dev = torch.device("cuda:0")
    v, f, sk = probe.character()
    clip = probe.swing(sk, a.frames)
    col = np.random.default_rng(1).random((len(v), 3)).astype(np.float32)
    infl, w = animate.bone_heat_weights(v, f, sk, device=dev)
    J = len(sk.names)
    tv = torch.from_numpy(v.astype(np.float32)).to(dev)
    tf = torch.from_numpy(f.astype(np.int32)).to(dev)
    ti, tw = torch.from_numpy(infl).to(dev), torch.from_numpy(w).to(dev)
    m64 = animate.skinning_matrices(sk, clip)
    mats32 = torch.from_numpy(m64.astype(np.float32)).to(dev)
    mats = torch.from_numpy(m64).to(dev)
    dq = torch.from_numpy(animate.dual_quaternions(m64)).to(dev)
    quats = torch.from_numpy(animate.rotation_quaternions(m64[..., :3])).to(dev)
    n_c = max(2, a.runs // 3)
    t_centres_op = probe.timed(lambda: ops.skin_cor_centres(tv, tf, infl, w, J), n_c, warmup=1)
    t_centres = probe.timed(lambda: animate.cor_centres(v, f, (infl, w), J, device=dev), n_c, warmup=1)
    cen, val = ops.skin_cor_centres(tv, tf, infl, w, J)
    t_lbs = probe.timed(lambda: ops.skin_lbs(tv, ti, tw, mats32), a.runs)
    t_dqs = probe.timed(lambda: ops.skin_dqs(tv, ti, tw, dq), a.runs)
    t_cor = probe.timed(lambda: ops.skin_cor(tv, ti, tw, mats, quats, cen, val), a.runs)
    cor, lbs, dqs = ops.skin_cor(tv, ti, tw, mats, quats, cen, val), ops.skin_lbs(tv, ti, tw, mats32), ops.skin_dqs(tv, ti, tw, dq)
    joints, _ = ops.skin_cor_table(infl, w, J)
    t_all = {}
    for blend in animate.skin.SKINNING:
        kw = {"centres": (cen, val)} if blend == "centre_of_rotation" else {}
        t_all[blend] = probe.timed(lambda: animate.animate_mesh(v, f, col, sk, clip, weights=(infl, w), device=dev,
                                                                skinning=blend, **kw), n_c, warmup=1)
    t_all["centre_of_rotation_centres_computed"] = probe.timed(
        lambda: animate.animate_mesh(v, f, col, sk, clip, weights=(infl, w), device=dev, skinning="centre_of_rotation"),
        n_c, warmup=1)
    res = {"mesh": "seeded tube character of tools/skin_probe.py", "verts": int(len(v)), "faces": int(len(f)),
           "joints": J, "frames": a.frames, "runs": a.runs, "sigma": 0.1, "K": int(infl.shape[1]),
           "canonical_K": int(joints.shape[1]), "vertex_triangle_pairs": int(len(v)) * int(len(f)),
           "valid_centres": int(val.sum().item()), "valid_share": float(val.float().mean().item()),
           "skin_cor_centres_ms": dict(t_centres_op, note="ops.skin_cor_centres: canonical table on the host (numpy), "
                                                          "upload, workspace, three launches"),
           "animate_cor_centres_ms": dict(t_centres, note="animate.cor_centres: host arrays in"),
           "skin_lbs_ms": t_lbs, "skin_dqs_ms": t_dqs, "skin_cor_ms": t_cor,
           "largest_distance_from_linear": float((cor - lbs).norm(dim=-1).max().item()),
           "largest_distance_from_dual_quaternion": float((cor - dqs).norm(dim=-1).max().item()),
           "largest_distance_dual_quaternion_from_linear": float((dqs - lbs).norm(dim=-1).max().item()),
           "animate_mesh_ms": dict(t_all, note="weights given; host arrays in, uploads included; centre_of_rotation "
                                               "with the centres handed in, and with them computed in the call"),
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
                            ns[k].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    missing = [k for k, x in ns.items() if not x]
    if missing:
        raise SystemExit(f"no launches of {missing} in the traces under {folder}")
    out = {k: {"median_us": statistics.median(d) / 1e3, "min_us": min(d) / 1e3, "max_us": max(d) / 1e3, "launches": len(d)}
           for k, d in ns.items()}
    out["skin_cor_over_skin_dqs"] = out["skin_cor_kernel"]["median_us"] / out["skin_dqs_kernel"]["median_us"]
    out["note"] = "rocprofv3 --kernel-trace --stats of a worker run of its own; the other figures are from a plain run"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skin_cor_probe.json"))
    ap.add_argument("--keep-trace", metavar="DIR", help="keep the tracer's output under DIR")
    ap.add_argument("--worker", metavar="JSON", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        raise SystemExit("rocprofv3 not found")
    tmp = a.keep_trace or tempfile.mkdtemp(prefix="skin_cor_probe_")
    os.makedirs(tmp, exist_ok=True)
    part = os.path.join(tmp, "worker.json")
    cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
           sys.executable, os.path.abspath(__file__), "--worker", part, "--frames", str(a.frames), "--runs", str(a.runs)]
    r = subprocess.run(cmd, cwd=ROOT)
    if r.returncode != 0 or not os.path.exists(part):
        raise SystemExit(f"the traced worker failed (exit {r.returncode})")
    # the wall times: the same worker without the tracer (this overwrites the traced run's figures)
    r = subprocess.run(cmd[cmd.index("--") + 1:], cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the plain worker failed (exit {r.returncode})")
    with open(part) as fh:
        res = json.load(fh)
    res["kernel_trace"] = read_trace(os.path.join(tmp, "trace"))
    res["kernels"] = kernel_resources()
    res["bend_tube_restatement"] = bend_tube_measures()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not a.keep_trace:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
