"""The one-wave-per-ray marcher against the serial rule of oracle/nerfacc_ref.py, bit for bit.

Every case goes through ops.ray_march (the shipped path: scratch rows, offsets scan, compaction)
and through the scratch-row entry itself (dsu_ray_march_scratch) and must give the oracle's counts,
ray indices and the bits of t_starts / t_ends.  The oracle is a Python loop, so the grids are res 16..32, the step is
2*1.732/256 and a case holds a few hundred rays; each oracle result is computed once.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from drawingspinup_amd import ops
from drawingspinup_amd._lib import check, lib, ptr, stream
from oracle import nerfacc_ref as nr

pytestmark = pytest.mark.gpu
f32 = np.float32
AABB = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
STEP = 2 * 1.732 / 256
G = 64                      # lanes per ray of the shipped kernel
GUARD = f32(-7.5)


def _grid(kind, res):
    if kind is None:
        return None
    ix = np.indices((res, res, res))
    if kind == "full":
        return np.ones(res ** 3, np.uint8)
    if kind == "empty":
        return np.zeros(res ** 3, np.uint8)
    if kind == "checker":
        return (ix.sum(0) % 2).reshape(-1).astype(np.uint8)
    c = (ix + 0.5) / res * 2 - 1
    r = np.sqrt((c ** 2).sum(0))
    return ((r > 0.45) & (r < 0.6)).reshape(-1).astype(np.uint8)      # shell


@functools.lru_cache(maxsize=None)
def _mixed_rays(aabb, n_oblique=120, n_axis=60, n_miss=23):
    """Oblique and axis-parallel rays with jittered starts, and rays that miss the box
    (near = far = 1e10).  203 rays: not a multiple of the four rays of a workgroup."""
    g = np.random.default_rng(17)
    half = f32(aabb[3])
    o1 = np.tile(np.array([[0.1, -0.2, -1.5]], f32) * half, (n_oblique, 1))
    d1 = g.normal(size=(n_oblique, 3)).astype(f32) * 0.25 + np.array([0, 0, 1], f32)
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    o2 = np.zeros((n_axis, 3), f32); d2 = np.zeros((n_axis, 3), f32)
    for r in range(n_axis):
        axis, sign = r % 3, (1.0 if (r // 3) % 2 == 0 else -1.0)
        uv = (g.random(2).astype(f32) - 0.5) * 2 * 0.9 * half
        oth = [a for a in range(3) if a != axis]
        o2[r, oth[0]], o2[r, oth[1]], o2[r, axis] = uv[0], uv[1], -1.3 * sign * half
        d2[r, axis] = sign
    o3 = np.tile(np.array([[3.0, 3.0, -1.3]], f32), (n_miss, 1))
    d3 = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (n_miss, 1))
    o = np.concatenate([o1, o2, o3]); d = np.concatenate([d1, d2, d3])
    perm = g.permutation(o.shape[0])
    o, d = o[perm], d[perm]
    tmin, tmax = nr.ray_aabb_intersect(o, d, aabb)
    assert (tmin[np.all(o == o3[0], axis=1)] == f32(1e10)).all()
    tmin = (tmin + g.random(o.shape[0]).astype(f32) * f32(STEP)).astype(f32)
    return o, d, tmin, tmax


@functools.lru_cache(maxsize=None)
def _mixed_case(kind, res, aabb=AABB):
    o, d, tmin, tmax = _mixed_rays(aabb)
    occ = _grid(kind, res)
    return (o, d, tmin, tmax, occ) + nr.ray_marching(o, d, tmin, tmax, aabb, occ, res, STEP)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run_scratch(dev, o, d, tmin, tmax, aabb, occ, res, step, cap):
    """dsu_ray_march_scratch into guard-filled rows; -> counts, rows of t_starts, t_ends, and the
    guard tail behind the last row."""
    n = o.shape[0]
    tail = 64
    sc0 = torch.full((n * cap + tail,), float(GUARD), dtype=torch.float32, device=dev)
    sc1 = torch.full((n * cap + tail,), float(GUARD), dtype=torch.float32, device=dev)
    counts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    a = (C.c_float * 6)(*aabb)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    tn, tx = torch.from_numpy(tmin).to(dev), torch.from_numpy(tmax).to(dev)
    occ_t = None if occ is None else torch.from_numpy(occ).to(dev)
    check(lib().dsu_ray_march_scratch(ptr(to), ptr(td), ptr(tn), ptr(tx), n, a,
                                      ptr(occ_t, torch.uint8) if occ is not None else None,
                                      int(res), float(step), int(cap), ptr(counts), ptr(sc0),
                                      ptr(sc1), stream()), "dsu_ray_march_scratch")
    torch.cuda.synchronize()
    s0, s1 = sc0.cpu().numpy(), sc1.cpu().numpy()
    return (counts.cpu().numpy(), s0[:n * cap].reshape(n, cap), s1[:n * cap].reshape(n, cap),
            np.concatenate([s0[n * cap:], s1[n * cap:]]))


def _check_both_entries(dev, o, d, tmin, tmax, aabb, occ, res, step, ref, cap=None):
    ri_r, ts_r, te_r, cnt_r = ref
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    tn, tx = torch.from_numpy(tmin).to(dev), torch.from_numpy(tmax).to(dev)
    occ_t = None if occ is None else torch.from_numpy(occ).to(dev)
    ri, ts, te, off, cnt = ops.ray_march(to, td, tn, tx, list(aabb), occ_t, res, step)
    assert np.array_equal(cnt.cpu().numpy(), cnt_r)
    assert np.array_equal(ri.cpu().numpy(), ri_r)
    assert np.array_equal(_bits(ts.cpu().numpy()), _bits(ts_r))
    assert np.array_equal(_bits(te.cpu().numpy()), _bits(te_r))
    # scratch rows: exact counts, row entries below min(count, cap), guards everywhere else
    if cap is None:
        cap = int(cnt_r.max()) + 3
    cnt_s, r0, r1, tail = _run_scratch(dev, o, d, tmin, tmax, aabb, occ, res, step, cap)
    assert np.array_equal(cnt_s, cnt_r)
    exp0 = np.full(r0.shape, GUARD, f32); exp1 = np.full(r1.shape, GUARD, f32)
    off_r = np.cumsum(cnt_r) - cnt_r
    for i in range(o.shape[0]):
        m = min(int(cnt_r[i]), cap)
        exp0[i, :m] = ts_r[off_r[i]:off_r[i] + m]
        exp1[i, :m] = te_r[off_r[i]:off_r[i] + m]
    assert np.array_equal(_bits(r0), _bits(exp0))
    assert np.array_equal(_bits(r1), _bits(exp1))
    assert (tail == GUARD).all()


@pytest.mark.parametrize("kind,res", [("shell", 32), ("checker", 16), ("full", 32),
                                      ("empty", 16), (None, 0)])
def test_grids_and_ray_kinds(dev, kind, res):
    o, d, tmin, tmax, occ, *ref = _mixed_case(kind, res)
    assert o.shape[0] % 4 != 0
    if kind in ("shell", "checker", "full", None):
        assert ref[3].sum() > 1000
    else:
        assert ref[3].sum() == 0
    _check_both_entries(dev, o, d, tmin, tmax, AABB, occ, res, STEP, ref)


def test_non_power_of_two_box_and_grid(dev):
    # res 24 and extent 1.5: the instantiation with IEEE divisions (P2 = false)
    aabb = (-0.75, -0.75, -0.75, 0.75, 0.75, 0.75)
    o, d, tmin, tmax, occ, *ref = _mixed_case("shell", 24, aabb)
    assert ref[3].sum() > 1000
    _check_both_entries(dev, o, d, tmin, tmax, aabb, occ, 24, STEP, ref)


@functools.lru_cache(maxsize=None)
def _window_edge_case():
    """Rays along +z at t = z + 1.3.  Runs of G - 1, G and G + 1 accepted samples, ended (a) by the
    far plane in a full grid and (b) by the empty cells behind a slab; behind the slab an empty
    stretch longer than one window that ends (b1) at a second slab, (b2) exactly at far."""
    res = 32
    dt = f32(STEP)
    g = np.random.default_rng(3)
    rays = []          # (grid id, x, y, near, far)
    for run in (G - 1, G, G + 1):
        for r in range(4):
            near = f32(0.3 + 0.37 * r)
            rays.append((0, near, f32(near + (run - 0.25) * dt)))
    # slab z in [-1, -0.125): 14 cells = 64.67 steps; the phase of the first sample makes the run
    # 63, 64 or 65 (checked on the oracle's counts in the test)
    for gid in (1, 2):
        for r in range(24):
            rays.append((gid, f32(0.3 + (r / 8.0) * dt), f32(2.3)))
    full = np.ones((res, res, res), np.uint8)
    two_slabs = np.zeros((res, res, res), np.uint8)
    two_slabs[:, :, :14] = 1
    two_slabs[:, :, 30:] = 1          # 16 empty cells = 73.9 steps between the slabs
    one_slab = two_slabs.copy()
    one_slab[:, :, 30:] = 0           # empty from the slab to the far plane
    grids = [full.reshape(-1), two_slabs.reshape(-1), one_slab.reshape(-1)]
    cases = []
    for gid, occ in enumerate(grids):
        sel = [r for r in rays if r[0] == gid]
        n = len(sel)
        o = np.zeros((n, 3), f32); d = np.zeros((n, 3), f32)
        o[:, :2] = (g.random((n, 2)).astype(f32) - 0.5) * 1.8
        o[:, 2] = -1.3
        d[:, 2] = 1.0
        tmin = np.array([r[1] for r in sel], f32); tmax = np.array([r[2] for r in sel], f32)
        cases.append((o, d, tmin, tmax, occ) + nr.ray_marching(o, d, tmin, tmax, AABB, occ, res, STEP))
    return cases


@pytest.mark.parametrize("gid", [0, 1, 2])
def test_window_edges(dev, gid):
    o, d, tmin, tmax, occ, *ref = _window_edge_case()[gid]
    cnt = ref[3]
    if gid == 0:
        assert sorted(set(cnt.tolist())) == [G - 1, G, G + 1]
    else:
        first_run = np.array([int(np.argmax(np.diff(ref[1][ref[0] == i]) > f32(1.5 * STEP)) + 1)
                              if gid == 1 else int(cnt[i]) for i in range(o.shape[0])])
        assert {G - 1, G, G + 1} <= set(first_run.tolist()), sorted(set(first_run.tolist()))
        if gid == 1:
            assert (cnt > first_run).all()        # every ray lands in the second slab
    _check_both_entries(dev, o, d, tmin, tmax, AABB, occ, 32, STEP, ref)


def test_one_skip_longer_than_a_window(dev):
    # a step so small that one res-16 cell holds 74 lattice points: a single voxel skip spans
    # more than a window and its target is carried into the next one
    res = 16
    occ = np.zeros((res, res, res), np.uint8)
    occ[:, :, 13:] = 1
    occ = occ.reshape(-1)
    o, d, tmin, tmax = (x[:40] for x in _mixed_rays(AABB))
    step = STEP / 8
    ref = nr.ray_marching(o, d, tmin, tmax, AABB, occ, res, step)
    assert ref[3].sum() > 1000
    _check_both_entries(dev, o, d, tmin, tmax, AABB, occ, res, step, ref)


def test_scratch_rows_shorter_than_the_longest_ray(dev):
    o, d, tmin, tmax, occ, *ref = _mixed_case("shell", 32)
    cap = 20
    assert (ref[3] > cap).sum() > 20 and ((ref[3] > 0) & (ref[3] < cap)).sum() > 5
    _check_both_entries(dev, o, d, tmin, tmax, AABB, occ, 32, STEP, ref, cap=cap)
    # a capacity that cuts a row in the middle of a window of accepted samples
    o, d, tmin, tmax, occ, *ref = _mixed_case("full", 32)
    assert ref[3].max() > 2 * G
    _check_both_entries(dev, o, d, tmin, tmax, AABB, occ, 32, STEP, ref, cap=G + 7)
