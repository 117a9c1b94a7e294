"""The windowed marching rule of ray_march_kernel (csrc/nsr_render.hip), restated in numpy.

The kernel gives G lanes to one ray and applies the serial nerfacc rule to G lattice points per
round.  `windowed_ray_marching` below is that scheme lane by lane, built from the oracle's own
point helpers; it has to give the bits of oracle/nerfacc_ref.py::ray_marching for every G.  This
pins the SCHEME on the CPU (which points a window holds, what the group does with them); the
kernel itself is compared with the oracle in tests/test_gpu_march_cooperative.py.
"""
import numpy as np
import pytest

from oracle import nerfacc_ref as nr

f32 = np.float32
AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
STEP = 2 * 1.732 / 256


def windowed_ray_marching(o, d, t_min, t_max, aabb, occ_binary, res, step, G, rounds=None):
    o = o.astype(f32); d = d.astype(f32); aabb = np.asarray(aabb, f32)
    mn, mx = aabb[:3], aabb[3:]
    dt = f32(step)
    half = f32(dt * f32(0.5))
    occ = None if occ_binary is None else np.asarray(occ_binary).reshape(-1)
    ri, ts, te, counts = [], [], [], []
    with np.errstate(divide="ignore"):
        for i in range(o.shape[0]):
            inv = (f32(1.0) / d[i]).astype(f32)
            far = f32(t_max[i])
            t0 = f32(t_min[i]); t1 = f32(t0 + dt); tm = f32((t0 + t1) * f32(0.5))
            j = 0
            rejected = carried = False
            carried_target = f32(0)
            n_rounds = 0
            while True:
                n_rounds += 1
                if not rejected:
                    # accept window: lane b holds (e_b, e_{b+1}) and their midpoint
                    e = [t0, t1]
                    for _ in range(G):
                        e.append(f32(e[-1] + dt))
                    em = [tm] + [f32((e[b] + e[b + 1]) * f32(0.5)) for b in range(1, G)]
                    s = G
                    for b in range(G):
                        if not (em[b] < far) or \
                                not nr._occupied((o[i] + em[b] * d[i]).astype(f32), mn, mx, occ, res):
                            s = b
                            break
                    for b in range(s):
                        ri.append(i); ts.append(e[b]); te.append(e[b + 1])
                    j += s
                    if s == G:
                        t0 = e[G]; t1 = e[G + 1]; tm = f32((t0 + t1) * f32(0.5))
                    elif not (em[s] < far):
                        break
                    else:
                        tm = em[s]; rejected = True; carried = False
                else:
                    # reject window: lane k holds c_k, its skip target and whether a landing on
                    # it ends the skipping
                    c = [tm]
                    for _ in range(G - 1):
                        c.append(f32(c[-1] + dt))
                    target, lands = [], []
                    for k in range(G):
                        p = (o[i] + c[k] * d[i]).astype(f32)
                        target.append(nr._fmin(
                            f32(c[k] + nr._dist_to_next_voxel(p, d[i], inv, mn, mx, res)), far))
                        lands.append(not (c[k] < far) or nr._occupied(p, mn, mx, occ, res))
                    if carried:
                        target[0] = carried_target
                    k = 0
                    while True:
                        nxt = next((m for m in range(k + 1, G) if not (c[m] < target[k])), None)
                        if nxt is None:          # the skip from k leaves the window
                            tm = c[G - 1]; carried = True; carried_target = target[k]
                            break
                        k = nxt
                        if lands[k]:
                            tm = c[k]; t0 = f32(tm - half); t1 = f32(tm + half)
                            rejected = False
                            break
            counts.append(j)
            if rounds is not None:
                rounds.append(n_rounds)
    return (np.asarray(ri, np.int64), np.asarray(ts, f32), np.asarray(te, f32),
            np.asarray(counts, np.int32))


def _rays(n, seed):
    g = np.random.default_rng(seed)
    o = np.tile(np.array([[0.1, -0.2, -1.5]], f32), (n, 1))
    d = g.normal(size=(n, 3)).astype(f32) * 0.25 + np.array([0, 0, 1], f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmin, tmax = nr.ray_aabb_intersect(o, d, AABB)
    tmin = (tmin + g.random(n).astype(f32) * f32(STEP)).astype(f32)
    return o, d, tmin, tmax


def _grid(kind, res):
    ix = np.indices((res, res, res))
    if kind == "full":
        return np.ones(res ** 3, np.uint8)
    if kind == "checker":
        return (ix.sum(0) % 2).reshape(-1).astype(np.uint8)
    c = (ix + 0.5) / res * 2 - 1
    r = np.sqrt((c ** 2).sum(0))
    return ((r > 0.45) & (r < 0.6)).reshape(-1).astype(np.uint8)      # shell


@pytest.mark.parametrize("kind,res", [("shell", 32), ("checker", 16), ("full", 32)])
def test_windowed_rule_has_the_serial_rules_bits(kind, res):
    occ = _grid(kind, res)
    o, d, tmin, tmax = _rays(120, 11)
    ref = nr.ray_marching(o, d, tmin, tmax, AABB, occ, res, STEP)
    assert ref[3].sum() > 1000
    for G in (16, 64):
        rounds = []
        got = windowed_ray_marching(o, d, tmin, tmax, AABB, occ, res, STEP, G, rounds)
        assert np.array_equal(got[3], ref[3])
        assert np.array_equal(got[0], ref[0])
        assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
        assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))
        print(f"{kind} res {res} G {G}: {np.mean(rounds):.1f} rounds per ray")


def test_windowed_rule_one_skip_longer_than_a_window():
    # a step so small that one voxel holds more lattice points than a window: the skip's target
    # is carried from window to window
    res = 16
    occ = np.zeros((res, res, res), np.uint8)
    occ[:, :, 12:] = 1
    o, d, tmin, tmax = _rays(6, 5)
    step = STEP / 8
    ref = nr.ray_marching(o, d, tmin, tmax, AABB, occ.reshape(-1), res, step)
    got = windowed_ray_marching(o, d, tmin, tmax, AABB, occ.reshape(-1), res, step, 16)
    assert ref[3].sum() > 500
    assert np.array_equal(got[3], ref[3])
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))
