"""CPU: the corrective smoothing (delta mush) without a device — the welded topology
(animate/corrective.py), and the host entries that compile the kernels' text
(csrc/corrective_smooth.h: dsu_corrective_bind_host, dsu_corrective_smooth_host) against the numpy
restatement of the rule (tests/corrective_ref.py) bit for bit, on the edges of the rule, under rigid
motion, and on the crease it is there to repair.

Rigid invariance: the bound per coordinate is 2^-24 |ref| + C (iterations + 2) 2^-24 max|x|.  C was
measured on the restatement over RIGID_CASES (both meshes, iterations 1, 2, 5, 10, 30, factor 0.5 and
1, the identity and one general rigid transform): the largest value is 0.6237 (the tube, 10
iterations, factor 1; the identity alone stays below 1e-10), and C is fixed at 4 x that, 2.4948.

The crease (a tube bound rigidly, half to each of two joints, joint 1 turned about x; linear
skinning, factor 0.5, 10 iterations), largest edge stretch corrected / skinned: 0.152 / 0.580 at 30
degrees, 0.371 / 0.826 at 60, 0.650 / 1.108 at 90."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import corrective_ref as CR
import skin_ref as R
from drawingspinup_amd import _lib, ops
from drawingspinup_amd.animate.corrective import smoothing_topology

C_MEASURED = 0.6237
C_RIGID = 4 * C_MEASURED
RIGID_CASES = [(mesh, it, lam) for mesh in ("tube", "icosphere") for it in (1, 2, 5, 10, 30) for lam in (0.5, 1.0)]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    v, f = {"tube": CR.tube, "icosphere": CR.icosphere}[name]()
    return v, f, smoothing_topology(v, f)


@functools.lru_cache(maxsize=None)
def _split():
    v, f, origin = CR.split_tube()
    return v, f, origin, smoothing_topology(v, f)


def _row(topo, which, v):
    ptr, cols = (topo["nbr_rowptr"], topo["nbr_cols"]) if which == "nbr" else (topo["cor_rowptr"], topo["cor_faces"])
    return cols[ptr[v]:ptr[v + 1]]


# ------------------------------------------------------------------ topology
@pytest.mark.parametrize("name", ["icosphere", "tube", "split"])
def test_topology_contract(name):
    if name == "split":
        v, f, origin, topo = _split()
    else:
        v, f, topo = _mesh(name)
    V = len(v)
    rep, G = topo["rep"], topo["faces"]
    for k in CR.KEYS:
        assert topo[k].dtype == np.int32, k
    assert rep.shape == (V,) and topo["nbr_rowptr"].shape == (V + 1,) and topo["cor_rowptr"].shape == (V + 1,)
    assert topo["nbr_rowptr"][0] == 0 and topo["nbr_rowptr"][-1] == len(topo["nbr_cols"])
    assert topo["cor_rowptr"][0] == 0 and topo["cor_rowptr"][-1] == len(topo["cor_faces"]) == 3 * len(G)
    assert (rep[rep] == rep).all() and (rep <= np.arange(V)).all()
    assert (np.abs(v[rep] - v).max(1) < 1e-6).all()                       # a representative is at the same place
    in_face = np.zeros(V, bool)
    in_face[G.ravel()] = True
    assert (rep[G] == G).all()                                            # faces over representatives
    pairs = set()
    for r in range(V):
        row, cor = _row(topo, "nbr", r), _row(topo, "cor", r)
        if rep[r] != r or not in_face[r]:
            assert len(row) == 0 and len(cor) == 0, r
            continue
        assert len(row) and (np.diff(row) > 0).all() and r not in row      # ascending, duplicate-free, not itself
        assert (np.diff(cor) > 0).all() and all(r in G[m] for m in cor)
        assert set(row) == set(G[cor].ravel()) - {r}
        pairs.update((r, int(c)) for c in row)
    assert all((b, a) in pairs for a, b in pairs)                          # symmetric
    if name == "split":
        n = len(CR.tube()[0])
        assert (rep[n:n + CR.RINGS] == np.arange(CR.RINGS) * CR.SEGS).all() and rep[-1] == V - 1
        assert len(_row(topo, "nbr", V - 1)) == 0 and not in_face[V - 1]   # the isolated vertex
        _, _, whole = _mesh("tube")
        for r in np.flatnonzero((rep == np.arange(V)) & in_face):
            assert np.array_equal(origin[_row(topo, "nbr", r)], _row(whole, "nbr", origin[r])), r
            assert np.array_equal(origin[G[_row(topo, "cor", r)]], whole["faces"][_row(whole, "cor", origin[r])]), r


# ------------------------------------------------------------------ the host entries
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("iterations", [1, 2, 5, 10])
@pytest.mark.parametrize("F", [1, 7])
@pytest.mark.parametrize("name", ["tube", "icosphere"])
def test_host_entries_equal_the_restatement_bit_for_bit(name, F, iterations, lam):
    v, f, topo = _mesh(name)
    assert len(v) == {"tube": 336, "icosphere": 642}[name]
    x = CR.wobble(v, F, seed=F)
    ref, rdelta, rvalid = CR.corrective(x, v, topo, lam, iterations)
    got, delta, valid = CR.host_corrective(x, v, topo, lam, iterations)
    assert valid.all() and CR.same_bits(valid, rvalid)
    assert CR.same_bits(delta, rdelta)
    assert got.dtype == np.float32 and CR.same_bits(got, ref)
    if lam > 0:
        assert not CR.same_bits(got, x)                                    # and it does something


def test_isolated_vertex_and_seam_duplicates():
    v, f, origin, topo = _split()
    wv, wf, whole = _mesh("tube")
    n = len(wv)
    xw = CR.wobble(wv, 3, seed=21)
    x = np.concatenate([xw[:, origin[:-1]], np.full((3, 1, 3), 0.25, np.float32)], 1)
    x[1, n:n + CR.RINGS] += 0.125               # a duplicate's own input does not count: its representative's does
    got, delta, valid = CR.host_corrective(x, v, topo, 0.5, 5)
    ref, rdelta, rvalid = CR.corrective(x, v, topo, 0.5, 5)
    assert CR.same_bits(got, ref) and CR.same_bits(delta, rdelta) and CR.same_bits(valid, rvalid)
    assert CR.same_bits(got[:, -1], x[:, -1]) and valid[-1] == 0           # the isolated vertex: its input
    assert not valid[n:].any() and valid[:n].all()
    assert CR.same_bits(got[:, n:n + CR.RINGS], got[:, np.arange(CR.RINGS) * CR.SEGS])
    unsplit, _, _ = CR.host_corrective(xw, wv, whole, 0.5, 5)
    assert CR.same_bits(got[:, :n], unsplit)


def test_a_frame_collapsed_to_one_point_is_returned_unchanged():
    v, f, topo = _mesh("tube")
    x = CR.wobble(v, 3, seed=4)
    x[1] = np.float32([0.3, -0.7, 0.11])
    got, delta, valid = CR.host_corrective(x, v, topo, 0.5, 5)
    assert CR.same_bits(got, CR.corrective(x, v, topo, 0.5, 5)[0])
    assert CR.same_bits(got[1], x[1]) and not CR.same_bits(got[0], x[0])


@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_one_nan_stops_at_iterations_plus_one_rings(iterations):
    v, f, topo = _mesh("tube")
    x = CR.wobble(v, 2, seed=9)
    clean, _, _ = CR.host_corrective(x, v, topo, 0.5, iterations)
    at = 10 * CR.SEGS + 3
    bad = x.copy()
    bad[1, at, 1] = np.nan
    got, _, _ = CR.host_corrective(bad, v, topo, 0.5, iterations)
    assert CR.same_bits(got, CR.corrective(bad, v, topo, 0.5, iterations)[0])
    near = CR.rings_from(f, at, len(v)) <= iterations + 1
    assert 0 < near.sum() < len(v)
    assert CR.same_bits(got[0], clean[0])
    assert CR.same_bits(got[1, near], bad[1, near])
    assert CR.same_bits(got[1, ~near], clean[1, ~near])
    assert (clean[1, near].view(np.uint32) != x[1, near].view(np.uint32)).any(1).all()   # where the clean run moves all of them


def test_factor_zero_moves_nothing():
    v, f, topo = _mesh("icosphere")
    x = CR.wobble(v, 2, seed=2)
    got, delta, valid = CR.host_corrective(x, v, topo, 0.0, 3)
    assert valid.all() and (delta == 0.0).all()
    assert CR.same_bits(got, x)


# ------------------------------------------------------------------ rigid motion
def _rigid_transforms():
    Rm = CR.rotation("Z", 33.0) @ CR.rotation("X", -71.0) @ CR.rotation("Y", 118.0)
    return [(np.eye(3), np.zeros(3)), (Rm, np.array([0.4, -0.3, 0.25]))]


@pytest.mark.parametrize("name,iterations,lam", RIGID_CASES)
def test_invariant_under_rigid_motion(name, iterations, lam):
    v, f, topo = _mesh(name)
    ref = np.stack([v.astype(np.float64) @ Rm.T + t for Rm, t in _rigid_transforms()])
    x = ref.astype(np.float32)
    got, _, valid = CR.host_corrective(x, v, topo, lam, iterations)
    assert valid.all()
    err = np.abs(got.astype(np.float64) - ref)
    scale = float(np.abs(ref).max())
    c = float((np.maximum(err - CR.EPS32 * np.abs(ref), 0.0) / ((iterations + 2) * CR.EPS32 * scale)).max())
    print(f"[corrective] {name} iterations {iterations} factor {lam}: largest error {err.max():.3e}, C {c:.4f} "
          f"(measured {C_MEASURED}, allowed {C_RIGID})")
    assert (err <= CR.bound(ref, iterations, scale, C_RIGID)).all()


# ------------------------------------------------------------------ what it is for
def test_it_reduces_the_stretch_of_a_rigidly_bound_bend():
    v, f, topo = _mesh("tube")
    infl = (v[:, 2] > 0).astype(np.int32)[:, None]                         # K = 1: joint 1 above z = 0, joint 0 below
    w = np.ones((len(v), 1), np.float32)
    for angle in (30.0, 60.0, 90.0):
        mats = np.zeros((1, 2, 3, 4))
        mats[0, 0, :, :3] = np.eye(3)
        mats[0, 1, :, :3] = R.rot("X", angle)
        skinned = R.skin_lbs(v, infl, w, mats)[0].astype(np.float32)
        got, _, _ = CR.host_corrective(skinned, v, topo, 0.5, 10)
        a, b = CR.stretch(got[0], v, f), CR.stretch(skinned[0], v, f)
        print(f"[corrective] bend {angle:.0f} degrees: largest edge stretch {a:.3f} corrected, {b:.3f} skinned")
        assert a < b


# ------------------------------------------------------------------ arguments
def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    v, f, topo = _mesh("tube")
    V, F = len(v), 2
    x = CR.wobble(v, F, seed=1)
    delta, valid = CR.host_bind(v, topo, 0.5, 2)
    t, targs = CR._topo_args(topo)
    ws = np.zeros(2 * F * V * 3, np.float32)
    out = np.zeros((F, V, 3), np.float32)
    p = CR._p
    assert lib.dsu_corrective_smooth_workspace_bytes(V, F) == 2 * F * V * 3 * 4 == ws.nbytes
    assert lib.dsu_corrective_smooth_workspace_bytes(0, 5) == 0 and lib.dsu_corrective_smooth_workspace_bytes(V, 0) == 0
    assert lib.dsu_corrective_smooth_workspace_bytes(-1, 1) == -1 and lib.dsu_corrective_smooth_workspace_bytes(V, -1) == -1
    assert lib.dsu_corrective_smooth_workspace_bytes(V, 65536) == -1

    def smooth(host, skinned=p(x), rep=p(t["rep"]), topo_args=targs, d=p(delta), ok=p(valid), nv=V, nf=F, lam=0.5, it=2,
               w=p(ws), wb=ws.nbytes, o=p(out)):
        a = (skinned, rep, *topo_args, d, ok, nv, nf, lam, it, w, wb, o)
        return lib.dsu_corrective_smooth_host(*a) if host else lib.dsu_corrective_smooth(*a, None)

    def bind(host, rest=p(v), topo_args=targs, nv=V, lam=0.5, it=2, w=p(ws), wb=ws.nbytes, d=p(delta), ok=p(valid)):
        a = (rest, *topo_args, nv, lam, it, w, wb, d, ok)
        return lib.dsu_corrective_bind_host(*a) if host else lib.dsu_corrective_bind(*a, None)

    assert smooth(True) == 0 and bind(True) == 0
    for host in (True, False):
        for bad in (dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")), dict(it=0), dict(it=256), dict(it=-1)):
            assert smooth(host, **bad) == -1, (host, bad)
            assert bind(host, **bad) == -1, (host, bad)
        for name in ("skinned", "rep", "d", "ok", "w", "o"):
            assert smooth(host, **{name: None}) == -1, (host, name)
        for name in ("rest", "w", "d", "ok"):
            assert bind(host, **{name: None}) == -1, (host, name)
        for i in (0, 1, 3, 4, 6):                                          # each pointer of the topology
            a = list(targs)
            a[i] = None
            assert smooth(host, topo_args=tuple(a)) == -1 and bind(host, topo_args=tuple(a)) == -1, (host, i)
        assert smooth(host, wb=ws.nbytes - 4) == -1 and bind(host, wb=2 * V * 3 * 4 - 4) == -1
        assert smooth(host, o=p(x)) == -1                                  # out may not be the input
        assert smooth(host, nv=-1) == -1 and smooth(host, nf=-1) == -1 and smooth(host, nf=65536) == -1
        assert bind(host, nv=-1) == -1
        # nothing to do: 0, whatever the pointers
        none = (None, None, 0, None, None, 0, None, 0)
        assert smooth(host, skinned=None, rep=None, topo_args=none, d=None, ok=None, nv=0, w=None, wb=0, o=None) == 0
        assert smooth(host, nf=0, w=None, wb=0, o=None) == 0
        assert bind(host, rest=None, topo_args=none, nv=0, w=None, wb=0, d=None, ok=None) == 0
        # ... but a bad parameter is refused even then
        assert smooth(host, nf=0, lam=2.0) == -1 and bind(host, nv=0, it=0) == -1


def test_ops_refuse_host_tensors_and_bad_shapes():
    v, f, topo = _mesh("tube")
    rest = torch.from_numpy(v)
    with pytest.raises(_lib.DsuError):
        ops.corrective_bind(rest, topo, 0.5, 2)                            # no CPU fallback
    x = torch.from_numpy(CR.wobble(v, 2, seed=1))
    delta, valid = (torch.from_numpy(a) for a in CR.host_bind(v, topo, 0.5, 2))
    with pytest.raises(_lib.DsuError):
        ops.corrective_smooth(x, topo, delta, valid, 0.5, 2)
    with pytest.raises(ValueError):
        ops.corrective_smooth(x[:, :-1], topo, delta, valid, 0.5, 2)       # another mesh's topology
    with pytest.raises(ValueError):
        ops.corrective_bind(rest[:, :2], topo, 0.5, 2)
    with pytest.raises(ValueError):
        ops.corrective_topology(dict(topo, nbr_rowptr=topo["nbr_rowptr"][:-1]), "cpu")


def test_animate_mesh_and_run_render_refuse_bad_parameters():
    from drawingspinup_amd import animate
    from drawingspinup_amd.entry import run_render
    for it, lam in ((-1, 0.5), (256, 0.5), (1.5, 0.5), (3, -0.1), (3, 2.0), (3, float("nan"))):
        with pytest.raises(ValueError):
            animate.corrective.check_parameters(it, lam)
        with pytest.raises(ValueError):
            animate.animate_mesh(None, None, None, None, None, corrective_iterations=it, corrective_factor=lam)
    animate.corrective.check_parameters(0, 0.0)
    animate.corrective.check_parameters(255, 1.0)
    for flags in (["--corrective_smooth", "-1"], ["--corrective_smooth", "256"], ["--corrective_factor", "2"],
                  ["--corrective_smooth", "3", "--corrective_factor", "-0.5"]):
        with pytest.raises(SystemExit) as e:
            run_render.run(["--data_dir", "/nonexistent", "--uid", "none", "--test", *flags])
        assert e.value.code == 2
