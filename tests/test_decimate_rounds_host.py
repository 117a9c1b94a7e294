"""The round checker of the device decimation (oracle/decimate_rounds_ref.py) tested on the host:
it accepts honest rounds of the plain simulation on every mesh the GPU tests use, rejects every
mutant with the violated rule named, and the share of collapses whose branch decision is fragile
stays under the cap on those meshes.  Plus the seeded serial finish (dsu_mesh_decimate_quadric_q),
which remesh hands the device rounds' result to, called directly."""
import functools

import numpy as np
import pytest
import torch

from drawingspinup_amd.nsr import mesh as M
from oracle import decimate_ref as D
from oracle import decimate_rounds_ref as R
from tests.test_export_host import _canonical, _grid, _uv_sphere

FRAGILE_CAP = 0.02
MESHES = ("sphere", "bump", "lattice", "torus", "pinched", "tiny")


def _jittered_sphere(seed=11):
    rng = np.random.default_rng(seed)
    v, f = _uv_sphere(40, 30)
    return v * (1 + 0.15 * rng.normal(size=(len(v), 1))) + 0.01 * rng.normal(size=v.shape), f


def _marching(field):
    c = torch.linspace(-1, 1, 28, dtype=torch.float64)
    v, f = M.marching_cubes(field(*torch.meshgrid(c, c, c, indexing="ij")), 0.0)
    return v.numpy().copy(), f.numpy().copy()


@functools.lru_cache(None)
def decimation_meshes(name):
    """-> tuple of (verts float64, faces int64): the meshes of the round tests (one per name, four for
    `tiny`).  Cached: treat as read-only."""
    if name == "sphere":                       # closed, general position, poles of degree 40
        out = [_jittered_sphere()]
    elif name == "bump":                       # open boundary: boundary planes, one-face collapses
        rng = np.random.default_rng(12)
        v, f = _grid(33, lambda x, y: 0.2 * np.exp(-(x * x + y * y) / (2 * 0.05 ** 2)))
        out = [(v + 0.002 * rng.normal(size=v.shape), f)]
    elif name == "lattice":                    # the workload's regularity: equal costs, near-planar quadrics
        out = [_marching(lambda x, y, z: 0.9 - torch.sqrt((x / 0.95) ** 2 + (y / 0.8) ** 2 + (z / 0.9) ** 2)
                         + 0.08 * torch.sin(9 * x) * torch.sin(7 * y + 1) * torch.sin(8 * z + 2))]
    elif name == "torus":                      # genus 1: the link rules fire
        out = [_marching(lambda x, y, z: 0.3 - torch.sqrt((torch.sqrt(x * x + y * y) - 0.6) ** 2 + z * z))]
    elif name == "pinched":                    # a non-manifold vertex and a fan of three triangles on one edge
        v, f = _jittered_sphere()
        v2, f2 = _jittered_sphere(13)
        v2 = v2 + (v[-1] - v2[0])               # the second copy's north pole on the first's south pole
        lut = np.concatenate([[len(v) - 1], len(v) + np.arange(len(v2) - 1)])
        n = len(v) + len(v2) - 1
        fan_v = np.array([[2, 0, 0], [2, 0, 0.3], [2.2, 0.01, 0.1], [1.9, 0.2, 0.15], [1.95, -0.2, 0.17]])
        fan_f = np.array([[n, n + 1, n + 2], [n, n + 1, n + 3], [n + 1, n, n + 4]])
        out = [(np.concatenate([v, v2[1:], fan_v]), np.concatenate([f, lut[f2], fan_f]))]
    elif name == "tiny":
        tet = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64),
               np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))
        ov = np.array([[1, 0, 0], [-1, 0.1, 0], [0, 1, 0.1], [0.1, -1, 0], [0, 0.05, 1], [0.02, 0, -1.1]], np.float64)
        of = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
        two = (np.array([[0, 0, 0], [1, 0, 0.1], [1, 1, 0], [0, 1, 0.2]], np.float64), np.array([[0, 1, 2], [0, 2, 3]]))
        out = [tet, (ov, of), two, (two[0][:3].copy(), two[1][:1].copy())]
    for v, f in out:
        v.setflags(write=False)
        f.setflags(write=False)
    return tuple((v, f.astype(np.int64)) for v, f in out)


def round_budget(n_faces):
    """stop and floor of the round tests: stop = n_faces / 4, floor = 0.8 stop"""
    stop = n_faces // 4
    return stop, int(stop * 0.8)


@functools.lru_cache(None)
def _simulated(name, part, keep):
    """three honest rounds on a mesh: [(v, f, Q)] with the initial state first"""
    v, f = decimation_meshes(name)[part]
    floor = round_budget(len(f))[1]
    rng = np.random.default_rng(5)
    states = [(v, f, R.init_quadrics(v, f, 1.0)[0])]
    for _ in range(3):
        states.append(R.simulate_round(*states[-1], lambda nf, ne: R.n_candidates(nf, ne, floor), rng,
                                       keep_manifold=keep))
    return states, floor


@pytest.mark.parametrize("name", MESHES)
def test_checker_accepts_honest_rounds_and_few_are_fragile(name):
    n_collapses = n_fragile = 0
    for part in range(len(decimation_meshes(name))):
        for keep in (True, False):
            states, floor = _simulated(name, part, keep)
            for before, after in zip(states, states[1:]):
                if R.has_twin_faces(before[1]):
                    break
                cs, nfr = R.check_round(*before, *after, floor_faces=floor, keep_manifold=keep)
                assert len(cs) == len(set(np.unique(before[1])) - set(np.unique(after[1])))
                n_collapses += len(cs)
                n_fragile += nfr
    print("%s: %d collapses, %d fragile" % (name, n_collapses, n_fragile))
    assert n_collapses > 0
    assert n_fragile <= FRAGILE_CAP * n_collapses


def test_float64_rounding_of_the_initial_quadrics_against_the_bound():
    """16 eps sum|terms| is the bound stated for the device quadrics.  The definition evaluated in
    plain float64 (same formula, numpy's order) fits it on the jittered meshes and misses it on the
    marching-cubes ones (see init_quadrics_bound, which raises the bound by what this evaluation
    needs, times 4): the figures are printed, and a need beyond 2 would mean a wrong reference."""
    for name in MESHES:
        for v, f in decimation_meshes(name):
            for bw in (0.0, 1.0):
                need = R.init_quadrics_bound(v, f, bw)[2]
                print("%s bw %g: float64 / (16 eps sum|terms|) = %.3f" % (name, bw, need))
                assert need <= 2.0


EXPECT = {"adjacent": "independence", "no_link": "admissibility", "no_flip": "admissibility", "wrong_sum": "quadrics",
          "midpoint": "target", "move_ring": "untouched data", "beyond_budget": "candidacy"}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_checker_rejects_the_mutant_and_names_the_rule(mutant):
    """Every round of the mutant that the checker refuses, it refuses for the rule the mutant
    breaks, and on at least one mesh it refuses.  (A round of `no_flip`, `no_link` or `midpoint`
    in which no collapse needed the rule is an honest round.)"""
    named = []
    for name in MESHES:
        for part in range(len(decimation_meshes(name))):
            states, floor = _simulated(name, part, True)
            before = states[0]
            after = R.simulate_round(*before, lambda nf, ne: R.n_candidates(nf, ne, floor), np.random.default_rng(7),
                                     mutate=mutant)
            try:
                R.check_round(*before, *after, floor_faces=floor, keep_manifold=True)
            except R.RoundViolation as e:
                assert e.rule == EXPECT[mutant], str(e)
                assert EXPECT[mutant] in str(e)
                named.append((name, e.rule))
    print(mutant, named)
    assert any(rule == EXPECT[mutant] for _, rule in named)
    if mutant in ("adjacent", "wrong_sum", "move_ring", "beyond_budget"):       # break a rule in every round
        assert {n for n, _ in named} >= {"sphere", "bump", "lattice", "torus", "pinched"}


def test_link_rules_refuse_every_edge_of_the_tetrahedron():
    """what `no_link` switches off is needed: with the link test every edge of the tetrahedron is refused"""
    v, f = decimation_meshes("tiny")[0]
    Q = R.init_quadrics(v, f, 1.0)[0]
    v2, f2, Q2 = R.simulate_round(v, f, Q, lambda nf, ne: 6, np.random.default_rng(0))
    assert np.array_equal(f2, f) and np.array_equal(v2, v)


# ------------------------------------------------------------------------------------------------
# dsu_mesh_decimate_quadric_q, the seeded serial finish
# ------------------------------------------------------------------------------------------------
def _small(closed):
    rng = np.random.default_rng(11)
    if closed:
        v, f = _uv_sphere(10, 8)
        return v * (1 + 0.15 * rng.normal(size=(len(v), 1))) + 0.01 * rng.normal(size=v.shape), f, 60
    v, f = _grid(7, lambda x, y: 0.3 * np.sin(3 * x) * np.cos(2 * y))
    return v + 0.02 * rng.normal(size=v.shape), f, 30


@pytest.mark.parametrize("closed", [True, False])
def test_seeded_finish_from_the_initial_quadrics_is_the_unseeded_queue(closed):
    """Seeded with the initial quadrics of the definition, the queue takes the collapses it takes
    when it builds them itself: the same faces, bit for bit.  The positions cannot be bit-equal: the
    seed is the long-double sum rounded once, the library's own sum rounds at every plane, so the
    quadrics differ in their last bits.  Bound: an accumulated quadric is a sum of p planes (p <= 64
    on these meshes), so its entries differ by at most p eps sum|terms| between the two runs; a
    minimiser -A^-1 b moves by at most cond(A) times the relative change of A and of b, times |x|:
    2 p eps cond(A) |x|, and as much again for the two solves' own rounding: 256 eps cond(A) |x|,
    with the largest cond(A) among the output vertices' accumulated quadrics (from the naive
    restatement, which takes the same collapses) and the largest |x|.  Observed: 1e-15."""
    v, f, target = _small(closed)
    f32 = np.ascontiguousarray(f.astype(np.int32))
    Q = np.ascontiguousarray(R.init_quadrics(v, f, 1.0)[0])
    for keep in (True, False):
        wv, wf = M._remesh_host(v, f32, target, 1.0, keep)
        gv, gf = M._remesh_host(v, f32, target, 1.0, keep, quadrics=Q)
        assert np.array_equal(gf, wf) and gv.shape == wv.shape
        quads = D.decimate(v, f, target, 1.0, keep, return_quadrics=True)[3]
        bound = 256 * R.EPS * max(np.linalg.cond(q[:3, :3]) for q in quads) * np.abs(wv).max()
        err = np.abs(gv - wv).max()
        print("seeded vs unseeded: largest difference %.3g, bound %.3g" % (err, bound))
        assert err <= bound < 1e-9
        assert _canonical(gv, gf) == _canonical(wv, wf)


def seeded_finish_matches_the_oracle(v, f, Q, target, keep):
    """(v, f, Q) over compact vertex indices: dsu_mesh_decimate_quadric_q against
    decimate_ref.decimate(quadrics=...)"""
    gv, gf = M._remesh_host(np.ascontiguousarray(v), np.ascontiguousarray(f.astype(np.int32)), target, 1.0, keep,
                            quadrics=np.ascontiguousarray(Q))
    wv, wf, used = D.decimate(v, f, target, 1.0, keep, quadrics=Q)
    remap = {u: k for k, u in enumerate(used)}
    wf = np.array([[remap[i] for i in t] for t in wf])
    assert len(gf) == len(wf) and len(gv) == len(wv)
    assert _canonical(gv, gf) == _canonical(wv, wf)
    return len(gf)


def compact(v, f, Q):
    used, inv = np.unique(f.reshape(-1), return_inverse=True)
    return v[used], inv.reshape(-1, 3), Q[used]


@pytest.mark.parametrize("closed", [True, False])
def test_seeded_finish_from_accumulated_quadrics_takes_the_oracles_collapses(closed):
    v, f, target = _small(closed)
    for keep in (True, False):
        rng = np.random.default_rng(3)
        state = (v, f, R.init_quadrics(v, f, 1.0)[0])
        floor = int(1.25 * target)
        for _ in range(2):
            state = R.simulate_round(*state, lambda nf, ne: R.n_candidates(nf, ne, floor), rng, keep_manifold=keep)
        assert target < len(state[1]) < len(f)
        assert seeded_finish_matches_the_oracle(*compact(*state), target, keep) <= target
