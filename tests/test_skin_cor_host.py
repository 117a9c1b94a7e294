"""Centre-of-rotation skinning without a GPU: the text the kernels compile (csrc/cor_blend.h through
dsu_skin_cor_centres_host and dsu_skin_cor_host) against the numpy restatement
(tests/skin_cor_ref.py), the canonical table, the blend's rigid, identity, bend and twist properties,
and the argument checks of the new entry points and keywords.

Centres: per coordinate within B = 2 (T + 1 / sigma^2 + 64) 2^-52 times the bounding-box diagonal of
the restatement (np.exp against libm's exp, the same ascending sums), `valid` equal.  Apply: bit for
bit.  Properties: the linear blend's bound of PARITY.md, (2K + 4) 2^-24 (|R||x| + |t|)."""
import ctypes
import itertools

import numpy as np
import pytest

import corrective_ref as CR
import skin_cor_ref as C
import skin_dqs_ref as D
import skin_ref as R
from drawingspinup_amd import animate, ops

P = ctypes.c_void_p


def _lib():
    from drawingspinup_amd import _lib
    return _lib.lib()


def _ptr(a):
    return P(a.ctypes.data)


def _check_centres(tag, rest, faces, joints, w, J, sigma):
    got, gv = C.host_centres(rest, faces, joints, w, J, sigma)
    ref, rv = C.centres(rest, faces, joints, w, J, sigma)
    B = C.centre_bound(rest, len(np.asarray(faces).reshape(-1, 3)), sigma)
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    print(f"[cor] {tag}: {int(gv.sum())} of {len(gv)} valid; largest |host - restatement| / B = {err / B:.4f} (B = {B:.3e})")
    assert np.array_equal(gv, rv)
    assert np.isfinite(got).all() and (got[gv == 0] == 0.0).all()
    assert err <= B
    return got, gv


# ------------------------------------------------------------------ centres
def test_one_influence_per_vertex_has_no_centre():
    v, f, joints, w, _, _ = C.mesh_case("tube", 1)
    assert joints.shape[1] == 1
    got, gv = _check_centres("tube K 1", v, f, joints, w, 9, 0.1)
    assert not gv.any() and not got.any()


@pytest.mark.parametrize("name,K,sigma", [("tube", 4, 0.1), ("tube", 4, 0.05), ("sphere", 4, 0.1), ("tube", 9, 0.1),
                                          ("sphere", 9, 0.05)])
def test_host_centres_within_the_bound_of_the_restatement(name, K, sigma):
    v, f, joints, w, _, _ = C.mesh_case(name, K)
    assert joints.shape[1] == K
    got, gv = _check_centres(f"{name} K {K} sigma {sigma}", v, f, joints, w, 9, sigma)
    assert gv.all()
    # a convex combination of centroids: inside the bounding box
    assert (got >= v.min(0) - 1e-12).all() and (got <= v.max(0) + 1e-12).all()


def test_character_case():
    v, f, infl, w, J = C.character()
    joints, cw = C.canonical(infl, w, J)
    got, gv = _check_centres("character", v, f, joints, cw, J, 0.1)
    assert gv.mean() > 0.9


def _edge_mesh():
    """The tube with five vertices appended — 336: alone on joints (7, 8) that nobody shares, without a
    face; 337: NaN; 338, 339, 340: on one line — and six faces: two with an index out of range, two of
    zero area (a repeated vertex, three collinear ones) and two at the NaN vertex; a caller's table
    with every kind of row the wrapper has to clean."""
    v, f, _, _, infl, w = C.mesh_case("tube", 4)
    infl, w = infl.copy(), w.copy()
    V0 = len(v)
    v = np.concatenate([v, [[0.3, 0.2, 0.1], [np.nan, 0.0, 0.0], [0.2, 0.0, 0.0], [0.4, 0.0, 0.0],
                            [0.3, 0.0, 0.0]]]).astype(np.float32)
    f = np.concatenate([f, [[0, 1, V0 + 5], [-1, 2, 3], [V0 + 2, V0 + 3, V0 + 4], [V0 + 2, V0 + 2, 7], [0, 1, V0 + 1],
                            [16, V0 + 1, 17]]])
    infl = np.concatenate([infl, [[7, 8, -1, -1]] + [[0, 1, 2, 3]] * 4]).astype(np.int32)
    w = np.concatenate([w, [[0.5, 0.5, 0, 0]] + [[0.25] * 4] * 4]).astype(np.float32)
    infl[infl >= 7] = 6                                                    # joints 7 and 8: vertex 336 alone
    infl[V0] = [7, 8, -1, -1]
    infl[0] = [99, infl[0, 1], -5, infl[0, 3]]                             # influences out of range
    w[1, 0], w[2, 1], w[3, 2] = 0.0, -0.25, np.nan                         # weights that are not > 0
    infl[4] = [infl[4, 0], infl[4, 0], infl[4, 2], infl[4, 0]]             # duplicate joints: added in k order
    infl[5] = infl[5, 0]                                                   # all on one joint after the merge
    return v, f, infl, w, V0


def test_edge_rows_of_the_centres():
    v, f, infl, w, V0 = _edge_mesh()
    joints, cw = C.canonical(infl, w, 9)
    got, gv = _check_centres("edge rows", v, f, joints, cw, 9, 0.1)
    assert gv[V0] == 0 and (got[V0] == 0).all()                            # no triangle shares its two joints
    assert gv[5] == 0                                                      # one joint after the merge
    assert gv[0] == 1 and gv[4] == 1 and gv[V0 + 1] == 1
    # the out-of-range, zero-area and NaN faces are skipped: the same bits without them.  The NaN vertex
    # poisons no centre, because a triangle at it has no finite area and its own row is not geometry
    kept = f[:len(f) - 6]
    again, av = C.host_centres(v, kept, joints, cw, 9, 0.1)
    assert C.same_bits(got, again) and np.array_equal(gv, av)
    # a table made elsewhere, handed straight to the entry: a weight of 0 inside a row is a zero factor,
    # its pairs contribute nothing (a vertex left with one positive weight has no centre)
    zj, zw = joints.copy(), cw.copy()
    zw[10, 1], zw[11, 0] = 0.0, 0.0
    zw[12, 1:] = 0.0
    zgot, zgv = _check_centres("zero weights inside rows", v, f, zj, zw, 9, 0.1)
    assert zgv[12] == 0 and zgv[10] == 1 and not C.same_bits(zgot[10], got[10])
    # T = 0: nothing valid, no pointer to the faces needed
    none, nv = C.host_centres(v, np.zeros((0, 3), np.int32), joints, cw, 9, 0.1)
    assert not nv.any() and not none.any()
    ref0, rv0 = C.centres(v, np.zeros((0, 3), np.int64), joints, cw, 9, 0.1)
    assert not rv0.any() and not ref0.any()


def test_wrapper_makes_the_canonical_table():
    v, f, infl, w, V0 = _edge_mesh()
    for J in (9, 7, 2):
        joints, cw = C.canonical(infl, w, J)
        gj, gw = ops.skin_cor_table(infl, w, J)
        assert gj.dtype == np.int32 and gw.dtype == np.float32
        assert np.array_equal(gj, joints) and C.same_bits(gw, cw), J
        n = (joints >= 0).sum(1)
        for row in range(len(joints)):
            assert (np.diff(joints[row, :n[row]]) > 0).all() and (joints[row, n[row]:] == -1).all()
            assert (cw[row, :n[row]] > 0).all() and (cw[row, n[row]:] == 0).all()
    joints, cw = C.canonical(infl, w, 9)
    at = np.flatnonzero(joints[4] == infl[4, 0])
    assert len(at) == 1 and (joints >= 0).sum(1).max() <= 4
    dup = (w[4, 0].astype(np.float64) + w[4, 1].astype(np.float64)) + w[4, 3].astype(np.float64)
    assert cw[4, at[0]] == np.float32(dup) and (joints[4] >= 0).sum() == 2
    # a canonical table is its own canonical table
    j2, w2 = ops.skin_cor_table(joints, cw, 9)
    assert np.array_equal(j2, joints) and C.same_bits(w2, cw)
    # nothing contributes: one column of padding
    j0, w0 = ops.skin_cor_table(np.full((3, 2), -1), np.ones((3, 2), np.float32), 4)
    assert j0.shape == (3, 1) and (j0 == -1).all() and not w0.any()


def test_vertices_with_equal_rows_get_equal_bits():
    """A seam-split export: the copies along the cut carry their originals' weights."""
    v, f, origin = CR.split_tube()
    base_i, base_w = C.smooth_weights(CR.tube()[0], 4, 9, 9)
    infl = np.concatenate([base_i[origin[:-1]], [[0, 1, 2, 3]]]).astype(np.int32)
    w = np.concatenate([base_w[origin[:-1]], [[0.25] * 4]]).astype(np.float32)
    joints, cw = C.canonical(infl, w, 9)
    got, gv = C.host_centres(v, f, joints, cw, 9, 0.1)
    dup = np.arange(len(CR.tube()[0]), len(v) - 1)
    assert len(dup) == CR.RINGS and gv[dup].all()
    assert C.same_bits(got[dup], got[origin[dup]])


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("name,K,F", [("tube", 1, 1), ("tube", 4, 7), ("sphere", 4, 1), ("tube", 9, 1), ("sphere", 9, 7)])
def test_host_apply_equals_the_restatement_bit_for_bit(name, K, F):
    a = C.apply_case(name, K, F, seed=K * 100 + F)
    got = C.host_cor(*a)
    ref, _ = C.skin_cor(*a)
    n = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"[cor] {name} K {K} F {F}: {n} of {got.size} coordinates differ from the restatement; "
          f"{int(a[6].sum())} of {len(a[6])} centres valid")
    assert C.same_bits(got, ref)
    assert np.abs(got - a[0][None]).max() > 0.1                                 # it moved
    assert bool(a[6].any()) == (K > 1)


def test_edge_rows_of_the_apply():
    rest, infl, w, mats, quats, cen, val, linear_rows = C.edge_rows()
    got = C.host_cor(rest, infl, w, mats, quats, cen, val)
    ref, _ = C.skin_cor(rest, infl, w, mats, quats, cen, val)
    assert C.same_bits(got, ref)
    # the rows that fall back: the bytes of the same call with nothing valid
    lin = C.host_cor(rest, infl, w, mats, quats, cen, np.zeros_like(val))
    for row in linear_rows:
        assert C.same_bits(got[:, row], lin[:, row]), row
    assert not got[:, 2].any()                                                  # no influence: L = 0
    moved = np.setdiff1d(np.arange(len(rest)), linear_rows)
    assert np.isfinite(got[:, moved]).all()
    # row 3 has one transform on both joints, so its linear blend is that transform too
    assert all(not C.same_bits(got[:, r], lin[:, r]) for r in moved if r != 3)
    one = lambda r, cols: C.host_cor(rest[r:r + 1], infl[r:r + 1, cols], w[r:r + 1, cols], mats, quats, cen[r:r + 1],
                                     val[r:r + 1])[:, 0]
    assert C.same_bits(got[:, 0], one(0, [2, 3]))                               # invalid influences contribute nothing
    assert C.same_bits(got[:, 1], one(1, [1, 2, 3]))                            # the pivot is the second influence
    assert C.same_bits(got[:, 5], one(5, [0, 3]))                               # negative and NaN weights
    # row 3: q and -q are the same rotation and add: joint 7's rigid transform
    x = rest[3].astype(np.float64)
    rigid = mats[:, 7, :, :3] @ x + mats[:, 7, :, 3]
    sc = np.abs(mats[:, 7, :, :3]) @ np.abs(x) + np.abs(mats[:, 7, :, 3])
    assert (np.abs(got[:, 3] - rigid) <= D.bound(rigid, sc)).all()


def test_negating_quaternions_changes_no_bit():
    J = 4
    v, f, joints, cw, infl, w = C.mesh_case("tube", 4, J)
    cen, val = C.host_centres(v, f, joints, cw, J, 0.1)
    assert val.all()
    mats = D.random_transforms(np.random.default_rng(78), 2, J)
    quats = C.quats_of(mats)
    want = C.host_cor(v, infl, w, mats, quats, cen, val)
    for n in range(J + 1):
        for subset in itertools.combinations(range(J), n):                     # all 16, the pivots' included
            q = quats.copy()
            q[:, list(subset)] *= -1.0
            assert C.same_bits(C.host_cor(v, infl, w, mats, q, cen, val), want), subset
    q = quats.copy()
    q[0, 1] *= -1.0
    assert C.same_bits(C.host_cor(v, infl, w, mats, q, cen, val), want)


# ------------------------------------------------------------------ properties
def _linear_bound(K, mats, x):
    """(2K + 4) 2^-24 (|R||x| + |t|) per (frame, vertex, coordinate) for one transform per frame."""
    scale = np.einsum("fab,vb->fva", np.abs(mats[:, 0, :, :3]), np.abs(x)) + np.abs(mats[:, None, 0, :, 3])
    return (2 * K + 4) * C.EPS32 * scale


@pytest.mark.parametrize("name,K", [("tube", 1), ("tube", 4), ("sphere", 9)])
def test_one_transform_on_every_joint_gives_that_rigid_transform(name, K):
    v, infl, w, mats, _, cen, val = C.apply_case(name, K, 5, seed=190 + K)
    mats = mats.copy()
    mats[:] = mats[:, :1]
    got = C.host_cor(v, infl, w, mats, C.quats_of(mats), cen, val).astype(np.float64)
    x = v.astype(np.float64)
    rigid = np.einsum("fab,vb->fva", mats[:, 0, :, :3], x) + mats[:, None, 0, :, 3]
    ratio = np.abs(got - rigid) / _linear_bound(K, mats, x)
    print(f"[cor] {name} K {K}: largest |got - rigid| / bound {float(ratio.max()):.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("name,K", [("tube", 4), ("sphere", 9)])
def test_identity_clip_gives_the_rest_mesh_within_the_linear_bound(name, K):
    """Under identity transforms M = 0 and r_v = 0 exactly, so out = x + 0: every vertex with a centre is
    expected to return its rest position (the count of coordinates that differ in bits is printed, not
    asserted; the bound is).  Both meshes have coordinates that are exactly 0 or next to it (the tube's
    y = r sin(k pi / 8) at the multiples of pi, about 1e-17), where the bound relative to |x_c| is 0 or
    next to it: the form L(p*) + d', which leaves (sum w - 1) p*_c there, cannot meet it."""
    v, infl, w, mats, _, cen, val = C.apply_case(name, K, 2, seed=3)
    mats = np.zeros_like(mats)
    mats[..., :3] = np.eye(3)
    got = C.host_cor(v, infl, w, mats, C.quats_of(mats), cen, val)
    want = np.ascontiguousarray(np.broadcast_to(v, got.shape))
    n = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    err = np.abs(got.astype(np.float64) - want)
    bound = _linear_bound(K, mats, v.astype(np.float64))
    out = err > bound
    print(f"[cor] identity {name} K {K}: {n} of {got.size} coordinates differ in bits from the rest mesh; "
          f"{int(out.sum())} outside the bound, largest |x_c| among them "
          f"{float(np.abs(want[out]).max()) if out.any() else 0.0:.2e} ({int((want[out] == 0).sum())} exactly 0), "
          f"largest error {float(err.max()):.2e}, largest error / bound elsewhere "
          f"{float((err[~out] / np.maximum(bound[~out], 1e-300)).max()):.3f}")
    assert not out.any()


def _tube_outputs(mats):
    """The float64 restatements of the three blends on the bend tube."""
    v, f, infl, w = C.bend_tube()
    joints, cw = C.canonical(infl, w, 2)
    cen, val = _tube_centres()
    _, cor = C.skin_cor(v, infl, w, mats, C.quats_of(mats), cen, val)
    _, dqs, _ = D.skin_dqs(v, infl, w, animate.dual_quaternions(mats))
    lbs, _ = R.skin_lbs(v, infl, w, mats.astype(np.float32))
    return v.astype(np.float64), cor[0], dqs[0], lbs[0]


_TUBE = {}


def _tube_centres():
    if "c" not in _TUBE:
        v, f, infl, w = C.bend_tube()
        joints, cw = C.canonical(infl, w, 2)
        _TUBE["c"] = C.centres(v, f, joints, cw, 2, 0.1)
    return _TUBE["c"]


def _tube_host(mats, ref64):
    """The same clip through the shipped text: dsu_skin_cor_centres_host within B of the restatement's
    centres with `valid` equal, dsu_skin_cor_host on the restatement's centres bit-equal to the
    restatement, then the host apply on the host centres.  -> (that output as float64, the f32
    rounding of a coordinate: 2^-24 of the largest, plus the centres' B carried through a rotation)."""
    v, f, infl, w = C.bend_tube()
    joints, cw = C.canonical(infl, w, 2)
    cen, val = _tube_centres()
    if "h" not in _TUBE:
        _TUBE["h"] = C.host_centres(v, f, joints, cw, 2, 0.1)
    hcen, hval = _TUBE["h"]
    B = C.centre_bound(v, len(f), 0.1)
    assert np.array_equal(hval, val) and np.abs(hcen - cen).max() <= B
    quats = C.quats_of(mats)
    ref32, _ = C.skin_cor(v, infl, w, mats, quats, cen, val)
    assert C.same_bits(C.host_cor(v, infl, w, mats, quats, cen, val), ref32)
    got = C.host_cor(v, infl, w, mats, quats, hcen, hval)[0].astype(np.float64)
    tol = C.EPS32 * float(np.abs(ref64).max()) + 4.0 * B
    assert np.abs(got - ref64).max() <= tol
    return got, tol


def _ring_distances(p):
    rings = p.reshape(C.TUBE_RINGS, C.TUBE_SEGS, 3)
    return np.linalg.norm(rings[:, :, None] - rings[:, None, :], axis=-1)


@pytest.mark.parametrize("deg", [90.0, 120.0])
def test_bend_tube_keeps_its_rings_and_bulges_less(deg):
    mats = C.two_joint_clip("Z", deg)
    x, cor, dqs, lbs = _tube_outputs(mats)
    cen, val = _tube_centres()
    mixed = val.reshape(C.TUBE_RINGS, C.TUBE_SEGS)
    assert (mixed.all(1) | ~mixed.any(1)).all() and 5 <= mixed.all(1).sum() < C.TUBE_RINGS
    # every ring of equal weights moves rigidly; the linear blend's shrinks
    rest_d = _ring_distances(x)
    cor_err = float(np.abs(_ring_distances(cor) - rest_d).max())
    lbs_err = float(np.abs(_ring_distances(lbs) - rest_d).max())
    assert cor_err <= 1e-9 and lbs_err > 1e-2
    r = C.TUBE_R
    far = {k: float(C.axis_distance(p, mats).max()) / r for k, p in (("cor", cor), ("dqs", dqs), ("lbs", lbs))}
    near = {k: float(C.axis_distance(p, mats).min()) / r for k, p in (("cor", cor), ("dqs", dqs), ("lbs", lbs))}
    radius = {k: float(np.linalg.norm(p.reshape(C.TUBE_RINGS, C.TUBE_SEGS, 3) -
                                      p.reshape(C.TUBE_RINGS, C.TUBE_SEGS, 3).mean(1, keepdims=True), axis=-1).min()) / r
              for k, p in (("cor", cor), ("dqs", dqs), ("lbs", lbs))}
    print(f"[cor] bend {deg:.0f}: ring congruence error {cor_err:.2e} (linear {lbs_err:.2e}); smallest ring radius / r "
          f"lbs {radius['lbs']:.3f} dqs {radius['dqs']:.3f} cor {radius['cor']:.3f}; largest distance from the bent "
          f"axis / r lbs {far['lbs']:.3f} dqs {far['dqs']:.3f} cor {far['cor']:.3f}; smallest lbs {near['lbs']:.3f} "
          f"dqs {near['dqs']:.3f} cor {near['cor']:.3f}")
    assert far["cor"] < far["dqs"]
    assert near["cor"] > near["lbs"]
    # the same properties of the host entries' f32 output: a distance between two rounded points is off
    # by at most 2 sqrt(3) tol, and the orderings' margins (>= 0.04 r) are far above it
    host, tol = _tube_host(mats, cor)
    host_err = float(np.abs(_ring_distances(host) - rest_d).max())
    print(f"[cor] bend {deg:.0f}, host entries: ring congruence error {host_err:.2e} (f32 rounding allows "
          f"{2 * 3 ** 0.5 * tol:.2e}); largest / smallest distance from the bent axis / r "
          f"{float(C.axis_distance(host, mats).max()) / r:.3f} / {float(C.axis_distance(host, mats).min()) / r:.3f}")
    assert host_err <= 2 * 3 ** 0.5 * tol
    assert float(C.axis_distance(host, mats).max()) / r < far["dqs"]
    assert float(C.axis_distance(host, mats).min()) / r > near["lbs"]


@pytest.mark.parametrize("deg", [120.0, 178.0])
def test_pure_twist_equals_the_dual_quaternion_blend(deg):
    """Both joints fix the tube's axis, the centres lie on it, and the two blends are the same rotation."""
    mats = C.two_joint_clip("Y", deg)
    x, cor, dqs, lbs = _tube_outputs(mats)
    err = float(np.abs(cor - dqs).max())
    radius = lambda p: np.hypot(p[:, 0], p[:, 2])
    print(f"[cor] twist {deg:.0f}: largest |cor - dqs| {err:.2e}; ring radius / r cor {radius(cor).min() / C.TUBE_R:.3f} "
          f"lbs {radius(lbs).min() / C.TUBE_R:.3f}")
    assert err <= 1e-12
    assert np.abs(radius(cor) - radius(x)).max() <= 1e-12
    # the host entries' f32 output: the dual-quaternion restatement's float64 value within its one rounding
    host, tol = _tube_host(mats, cor)
    host_err = float(np.abs(host - dqs).max())
    print(f"[cor] twist {deg:.0f}, host entries: largest |host - dqs| {host_err:.2e} (f32 rounding allows {tol + 1e-12:.2e})")
    assert host_err <= tol + 1e-12
    assert np.abs(radius(host) - radius(x)).max() <= 2 ** 0.5 * tol + 1e-12


# ------------------------------------------------------------------ arguments
def test_entry_points_validate_without_a_gpu():
    lib = _lib()
    v, f, joints, cw, infl, w = C.mesh_case("tube", 4)
    f32 = np.ascontiguousarray(f, np.int32)
    V, T = len(v), len(f32)
    cen, val = np.zeros((V, 3)), np.zeros(V, np.uint8)
    a = [_ptr(v), _ptr(f32), _ptr(joints), _ptr(cw)]
    assert lib.dsu_skin_cor_centres_host(*a, V, T, 4, 9, 0.1, _ptr(cen), _ptr(val)) == 0
    nbytes = lib.dsu_skin_cor_centres_workspace_bytes(V, T, 4, 9)
    parts, per, tile = C.plan(V, T)
    rw = min(12, 9)
    assert nbytes == (parts * V * 4 + T * 4 + T * rw) * 8 + (T + T * rw + 1) // 2 * 8
    # whole doubles also where the int32 part is odd: T odd, rw = min(3K, J) even
    assert lib.dsu_skin_cor_centres_workspace_bytes(V, 63, 4, 19) % 8 == 0
    assert lib.dsu_skin_cor_centres_workspace_bytes(V, 63, 4, 19) >= (parts * V * 4 + 63 * 16) * 8 + 63 * 13 * 4
    ws = np.zeros(nbytes // 8 + 1)
    for i in range(4):                                                          # each null pointer
        b = list(a)
        b[i] = None
        assert lib.dsu_skin_cor_centres_host(*b, V, T, 4, 9, 0.1, _ptr(cen), _ptr(val)) == -1
        assert lib.dsu_skin_cor_centres(*b, V, T, 4, 9, 0.1, _ptr(ws), nbytes, _ptr(cen), _ptr(val), None) == -1
    assert lib.dsu_skin_cor_centres_host(*a, V, T, 4, 9, 0.1, None, _ptr(val)) == -1
    assert lib.dsu_skin_cor_centres_host(*a, V, T, 4, 9, 0.1, _ptr(cen), None) == -1
    assert lib.dsu_skin_cor_centres(*a, V, T, 4, 9, 0.1, None, nbytes, _ptr(cen), _ptr(val), None) == -1
    assert lib.dsu_skin_cor_centres(*a, V, T, 4, 9, 0.1, _ptr(ws), nbytes - 1, _ptr(cen), _ptr(val), None) == -1
    for Vb, Tb, K, J, sg in ((-1, T, 4, 9, 0.1), (V, -1, 4, 9, 0.1), (V, T, 0, 9, 0.1), (V, T, 4097, 9, 0.1),
                             (V, T, 4, 0, 0.1), (V, T, 4, 9, 0.0), (V, T, 4, 9, -0.1), (V, T, 4, 9, float("nan")),
                             (V, T, 4, 9, 1e-200), ((1 << 26) + 1, T, 4, 9, 0.1)):
        assert lib.dsu_skin_cor_centres_host(*a, Vb, Tb, K, J, sg, _ptr(cen), _ptr(val)) == -1, (Vb, Tb, K, J, sg)
        assert lib.dsu_skin_cor_centres(*a, Vb, Tb, K, J, sg, _ptr(ws), nbytes, _ptr(cen), _ptr(val), None) == -1
    assert lib.dsu_skin_cor_centres_workspace_bytes(V, T, 0, 9) == -1
    assert lib.dsu_skin_cor_centres_host(None, None, None, None, 0, 0, 4, 9, 0.1, None, None) == 0
    assert lib.dsu_skin_cor_centres(None, None, None, None, 0, 0, 4, 9, 0.1, None, 0, None, None, None) == 0
    # the apply
    mats = D.random_transforms(np.random.default_rng(1), 1, 9)
    quats = C.quats_of(mats)
    out = np.zeros((1, V, 3), np.float32)
    a = [_ptr(v), _ptr(infl), _ptr(w), _ptr(mats), _ptr(quats), _ptr(cen), _ptr(val)]
    assert lib.dsu_skin_cor_host(*a, V, 4, 1, 9, _ptr(out)) == 0
    for i in range(7):
        b = list(a)
        b[i] = None
        assert lib.dsu_skin_cor_host(*b, V, 4, 1, 9, _ptr(out)) == -1
        assert lib.dsu_skin_cor(*b, V, 4, 1, 9, _ptr(out), None) == -1
    assert lib.dsu_skin_cor_host(*a, V, 4, 1, 9, None) == -1
    assert lib.dsu_skin_cor(*a, V, 4, 1, 9, None, None) == -1
    for Vb, K, F, J in ((-1, 4, 1, 9), (V, 0, 1, 9), (V, 4097, 1, 9), (V, 4, 0, 9), (V, 4, 65536, 9), (V, 4, 1, 0)):
        assert lib.dsu_skin_cor_host(*a, Vb, K, F, J, _ptr(out)) == -1
        assert lib.dsu_skin_cor(*a, Vb, K, F, J, _ptr(out), None) == -1
    assert lib.dsu_skin_cor_host(*[None] * 7, 0, 4, 1, 9, None) == 0
    assert lib.dsu_skin_cor(*[None] * 7, 0, 4, 1, 9, None, None) == 0
    assert lib.dsu_abi_version() == 3


def test_ops_refuse_host_tensors_and_bad_shapes():
    import torch
    from drawingspinup_amd import _lib
    v, infl, w, mats, quats, cen, val = C.apply_case("tube", 4, 1, seed=2)
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in (v, infl, w, mats, quats, cen, val)]
    with pytest.raises(_lib.DsuError):
        ops.skin_cor(*t)                                                        # no CPU fallback
    with pytest.raises(ValueError):
        ops.skin_cor(t[0], t[1], t[2], t[3], t[4][:, :, :3], t[5], t[6])
    with pytest.raises(ValueError):
        ops.skin_cor(t[0], t[1], t[2], t[3], t[4], t[5][:-1], t[6])
    with pytest.raises(_lib.DsuError):
        ops.skin_cor_centres(t[0], torch.from_numpy(np.ascontiguousarray(CR.tube()[1], np.int32)), infl, w, 9)
    with pytest.raises(ValueError):
        ops.skin_cor_centres(t[0], torch.zeros((0, 3), dtype=torch.int32), infl[:-1], w[:-1], 9)


def test_the_python_layers_know_the_third_blend(tmp_path, capsys):
    from drawingspinup_amd.entry import run_render
    assert animate.skin.SKINNING == ("linear", "dual_quaternion", "centre_of_rotation")
    assert animate.skin.COR_SIGMA == 0.1 and callable(animate.cor_centres)
    v, f = R.capsule((0, 0, 0), (0, 0.3, 0), 0.05)
    sk = animate.Skeleton(["a", "b"], [-1, 0], [[0, 0, 0], [0, 0.3, 0]])
    with pytest.raises(ValueError, match="centre_of_rotation"):
        animate.animate_mesh(v, f, R.vertex_colours(len(v), 1), sk, animate.rest_clip(sk), skinning="cubic",
                             device="cuda:0")
    # the accepted value gets as far as looking for the mesh
    with pytest.raises(FileNotFoundError):
        run_render.run(["--data_dir", str(tmp_path), "--uid", "none", "--test", "--skinning", "centre_of_rotation"])
    capsys.readouterr()
