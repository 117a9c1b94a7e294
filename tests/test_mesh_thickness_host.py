"""The thickness map without a GPU: dsu_mesh_thickness_ortho_host (the text the kernel compiles,
csrc/mesh_thickness.h) bit-equal to the dense float64 restatement tests/mesh_thickness_ref.py, on the
cases that pin the tie rule on shared edges, the pairing, open meshes, more triangles than one LDS
tile of the kernel, and the inputs the rule ignores.  tests/test_gpu_mesh_thickness.py holds the
kernel to the host entry on the same cases (CASES below)."""
import numpy as np
import pytest

from drawingspinup_amd import ops
import mesh_thickness_ref as R


CASES = R.cases()
_REF = {}


def reference(name):
    if name not in _REF:
        _REF[name] = R.thickness(*CASES[name])
    return _REF[name]


def host(name):
    return ops.mesh_thickness_host(*CASES[name])


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_entry_is_bit_equal_to_the_restatement(name):
    got, want = host(name), reference(name)
    for g, w, what in zip(got, want, ("mid", "thickness", "count")):
        assert R.same_bits(g, w), f"{name}: {what} differs at {np.argwhere(g != w)[:4].tolist()}"


def test_cube_tie_rule_counts_a_shared_diagonal_once():
    # the samples with r == c lie exactly on the diagonal the two triangles of the top and of the
    # bottom face share
    mid, thick, count = host("a_cube")
    assert (count == 2).all() and (thick == 1.0).all() and (mid == 0.5).all()


def test_rim_outside_the_cube_is_empty():
    mid, thick, count = host("b_cube_rim")
    inner = np.zeros((6, 6), bool)
    inner[1:5, 1:5] = True
    assert (count[inner] == 2).all() and (thick[inner] == 1.0).all() and (mid[inner] == 0.5).all()
    assert (count[~inner] == 0).all() and (thick[~inner] == 0.0).all() and (mid[~inner] == 0.0).all()


def test_thickest_pair_wins_and_a_tie_goes_to_the_lower_z():
    mid, thick, count = host("c_boxes_03_05")
    assert (count == 4).all() and (thick == 0.5).all() and (mid == 2.25).all()
    mid, thick, count = host("c_boxes_05_03")
    assert (count == 4).all() and (thick == 0.5).all() and (mid == 0.25).all()
    mid, thick, count = host("c_boxes_equal")
    assert (count == 4).all() and (thick == 0.5).all() and (mid == 0.25).all()


def test_open_box_has_an_odd_count_and_no_thickness():
    mid, thick, count = host("d_open_box")
    assert (count == 1).all() and (thick == 0.0).all() and (mid == 0.0).all()


def test_icosphere_thickness_within_the_sagitta():
    """The flat faces lie in the shell 1 - s <= |p| <= 1, s = the sagitta of a face's circumscribed cap
    (1 - the distance of the face's plane from the centre, the largest over the faces; the f32
    rounding of a vertex, 2^-24, is covered by EPS).  A ray at distance rho < 1 - s from the axis
    crosses the shell twice, each crossing within e(rho) = sqrt(1 - rho^2) - sqrt((1 - s)^2 - rho^2)
    inside the sphere's: the thickness is short of 2 sqrt(1 - rho^2) by at most 2 e(rho) and |mid| is
    at most e(rho) / 2.  e grows with rho (a ray near the silhouette meets the surface at a slant),
    e(0) = s: the bound 2 s on the thickness is what this argument gives on the axis, the bound 2 s on
    mid wherever e(rho) <= 4 s; both are asserted there, and 2 e(rho) and e(rho) / 2 on every ray that
    crosses the shell."""
    EPS = 1e-6
    v, f = CASES["e_icosphere"][:2]
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    s = float((1.0 - np.abs((n * tri[:, 0]).sum(1)) / np.linalg.norm(n, axis=1)).max())
    mid, thick, count = host("e_icosphere")
    x0, y0, h, W, H = CASES["e_icosphere"][2:]
    sx, sy = np.meshgrid(R.samples(x0, W, h), R.samples(y0, H, h))
    rho2 = sx * sx + sy * sy
    through = rho2 < (1.0 - s) ** 2 - EPS
    assert through.sum() > 600 and (count[through] == 2).all()
    full = 2.0 * np.sqrt(1.0 - rho2[through])
    e = full / 2.0 - np.sqrt((1.0 - s) ** 2 - rho2[through])
    short = full - thick[through]
    print(f"[thickness] icosphere 320: sagitta {s:.4f}; thickness short of the sphere's by at most "
          f"{short.max():.4f} (largest short / 2 e {np.max(short / (2.0 * e)):.3f}); largest |mid| "
          f"{np.abs(mid[through]).max():.2e}")
    assert (short >= -EPS).all() and (short <= 2.0 * e + EPS).all()
    assert (np.abs(mid[through]) <= e / 2.0 + EPS).all()
    axis = rho2[through] == 0.0
    assert axis.sum() == 1 and (np.abs(short[axis]) <= 2.0 * s).all()
    near = e <= 4.0 * s
    assert near.sum() > 600 and (np.abs(mid[through][near]) <= 2.0 * s).all()
    assert (count[rho2 > 1.0 + EPS] == 0).all()


@pytest.mark.parametrize("n", [21, 22, 23])
def test_slabs_pick_the_thickest_of_many_pairs(n):
    _, _, depth, centre = R.slabs(n, np.random.default_rng(n))
    assert len(CASES[f"f_slabs_{n}"][1]) == 12 * n
    mid, thick, count = host(f"f_slabs_{n}")
    assert (count == 2 * n).all() and (thick == depth).all() and (mid == centre).all()


def test_ignored_inputs():
    for name in ("g_no_faces", "g_no_verts"):
        mid, thick, count = host(name)
        assert not count.any() and not thick.any() and not mid.any()
    mid, thick, count = host("g_one_column")
    assert mid.shape == (8, 1) and (count == 2).all() and (thick == 1.0).all()
    mid, thick, count = host("g_one_row")
    assert mid.shape == (1, 8) and (count == 2).all() and (thick == 1.0).all()
    mid, thick, count = host("g_broken")               # only the cube is seen
    assert (count == 2).all() and (thick == 1.0).all() and (mid == 0.5).all()


def test_entry_points_validate_their_arguments():
    v, f = CASES["a_cube"][:2]
    for bad in (dict(h=0.0), dict(h=float("nan")), dict(x0=float("inf")), dict(W=4097), dict(H=-1)):
        a = dict(x0=0.0, y0=0.0, h=0.25, W=4, H=4)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.mesh_thickness_host(v, f, **a)
    from drawingspinup_amd._lib import lib
    import ctypes as C
    p = [x.ctypes.data_as(C.c_void_p) for x in (v, f, np.zeros(16), np.zeros(16), np.zeros(16, np.int32))]
    L = lib()
    assert L.dsu_mesh_thickness_ortho_host(p[0], 8, p[1], 12, 0.0, 0.0, 0.25, 4, 4, p[2], p[3], p[4]) == 0
    assert L.dsu_mesh_thickness_ortho_host(p[0], 8, p[1], 12, 0.0, 0.0, 0.0, 4, 4, p[2], p[3], p[4]) != 0
    assert L.dsu_mesh_thickness_ortho_host(p[0], 8, p[1], 12, 0.0, 0.0, 0.25, 4097, 4, p[2], p[3], p[4]) != 0
    assert L.dsu_mesh_thickness_ortho_host(p[0], 8, p[1], 12, 0.0, 0.0, 0.25, 4, 4, None, p[3], p[4]) != 0
    assert L.dsu_mesh_thickness_ortho_host(p[0], -1, p[1], 12, 0.0, 0.0, 0.25, 4, 4, p[2], p[3], p[4]) != 0
    # the device entry refuses the same before it launches anything
    assert L.dsu_mesh_thickness_ortho(None, 8, None, 12, 0.0, 0.0, 1.0, 1, None, None, 0, 0.0, 0.0, 0.0, 4, 4,
                                      None, None, None, None) != 0
    assert L.dsu_mesh_thickness_ortho(None, 8, None, 12, 0.0, 0.0, 1.0, 0, None, None, 0, 0.0, 0.0, 0.25, 4, 4,
                                      None, None, None, None) != 0
