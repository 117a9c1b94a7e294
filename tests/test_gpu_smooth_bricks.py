"""Export smoothing on the brick layout (csrc/mesh_smooth.hip, dsu_smooth_bricks_*): the band compacted
in 8^3 bricks against the band compacted voxel by voxel (`layout="slots"`) in the same build — equal
bit for bit, iteration by iteration: marching cubes' `<=` corner rule sits on the exact zeros the
projection produces."""
import numpy as np
import pytest
import torch

from drawingspinup_amd import ops
from drawingspinup_amd.nsr import mesh as M
from tests.test_gpu_mesh import _shape

pytestmark = pytest.mark.gpu

ITERS = (1, 2, 3, 10, 25)            # odd and even counts: both ping-pong outcomes


def _box_plus_sphere():
    x, y, z = torch.meshgrid(torch.arange(37), torch.arange(21), torch.arange(26), indexing="ij")
    b = ((x - 22) ** 2 + (y - 10) ** 2 + (z - 14) ** 2 <= 49)
    b[6:19, 5:15, 4:17] = True
    return b


def _slab_96():
    x, y, z = torch.meshgrid(torch.arange(96), torch.arange(40), torch.arange(24), indexing="ij")
    return ((x - 47.5) / 40) ** 2 + ((y - 19.5) / 13) ** 2 + ((z - 11.5) / 6) ** 2 <= 1.0


def _against_three_faces():
    b = torch.zeros(20, 20, 20, dtype=torch.bool)
    b[:9, :11, :7] = True
    return b


def _plate():
    b = torch.zeros(24, 24, 24, dtype=torch.bool)
    b[8, 3:21, 3:21] = True                   # one voxel thick, across brick boundaries in y and z
    return b


def _single_voxel():
    b = torch.zeros(17, 17, 17, dtype=torch.bool)
    b[8, 8, 8] = True
    return b


def _two_blobs():
    b = torch.zeros(64, 24, 24, dtype=torch.bool)
    b[10, 12, 12] = True                      # bands in bricks 0-1 and 5-6 along x: bricks 2-4 and
    b[50, 12, 12] = True                      # the outer rings along y, z are missing neighbours
    return b


SHAPES = {"shape20": lambda: _shape(20), "box_plus_sphere": _box_plus_sphere, "slab_96x40x24": _slab_96,
          "three_faces": _against_three_faces, "plate": _plate, "single_voxel": _single_voxel,
          "two_blobs": _two_blobs}
_VALUES = torch.from_numpy(np.unique(M._band_tables(5.0, 4.0)[1]))
_cache = {}


def _band(name, dev):
    """(dist, band) of a shape on the device, computed once."""
    if name not in _cache:
        b = (_shape(96) if name == "shape96" else SHAPES[name]()).to(dev)
        _cache[name] = M.signed_distance_band_device(b, 5.0, 4.0)
    return _cache[name]


def _run(name, dev, iters, layout, **kw):
    dist, band = _band(name, dev)
    key = (name, iters, layout, tuple(sorted(kw.items())))
    if key not in _cache:
        # rel_tol < 0: the stopping test never fires, exactly `iters` iterations
        _cache[key] = M.smooth_band(dist.clone(), band, max_iters=iters, rel_tol=-1.0, layout=layout,
                                    **kw)[0]
    return _cache[key]


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_iterations_equal_the_slot_layout_bit_for_bit(dev, name, iters):
    dist, band = _band(name, dev)
    assert int(band.sum()) > 0
    ref = _run(name, dev, iters, "slots")
    got = _run(name, dev, iters, "bricks", values=_VALUES)
    assert torch.equal(got, ref)
    assert torch.equal(got[~band], dist[~band])             # written where the mask is set only


@pytest.mark.parametrize("name", ["box_plus_sphere", "two_blobs"])
def test_direct_loads_equal_the_staged_kernel(dev, name):
    ref = _run(name, dev, 3, "slots")
    assert torch.equal(_run(name, dev, 3, "bricks", values=_VALUES, direct=True), ref)
    assert torch.equal(_run(name, dev, 3, "bricks", bounds="stored", direct=True), ref)


def test_whole_function_with_default_arguments(dev):
    b = _shape(96).to(dev)
    dist, band = _band("shape96", dev)
    ref, n_ref = M.smooth_band(dist.clone(), band, layout="slots")
    got, n_got = M.smooth_band(dist.clone(), band, values=_VALUES)
    assert n_got == n_ref and 0 < n_ref <= 250 and n_ref % 10 == 0
    assert torch.equal(got, ref)
    assert torch.equal(M.smooth_constrained(b), ref)
    assert torch.equal(M.smooth_constrained(b, layout="slots"), ref)


def test_empty_band(dev):
    b = torch.zeros(8, 8, 8, dtype=torch.bool, device=dev)
    dist, band = M.signed_distance_band_device(b, 5.0, 4.0)
    assert int(band.sum()) == 0
    out, n = M.smooth_band(dist, band, layout="bricks")
    assert out is dist and n == 0
    assert ops.smooth_bricks_build(band, dist) is None
    assert torch.equal(M.smooth_constrained(b), M.smooth_constrained(b, layout="slots"))


def test_byte_coded_bounds_equal_stored_doubles(dev):
    name = "box_plus_sphere"
    dist, band = _band(name, dev)
    assert ops.smooth_bricks_build(band, dist, _VALUES).code is not None
    assert ops.smooth_bricks_build(band, dist, None).x0 is not None
    for iters in (3, 25):
        ref = _run(name, dev, iters, "slots")
        assert torch.equal(_run(name, dev, iters, "bricks", values=_VALUES, bounds="coded"), ref)
        assert torch.equal(_run(name, dev, iters, "bricks", bounds="coded"), ref)     # torch.unique
        assert torch.equal(_run(name, dev, iters, "bricks", bounds="stored"), ref)


def test_more_than_255_distinct_distances_take_the_stored_doubles(dev):
    dist, band = _band("box_plus_sphere", dev)
    dist = dist.clone()
    nv = int(band.sum())
    ramp = (torch.arange(nv, device=dev) % 300).to(torch.float64) * 1e-3
    dist[band] = dist[band] + torch.sign(dist[band]) * ramp           # signs kept, 300 offsets
    assert torch.unique(dist[band]).shape[0] > 255
    ref = M.smooth_band(dist.clone(), band, max_iters=25, rel_tol=-1.0, layout="slots")[0]
    # too many values; and a table that lacks some of the band's values (the gather reports the miss)
    for values in (None, _VALUES):
        bricks = ops.smooth_bricks_build(band, dist, torch.unique(dist[band]) if values is None else values)
        assert bricks.code is None and bricks.x0 is not None
        got = M.smooth_band(dist.clone(), band, max_iters=25, rel_tol=-1.0, layout="bricks",
                            values=values, bounds="coded")[0]
        assert torch.equal(got, ref)


def test_brick_energy(dev):
    name = "box_plus_sphere"
    dist, band = _band(name, dev)
    flat, nbr_slots, x, lower, upper = M._slot_layout(dist, band)
    nbr_t = torch.stack(nbr_slots).contiguous()
    x = x.contiguous()
    ybuf = torch.empty(3 * x.shape[0], dtype=torch.float64, device=dev)
    bricks = ops.smooth_bricks_build(band, dist, _VALUES)
    for iters in (0, 10):
        if iters:
            ops.smooth_iterate(nbr_t, lower.contiguous(), upper.contiguous(), x, ybuf, 0.5, iters)
            ops.smooth_bricks_iterate(bricks, 0.5, iters)
        ref = float(ops.smooth_energy(nbr_t, x, ybuf))
        got = float(ops.smooth_bricks_energy(bricks))
        print(f"energy after {iters} iterations: slots {ref!r} bricks {got!r} rel {abs(got - ref) / ref:.3e}")
        assert ref > 0 and abs(got - ref) <= 1e-12 * ref
        assert float(ops.smooth_bricks_energy(bricks)) == got             # fixed summation order
