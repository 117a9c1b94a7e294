"""GPU: the kernel of dsu_uv_project_area (csrc/uv_project_area.hip) against the library's host entry
dsu_uv_project_area_host — one text (csrc/uv_project_area.h) compiled twice, float64 without fused
products on both sides — so image, source and count are held to EQUALITY in every byte.
tests/test_uv_project_area_host.py holds the host entry to the numpy restatement of the rule.  Then
determinism, dsu_uv_project, bake_drawings on the device against the numpy backend, and the file
save_obj writes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_project_area_ref as A  # noqa: E402
import uv_project_ref as P  # noqa: E402
import uv_ref as R  # noqa: E402
from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dev, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def device_inputs(dev, c):
    return (_t(c["uvs"], dev, np.float32), _t(c["indices"], dev, np.int32), _t(c["positions"], dev, np.float32),
            _t(c["face_id"], dev, np.int32), _t(c["color_front"], dev), _t(c["mask_front"], dev),
            _t(c["color_back"], dev), _t(c["mask_back"], dev), c["z_tolerance"])


def device_project_area(dev, c, s, pixel_filter, inputs=None, **kw):
    out = ops.uv_project_area(*(inputs or device_inputs(dev, c)), s, pixel_filter, **kw)
    return tuple(a.cpu().numpy() for a in out)


def assert_equal(got, want):
    for name, g, w in zip(("image", "source", "count"), got, want):
        assert g.dtype == np.uint8 and g.shape == w.shape
        assert np.array_equal(g, w), (name, int((g != w).sum()))


# ------------------------------------------------------------------ 1. the kernel against the host entry
@pytest.mark.parametrize("name,size,masks", A.GPU_CASES)
def test_kernel_equals_the_host_entry(dev, name, size, masks):
    """s = 1, 2, 3, 4, 8 (the one-point instantiation, one group, a group and a tail, whole groups, sixteen groups) under
    both filters; the device's grid is ops.ZGrid's, the host's a numpy one."""
    c = A.case(name, size, masks)
    inputs = device_inputs(dev, c)
    tris, ok = A.case_tris(c)
    grid = A.HostGrid(tris, 24, ok)
    for s in (1, 2, 3, 4, 8):
        for pixel_filter in A.FILTERS:
            want = A.host_project_area(c, s, pixel_filter, grid=grid)
            got = device_project_area(dev, c, s, pixel_filter, inputs)
            assert_equal(got, want)
            assert (want[1] > 0).sum() > 50 and want[2].max() == s * s
    # (a): one nearest sample is dsu_uv_project (the same launch without a count), byte for byte
    img, src = ops.uv_project(*inputs)
    one = device_project_area(dev, c, 1, "nearest", inputs)
    assert np.array_equal(one[0], img.cpu().numpy()) and np.array_equal(one[1], src.cpu().numpy())
    assert np.array_equal(one[2], (one[1] > 0).astype(np.uint8))


@pytest.mark.parametrize("cells", (3, 40))
def test_result_does_not_depend_on_the_grid(dev, cells):
    c = A.case("body_and_arm", 64)
    inputs = device_inputs(dev, c)
    for s, pixel_filter in ((2, "nearest"), (3, "bilinear"), (4, "bilinear")):
        want = A.host_project_area(c, s, pixel_filter)
        assert_equal(device_project_area(dev, c, s, pixel_filter, inputs, cells_per_axis=cells), want)


EDGE = A.edge_rows()


@pytest.mark.parametrize("row", sorted(EDGE))
def test_edge_rows_equal_the_host_entry(dev, row):
    """The grid is the host's, uploaded: ops.ZGrid gathers positions[indices], which an index out of
    range cannot go through."""
    c = EDGE[row]
    tris, ok = A.case_tris(c)
    grid = A.HostGrid(tris, 24, ok)
    inputs = device_inputs(dev, c)
    for s, pixel_filter in ((1, "nearest"), (1, "bilinear"), (2, "bilinear"), (3, "nearest"), (3, "bilinear")):
        want = A.host_project_area(c, s, pixel_filter, grid=grid)
        assert_equal(device_project_area(dev, c, s, pixel_filter, inputs, grid=A.DeviceGrid(grid, dev)), want)


def test_aliasing_case(dev):
    c = A.aliasing_case()
    covered = c["face_id"] >= 0
    inputs = device_inputs(dev, c)
    for pixel_filter in A.FILTERS:
        got = device_project_area(dev, c, 4, pixel_filter, inputs)
        assert_equal(got, A.host_project_area(c, 4, pixel_filter, g=4))
        assert np.all(got[0][covered] == 128) and np.all(got[2][covered] == 16) and not got[0][~covered].any()
    for s in (1, 2):
        got = device_project_area(dev, c, s, "nearest", inputs)
        assert_equal(got, A.host_project_area(c, s, "nearest", g=4))
        assert np.all(np.isin(got[0][covered], (0, 255)))


def test_empty_mesh_and_wrapper_checks(dev):
    cf, cb = P.drawings()
    mf, mb = P.disc_masks()
    args = (torch.zeros(0, 2, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
            torch.zeros(0, 3, device=dev), torch.full((20, 20), -1, dtype=torch.int32, device=dev),
            _t(cf, dev), _t(mf, dev), _t(cb, dev), _t(mb, dev), U.Z_TOLERANCE)
    img, src, cnt = ops.uv_project_area(*args, 4, "bilinear")
    assert img.shape == (20, 20, 3) and src.shape == cnt.shape == (20, 20)
    assert not img.any() and not src.any() and not cnt.any()
    for s, f in ((0, "nearest"), (9, "nearest"), (2, "area")):
        with pytest.raises(ValueError):
            ops.uv_project_area(*args, s, f)


# ------------------------------------------------------------------ 2. determinism
def test_bit_identical_repeats_and_streams(dev):
    c = A.case("body_and_arm", 64)
    inputs = device_inputs(dev, c)

    def run():
        return ops.uv_project_area(*inputs, 4, "bilinear")
    a = run()
    b = run()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        d = run()
    e = run()                                                                 # beside the side stream's run
    torch.cuda.synchronize(dev)
    for other in (b, d, e):
        for x, y in zip(a, other):
            assert torch.equal(x, y)


# ------------------------------------------------------------------ 3. bake_drawings on the device
def _device_masks(dev, positions, indices, erode):
    from drawingspinup_amd.nsr.mesh_post import projection_masks
    full = torch.full((P.RES, P.RES), 255, dtype=torch.uint8, device=dev)
    front, back = projection_masks(_t(positions, dev, np.float32), _t(indices, dev, np.int64), full, res=P.RES,
                                   ksize=erode)
    return front.cpu().numpy(), back.cpu().numpy()


def test_bake_drawings_equals_the_numpy_backend(dev):
    """bake_drawings(samples=4, pixel_filter="bilinear", seam="level") through the device backend and
    through the numpy one (which gets the device's prepared masks), byte for byte."""
    c = P.fixed("body_and_arm", 64)
    verts, faces = R.meshes()["body_and_arm"]
    vm = R.reference("body_and_arm", 64)["vmapping"]
    groups, gf = U.seam_groups(verts, faces, vm)
    fallback = np.random.default_rng(3).random((len(vm), 3)).astype(np.float32)
    full = np.full((P.RES, P.RES), 255, np.uint8)
    args = (c["uvs"], c["indices"], c["positions"], c["color_front"], full, c["color_back"], fallback, 64, 2)
    kw = dict(erode=P.SIL_ERODE, seam="level", groups=groups, group_faces=gf, return_maps=True)
    got = U.bake_drawings(*args, device=dev, samples=4, pixel_filter="bilinear", **kw)
    be = A.RefBackend(_device_masks(dev, c["positions"], c["indices"], P.SIL_ERODE))
    want = U.bake_drawings(*args, backend=be, samples=4, pixel_filter="bilinear", **kw)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), int((g != w).sum())
    plain = U.bake_drawings(*args, device=dev, **kw)
    assert (got[2] > 0).sum() > (plain[2] > 0).sum() > 100 and (got[0] != plain[0]).any()
    # the defaults are the call without the keywords
    for g, w in zip(U.bake_drawings(*args, device=dev, samples=1, pixel_filter="nearest", **kw), plain):
        assert np.array_equal(g, w)


# ------------------------------------------------------------------ 4. the file
def test_save_obj_writes_the_area_sampled_atlas(dev, tmp_path):
    """The PNG of save_obj(texture_drawing_samples=3, texture_drawing_filter="bilinear") = uv_mapping
    over the restatement, from the frame post_process_mesh hands back; the keywords at their defaults
    are the export without them, byte for byte."""
    from PIL import Image
    from drawingspinup_amd.nsr import mesh as M
    verts, faces = R.meshes()["character"]
    fr = P.into_frame("character", verts, faces).astype(np.float64)
    v = torch.from_numpy(np.stack([2 * fr[:, 0], -2 * fr[:, 2], 2 * fr[:, 1]], -1)).to(dev)
    f = torch.from_numpy(faces).to(dev)
    cf, cb = P.drawings()
    cbp = {"color_front": _t(cf, dev), "color_back": _t(cb, dev), "erode": 5,
           "mask_front": torch.full((P.RES, P.RES), 255, dtype=torch.uint8, device=dev)}
    kw = dict(shearing=True, color_back_projection=cbp, export_uv=True, texture_size=100, texture_source="drawings")
    M.save_obj(str(tmp_path / "s" / "c.obj"), v, f, None, texture_drawing_samples=3,
               texture_drawing_filter="bilinear", **kw)
    M.save_obj(str(tmp_path / "d" / "c.obj"), v, f, None, texture_drawing_samples=1,
               texture_drawing_filter="nearest", **kw)
    M.save_obj(str(tmp_path / "o" / "c.obj"), v, f, None, **kw)
    for name in ("c.mtl", "c.obj", "c.png"):
        assert open(tmp_path / "d" / name, "rb").read() == open(tmp_path / "o" / name, "rb").read(), name
    for name in ("c.mtl", "c.obj"):
        assert open(tmp_path / "s" / name, "rb").read() == open(tmp_path / "o" / name, "rb").read(), name
    out, fz, col, frame = M.post_process_mesh(v, f, None, 1.35, False, True, cbp, return_projection_frame=True)
    be = A.RefBackend(_device_masks(dev, frame, faces, 5))
    want = U.uv_mapping(out, fz, col, "c", size=100, backend=be,
                        projection={"positions": frame, "color_front": cf, "mask_front": None, "color_back": cb,
                                    "erode": 5, "samples": 3, "filter": "bilinear"})
    tex = np.array(Image.open(tmp_path / "s" / "c.png"))
    old = np.array(Image.open(tmp_path / "o" / "c.png"))
    assert np.array_equal(tex, want["image"]) and (tex != old).any(-1).sum() > 500
