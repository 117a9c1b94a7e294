"""GPU: dsu_uv_project (csrc/uv_project_area.hip) against the float64 restatement of its rule
(tests/uv_project_ref.py).  The device runs the restatement's float64 operations in the same order
(no fused products, IEEE division, rint), so EQUALITY is asserted on image and source; the texels
the restatement marks fragile may be left out, at most 0.5 % of them and none on the lattice case.
tests/test_uv_project_host.py checks on the CPU that these cases are not vacuous.  Beside that, the
kernel against its own text compiled for the host (dsu_uv_project_area_host at s = 1, filter 0, which
tests/test_uv_project_host.py holds to the restatement): every byte, no texel left out.

tools/uv_project_probe.py counts the differences and the fragile texels on these cases and writes
them to profiles/uv_project_probe.json (`accuracy`)."""
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


def device_project(dev, c, positions=None, masks=None, **kw):
    mf, mb = masks if masks is not None else (c["mask_front"], c["mask_back"])
    img, src = ops.uv_project(_t(c["uvs"], dev, np.float32), _t(c["indices"], dev, np.int32),
                              _t(c["positions"] if positions is None else positions, dev, np.float32),
                              _t(c["face_id"], dev, np.int32), _t(c["color_front"], dev), _t(mf, dev),
                              _t(c["color_back"], dev), _t(mb, dev), c["z_tolerance"], **kw)
    return img, src


def assert_projection_equal(got, want, fragile, allow_fragile):
    """(image, source) pairs; fragile texels may be left out (at most 0.5 %), when allowed at all."""
    keep = np.ones(fragile.shape, bool)
    if allow_fragile:
        assert fragile.mean() <= 0.005
        keep = ~fragile
    else:
        assert not fragile.any()
    print("source differs at", int((got[1] != want[1]).sum()), "image at", int((got[0] != want[0]).any(-1).sum()),
          "fragile", int(fragile.sum()))
    assert np.array_equal(got[1][keep], want[1][keep]), int((got[1] != want[1])[keep].sum())
    assert np.array_equal(got[0][keep], want[0][keep]), int((got[0] != want[0])[keep].any(-1).sum())


def device_silhouette_masks(dev, c):
    """The masks as bake_drawings prepares them (silhouette, erosion, mirror), copied to the host."""
    from drawingspinup_amd.nsr.mesh_post import projection_masks
    full = torch.full((P.RES, P.RES), 255, dtype=torch.uint8, device=dev)
    front, back = projection_masks(_t(c["positions"], dev), _t(c["indices"], dev), full, res=P.RES, ksize=P.SIL_ERODE)
    return front.cpu().numpy(), back.cpu().numpy()


@pytest.mark.parametrize("masks", P.MASK_KINDS)
@pytest.mark.parametrize("name,size", P.CASES)
def test_project_equals_restatement(dev, name, size, masks):
    if masks == "disc":
        c = P.case(name, size)
    else:
        m = device_silhouette_masks(dev, P.fixed(name, size))
        assert 0 < (m[0] > 0).mean() < 0.6 and np.array_equal(m[1], m[0][:, ::-1])
        c = P.restate(P.fixed(name, size), m, P.Z_TOL)
        assert (c["source"] == 1).sum() > 50                                  # not vacuous under these masks either
        assert ((c["source"] > 0) != (P.case(name, size)["source"] > 0)).any()
    img, src = device_project(dev, c)
    assert_projection_equal((img.cpu().numpy(), src.cpu().numpy()), (c["image"], c["source"]), c["fragile"],
                            allow_fragile=name != "lattice")
    if name == "body_and_arm":
        # covered texels that neither view takes: behind the arm, edge-on, or outside the mask
        assert ((c["source"] == 0) & (c["face_id"] >= 0)).sum() > 100


def assert_equals_the_host_entry(dev, c, **kw):
    want = A.host_project_area(c, 1, "nearest", with_count=False)
    img, src = device_project(dev, c, **kw)
    img, src = img.cpu().numpy(), src.cpu().numpy()
    assert np.array_equal(src, want[1]), int((src != want[1]).sum())
    assert np.array_equal(img, want[0]), int((img != want[0]).any(-1).sum())
    return src


@pytest.mark.parametrize("name,size,masks", A.GPU_CASES)
def test_project_equals_the_host_entry(dev, name, size, masks):
    """Long lists, fragile texels, both views, an atlas that is no multiple of the tile."""
    c = A.case(name, size, masks)
    src = assert_equals_the_host_entry(dev, c)
    assert (src == 1).sum() > 50 and ((src == 2).sum() > 50 or name not in P.CLOSED)
    assert name != "helicoid" or c["fragile"].sum() > 10


def test_non_finite_position_equals_the_host_entry(dev):
    assert_equals_the_host_entry(dev, P.nan_vertex_case())


@pytest.mark.parametrize("cells", (1, 2))
def test_long_cell_lists_equal_the_host_entry(dev, cells):
    """The walk's long-list path: one list of every triangle, four of hundreds (the host's grid is its
    own 24 x 24)."""
    assert_equals_the_host_entry(dev, P.case("body_and_arm", 64), cells_per_axis=cells)


def test_long_cell_lists(dev):
    """Two cells per axis: every list holds hundreds of triangles (any staging in batches would run
    many rounds and a tail); the answer does not depend on the grid."""
    c = P.case("body_and_arm", 64)
    pos, ind = _t(c["positions"], dev, np.float32), _t(c["indices"], dev, np.int64)
    tris = pos[ind].contiguous()
    xy = tris[..., :2].reshape(-1, 2)
    grid = ops.ZGrid(tris, xy.amin(0).tolist(), xy.amax(0).tolist(), cells_per_axis=2)
    counts = (grid.offsets[1:] - grid.offsets[:-1]).cpu().numpy()
    assert len(counts) == 4 and counts.min() > 2 * 256 and (counts % 256 != 0).all()
    for kw in (dict(grid=grid), dict(cells_per_axis=2), dict(cells_per_axis=1)):
        img, src = device_project(dev, c, **kw)
        assert_projection_equal((img.cpu().numpy(), src.cpu().numpy()), (c["image"], c["source"]), c["fragile"],
                                allow_fragile=True)


def test_zero_tolerance(dev):
    c = P.case("torus", 256, 0.0)
    img, src = device_project(dev, c)
    assert_projection_equal((img.cpu().numpy(), src.cpu().numpy()), (c["image"], c["source"]), c["fragile"],
                            allow_fragile=True)


def test_empty_mesh(dev):
    cf, cb = P.drawings()
    mf, mb = P.disc_masks()
    img, src = ops.uv_project(torch.zeros(0, 2, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
                              torch.zeros(0, 3, device=dev), torch.full((20, 20), -1, dtype=torch.int32, device=dev),
                              _t(cf, dev), _t(mf, dev), _t(cb, dev), _t(mb, dev), U.Z_TOLERANCE)
    assert img.shape == (20, 20, 3) and src.shape == (20, 20) and not img.any() and not src.any()


def test_non_finite_position_projects_nothing(dev):
    c = P.case("character", 100)
    seen = np.unique(c["face_id"][c["source"] > 0])
    bad = int(c["indices"][seen[len(seen) // 2], 0])                          # a vertex of a projected face
    pos = c["positions"].copy()
    pos[bad] = np.nan
    want = P.project(c["uvs"], c["indices"], pos, c["face_id"], c["color_front"], c["mask_front"], c["color_back"],
                     c["mask_back"], c["z_tolerance"], R.reference("character", 100)["fragile"])
    img, src = device_project(dev, c, positions=pos)
    img, src = img.cpu().numpy(), src.cpu().numpy()
    touched = np.isin(c["face_id"], np.nonzero((c["indices"] == bad).any(1))[0])
    assert (c["source"][touched] > 0).any() and not src[touched].any() and not img[touched].any()
    assert_projection_equal((img, src), want[:2], want[2], allow_fragile=True)


def test_bit_identical_repeats_and_streams(dev):
    c = P.case("body_and_arm", 64)

    def run():
        return device_project(dev, c)
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


def _grow(mask, rounds):
    out = mask.copy()
    for _ in range(rounds):
        p = np.pad(out, 1)
        out = np.maximum.reduce([p[1 + dr:p.shape[0] - 1 + dr, 1 + dc:p.shape[1] - 1 + dc]
                                 for dr in (-1, 0, 1) for dc in (-1, 0, 1)])
    return out


def test_export_end_to_end(dev, tmp_path):
    """save_obj(texture_source="drawings") = uv_mapping with the restatement behind it, from the frame
    post_process_mesh hands back; the vertex-colour export is untouched by the new keyword."""
    from PIL import Image
    from drawingspinup_amd import animate
    from drawingspinup_amd.nsr import mesh as M
    from drawingspinup_amd.nsr.mesh_post import projection_masks
    verts, faces = R.meshes()["character"]
    fr = P.into_frame("character", verts, faces).astype(np.float64)
    # save_obj halves and swaps (x, y, z) -> (x, z, -y): hand it what lands on `fr`
    v = torch.from_numpy(np.stack([2 * fr[:, 0], -2 * fr[:, 2], 2 * fr[:, 1]], -1)).to(dev)
    f = torch.from_numpy(faces).to(dev)
    cf, cb = P.drawings()
    cbp = {"color_front": _t(cf, dev), "color_back": _t(cb, dev), "erode": 5,
           "mask_front": torch.full((P.RES, P.RES), 255, dtype=torch.uint8, device=dev)}
    kw = dict(shearing=True, color_back_projection=cbp, export_uv=True, texture_size=100)
    path = M.save_obj(str(tmp_path / "d" / "c.obj"), v, f, None, texture_source="drawings", **kw)
    assert sorted(os.listdir(tmp_path / "d")) == ["c.mtl", "c.obj", "c.png"]
    out, fz, col, frame = M.post_process_mesh(v, f, None, 1.35, False, True, cbp, return_projection_frame=True)
    assert np.array_equal(frame.astype(np.float32), fr.astype(np.float32))
    front, back = projection_masks(_t(frame, dev, np.float32), f, cbp["mask_front"], res=P.RES, ksize=5)
    be = P.RefBackend((front.cpu().numpy(), back.cpu().numpy()))
    want = U.uv_mapping(out, fz, col, "c", size=100, backend=be,
                        projection={"positions": frame, "color_front": cf, "mask_front": None, "color_back": cb,
                                    "erode": 5})
    keep = ~_grow(be.fragile, 2)                                              # the gutter fill spreads a texel by 2
    assert be.fragile.mean() <= 0.005
    tex = np.array(Image.open(tmp_path / "d" / "c.png"))
    assert np.array_equal(tex[keep], want["image"][keep])
    plain = U.uv_mapping(out, fz, col, "c", size=100, device=dev)["image"]
    assert (tex != plain).any(-1).sum() > 500                                 # the drawings are in there
    rv, rf, rc = animate.read_obj(path)
    assert len(rf) == len(faces) and rc is not None and len(rv) == len(want["verts"])
    # "vertex" = the keyword left out, byte for byte
    M.save_obj(str(tmp_path / "a" / "c.obj"), v, f, None, texture_source="vertex", **kw)
    M.save_obj(str(tmp_path / "b" / "c.obj"), v, f, None, **kw)
    for name in ("c.mtl", "c.obj", "c.png"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read(), name
    assert np.array_equal(np.array(Image.open(tmp_path / "b" / "c.png")), plain)
