"""GPU: the field bake's kernels (dsu_uv_field_points / dsu_uv_field_resolve, csrc/mesh_uv.hip)
against the library's host entries, which run the same text (csrc/uv_field.h) on the CPU and are
held to the float64 restatement by tests/test_uv_field_host.py: EQUALITY of every bit is asserted.
Then bake_field / uv_mapping / save_obj on the device against the numpy backend
(tests/uv_field_ref.py), with a per-point callable whose arithmetic is exact on both sides, and
with the real network."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_field_ref as F  # noqa: E402
import uv_project_ref as P  # noqa: E402
from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dev, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def device_points(dev, c, s, texels=None):
    return ops.uv_field_points(_t(c["uvs"], dev, np.float32), _t(c["indices"], dev, np.int32),
                               _t(c["positions"], dev, np.float32), _t(c["face_id"], dev, np.int32),
                               _t(c["texels"] if texels is None else texels, dev, np.int32), s)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("s", F.SAMPLES)
@pytest.mark.parametrize("name,size", F.CASES)
def test_points_equal_the_host_entry(dev, name, size, s):
    c = F.case(name, size)
    want_p, want_v = F.host_points(c, s)
    points, valid = device_points(dev, c, s)
    assert points.shape == want_p.shape and valid.shape == want_v.shape and valid.dtype == torch.uint8
    assert np.array_equal(valid.cpu().numpy(), want_v) and want_v.all()
    assert np.array_equal(bits(points.cpu().numpy()), bits(want_p))


@pytest.mark.parametrize("s", F.SAMPLES)
def test_edge_rows_equal_the_host_entry(dev, s):
    """Uncovered texels, indices outside the atlas, a face id and vertex indices out of range, a NaN
    vertex: invalid, the point zero, nothing read out of bounds."""
    c, rows = F.edge_rows()
    want_p, want_v = F.host_points(c, s)
    points, valid = device_points(dev, c, s)
    points, valid = points.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(valid, want_v) and np.array_equal(bits(points), bits(want_p))
    assert not np.isnan(points).any() and 0 < (valid == 0).sum() < 0.1 * valid.size
    where = {int(t): k for k, t in enumerate(c["texels"])}
    for kind, texels in rows.items():
        k = [where[int(t)] for t in texels]
        assert not valid[k].any() and not points[k].any(), kind


def test_empty_list_and_wrapper_checks(dev):
    c = F.case("triangle")
    points, valid = device_points(dev, c, 2, texels=np.zeros(0, np.int32))
    assert points.shape == (0, 4, 3) and valid.shape == (0, 4)
    img = torch.full((16, 16, 3), 33, dtype=torch.uint8, device=dev)
    out = ops.uv_field_resolve(torch.zeros(0, 4, 3, device=dev), valid, torch.zeros(0, dtype=torch.int32, device=dev),
                               img)
    assert out is img and bool((img == 33).all())
    with pytest.raises(ValueError):
        device_points(dev, c, 9)
    with pytest.raises(ValueError):
        ops.uv_field_resolve(torch.zeros(5, 3, 3, device=dev), torch.zeros(5, 3, dtype=torch.uint8, device=dev),
                             torch.zeros(5, dtype=torch.int32, device=dev), img)


@pytest.mark.parametrize("s", F.SAMPLES)
def test_resolve_equals_the_host_entry(dev, s):
    """Values below 0, above 1 and NaN among the colours, texels without a valid sample (their
    pre-filled bytes stay), two indices outside the image (nothing is written)."""
    c = F.case("icosphere", 64)
    tex = np.concatenate([c["texels"], np.asarray([-1, 64 * 64], np.int32)])
    col, valid = F.resolve_inputs(len(tex), s, seed=10 + s)
    want = F.host_resolve(col, valid, tex, np.full((64, 64, 3), 201, np.uint8), s)
    img = torch.full((64, 64, 3), 201, dtype=torch.uint8, device=dev)
    got = ops.uv_field_resolve(_t(col, dev), _t(valid, dev), _t(tex, dev), img).cpu().numpy()
    assert np.array_equal(got, want)
    empty = c["texels"][valid[:len(c["texels"])].sum(1) == 0]
    assert len(empty) >= len(c["texels"]) // 7 and (got.reshape(-1, 3)[empty] == 201).all()
    assert (got[c["face_id"] < 0] == 201).all() and (got[c["face_id"] >= 0] != 201).any()


def test_bit_identical_repeats_and_streams(dev):
    c = F.case("icosphere", 64)
    col, _ = F.resolve_inputs(len(c["texels"]), 4, seed=3)
    col = _t(col, dev)

    def run():
        points, valid = device_points(dev, c, 4)
        img = torch.full((64, 64, 3), 7, dtype=torch.uint8, device=dev)
        return points, valid, ops.uv_field_resolve(col, valid, _t(c["texels"], dev), img)
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
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y)


# ------------------------------------------------------------------ bake_field
@pytest.mark.parametrize("s", F.SAMPLES)
@pytest.mark.parametrize("size", [64, 37])
def test_bake_field_equals_the_numpy_backend(dev, size, s):
    """The stripes (period 0.05, a third of an edge) through the device and through the numpy backend,
    in three or more pieces on the device: byte for byte, maps included.  The vertex bake of the same
    function is another image: the feature adds what the vertex bake cannot hold."""
    c = F.case("icosphere", size)
    n = len(c["texels"])
    calls = []

    def counted(p):
        assert torch.is_tensor(p) and p.is_cuda and p.dtype == torch.float32 and p.shape[1] == 3
        calls.append(p.shape[0])
        return F.stripes(p)
    piece = n // 3 - 1
    fallback = np.full((len(c["uvs"]), 3), 0.3, np.float32)
    got = U.bake_field(c["uvs"], c["indices"], c["positions"], counted, fallback, size, 2, samples=s,
                       chunk=piece * s * s, device=dev, return_maps=True)
    assert len(calls) >= 3 and sum(calls) == n * s * s and max(calls) <= piece * s * s
    want = U.bake_field(c["uvs"], c["indices"], c["positions"], F.stripes, fallback, size, 2, samples=s,
                        backend=F.RefBackend(), return_maps=True)
    for g, w, what in zip(got, want, ("image", "face_id", "evaluated")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    covered = c["face_id"] >= 0
    assert np.array_equal(got[2] > 0, covered)
    vertex = U.bake_vertex_colours(c["uvs"], c["indices"], F.stripes(c["positions"]), size, 2, device=dev)
    print("covered", int(covered.sum()), "texels where the vertex bake differs",
          int((vertex[covered] != got[0][covered]).any(-1).sum()))
    assert (vertex != got[0]).any()


def _quantise(col):
    v = col.double() * 255.0
    v = torch.where(torch.isnan(v), torch.zeros_like(v), v.clamp(0.0, 255.0))
    return v.to(torch.uint8).cpu().numpy()                                  # truncation


def test_bake_field_of_the_network_is_the_network_at_the_restated_points(dev):
    """A sphere-initialised NeuSModel, an icosphere of radius 0.5 (its zero level set), one sample
    per texel: the atlas holds vertex_colors(model, p) at the restated points, quantised — byte for
    byte, the evaluation being per point whatever the batch (here three pieces against one)."""
    from drawingspinup_amd.nsr.mesh import field_colours, vertex_colors
    from drawingspinup_amd.nsr.model import NeuSModel
    torch.manual_seed(5)
    model = NeuSModel().to(dev).eval()
    model.update_step(0, 0)                                                   # level / finite-difference schedule of step 0
    c = F.case("icosphere", 64)
    n = len(c["texels"])
    img, fid, ev = U.bake_field(c["uvs"], c["indices"], c["positions"], field_colours(model), None, 64, 0, samples=1,
                                chunk=n // 3 + 1, device=dev, return_maps=True)
    points = F.restated("icosphere", 64, 1)["points"][:, 0]
    want = _quantise(vertex_colors(model, _t(points, dev)))
    got = img.reshape(-1, 3)[c["texels"]]
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print("texels", n, "differing bytes", int((diff > 0).sum()), "largest difference", int(diff.max()))
    assert len(np.unique(want)) > 3                                        # a field, not a constant
    assert np.array_equal(got, want)
    assert np.array_equal(ev > 0, fid >= 0) and not img[fid < 0].any()


# ------------------------------------------------------------------ save_obj
def _export_mesh(dev):
    v, f = F.icosphere()
    col = torch.from_numpy(F.affine(v).astype(np.float32)).to(dev)
    return torch.from_numpy(v.astype(np.float64)).to(dev), torch.from_numpy(f).to(dev), col


def test_save_obj_field_equals_uv_mapping_over_the_restatement(dev, tmp_path):
    from PIL import Image
    from drawingspinup_amd import animate
    from drawingspinup_amd.nsr import mesh as M
    v, f, col = _export_mesh(dev)
    kw = dict(shearing=False, export_uv=True, texture_size=64)                # a sphere has no axis to shear along
    path = M.save_obj(str(tmp_path / "d" / "c.obj"), v, f, col, texture_source="field", texture_field=F.stripes,
                      texture_samples=2, **kw)
    assert sorted(os.listdir(tmp_path / "d")) == ["c.mtl", "c.obj", "c.png"]
    out, fz, cz = M.post_process_mesh(v, f, col, 1.35, False, False)
    want = U.uv_mapping(out, fz, cz, "c", size=64, backend=F.RefBackend(),
                        field={"positions": v.float().cpu().numpy(), "eval_colours": F.stripes, "samples": 2})
    tex = np.array(Image.open(tmp_path / "d" / "c.png"))
    assert np.array_equal(tex, want["image"])
    rv, rf, rc = animate.read_obj(path)
    assert len(rf) == len(fz) and len(rv) == len(want["verts"])
    # "vertex" with and without a field = the keywords left out, byte for byte; and not the field's image
    M.save_obj(str(tmp_path / "a" / "c.obj"), v, f, col, texture_source="vertex", texture_field=F.stripes,
               texture_samples=4, **kw)
    M.save_obj(str(tmp_path / "b" / "c.obj"), v, f, col, texture_source="vertex", **kw)
    M.save_obj(str(tmp_path / "n" / "c.obj"), v, f, col, **kw)
    for name in ("c.mtl", "c.obj", "c.png"):
        plain = open(tmp_path / "n" / name, "rb").read()
        assert open(tmp_path / "a" / name, "rb").read() == plain, name
        assert open(tmp_path / "b" / name, "rb").read() == plain, name
    assert (np.array(Image.open(tmp_path / "n" / "c.png")) != tex).any()


def test_save_obj_drawings_fall_back_to_the_field(dev, tmp_path):
    """"drawings" plus a field: texels a drawing sees carry its bytes, the others the field bake's."""
    from PIL import Image
    from drawingspinup_amd.nsr import mesh as M
    v, f, _ = _export_mesh(dev)
    v = v * 1.9                                                               # radius 0.475 in the projection frame
    cf, cb = P.drawings()
    cbp = {"color_front": _t(cf, dev), "color_back": _t(cb, dev), "erode": 5,
           "mask_front": _t(P.disc_masks()[0], dev)}
    kw = dict(shearing=True, color_back_projection=cbp, export_uv=True, texture_size=64)
    M.save_obj(str(tmp_path / "d" / "c.obj"), v, f, None, texture_source="drawings", texture_field=F.stripes,
               texture_samples=2, **kw)
    tex = np.array(Image.open(tmp_path / "d" / "c.png"))
    out, fz, col, frame = M.post_process_mesh(v, f, None, 1.35, False, True, cbp, return_projection_frame=True)
    vm, ind, uvs = U.parametrize(out, fz, 64, 2, device=dev)
    drawn, fid, src = U.bake_drawings(uvs, ind, frame[vm], cbp["color_front"], cbp["mask_front"], cbp["color_back"],
                                      col[vm], 64, 0, erode=5, device=dev, return_maps=True)
    field = U.bake_field(uvs, ind, v.float().cpu().numpy()[vm], F.stripes, col[vm], 64, 0, samples=2, device=dev)
    covered = fid >= 0
    seen, unseen = covered & (src > 0), covered & (src == 0)
    assert seen.sum() > 100 and unseen.sum() > 20
    assert np.array_equal(tex[seen], drawn[seen]) and np.array_equal(tex[unseen], field[unseen])
    assert (field[unseen] != drawn[unseen]).any()                            # not the vertex bake under another name
    # without the field the same call keeps the vertex bake there
    M.save_obj(str(tmp_path / "e" / "c.obj"), v, f, None, texture_source="drawings", **kw)
    old = np.array(Image.open(tmp_path / "e" / "c.png"))
    assert np.array_equal(old[unseen], drawn[unseen]) and np.array_equal(old[seen], drawn[seen])
