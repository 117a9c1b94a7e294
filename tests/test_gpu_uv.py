"""GPU: the UV-export kernels (csrc/mesh_uv.hip) against the float64 restatement of their rules
(tests/uv_ref.py).  The device runs the restatement's float64 operations in the same order (no
fused products, IEEE division, no square root anywhere), so EQUALITY is asserted: labels, normals,
chart ids, face_id, demote flags and the uint8 image.  The comparison helper still knows the
samples uv_ref marks fragile (an edge function within 1e-12 of zero relative to the face's uv area)
and would exclude up to 0.5 % of them, none on the lattice case.

tools/uv_probe.py counts the differing labels / chart ids / face ids / flags / image bytes and the
fragile samples on these meshes and writes them to profiles/uv_probe.json (`accuracy`)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_ref as R  # noqa: E402
from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def device_bake(dev, uvs, ind, col, size, depth=None):
    img, fid, dem = ops.uv_bake(_t(uvs, np.float32, dev), _t(ind, np.int32, dev), _t(col, np.float32, dev), size,
                                None if depth is None else _t(depth, np.float64, dev))
    return img.cpu().numpy(), fid.cpu().numpy(), None if dem is None else dem.cpu().numpy()


def assert_bake_equal(got, want, fragile, allow_fragile):
    """(image, face_id) pairs; fragile samples may be left out (at most 0.5 %), when allowed at all."""
    keep = np.ones(fragile.shape, bool)
    if allow_fragile:
        assert fragile.mean() <= 0.005
        keep = ~fragile
    else:
        assert not fragile.any()
    assert np.array_equal(got[1][keep], want[1][keep]), int((got[1] != want[1])[keep].sum())
    assert np.array_equal(got[0][keep], want[0][keep]), int((got[0] != want[0])[keep].any(-1).sum())


@pytest.mark.parametrize("name", ["character", "torus", "sheet", "body_and_arm", "helicoid", "ribbon", "lattice"])
def test_labels_and_components(dev, name):
    verts, faces = R.meshes()[name]
    normal, label, area = ops.uv_face_labels(_t(verts, np.float32, dev), _t(faces, np.int64, dev))
    rn, rl, ra = R.face_labels(verts, faces)
    assert np.array_equal(label.cpu().numpy(), rl)
    assert np.array_equal(normal.cpu().numpy(), rn) and np.array_equal(area.cpu().numpy(), ra)
    adj = ops.face_adjacency(_t(faces, np.int64, dev))
    assert np.array_equal(adj.cpu().numpy(), R.adjacency(faces))
    chart, rounds = ops.uv_components(adj, label, check_every=4)
    assert np.array_equal(chart.cpu().numpy(), R.components(faces, rl))
    # never behind the synchronous sweep, which changes something in its first sync - 1 rounds; the
    # flag is read every fourth round, and the loop ends after a group of four without a change
    sync = R.synchronous_rounds(R.adjacency(faces), rl)[1]
    assert rounds % 4 == 0 and rounds <= 4 * ((sync - 1 + 3) // 4) + 4, (rounds, sync)
    if name == "ribbon":
        # 4000 faces, 16 workgroups, one chart: the reach at least doubles per round, so at most
        # ceil(log2 M) rounds change anything
        assert len(np.unique(chart.cpu().numpy())) == 1
        changing = int(np.ceil(np.log2(len(faces))))
        assert sync - 1 <= changing and rounds <= 4 * ((changing + 3) // 4) + 4, (rounds, sync)


def test_components_with_negative_and_demoted_labels(dev):
    verts, faces = R.meshes()["torus"]
    _, rl, _ = R.face_labels(verts, faces)
    lab = rl.copy()
    lab[::7] += 6
    lab[5::31] = -2
    lab[3::53] = -1
    adj = ops.face_adjacency(_t(faces, np.int64, dev))
    chart, _ = ops.uv_components(adj, _t(lab, np.int32, dev), check_every=1)
    assert np.array_equal(chart.cpu().numpy(), R.components(faces, lab))


# (mesh, atlas size): 64 with 4728 faces = far more than 256 faces per tile, the LDS batch loop and
# its tail; 128 / 256 = faces over several tiles, rectangles no multiple of 16; 100 = no multiple
# of the tile, the tile / image edge; the lattice = every quantity exact, samples on edges and vertices
BAKE_CASES = [("body_and_arm", 64), ("character", 128), ("torus", 256), ("character", 100), ("helicoid", 128),
              ("ribbon", 128), ("lattice", 128)]


@pytest.mark.parametrize("name,size", BAKE_CASES)
def test_bake_equals_restatement(dev, name, size):
    r = R.reference(name, size)
    depth = U.face_depths(r["verts"], r["faces"], r["info"]["label"])
    img, fid, dem = device_bake(dev, r["uvs"], r["indices"], r["colours"], size, depth)
    assert_bake_equal((img, fid), (r["image"], r["face_id"]), r["fragile"], allow_fragile=name != "lattice")
    assert np.array_equal(dem, r["demote"]) and not dem.any()
    if name == "body_and_arm":
        plan = ops.UvBakePlan(_t(r["uvs"], np.float32, dev), _t(r["indices"], np.int32, dev), size).bin()
        counts = plan.workspace[:plan.bins].cpu().numpy()
        assert counts.max() > 2 * 256 and (counts % 256 != 0).any()
    if name == "lattice":
        # vertices sit on sample points: the inclusive edges are exercised
        t = r["uvs"].astype(np.float64) * size
        assert np.array_equal(t, np.round(t))


def test_demote_flags_on_the_unsplit_helicoid(dev):
    """One chart covering itself: the faces behind are flagged, exactly those the restatement flags."""
    verts, faces = R.helicoid()
    _, label, _ = R.face_labels(verts, faces)
    vm, ind, uvs, _ = U.layout(verts, faces, label, R.components(faces, label), 128, 2)
    depth = U.face_depths(verts, faces, label)
    col = R.vertex_colours(verts)[vm]
    want = R.bake(uvs, ind, col, 128, depth)
    img, fid, dem = device_bake(dev, uvs, ind, col, 128, depth)
    assert want[2].sum() > 50 and np.array_equal(dem, want[2])
    assert_bake_equal((img, fid), want[:2], want[3], allow_fragile=True)


@pytest.mark.parametrize("gutter", [0, 1, 3])
def test_dilate_rounds(dev, gutter):
    r = R.reference("character", 100)
    out = U.bake_vertex_colours(r["uvs"], r["indices"], r["colours"], 100, gutter, device=dev)
    assert np.array_equal(out, R.dilate(r["image"], r["face_id"] >= 0, gutter)[0])


@pytest.mark.parametrize("name", ["helicoid", "character", "lattice", "ribbon"])
def test_parametrize_on_the_device_equals_the_host_path(dev, name):
    """The whole loop (labels, charts, packing, raster, split) with the kernels against the same
    loop with the restatement; the helicoid goes through a split round."""
    r = R.reference(name, 128)
    vm, ind, uvs, info = U.parametrize(r["verts"], r["faces"], 128, 2, return_info=True, device=dev,
                                       scale=R.LATTICE_SCALE if name == "lattice" else None)
    assert np.array_equal(vm, r["vmapping"]) and np.array_equal(ind, r["indices"])
    assert np.array_equal(uvs, r["uvs"])
    for k in ("face_chart", "chart_rect", "chart_axis", "chart_sign", "label"):
        assert np.array_equal(info[k], r["info"][k]), k
    assert info["split_rounds"] == r["info"]["split_rounds"] and info["scale"] == r["info"]["scale"]
    if name == "helicoid":
        assert info["split_rounds"] >= 1 and len(info["chart_ids"]) >= 2


def test_bit_identical_repeats_and_streams(dev):
    r = R.reference("body_and_arm", 64)
    depth = U.face_depths(r["verts"], r["faces"], r["info"]["label"])
    args = (_t(r["uvs"], np.float32, dev), _t(r["indices"], np.int32, dev), _t(r["colours"], np.float32, dev), 64,
            _t(depth, np.float64, dev))

    def run():
        img, fid, dem = ops.uv_bake(*args)
        return ops.uv_dilate(img, fid >= 0, 2)[0], fid, dem
    a = run()
    b = run()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = run()
    d = run()                                                                 # beside the side stream's run
    torch.cuda.synchronize(dev)
    for other in (b, c, d):
        for x, y in zip(a, other):
            assert torch.equal(x, y)


def test_reference_fixture_on_the_device(dev):
    """tests/golden/uv_reference.npz: the reference's compute_interpolation_map."""
    from test_uv_host import check_against_reference_fixture
    rep = check_against_reference_fixture(lambda u, i, c, s: device_bake(dev, u, i, c, s)[:2])
    assert set(rep) == {"character", "helicoid"}


def test_export_end_to_end(dev, tmp_path):
    """uv_mapping on the device = the host reference path; the textured OBJ reads back and renders
    to the frames of the vertex-coloured mesh whose colours are the texture's samples."""
    from drawingspinup_amd import animate
    from drawingspinup_amd.animate.render import sample_texture
    from drawingspinup_amd.nsr import mesh as M
    verts, faces = R.meshes()["character"]
    col = R.vertex_colours(verts)
    got = U.uv_mapping(verts, faces, col, "c", size=128, device=dev)
    want = U.uv_mapping(verts, faces, col, "c", size=128, backend=R.RefBackend())
    for k in ("verts", "faces", "uvs", "image"):
        assert np.array_equal(got[k], want[k]), k
    path = M.save_obj(str(tmp_path / "c.obj"), torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev),
                      torch.from_numpy(col).to(dev), export_uv=True, texture_size=128)
    assert sorted(os.listdir(tmp_path)) == ["c.mtl", "c.obj", "c.png"]
    v, f, c = animate.read_obj(path)
    assert len(f) == len(faces) and c is not None and len(v) > len(verts)
    from PIL import Image
    tex = np.array(Image.open(tmp_path / "c.png"))
    uvs = np.asarray([[float(x) for x in l.split()[1:3]] for l in open(path) if l.startswith("vt ")])
    assert np.array_equal(c, sample_texture(tex, uvs))
    window = (0.0, 0.0, 64, 1.35)
    a = animate.render_frames(v, f, c, "rest_pose", ss=2, device=dev, window=window)
    b = animate.render_frames(v, f, sample_texture(tex, uvs), "rest_pose", ss=2, device=dev, window=window)
    for k in ("color", "pos", "edge"):
        assert torch.equal(a[k], b[k])
    assert int((a["color"][..., 3] > 0).sum()) > 100
