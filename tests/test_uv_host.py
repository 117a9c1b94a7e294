"""CPU: the contract of nsr/uv.parametrize on the float64 restatement (tests/uv_ref.py), the shelf
packing, the textured OBJ round trip, save_obj's export_uv branch, and the reference fixture
(tests/golden/uv_reference.npz: the REFERENCE's compute_interpolation_map) against uv_ref.bake."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_ref as R  # noqa: E402
from drawingspinup_amd.animate import read_obj  # noqa: E402
from drawingspinup_amd.animate.render import sample_texture  # noqa: E402
from drawingspinup_amd.nsr import mesh as M  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402

SIZE = 128
NAMES = ["character", "torus", "sheet", "body_and_arm", "helicoid", "ribbon", "lattice"]


@pytest.mark.parametrize("name", NAMES)
def test_parametrize_contract(name):
    r = R.reference(name, SIZE)
    verts, faces, vm, ind, uvs, info = (r[k] for k in ("verts", "faces", "vmapping", "indices", "uvs", "info"))
    assert vm.dtype == np.int64 and ind.dtype == np.int64 and uvs.dtype == np.float32
    assert np.array_equal(vm[ind], faces)
    assert uvs.min() >= 0.0 and uvs.max() <= 1.0
    # new vertices ordered by (old vertex, chart id), one per pair
    vchart = np.zeros(len(vm), np.int64)
    vchart[ind.reshape(-1)] = np.repeat(info["face_chart"], 3)
    key = vm * len(faces) + vchart
    assert np.all(np.diff(key) > 0)
    # chart id = the smallest face index of the chart
    ids, first = np.unique(info["face_chart"], return_index=True)
    assert np.array_equal(ids, first) and np.array_equal(ids, info["chart_ids"])
    assert info["min_cos"] == pytest.approx(1 / np.sqrt(3)) and info["min_cos"] >= 0.25

    # orientation and area.  uv = f32(U / size) moves a coordinate by at most half an ulp of a value
    # <= 1, d = 2^-25 (in uv units); the doubled area e1 x e2 then moves by at most 2 d (|e1| + |e2|) +
    # 4 d^2 <= 4 d Lmax (1 + tiny), i.e. relatively by 4 d Lmax / (Lmax h) = 4 d / h = 2 * 2^-24 / h with h the
    # altitude on the longest edge (<= the shortest edge).  3 * 2^-24 / h leaves the second-order
    # term and the float64 evaluation.
    v64 = verts.astype(np.float64)
    e1, e2 = v64[faces[:, 1]] - v64[faces[:, 0]], v64[faces[:, 2]] - v64[faces[:, 0]]
    n = np.cross(e1, e2)
    p = uvs.astype(np.float64)
    a, b, c = p[ind[:, 0]], p[ind[:, 1]], p[ind[:, 2]]
    area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    ok = info["label"] >= 0
    assert ok.all() or name not in NAMES                               # no degenerate face in these meshes
    assert np.all(area2[ok] > 0), "a face is not counter-clockwise in uv"
    lmax = np.sqrt(np.maximum.reduce([((b - a) ** 2).sum(1), ((c - b) ** 2).sum(1), ((a - c) ** 2).sum(1)]))
    h = area2 / lmax
    s_uv = info["scale"] / SIZE
    ratio = area2 / (s_uv * s_uv * np.linalg.norm(n, axis=1))
    ax = info["label"] // 2
    want = np.abs(n[np.arange(len(faces)), ax]) / np.linalg.norm(n, axis=1)
    tol = 3 * 2.0 ** -24 / h + 1e-12
    assert np.all(np.abs(ratio - want) <= tol * want), float(np.max(np.abs(ratio - want) / (tol * want)))
    assert np.all(want >= info["min_cos"] - 1e-12) and np.all(want <= 1 + 1e-12)

    # rectangles: inside the atlas, `gutter` from the border and from each other
    rect = info["chart_rect"]
    g = 2
    assert np.all(rect[:, :2] >= g) and np.all(rect[:, :2] + rect[:, 2:] + g <= SIZE)
    x0, y0, x1, y1 = rect[:, 0], rect[:, 1], rect[:, 0] + rect[:, 2], rect[:, 1] + rect[:, 3]
    apart_x = (x0[:, None] >= x1[None] + g) | (x0[None] >= x1[:, None] + g)
    apart_y = (y0[:, None] >= y1[None] + g) | (y0[None] >= y1[:, None] + g)
    assert np.all((apart_x | apart_y) | np.eye(len(rect), dtype=bool))
    # every vertex inside its chart's rectangle (f32 rounding of uv: far below a texel)
    slot = np.searchsorted(ids, vchart)
    t = p * SIZE
    assert np.all(t[:, 0] >= x0[slot] - 1e-3) and np.all(t[:, 0] <= x1[slot] - 1 + 1e-3)
    assert np.all(t[:, 1] >= y0[slot] - 1e-3) and np.all(t[:, 1] <= y1[slot] - 1 + 1e-3)

    # no sample point strictly inside two faces, by a rasteriser that knows no chart and no depth
    assert R.conflicts(uvs, ind, SIZE) == 0
    assert not r["demote"].any()
    if name == "helicoid":
        assert info["split_rounds"] >= 1 and len(ids) >= 2
    if name in ("ribbon", "sheet"):
        assert len(ids) == 1 and info["split_rounds"] == 0
    if name == "lattice":
        assert len(ids) == 6 and info["scale"] == R.LATTICE_SCALE


def test_helicoid_overlaps_before_the_split():
    """The unsplit single chart really covers itself: the case does force the split."""
    from drawingspinup_amd.nsr.uv import layout
    verts, faces = R.helicoid()
    _, label, _ = R.face_labels(verts, faces)
    chart = R.components(faces, label)
    assert len(np.unique(chart)) == 1
    _, ind, uvs, _ = layout(verts, faces, label, chart, SIZE, 2)
    assert R.conflicts(uvs, ind, SIZE) > 0


def test_components_rule_and_round_bound():
    """Union-find, the synchronous restatement of the device's rounds, and the bound pointer jumping
    gives on a strip numbered along its length: the reach at least doubles per round."""
    for name in ("ribbon", "torus", "body_and_arm"):
        verts, faces = R.meshes()[name]
        _, label, _ = R.face_labels(verts, faces)
        chart, rounds = R.synchronous_rounds(R.adjacency(faces), label)
        assert np.array_equal(chart, R.components(faces, label))
        if name == "ribbon":
            assert rounds <= int(np.ceil(np.log2(len(faces)))) + 1


def test_non_manifold_edge_joins_nothing():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, -1, 0], [0.5, 0.5, 0]], np.float32)
    f = np.asarray([[0, 1, 2], [1, 3, 2], [0, 4, 1], [0, 1, 5]], np.int64)    # edge (0,1) used three times
    _, label, _ = R.face_labels(v, f)
    assert len(set(label)) == 1
    assert R.components(f, label).tolist() == [0, 0, 2, 3]
    assert R.adjacency(f)[0].tolist() == [-1, 1, -1]
    adj = __import__("drawingspinup_amd.ops", fromlist=["face_adjacency"]).face_adjacency(torch.from_numpy(f))
    assert np.array_equal(adj.numpy(), R.adjacency(f))


@pytest.mark.parametrize("name", ["torus", "body_and_arm"])
def test_adjacency_plumbing_matches(name):
    from drawingspinup_amd import ops
    _, faces = R.meshes()[name]
    assert np.array_equal(ops.face_adjacency(torch.from_numpy(faces)).numpy(), R.adjacency(faces))


def test_degenerate_face_is_a_point_chart():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]], np.float32)
    f = np.asarray([[0, 1, 2], [0, 1, 3]], np.int64)                          # the second has no area
    vm, ind, uvs, info = U.parametrize(v, f, 32, 1, return_info=True, backend=R.RefBackend())
    assert info["label"].tolist() == [4, -1] and info["face_chart"].tolist() == [0, 1]
    assert np.array_equal(vm[ind], f)
    assert len(np.unique(uvs[ind[1]], axis=0)) == 1


def test_shelf_packing():
    wh = np.asarray([[10, 5], [4, 9], [7, 9], [28, 2], [3, 3]])
    ids = np.asarray([0, 3, 5, 8, 9])
    a = U.shelf_pack(wh, ids, 32, 2)
    assert np.array_equal(a, U.shelf_pack(wh.copy(), ids.copy(), 32, 2))
    # (h descending, id): 3, 5 and 0 on the first shelf, 9 on the second, the wide one on the third
    assert a.tolist() == [[17, 2], [2, 2], [8, 2], [2, 18], [2, 13]]
    assert U.shelf_pack(wh, ids, 24, 2) is None and U.shelf_pack([[29, 1]], [0], 32, 2) is None
    # the retry path: a first scale far too large for the atlas shrinks by the fixed factor
    verts, faces = R.meshes()["sheet"]
    *_, info = U.parametrize(verts, faces, 64, 2, return_info=True, backend=R.RefBackend(), scale=500.0)
    k = info["pack_retries"]
    assert k >= 1 and info["scale"] == pytest.approx(500.0 * U.SHRINK ** k, rel=1e-12)
    assert 500.0 * U.SHRINK ** (k - 1) * 1.0 > 60                             # one step earlier did not fit


def test_bake_gutter_rule():
    r = R.reference("character", SIZE)
    cov = r["face_id"] >= 0
    for g in (0, 1, 3):
        out = U.bake_vertex_colours(r["uvs"], r["indices"], r["colours"], SIZE, g, backend=R.RefBackend())
        assert np.array_equal(out[cov], r["image"][cov])
        grown = (out != 0).any(-1) & ~cov
        if g == 0:
            assert not grown.any()
        else:
            assert grown.any()
            # nothing further than g texels (Chebyshev) from a covered one
            reach = R.dilate(np.zeros_like(out), cov, g)[1]
            assert not (grown & ~reach).any()


def test_textured_obj_round_trip(tmp_path):
    r = R.reference("character", SIZE)
    verts = r["verts"].astype(np.float64)[r["vmapping"]]
    path = M.write_obj_textured(str(tmp_path / "out" / "x.obj"), verts, r["indices"], r["uvs"], r["filled"], "char")
    assert path.endswith("char.obj") and sorted(os.listdir(tmp_path / "out")) == ["char.mtl", "char.obj", "char.png"]
    mtl = open(tmp_path / "out" / "char.mtl").read().split("\n")
    assert "map_Kd char.png" in mtl and any(l.startswith("Kd 1.0") for l in mtl) and any(l.startswith("Ns 0.0") for l in mtl)
    head = open(path).read().split("\n")[:2]
    assert head == ["mtllib char.mtl", "usemtl char"]
    v, f, c = read_obj(path)
    assert np.array_equal(f, r["indices"])
    assert np.abs(v - verts).max() <= 0.5e-8 + 1e-15
    # the colour of a vertex is the baked texel at its uv (nearest sample, the bake's convention)
    t = r["uvs"].astype(np.float64) * SIZE
    col = np.clip(np.floor(t[:, 0] + 0.5).astype(int), 0, SIZE - 1)
    row = np.clip(SIZE - 1 - np.floor(t[:, 1] + 0.5).astype(int), 0, SIZE - 1)
    assert c.dtype == np.float32 and np.array_equal(c, r["filled"][row, col].astype(np.float32) / np.float32(255))
    assert np.array_equal(c, sample_texture(r["filled"], r["uvs"]))
    # ... and close to the vertex colour that was baked: a vertex sits within half a texel of its sample
    assert np.abs(c - r["colours"]).mean() < 0.05
    # a file without vt reads as before
    p2 = M.write_obj(str(tmp_path / "plain.obj"), verts, r["indices"], r["colours"])
    v2, f2, c2 = read_obj(p2)
    assert np.array_equal(f2, r["indices"]) and np.allclose(c2, r["colours"], atol=1e-6)
    p3 = M.write_obj(str(tmp_path / "bare.obj"), verts, r["indices"])
    assert read_obj(p3)[2] is None


def test_first_uv_in_file_order_wins(tmp_path):
    from PIL import Image
    img = np.zeros((4, 4, 3), np.uint8)
    img[3, 0] = (255, 0, 0)                                                   # uv * 4 = (0, 0)
    img[3, 2] = (0, 255, 0)                                                   # uv * 4 = (2, 0)
    Image.fromarray(img).save(tmp_path / "m.png")
    open(tmp_path / "m.mtl", "w").write("newmtl m\nmap_Kd m.png\n")
    open(tmp_path / "m.obj", "w").write("mtllib m.mtl\nusemtl m\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\n"
                                        "vt 0 0\nvt 0.5 0\nf 1/2 2/1 3/1\nf 1/1 2/2 4/2\n")
    _, f, c = read_obj(str(tmp_path / "m.obj"))
    assert f.tolist() == [[0, 1, 2], [0, 1, 3]]
    assert c.tolist() == [[0, 1, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0]]


def test_save_obj_default_bytes_unchanged_and_uv_branch(tmp_path, monkeypatch):
    verts, faces = R.meshes()["character"]
    v, f = torch.from_numpy(verts), torch.from_numpy(faces)
    c = torch.from_numpy(R.vertex_colours(verts))
    a = M.save_obj(str(tmp_path / "a" / "m.obj"), v, f, c)
    b = M.save_obj(str(tmp_path / "b" / "m.obj"), v, f, c, export_uv=False)
    out, fz, cc = M.post_process_mesh(v, f, c, 1.35, False, False, None, None)
    M.write_obj(str(tmp_path / "c" / "m.obj"), out, fz, cc)
    data = open(a, "rb").read()
    assert data == open(b, "rb").read() == open(tmp_path / "c" / "m.obj", "rb").read()
    assert os.listdir(tmp_path / "a") == ["m.obj"]
    # the uv branch, with the numpy backend standing in for the device
    real = U.uv_mapping
    monkeypatch.setattr(U, "uv_mapping", lambda *a_, **k: real(*a_, **{**k, "backend": R.RefBackend()}))
    p = M.save_obj(str(tmp_path / "u" / "m.obj"), v, f, c, export_uv=True, texture_size=SIZE)
    assert sorted(os.listdir(tmp_path / "u")) == ["m.mtl", "m.obj", "m.png"] and p.endswith("m.obj")
    v2, f2, c2 = read_obj(p)
    assert len(f2) == len(faces) and c2 is not None and len(v2) > len(verts)
    from scipy.spatial import cKDTree                                         # the same points, some of them repeated
    assert cKDTree(out).query(v2)[0].max() < 1e-7 and cKDTree(v2).query(out)[0].max() < 1e-7


def test_export_uv_stays_off_by_default():
    from drawingspinup_amd.entry import config as C
    import inspect
    assert inspect.signature(M.save_obj).parameters["export_uv"].default is False
    assert "export_uv\": False" in inspect.getsource(C)


# ------------------------------------------------------------------ the reference's compute_interpolation_map
def check_against_reference_fixture(bake):
    """bake(uvs, indices, colours, size) -> (image, face_id).  The comparison rule of the fixture:
    equal on every texel whose sample lies strictly inside a face; one level of difference only
    where colour * 255 is within 1e-6 of an integer, and on at most 0.5 % of the compared texels."""
    z = np.load(os.path.join(R.GOLDEN, "uv_reference.npz"))
    report = {}
    for name in ("character", "helicoid"):
        uvs, ind, col, want = (z[f"{name}_{k}"] for k in ("uvs", "indices", "colours", "image"))
        size = want.shape[0]
        image, face_id = bake(uvs, ind, col, size)
        strict = strictly_inside(uvs, ind, size)
        assert strict.sum() > 0.15 * size * size
        exact = affine_value(z[f"{name}_A"], z[f"{name}_b"], size) * 255.0
        near = (np.abs(exact - np.round(exact)) <= 1e-6).any(-1)
        diff = np.abs(image.astype(int) - want.astype(int)).max(-1)
        assert np.all(face_id[strict] >= 0)
        assert np.all(diff[strict & ~near] == 0), int((diff[strict & ~near] != 0).sum())
        assert np.all(diff[strict] <= 1)
        excused = int((strict & near & (diff > 0)).sum())
        assert excused <= 0.005 * strict.sum()
        report[name] = (int(strict.sum()), excused)
    return report


def strictly_inside(uvs, indices, size):
    S = int(size)
    uv = np.asarray(uvs, np.float32).astype(np.float64) * S
    out = np.zeros((S, S), bool)
    for ia, ib, ic in indices:
        t = (uv[ia, 0], uv[ia, 1], uv[ib, 0], uv[ib, 1], uv[ic, 0], uv[ic, 1])
        py, px = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
        x0, x1 = max(int(min(t[0::2])) - 1, 0), min(int(max(t[0::2])) + 2, S - 1)
        y0, y1 = max(int(min(t[1::2])) - 1, 0), min(int(max(t[1::2])) + 2, S - 1)
        w0, w1, w2 = R._edges(t, px[y0:y1 + 1, x0:x1 + 1], py[y0:y1 + 1, x0:x1 + 1])
        eps = 1e-9 * abs((w0 + w1 + w2).flat[0]) if w0.size else 0.0
        out[y0:y1 + 1, x0:x1 + 1] |= (w0 > eps) & (w1 > eps) & (w2 > eps)
    return out[::-1]                                                          # image rows run against y


def affine_value(A, b, size):
    """A uv + b at every texel's sample, (S,S,3), image orientation."""
    S = int(size)
    y, x = np.meshgrid(np.arange(S)[::-1] / S, np.arange(S) / S, indexing="ij")
    return x[..., None] * A[:, 0] + y[..., None] * A[:, 1] + b


def test_reference_fixture_against_restatement():
    rep = check_against_reference_fixture(lambda u, i, c, s: R.bake(u, i, c, s)[:2])
    assert set(rep) == {"character", "helicoid"}
