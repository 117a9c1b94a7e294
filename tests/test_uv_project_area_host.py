"""CPU: dsu_uv_project_area (include/dsu_hip.h, UV export j.) through the library's host entry
dsu_uv_project_area_host — the text the kernel compiles (csrc/uv_project_area.h) — against the
float64 restatement tests/uv_project_area_ref.py: image, source and count equal in every byte, no
texel left out (both sides run the same operations in the same order).  Then what follows from the
rule, the aliasing case it is for, the edge rows and refusals, and the Python layers
(bake_drawings / uv_mapping through the numpy backend, save_obj, recon).
tests/test_gpu_uv_project_area.py holds the kernel to this host entry."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_project_area_ref as A  # noqa: E402
import uv_project_ref as P  # noqa: E402
from drawingspinup_amd import _lib  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402

RUNS = [c + (s,) for c in A.GENERAL for s in (1, 2, 3, 4)] + [A.GENERAL[0] + (8,)]


def assert_equal(got, want):
    for name, g, w in zip(("image", "source", "count"), got, want):
        assert g.dtype == np.uint8 and g.shape == w.shape
        assert np.array_equal(g, w), (name, int((g != w).sum()))


# ------------------------------------------------------------------ 1. the host entry, byte for byte
@pytest.mark.parametrize("pixel_filter", A.FILTERS)
@pytest.mark.parametrize("name,size,masks,s", RUNS)
def test_host_entry_equals_the_restatement(name, size, masks, s, pixel_filter):
    c = A.case(name, size, masks)
    want = A.want(name, size, masks, s, pixel_filter)
    assert_equal(A.host_project_area(c, s, pixel_filter), want)
    image, source, count = want
    old = c["source"]
    # not vacuous: both outcomes, and for s > 1 texels with some but not all of their samples
    assert (source > 0).sum() > 50 and ((source == 0) & (c["face_id"] >= 0)).sum() > 20
    assert count.max() == s * s and (s == 1 or ((count > 0) & (count < s * s)).sum() >= 10)
    # (b): the projected set only grows, and keeps its views
    assert np.array_equal(source[old > 0], old[old > 0])
    assert not image[source == 0].any() and not count[c["face_id"] < 0].any()
    # where no grid sample passed, the own point decided: the texel is one rule e. projects
    own = (source > 0) & (count == 0)
    assert (old[own] > 0).all() and (s % 2 == 0 or not own.any())
    if (name, s) == ("character", 2):
        assert own.sum() >= 1
    if s > 1:
        assert (source > 0).sum() > (old > 0).sum()                          # texels gained


@pytest.mark.parametrize("name,size,masks", A.GENERAL)
def test_one_nearest_sample_is_rule_e(name, size, masks):
    """(a): s = 1, nearest is dsu_uv_project byte for byte — here its restatement uv_project_ref.project."""
    c = A.case(name, size, masks)
    image, source, count = A.host_project_area(c, 1, "nearest")
    assert np.array_equal(image, c["image"]) and np.array_equal(source, c["source"])
    assert np.array_equal(count, (source > 0).astype(np.uint8))
    # and bilinear reads something else
    assert (A.host_project_area(c, 1, "bilinear")[0] != image).any()


@pytest.mark.parametrize("pixel_filter", A.FILTERS)
def test_result_does_not_depend_on_the_grid(pixel_filter):
    """(c): a one-cell grid (offsets [0, F], items 0 .. F - 1) and a 40^2 grid give the same bytes."""
    c = A.case("body_and_arm", 64)
    tris, ok = A.case_tris(c)
    one = A.HostGrid(tris, 1)
    F = len(c["indices"])
    assert one.g == 1 and one.offsets.tolist() == [0, F] and np.array_equal(one.items, np.arange(F))
    fine = A.HostGrid(tris, 40)
    assert len(fine.offsets) == 1601 and (np.diff(fine.offsets) == 0).any()
    for s in (2, 3):
        want = A.want("body_and_arm", 64, "disc", s, pixel_filter)
        assert_equal(A.host_project_area(c, s, pixel_filter, grid=one), want)
        assert_equal(A.host_project_area(c, s, pixel_filter, grid=fine), want)


# ------------------------------------------------------------------ 2. what it is for
def test_aliasing_case():
    """A one-pixel column pattern at four pixels per texel.  One nearest sample per texel (and 2 x 2 of
    them, which land on pixel coordinates k + 1/2 +- 1) read one parity only: every byte is 0 or
    255.  4 x 4 sub-samples sit on exact integer pixel coordinates, two of each parity per row: the
    mean is 127.5 and the byte 128, under both filters."""
    c = A.aliasing_case()
    covered = c["face_id"] >= 0
    assert covered.sum() == 33 * 33
    for pixel_filter in A.FILTERS:
        image, source, count = A.host_project_area(c, 4, pixel_filter, g=4)
        assert_equal((image, source, count), A.project_area(*_rule_args(c), 4, pixel_filter))
        assert np.all(source[covered] == 1) and not source[~covered].any() and np.all(count[covered] == 16)
        assert np.all(image[covered] == 128) and not image[~covered].any()
    for s in (1, 2):
        image, source, count = A.host_project_area(c, s, "nearest", g=4)
        assert_equal((image, source, count), A.project_area(*_rule_args(c), s, "nearest"))
        assert np.all(source[covered] == 1) and np.all(np.isin(image[covered], (0, 255)))


def _rule_args(c):
    return (c["uvs"], c["indices"], c["positions"], c["face_id"], c["color_front"], c["mask_front"], c["color_back"],
            c["mask_back"], c["z_tolerance"])


# ------------------------------------------------------------------ 3. edge rows and refusals
EDGE = A.edge_rows()


@pytest.mark.parametrize("pixel_filter", A.FILTERS)
@pytest.mark.parametrize("row", sorted(EDGE))
def test_edge_rows_equal_the_restatement(row, pixel_filter):
    c = EDGE[row]
    base = A.case("body_and_arm", 64)
    for s in (1, 2, 3):
        want = A.project_area(*_rule_args(c), s, pixel_filter)
        got = A.host_project_area(c, s, pixel_filter)
        assert_equal(got, want)
        image, source, count = got
        if row == "uncovered_texel":
            bare = c["face_id"] < 0
            assert bare.sum() > 100 and not image[bare].any() and not source[bare].any() and not count[bare].any()
        elif row == "face_id_out_of_range":
            bad = (c["face_id"] >= len(c["indices"])) | (c["face_id"] < -1)
            assert bad.sum() > 100 and (base["source"][bad] > 0).all()
            assert not image[bad].any() and not source[bad].any() and not count[bad].any()
        elif row == "vertex_index_out_of_range":
            ind = np.asarray(c["indices"])
            broken = np.nonzero((ind < 0).any(1) | (ind >= len(c["positions"])).any(1))[0]
            touched = np.isin(c["face_id"], broken)
            assert len(broken) == 2 and (base["source"][touched] > 0).any()
            assert not image[touched].any() and not source[touched].any() and not count[touched].any()
        elif row == "nan_vertex":
            bad = int(np.nonzero(np.isnan(c["positions"]).any(1))[0][0])
            touched = np.isin(c["face_id"], np.nonzero((c["indices"] == bad).any(1))[0])
            assert (base["source"][touched] > 0).any() and not source[touched].any() and not image[touched].any()
            assert (source > 0).sum() > 500
        elif row == "all_zero_mask":
            assert not image.any() and not source.any() and not count.any()
        elif row == "res_1":
            assert (source == 1).sum() > 50 and (source == 2).sum() > 50
            assert np.all(image[source == 1] == 201) and np.all(image[source == 2] == 55)


def test_no_faces_and_no_count():
    c = A.case("body_and_arm", 64)
    empty = dict(c, uvs=np.zeros((0, 2), np.float32), indices=np.zeros((0, 3), np.int64),
                 positions=np.zeros((0, 3), np.float32))
    for out in (A.host_project_area(empty, 2, "bilinear"), A.project_area(*_rule_args(empty), 2, "bilinear")):
        assert all(a.shape[:2] == (64, 64) and not a.any() for a in out)
    # count = NULL: the other two outputs are the same
    want = A.want("body_and_arm", 64, "disc", 3, "bilinear")
    image, source, count = A.host_project_area(c, 3, "bilinear", with_count=False)
    assert count is None and np.array_equal(image, want[0]) and np.array_equal(source, want[1])


def test_entry_points_validate_before_any_launch():
    """include/dsu_hip.h j.: DSU_EINVAL for every argument named there, from the device entry (which
    returns before any launch) and from the host entry alike."""
    lib = _lib.lib()
    p = ctypes.c_void_p(64)                                                   # never dereferenced

    def call(fn, **kw):
        a = dict(uvs=p, indices=p, positions=p, n_verts=4, n_faces=2, size=64, face_id=p, tris=p, x0=0.0, y0=0.0,
                 cell=0.1, g=8, offsets=p, items=p, color_front=p, mask_front=p, color_back=p, mask_back=p, res=256,
                 z_tolerance=1e-4, s=2, filter=1, image=p, source=p, count=p)
        assert set(kw) <= set(a)
        a.update(kw)
        return fn(*a.values(), *([None] if fn is lib.dsu_uv_project_area else []))
    for fn in (lib.dsu_uv_project_area, lib.dsu_uv_project_area_host):
        for bad in (dict(s=0), dict(s=9), dict(s=-1), dict(filter=-1), dict(filter=2),
                    dict(size=0), dict(size=8193), dict(res=0), dict(res=16385), dict(g=0), dict(g=4097),
                    dict(cell=0.0), dict(cell=float("nan")), dict(x0=float("inf")), dict(y0=float("nan")),
                    dict(z_tolerance=-1e-9), dict(z_tolerance=float("nan")), dict(z_tolerance=float("inf")),
                    dict(n_verts=-1), dict(n_faces=-1), dict(n_faces=(1 << 30) + 1), dict(n_verts=(1 << 30) + 1),
                    dict(n_verts=0), dict(image=None), dict(source=None), dict(n_faces=0, image=None),
                    dict(n_faces=0, s=9), dict(n_faces=0, filter=2)):
            assert call(fn, **bad) == -1, bad
        for name in ("uvs", "indices", "positions", "face_id", "tris", "offsets", "items", "color_front", "mask_front",
                     "color_back", "mask_back"):
            assert call(fn, **{name: None}) == -1, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dsu_hip.h")).read()
    for name in ("dsu_uv_project_area", "dsu_uv_project_area_host"):
        assert f"int {name}(" in header and callable(getattr(lib, name))
    assert _lib.ABI_VERSION == 3


# ------------------------------------------------------------------ 4. the Python layers
def _baked(c, be, **kw):
    fallback = np.full((len(c["uvs"]), 3), 0.5, np.float32)
    return U.bake_drawings(c["uvs"], c["indices"], c["positions"], c["color_front"], None, c["color_back"], fallback,
                           c["size"], 0, backend=be, return_maps=True, **kw)


def test_bake_drawings_samples_and_filter_through_the_numpy_backend():
    c = A.case("body_and_arm", 64)
    masks = (c["mask_front"], c["mask_back"])
    plain = _baked(c, A.RefBackend(masks))
    for kw in (dict(samples=1), dict(pixel_filter="nearest"), dict(samples=1, pixel_filter="nearest")):
        for a, b in zip(_baked(c, A.RefBackend(masks), **kw), plain):         # defaults: the bytes of today
            assert np.array_equal(a, b)
    # the default path asks the backend for project() with today's arguments: a backend without
    # project_area serves it
    for a, b in zip(_baked(c, P.RefBackend(masks)), plain):
        assert np.array_equal(a, b)
    with pytest.raises(AttributeError):
        _baked(c, P.RefBackend(masks), samples=2)
    for s, f in ((4, "bilinear"), (1, "bilinear"), (3, "nearest")):
        img, fid, src = _baked(c, A.RefBackend(masks), samples=s, pixel_filter=f)
        want = A.want("body_and_arm", 64, "disc", s, f)
        assert np.array_equal(src, want[1]) and np.array_equal(fid, c["face_id"])
        assert np.array_equal(img[src > 0], want[0][src > 0]) and np.all(img[(src == 0) & (fid >= 0)] == 127)
        assert (img != plain[0]).any()
    for kw in (dict(samples=0), dict(samples=9), dict(pixel_filter="area"), dict(pixel_filter=None)):
        with pytest.raises(ValueError):
            _baked(c, A.RefBackend(masks), **kw)


def test_uv_mapping_hands_the_samples_on():
    import uv_field_ref as F
    v, f = F.icosphere()
    frame = np.stack([v[:, 0], v[:, 2], -v[:, 1]], -1)
    cf, cb = P.drawings()
    be = A.RefBackend(P.disc_masks())
    col = np.full((len(v), 3), 0.5, np.float32)
    pr = {"positions": frame, "color_front": cf, "mask_front": None, "color_back": cb}
    plain = U.uv_mapping(v, f, col, "s", size=64, backend=be, projection=pr)
    same = U.uv_mapping(v, f, col, "s", size=64, backend=be, projection=dict(pr, samples=1, filter="nearest"))
    assert np.array_equal(same["image"], plain["image"])
    got = U.uv_mapping(v, f, col, "s", size=64, backend=be, projection=dict(pr, samples=3, filter="bilinear"))
    vm, ind, uvs = U.parametrize(v, f, 64, 2, backend=be)
    want = U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 2, backend=be, samples=3,
                           pixel_filter="bilinear")
    assert np.array_equal(got["image"], want) and not np.array_equal(want, plain["image"])
    for k in ("verts", "faces", "uvs"):
        assert np.array_equal(got[k], plain[k])


def test_save_obj_refuses_the_keywords_without_the_drawings(tmp_path):
    from drawingspinup_amd.nsr import mesh as M
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    f, c = torch.tensor([[0, 1, 2]]), torch.full((3, 3), 0.5)
    for src in (dict(), dict(texture_source="vertex"),
                dict(texture_source="field", export_uv=True, texture_field=lambda p: p)):
        for kw in (dict(texture_drawing_samples=2), dict(texture_drawing_filter="bilinear")):
            with pytest.raises(ValueError):
                M.save_obj(str(tmp_path / "a.obj"), v, f, c, **kw, **src)
    cbp = {"color_front": None, "mask_front": None, "color_back": None}
    for kw in (dict(texture_drawing_samples=0), dict(texture_drawing_samples=9), dict(texture_drawing_samples=2.5),
               dict(texture_drawing_filter="area")):
        with pytest.raises(ValueError):
            M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="drawings", export_uv=True,
                       color_back_projection=cbp, **kw)
    assert os.listdir(tmp_path) == []
    M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_drawing_samples=1, texture_drawing_filter="nearest")
    M.save_obj(str(tmp_path / "b.obj"), v, f, c)
    assert open(tmp_path / "a.obj", "rb").read() == open(tmp_path / "b.obj", "rb").read()


def test_recon_reads_the_switches_without_default_keys():
    from drawingspinup_amd.entry import recon
    _, conf = recon.parse(["--uid", "u"])
    assert "texture_drawing_samples" not in conf["export"] and "texture_drawing_filter" not in conf["export"]
    on = ["--uid", "u", "--texture_source", "drawings", "export.export_uv=true"]
    _, conf = recon.parse(on + ["--texture_drawing_samples", "4", "--texture_drawing_filter", "bilinear"])
    assert conf["export"]["texture_drawing_samples"] == 4 and conf["export"]["texture_drawing_filter"] == "bilinear"
    _, conf = recon.parse(on + ["export.texture_drawing_samples=8", "export.texture_drawing_filter=nearest"])
    assert conf["export"]["texture_drawing_samples"] == 8 and conf["export"]["texture_drawing_filter"] == "nearest"
    _, conf = recon.parse(on + ["--texture_drawing_samples", "1"])
    assert conf["export"]["texture_drawing_samples"] == 1 and "texture_drawing_filter" not in conf["export"]
    for argv in (on + ["--texture_drawing_samples", "0"], on + ["--texture_drawing_samples", "9"],
                 on + ["export.texture_drawing_samples=0"], on + ["export.texture_drawing_samples=two"],
                 on + ["--texture_drawing_filter", "area"], on + ["export.texture_drawing_filter=area"],
                 ["--uid", "u", "--texture_drawing_samples", "2"], ["--uid", "u", "--texture_drawing_filter", "bilinear"],
                 ["--uid", "u", "export.texture_drawing_samples=1"],
                 ["--uid", "u", "--texture_source", "field", "export.export_uv=true", "--texture_drawing_samples", "2"],
                 ["--uid", "u", "--texture_source", "vertex", "--texture_drawing_filter", "nearest"]):
        with pytest.raises(SystemExit):
            recon.parse(argv)
