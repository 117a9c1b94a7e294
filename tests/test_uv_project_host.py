"""CPU: the per-texel projection of the drawings into the atlas through the public
nsr.uv.bake_drawings / uv_mapping with the float64 backend (tests/uv_project_ref.py), on sheets
whose every quantity is exact, and the properties of the cases tests/test_gpu_uv_project.py runs
on the device (few fragile texels, none on the lattice, both views present)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_project_area_ref as A  # noqa: E402
import uv_project_ref as P  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402

# a 1/8 x 1/8 sheet = 32 x 32 texels, a texel about a pixel of the 256^2 drawing: uv, barycentrics
# and points exact; off x = 0 and y = 0, where the pixel coordinate is the half-integer 127.5
# (fragile by the rule, if exact here)
SIZE, SCALE, X0, Y0, SIDE = 128, 256.0, 0.125, -0.375, 0.125
QUAD = np.asarray([[X0, Y0], [X0 + SIDE, Y0], [X0 + SIDE, Y0 + SIDE], [X0, Y0 + SIDE]])
FULL = (np.full((P.RES, P.RES), 255, np.uint8),) * 2


def sheets(zs, flipped):
    """One quad per z; `flipped` ones face -z."""
    verts, faces = [], []
    for k, (z, fl) in enumerate(zip(zs, flipped)):
        verts += [[x, y, z] for x, y in QUAD]
        a = 4 * k
        faces += [[a, a + 2, a + 1], [a, a + 3, a + 2]] if fl else [[a, a + 1, a + 2], [a, a + 2, a + 3]]
    return np.asarray(verts, np.float32), np.asarray(faces, np.int64)


def baked(verts, faces, masks=FULL, **kw):
    be = P.RefBackend(masks)
    vm, ind, uvs, info = U.parametrize(verts, faces, SIZE, 2, return_info=True, backend=be, scale=SCALE)
    cf, cb = P.drawings()
    fallback = np.full((len(vm), 3), 0.5, np.float32)
    img, fid, src = U.bake_drawings(uvs, ind, verts[vm], cf, FULL[0], cb, fallback, SIZE, 0, backend=be,
                                    return_maps=True, **kw)
    return {"image": img, "face_id": fid, "source": src, "info": info, "uvs": uvs, "indices": ind, "vm": vm,
            "fallback": fallback, "fragile": be.fragile}


def texel_points(b, face, swap):
    """Mesh (x, y) of the texels of `face`'s chart from the chart's rectangle alone (exact here): u
    runs along x and v along y, or the other way round for a chart seen from -z."""
    info = b["info"]
    slot = int(np.searchsorted(info["chart_ids"], info["face_chart"][face]))
    x0, y0 = info["chart_rect"][slot][:2]
    rows, cols = np.nonzero(np.isin(b["face_id"], np.nonzero(info["face_chart"] == info["face_chart"][face])[0]))
    u, v = (cols - x0) / SCALE, ((SIZE - 1 - rows) - y0) / SCALE
    return rows, cols, (v + X0, u + Y0) if swap else (u + X0, v + Y0)


def pixels(x, y, back=False):
    span = P.RES - 1
    X = np.rint(((-x if back else x) + 0.5) * span).astype(np.int64)
    return np.rint((-y + 0.5) * span).astype(np.int64), X


def test_flat_sheet_reproduces_the_checker_and_the_vertex_bake_does_not():
    verts, faces = sheets([0.0], [False])
    b = baked(verts, faces)
    covered = b["face_id"] >= 0
    assert covered.sum() == 33 * 33 and not b["fragile"].any()
    assert np.all(b["source"][covered] == 1) and not b["source"][~covered].any()
    rows, cols, (x, y) = texel_points(b, 0, False)
    assert len(rows) == covered.sum()
    cf, _ = P.drawings()
    Y, X = pixels(x, y)
    assert np.array_equal(b["image"][rows, cols], cf[Y, X])
    assert len(np.unique(b["image"][rows, cols, 2])) == 2                    # the one-pixel checker is in there
    # the vertex-colour bake of the same sheet, its vertices coloured from the same drawing
    vy, vx = pixels(verts[b["vm"], 0].astype(np.float64), verts[b["vm"], 1].astype(np.float64))
    vertex = U.bake_vertex_colours(b["uvs"], b["indices"], cf[vy, vx].astype(np.float32) / 255.0, SIZE, 0,
                                   backend=P.RefBackend())
    # the ramps interpolate, the checker cannot: four corners of one parity give one flat value
    assert len(np.unique(vertex[rows, cols, 2])) == 1
    assert (vertex[rows, cols] != cf[Y, X]).any(-1).mean() > 0.4


def test_rear_sheet_reads_the_back_drawing_mirrored():
    verts, faces = sheets([0.1, -0.1], [False, True])
    b = baked(verts, faces)
    front_texels, rear_texels = np.isin(b["face_id"], [0, 1]), np.isin(b["face_id"], [2, 3])
    assert front_texels.sum() == rear_texels.sum() == 33 * 33 and not b["fragile"].any()
    assert np.all(b["source"][front_texels] == 1)                            # never the back image
    assert np.all(b["source"][rear_texels] == 2)
    cf, cb = P.drawings()
    rows, cols, (x, y) = texel_points(b, 0, False)
    assert np.array_equal(b["image"][rows, cols], cf[pixels(x, y)])
    rows, cols, (x, y) = texel_points(b, 2, True)
    assert np.array_equal(b["image"][rows, cols], cb[pixels(x, y, back=True)])
    assert not np.array_equal(b["image"][rows, cols], cb[pixels(x, y)])      # the mirror matters


def test_occlusion_and_the_tolerance_above_the_gap():
    verts, faces = sheets([0.1, -0.1], [False, False])                       # both face +z, 0.2 apart
    b = baked(verts, faces)
    front_texels, rear_texels = np.isin(b["face_id"], [0, 1]), np.isin(b["face_id"], [2, 3])
    assert np.all(b["source"][front_texels] == 1) and not b["source"][rear_texels].any()
    assert np.all(b["image"][rear_texels] == 127)                            # the fallback: 0.5 * 255 truncated
    b = baked(verts, faces, z_tolerance=0.25)
    assert np.all(b["source"][rear_texels] == 1) and np.all(b["source"][front_texels] == 1)
    rows, cols, (x, y) = texel_points(b, 2, False)
    assert np.array_equal(b["image"][rows, cols], P.drawings()[0][pixels(x, y)])


def test_all_zero_masks_leave_the_vertex_bake():
    """Through the backend's own mask preparation (silhouette, erosion, mirror) and the gutter fill."""
    verts, faces = sheets([0.1, -0.1], [False, True])
    be = P.RefBackend()
    vm, ind, uvs = U.parametrize(verts, faces, SIZE, 2, backend=be, scale=SCALE)
    cf, cb = P.drawings()
    col = np.random.default_rng(0).random((len(vm), 3)).astype(np.float32)
    img, fid, src = U.bake_drawings(uvs, ind, verts[vm], cf, np.zeros((P.RES, P.RES), np.uint8), cb, col, SIZE, 2,
                                    backend=be, return_maps=True)
    assert not src.any()
    assert np.array_equal(img, U.bake_vertex_colours(uvs, ind, col, SIZE, 2, backend=P.RefBackend()))
    # and with the drawing's mask in place the same call projects (the preparation keeps the inside)
    img2, _, src2 = U.bake_drawings(uvs, ind, verts[vm], cf, FULL[0], cb, col, SIZE, 2, backend=be, erode=3,
                                    return_maps=True)
    assert (src2 == 1).sum() > 600 and (src2 == 2).sum() > 600 and not np.array_equal(img, img2)


def test_uv_mapping_takes_the_projection_in_old_vertex_order():
    verts, faces = sheets([0.1, -0.1], [False, True])
    cf, cb = P.drawings()
    col = np.full((len(verts), 3), 0.5, np.float32)
    shown = verts.astype(np.float64) * 1.35 + 0.01                           # the exported frame is another one
    pr = {"positions": verts, "color_front": torch.from_numpy(cf), "mask_front": FULL[0], "color_back": cb}
    got = U.uv_mapping(shown, faces, col, "s", size=SIZE, backend=P.RefBackend(FULL), projection=pr)
    plain = U.uv_mapping(shown, faces, col, "s", size=SIZE, backend=P.RefBackend(FULL))
    for k in ("verts", "faces", "uvs"):
        assert np.array_equal(got[k], plain[k])
    vm, ind, uvs = U.parametrize(shown, faces, SIZE, 2, backend=P.RefBackend())
    want = U.bake_drawings(uvs, ind, verts[vm], cf, FULL[0], cb, col[vm], SIZE, 2, backend=P.RefBackend(FULL))
    assert np.array_equal(got["image"], want) and not np.array_equal(got["image"], plain["image"])
    assert np.array_equal(U.uv_mapping(shown, faces, col, "s", size=SIZE, backend=P.RefBackend(FULL),
                                       projection=None)["image"], plain["image"])


def test_drawings_need_export_uv_and_the_images(tmp_path):
    from drawingspinup_amd.nsr import mesh as M
    verts, faces = sheets([0.0], [False])
    v, f, c = torch.from_numpy(verts), torch.from_numpy(faces), torch.full((4, 3), 0.5)
    cbp = {"color_front": None, "mask_front": None, "color_back": None}
    with pytest.raises(ValueError):
        M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="drawings", color_back_projection=cbp)
    with pytest.raises(ValueError):
        M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="drawings", export_uv=True)
    with pytest.raises(ValueError):
        M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="photo", export_uv=True)
    assert os.listdir(tmp_path) == []


def test_post_process_mesh_hands_back_the_projection_frame():
    from drawingspinup_amd.nsr import mesh as M
    rng = np.random.default_rng(1)
    v = torch.from_numpy(rng.random((6, 3)) - 0.5)
    f = torch.tensor([[0, 1, 2], [3, 4, 5]])
    three = M.post_process_mesh(v, f, None, 1.35, False, True)
    four = M.post_process_mesh(v, f, None, 1.35, False, True, return_projection_frame=True)
    assert len(three) == 3 and len(four) == 4
    assert np.array_equal(three[0], four[0]) and np.array_equal(three[1], four[1])
    half = v.numpy() * 0.5
    assert np.array_equal(four[3], np.stack([half[:, 0], half[:, 2], -half[:, 1]], -1))
    assert not np.allclose(four[3] * 1.35, four[0])                          # before the shear and the scale


def test_recon_reads_the_texture_source_without_a_default_key():
    from drawingspinup_amd.entry import recon
    _, conf = recon.parse(["--uid", "u"])
    assert "texture_source" not in conf["export"] and conf["export"].get("texture_source", "vertex") == "vertex"
    _, conf = recon.parse(["--uid", "u", "--texture_source", "drawings", "export.export_uv=true"])
    assert conf["export"]["texture_source"] == "drawings" and conf["export"]["export_uv"] is True
    _, conf = recon.parse(["--uid", "u", "export.texture_source=drawings", "export.export_uv=true"])
    assert conf["export"]["texture_source"] == "drawings"
    # refused when the command is read, not by save_obj after the optimisation
    for argv in (["--texture_source", "photo"], ["--texture_source", "drawings"], ["export.texture_source=photo"],
                 ["--texture_source", "drawings", "export.export_uv=true", "--no-color_back_projection"]):
        with pytest.raises(SystemExit):
            recon.parse(["--uid", "u"] + argv)


def test_the_exported_mesh_is_wound_outward_in_the_projection_frame():
    """The facing test reads the winding: marching cubes' triangles, through the halving and the axis
    swap of post_process_mesh, must enclose a positive volume in color_projection's frame (wound
    inward, every texel would silently keep the vertex colours)."""
    from drawingspinup_amd.nsr import mesh as M
    res = 24
    g = torch.linspace(-1, 1, res)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    level = (x ** 2 / 0.36 + y ** 2 / 0.16 + z ** 2 / 0.25).sqrt() - 1.0    # an ellipsoid, negative inside
    m = M.MarchingCubeHelper(res)(level.reshape(-1))
    _, fz, _, frame = M.post_process_mesh(m["verts"] * 2 - 1, m["faces"], None, 1.35, True, True,
                                          return_projection_frame=True)
    t = frame[fz]
    volume = np.einsum("ij,ij->", t[:, 0], np.cross(t[:, 1], t[:, 2])) / 6
    assert 0.8 < volume / (4 / 3 * np.pi * 0.3 * 0.2 * 0.25) < 1.1, volume
    nz = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])[:, 2]
    assert np.all(t[nz > 1e-9][:, :, 2].mean(1) > -0.05) and (nz > 0).sum() > 400   # +z faces are the front ones


def test_entry_point_validates_before_any_launch():
    """include/dsu_hip.h, dsu_uv_project: DSU_EINVAL for every argument named there, DSU_OK for the
    one legal call that needs no device (checked in this order: ranges, outputs, then inputs)."""
    import ctypes
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(64)                                                   # never dereferenced: no launch

    def call(**kw):
        a = dict(uvs=p, indices=p, positions=p, n_verts=4, n_faces=2, size=64, face_id=p, tris=p, x0=0.0, y0=0.0,
                 cell=0.1, g=8, offsets=p, items=p, color_front=p, mask_front=p, color_back=p, mask_back=p, res=256,
                 z_tolerance=1e-4, image=p, source=p, stream=None)
        assert set(kw) <= set(a)
        a.update(kw)
        return lib.dsu_uv_project(*a.values())
    for bad in (dict(size=0), dict(size=8193), dict(res=0), dict(res=16385), dict(g=0), dict(g=4097),
                dict(cell=0.0), dict(cell=float("nan")), dict(x0=float("inf")), dict(y0=float("nan")),
                dict(z_tolerance=-1e-9), dict(z_tolerance=float("nan")), dict(z_tolerance=float("inf")),
                dict(n_verts=-1), dict(n_faces=-1), dict(n_faces=(1 << 30) + 1), dict(n_verts=(1 << 30) + 1),
                dict(n_verts=0), dict(image=None), dict(source=None), dict(n_faces=0, image=None)):
        assert call(**bad) == -1, bad
    for name in ("uvs", "indices", "positions", "face_id", "tris", "offsets", "items", "color_front", "mask_front",
                 "color_back", "mask_back"):
        assert call(**{name: None}) == -1, name


# every case of tests/test_gpu_uv_project.py: the five meshes under both kinds of mask, the torus at tolerance 0
GPU_CASES = [c + (P.Z_TOL, k) for c in P.CASES for k in P.MASK_KINDS] + [("torus", 256, 0.0, "disc")]


@pytest.mark.parametrize("name,size,tol,masks", GPU_CASES)
def test_gpu_cases_are_sound(name, size, tol, masks):
    assert P.Z_TOL == U.Z_TOLERANCE
    c = P.case(name, size, tol, masks)
    assert np.abs(c["positions"]).max() <= 0.5
    share = c["fragile"].mean()
    assert share <= 0.005, share
    if name == "lattice":
        assert not c["fragile"].any()
    counts = [int((c["source"] == k).sum()) for k in (0, 1, 2)]
    assert counts[1] > 50, counts
    if name in P.CLOSED:
        assert counts[2] > 50, counts
    assert counts[0] > (c["face_id"] < 0).sum(), counts                      # some covered texel is left to the fallback
    if tol == 0.0:                                                           # a tolerance only ever admits texels
        assert not ((c["source"] > 0) & (P.case(name, size, P.Z_TOL, masks)["source"] == 0)).any()


# ------------------------------------------------------------------ the host statement of dsu_uv_project
def assert_host_entry_is_rule_e(c, **kw):
    """dsu_uv_project_area_host at s = 1, filter 0, count = NULL — the call dsu_uv_project's kernel is
    held to in tests/test_gpu_uv_project.py — against the restatement: every byte, fragile texels
    included."""
    image, source, count = A.host_project_area(c, 1, "nearest", with_count=False, **kw)
    assert count is None and image.dtype == source.dtype == np.uint8
    assert np.array_equal(source, c["source"]), int((source != c["source"]).sum())
    assert np.array_equal(image, c["image"]), int((image != c["image"]).any(-1).sum())


@pytest.mark.parametrize("name,size,tol,masks", GPU_CASES)
def test_host_entry_equals_the_restatement(name, size, tol, masks):
    assert_host_entry_is_rule_e(P.case(name, size, tol, masks))


def test_host_entry_with_a_non_finite_position():
    c = P.nan_vertex_case()
    bad = int(np.nonzero(np.isnan(c["positions"]).any(1))[0][0])
    touched = np.isin(c["face_id"], np.nonzero((c["indices"] == bad).any(1))[0])
    assert (P.case("character", 100)["source"][touched] > 0).any() and not c["source"][touched].any()
    assert_host_entry_is_rule_e(c)


@pytest.mark.parametrize("cells", (1, 40))
def test_host_entry_does_not_depend_on_the_grid(cells):
    c = P.case("body_and_arm", 64)
    grid = A.HostGrid(A.case_tris(c)[0], cells)
    assert len(grid.offsets) == cells * cells + 1 and (cells == 1 or (np.diff(grid.offsets) == 0).any())
    assert_host_entry_is_rule_e(c, grid=grid)
