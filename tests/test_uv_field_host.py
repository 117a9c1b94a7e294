"""CPU: the field bake's rule (include/dsu_hip.h, UV export f. and g.) through the library's host
entries dsu_uv_field_points_host / dsu_uv_field_resolve_host — the text the kernels compile
(csrc/uv_field.h) — against the float64 restatement tests/uv_field_ref.py, bit for bit; bake_field /
uv_mapping through the numpy backend; the switches of save_obj and recon.
tests/test_gpu_uv_field.py holds the kernels to these host entries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_field_ref as F  # noqa: E402
import uv_ref as R  # noqa: E402
from drawingspinup_amd import _lib  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402


host_points, host_resolve = F.host_points, F.host_resolve


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ points
@pytest.mark.parametrize("s", F.SAMPLES)
@pytest.mark.parametrize("name,size", F.CASES)
def test_points_equal_the_restatement_bit_for_bit(name, size, s):
    c, want = F.case(name, size), F.restated(name, size, s)
    # the small cases fill part of a workgroup, the icosphere more than one even at s = 1
    assert len(c["texels"]) >= (60 if name != "icosphere" else 257)
    points, valid = host_points(c, s)
    assert np.array_equal(valid, want["valid"]) and valid.all()            # covered texels of sound faces
    assert np.array_equal(bits(points), bits(want["points"]))
    # not vacuous: the samples differ from one another, and for s > 1 some fall outside their face
    assert len(np.unique(points.reshape(-1, 3), axis=0)) > 0.9 * points.shape[0] * s * s
    if s > 1:
        assert (want["b"].min(-1) < 0).any()


@pytest.mark.parametrize("name,size", F.CASES)
def test_one_sample_is_the_projection_rule_point(name, size):
    """s = 1: the texel's own sample point, b_i and p as dsu_uv_project's steps 1-2 — restated here
    with the expression of tests/uv_project_ref.py (project(): R._edges at (c, size - 1 - r), w / area,
    (b0 Pa + b1 Pb) + b2 Pc)."""
    c = F.case(name, size)
    S = c["size"]
    uv = c["uvs"].astype(np.float64) * float(S)
    pos = c["positions"].astype(np.float64)
    rows, cols = np.nonzero(c["face_id"] >= 0)
    m = c["face_id"][rows, cols]
    ia, ib, ic = c["indices"][m, 0], c["indices"][m, 1], c["indices"][m, 2]
    px, py = cols.astype(np.float64), (S - 1 - rows).astype(np.float64)
    w0, w1, w2 = R._edges((uv[ia, 0], uv[ia, 1], uv[ib, 0], uv[ib, 1], uv[ic, 0], uv[ic, 1]), px, py)
    area = (w0 + w1) + w2
    b0, b1, b2 = w0 / area, w1 / area, w2 / area
    p = (b0[:, None] * pos[ia] + b1[:, None] * pos[ib]) + b2[:, None] * pos[ic]
    assert np.array_equal(rows * S + cols, c["texels"])                    # ascending, row-major
    points, valid = host_points(c, 1)
    assert valid.all() and np.array_equal(bits(points[:, 0]), bits(p.astype(np.float32)))
    assert min(b0.min(), b1.min(), b2.min()) >= 0                          # the bake's own sample: inside


def test_lattice_points_are_exact():
    """Dyadic uvs and positions: every sample is its exact point, x = u - 1/2, y = v - 1/4,
    z = u / 4 + v / 2 - 1/8 at u = (c + o) / 16, v = (15 - r + o) / 16 — outside the square too."""
    c = F.case("lattice")
    assert len(c["texels"]) == 81
    for s in F.SAMPLES:
        points, valid = host_points(c, s)
        assert valid.all()
        r, col = c["texels"] // 16, c["texels"] % 16
        j = np.arange(s * s)
        o = lambda i: (2 * i + 1 - s) / (2.0 * s)
        u = (col[:, None] + o(j % s)[None]) / 16.0
        v = ((15 - r)[:, None] + o(j // s)[None]) / 16.0
        want = np.stack([u - 0.5, v - 0.25, 0.25 * u + 0.5 * v - 0.125], -1)
        assert np.array_equal(points.astype(np.float64), want)
        if s > 1:
            assert ((u < 2 / 16) | (v > 10 / 16)).any()                    # beyond the square's border


def test_sub_samples_outside_their_face_stay_in_its_plane():
    for name, size in F.CASES:
        c, r = F.case(name, size), F.restated(name, size, 4)
        outside = (r["b"].min(-1) < 0) & (r["valid"] > 0)
        assert outside.sum() > 20, name
        points, valid = host_points(c, 4)
        assert valid[outside].all()
        tri = c["positions"].astype(np.float64)[c["indices"][c["face_id"].reshape(-1)[c["texels"]]]]   # (T,3,3)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        dist = np.abs(np.einsum("tjk,tk->tj", r["p64"] - tri[:, None, 0], n))
        assert dist[outside].max() <= 1e-12, (name, dist[outside].max())
        # the f32 point is that point's one rounding
        assert np.array_equal(bits(points[outside]), bits(r["p64"][outside].astype(np.float32)))
        if name == "lattice":                                              # exact there: the f32 point itself
            d32 = np.abs(np.einsum("tjk,tk->tj", points.astype(np.float64) - tri[:, None, 0], n))
            assert d32[outside].max() <= 1e-12


@pytest.mark.parametrize("s", F.SAMPLES)
def test_edge_rows_are_invalid_and_zero(s):
    c, rows = F.edge_rows()
    points, valid = host_points(c, s)
    want = F.field_samples(c["uvs"], c["indices"], c["positions"], c["face_id"], c["texels"], s)
    assert np.array_equal(valid, want["valid"]) and np.array_equal(bits(points), bits(want["points"]))
    assert not np.isnan(points).any()
    where = {int(t): k for k, t in enumerate(c["texels"])}
    for kind, texels in rows.items():
        assert len(texels) > 0, kind
        k = [where[int(t)] for t in texels]
        assert not valid[k].any() and not points[k].any(), kind
    assert valid.mean() > 0.9                                              # the rest is untouched by them


def test_no_texels_and_argument_checks():
    """include/dsu_hip.h f. and g.: DSU_EINVAL for every argument named there, DSU_OK and nothing
    touched for an empty list (checked in this order: ranges, outputs, the empty list, inputs) — the
    device entries return before any launch, so they are called here too."""
    lib = _lib.lib()
    p = ctypes.c_void_p(64)                                                   # never dereferenced

    def points(fn, **kw):
        a = dict(uvs=p, indices=p, positions=p, n_verts=4, n_faces=2, size=64, face_id=p, texels=p, n_texels=0,
                 s=2, points=p, valid=p)
        assert set(kw) <= set(a)
        a.update(kw)
        return fn(*a.values(), *([None] if fn is lib.dsu_uv_field_points else []))

    def resolve(fn, **kw):
        a = dict(colours=p, valid=p, texels=p, n_texels=0, s=2, size=64, image=p)
        assert set(kw) <= set(a)
        a.update(kw)
        return fn(*a.values(), *([None] if fn is lib.dsu_uv_field_resolve else []))
    big = (1 << 30) + 1
    for fn in (lib.dsu_uv_field_points, lib.dsu_uv_field_points_host):
        assert points(fn) == 0
        assert points(fn, uvs=None, indices=None, positions=None, face_id=None, texels=None) == 0
        for bad in (dict(size=0), dict(size=8193), dict(s=0), dict(s=9), dict(n_verts=-1), dict(n_faces=-1),
                    dict(n_texels=-1), dict(n_verts=big), dict(n_faces=big), dict(n_texels=big), dict(points=None),
                    dict(valid=None), dict(n_texels=3, face_id=None), dict(n_texels=3, texels=None),
                    dict(n_texels=3, uvs=None), dict(n_texels=3, indices=None), dict(n_texels=3, positions=None),
                    dict(n_texels=3, n_verts=0)):
            assert points(fn, **bad) == -1, bad
    for fn in (lib.dsu_uv_field_resolve, lib.dsu_uv_field_resolve_host):
        assert resolve(fn) == 0 and resolve(fn, colours=None, valid=None, texels=None) == 0
        for bad in (dict(size=0), dict(size=8193), dict(s=0), dict(s=9), dict(n_texels=-1), dict(n_texels=big),
                    dict(image=None), dict(n_texels=3, colours=None), dict(n_texels=3, valid=None),
                    dict(n_texels=3, texels=None)):
            assert resolve(fn, **bad) == -1, bad
    # an empty list writes nothing
    c = F.case("triangle")
    pts, valid = host_points(c, 2, texels=np.zeros(0, np.int32))
    assert pts.shape == (0, 4, 3) and valid.shape == (0, 4)
    img = np.full((16, 16, 3), 33, np.uint8)
    host_resolve(np.zeros((0, 4, 3), np.float32), np.zeros((0, 4), np.uint8), np.zeros(0, np.int32), img, 2)
    assert (img == 33).all()


# ------------------------------------------------------------------ resolve
@pytest.mark.parametrize("s", F.SAMPLES)
def test_resolve_equals_the_restatement_byte_for_byte(s):
    c = F.case("icosphere", 37)
    tex = np.concatenate([c["texels"], np.asarray([-1, 37 * 37], np.int32)])      # two that write nothing
    col, valid = F.resolve_inputs(len(tex), s, seed=s)
    got = host_resolve(col, valid, tex, np.full((37, 37, 3), 201, np.uint8), s)
    want = F.field_resolve(col, valid, tex, np.full((37, 37, 3), 201, np.uint8))
    assert np.array_equal(got, want)
    listed = np.zeros(37 * 37, bool)
    listed[c["texels"]] = True
    assert (got.reshape(-1, 3)[~listed] == 201).all()                      # written only at the listed texels
    empty = c["texels"][valid[:len(c["texels"])].sum(1) == 0]
    assert len(empty) >= len(c["texels"]) // 7 and (got.reshape(-1, 3)[empty] == 201).all()    # no valid sample: the byte stays
    assert len(np.unique(got.reshape(-1, 3)[listed])) > 100


def test_resolve_quantises_as_the_bake_does():
    tex = np.arange(6, dtype=np.int32)
    col = np.zeros((6, 4, 3), np.float32)
    valid = np.ones((6, 4), np.uint8)
    col[0] = [[0.5, 1.0, 0.0]] * 4                                         # 127.5 -> 127 (truncated), 255, 0
    col[1] = [[-3.0, 1.5, 0.999]] * 4                                      # below 0 and above 1 clip
    col[2, 0] = [np.nan, 0.2, 0.2]                                         # a NaN among the valid: NaN -> 0
    col[2, 1:] = 0.2
    col[3] = 0.9
    valid[3] = 0                                                           # no valid sample
    col[4, :2], col[4, 2:] = 1.0, np.nan                                   # the invalid ones are not read
    valid[4, 2:] = 0
    col[5, 0], col[5, 1:] = 0.25, 0.75                                     # mean of four: (0.25 + 3 * 0.75) / 4
    img = host_resolve(col, valid, tex, np.full((4, 4, 3), 99, np.uint8), 2).reshape(-1, 3)
    assert img[0].tolist() == [127, 255, 0]
    assert img[1].tolist() == [0, 255, int(np.float64(np.float32(0.999)) * 255)]
    assert img[2, 0] == 0 and img[2, 1] == img[2, 2] == 51
    assert img[3].tolist() == [99, 99, 99] and (img[6:] == 99).all()
    assert img[4].tolist() == [255, 255, 255]
    assert img[5].tolist() == [int(0.625 * 255)] * 3


# ------------------------------------------------------------------ bake_field through the numpy backend
def _affine_vertex_colours(c):
    return F.affine(c["positions"])                                        # float64 at the (f32) vertices


def test_bake_field_of_an_affine_field_is_the_vertex_bake():
    """Barycentric interpolation of an affine function is the function: with one sample per texel the
    field bake and the vertex bake of the same affine colours differ by at most one level, and only
    where the float64 value x 255 lies within 1e-4 of an integer (the f32 roundings of p and of the
    colours move it by about 2e-5 of a level)."""
    for size in (64, 37):
        c = F.case("icosphere", size)
        be = F.RefBackend()
        vertex = U.bake_vertex_colours(c["uvs"], c["indices"], _affine_vertex_colours(c), size, 0, backend=be)
        field, fid, evaluated = U.bake_field(c["uvs"], c["indices"], c["positions"], F.affine, None, size, 0, samples=1,
                                             backend=be, return_maps=True)
        covered = c["face_id"] >= 0
        assert np.array_equal(fid, c["face_id"]) and np.array_equal(evaluated > 0, covered)
        assert not field[~covered].any() and not vertex[~covered].any()
        exact = F.affine(F.restated("icosphere", size, 1)["p64"][:, 0]) * 255.0        # (T,3) levels
        assert 0.05 * 255 <= exact.min() and exact.max() <= 0.95 * 255
        a, b = field[covered].astype(np.int64), vertex[covered].astype(np.int64)
        diff = np.abs(a - b)
        print(size, "texels", int(covered.sum()), "differing bytes", int((diff > 0).sum()))
        assert diff.max() <= 1
        near = np.abs(exact - np.rint(exact)) <= 1e-4
        assert not (diff > 0)[~near].any(), int((diff > 0)[~near].sum())
        assert np.abs(a - np.floor(exact))[~near].max() == 0               # and both are the function itself
        assert len(np.unique(a)) > 60


def test_bake_field_chunks_fallback_and_gutter():
    c = F.case("icosphere", 37)
    be = F.RefBackend()
    calls = []

    def counted(p):
        calls.append(len(p))
        return F.stripes(p)
    n = len(c["texels"])
    whole = U.bake_field(c["uvs"], c["indices"], c["positions"], F.stripes, None, 37, 2, samples=2, backend=be)
    pieces = U.bake_field(c["uvs"], c["indices"], c["positions"], counted, None, 37, 2, samples=2, chunk=4 * 90,
                          backend=be)
    assert np.array_equal(whole, pieces)
    assert calls == [360] * (n // 90) + ([4 * (n % 90)] if n % 90 else []) and len(calls) >= 3
    # the gutter fill runs over the result
    bare, fid, ev = U.bake_field(c["uvs"], c["indices"], c["positions"], F.stripes, None, 37, 0, samples=2, backend=be,
                                 return_maps=True)
    assert np.array_equal(whole, R.dilate(bare, fid >= 0, 2)[0]) and (whole != bare).any()
    # a texel without a valid sample keeps the vertex bake of the fallback colours
    pos = np.array(c["positions"])
    bad = int(c["indices"][fid[fid >= 0][n // 2], 0])
    pos[bad] = np.inf
    fallback = np.full((len(pos), 3), 0.4, np.float32)
    got, fid2, ev2 = U.bake_field(c["uvs"], c["indices"], pos, F.stripes, fallback, 37, 0, samples=2, backend=be,
                                  return_maps=True)
    touched = np.isin(fid, np.nonzero((c["indices"] == bad).any(1))[0])
    assert touched.sum() > 0 and not ev2[touched].any() and np.array_equal(ev2 > 0, (fid >= 0) & ~touched)
    assert (got[touched] == int(np.float64(np.float32(0.4)) * 255)).all()
    assert np.array_equal(got[~touched], bare[~touched])
    with pytest.raises(ValueError):
        U.bake_field(c["uvs"], c["indices"], c["positions"], F.stripes, None, 37, 2, samples=9, backend=be)
    with pytest.raises(ValueError):
        U.bake_field(c["uvs"], c["indices"], c["positions"], None, None, 37, 2, backend=be)


def test_the_vertex_bake_cannot_hold_the_stripes():
    """What the feature adds: stripes narrower than an edge are in the field bake and not in the
    vertex bake of the same function."""
    c = F.case("icosphere", 64)
    be = F.RefBackend()
    field = U.bake_field(c["uvs"], c["indices"], c["positions"], F.stripes, None, 64, 0, samples=1, backend=be)
    vertex = U.bake_vertex_colours(c["uvs"], c["indices"], F.stripes(c["positions"]), 64, 0, backend=be)
    covered = c["face_id"] >= 0
    want = (F.stripes(F.restated("icosphere", 64, 1)["points"][:, 0]) * 255.0).astype(np.uint8)
    assert np.array_equal(field[covered], want)
    assert (field[covered] != vertex[covered]).any(-1).mean() > 0.5


def test_uv_mapping_takes_the_field_in_old_vertex_order():
    v, f = F.icosphere()
    shown = v.astype(np.float64) * 1.35 + 0.01                             # the exported frame is another one
    col = np.full((len(v), 3), 0.5, np.float32)
    be = F.RefBackend()
    fld = {"positions": v, "eval_colours": F.stripes, "samples": 2, "chunk": 1000}
    got = U.uv_mapping(shown, f, col, "s", size=37, backend=be, field=fld)
    plain = U.uv_mapping(shown, f, col, "s", size=37, backend=be)
    for k in ("verts", "faces", "uvs"):
        assert np.array_equal(got[k], plain[k])
    vm, ind, uvs = U.parametrize(shown, f, 37, 2, backend=be)
    want = U.bake_field(uvs, ind, v[vm], F.stripes, col[vm], 37, 2, samples=2, backend=be)
    assert np.array_equal(got["image"], want) and not np.array_equal(got["image"], plain["image"])
    assert np.array_equal(U.uv_mapping(shown, f, col, "s", size=37, backend=be, field=None)["image"], plain["image"])


def test_drawings_are_composed_over_the_field_bake():
    """bake_drawings(fallback_image=): texels a drawing sees carry the drawing, the others the field
    bake; without the argument nothing changes."""
    import uv_project_ref as P
    v, f = F.icosphere()
    # another frame than the field's; radius 0.5 against the masks' disc of 0.45: a rim is left to the fallback
    frame = np.stack([v[:, 0], v[:, 2], -v[:, 1]], -1)
    cf, cb = P.drawings()
    masks = P.disc_masks()
    be = F.RefBackend(masks)
    col = np.full((len(v), 3), 0.5, np.float32)
    pr = {"positions": frame, "color_front": cf, "mask_front": None, "color_back": cb}
    fld = {"positions": v, "eval_colours": F.stripes, "samples": 2}
    both = U.uv_mapping(v, f, col, "s", size=64, backend=be, projection=pr, field=fld)["image"]
    vm, ind, uvs = U.parametrize(v, f, 64, 2, backend=be)
    drawn, fid, src = U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 0, backend=be, return_maps=True)
    field = U.bake_field(uvs, ind, v[vm], F.stripes, col[vm], 64, 0, samples=2, backend=be)
    covered = fid >= 0
    assert (src[covered] > 0).sum() > 100 and (src[covered] == 0).sum() > 100
    want = np.where((src > 0)[..., None], drawn, field)
    assert np.array_equal(both, R.dilate(want, covered, 2)[0])
    assert (field[covered & (src == 0)] != drawn[covered & (src == 0)]).any()
    again = U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 0, backend=be, fallback_image=None)
    assert np.array_equal(again, drawn)


# ------------------------------------------------------------------ switches
def test_save_obj_refuses_the_field_without_its_needs(tmp_path):
    from drawingspinup_amd.nsr import mesh as M
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    f, c = torch.tensor([[0, 1, 2]]), torch.full((3, 3), 0.5)
    fn = lambda p: p
    with pytest.raises(ValueError):
        M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="field", texture_field=fn)          # no export_uv
    with pytest.raises(ValueError):
        M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="field", export_uv=True)            # no callable
    with pytest.raises(ValueError):
        M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="field", export_uv=True, texture_field=3)
    with pytest.raises(ValueError):
        M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="photo", export_uv=True, texture_field=fn)
    assert os.listdir(tmp_path) == []
    # "vertex" ignores the field: the plain export, byte for byte
    M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_source="vertex", texture_field=fn, texture_samples=4)
    M.save_obj(str(tmp_path / "b.obj"), v, f, c)
    assert open(tmp_path / "a.obj", "rb").read() == open(tmp_path / "b.obj", "rb").read()


def test_field_colours_evaluates_as_vertex_colors():
    from drawingspinup_amd.nsr import mesh as M

    class Model:
        def geometry(self, p, with_grad, with_feature):
            assert with_grad and with_feature and p.dtype == torch.float32
            return p[:, 0], p * 2.0, p + 1.0

        def texture(self, feat, view, normal):
            return feat * 0.25 + normal - view
    fn = M.field_colours(Model())
    p = torch.tensor([[0.1, 0.2, 0.3], [-0.5, 0.25, 0.0]])
    assert torch.equal(fn(p), M.vertex_colors(Model(), p)) and fn(p).shape == (2, 3)


def test_recon_reads_the_field_source_without_a_default_key():
    from drawingspinup_amd.entry import recon
    _, conf = recon.parse(["--uid", "u"])
    assert "texture_source" not in conf["export"] and "texture_samples" not in conf["export"]
    _, conf = recon.parse(["--uid", "u", "--texture_source", "field", "export.export_uv=true"])
    assert conf["export"]["texture_source"] == "field" and conf["export"].get("texture_samples", 2) == 2
    _, conf = recon.parse(["--uid", "u", "export.texture_source=field", "export.export_uv=true",
                           "export.texture_samples=4", "--no-color_back_projection"])
    assert conf["export"]["texture_source"] == "field" and int(conf["export"]["texture_samples"]) == 4
    for argv in (["--texture_source", "field"], ["export.texture_source=field"], ["--texture_source", "photo"],
                 ["--texture_source", "field", "export.export_uv=true", "export.texture_samples=9"]):
        with pytest.raises(SystemExit):
            recon.parse(["--uid", "u"] + argv)
