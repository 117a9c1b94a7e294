"""GPU: the seam-levelling kernels (dsu_uv_seam_gather / dsu_uv_seam_apply, csrc/mesh_uv.hip) against
the library's host entries, which run the same text (csrc/uv_seam.h) on the CPU and are held to the
restatement by tests/test_uv_seam_host.py: EQUALITY of every byte is asserted, the gather's sums
being integers.  Then the solve through dsu_spd_cg_block against the restatement's sparse LU, and
bake_drawings(seam="level") on the device against the numpy backend (tests/uv_seam_ref.py) with a
synthetic projection, so dsu_uv_project is not involved."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_seam_ref as S  # noqa: E402
from drawingspinup_amd import ops  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dev, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _inputs(dev, c):
    return (_t(c["uvs"], dev, np.float32), _t(c["indices"], dev, np.int32), _t(c["group"], dev, np.int32),
            _t(c["face_id"], dev, np.int32), _t(c["source"], dev, np.uint8), _t(c["proj"], dev, np.uint8),
            _t(c["fallback"], dev, np.uint8))


def device_gather(dev, c):
    return ops.uv_seam_gather(*_inputs(dev, c), c["n_groups"])


def device_apply(dev, c, d):
    return ops.uv_seam_apply(*_inputs(dev, c), _t(np.asarray(d, np.float64).reshape(-1, 3), dev))


# ------------------------------------------------------------------ 1. kernels against host entries
@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("name,size", S.CASES)
def test_kernels_equal_the_host_entries(dev, name, size, pattern):
    c = S.seam_case(name, size, pattern)
    want_num, want_den = S.host_gather(c)
    num, den = device_gather(dev, c)
    assert num.dtype == torch.int64 and den.dtype == torch.int64 and num.shape == (c["n_groups"], 3)
    assert np.array_equal(num.cpu().numpy(), want_num) and np.array_equal(den.cpu().numpy(), want_den)
    assert want_num.any() and (want_den >= S.ONE).any()
    d = S.restated(name, size, pattern)["d"]
    image = device_apply(dev, c, d)
    assert image.dtype == torch.uint8 and np.array_equal(image.cpu().numpy(), S.host_apply(c, d))


EDGE = S.edge_cases()


@pytest.mark.parametrize("row", sorted(EDGE))
def test_edge_rows_equal_the_host_entries(dev, row):
    """Face ids, vertex indices and groups out of range, a NaN uv, a zero-area face, source 1 / 2 / 255,
    slivers, nothing and everything projected, NaN and huge offsets: nothing is read out of bounds and
    every byte is the host entry's."""
    c, d = EDGE[row]
    want_num, want_den = S.host_gather(c)
    num, den = device_gather(dev, c)
    assert np.array_equal(num.cpu().numpy(), want_num) and np.array_equal(den.cpu().numpy(), want_den)
    if d is None:
        d = S.offsets(want_num, want_den, c["group_faces"])[0]
    assert np.array_equal(device_apply(dev, c, d).cpu().numpy(), S.host_apply(c, d))


def test_no_groups_and_wrapper_checks(dev):
    c = S.seam_case("triangle")
    args = _inputs(dev, c)
    num, den = ops.uv_seam_gather(*args, 0)
    assert num.shape == (0, 3) and den.shape == (0,)
    keep = np.where((c["source"] != 0)[..., None], c["proj"], c["fallback"])
    want = np.where((c["face_id"] >= 0)[..., None], keep, 0)
    assert np.array_equal(ops.uv_seam_apply(*args, torch.zeros(0, 3, dtype=torch.float64, device=dev)).cpu().numpy(),
                          want)
    with pytest.raises(ValueError):
        ops.uv_seam_gather(*args[:2], args[2][:-1], *args[3:], 3)             # one group short
    with pytest.raises(ValueError):
        ops.uv_seam_gather(*args[:4], args[4].to(torch.int32), *args[5:], 3)  # source not uint8
    with pytest.raises(ValueError):
        ops.uv_seam_apply(*args, torch.zeros(3, 2, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        ops.uv_seam_apply(*args[:6], args[6][:-1], torch.zeros(3, 3, dtype=torch.float64, device=dev))


def test_bit_identical_repeats_and_streams(dev):
    c = S.seam_case("icosphere", 64)
    d = S.restated("icosphere", 64)["d"]

    def run():
        num, den = device_gather(dev, c)
        return num, den, device_apply(dev, c, d)
    a = run()
    b = run()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        e = run()
    f = run()                                                                 # beside the side stream's run
    torch.cuda.synchronize(dev)
    for other in (b, e, f):
        for x, y in zip(a, other):
            assert torch.equal(x, y)


# ------------------------------------------------------------------ 2. the solve
@pytest.mark.parametrize("name,size,pattern,colours", S.LEVEL_CASES[:4])
def test_cg_solve_equals_the_sparse_lu(dev, name, size, pattern, colours):
    c, r = S.seam_case(name, size, pattern, colours), S.restated(name, size, pattern, colours)
    be = U.DeviceBackend(dev)
    d, known = U.seam_offsets(r["num"], r["den"], c["group_faces"], be)
    assert np.array_equal(known, r["known"]) and (~known).sum() >= 10
    err = np.abs(d - r["d"]).max()
    print(name, size, pattern, colours, "unknown", int((~known).sum()), "iterations", be.seam_iterations, "error", err)
    assert be.seam_iterations >= 2 and err <= 1e-8
    assert np.array_equal(d[known], r["d"][known])


# ------------------------------------------------------------------ 3. bake_drawings on the device
@pytest.mark.parametrize("name,size,pattern,colours", S.LEVEL_CASES)
def test_bake_drawings_level_equals_the_numpy_backend(dev, name, size, pattern, colours):
    """Equal outside the restatement's fragile texels (v + 0.5 within 1e-6 of an integer: the CG's
    rounding may tip them), which are at most 0.5 % of the levelled texels; none for the constant
    offset, which is byte-equal."""
    c, r = S.seam_case(name, size, pattern, colours), S.restated(name, size, pattern, colours)
    got = S.bake_level(c, U.DeviceBackend(dev), convert=lambda a: _t(a, dev))
    levelled, fragile = int(r["levelled"].sum()), int(r["fragile"].sum())
    print(name, size, pattern, colours, "levelled", levelled, "fragile", fragile, "differing texels",
          int((got != r["image"]).any(-1).sum()))
    assert fragile <= S.FRAGILE_CAP * levelled and (colours != "constant" or fragile == 0)
    keep = ~r["fragile"]
    assert got.dtype == np.uint8 and np.array_equal(got[keep], r["image"][keep])
    filled = S.bake_level(c, U.DeviceBackend(dev), gutter=2, convert=lambda a: _t(a, dev))
    assert np.array_equal(filled[c["face_id"] >= 0], got[c["face_id"] >= 0]) and (filled != got).any()


# ------------------------------------------------------------------ 4. end to end
def test_save_obj_level_keeps_the_drawing_texels(dev, tmp_path):
    """save_obj(texture_source="drawings", texture_seam="level") with the real projection: the texels a
    drawing sees carry the bytes of the export without the keyword, the others are levelled, and the
    PNG is bake_drawings(seam="level") over seam_groups of the exported mesh; "none" = the keyword
    left out, byte for byte."""
    from PIL import Image
    import uv_field_ref as F
    import uv_project_ref as P
    from drawingspinup_amd.nsr import mesh as M
    v, f = F.icosphere()
    v = torch.from_numpy(v.astype(np.float64) * 1.9).to(dev)                # radius 0.475 in the projection frame
    f = torch.from_numpy(f).to(dev)
    cf, cb = P.drawings()
    cbp = {"color_front": _t(cf, dev), "color_back": _t(cb, dev), "erode": 5, "mask_front": _t(P.disc_masks()[0], dev)}
    kw = dict(shearing=True, color_back_projection=cbp, export_uv=True, texture_size=64, texture_source="drawings")
    M.save_obj(str(tmp_path / "l" / "c.obj"), v, f, None, texture_seam="level", **kw)
    M.save_obj(str(tmp_path / "n" / "c.obj"), v, f, None, texture_seam="none", **kw)
    M.save_obj(str(tmp_path / "o" / "c.obj"), v, f, None, **kw)
    for name in ("c.mtl", "c.obj", "c.png"):
        assert open(tmp_path / "n" / name, "rb").read() == open(tmp_path / "o" / name, "rb").read(), name
    for name in ("c.mtl", "c.obj"):
        assert open(tmp_path / "l" / name, "rb").read() == open(tmp_path / "o" / name, "rb").read(), name
    level, old = np.array(Image.open(tmp_path / "l" / "c.png")), np.array(Image.open(tmp_path / "o" / "c.png"))
    out, fz, col, frame = M.post_process_mesh(v, f, None, 1.35, False, True, cbp, return_projection_frame=True)
    vm, ind, uvs = U.parametrize(out, fz, 64, 2, device=dev)
    args = (uvs, ind, frame[vm], cbp["color_front"], cbp["mask_front"], cbp["color_back"], col[vm], 64)
    _, fid, src = U.bake_drawings(*args, 0, erode=5, device=dev, return_maps=True)
    seen, unseen = (fid >= 0) & (src > 0), (fid >= 0) & (src == 0)
    assert seen.sum() > 100 and unseen.sum() > 20
    assert np.array_equal(level[seen], old[seen]) and (level[unseen] != old[unseen]).any()
    groups, gf = U.seam_groups(np.asarray(out, np.float64), np.asarray(fz), vm)
    want = U.bake_drawings(*args, 2, erode=5, device=dev, seam="level", groups=groups, group_faces=gf)
    assert np.array_equal(level, want)


def test_levelling_removes_the_tone_step_on_the_device(dev):
    """tests/test_uv_seam_host.py's test of the same name on the device: the seam step against the figures
    measured there on the CPU (uv_seam_ref.STEP_BEFORE / STEP_AFTER), with the same margin of 2."""
    c = S.seam_case("icosphere", 64, "z", "tone")
    src, fid, chart = c["source"], c["face_id"], c["face_chart"]
    hard = np.where((src > 0)[..., None], c["proj"], c["fallback"])
    before = S.seam_step(hard, src, fid, chart)[0]
    got = S.bake_level(c, U.DeviceBackend(dev), convert=lambda a: _t(a, dev))
    after, pairs = S.seam_step(got, src, fid, chart)
    print("pairs", pairs, "before", before, "after", after)
    assert before == pytest.approx(S.STEP_BEFORE, abs=1e-9)
    assert after <= 2.0 * S.STEP_AFTER and after < before
    assert np.array_equal(got[src > 0], c["proj"][src > 0])                 # the drawing texels are left alone
