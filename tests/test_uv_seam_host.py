"""CPU: seam levelling (include/dsu_hip.h, UV export h. and i.) through the library's host entries
dsu_uv_seam_gather_host / dsu_uv_seam_apply_host — the text the kernels compile (csrc/uv_seam.h) —
against the float64 / int64 restatement tests/uv_seam_ref.py, bit for bit; the host step
(nsr/uv.seam_offsets) against the restatement's own; bake_drawings / uv_mapping through the numpy
backend; the switches of save_obj and recon.  tests/test_gpu_uv_seam.py holds the kernels to these
host entries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_field_ref as F  # noqa: E402
import uv_project_ref as P  # noqa: E402
import uv_ref as R  # noqa: E402
import uv_seam_ref as S  # noqa: E402
from drawingspinup_amd import _lib  # noqa: E402
from drawingspinup_amd.nsr import uv as U  # noqa: E402

STEP_BEFORE, STEP_AFTER = S.STEP_BEFORE, S.STEP_AFTER


def _args(c):
    return c["uvs"], c["indices"], c["group"], c["n_groups"], c["face_id"], c["source"], c["proj"], c["fallback"]


def _restate(c, d=None):
    num, den = S.gather(*_args(c))
    if d is None:
        d = S.offsets(num, den, c["group_faces"])[0]
    a = _args(c)
    return num, den, d, S.apply(*a[:3], *a[4:], d)


# ------------------------------------------------------------------ 1. the host entries, bit for bit
@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("name,size", S.CASES)
def test_host_entries_equal_the_restatement(name, size, pattern):
    c, want = S.seam_case(name, size, pattern), S.restated(name, size, pattern)
    covered = c["face_id"] >= 0
    # not vacuous: projected and fallback texels, known groups, and on the icosphere unknown ones
    assert (c["source"][covered] != 0).sum() >= 10 and (c["source"][covered] == 0).sum() >= 10
    assert want["known"].any() and (name != "icosphere" or (~want["known"]).sum() >= 10)
    num, den = S.host_gather(c)
    assert np.array_equal(num, want["num"]) and np.array_equal(den, want["den"])
    assert num.any() and (den > 0).any()
    image = S.host_apply(c, want["d"])
    assert np.array_equal(image, want["image"])
    assert not image[~covered].any()
    lev = want["levelled"]
    assert lev.sum() >= 10 and (image[lev] != c["fallback"][lev]).any()
    # the host step of the package against the restatement's own bookkeeping
    d, known = U.seam_offsets(num, den, c["group_faces"], S.RefBackend())
    assert np.array_equal(known, want["known"]) and np.abs(d - want["d"]).max() <= 1e-9
    assert np.array_equal(d[known], want["d"][known])


EDGE = S.edge_cases()


@pytest.mark.parametrize("row", sorted(EDGE))
def test_edge_rows_equal_the_restatement(row):
    c, d = EDGE[row]
    num, den, d, want = _restate(c, d)
    got_num, got_den = S.host_gather(c)
    assert np.array_equal(got_num, num) and np.array_equal(got_den, den)
    image = S.host_apply(c, d)
    assert np.array_equal(image, want)
    covered = c["face_id"] >= 0
    base = S.restated("icosphere", 37)
    if row in ("face_id_out_of_range", "vertex_index_out_of_range", "group_out_of_range", "nan_uv", "zero_area_face"):
        sound = S.corners(c["uvs"], c["indices"], c["group"], c["n_groups"], c["face_id"])[0].reshape(covered.shape)
        broken = covered & ~sound
        assert broken.sum() >= 2 and (broken & (c["source"] == 0)).any() and (broken & (c["source"] != 0)).any()
        assert np.array_equal(image[broken], np.where((c["source"] != 0)[..., None], c["proj"], c["fallback"])[broken])
        assert not np.array_equal(num, base["num"])                        # their texels added nothing
    elif row == "source_1_2_255":
        assert set(np.unique(c["source"])) == {0, 1, 2, 255}
        assert np.array_equal(num, base["num"]) and np.array_equal(image, base["image"])   # any non-zero is projected
    elif row == "nothing_projected":
        assert not num.any() and not den.any() and not d.any()
        assert np.array_equal(image, np.where(covered[..., None], c["fallback"], 0))
    elif row == "everything_projected":
        assert np.array_equal(image, np.where(covered[..., None], c["proj"], 0))
    elif row == "nan_in_d":
        lev = base["levelled"]
        assert (image[lev] == c["fallback"][lev]).all(-1).any() and (image[lev] != c["fallback"][lev]).any()
        assert not np.isfinite(d).all()
    elif row == "past_0_and_255":
        lev = base["levelled"]
        assert (image[lev] == 0).any() and (image[lev] == 255).any()
    elif row == "slivers_only":
        assert ((den > 0) & (den < S.ONE)).sum() == 3 and int(den.sum()) in (S.ONE - 1, S.ONE, S.ONE + 1)
        d2, known = U.seam_offsets(num, den, c["group_faces"], S.RefBackend())
        assert not known.any() and not d2.any()
        keep = np.where((c["source"] != 0)[..., None], c["proj"], c["fallback"])
        assert np.array_equal(image, np.where(covered[..., None], keep, 0))


def test_argument_checks():
    """include/dsu_hip.h h. and i.: DSU_EINVAL for every argument named there, DSU_OK and nothing touched
    for a gather without groups or faces — the device entries return before any launch for these, so
    they are called here too."""
    lib = _lib.lib()
    p = ctypes.c_void_p(64)                                                   # never dereferenced
    big = (1 << 30) + 1

    def gather(fn, **kw):
        a = dict(uvs=p, indices=p, group=p, n_verts=4, n_faces=0, n_groups=3, size=64, face_id=p, source=p, proj=p,
                 fallback=p, num=p, den=p)
        assert set(kw) <= set(a)
        a.update(kw)
        return fn(*a.values(), *([None] if fn is lib.dsu_uv_seam_gather else []))

    def apply(fn, **kw):
        a = dict(uvs=p, indices=p, group=p, n_verts=4, n_faces=2, n_groups=3, size=64, face_id=p, source=p, proj=p,
                 fallback=p, d=p, image=p)
        assert set(kw) <= set(a)
        a.update(kw)
        return fn(*a.values(), *([None] if fn is lib.dsu_uv_seam_apply else []))
    ranges = (dict(size=0), dict(size=8193), dict(n_verts=-1), dict(n_faces=-1), dict(n_groups=-1), dict(n_verts=big),
              dict(n_faces=big), dict(n_groups=big))
    for fn in (lib.dsu_uv_seam_gather, lib.dsu_uv_seam_gather_host):
        assert gather(fn) == 0 and gather(fn, n_faces=2, n_groups=0) == 0
        assert gather(fn, uvs=None, indices=None, group=None, face_id=None, source=None, proj=None, fallback=None) == 0
        for bad in ranges + (dict(num=None), dict(den=None), dict(n_faces=2, uvs=None), dict(n_faces=2, indices=None),
                             dict(n_faces=2, group=None), dict(n_faces=2, n_verts=0), dict(n_faces=2, face_id=None),
                             dict(n_faces=2, source=None), dict(n_faces=2, proj=None), dict(n_faces=2, fallback=None)):
            assert gather(fn, **bad) == -1, bad
    for fn in (lib.dsu_uv_seam_apply, lib.dsu_uv_seam_apply_host):
        for bad in ranges + (dict(image=None), dict(face_id=None), dict(source=None), dict(proj=None),
                             dict(fallback=None), dict(uvs=None), dict(indices=None), dict(group=None), dict(d=None),
                             dict(n_verts=0)):
            assert apply(fn, **bad) == -1, bad
    # without groups or faces nothing of the atlas is read, and the composition is still written
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in S.seam_case("triangle").items()}
    keep = np.where((c["source"] != 0)[..., None], c["proj"], c["fallback"])
    want = np.where((c["face_id"] >= 0)[..., None], keep, 0)
    assert np.array_equal(S.host_apply(c, np.zeros((0, 3))), want)
    assert np.array_equal(S.apply(*_args(c)[:3], *_args(c)[4:], np.zeros((0, 3))), want)
    num, den = S.host_gather(dict(c, n_groups=0))
    assert num.shape == (0, 3) and den.shape == (0,)


# ------------------------------------------------------------------ 2. a constant offset
@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("name,size", S.CASES)
def test_constant_offset_is_recovered_exactly(name, size, pattern):
    c = S.seam_case(name, size, pattern, "constant")
    off = np.asarray([10.0, -7.0, 0.0])
    num, den = S.host_gather(c)
    d, known = U.seam_offsets(num, den, c["group_faces"], S.RefBackend())
    assert known.any() and np.array_equal(d[known], np.tile(off, (int(known.sum()), 1)))       # integer ratios
    assert np.abs(d - off).max() <= 1e-8
    image = S.host_apply(c, d)
    covered = c["face_id"] >= 0
    assert np.array_equal(image[covered], c["proj"][covered])              # v = an integer +- 1e-8: no tie
    assert (c["fallback"][covered & (c["source"] == 0)] != c["proj"][covered & (c["source"] == 0)]).any()


# ------------------------------------------------------------------ 3. the maximum principle
def test_offsets_obey_the_maximum_principle():
    c = S.atlas("icosphere", 64)
    G = c["n_groups"]
    # the welded icosphere, plus a component of its own that nothing known touches
    gf = np.concatenate([c["group_faces"], [[G, G + 1, G + 2], [G, G + 2, G + 3]]], 0)
    centre = np.zeros((G, 3))
    np.add.at(centre, c["group"], c["verts"][c["vmapping"]].astype(np.float64))
    centre /= np.bincount(c["group"], minlength=G)[:, None]
    rng = np.random.default_rng(5)
    for trial in range(3):
        # known regions: caps about three random directions, one random offset per region
        den = np.zeros(G + 4, np.int64)
        num = np.zeros((G + 4, 3), np.int64)
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for _ in range(3):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            cap = (centre @ axis > 0.35) & (den[:G] == 0)
            assert cap.sum() >= 3
            off = rng.integers(-60, 61, 3)
            weight = rng.integers(S.ONE, 50 * S.ONE, int(cap.sum()))
            den[:G][cap] = weight
            num[:G][cap] = weight[:, None] * off
            lo, hi = np.minimum(lo, off), np.maximum(hi, off)
        sliver = np.flatnonzero(den[:G] == 0)[::4]
        den[sliver], num[sliver] = S.ONE - 1, 255 * (S.ONE - 1)           # slivers: unknown whatever they hold
        d, known = U.seam_offsets(num, den, gf, S.RefBackend())
        want, known_ref = S.offsets(num, den, gf)
        assert np.array_equal(known, known_ref) and not known[sliver].any() and (~known[:G]).sum() >= 20
        assert np.abs(d - want).max() <= 1e-9
        assert (d[:G] >= lo - 1e-8).all() and (d[:G] <= hi + 1e-8).all()
        assert not d[G:].any() and np.array_equal(d[G:], np.zeros((4, 3)))  # no known group: exactly 0
        inner = d[:G][~known[:G]]
        assert np.ptp(inner, 0).min() > 1.0                                 # a solve, not a constant


# ------------------------------------------------------------------ 4. projected texels, and "none"
def _sphere_projection():
    v, f = F.icosphere()
    # another frame than the field's; radius 0.5 against the masks' disc of 0.45: a rim is left to the fallback
    frame = np.stack([v[:, 0], v[:, 2], -v[:, 1]], -1)
    cf, cb = P.drawings()
    return v, f, frame, cf, cb, S.RefBackend(P.disc_masks())


def test_projected_texels_are_untouched_and_none_is_the_old_composition():
    v, f, frame, cf, cb, be = _sphere_projection()
    col = np.full((len(v), 3), 0.5, np.float32)
    vm, ind, uvs = U.parametrize(v, f, 64, 2, backend=be)
    groups, gf = U.seam_groups(v, f, vm)
    field = U.bake_field(uvs, ind, v[vm], F.stripes, col[vm], 64, 0, samples=2, backend=be)
    for fallback_image in (None, field):
        kw = dict(backend=be, fallback_image=fallback_image)
        old, fid, src = U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 0, return_maps=True, **kw)
        none = U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 0, seam="none", **kw)
        assert np.array_equal(none, old)
        assert np.array_equal(U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 2, seam="none", **kw),
                              U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 2, **kw))
        level = U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 0, seam="level", groups=groups,
                                group_faces=gf, **kw)
        on = src > 0
        assert on.sum() > 100 and ((fid >= 0) & ~on).sum() > 100
        assert np.array_equal(level[on], old[on]) and not level[fid < 0].any()
        assert (level[(fid >= 0) & ~on] != old[(fid >= 0) & ~on]).any()
        # the gutter fill runs over the levelled composition
        filled = U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 2, seam="level", groups=groups,
                                 group_faces=gf, **kw)
        assert np.array_equal(filled, R.dilate(level, fid >= 0, 2)[0]) and (filled != level).any()
    with pytest.raises(ValueError):
        U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 0, seam="level", backend=be)
    with pytest.raises(ValueError):
        U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 0, seam="feather", backend=be)


# ------------------------------------------------------------------ 5. what it is for
def test_levelling_removes_the_tone_step():
    """Icosphere at 64^2, source pattern "z", drawing = a smooth function of the surface point,
    fallback = rint(0.8 drawing + 10).  Seam step measured on the restatement: 15.66 levels before,
    2.88 after (112 texel pairs inside one chart, one projected and one not).  At 37^2: 15.54 before,
    6.99 after.  What is left is the drawing's own slope across one texel plus the slope the factor
    0.8 takes away, which no offset that is one number per vertex can restore."""
    c, r = S.seam_case("icosphere", 64, "z", "tone"), S.restated("icosphere", 64, "z", "tone")
    src, fid, chart = c["source"], c["face_id"], c["face_chart"]
    hard = np.where((src > 0)[..., None], c["proj"], c["fallback"])
    before, pairs = S.seam_step(hard, src, fid, chart)
    ref_after = S.seam_step(r["image"], src, fid, chart)[0]
    print("pairs", pairs, "before", before, "after (restatement)", ref_after)
    assert pairs >= 100
    assert before == pytest.approx(STEP_BEFORE, abs=1e-9) and ref_after == pytest.approx(STEP_AFTER, abs=1e-9)
    num, den = S.host_gather(c)
    d, _ = U.seam_offsets(num, den, c["group_faces"], S.RefBackend())
    after = S.seam_step(S.host_apply(c, d), src, fid, chart)[0]
    print("after (host entries)", after)
    assert after <= 2.0 * STEP_AFTER and after < before
    # a plain cross-fade of the two sources would leave the drawing texels changed; they are not
    assert np.array_equal(S.host_apply(c, d)[src > 0], c["proj"][src > 0])


@pytest.mark.parametrize("name,size,pattern,colours", S.LEVEL_CASES)
def test_bake_drawings_level_is_the_three_steps_and_few_texels_are_fragile(name, size, pattern, colours):
    """The cases the device's bake_drawings is compared on (tests/test_gpu_uv_seam.py): through the numpy
    backend the call is gather, offsets, apply and the gutter fill; and the restatement alone keeps its
    fragile texels (v + 0.5 within 1e-6 of an integer) under the cap, none for the constant offset."""
    c, r = S.seam_case(name, size, pattern, colours), S.restated(name, size, pattern, colours)
    be = S.RefBackend()
    got = S.bake_level(c, be)
    assert np.array_equal(got, r["image"]) and np.array_equal(be.seam_fragile, r["fragile"])
    assert np.array_equal(S.bake_level(c, S.RefBackend(), gutter=2), R.dilate(r["image"], c["face_id"] >= 0, 2)[0])
    levelled, fragile = int(r["levelled"].sum()), int(r["fragile"].sum())
    print(name, size, pattern, colours, "levelled", levelled, "fragile", fragile)
    assert levelled >= 30 and fragile <= S.FRAGILE_CAP * levelled
    if colours == "constant":
        assert fragile == 0


# ------------------------------------------------------------------ 6. uv_mapping
def test_uv_mapping_levels_with_one_offset_per_welded_vertex():
    v, f, frame, cf, cb, be = _sphere_projection()
    col = np.full((len(v), 3), 0.5, np.float32)
    pr = {"positions": frame, "color_front": cf, "mask_front": None, "color_back": cb}
    plain = U.uv_mapping(v, f, col, "s", size=64, backend=be, projection=pr)
    assert np.array_equal(U.uv_mapping(v, f, col, "s", size=64, backend=be, projection=dict(pr, seam="none"))["image"],
                          plain["image"])
    got = U.uv_mapping(v, f, col, "s", size=64, backend=be, projection=dict(pr, seam="level"))
    for k in ("verts", "faces", "uvs"):
        assert np.array_equal(got[k], plain[k])
    vm, ind, uvs = U.parametrize(v, f, 64, 2, backend=be)
    groups, gf = U.seam_groups(v, f, vm)
    want, fid, src = U.bake_drawings(uvs, ind, frame[vm], cf, None, cb, col[vm], 64, 2, backend=be, seam="level",
                                     groups=groups, group_faces=gf, return_maps=True)
    assert np.array_equal(got["image"], want) and not np.array_equal(want, plain["image"])
    # the chart copies of one vertex are one unknown: one d, so no step of the offset across a chart border
    assert len(vm) > len(v) and groups.max() + 1 == len(v)
    for old in np.flatnonzero(np.bincount(vm) > 1)[:40]:
        assert len(np.unique(groups[vm == old])) == 1
    assert np.array_equal(groups, vm)                                      # no coincident vertices here: the vertex itself
    assert np.array_equal(gf, f)
    # coincident vertices are welded too
    v2 = np.concatenate([v, v[:5]], 0)
    f2 = np.array(f)
    f2[f2 < 5] += len(v)                                                   # every face now uses the copies
    f2[0] = f[0]                                                           # but one
    vm2, _, _ = U.parametrize(v2, f2, 64, 2, backend=be)
    g2, gf2 = U.seam_groups(v2, f2, vm2)
    assert g2.max() + 1 == len(v) and len(gf2) == len(f)


# ------------------------------------------------------------------ 7. switches
def test_save_obj_refuses_levelling_without_the_drawings(tmp_path):
    from drawingspinup_amd.nsr import mesh as M
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    f, c = torch.tensor([[0, 1, 2]]), torch.full((3, 3), 0.5)
    for kw in (dict(), dict(texture_source="vertex"), dict(texture_source="field", export_uv=True, texture_field=lambda p: p)):
        with pytest.raises(ValueError):
            M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_seam="level", **kw)
    with pytest.raises(ValueError):
        M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_seam="feather")
    assert os.listdir(tmp_path) == []
    M.save_obj(str(tmp_path / "a.obj"), v, f, c, texture_seam="none")
    M.save_obj(str(tmp_path / "b.obj"), v, f, c)
    assert open(tmp_path / "a.obj", "rb").read() == open(tmp_path / "b.obj", "rb").read()


def test_recon_reads_the_seam_switch_without_a_default_key():
    from drawingspinup_amd.entry import recon
    _, conf = recon.parse(["--uid", "u"])
    assert "texture_seam" not in conf["export"]
    _, conf = recon.parse(["--uid", "u", "--texture_source", "drawings", "--texture_seam", "level",
                           "export.export_uv=true"])
    assert conf["export"]["texture_seam"] == "level" and conf["export"]["texture_source"] == "drawings"
    _, conf = recon.parse(["--uid", "u", "export.texture_source=drawings", "export.texture_seam=level",
                           "export.export_uv=true"])
    assert conf["export"]["texture_seam"] == "level"
    _, conf = recon.parse(["--uid", "u", "--texture_seam", "none"])
    assert conf["export"]["texture_seam"] == "none"
    for argv in (["--texture_seam", "level"], ["export.texture_seam=level"], ["--texture_seam", "feather"],
                 ["export.texture_seam=feather"], ["--texture_seam", "level", "--texture_source", "vertex"],
                 ["--texture_seam", "level", "--texture_source", "field", "export.export_uv=true"]):
        with pytest.raises(SystemExit):
            recon.parse(["--uid", "u"] + argv)


# ------------------------------------------------------------------ 8. the exports
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dsu_hip.h")).read()
    lib = _lib.lib()
    for name in ("dsu_uv_seam_gather", "dsu_uv_seam_apply", "dsu_uv_seam_gather_host", "dsu_uv_seam_apply_host"):
        assert f"int {name}(" in header and callable(getattr(lib, name))
