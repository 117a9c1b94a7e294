"""Mip-mapped frames without a GPU: the level layout, the restated pyramid on hand-checked cases, the
sampling arithmetic the kernel compiles (csrc/mip_sample.h through dsu_mip_sample_host) against the
numpy restatement bit for bit, and the argument checks of the new entry points and keywords."""
import ctypes

import numpy as np
import pytest

import frame_render_mip_ref as MR
import frame_render_tex_ref as TR
from drawingspinup_amd import animate

P = ctypes.c_void_p


def _lib():
    from drawingspinup_amd import _lib
    return _lib.lib()


def _ptr(a):
    return P(a.ctypes.data)


def _host_sample(flat, T, tx, ty, rho):
    flat = np.ascontiguousarray(flat, np.uint8)
    tx, ty, rho = (np.ascontiguousarray(a, np.float64) for a in (tx, ty, rho))
    out = np.full((len(tx), 3), -1.0, np.float32)
    assert _lib().dsu_mip_sample_host(_ptr(flat), T, _ptr(tx), _ptr(ty), _ptr(rho), len(tx), _ptr(out)) == 0
    return out


# ------------------------------------------------------------------ layout
@pytest.mark.parametrize("T,sizes", [(1, [1]), (2, [2, 1]), (5, [5, 3, 2, 1]), (37, [37, 19, 10, 5, 3, 2, 1]),
                                     (64, [64, 32, 16, 8, 4, 2, 1])])
def test_level_sizes_and_offsets(T, sizes):
    lib = _lib()
    assert MR.level_sizes(T) == sizes
    offsets = MR.level_offsets(T)
    assert offsets[0] == 0 and all(offsets[k + 1] - offsets[k] == s * s for k, s in enumerate(sizes))
    assert lib.dsu_mip_levels(T) == len(sizes)
    assert lib.dsu_mip_pyramid_texels(T) == offsets[-1] == sum(s * s for s in sizes)
    t1, t2 = (T + 1) // 2, (T + 3) // 4
    assert lib.dsu_mip_workspace_bytes(T) == (32 * (t1 * t1 + t2 * t2) + 4 * t1 * t1 if T > 1 else 0)
    levels = MR.pyramid(np.zeros((T, T, 4), np.uint8))
    assert [lv.shape for lv in levels] == [(s, s, 4) for s in sizes]
    assert MR.flatten(levels).shape == (offsets[-1], 4)


def test_layout_entries_refuse_bad_sizes():
    lib = _lib()
    for T in (0, -3, 8193):
        assert lib.dsu_mip_levels(T) == -1 and lib.dsu_mip_pyramid_texels(T) == -1
        assert lib.dsu_mip_workspace_bytes(T) == -1
    assert lib.dsu_mip_levels(8192) == 14 and lib.dsu_mip_pyramid_texels(8192) == sum(4 ** k for k in range(14))


# ------------------------------------------------------------------ the restated pyramid by hand
def _rgba(rgb):
    rgb = np.asarray(rgb, np.uint8)
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], -1)


def test_two_by_two_to_one_by_covered_count():
    img = _rgba([[[10, 0, 255], [11, 0, 255]], [[13, 1, 254], [20, 2, 255]]])
    cases = {0: ([], [0, 0, 0, 0]),
             1: ([(1, 0)], [13, 1, 254, 255]),
             3: ([(0, 0), (0, 1), (1, 1)], [14, 1, 255, 255]),       # 41 / 3 = 13.67, 2 / 3, 255
             4: ([(0, 0), (0, 1), (1, 0), (1, 1)], [14, 1, 255, 255])}   # 54 / 4 = 13.5 -> 14 (half up), 0.75, 254.75
    for n, (where, want) in cases.items():
        cov = np.zeros((2, 2), bool)
        for rc in where:
            cov[rc] = True
        for gutter in (0, 2):
            levels = MR.pyramid(img, cov, gutter)
            assert len(levels) == 2 and np.array_equal(levels[0], img)
            assert levels[1].reshape(4).tolist() == want, (n, gutter)
    # no mask = all covered
    assert np.array_equal(MR.pyramid(img)[1], MR.pyramid(img, np.ones((2, 2), bool))[1])


@pytest.mark.parametrize("T", [8, 37])
def test_checkerboard_of_one_texel_squares_is_128_above_level_0(T):
    yy, xx = np.mgrid[:T, :T]
    img = _rgba(np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, -1))
    levels = MR.pyramid(img)
    if T == 8:
        # every block holds as many 0 as 255: 127.5 -> 128
        for lv in levels[1:]:
            assert (lv[..., :3] == 128).all() and (lv[..., 3] == 255).all()
    else:
        # odd sizes: a clipped block may hold one texel more of either kind
        for k, lv in enumerate(levels[1:], 1):
            inner = lv[:T // (1 << k), :T // (1 << k), :3]
            assert (inner == 128).all()


def test_a_single_covered_texel_survives_to_the_top():
    T = 37
    img = _rgba(np.random.default_rng(0).integers(0, 256, (T, T, 3)))
    cov = np.zeros((T, T), bool)
    cov[29, 6] = True
    levels = MR.pyramid(img, cov, gutter=0)
    for k, lv in enumerate(levels[1:], 1):
        has = lv[..., 3] == 255
        assert has.sum() == 1 and has[29 >> k, 6 >> k]
        assert np.array_equal(lv[29 >> k, 6 >> k, :3], img[29, 6, :3])
        assert (lv[~has] == 0).all()
    assert np.array_equal(levels[-1][0, 0, :3], img[29, 6, :3])
    # with the gutter the value spreads, unchanged (the mean of one value), and level 0 stays
    spread = MR.pyramid(img, cov, gutter=2)
    assert np.array_equal(spread[0], img)
    for lv in spread[1:]:
        has = lv[..., 3] == 255
        assert has.sum() > 1 or lv.shape[0] == 1
        assert (lv[has][:, :3] == img[29, 6, :3]).all()


# ------------------------------------------------------------------ the compiled sampling against the restatement
def _sampling_cases(T, n, seed):
    """(tx, ty, rho): random draws and the edges of every rule."""
    rng = np.random.default_rng(seed)
    L = len(MR.level_sizes(T))
    tx = rng.uniform(-2.0, T + 2.0, n)
    ty = rng.uniform(-2.0, T + 2.0, n)
    rho = 2.0 ** rng.uniform(-2.0, L + 1.0, n)
    pw = 2.0 ** rng.integers(0, L + 2, n).astype(np.float64)
    kind = rng.integers(0, 10, n)
    rho = np.where(kind == 0, rng.uniform(0.0, 1.0, n), rho)                  # rho <= 1
    rho = np.where(kind == 1, pw, rho)                                        # exactly 2^k
    rho = np.where(kind == 2, np.nextafter(2.0 * pw, 0.0), rho)               # just under 2^(k+1)
    rho = np.where(kind == 3, 2.0 ** L * rng.uniform(1.0, 1e6, n), rho)       # above 2^L
    special = np.array([np.nan, np.inf, -np.inf, 1e306, -1e306, 0.0, -0.0, 1.0, 0.5, T - 1.0, T - 0.5])
    tx = np.where(kind == 4, rng.choice(special, n), tx)
    ty = np.where(kind == 5, rng.choice(special, n), ty)
    rho = np.where(kind == 6, rng.choice(np.array([np.nan, np.inf, -np.inf, 1e306, -4.0, 0.0, 1.0,
                                                   np.nextafter(1.0, 2.0)]), n), rho)
    tx = np.where(kind == 7, np.round(tx), tx)                                # texel centres
    ty = np.where(kind == 7, np.round(ty) + 0.5, ty)                          # and half-way points
    return tx, ty, rho


@pytest.mark.parametrize("T,n", [(1, 10000), (2, 10000), (5, 10000), (37, 50000), (64, 20000)])
def test_compiled_sampling_equals_the_restatement_bit_for_bit(T, n):
    rng = np.random.default_rng(100 + T)
    img = rng.integers(0, 256, (T, T, 4)).astype(np.uint8)
    cov = rng.random((T, T)) < 0.6 if T > 2 else None
    levels = MR.pyramid(img, cov)
    tx, ty, rho = _sampling_cases(T, n, T)
    k, t = MR.lod(rho, len(levels))
    assert T == 1 or (set(np.unique(k)) == set(range(len(levels))) and (t > 0.9).any() and (t == 0).any())
    assert ((t >= 0.0) & (t < 1.0)).all()
    got = _host_sample(MR.flatten(levels), T, tx, ty, rho)
    want = MR.sample_rho(levels, tx, ty, rho)
    assert np.isfinite(got).all()
    assert np.array_equal(got.astype(np.float64), want)
    # rho <= 1 (and every rho that is not a finite number above 1): the bilinear rule, bit for bit
    flat0 = ~(np.isfinite(rho) & (rho > 1.0))
    assert flat0.sum() > n // 20 and (k[flat0] == 0).all() and (t[flat0] == 0).all()
    ftx, fty = (np.where(np.isfinite(a), a, 0.0) for a in (tx, ty))
    bil = TR.sample(levels[0], ftx[flat0], fty[flat0], TR.BILINEAR)
    assert np.array_equal(got[flat0].astype(np.float64), bil)


def test_lod_by_hand():
    k, t = MR.lod(np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 3.999, 4.0, 64.0, 100.0, 1e300, np.nan, np.inf, -8.0]), 7)
    assert k.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 6, 6, 6, 0, 0, 0]
    assert np.allclose(t, [0, 0, 0, 0.5, 0, 0.5, 0.9995, 0, 0, 0, 0, 0, 0, 0], atol=1e-12)
    # the quad of the aliasing test: every number a power of two, rho = 2 exactly
    a, b, c = (np.array([p], np.float64) for p in ([-0.25, -0.25], [0.25, -0.25], [0.25, 0.25]))
    ta, tb, tc = (np.array([p], np.float64) for p in ([0.0, 0.0], [1.0, 0.0], [1.0, 1.0]))
    assert MR.footprint(a, b, c, ta, tb, tc, 64, 1.0 / 64).tolist() == [2.0]
    assert MR.footprint(a, b, c, ta, tb, tc, 8, 1.0 / 256).tolist() == [0.0625]
    assert MR.footprint(a, a, c, ta, tb, tc, 8, 1.0).tolist() == [0.0]          # no screen area


def test_top_level_and_constant_texture():
    T = 37
    img = np.broadcast_to(np.array([201, 7, 98, 255], np.uint8), (T, T, 4)).copy()
    levels = MR.pyramid(img)
    tx, ty, rho = _sampling_cases(T, 5000, 3)
    got = _host_sample(MR.flatten(levels), T, tx, ty, rho)
    want = (np.array([201, 7, 98], np.float64) / 255.0).astype(np.float32)
    # (1 - t) c + t c may differ from c by an ulp of float64: far below f32 rounding except on a tie
    assert np.abs(got - want).max() <= 2.0 ** -24


# ------------------------------------------------------------------ argument checks
def test_pyramid_build_validates_before_launching():
    lib = _lib()
    buf = np.zeros(1 << 16, np.int32)
    fake = P(buf.ctypes.data)

    def call(texture=fake, covered=None, T=8, gutter=2, pyramid=fake, workspace=fake, wbytes=1 << 18):
        return lib.dsu_mip_pyramid_build(texture, covered, T, gutter, pyramid, workspace, wbytes, None)

    assert call(T=0) == -1 and call(T=8193) == -1 and call(T=-1) == -1
    assert call(gutter=-1) == -1 and call(gutter=65) == -1
    assert call(texture=None) == -1 and call(pyramid=None) == -1
    assert call(texture=P(buf.ctypes.data + 2)) == -1 and call(pyramid=P(buf.ctypes.data + 1)) == -1
    assert call(workspace=None) == -1 and call(wbytes=int(lib.dsu_mip_workspace_bytes(8)) - 1) == -1
    assert call(workspace=P(buf.ctypes.data + 4)) == -1
    assert not buf.any()


def test_mip_entry_point_validates_before_launching():
    from test_frame_render_host import render_entry_refusals
    render_entry_refusals(2)                                # DSU_TEX_TRILINEAR
    lib = _lib()
    fake = P(np.zeros(16, np.int32).ctypes.data)
    assert lib.dsu_mip_sample_host(None, 8, None, None, None, 0, None) == -1
    assert lib.dsu_mip_sample_host(fake, 8, None, None, None, 1, None) == -1
    assert lib.dsu_mip_sample_host(fake, 8, None, None, None, 0, None) == 0


def test_keyword_errors():
    from drawingspinup_amd import ops
    assert ops.MIP_TRILINEAR == "trilinear" and ops.TEXTURE_FILTERS == {"nearest": 0, "bilinear": 1, "trilinear": 2}
    v = np.zeros((3, 3))
    tex = dict(texture=np.zeros((2, 2, 3), np.uint8), uvs=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="texture_filter"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", texture_filter="cubic", device="cpu", **tex)
    with pytest.raises(ValueError, match="together"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", texture_filter="trilinear", device="cpu")
    with pytest.raises(ValueError, match="together"):
        animate.render_frames(v, [[0, 1, 2]], np.zeros((3, 3)), "rest_pose", texture_filter="trilinear",
                              uvs=np.zeros((3, 2)), device="cpu")
    with pytest.raises(ValueError, match="mip_coverage"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", texture_filter="trilinear", mip_coverage="x",
                              device="cpu", **tex)


def test_run_render_keeps_refusing_unknown_choices(tmp_path):
    from drawingspinup_amd.entry import run_render
    for bad in (["--texture", "mipmap"], ["--texture_filter", "cubic"], ["--mip_coverage", "x"]):
        with pytest.raises(SystemExit):
            run_render.run(["--data_dir", str(tmp_path), "--uid", "uid0", *bad])
