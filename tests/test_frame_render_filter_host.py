"""CPU: the pixel filter of the frame rasteriser — the tap tables of animate.pixel_filter, the host
entry dsu_pixel_filter_resolve_host (the text the kernel compiles, csrc/film_filter.h) bit for bit
against the float64 restatement (tests/frame_render_filter_ref.py), and every refusal of the two new
entry points.  No GPU: the device entry is only taken as far as its argument checks."""
import ctypes
import math

import numpy as np
import pytest

import frame_render_filter_ref as FR
from drawingspinup_amd import animate

P = ctypes.c_void_p


def _ptr(a):
    return None if a is None else P(a.ctypes.data)


# ------------------------------------------------------------------ 1. taps
@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("width", [1.0, 1.5, 3.0])
def test_taps_follow_the_formula(ss, width):
    taps, halo = animate.pixel_filter("blackman_harris", width, ss)
    assert halo == max(math.ceil((width / 2 - 0.5) * ss), 0) and 0 <= halo <= 2 * ss
    assert taps.dtype == np.float64 and taps.shape == (ss + 2 * halo,)
    assert np.array_equal(taps, taps[::-1])                               # symmetric, bit for bit
    assert (taps >= 0).all() and taps[halo:halo + ss].sum() > 0
    for q in range(-halo, ss + halo):
        d = (q + 0.5) / ss - 0.5
        u = d / width + 0.5
        k = 0.35875 - 0.48829 * math.cos(2 * math.pi * u) + 0.14128 * math.cos(4 * math.pi * u) \
            - 0.01168 * math.cos(6 * math.pi * u)
        assert taps[q + halo] == pytest.approx(k if abs(d) < width / 2 else 0.0, abs=1e-15)


def test_window_values_and_presets():
    from drawingspinup_amd.animate.render import _blackman_harris
    for width in (1.0, 1.5, 3.0):
        assert _blackman_harris(0.0, width) == pytest.approx(1.0, abs=1e-15)
        for d in (-width / 2, width / 2):                                   # the coefficients' alternating sum
            assert _blackman_harris(d, width) == pytest.approx(6e-5, abs=1e-15)
    # ss 1 at width 1.5: the neighbours lie at |d| = 1 >= 0.75, only the pixel's own sample counts
    taps, halo = animate.pixel_filter("blackman_harris", 1.5, 1)
    assert halo == 1 and taps.tolist() == [0.0, taps[1], 0.0] and taps[1] == pytest.approx(1.0, abs=1e-15)
    taps, halo = animate.pixel_filter("box", None, 4)
    assert halo == 0 and taps.tolist() == [1.0] * 4
    for name, width in (("cycles", 1.5), ("eevee", 3.0)):
        assert animate.PIXEL_FILTER_PRESETS[name] == ("blackman_harris", width)
        for ss in (1, 2, 4):
            a, b = animate.pixel_filter(name, None, ss), animate.pixel_filter("blackman_harris", width, ss)
            assert a[1] == b[1] and np.array_equal(a[0], b[0])
    a = animate.pixel_filter("eevee", 2.0, 4)                               # a width overrides the preset's
    assert a[1] == 2 and np.array_equal(a[0], animate.pixel_filter("blackman_harris", 2.0, 4)[0])


def test_taps_refusals():
    for ss in (1, 2, 4):
        assert animate.pixel_filter("blackman_harris", 5.0, ss)[1] == 2 * ss     # the widest that fits
        with pytest.raises(ValueError, match="beyond the pixel"):
            animate.pixel_filter("blackman_harris", 5.0 + 2.0 / ss + 0.01, ss)
    for bad in (None, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            animate.pixel_filter("blackman_harris", bad, 4)
    with pytest.raises(ValueError):
        animate.pixel_filter("gaussian", 1.5, 4)
    with pytest.raises(ValueError):
        animate.pixel_filter("eevee", None, 3)


# ------------------------------------------------------------------ 2. the host entry
def _host(colour, pos, covered, taps, halo, ss, want=("pixels", "color_u8", "pos_u8")):
    from drawingspinup_amd import _lib
    F, N = covered.shape[:2]
    S = N // ss
    colour, pos = np.ascontiguousarray(colour, np.float32), np.ascontiguousarray(pos, np.float32)
    cov = np.ascontiguousarray(covered, np.uint8)
    taps = np.ascontiguousarray(taps, np.float64)
    out = {"pixels": np.full((F, S, S, 8), 7.0, np.float32), "color_u8": np.full((F, S, S, 4), 7, np.uint8),
           "pos_u8": np.full((F, S, S, 4), 7, np.uint8)}
    rc = _lib.lib().dsu_pixel_filter_resolve_host(_ptr(colour), _ptr(pos), _ptr(cov), F, S, ss, _ptr(taps), halo,
                                                  *[_ptr(out[k]) if k in want else None for k in out])
    assert rc == 0
    return {k: out[k] for k in want}


def _same(got, attr, covered, taps, halo, ss):
    """Bit-equal to the restatement: pixels as its float64 values rounded to f32, NaNs in the same places."""
    ref = FR.resolve(attr, covered, taps, halo, ss)
    with np.errstate(invalid="ignore"):
        want = ref["pixels"].astype(np.float32)
    assert np.array_equal(got["pixels"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["color_u8"], ref["color_u8"]) and np.array_equal(got["pos_u8"], ref["pos_u8"])
    return ref


def _random_field(F, N, seed, cover=0.6):
    g = np.random.default_rng(seed)
    colour, pos = g.random((F, N, N, 3)).astype(np.float32), g.random((F, N, N, 3)).astype(np.float32)
    # a blob with holes and specks in the upper rows, so that pixels are empty, partial and full
    yy, xx = np.mgrid[:N, :N]
    covered = np.stack([((yy - N * g.uniform(0.3, 0.7)) ** 2 + (xx - N * g.uniform(0.3, 0.7)) ** 2 < (cover * N / 2) ** 2)
                        ^ ((g.random((N, N)) < 0.05) & (yy < 0.4 * N)) for _ in range(F)])
    return colour, pos, covered


@pytest.mark.parametrize("width", [1.5, 3.0])
@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("size", [20, 36])
def test_host_entry_equals_the_restatement_on_random_fields(size, ss, width):
    taps, halo = animate.pixel_filter("blackman_harris", width, ss)
    colour, pos, covered = _random_field(2, size * ss, 100 * size + 10 * ss + int(width))
    got = _host(colour, pos, covered, taps, halo, ss)
    ref = _same(got, np.concatenate([colour, pos], -1), covered, taps, halo, ss)
    a = ref["pixels"][..., 3]
    assert (a == 0).any() and (a == 1).any()
    assert ((a > 0) & (a < 1)).any() or (ss == 1 and width == 1.5)          # that one is the box over one sample
    # a single optional output
    only = _host(colour, pos, covered, taps, halo, ss, want=("color_u8",))
    assert np.array_equal(only["color_u8"], got["color_u8"])


@pytest.mark.parametrize("ss", [1, 2, 4])
def test_host_entry_edge_rows(ss):
    S = 20
    N = S * ss
    taps, halo = animate.pixel_filter("eevee", None, ss)
    colour, pos, _ = _random_field(1, N, 5 + ss)
    attr = np.concatenate([colour, pos], -1)
    # nothing covered
    none = np.zeros((1, N, N), bool)
    got = _host(colour, pos, none, taps, halo, ss)
    _same(got, attr, none, taps, halo, ss)
    assert not got["pixels"].any() and not got["color_u8"].any() and not got["pos_u8"].any()
    # everything covered: alpha exactly 1 in every pixel, the border included, and the colour a mean
    full = np.ones((1, N, N), bool)
    got = _host(colour, pos, full, taps, halo, ss)
    _same(got, attr, full, taps, halo, ss)
    assert (got["pixels"][..., 3] == 1.0).all() and (got["color_u8"][..., 3] == 255).all()
    const = np.broadcast_to(np.float32([0.25, 0.5, 0.75]), colour.shape)
    flat = _host(const, const, full, taps, halo, ss)
    assert np.abs(flat["pixels"][..., :3].astype(np.float64) - [0.25, 0.5, 0.75]).max() <= 2.0 ** -24
    assert (flat["color_u8"][..., :3] == [64, 128, 191]).all()
    # one covered sample in a corner: it reaches the pixels within hp of the corner and no others
    one = np.zeros((1, N, N), bool)
    one[0, N - 1, 0] = True
    got = _host(colour, pos, one, taps, halo, ss)
    _same(got, attr, one, taps, halo, ss)
    hp = -(-halo // ss)
    seen = got["pixels"][0, :, :, 3] > 0
    assert seen[S - 1, 0] and seen.sum() > 1 and not seen[:S - 1 - hp].any() and not seen[:, hp + 1:].any()
    assert np.abs(got["pixels"][0][seen][:, :3] - colour[0, N - 1, 0]).max() <= 2.0 ** -23    # (w v) / w of one sample
    # a NaN attribute: it spreads to the pixels that reach it, as NaN in pixels and 0 in uint8
    bad = colour.copy()
    bad[0, N // 2, N // 2, 1] = np.nan
    got = _host(bad, pos, full, taps, halo, ss)
    _same(got, np.concatenate([bad, pos], -1), full, taps, halo, ss)
    nan = np.isnan(got["pixels"][0, :, :, 1])
    assert nan[N // 2 // ss, N // 2 // ss] and 1 <= nan.sum() <= (2 * hp + 1) ** 2
    assert (got["color_u8"][0][nan][:, 1] == 0).all() and not np.isnan(got["pixels"][..., [0, 2, 3, 4, 5, 6, 7]]).any()


@pytest.mark.parametrize("ss", [1, 2, 4])
def test_ones_without_a_halo_are_the_plain_mean(ss):
    S = 20
    N = S * ss
    colour, pos, covered = _random_field(2, N, 40 + ss)
    got = _host(colour, pos, covered, np.ones(ss), 0, ss)
    attr = np.concatenate([colour, pos], -1).astype(np.float64)
    acc, cnt = np.zeros((2, S, S, 6)), np.zeros((2, S, S))
    for sy in range(ss):                                                    # the unfiltered rule, its order
        for sx in range(ss):
            cv = covered[:, sy::ss, sx::ss]
            acc += np.where(cv[..., None], attr[:, sy::ss, sx::ss], 0.0)
            cnt += cv
    v = np.where(cnt[..., None] > 0, acc / np.maximum(cnt, 1)[..., None], 0.0)
    alpha = cnt / float(ss * ss)
    pixels = np.concatenate([v[..., :3], alpha[..., None], v[..., 3:], alpha[..., None]], -1)
    assert np.array_equal(got["pixels"], pixels.astype(np.float32))
    q = np.floor(pixels * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(got["color_u8"], q[..., :4]) and np.array_equal(got["pos_u8"], q[..., 4:])


# ------------------------------------------------------------------ 3. refusals
def test_host_entry_refusals():
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    S, ss = 8, 2
    N = S * ss
    col, pos = np.zeros((1, N, N, 3), np.float32), np.zeros((1, N, N, 3), np.float32)
    cov = np.zeros((1, N, N), np.uint8)
    pix = np.zeros((1, S, S, 8), np.float32)
    taps, halo = animate.pixel_filter("eevee", None, ss)

    def call(colour=col, pos=pos, covered=cov, F=1, S=S, ss=ss, taps=taps, halo=halo):
        return lib.dsu_pixel_filter_resolve_host(_ptr(colour), _ptr(pos), _ptr(covered), F, S, ss, _ptr(taps), halo,
                                                 _ptr(pix), None, None)

    assert call() == 0
    assert call(colour=None) == -1 and call(pos=None) == -1 and call(covered=None) == -1
    assert call(F=0) == -1 and call(S=0) == -1 and call(S=18) == -1 and call(S=2052) == -1 and call(ss=3) == -1
    _taps_refusals(call, taps, halo, ss)


def _taps_refusals(call, taps, halo, ss):
    """What both entry points refuse of (taps, halo); call(taps=, halo=) returns the status."""
    assert call(taps=None) == -1
    assert call(halo=-1) == -1 and call(halo=2 * ss + 1) == -1
    long = np.ones(ss + 2 * (2 * ss + 1))
    assert call(taps=long, halo=2 * ss + 1) == -1
    for bad in (-1e-300, -1.0, float("nan"), float("inf"), -float("inf")):
        for at in (0, halo, len(taps) - 1):
            t = taps.copy()
            t[at] = bad
            assert call(taps=t) == -1, (bad, at)
    t = taps.copy()
    t[halo:halo + ss] = 0.0                                                 # the pixel's own samples weigh nothing
    assert call(taps=t) == -1
    t = np.zeros_like(taps)
    t[halo] = 1e-300                                                        # any positive centre will do
    assert call(taps=t) != -1


def _device_entry(flt):
    """dsu_mesh_render_ortho_filtered with host memory standing in for every device pointer, as
    test_frame_render_host.render_entry_refusals has it for the unfiltered entry: no call may get as far
    as a launch with faces."""
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(4096, np.int32)
    ws, fake = P(buf.ctypes.data), P(buf.ctypes.data)
    box = np.ones(4)

    def call(stage=0, screen=fake, faces=fake, colour=fake if flt is None else None, pos=fake, uv=fake,
             texels=fake, T=8, flt=flt, F=1, V=3, M=1, span=1.35, S=16, ss=4, taps=box, halo=0, workspace=ws,
             wbytes=4096 * 4, items=fake, n_items=1):
        tex = None if flt is None else ctypes.byref(_lib.RenderTexture(uv, texels, T, flt))
        return lib.dsu_mesh_render_ortho_filtered(stage, screen, faces, colour, pos, tex, F, V, M, 0.0, 0.0, span, S,
                                                  ss, _ptr(taps), halo, workspace, wbytes, items, n_items, None,
                                                  None, None, None, None, None, None)
    return call, buf


@pytest.mark.parametrize("flt", [None, 0, 1, 2])
def test_device_entry_mirrors_the_refusals_of_the_unfiltered_entry(flt):
    call, buf = _device_entry(flt)
    for stage in (0, 2):
        assert call(stage, ss=3) == -1
        assert call(stage, S=18) == -1 and call(stage, S=0) == -1 and call(stage, S=2052) == -1
        assert call(stage, workspace=None) == -1 and call(stage, wbytes=8) == -1
        assert call(stage, screen=None) == -1 and call(stage, faces=None) == -1
        assert call(stage, span=0.0) == -1 and call(stage, span=float("nan")) == -1
        assert call(stage, F=0) == -1 and call(stage, M=-1) == -1
    assert call(stage=1, items=None) == -1 and call(stage=3) == -1 and call(stage=-1) == -1
    assert call(stage=2, pos=None) == -1 and call(stage=2, items=None) == -1
    if flt is None:
        assert call(stage=2, colour=None) == -1
    else:
        assert call(stage=2, uv=None) == -1 and call(stage=2, texels=None) == -1
        assert call(stage=2, T=0) == -1 and call(stage=2, T=8193) == -1 and call(stage=2, T=-4) == -1
        assert call(stage=2, flt=3) == -1 and call(stage=2, flt=-1) == -1
        assert call(stage=2, texels=P(buf.ctypes.data + 2)) == -1
    assert not buf.any()


def test_device_entry_refuses_bad_taps_before_any_launch():
    call, buf = _device_entry(None)
    taps, halo = animate.pixel_filter("eevee", None, 4)
    # with faces: every refusal must come before the launch (the pointers are host memory)
    raster = lambda **kw: call(stage=2, **{"taps": taps, "halo": halo, **kw})
    assert raster(taps=None) == -1
    assert raster(halo=-1) == -1 and raster(halo=9) == -1
    for bad in (-1.0, float("nan"), float("inf")):
        t = taps.copy()
        t[3] = bad
        assert raster(taps=t) == -1
    t = taps.copy()
    t[halo:halo + 4] = 0.0
    assert raster(taps=t) == -1
    # halo is read at every stage, taps at RASTER only
    for stage in (0, 1):
        assert call(stage, halo=-1) == -1 and call(stage, halo=9) == -1
        assert call(stage, M=0, halo=8, taps=None) == call(stage, M=0, halo=8, taps=np.ones(20))
    assert not buf.any()


def test_python_layers_refuse_mismatched_arguments():
    from drawingspinup_amd.animate.render import _pixel_filter_args
    assert _pixel_filter_args(None, None, 4) == {}
    with pytest.raises(ValueError, match="filter_width goes with"):
        _pixel_filter_args(None, 1.5, 4)
    taps, halo = _pixel_filter_args("cycles", None, 2)["pixel_filter"]
    assert halo == 1 and len(taps) == 4
    from drawingspinup_amd.entry import run_render
    with pytest.raises(SystemExit):
        run_render.run(["--pixel_filter", "blackman_harris"])                # no width
    with pytest.raises(SystemExit):
        run_render.run(["--filter_width", "1.5"])                            # no filter
    with pytest.raises(SystemExit):
        run_render.run(["--pixel_filter", "gaussian"])
