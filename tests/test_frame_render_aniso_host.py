"""Anisotropic frames without a GPU: the text the kernel compiles (csrc/mip_sample.h through
dsu_aniso_sample_host) against the numpy restatement of the header's rule bit for bit, the three
properties the rule promises, the stripe case by hand, and every refusal of the new entry and keywords."""
import ctypes

import numpy as np
import pytest

import frame_render_aniso_ref as AR
import frame_render_mip_ref as MR
from drawingspinup_amd import animate

P = ctypes.c_void_p
CAPS = (1, 2, 8, 16)


def _lib():
    from drawingspinup_amd import _lib
    return _lib.lib()


def _ptr(a):
    return None if a is None else P(a.ctypes.data)


def _host(flat, T, tri, uv, h, tx, ty, cap):
    """dsu_aniso_sample_host -> rgb (n,3) f32, probes (n) i32, rho (n) f64, axis (n,2) f64."""
    flat = np.ascontiguousarray(flat, np.uint8)
    tri, tx, ty = (np.ascontiguousarray(a, np.float64) for a in (tri, tx, ty))
    uv = np.ascontiguousarray(uv, np.float32)
    n = len(tx)
    assert tri.shape == (n, 6) and uv.shape == (n, 6)
    rgb, probes = np.full((n, 3), -1.0, np.float32), np.full(n, -1, np.int32)
    rho, axis = np.full(n, -1.0), np.full((n, 2), -7.0)
    assert _lib().dsu_aniso_sample_host(_ptr(flat), T, _ptr(tri), _ptr(uv), float(h), _ptr(tx), _ptr(ty), cap, n,
                                        _ptr(rgb), _ptr(probes), _ptr(rho), _ptr(axis)) == 0
    return rgb, probes, rho, axis


def _host_trilinear(flat, T, tx, ty, rho):
    flat = np.ascontiguousarray(flat, np.uint8)
    tx, ty, rho = (np.ascontiguousarray(a, np.float64) for a in (tx, ty, rho))
    out = np.full((len(tx), 3), -1.0, np.float32)
    assert _lib().dsu_mip_sample_host(_ptr(flat), T, _ptr(tx), _ptr(ty), _ptr(rho), len(tx), _ptr(out)) == 0
    return out


def _restated(levels, tri, uv, h, tx, ty, cap):
    tri, uv = np.asarray(tri, np.float64), np.asarray(uv, np.float32).astype(np.float64)
    fp = AR.footprint(tri[:, 0:2], tri[:, 2:4], tri[:, 4:6], uv[:, 0:2], uv[:, 2:4], uv[:, 4:6],
                      levels[0].shape[0], h, cap, len(levels))
    return fp, AR.sample(levels, tx, ty, fp)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _unit_items(T, dpx, dpy, dqx, dqy):
    """Items on the triangle (0,0), (1,0), (0,1) (det = 1, so the Jacobian is the uv differences times T):
    tri (n,6) f64 and uv (n,6) f32 whose texel-per-unit Jacobian is ((dpx, dpy), (dqx, dqy)) up to the
    rounding of the uvs to f32 (none where the entries over T are dyadic)."""
    dpx, dpy, dqx, dqy = (np.asarray(a, np.float64) for a in np.broadcast_arrays(dpx, dpy, dqx, dqy))
    n = len(dpx)
    tri = np.tile(np.array([0.0, 0.0, 1.0, 0.0, 0.0, 1.0]), (n, 1))
    uv = np.zeros((n, 6), np.float32)
    uv[:, 2], uv[:, 3] = dpx / T, dqx / T
    uv[:, 4], uv[:, 5] = dpy / T, dqy / T
    return tri, uv


def _cases(T, n, seed):
    """(tri, uv, h, tx, ty): random footprints with ratios across 1..40 and the edges of every rule."""
    rng = np.random.default_rng(seed)
    L = len(MR.level_sizes(T))
    h = 1.0 / 64
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    a = f32(rng.uniform(-1.0, 1.0, (n, 2)))
    e1, e2 = rng.normal(0.0, 0.3, (n, 2)), rng.normal(0.0, 0.3, (n, 2))
    b, c = f32(a + e1), f32(a + e2)
    s1 = 2.0 ** rng.uniform(-2.0, L + 1.0, n)
    ratio = np.exp(rng.uniform(0.0, np.log(40.0), n))
    th, ph = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    rot = lambda t: np.stack([np.stack([np.cos(t), -np.sin(t)], -1), np.stack([np.sin(t), np.cos(t)], -1)], -2)
    sig = np.zeros((n, 2, 2))
    sig[:, 0, 0], sig[:, 1, 1] = s1, s1 / ratio
    J = rot(th) @ sig @ rot(ph) / (h * T)                     # uv per world unit
    ua = rng.uniform(0.1, 0.9, (n, 2))
    uv = np.concatenate([ua, ua + np.einsum("nij,nj->ni", J, b - a), ua + np.einsum("nij,nj->ni", J, c - a)], 1)
    tri = np.concatenate([a, b, c], 1)
    kind = rng.integers(0, 16, n)
    # det = 0: a repeated vertex, or three collinear ones on a dyadic line
    tri[kind == 0, 2:4] = tri[kind == 0, 0:2]
    sel = kind == 1
    tri[sel] = np.stack([0 * s1, 0 * s1, 0.25 + 0 * s1, 0.5 + 0 * s1, -0.5 + 0 * s1, -1.0 + 0 * s1], 1)[sel]
    # non-finite and huge vertices and uvs
    special = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30])
    sel = np.nonzero(kind == 2)[0]
    tri[sel, rng.integers(0, 6, len(sel))] = rng.choice(special, len(sel))
    sel = np.nonzero(kind == 3)[0]
    uv[sel, rng.integers(0, 6, len(sel))] = rng.choice(special, len(sel))
    uv = uv.astype(np.float32)
    # lattice-aligned maps on the unit triangle, h = 1 / 64 scaled out: s1 just below, at and above 1,
    # integer ratios from dyadic entries (ceil at its boundary), rank one (s2 = 0), equal scale
    one = np.float32(1.0)
    near = np.array([np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))], np.float64)
    g = 2.0 ** rng.integers(-2, 4, n).astype(np.float64)
    R = rng.integers(1, 21, n).astype(np.float64)
    sign = rng.choice([-1.0, 1.0], n)
    swap = rng.random(n) < 0.5
    for kd, (px, qy) in {4: (rng.choice(near, n) / h, 0.25 / h + 0 * g),
                         5: (sign * R * g / h, g / h),
                         6: (sign * g * 8.0 / h, 0 * g),
                         7: (sign * g / h, g / h)}.items():
        sel = kind == kd
        big, small = np.where(swap, qy, px), np.where(swap, px, qy)
        t_, u_ = _unit_items(T, big, 0.0 * g, 0.0 * g, small)
        tri[sel], uv[sel] = t_[sel], u_[sel]
    tx = rng.uniform(-2.0, T + 2.0, n)
    ty = rng.uniform(-2.0, T + 2.0, n)
    odd = np.array([np.nan, np.inf, -np.inf, 1e306, -1e306, 0.0, -0.0, 0.5, T - 1.0, T - 0.5])
    tx = np.where(kind == 8, rng.choice(odd, n), tx)
    ty = np.where(kind == 9, rng.choice(odd, n), ty)
    tx = np.where(kind == 10, np.round(tx), tx)
    ty = np.where(kind == 10, np.round(ty) + 0.5, ty)
    meta = {"kind": kind, "R": R, "g": g}
    return tri, uv, h, tx, ty, meta


@pytest.mark.parametrize("T", [1, 2, 5, 37, 64])
def test_compiled_rule_equals_the_restatement_bit_for_bit(T):
    """10^5 items in all: 5 sizes x 4 caps x 5000."""
    rng = np.random.default_rng(300 + T)
    img = rng.integers(0, 256, (T, T, 4)).astype(np.uint8)
    levels = MR.pyramid(img, rng.random((T, T)) < 0.6 if T > 2 else None)
    flat = MR.flatten(levels)
    for cap in CAPS:
        tri, uv, h, tx, ty, meta = _cases(T, 5000, 1000 * T + cap)
        fp, want = _restated(levels, tri, uv, h, tx, ty, cap)
        rgb, probes, rho, axis = _host(flat, T, tri, uv, h, tx, ty, cap)
        assert np.isfinite(rgb).all() and (rgb >= 0).all() and (rgb <= 1).all()
        assert np.array_equal(probes, fp["N"])
        assert np.array_equal(_bits(rho), _bits(fp["rho"]))
        assert np.array_equal(_bits(axis), _bits(np.stack([fp["ax"], fp["ay"]], 1)))
        assert np.array_equal(rgb.astype(np.float64), want)
        # the case list reaches what it is meant to reach
        N = fp["N"]
        assert ((N >= 1) & (N <= cap)).all() and set(np.unique(N)) == set(range(1, cap + 1))
        assert (np.abs(np.hypot(axis[:, 0], axis[:, 1]) - 1.0) <= 1e-15).all()
        kind = meta["kind"]
        for kd in (0, 1, 2):                                  # no screen area, non-finite vertices
            sel = (kind == kd) & ((kd < 2) | ~np.isfinite(tri).all(1))
            assert sel.sum() > 50 and (N[sel] == 1).all() and (rho[sel] == 0).all()
            assert (axis[sel] == [1.0, 0.0]).all()
        sel = kind == 4                                       # around s1 = 1, on both sides and on it
        assert {1} <= set(N[sel]) and (fp["s1"][sel] < 1).any() and (fp["s1"][sel] > 1).any()
        if T in (1, 2, 64):                                   # dyadic: the uvs hold the entries exactly
            assert (fp["s1"][sel] == 1).any()
            assert (N[sel & (fp["s1"] <= 1)] == 1).all()
            sel = kind == 5                                   # s1 / s2 = R exactly: ceil on its boundary
            assert np.array_equal(fp["s1"][sel], meta["R"][sel] * meta["g"][sel])
            many = np.where(fp["s1"][sel] > 1.0, np.minimum(meta["R"][sel], cap), 1)
            assert np.array_equal(N[sel], many.astype(np.int64)) and len(set(many)) == min(cap, 20)
            sel = kind == 6                                   # rank one: s2 = 0, N = cap
            assert (N[sel] == cap).all() and (fp["s1"][sel] > 1).all()
            sel = kind == 7                                   # equal scale: one probe
            assert (N[sel] == 1).all() and np.array_equal(fp["s1"][sel], meta["g"][sel])


def test_property_a_footprints_up_to_one_texel_are_the_bilinear_rule():
    T = 37
    rng = np.random.default_rng(5)
    levels = MR.pyramid(rng.integers(0, 256, (T, T, 4)).astype(np.uint8))
    flat = MR.flatten(levels)
    tri, uv, h, tx, ty, _ = _cases(T, 20000, 77)
    fp, _ = _restated(levels, tri, uv, h, tx, ty, 8)
    flat0 = fp["s1"] <= 1.0                                    # also every face without a footprint (s1 = 0)
    assert flat0.sum() > 2000 and (fp["N"][flat0] == 1).all() and (fp["k"][flat0] == 0).all()
    rgb = _host(flat, T, tri[flat0], uv[flat0], h, tx[flat0], ty[flat0], 8)[0]
    bil = _host_trilinear(flat, T, tx[flat0], ty[flat0], np.full(int(flat0.sum()), 0.5))
    assert np.array_equal(_bits(rgb), _bits(bil))


def test_property_b_equal_scale_maps_are_the_trilinear_rule():
    T = 64
    rng = np.random.default_rng(6)
    levels = MR.pyramid(rng.integers(0, 256, (T, T, 4)).astype(np.uint8))
    flat = MR.flatten(levels)
    n = 4000
    for scale in (1.0, 2.0, 3.5, 8.0):
        sx, sy = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
        tri, uv = _unit_items(T, sx * scale, 0.0, 0.0, sy * scale + np.zeros(n))
        tx, ty = rng.uniform(-2.0, T + 2.0, n), rng.uniform(-2.0, T + 2.0, n)
        u64 = uv.astype(np.float64)
        rho = MR.footprint(tri[:, 0:2], tri[:, 2:4], tri[:, 4:6], u64[:, 0:2], u64[:, 2:4], u64[:, 4:6], T, 1.0)
        assert (rho == scale).all()
        for cap in CAPS:
            rgb, probes, rho_a, axis = _host(flat, T, tri, uv, 1.0, tx, ty, cap)
            assert (probes == 1).all() and np.array_equal(_bits(rho_a), _bits(rho))
            assert np.array_equal(_bits(rgb), _bits(_host_trilinear(flat, T, tx, ty, rho)))


def test_property_c_one_probe_is_a_trilinear_filter_on_s1():
    T = 37
    rng = np.random.default_rng(7)
    levels = MR.pyramid(rng.integers(0, 256, (T, T, 4)).astype(np.uint8), rng.random((T, T)) < 0.7)
    flat = MR.flatten(levels)
    tri, uv, h, tx, ty, _ = _cases(T, 20000, 78)
    rgb, probes, rho, _ = _host(flat, T, tri, uv, h, tx, ty, 1)
    fp, _ = _restated(levels, tri, uv, h, tx, ty, 1)
    assert (probes == 1).all() and np.array_equal(_bits(rho), _bits(fp["s1"]))
    assert (rho > 4).sum() > 1000
    assert np.array_equal(_bits(rgb), _bits(_host_trilinear(flat, T, tx, ty, rho)))


def test_the_axis_sign_changes_only_the_order_of_the_sum():
    """The rule fixes the axis up to nothing (it names one of the two unit vectors), and the other one
    mirrors the probes: probe i takes the place of probe N - 1 - i.  One and two probes give the same
    bits (a two-term sum commutes; o = 0 has no side); more give the same sum up to its order and the
    last bit of the offsets — at most one f32 step of a value in [0, 1]."""
    T = 64
    rng = np.random.default_rng(8)
    levels = MR.pyramid(rng.integers(0, 256, (T, T, 4)).astype(np.uint8))
    tri, uv, h, tx, ty, _ = _cases(T, 20000, 79)
    keep = np.isfinite(tx) & np.isfinite(ty)
    fp, want = _restated(levels, tri[keep], uv[keep], h, tx[keep], ty[keep], 8)
    flipped = dict(fp, ax=-fp["ax"], ay=-fp["ay"])
    other = AR.sample(levels, tx[keep], ty[keep], flipped)
    one = fp["N"] == 1
    assert one.sum() > 1000 and (fp["N"] > 2).sum() > 1000
    assert np.array_equal(other[one], want[one])
    assert np.abs(other - want).max() <= 2.0 ** -23


# ------------------------------------------------------------------ the stripe case
def _stripes(T=64, along_rows=True):
    """Bands of 4 texel rows (or columns) alternating 0 / 255, RGBA."""
    band = ((np.arange(T) // 4) % 2 * 255).astype(np.uint8)
    grey = np.broadcast_to(band[:, None] if along_rows else band[None, :], (T, T))
    return np.concatenate([np.repeat(grey[..., None], 3, -1), np.full((T, T, 1), 255, np.uint8)], -1)


def _stripe_samples(T=64):
    """Texel points whose probes and level reads stay inside the image: tx, ty in 4 .. 59."""
    ty, tx = (a.reshape(-1).astype(np.float64) for a in np.mgrid[4:60, 4:60])
    return tx, ty


@pytest.mark.parametrize("through", ["restatement", "host"])
def test_stripes_survive_along_the_axis_that_is_not_compressed(through):
    T = 64
    tx, ty = _stripe_samples(T)
    n = len(tx)
    tri, uv = _unit_items(T, np.full(n, 8.0), 0.0, 0.0, 1.0)   # 8 texels per sample in u, 1 in v: s1 = 8, s2 = 1
    u8 = lambda rgb: np.floor(rgb.astype(np.float64) * 255.0 + 0.5).astype(np.int64)

    def run(levels, cap):
        if through == "host":
            rgb, probes, rho, axis = _host(MR.flatten(levels), T, tri, uv, 1.0, tx, ty, cap)
        else:
            fp, rgb = _restated(levels, tri, uv, 1.0, tx, ty, cap)
            probes, rho, axis = fp["N"], fp["rho"], np.stack([fp["ax"], fp["ay"]], 1)
        assert (probes == min(8, cap)).all() and (rho == 8.0 / min(8, cap)).all() and (axis == [1.0, 0.0]).all()
        return u8(rgb)

    def trilinear(levels):
        rho = np.full(n, 8.0)
        if through == "host":
            return u8(_host_trilinear(MR.flatten(levels), T, tx, ty, rho))
        return u8(MR.sample_rho(levels, tx, ty, rho))

    rows = MR.pyramid(_stripes(T, True))
    band = ((T - 1 - ty.astype(np.int64)) // 4) % 2 * 255       # image row of the sample = T - 1 - ty
    sharp, blurred, between = run(rows, 8), trilinear(rows), run(rows, 2)
    assert np.array_equal(sharp, np.repeat(band[:, None], 3, 1))
    assert np.isin(blurred, (127, 128)).all()
    assert ((between > np.minimum(sharp, blurred)) & (between < np.maximum(sharp, blurred))).all()
    # the same bands turned by 90 degrees vary along the compressed axis: both filters average them
    cols = MR.pyramid(_stripes(T, False))
    assert np.isin(run(cols, 8), (127, 128)).all() and np.isin(trilinear(cols), (127, 128)).all()


# ------------------------------------------------------------------ refusals
def test_the_host_entry_validates_its_arguments():
    lib = _lib()
    buf = np.zeros(4096, np.float64)
    fake = P(buf.ctypes.data)

    def call(pyramid=fake, T=8, tri=fake, uv=fake, h=1.0, tx=fake, ty=fake, cap=8, n=1, rgb=fake):
        return lib.dsu_aniso_sample_host(pyramid, T, tri, uv, h, tx, ty, cap, n, rgb, None, None, None)

    assert call() == 0
    assert call(T=0) == -1 and call(T=8193) == -1 and call(T=-2) == -1
    assert call(cap=0) == -1 and call(cap=17) == -1 and call(cap=-1) == -1
    assert call(n=-1) == -1
    assert call(h=float("nan")) == -1 and call(h=float("inf")) == -1
    for k in ("pyramid", "tri", "uv", "tx", "ty", "rgb"):
        assert call(**{k: None}) == -1, k
    assert call(pyramid=P(buf.ctypes.data + 2)) == -1
    assert lib.dsu_aniso_sample_host(None, 8, None, None, 1.0, None, None, 8, 0, None, None, None, None) == 0
    assert lib.dsu_aniso_sample_host(None, 8, None, None, 1.0, None, None, 0, 0, None, None, None, None) == -1


def test_the_render_entry_refuses_a_cap_outside_1_to_16_before_any_launch():
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    assert _lib.DEFINES["DSU_TEX_ANISOTROPIC"] == 3
    assert [f for f, _ in _lib.RenderTexture._fields_] == ["uv", "texels", "tex_size", "filter", "max_aniso"]
    buf = np.zeros(4096, np.int32)                            # host memory standing in: nothing may touch it
    fake = P(buf.ctypes.data)

    def call(filtered, stage=2, uv=fake, texels=fake, T=8, flt=3, cap=8, M=1):
        tex = ctypes.byref(_lib.RenderTexture(uv, texels, T, flt, cap))
        head = (stage, fake, fake, None, fake, tex, 1, 3, M, 0.0, 0.0, 1.35, 16, 4)
        tail = (fake, 4096 * 4, fake, 1, None, None, None, None, None, None, None)
        if filtered:
            taps = np.ones(4, np.float64)
            return lib.dsu_mesh_render_ortho_filtered(*head, _ptr(taps), 0, *tail)
        return lib.dsu_mesh_render_ortho(*head, *tail)

    for filtered in (False, True):
        for cap in (0, -1, 17, 1 << 20):
            assert call(filtered, cap=cap) == -1, cap
        assert call(filtered, flt=4) == -1 and call(filtered, flt=4, cap=8) == -1
        # a cap in range does not excuse the other fields
        assert call(filtered, uv=None) == -1 and call(filtered, texels=None) == -1
        assert call(filtered, T=0) == -1 and call(filtered, T=8193) == -1
        assert call(filtered, texels=P(buf.ctypes.data + 2)) == -1
        # the cap is read with DSU_TEX_ANISOTROPIC only, and at RASTER only
        for stage in (0, 1):
            assert call(filtered, stage=stage, M=0, cap=99) != -1
    assert not buf.any()


def test_keyword_errors():
    from drawingspinup_amd import ops
    assert ops.ANISOTROPIC == "anisotropic" and ops.TEX_ANISOTROPIC == 3
    assert ops.check_texture_filter("anisotropic") == 8 and ops.check_texture_filter("anisotropic", 16) == 16
    assert ops.check_texture_filter("bilinear") is None and ops.check_texture_filter("trilinear") is None
    for bad in (0, 17, -3, 2.5, True, "8"):
        with pytest.raises((ValueError, TypeError)):
            ops.check_texture_filter("anisotropic", bad)
    with pytest.raises(ValueError, match="max_anisotropy"):
        ops.check_texture_filter("trilinear", 4)
    with pytest.raises(ValueError, match="anisotropic"):
        ops.check_texture_filter("cubic")
    v = np.zeros((3, 3))
    tex = dict(texture=np.zeros((2, 2, 3), np.uint8), uvs=np.zeros((3, 2)))
    kw = dict(texture_filter="anisotropic", device="cpu")
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match="max_anisotropy"):
            animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", max_anisotropy=bad, **kw, **tex)
    with pytest.raises(ValueError, match="max_anisotropy"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", texture_filter="trilinear", max_anisotropy=4,
                              device="cpu", **tex)
    with pytest.raises(ValueError, match="together"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", **kw)
    with pytest.raises(ValueError, match="together"):
        animate.render_frames(v, [[0, 1, 2]], np.zeros((3, 3)), "rest_pose", uvs=np.zeros((3, 2)), **kw)
    with pytest.raises(ValueError, match="mip_coverage"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", mip_coverage="x", **kw, **tex)
    with pytest.raises(ValueError, match="texture_filter"):
        animate.render_frames(v, [[0, 1, 2]], None, "rest_pose", texture_filter="ewa", device="cpu", **tex)
    # the skinned route reads the same keywords before it touches the device
    import skin_ref as SK
    sk = animate.Skeleton(*SK.humanoid())
    with pytest.raises(ValueError, match="max_anisotropy"):
        animate.animate_mesh(v, [[0, 1, 2]], None, sk, animate.rest_clip(sk, 1), max_anisotropy=17, **kw, **tex)


def test_run_render_refuses_bad_anisotropy_when_the_arguments_are_read(tmp_path):
    from drawingspinup_amd.entry import run_render
    base = ["--data_dir", str(tmp_path), "--uid", "uid0", "--texture", "atlas"]
    for bad in (["--texture_filter", "anisotropic", "--max_anisotropy", "0"],
                ["--texture_filter", "anisotropic", "--max_anisotropy", "17"],
                ["--texture_filter", "anisotropic", "--max_anisotropy", "2.5"],
                ["--texture_filter", "trilinear", "--max_anisotropy", "4"],
                ["--texture_filter", "ewa"]):
        with pytest.raises(SystemExit):
            run_render.run(base + bad)
    # a good pair gets as far as looking for the mesh
    with pytest.raises(FileNotFoundError):
        run_render.run(base + ["--texture_filter", "anisotropic", "--max_anisotropy", "16"])
