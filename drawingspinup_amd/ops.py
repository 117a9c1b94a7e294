"""Thin tensor-level wrappers over the C ABI (one function per exported kernel).

These only allocate outputs (torch caching allocator), pass raw device pointers and the
current torch stream, and turn non-zero return codes into DsuError.  No arithmetic
happens in Python.
"""
import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import DsuError, HashGridCfg, NormCfg, SdfMlp, check, lib, ptr, stream


@dataclass(frozen=True)
class HashGridConfig:
    """configs/neuralangelo-ortho-wmask.yaml:52-62 (xyz_encoding_config)."""
    n_levels: int = 10
    n_features_per_level: int = 2
    log2_hashmap_size: int = 19
    base_resolution: int = 32
    per_level_scale: float = 1.3195079107728942

    def c(self):
        return HashGridCfg(self.n_levels, self.n_features_per_level, self.log2_hashmap_size,
                           self.base_resolution, self.per_level_scale)

    def levels(self):
        return _lib.hashgrid_levels(self.c())

    @property
    def n_entries(self):
        return self.levels()["offsets"][self.n_levels]

    @property
    def n_params(self):
        return self.n_entries * self.n_features_per_level

    @property
    def n_output_dims(self):
        return self.n_levels * self.n_features_per_level


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


# ------------------------------------------------------------------ hash grid / SDF network
def hashgrid_encode_fwd(cfg: HashGridConfig, table_f16, x, active_levels):
    x = _f32c(x)
    n = x.shape[0]
    out = torch.empty((n, cfg.n_output_dims), dtype=torch.float16, device=x.device)
    c = cfg.c()
    check(lib().dsu_hashgrid_encode_fwd(C.byref(c), ptr(table_f16, torch.float16), ptr(x), n,
                                        int(active_levels), ptr(out), stream()),
          "dsu_hashgrid_encode_fwd")
    return out


def hashgrid_encode_bwd(cfg: HashGridConfig, x, dout, active_levels, grad_table=None):
    x = _f32c(x)
    dout = _f32c(dout)
    n = x.shape[0]
    if grad_table is None:
        grad_table = torch.zeros(cfg.n_params, dtype=torch.float32, device=x.device)
    c = cfg.c()
    check(lib().dsu_hashgrid_encode_bwd(C.byref(c), ptr(x), ptr(dout), n, int(active_levels),
                                        ptr(grad_table, torch.float32), stream()),
          "dsu_hashgrid_encode_bwd")
    return grad_table


def _mlp_struct(w0, b0, w1, b1):
    for t in (w0, b0, w1, b1):
        ptr(t, torch.float32)
    return SdfMlp(w0.data_ptr(), b0.data_ptr(), w1.data_ptr(), b1.data_ptr())


def sdf_fwd(cfg, table_f16, mlp, pts, radius, active_levels, n_out=1):
    """mlp = (w0 (64,3+2L), b0 (64), w1 (13,64), b1 (13)) effective f32 weights."""
    pts = _f32c(pts)
    n = pts.shape[0]
    out = torch.empty((n, n_out), dtype=torch.float32, device=pts.device)
    c, m = cfg.c(), _mlp_struct(*mlp)
    check(lib().dsu_sdf_fwd(C.byref(c), ptr(table_f16, torch.float16), C.byref(m), ptr(pts), n,
                            float(radius), int(active_levels), int(n_out), ptr(out), stream()),
          "dsu_sdf_fwd")
    return out


def sdf_fwd_lattice(cfg, table_f16, mlp, lin, x0, nx, lo, span, radius, active_levels, out):
    """SDF on x-slabs [x0, x0 + nx) of the res^3 export lattice, points formed in the kernel
    (p = lin[i] * span + lo per axis); lin (res) f32 device, lo / span three host floats (f32 values);
    out: f32 view of nx * res * res elements, written in place."""
    res = lin.shape[0]
    c, m = cfg.c(), _mlp_struct(*mlp)
    lo3 = (C.c_float * 3)(*[float(v) for v in lo])
    sp3 = (C.c_float * 3)(*[float(v) for v in span])
    if out.numel() != nx * res * res:
        raise DsuError("sdf_fwd_lattice: output size")
    check(lib().dsu_sdf_fwd_lattice(C.byref(c), ptr(table_f16, torch.float16), C.byref(m),
                                    ptr(lin, torch.float32), res, int(x0), int(nx), lo3, sp3,
                                    float(radius), int(active_levels), ptr(out, torch.float32), stream()),
          "dsu_sdf_fwd_lattice")
    return out


def spatial_sort(pts, radius, bits=6):
    """Morton-bin the points of one step (csrc/spatial_sort.hip): returns (pts_sorted, perm) with
    pts_sorted[i] = pts[perm[i]].  Pass both to sdf_fd_fwd / sdf_fd_bwd (perm=...)."""
    pts = _f32c(pts)
    n = pts.shape[0]
    dev = pts.device
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty_like(pts)
    wbytes = int(lib().dsu_spatial_sort_workspace_bytes(n, int(bits)))
    if wbytes < 0:
        check(wbytes, "dsu_spatial_sort_workspace_bytes")
    ws = torch.empty(max(wbytes, 4) // 4, dtype=torch.int32, device=dev)
    check(lib().dsu_spatial_sort(ptr(pts), n, float(radius), int(bits), ptr(perm), ptr(out),
                                 ptr(ws), wbytes, stream()), "dsu_spatial_sort")
    return out, perm


def sdf_fd_fwd(cfg, table_f16, mlp, pts, radius, eps, active_levels, with_grad=True,
               with_feature=True, with_laplace=True, enc_cache=None, perm=None):
    """enc_cache: True -> also return the feature cache tensor for sdf_fd_bwd (5th value).
    perm (int32, from spatial_sort): `pts` are the sorted points; outputs come back in the
    caller's original row order (row perm[i] = result of pts[i]); the cache stays in sorted order."""
    pts = _f32c(pts)
    n = pts.shape[0]
    dev = pts.device
    cache = None
    if enc_cache:
        nbytes = int(lib().dsu_sdf_fd_enc_cache_bytes(n, int(active_levels)))
        cache = torch.empty(max(nbytes, 4) // 2, dtype=torch.float16, device=dev)
    sdf = torch.empty(n, dtype=torch.float32, device=dev)
    grad = torch.empty((n, 3), dtype=torch.float32, device=dev) if with_grad else None
    feat = torch.empty((n, 13), dtype=torch.float32, device=dev) if with_feature else None
    lap = torch.empty(n, dtype=torch.float32, device=dev) if with_laplace else None
    c, m = cfg.c(), _mlp_struct(*mlp)
    check(lib().dsu_sdf_fd_fwd_sorted(C.byref(c), ptr(table_f16, torch.float16), C.byref(m),
                                      ptr(pts), ptr(perm, torch.int32), n, float(radius),
                                      float(eps), int(active_levels),
                                      ptr(sdf), ptr(grad), ptr(feat), ptr(lap), ptr(cache),
                                      stream()), "dsu_sdf_fd_fwd_sorted")
    if enc_cache:
        return sdf, grad, feat, lap, cache
    return sdf, grad, feat, lap


def sdf_fd_bwd(cfg, table_f16, mlp, pts, radius, eps, active_levels, d_sdf, d_grad, d_feature,
               d_laplace, grad_table=None, enc_cache=None, perm=None, extra=None):
    """perm: as in sdf_fd_fwd (`pts` sorted, the upstream gradients in the original row order).
    extra: a DeferredSum (texture_bwd_shaded_partials) carried out by the scatter launch."""
    pts = _f32c(pts)
    n = pts.shape[0]
    dev = pts.device
    w0, b0, w1, b1 = mlp
    if grad_table is None:
        grad_table = torch.zeros(cfg.n_params, dtype=torch.float32, device=dev)
    sizes = [t.numel() for t in (w0, b0, w1, b1)]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)      # one memset
    g = [v.view_as(t) for v, t in zip(torch.split(flat, sizes), (w0, b0, w1, b1))]
    c, m = cfg.c(), _mlp_struct(*mlp)
    d = [None if t is None else _f32c(t) for t in (d_sdf, d_grad, d_feature, d_laplace)]
    wbytes = lib().dsu_sdf_fd_bwd_workspace_bytes(C.byref(c), n)
    if wbytes < 0:
        check(int(wbytes), "dsu_sdf_fd_bwd_workspace_bytes")
    ws = torch.empty(max(int(wbytes), 4) // 4, dtype=torch.float32, device=dev)
    if enc_cache is not None:
        need = int(lib().dsu_sdf_fd_enc_cache_bytes(n, int(active_levels)))
        if enc_cache.numel() * enc_cache.element_size() < need:
            raise DsuError("feature cache smaller than dsu_sdf_fd_enc_cache_bytes")
    if extra is not None:
        # the scatter launch also carries out a deferred partial sum of another kernel
        check(lib().dsu_sdf_fd_bwd_sorted_fold(C.byref(c), ptr(table_f16, torch.float16), C.byref(m),
                                               ptr(pts), ptr(perm, torch.int32), n, float(radius),
                                               float(eps), int(active_levels),
                                               ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]),
                                               ptr(grad_table), ptr(g[0]), ptr(g[1]), ptr(g[2]),
                                               ptr(g[3]), ptr(ws), int(wbytes), ptr(enc_cache), None,
                                               C.byref(extra.record), stream()),
              "dsu_sdf_fd_bwd_sorted_fold")
        return grad_table, g
    check(lib().dsu_sdf_fd_bwd_sorted(C.byref(c), ptr(table_f16, torch.float16), C.byref(m),
                                      ptr(pts), ptr(perm, torch.int32), n, float(radius),
                                      float(eps), int(active_levels),
                                      ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(grad_table),
                                      ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(ws),
                                      int(wbytes), ptr(enc_cache), stream()),
          "dsu_sdf_fd_bwd_sorted")
    return grad_table, g


# ------------------------------------------------------------------ hash-table optimizer
def table_adamw(p, g, m, v, img_f16, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt):
    """One torch.optim.AdamW update of the first n floats of the table (active levels), fused
    with the f16 image rewrite and the gradient reset."""
    check(lib().dsu_table_adamw(ptr(p, torch.float32), ptr(g, torch.float32), ptr(m, torch.float32),
                                ptr(v, torch.float32), ptr(img_f16, torch.float16), int(n),
                                float(lr), float(beta1), float(beta2), float(eps),
                                float(weight_decay), float(bc1), float(bc2_sqrt), stream()),
          "dsu_table_adamw")


def adamw_multi(entries, beta1, beta2, eps, weight_decay):
    """entries: list of (p, g, m, v, lr, bc1, bc2_sqrt) f32 device tensors / floats (<= 24): one
    launch of torch.optim.AdamW's update for all of them."""
    n = len(entries)
    if n == 0:
        return
    arr = (_lib.AdamwTensor * n)()
    for k, (p, g, m, v, lr, bc1, bc2s) in enumerate(entries):
        a = arr[k]
        a.p, a.g, a.m, a.v = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        a.n, a.lr, a.bias_correction1, a.bias_correction2_sqrt = p.numel(), lr, bc1, bc2s
    check(lib().dsu_adamw_multi(arr, n, float(beta1), float(beta2), float(eps), float(weight_decay),
                                stream()), "dsu_adamw_multi")


def table_decay(p, img_f16, start, n, factor):
    """p[start:start+n] *= factor (+ f16 image); start, n multiples of 4 floats."""
    check(lib().dsu_table_decay(C.c_void_p(p.data_ptr() + 4 * int(start)),
                                C.c_void_p(img_f16.data_ptr() + 2 * int(start)), int(n),
                                float(factor), stream()), "dsu_table_decay")


# ------------------------------------------------------------------ export: mcubes.smooth
def smooth_iterate(nbr, lower, upper, x, y, weight, iters):
    """`iters` projected weighted-Jacobi iterations on the band voxels, in place on x (f64);
    lower / upper: per-voxel bounds (f64, +-inf = none)."""
    nv = x.shape[0]
    check(lib().dsu_smooth_iterate(ptr(nbr, torch.int32), nv, ptr(lower, torch.float64),
                                   ptr(upper, torch.float64), float(weight), int(iters), ptr(x, torch.float64),
                                   ptr(y, torch.float64), stream()), "dsu_smooth_iterate")
    return x


def smooth_energy(nbr, x, y):
    """x . Q x / 2 (device scalar, f64; fixed summation order)."""
    nv = x.shape[0]
    part = torch.empty(int(lib().dsu_smooth_energy_partials()), dtype=torch.float64,
                       device=x.device)
    check(lib().dsu_smooth_energy(ptr(nbr, torch.int32), nv, ptr(x, torch.float64),
                                  ptr(y, torch.float64), ptr(part), stream()),
          "dsu_smooth_energy")
    return part.sum() / 2


class SmoothBricks:
    """The band of one volume in the brick layout of csrc/mesh_smooth.hip (include/dsu_hip.h,
    dsu_smooth_bricks_*): nb active bricks, x / y (nb, 512) f64, mask (nb, 8) i64 words, nbr6
    (nb, 8) i32, bcoord (nb,) i32, and the bounds' initial distance as x0 (nb, 512) f64 or as code
    (nb, 512) u8 into values (<= 255 ascending f64)."""
    __slots__ = ("shape", "nb", "x", "y", "mask", "nbr6", "bcoord", "x0", "code", "values")


def smooth_bricks_build(band, dist, values=None):
    """band (X,Y,Z) bool/uint8, dist (X,Y,Z) f64 -> SmoothBricks, or None when the band is empty
    (nothing but the occupancy pass is launched then).  values: ascending f64 candidates of the
    band's distinct distances (<= 255) for the byte-coded bounds; None, or a band value outside
    them, stores the distances as doubles instead."""
    b = band.contiguous()
    if b.dtype == torch.bool:
        b = b.view(torch.uint8)
    X, Y, Z = b.shape
    dev = b.device
    side = int(lib().dsu_smooth_brick_side())
    nbricks = -(-X // side) * -(-Y // side) * -(-Z // side)
    flags = torch.zeros(nbricks, dtype=torch.int32, device=dev)
    check(lib().dsu_smooth_bricks_flags(ptr(b, torch.uint8), X, Y, Z, ptr(flags), stream()),
          "dsu_smooth_bricks_flags")
    bcoord = torch.nonzero(flags).view(-1).to(torch.int32)
    nb = bcoord.shape[0]
    if nb == 0:
        return None
    table = torch.full((nbricks,), -1, dtype=torch.int32, device=dev)
    table[bcoord.long()] = torch.arange(nb, dtype=torch.int32, device=dev)
    s = SmoothBricks()
    s.shape, s.nb, s.bcoord = (X, Y, Z), nb, bcoord
    s.x = torch.empty((nb, 512), dtype=torch.float64, device=dev)
    s.y = torch.zeros((nb, 512), dtype=torch.float64, device=dev)
    s.mask = torch.empty((nb, 8), dtype=torch.int64, device=dev)
    s.nbr6 = torch.empty((nb, 8), dtype=torch.int32, device=dev)
    s.x0 = s.code = s.values = None

    def gather(x0, code, vals, miss):
        check(lib().dsu_smooth_bricks_gather(
            ptr(b, torch.uint8), ptr(dist, torch.float64), X, Y, Z, ptr(table), ptr(bcoord), nb,
            ptr(vals, torch.float64), 0 if vals is None else vals.shape[0], ptr(s.x), ptr(x0),
            ptr(code), ptr(s.mask), ptr(s.nbr6), ptr(miss), stream()), "dsu_smooth_bricks_gather")

    if values is not None and 0 < values.shape[0] <= 255:
        vals = values.to(device=dev, dtype=torch.float64).contiguous()
        code = torch.empty((nb, 512), dtype=torch.uint8, device=dev)
        miss = torch.zeros(1, dtype=torch.int32, device=dev)
        gather(None, code, vals, miss)
        if int(miss.item()) == 0:
            s.code, s.values = code, vals
            return s
    s.x0 = torch.empty((nb, 512), dtype=torch.float64, device=dev)
    gather(s.x0, None, None, None)
    return s


def smooth_bricks_iterate(s, weight, iters, direct=False):
    """`iters` projected weighted-Jacobi iterations in place on s.x (one launch each)."""
    check(lib().dsu_smooth_bricks_iterate(
        ptr(s.nbr6, torch.int32), ptr(s.mask, torch.int64), s.nb, ptr(s.x0, torch.float64),
        ptr(s.code, torch.uint8), ptr(s.values, torch.float64),
        0 if s.values is None else s.values.shape[0], float(weight), int(iters), int(bool(direct)),
        ptr(s.x, torch.float64), ptr(s.y, torch.float64), stream()), "dsu_smooth_bricks_iterate")


def smooth_bricks_energy(s):
    """x . Q x / 2 on the brick layout (device scalar, f64; fixed summation order)."""
    part = torch.empty(s.nb, dtype=torch.float64, device=s.x.device)
    check(lib().dsu_smooth_bricks_energy(ptr(s.nbr6, torch.int32), ptr(s.mask, torch.int64), s.nb,
                                         ptr(s.x, torch.float64), ptr(part), stream()),
          "dsu_smooth_bricks_energy")
    return part.sum() / 2


def smooth_bricks_scatter(s, dist):
    """dist[band] = x, in place."""
    X, Y, Z = s.shape
    check(lib().dsu_smooth_bricks_scatter(ptr(s.x, torch.float64), ptr(s.mask, torch.int64),
                                          ptr(s.bcoord, torch.int32), s.nb, X, Y, Z,
                                          ptr(dist, torch.float64), stream()),
          "dsu_smooth_bricks_scatter")
    return dist


def volume_band_distance(binary, R, value_table, band_table):
    """binary (X,Y,Z) bool/uint8 device volume -> (dist f64 (X,Y,Z), band bool (X,Y,Z)) through the
    caller's tables over d2 = min(squared distance to the nearest voxel of the other class, (R+1)^2):
    value_table (2, (R+1)^2 + 1) f64 (row 0: inside voxels), band_table ((R+1)^2 + 1) uint8."""
    b = binary.contiguous()
    if b.dtype == torch.bool:
        b = b.view(torch.uint8)
    X, Y, Z = b.shape
    dev = b.device
    dist = torch.empty((X, Y, Z), dtype=torch.float64, device=dev)
    band = torch.empty((X, Y, Z), dtype=torch.uint8, device=dev)
    wbytes = int(lib().dsu_volume_band_distance_workspace_bytes(X, Y, Z))
    if wbytes < 0:
        check(wbytes, "dsu_volume_band_distance_workspace_bytes")
    ws = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    check(lib().dsu_volume_band_distance(ptr(b, torch.uint8), X, Y, Z, int(R),
                                         ptr(value_table, torch.float64), ptr(band_table, torch.uint8),
                                         ptr(dist), ptr(band), ptr(ws), wbytes, stream()),
          "dsu_volume_band_distance")
    return dist, band.view(torch.bool)


def mc_cube_index(volume, isovalue):
    """(X,Y,Z) f64 device volume -> (X-1,Y-1,Z-1) uint8 marching-cubes configuration bytes."""
    X, Y, Z = volume.shape
    cube = torch.empty((X - 1, Y - 1, Z - 1), dtype=torch.uint8, device=volume.device)
    check(lib().dsu_mc_cube_index(ptr(volume, torch.float64), X, Y, Z, float(isovalue), ptr(cube),
                                  stream()), "dsu_mc_cube_index")
    return cube


# ------------------------------------------------------------------ nerfacc replacements
def ray_aabb(rays_o, rays_d, aabb6, jitter=None, step=0.0):
    rays_o, rays_d = _f32c(rays_o), _f32c(rays_d)
    n = rays_o.shape[0]
    t_min = torch.empty(n, dtype=torch.float32, device=rays_o.device)
    t_max = torch.empty_like(t_min)
    a = (C.c_float * 6)(*[float(v) for v in aabb6])
    check(lib().dsu_ray_aabb(ptr(rays_o), ptr(rays_d), n, a, ptr(jitter), float(step),
                             ptr(t_min), ptr(t_max), stream()), "dsu_ray_aabb")
    return t_min, t_max


# lazily built, process-wide; keyed by stream: drawings in flight on one GPU run on their own streams
_MARCH_SCRATCH = {}


class MarchHandle:
    """State between ray_march_begin (march + offsets scan, all asynchronous) and the packing
    (needs the host-side total to size the packed outputs)."""
    __slots__ = ("rays_o", "rays_d", "counts", "offsets", "stats", "scratch", "cap", "n")

    def check_capacity(self, cmax):
        """The rows hold cap = int(diag / step) + 8 samples, diag the box diagonal.  A ray has at
        most (far - near) / step + 2 samples and far - near <= diag (both ends lie in the box), so
        this cannot trip; the marcher drops what a longer ray would write past its row."""
        if cmax > self.cap:
            raise DsuError(f"a ray produced {cmax} samples, above the scratch capacity {self.cap}")


def ray_march_begin(rays_o, rays_d, t_min, t_max, aabb6, occ_binary, res, step):
    """Launch the march into the scratch rows and the offsets scan.  Nothing here waits for the
    device; the caller reads `handle.stats` (int32[2] = total, max count)."""
    import math
    rays_o, rays_d = _f32c(rays_o), _f32c(rays_d)
    n = rays_o.shape[0]
    dev = rays_o.device
    a = (C.c_float * 6)(*[float(v) for v in aabb6])
    diag = math.sqrt(sum((aabb6[3 + d] - aabb6[d]) ** 2 for d in range(3)))
    cap = int(diag / step) + 8
    key = (str(dev), cap, stream().value)          # scratch rows belong to ONE stream's launches
    sc = _MARCH_SCRATCH.get(key)
    if sc is None or sc[0].shape[0] < n * cap:
        rows = max(n, 8192)
        sc = (torch.empty(rows * cap, dtype=torch.float32, device=dev),
              torch.empty(rows * cap, dtype=torch.float32, device=dev))
        _MARCH_SCRATCH[key] = sc
    h = MarchHandle()
    h.rays_o, h.rays_d, h.scratch, h.cap, h.n = rays_o, rays_d, sc, cap, n
    h.counts = torch.empty(n, dtype=torch.int32, device=dev)
    h.offsets = torch.empty(n, dtype=torch.int32, device=dev)
    h.stats = torch.empty(2, dtype=torch.int32, device=dev)
    occp = ptr(occ_binary, torch.uint8) if occ_binary is not None else None
    check(lib().dsu_ray_march_scratch(ptr(rays_o), ptr(rays_d), ptr(t_min), ptr(t_max), n, a, occp,
                                      int(res), float(step), cap, ptr(h.counts), ptr(sc[0]),
                                      ptr(sc[1]), stream()), "dsu_ray_march_scratch")
    check(lib().dsu_ray_offsets(ptr(h.counts), n, ptr(h.offsets), ptr(h.stats), stream()),
          "dsu_ray_offsets")
    return h


def ray_march(rays_o, rays_d, t_min, t_max, aabb6, occ_binary, res, step):
    """nerfacc's ray_marching.  Returns ray_indices (int64), t_starts, t_ends (n,), and the per-ray
    (offsets, counts) int32 packing the compositing kernels consume."""
    h = ray_march_begin(rays_o, rays_d, t_min, t_max, aabb6, occ_binary, res, step)
    total, cmax = h.stats.tolist()                                # one host sync
    h.check_capacity(cmax)
    dev = h.rays_o.device
    ray_indices = torch.empty(total, dtype=torch.int64, device=dev)
    t_starts = torch.empty(total, dtype=torch.float32, device=dev)
    t_ends = torch.empty(total, dtype=torch.float32, device=dev)
    if total > 0:
        check(lib().dsu_ray_compact(ptr(h.scratch[0]), ptr(h.scratch[1]), h.cap, ptr(h.offsets),
                                    ptr(h.counts), h.n, ptr(ray_indices), ptr(t_starts),
                                    ptr(t_ends), stream()), "dsu_ray_compact")
    return ray_indices, t_starts, t_ends, h.offsets, h.counts


def ray_march_finish(h, total, cmax, tail_rows=0):
    """Pack the scratch rows: returns (points (total + tail_rows, 3), t_starts, t_ends)."""
    h.check_capacity(cmax)
    dev = h.rays_o.device
    points = torch.empty(total + tail_rows, 3, dtype=torch.float32, device=dev)
    t_starts = torch.empty(total, dtype=torch.float32, device=dev)
    t_ends = torch.empty(total, dtype=torch.float32, device=dev)
    if total > 0:
        check(lib().dsu_ray_compact_points(ptr(h.scratch[0]), ptr(h.scratch[1]), h.cap,
                                           ptr(h.offsets), ptr(h.counts), h.n, ptr(h.rays_o),
                                           ptr(h.rays_d), ptr(t_starts), ptr(t_ends), ptr(points),
                                           stream()), "dsu_ray_compact_points")
    return points, t_starts, t_ends


def ray_march_points(rays_o, rays_d, t_min, t_max, aabb6, occ_binary, res, step, tail_rows=0):
    """Single-pass march for the fused optimisation step: returns
    (points (total + tail_rows, 3), t_starts, t_ends, offsets, counts, total) where
    points[:total] = rays_o[r] + rays_d[r] * (t_start + t_end) / 2 and the tail rows are left for
    the caller (random / perturbed points evaluated in the same geometry launch).  One host copy
    (total, max count); no ray_indices."""
    h = ray_march_begin(rays_o, rays_d, t_min, t_max, aabb6, occ_binary, res, step)
    total, cmax = h.stats.tolist()                                # the step's one host sync
    points, t_starts, t_ends = ray_march_finish(h, total, cmax, tail_rows)
    return points, t_starts, t_ends, h.offsets, h.counts, total


def _tex_struct(params):
    from ._lib import TexMlp
    for t, shape in zip(params, ((64, 16), (64,), (64, 64), (64,), (3, 64), (3,))):
        if tuple(t.shape) != shape:
            raise DsuError(f"texture MLP parameter of shape {tuple(t.shape)}, expected {shape}")
    return TexMlp(*[ptr(t, torch.float32).value for t in params])


def texture_fwd(params, tex_in):
    """params = [w0 (64,16), b0, w1 (64,64), b1, w2 (3,64), b2] f32 contiguous;
    returns rgb (n,3) = sigmoid(MLP(tex_in))."""
    tex_in = _f32c(tex_in)
    n = tex_in.shape[0]
    assert tex_in.shape[1] == 16
    rgb = torch.empty((n, 3), dtype=torch.float32, device=tex_in.device)
    m = _tex_struct(params)
    check(lib().dsu_texture_fwd(C.byref(m), ptr(tex_in), n, ptr(rgb), stream()), "dsu_texture_fwd")
    return rgb


def texture_bwd(params, tex_in, rgb, d_rgb):
    """Returns (d_tex_in (n,16), [g_w0, g_b0, g_w1, g_b1, g_w2, g_b2])."""
    tex_in, rgb, d_rgb = _f32c(tex_in), _f32c(rgb), _f32c(d_rgb)
    n = tex_in.shape[0]
    dev = tex_in.device
    d_in = torch.empty_like(tex_in)
    sizes = [t.numel() for t in params]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
    g = [v.view_as(t) for v, t in zip(torch.split(flat, sizes), params)]
    wbytes = int(lib().dsu_texture_bwd_workspace_bytes(n))
    ws = torch.empty(max(wbytes, 4) // 4, dtype=torch.float32, device=dev)
    m = _tex_struct(params)
    check(lib().dsu_texture_bwd(C.byref(m), ptr(tex_in), ptr(rgb), ptr(d_rgb), n, ptr(d_in),
                                *[ptr(t) for t in g], ptr(ws), wbytes, stream()),
          "dsu_texture_bwd")
    return d_in, g


def texture_fwd_shaded(params, feature, grad, with_mask=False):
    """shade_prep_fwd + texture_fwd in one launch: returns (normal (n,3), rgb (n,3)) and, with_mask,
    the ReLU pattern of hidden layer 1 ((n,2) int32 words) for texture_bwd_shaded_partials(h1_mask=)."""
    feature, grad = _f32c(feature), _f32c(grad)
    n = feature.shape[0]
    normal = torch.empty((n, 3), dtype=torch.float32, device=feature.device)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=feature.device)
    m = _tex_struct(params)
    mask = torch.empty((n, 2), dtype=torch.int32, device=feature.device) if with_mask else None
    check(lib().dsu_texture_fwd_shaded_m(C.byref(m), ptr(feature), ptr(grad), n, ptr(normal), ptr(rgb),
                                         ptr(mask), stream()), "dsu_texture_fwd_shaded_m")
    return (normal, rgb, mask) if with_mask else (normal, rgb)


def texture_bwd_shaded(params, feature, grad, rgb, d_rgb, d_normal, tail_rows=0):
    """texture_bwd + shade_prep_bwd in one launch (+ the reduction): returns
    (d_grad (n,3), d_feature (n + tail_rows, 13) with zero tail rows, [g_w0 .. g_b2])."""
    feature, grad, rgb, d_rgb = _f32c(feature), _f32c(grad), _f32c(rgb), _f32c(d_rgb)
    n = rgb.shape[0]
    dev = rgb.device
    d_grad = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d_feat = torch.empty((n + tail_rows, 13), dtype=torch.float32, device=dev)
    sizes = [t.numel() for t in params]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
    g = [v.view_as(t) for v, t in zip(torch.split(flat, sizes), params)]
    wbytes = int(lib().dsu_texture_bwd_workspace_bytes(n))
    ws = torch.empty(max(wbytes, 4) // 4, dtype=torch.float32, device=dev)
    m = _tex_struct(params)
    dn = None if d_normal is None else _f32c(d_normal)
    check(lib().dsu_texture_bwd_shaded(C.byref(m), ptr(feature), ptr(grad), ptr(rgb), ptr(d_rgb),
                                       ptr(dn), n, int(tail_rows), ptr(d_grad), ptr(d_feat),
                                       *[ptr(t) for t in g], ptr(ws), wbytes, stream()),
          "dsu_texture_bwd_shaded")
    return d_grad, d_feat, g


def texture_partial_map():
    """Destination of every element of the texture backward's partial vectors inside a contiguous
    [w0 | b0 | w1 | b1 | w2 | b2] gradient block (-1: padding), host int32 array."""
    import numpy as np
    n = int(lib().dsu_texture_partial_map(None))
    m = np.empty(n, dtype=np.int32)
    lib().dsu_texture_partial_map(m.ctypes.data_as(C.c_void_p))
    return m


class DeferredSum:
    """A dsu_partial_reduce record plus the tensors it points into (kept alive with it)."""

    def __init__(self, record, keep):
        self.record, self.keep = record, keep


def texture_bwd_shaded_partials(params, feature, grad, rgb, d_rgb, d_normal, tail_rows=0, h1_mask=None):
    """texture_bwd_shaded WITHOUT the final sum: returns (d_grad, d_feature, g_flat, deferred) where
    g_flat (zeros now) is the contiguous gradient block the deferred sum will be added to by the
    launch it is handed to (sdf_fd_bwd(..., extra=deferred)).  h1_mask: texture_fwd_shaded(with_mask=True)'s
    pattern (the recompute of layer 1 then runs as bf16 x 3)."""
    from ._lib import PartialReduce
    feature, grad, rgb, d_rgb = _f32c(feature), _f32c(grad), _f32c(rgb), _f32c(d_rgb)
    n = rgb.shape[0]
    dev = rgb.device
    d_grad = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d_feat = torch.empty((n + tail_rows, 13), dtype=torch.float32, device=dev)
    flat = torch.zeros(sum(t.numel() for t in params), dtype=torch.float32, device=dev)
    wbytes = int(lib().dsu_texture_bwd_workspace_bytes(n))
    ws = torch.empty(max(wbytes, 4) // 4, dtype=torch.float32, device=dev)
    m = _tex_struct(params)
    dn = None if d_normal is None else _f32c(d_normal)
    rec = PartialReduce()
    check(lib().dsu_texture_bwd_shaded_partials_m(C.byref(m), ptr(feature), ptr(grad), ptr(rgb),
                                                  ptr(d_rgb), ptr(dn), n, int(tail_rows), ptr(d_grad),
                                                  ptr(d_feat), ptr(h1_mask, torch.int32), ptr(ws), wbytes,
                                                  C.byref(rec), stream()),
          "dsu_texture_bwd_shaded_partials_m")
    tmap = torch.from_numpy(texture_partial_map()).to(dev)
    rec.map, rec.base = tmap.data_ptr(), flat.data_ptr()
    return d_grad, d_feat, flat, DeferredSum(rec, (ws, tmap, flat))


def ortho_ray_batch(index, x, y, c2w, origins, directions, images, normals, masks, view_weights):
    """Fused preprocess_data: returns the batch dict (rays (n,6), rgb, normal, mask, cosines,
    view_weights) for int64 (index, x, y) draws.  Dataset tensors (V,H,W,*) f32 contiguous."""
    n = index.shape[0]
    dev = images.device
    V, H, W, ch = images.shape
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = {"rays": f(n, 6), "rgb": f(n, ch), "normal": f(n, 3), "mask": f(n), "cosines": f(n),
           "view_weights": f(n)}
    i64 = torch.int64
    check(lib().dsu_ortho_ray_batch(ptr(index, i64), ptr(x, i64), ptr(y, i64), n, ptr(_f32c(c2w)),
                                    ptr(origins, torch.float32), ptr(directions, torch.float32),
                                    ptr(images, torch.float32), ch, ptr(normals, torch.float32),
                                    ptr(masks, torch.float32), ptr(view_weights, torch.float32), H,
                                    W, ptr(out["rays"]), ptr(out["rgb"]), ptr(out["normal"]),
                                    ptr(out["mask"]), ptr(out["cosines"]), ptr(out["view_weights"]),
                                    stream()), "dsu_ortho_ray_batch")
    return out


RAY_LOSS_MAX_RAYS = _lib.DEFINES["DSU_RAY_LOSS_MAX_RAYS"]


def ray_losses(comp, rgb, normal, mask, cosines, view_weights, cfg):
    """Fused ray-level loss terms + d/d comp.  cfg: dict with rgb_p_ratio, normal_p_ratio,
    mask_p_ratio, lambda_rgb_mse, lambda_rgb_l1, lambda_normal, lambda_mask, geo_aware.
    Returns (terms (4,) = [rgb_mse, rgb_l1, normal, mask], d_comp (R,8))."""
    from ._lib import RayLossCfg
    comp = _f32c(comp)
    r = comp.shape[0]
    c = RayLossCfg(float(cfg["rgb_p_ratio"]), float(cfg["normal_p_ratio"]),
                   float(cfg["mask_p_ratio"]), float(cfg["lambda_rgb_mse"]),
                   float(cfg["lambda_rgb_l1"]), float(cfg["lambda_normal"]),
                   float(cfg["lambda_mask"]), int(bool(cfg["geo_aware"])), 0)
    terms = torch.empty(4, dtype=torch.float32, device=comp.device)
    d_comp = torch.empty_like(comp)
    check(lib().dsu_ray_losses(ptr(comp), ptr(_f32c(rgb)), ptr(_f32c(normal)), ptr(_f32c(mask)),
                               ptr(_f32c(cosines)), ptr(_f32c(view_weights)), r, C.byref(c),
                               ptr(terms), ptr(d_comp), stream()), "dsu_ray_losses")
    return terms, d_comp


def sample_losses(sdf_all, grad_all, n_samples, n_random, lambda_eikonal, lambda_sparsity,
                  sparsity_scale, lambda_smooth, d_sdf_all=None, d_grad_all=None):
    """Fused sample-level loss terms + gradients.  With d_sdf_all / d_grad_all given, their
    first n_samples rows already hold the compositing / shading gradients and the eikonal part
    is added; otherwise fresh tensors are returned.
    Returns (terms (3,) = [eikonal, sparsity, normal_smooth], d_sdf_all, d_grad_all)."""
    sdf_all, grad_all = _f32c(sdf_all), _f32c(grad_all)
    acc = d_sdf_all is not None
    if not acc:
        d_sdf_all = torch.empty_like(sdf_all)
        d_grad_all = torch.empty_like(grad_all)
    assert sdf_all.shape[0] == n_samples + 2 * n_random
    terms = torch.empty(3, dtype=torch.float32, device=sdf_all.device)
    check(lib().dsu_sample_losses(ptr(sdf_all), ptr(grad_all), n_samples, n_random,
                                  float(lambda_eikonal), float(lambda_sparsity),
                                  float(sparsity_scale), float(lambda_smooth), int(acc),
                                  ptr(d_sdf_all, torch.float32), ptr(d_grad_all, torch.float32),
                                  ptr(terms), stream()), "dsu_sample_losses")
    return terms, d_sdf_all, d_grad_all


def weights_from_alpha_fwd(alpha, offsets, counts):
    alpha = _f32c(alpha)
    w = torch.empty_like(alpha)
    check(lib().dsu_weights_from_alpha_fwd(ptr(alpha), ptr(offsets, torch.int32),
                                           ptr(counts, torch.int32), offsets.shape[0], ptr(w),
                                           stream()), "dsu_weights_from_alpha_fwd")
    return w


def weights_from_alpha_bwd(alpha, weights, d_weights, offsets, counts):
    d_alpha = torch.empty_like(alpha)
    check(lib().dsu_weights_from_alpha_bwd(ptr(_f32c(alpha)), ptr(_f32c(weights)),
                                           ptr(_f32c(d_weights)), ptr(offsets, torch.int32),
                                           ptr(counts, torch.int32), offsets.shape[0],
                                           ptr(d_alpha), stream()), "dsu_weights_from_alpha_bwd")
    return d_alpha


def accumulate_fwd(weights, values, offsets, counts):
    weights = _f32c(weights)
    n_rays = offsets.shape[0]
    ch = 1 if values is None else values.shape[-1]
    v = None if values is None else _f32c(values)
    out = torch.empty((n_rays, ch), dtype=torch.float32, device=weights.device)
    check(lib().dsu_accumulate_fwd(ptr(weights), ptr(v), ch, ptr(offsets, torch.int32),
                                   ptr(counts, torch.int32), n_rays, ptr(out), stream()),
          "dsu_accumulate_fwd")
    return out


def occgrid_ema(occs, idx, occ, decay):
    """occs[idx] = max(occs[idx] * decay, occ): old values gathered first; a cell listed several
    times is decayed once and keeps its largest candidate."""
    scratch = torch.empty(occ.shape[0], dtype=torch.float32, device=occs.device) \
        if idx is not None else None
    check(lib().dsu_occgrid_ema(ptr(occs, torch.float32), ptr(idx, torch.int64) if idx is not None
                                else None, ptr(_f32c(occ)), occ.shape[0], float(decay),
                                ptr(scratch) if scratch is not None else None, stream()),
          "dsu_occgrid_ema")


def occgrid_binarize(occs, thre):
    out = torch.empty(occs.shape[0], dtype=torch.uint8, device=occs.device)
    check(lib().dsu_occgrid_binarize(ptr(occs, torch.float32), occs.shape[0], float(thre),
                                     ptr(out), stream()), "dsu_occgrid_binarize")
    return out


# ------------------------------------------------------------------ style translator
ACT = {"none": 0, None: 0, "relu": 1, "leaky_relu": 2, "tanh": 3}


def ric_offsets(H, W, device):
    out = torch.empty((18, H, W), dtype=torch.float32, device=device)
    check(lib().dsu_ric_offsets(H, W, ptr(out), stream()), "dsu_ric_offsets")
    return out


def deform_conv3x3(x, offset, weight, ep_scale=None, ep_shift=None, act=None, residual=None,
                   in_relu=False):
    """offset: (18,H,W) shared by the batch, or (B,18,H,W)."""
    x, weight, offset = _f32c(x), _f32c(weight), _f32c(offset)
    B, Cin, H, W = x.shape
    O = weight.shape[0]
    assert weight.shape[1:] == (Cin, 3, 3), "dsu deform conv: 3x3, groups=1 only"
    bstride = 0 if offset.dim() == 3 or offset.shape[0] == 1 else 18 * H * W
    out = torch.empty((B, O, H, W), dtype=torch.float32, device=x.device)
    check(lib().dsu_deform_conv3x3_fwd(ptr(x), ptr(offset), bstride, ptr(weight), B, Cin, H, W, O,
                                       int(in_relu), ptr(ep_scale), ptr(ep_shift), ACT[act],
                                       ptr(residual), ptr(out), stream()),
          "dsu_deform_conv3x3_fwd")
    return out


def conv2d(x, weight, bias=None, stride=1, padding=0, ep_scale=None, ep_shift=None, act=None,
           residual=None, in_relu=False):
    x, weight = _f32c(x), _f32c(weight)
    B, Cin, H, W = x.shape
    O, Cw, k, k2 = weight.shape
    assert Cw == Cin and k == k2
    OH = (H + 2 * padding - k) // stride + 1
    OW = (W + 2 * padding - k) // stride + 1
    out = torch.empty((B, O, OH, OW), dtype=torch.float32, device=x.device)
    check(lib().dsu_conv2d_fwd(ptr(x), ptr(weight), ptr(bias), B, Cin, H, W, O, k, stride,
                               padding, int(in_relu), ptr(ep_scale), ptr(ep_shift), ACT[act],
                               ptr(residual),
                               ptr(out), stream()), "dsu_conv2d_fwd")
    return out


class PackedConvWeight:
    """A convolution weight in the layout the evaluation kernels read, built on the device once per
    weight version: split into bf16 hi/mid parts (dsu_conv_x3_pack_weights; bf16 x 3 kernels) or,
    with exact=True, as f32 (dsu_conv_f32p_pack_weights; exact-f32 kernels)."""

    def __init__(self, weight, exact=False):
        weight = _f32c(weight.detach())
        self.O, self.C, self.k, k2 = weight.shape
        assert self.k == k2
        self.exact = bool(exact)
        self.C8 = (self.C + 7) & ~7      # the kernels read channels in groups of eight
        n = int(lib().dsu_conv_x3_packed_elems(self.O, self.C, self.k))
        if n <= 0:
            raise DsuError("dsu_conv_x3_packed_elems: unsupported shape")
        if self.exact:
            self.f32 = torch.empty(n, dtype=torch.float32, device=weight.device)
            check(lib().dsu_conv_f32p_pack_weights(ptr(weight), self.O, self.C, self.k,
                                                   ptr(self.f32), stream()),
                  "dsu_conv_f32p_pack_weights")
            return
        self.hi = torch.empty(n, dtype=torch.int16, device=weight.device)
        self.mid = torch.empty(n, dtype=torch.int16, device=weight.device)
        check(lib().dsu_conv_x3_pack_weights(ptr(weight), self.O, self.C, self.k, ptr(self.hi),
                                             ptr(self.mid), stream()), "dsu_conv_x3_pack_weights")


def cat_channels8(tensors):
    """torch.cat(tensors, 1) with zero channels appended up to a multiple of eight (what the
    bf16 x 3 kernels read; the packed weights of those channels are zero)."""
    c = sum(t.shape[1] for t in tensors)
    if c % 8:
        t0 = tensors[0]
        z = torch.zeros((t0.shape[0], 8 - c % 8) + tuple(t0.shape[2:]), dtype=t0.dtype,
                        device=t0.device)
        tensors = tuple(tensors) + (z,)
    return torch.cat(tensors, 1)


def _channels8(x, packed):
    if x.shape[1] == packed.C8:
        return x
    assert x.shape[1] == packed.C, (x.shape, packed.C)
    return cat_channels8((x,))


def deform_conv3x3_x3(x, offset, packed, ep_scale=None, ep_shift=None, act=None, residual=None,
                      in_relu=False):
    """deform_conv3x3 with a PackedConvWeight: bf16 x 3 products with f32 accumulation, or — for a
    weight packed with exact=True — exact f32 products (dsu_deform_conv3x3_fwd_f32p)."""
    x, offset = _channels8(_f32c(x), packed), _f32c(offset)
    B, Cin, H, W = x.shape
    assert packed.k == 3, "dsu deform conv: 3x3, groups=1 only"
    bstride = 0 if offset.dim() == 3 or offset.shape[0] == 1 else 18 * H * W
    out = torch.empty((B, packed.O, H, W), dtype=torch.float32, device=x.device)
    if packed.exact:
        check(lib().dsu_deform_conv3x3_fwd_f32p(ptr(x), ptr(offset), bstride, ptr(packed.f32), B, Cin,
                                                H, W, packed.O, int(in_relu), ptr(ep_scale),
                                                ptr(ep_shift), ACT[act], ptr(residual), ptr(out),
                                                stream()), "dsu_deform_conv3x3_fwd_f32p")
        return out
    check(lib().dsu_deform_conv3x3_fwd_x3(ptr(x), ptr(offset), bstride, ptr(packed.hi),
                                          ptr(packed.mid), B, Cin, H, W, packed.O, int(in_relu),
                                          ptr(ep_scale), ptr(ep_shift), ACT[act], ptr(residual),
                                          ptr(out), stream()), "dsu_deform_conv3x3_fwd_x3")
    return out


def conv2d_x3(x, packed, bias=None, stride=1, padding=0, ep_scale=None, ep_shift=None, act=None,
              residual=None, in_relu=False):
    """conv2d with a PackedConvWeight: bf16 x 3 products with f32 accumulation, or — for a weight
    packed with exact=True — exact f32 products (dsu_conv2d_fwd_f32p; k in {1, 3})."""
    x = _channels8(_f32c(x), packed)
    B, Cin, H, W = x.shape
    k = packed.k
    OH = (H + 2 * padding - k) // stride + 1
    OW = (W + 2 * padding - k) // stride + 1
    out = torch.empty((B, packed.O, OH, OW), dtype=torch.float32, device=x.device)
    if packed.exact:
        check(lib().dsu_conv2d_fwd_f32p(ptr(x), ptr(packed.f32), ptr(bias), B, Cin, H, W, packed.O,
                                        k, stride, padding, int(in_relu), ptr(ep_scale),
                                        ptr(ep_shift), ACT[act], ptr(residual), ptr(out), stream()),
              "dsu_conv2d_fwd_f32p")
        return out
    check(lib().dsu_conv2d_fwd_x3(ptr(x), ptr(packed.hi), ptr(packed.mid), ptr(bias), B, Cin, H, W,
                                  packed.O, k, stride, padding, int(in_relu), ptr(ep_scale),
                                  ptr(ep_shift), ACT[act], ptr(residual), ptr(out), stream()),
          "dsu_conv2d_fwd_x3")
    return out


# ------------------------------------------------------------------ style translator: training
class DeformPlan:
    """Everything the fixed-offset deformable convolution needs besides the weights, for one
    (18,H,W) offset map: the per-(pixel, tap) sampling table (dsu_deform_tap_table) and its
    transpose as CSR over input pixels (built once on the host from that table)."""

    def __init__(self, offset):
        offset = _f32c(offset)
        assert offset.dim() == 3 and offset.shape[0] == 18
        self.offset = offset
        _, H, W = offset.shape
        self.H, self.W, self.npix = H, W, H * W
        nbytes = int(lib().dsu_deform_tap_table_bytes(H, W))
        self.table = torch.empty(nbytes, dtype=torch.uint8, device=offset.device)
        check(lib().dsu_deform_tap_table(ptr(offset), H, W, ptr(self.table), stream()),
              "dsu_deform_tap_table")
        rowptr, src, wgt = transpose_tap_table(self.table.cpu().numpy(), self.npix)
        dev = offset.device
        self.rowptr = torch.from_numpy(rowptr).to(dev)
        self.src = torch.from_numpy(src).to(dev)
        self.wgt = torch.from_numpy(wgt).to(dev)


def transpose_tap_table(table_bytes, npix):
    """(npix*9 records of 4 int32 corner offsets + 4 f32 weights) -> CSR over input pixels:
    rowptr (npix+1) int32, src = tap*npix + output_pixel int32, wgt f32.  Zero-weight corners
    (outside the image) are dropped; entries of a row keep (pixel, tap, corner) order."""
    import numpy as np
    rec = np.frombuffer(table_bytes, dtype=np.int32).reshape(npix * 9, 8)
    idx = rec[:, :4].reshape(-1)                                  # (npix*9*4,)
    w = rec[:, 4:].copy().view(np.float32).reshape(-1)
    pt = np.repeat(np.arange(npix * 9, dtype=np.int64), 4)        # record index = pix*9 + tap
    pix, tap = pt // 9, pt % 9
    keep = w != 0.0
    idx, w, srcv = idx[keep].astype(np.int64), w[keep], (tap * npix + pix)[keep]
    order = np.argsort(idx, kind="stable")
    counts = np.bincount(idx, minlength=npix)
    rowptr = np.zeros(npix + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(counts)
    return rowptr, srcv[order].astype(np.int32), w[order].astype(np.float32)


_DEFORM_PLANS = {}


def deform_plan(offset):
    """Cached DeformPlan for an offset map (keyed by storage, shape and device)."""
    key = (offset.data_ptr(), tuple(offset.shape), str(offset.device))
    plan = _DEFORM_PLANS.get(key)
    if plan is None:
        plan = DeformPlan(offset)
        _lib.publish_sync(offset.device)
        _DEFORM_PLANS[key] = plan
    return plan


def conv2d_wgrad(x, dout, k, stride=1, padding=0, plan=None, out=None, accumulate=False):
    """dW of nn.Conv2d, or of the fixed-offset deformable convolution when plan is given."""
    x, dout = _f32c(x), _f32c(dout)
    B, Cin, H, W = x.shape
    O, OH, OW = dout.shape[1], dout.shape[2], dout.shape[3]
    nbytes = int(lib().dsu_conv2d_wgrad_workspace_bytes(1 if plan is not None else 0, B, Cin, O,
                                                        OH, OW, k))
    if nbytes <= 0:
        raise DsuError("dsu_conv2d_wgrad_workspace_bytes: unsupported shape")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    dw = out if out is not None else torch.empty((O, Cin, k, k), dtype=torch.float32,
                                                 device=x.device)
    check(lib().dsu_conv2d_wgrad(ptr(x), ptr(dout), ptr(plan.table) if plan is not None else None,
                                 B, Cin, H, W, O, k, stride, padding, ptr(ws), ptr(dw),
                                 int(accumulate), stream()), "dsu_conv2d_wgrad")
    return dw


def conv2d_dgrad(dout, weight, in_hw, stride=1, padding=0):
    """dX of nn.Conv2d: the forward kernel on (zero-dilated, for stride > 1) dout with the
    spatially flipped, channel-transposed weight and padding k-1-p."""
    O, Cin, k, _ = weight.shape
    H, W = in_hw
    wt = weight.flip(2, 3).transpose(0, 1).contiguous()
    dout = _f32c(dout)
    if stride != 1:
        B, _, OH, OW = dout.shape
        d = torch.zeros((B, O, H - k + 1 + 2 * padding, W - k + 1 + 2 * padding),
                        dtype=torch.float32, device=dout.device)
        d[:, :, ::stride, ::stride][:, :, :OH, :OW] = dout
        dout = d
    dx = conv2d(dout, wt, None, 1, k - 1 - padding)
    assert tuple(dx.shape[2:]) == (H, W), (dx.shape, in_hw)
    return dx


def deform_conv3x3_dgrad(dout, weight, plan):
    """dX of the fixed-offset deformable convolution: dcol = W^T dout (1x1 convolution), then
    the transposed sampling operator as a gather."""
    dout = _f32c(dout)
    B, O, H, W = dout.shape
    Cin = weight.shape[1]
    wt = weight.permute(1, 2, 3, 0).reshape(Cin * 9, O, 1, 1).contiguous()
    dcol = conv2d(dout, wt, None, 1, 0)
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=dout.device)
    check(lib().dsu_deform_conv3x3_dgrad_gather(ptr(dcol), ptr(plan.rowptr), ptr(plan.src),
                                                ptr(plan.wgt), B * Cin, H * W, ptr(dx), stream()),
          "dsu_deform_conv3x3_dgrad_gather")
    return dx


def _norm_cfg(x, instance, act, eps, momentum, stat_updates):
    B, Cn = x.shape[0], x.shape[1]
    return NormCfg(B, Cn, x[0, 0].numel(), int(instance), ACT[act], int(stat_updates), float(eps),
                   float(momentum))


def norm_train_fwd(x, gamma=None, beta=None, running_mean=None, running_var=None, instance=False,
                   act=None, eps=1e-5, momentum=0.1, stat_updates=1):
    """BatchNorm2d (training) / InstanceNorm2d + activation.  Returns y, save_mean, save_invstd."""
    x = _f32c(x)
    cfg = _norm_cfg(x, instance, act, eps, momentum, stat_updates)
    groups = x.shape[0] * x.shape[1] if instance else x.shape[1]
    y = torch.empty_like(x)
    stats = torch.empty((2, groups), dtype=torch.float32, device=x.device)
    check(lib().dsu_norm_train_fwd(C.byref(cfg), ptr(x), ptr(gamma), ptr(beta), ptr(running_mean),
                                   ptr(running_var), ptr(y), ptr(stats[0]), ptr(stats[1]),
                                   stream()), "dsu_norm_train_fwd")
    return y, stats[0], stats[1]


def norm_train_bwd(x, y, dy, gamma, save_mean, save_invstd, instance=False, act=None,
                   affine_grads=True):
    x, y, dy = _f32c(x), _f32c(y), _f32c(dy)
    cfg = _norm_cfg(x, instance, act, 0.0, 0.0, 0)
    dx = torch.empty_like(x)
    dgb = None
    if affine_grads and not instance:
        dgb = torch.empty((2, x.shape[1]), dtype=torch.float32, device=x.device)
    check(lib().dsu_norm_train_bwd(C.byref(cfg), ptr(x), ptr(y), ptr(dy), ptr(gamma),
                                   ptr(save_mean), ptr(save_invstd), ptr(dx),
                                   ptr(dgb[0]) if dgb is not None else None,
                                   ptr(dgb[1]) if dgb is not None else None, stream()),
          "dsu_norm_train_bwd")
    return (dx, dgb[0], dgb[1]) if dgb is not None else (dx, None, None)


def channel_sum(x):
    x = _f32c(x)
    B, Cn = x.shape[0], x.shape[1]
    out = torch.empty(Cn, dtype=torch.float32, device=x.device)
    check(lib().dsu_channel_sum(ptr(x), B, Cn, x[0, 0].numel(), ptr(out), stream()),
          "dsu_channel_sum")
    return out


def act_fwd(x, act):
    x = _f32c(x)
    y = torch.empty_like(x)
    check(lib().dsu_act_fwd(ptr(x), ptr(y), x.numel(), ACT[act], stream()), "dsu_act_fwd")
    return y


def act_bwd(dy, y, act):
    dy, y = _f32c(dy), _f32c(y)
    dx = torch.empty_like(y)
    check(lib().dsu_act_bwd(ptr(dy), ptr(y), ptr(dx), y.numel(), ACT[act], stream()), "dsu_act_bwd")
    return dx


def maxpool2_fwd(x):
    x = _f32c(x)
    B, Cn, H, W = x.shape
    y = torch.empty((B, Cn, H // 2, W // 2), dtype=torch.float32, device=x.device)
    check(lib().dsu_maxpool2_fwd(ptr(x), ptr(y), B * Cn, H, W, stream()), "dsu_maxpool2_fwd")
    return y


def maxpool2_bwd(x, dy):
    x, dy = _f32c(x), _f32c(dy)
    B, Cn, H, W = x.shape
    dx = torch.empty_like(x)
    check(lib().dsu_maxpool2_bwd(ptr(x), ptr(dy), ptr(dx), B * Cn, H, W, stream()),
          "dsu_maxpool2_bwd")
    return dx


def upsample2_fwd(x):
    x = _f32c(x)
    B, Cn, H, W = x.shape
    y = torch.empty((B, Cn, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    check(lib().dsu_upsample2_fwd(ptr(x), ptr(y), B * Cn, H, W, stream()), "dsu_upsample2_fwd")
    return y


def upsample2_bwd(dy):
    dy = _f32c(dy)
    B, Cn, H2, W2 = dy.shape
    dx = torch.empty((B, Cn, H2 // 2, W2 // 2), dtype=torch.float32, device=dy.device)
    check(lib().dsu_upsample2_bwd(ptr(dy), ptr(dx), B * Cn, H2 // 2, W2 // 2, stream()),
          "dsu_upsample2_bwd")
    return dx


def pair_loss(x, target, kind, grad_scale=None):
    """kind 'l1' | 'mse'; target: tensor like x or a float.  Returns (sum of |d| or d^2 as a
    0-dim tensor, grad or None) with grad = d(grad_scale * sum)/dx."""
    x = _f32c(x)
    t = _f32c(target) if torch.is_tensor(target) else None
    tconst = 0.0 if t is not None else float(target)
    partial = torch.empty(256, dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x) if grad_scale is not None else None
    check(lib().dsu_pair_loss(ptr(x), ptr(t), tconst, x.numel(), {"l1": 0, "mse": 1}[kind],
                              float(grad_scale or 0.0), ptr(grad), ptr(partial), stream()),
          "dsu_pair_loss")
    return partial.sum(), grad


# ------------------------------------------------------------------ multi-view attention
def _i64x3(a, b, c):
    return (C.c_int64 * 3)(int(a), int(b), int(c))


def mv_attention(q, k, vt, seg_batch, heads, seg_len, scale=None):
    """q (Bq,Nq,H*d) f16; k (Bk,Nk,H*d) f16; vt (Bk,H*d,Nk) f16 (V transposed);
    seg_batch (Bq,S) int32: batch index of each seg_len-token K/V segment of query batch b.
    Returns (Bq,Nq,H*d) f16."""
    Bq, Nq, Cq = q.shape
    d = Cq // heads
    S = seg_batch.shape[1]
    assert q.dtype == torch.float16 and k.dtype == torch.float16 and vt.dtype == torch.float16
    # unit stride on the innermost axis (a size-1 axis keeps whatever stride its view had)
    assert q.stride(2) == 1 and k.stride(2) == 1 and (vt.stride(2) == 1 or vt.shape[2] == 1)
    out = torch.empty((Bq, Nq, Cq), dtype=torch.float16, device=q.device)
    if scale is None:
        scale = d ** -0.5
    check(lib().dsu_mv_attention_fwd(
        C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(vt.data_ptr()), ptr(out),
        ptr(seg_batch, torch.int32), Bq, heads, Nq, d, S, int(seg_len),
        _i64x3(q.stride(0), q.stride(1), d), _i64x3(k.stride(0), k.stride(1), d),
        _i64x3(vt.stride(0), d * vt.stride(1), vt.stride(1)),
        _i64x3(out.stride(0), out.stride(1), d), float(scale), stream()), "dsu_mv_attention_fwd")
    return out


# ------------------------------------------------------------------ f16 NHWC convolution
def conv_weight_okc(weight):
    """(O,C,k,k) nn.Conv2d weight -> (O,k*k,C) f16 contiguous (K ordered tap-major)."""
    O, Cin, k, _ = weight.shape
    return weight.detach().permute(0, 2, 3, 1).reshape(O, k * k, Cin).to(torch.float16).contiguous()


_TILE_COUNTERS = {}
_N_TILE_COUNTERS = 1 << 16
import os as _os
SPLITK_FIXUP = _os.environ.get("DSU_SPLITK_FIXUP", "0") == "1"   # in-kernel split-K fix-up instead of the separate reduce launch (A/B)


def _tile_counters(device):
    """Zeroed, persistent per (device, stream) int32 buffer for the in-kernel split-K fix-up (the
    kernel resets what it touches; launches that share a buffer must share a stream).  Only when
    SPLITK_FIXUP is set (tests / tools; off in the product): the device-scope release / acquire
    around the ticket writes back and invalidates the XCD's L2 per workgroup — the UNet forward
    took 26.6 ms with it against 12.6 ms with the separate reduce launches
    (profiles/round3_unet_splitk_fixup.txt)."""
    if not SPLITK_FIXUP:
        return None
    key = (str(device), stream().value)
    t = _TILE_COUNTERS.get(key)
    if t is None:
        t = _TILE_COUNTERS[key] = torch.zeros(_N_TILE_COUNTERS, dtype=torch.int32, device=device)
    return t


def conv2d_nhwc_f16(x_nhwc, w_okc, bias=None, k=3, stride=1, pad=1, upsample2x=False, addvec=None,
                    residual=None, split_k=None):
    """x_nhwc (B,H,W,C) f16 contiguous -> (B,OH,OW,O) f16.  split_k None = the library's choice
    (1 unless the output tiles alone leave most CUs idle), or an explicit factor."""
    B, H, W, Cin = x_nhwc.shape
    O = w_okc.shape[0]
    assert w_okc.shape[1] == k * k and w_okc.shape[2] == Cin
    IH, IW = (2 * H, 2 * W) if upsample2x else (H, W)
    OH, OW = (IH + 2 * pad - k) // stride + 1, (IW + 2 * pad - k) // stride + 1
    out = torch.empty((B, OH, OW, O), dtype=torch.float16, device=x_nhwc.device)
    f16 = torch.float16
    up = int(upsample2x)
    if split_k is None:
        split_k = int(lib().dsu_conv2d_nhwc_f16_split_k(B, H, W, Cin, O, k, stride, pad, up))
    ws, wbytes = None, 0
    if split_k > 1:
        wbytes = int(lib().dsu_conv2d_nhwc_f16_workspace_bytes(B, H, W, O, k, stride, pad, up,
                                                               split_k))
        ws = torch.empty(wbytes // 4, dtype=torch.float32, device=x_nhwc.device)
    cnt = _tile_counters(x_nhwc.device) if split_k > 1 else None
    check(lib().dsu_conv2d_nhwc_f16_fwd_fx(ptr(x_nhwc, f16), ptr(w_okc, f16), ptr(bias, f16), B, H,
                                           W, Cin, O, k, stride, pad, up, ptr(addvec, f16),
                                           ptr(residual, f16), ptr(out), int(split_k), ptr(ws),
                                           wbytes, ptr(cnt), _N_TILE_COUNTERS if cnt is not None else 0,
                                           stream()), "dsu_conv2d_nhwc_f16_fwd_fx")
    return out


def linear_f16(x, weight, bias=None, residual=None, transposed_tokens=0, split_k=None):
    """nn.Linear on the hand-written MFMA kernel.  x (..., K) f16 contiguous, weight (N, K) f16,
    residual (..., N) added last.  transposed_tokens = T > 0: x is (B, T, K) and the result is
    (B, N, T) (V^T for mv_attention).  Returns (..., N) f16."""
    K = x.shape[-1]
    N = weight.shape[0]
    M = x.numel() // K
    f16 = torch.float16
    assert x.dtype == f16 and weight.dtype == f16 and x.is_contiguous() and weight.is_contiguous()
    if transposed_tokens:
        out = torch.empty((M // transposed_tokens, N, transposed_tokens), dtype=f16, device=x.device)
        split_k = 1
    else:
        out = torch.empty(x.shape[:-1] + (N,), dtype=f16, device=x.device)
    if split_k is None:
        split_k = int(lib().dsu_gemm_f16_split_k(M, K, N))
    ws, wbytes = None, 0
    if split_k > 1:
        wbytes = int(lib().dsu_gemm_f16_workspace_bytes(M, N, split_k))
        ws = torch.empty(wbytes // 4, dtype=torch.float32, device=x.device)
    if residual is not None:
        assert residual.is_contiguous() and residual.numel() == M * N
    cnt = _tile_counters(x.device) if split_k > 1 else None
    check(lib().dsu_gemm_f16_fwd_fx(ptr(x, f16), ptr(weight, f16), ptr(bias, f16), M, K, N,
                                    ptr(residual, f16), ptr(out), int(transposed_tokens), int(split_k),
                                    ptr(ws), wbytes, ptr(cnt),
                                    _N_TILE_COUNTERS if cnt is not None else 0, stream()),
          "dsu_gemm_f16_fwd_fx")
    return out


def linear_geglu_f16(x, weight, bias=None):
    """FeedForward's first layer + GEGLU: x (..., K), weight (2N, K), bias (2N) -> (..., N)."""
    K = x.shape[-1]
    N = weight.shape[0] // 2
    M = x.numel() // K
    f16 = torch.float16
    assert x.dtype == f16 and weight.dtype == f16 and x.is_contiguous() and weight.is_contiguous()
    out = torch.empty(x.shape[:-1] + (N,), dtype=f16, device=x.device)
    check(lib().dsu_gemm_geglu_fwd(ptr(x, f16), ptr(weight, f16), ptr(bias, f16), M, K, N, ptr(out),
                                   stream()), "dsu_gemm_geglu_fwd")
    return out


# ------------------------------------------------------------------ norms / activations (f16)
def groupnorm_nhwc_f16(x, gamma, beta, groups, eps=1e-5, silu=False):
    """x (B,H,W,C) or (B,HW,C) f16 contiguous."""
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    out = torch.empty_like(x)
    ws = torch.empty(B * groups * 2, dtype=torch.float32, device=x.device)
    f16 = torch.float16
    check(lib().dsu_groupnorm_nhwc_f16(ptr(x, f16), ptr(gamma, f16), ptr(beta, f16), B, HW, Cc,
                                       groups, float(eps), int(silu), ptr(ws), ptr(out), stream()),
          "dsu_groupnorm_nhwc_f16")
    return out


def layernorm_f16(x, gamma, beta, eps=1e-5):
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    out = torch.empty_like(x)
    f16 = torch.float16
    check(lib().dsu_layernorm_f16(ptr(x, f16), ptr(gamma, f16), ptr(beta, f16), rows, Cc,
                                  float(eps), ptr(out), stream()), "dsu_layernorm_f16")
    return out


def geglu_f16(h):
    D = h.shape[-1] // 2
    rows = h.numel() // (2 * D)
    out = torch.empty(h.shape[:-1] + (D,), dtype=torch.float16, device=h.device)
    check(lib().dsu_geglu_f16(ptr(h, torch.float16), rows, D, ptr(out), stream()), "dsu_geglu_f16")
    return out


# ------------------------------------------------------------------ classifier-free guidance (mv pipeline)
def cfg_model_input(latents, image_latents):
    """latents, image_latents (B,C,h,w) f16 -> the guided UNet input (2B,2C,h,w):
    rows 0..B-1 [latents | 0], rows B..2B-1 [latents | image_latents]."""
    assert latents.dim() == 4 and latents.shape == image_latents.shape
    B, Cc, h, w = latents.shape
    f16 = torch.float16
    out = torch.empty((2 * B, 2 * Cc, h, w), dtype=f16, device=latents.device)
    check(lib().dsu_cfg_model_input(ptr(latents, f16), ptr(image_latents, f16), B, Cc * h * w,
                                    ptr(out), stream()), "dsu_cfg_model_input")
    return out


def ddim_cfg_step(noise_pred, latents, variance_noise, guidance_scale, sqrt_a_t, sqrt_1m_a_t,
                  sqrt_a_prev, std):
    """noise_pred (2B,C,h,w) f16 (unconditional rows first), latents (B,C,h,w) f16, variance_noise
    (B,C,h,w) f16 or None -> the next latents (B,C,h,w) f16: guidance u + g (c - u) and the DDIM
    step (epsilon prediction) in double, rounded to f16 once (include/dsu_hip.h has the rule)."""
    assert noise_pred.shape == (2 * latents.shape[0],) + tuple(latents.shape[1:])
    assert variance_noise is None or variance_noise.shape == latents.shape
    f16 = torch.float16
    out = torch.empty_like(latents, memory_format=torch.contiguous_format)
    check(lib().dsu_ddim_cfg_step(ptr(noise_pred, f16), ptr(latents, f16), ptr(variance_noise, f16),
                                  latents.numel(), float(guidance_scale), float(sqrt_a_t),
                                  float(sqrt_1m_a_t), float(sqrt_a_prev), float(std), ptr(out),
                                  stream()), "dsu_ddim_cfg_step")
    return out


# ------------------------------------------------------------------ fused NeuS shading / compositing
def shade_prep_fwd(grad, feature):
    grad, feature = _f32c(grad), _f32c(feature)
    n = grad.shape[0]
    normal = torch.empty((n, 3), dtype=torch.float32, device=grad.device)
    tex_in = torch.empty((n, 16), dtype=torch.float32, device=grad.device)
    check(lib().dsu_shade_prep_fwd(ptr(grad), ptr(feature), n, ptr(normal), ptr(tex_in), stream()),
          "dsu_shade_prep_fwd")
    return normal, tex_in


def shade_prep_bwd(grad, d_normal, d_tex_in, out=None):
    """out = (d_grad (n,3), d_feat (n,13)) preallocated contiguous f32 (e.g. row prefixes of the
    buffers the geometry backward consumes)."""
    grad = _f32c(grad)
    n = grad.shape[0]
    if out is None:
        d_grad = torch.empty((n, 3), dtype=torch.float32, device=grad.device)
        d_feat = torch.empty((n, 13), dtype=torch.float32, device=grad.device)
    else:
        d_grad, d_feat = out
        assert d_grad.shape == (n, 3) and d_feat.shape == (n, 13)
    dn = None if d_normal is None else _f32c(d_normal)
    check(lib().dsu_shade_prep_bwd(ptr(grad), ptr(dn), ptr(_f32c(d_tex_in)), n, ptr(d_grad),
                                   ptr(d_feat), stream()), "dsu_shade_prep_bwd")
    return d_grad, d_feat


def neus_composite_fwd(sdf, normal, rgb, rays_d, t_starts, t_ends, offsets, counts, inv_s, car):
    n, n_rays = sdf.shape[0], rays_d.shape[0]
    dev = sdf.device
    alpha = torch.empty(n, dtype=torch.float32, device=dev)
    w = torch.empty(n, dtype=torch.float32, device=dev)
    comp = torch.empty((n_rays, 8), dtype=torch.float32, device=dev)
    check(lib().dsu_neus_composite_fwd(ptr(_f32c(sdf)), ptr(_f32c(normal)), ptr(_f32c(rgb)),
                                       ptr(_f32c(rays_d)), ptr(_f32c(t_starts)), ptr(_f32c(t_ends)),
                                       ptr(offsets, torch.int32), ptr(counts, torch.int32), n_rays,
                                       ptr(inv_s, torch.float32), float(car), ptr(alpha), ptr(w),
                                       ptr(comp), stream()), "dsu_neus_composite_fwd")
    return comp, alpha, w


def neus_composite_bwd(sdf, normal, rgb, rays_d, t_starts, t_ends, offsets, counts, inv_s, car,
                       alpha, weights, d_comp, d_weights=None, d_sdf_out=None):
    n, n_rays = sdf.shape[0], rays_d.shape[0]
    dev = sdf.device
    d_sdf = torch.empty(n, dtype=torch.float32, device=dev) if d_sdf_out is None else d_sdf_out
    assert d_sdf.shape == (n,)
    d_normal = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d_rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d_inv = torch.zeros(1, dtype=torch.float32, device=dev)
    dw = None if d_weights is None else _f32c(d_weights)
    check(lib().dsu_neus_composite_bwd(ptr(_f32c(sdf)), ptr(_f32c(normal)), ptr(_f32c(rgb)),
                                       ptr(_f32c(rays_d)), ptr(_f32c(t_starts)), ptr(_f32c(t_ends)),
                                       ptr(offsets, torch.int32), ptr(counts, torch.int32), n_rays,
                                       ptr(inv_s, torch.float32), float(car), ptr(alpha),
                                       ptr(weights), ptr(_f32c(d_comp)), ptr(dw), ptr(d_sdf),
                                       ptr(d_normal), ptr(d_rgb), ptr(d_inv), stream()),
          "dsu_neus_composite_bwd")
    return d_sdf, d_normal, d_rgb, d_inv


def neus_composite_bwd_live(sdf, normal, rgb, rays_d, t_starts, t_ends, offsets, counts, inv_s, car,
                            alpha, weights, d_comp):
    """neus_composite_bwd as the NSR step runs it: also returns the liveness bitmap of the texture
    backward (int32 words, one bit per 32-sample half: some d_rgb of the half is not zero)."""
    n, n_rays = sdf.shape[0], rays_d.shape[0]
    dev = sdf.device
    d_sdf = torch.empty(n, dtype=torch.float32, device=dev)
    d_normal = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d_rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d_inv = torch.zeros(1, dtype=torch.float32, device=dev)
    live = torch.zeros((n + 1023) // 1024, dtype=torch.int32, device=dev)
    check(lib().dsu_neus_composite_bwd_live(ptr(_f32c(sdf)), ptr(_f32c(normal)), ptr(_f32c(rgb)),
                                            ptr(_f32c(rays_d)), ptr(_f32c(t_starts)), ptr(_f32c(t_ends)),
                                            ptr(offsets, torch.int32), ptr(counts, torch.int32), n_rays,
                                            ptr(inv_s, torch.float32), float(car), ptr(alpha),
                                            ptr(weights), ptr(_f32c(d_comp)), None, ptr(d_sdf),
                                            ptr(d_normal), ptr(d_rgb), ptr(d_inv), ptr(live, torch.int32),
                                            stream()),
          "dsu_neus_composite_bwd_live")
    return d_sdf, d_normal, d_rgb, d_inv, live


def texture_live_partition(live_words, n_halves, parts, waves=4):
    """Host only: the runs of 32-sample halves the texture backward gives `parts` workgroups of `waves`
    waves for a liveness bitmap (numpy uint32 words): int32 array (parts, waves, 2) of [first, end)."""
    import numpy as np
    words = np.ascontiguousarray(live_words, dtype=np.uint32)
    assert words.size * 32 >= n_halves
    runs = np.empty((parts, waves, 2), dtype=np.int32)
    check(lib().dsu_texture_live_partition(words.ctypes.data_as(C.c_void_p), int(n_halves), int(parts),
                                           int(waves), runs.ctypes.data_as(C.c_void_p)),
          "dsu_texture_live_partition")
    return runs


# ------------------------------------------------------------------ export: mesh post-processing
class ZGrid:
    """Uniform xy grid over a triangle soup (tris (F,3,3) f32 on the device) for z-parallel ray
    queries, or over a point set (xy (n,2)) for the k-nearest-neighbour search: counting sort by
    cell (csrc/mesh_post.hip)."""

    def __init__(self, data, lo, hi, points=False, cells_per_axis=None):
        import math
        dev = data.device
        n = data.shape[0]
        g = cells_per_axis or int(min(1024, max(8, math.sqrt(max(n, 1) / 2.0))))
        span = max(float(hi[0] - lo[0]), float(hi[1] - lo[1]), 1e-9)
        self.g, self.cell = g, span / g * (1.0 + 1e-6)
        self.x0, self.y0 = float(lo[0]), float(lo[1])
        count_fn = lib().dsu_point_bin_count if points else lib().dsu_zgrid_count
        fill_fn = lib().dsu_point_bin_fill if points else lib().dsu_zgrid_fill
        counts = torch.zeros(g * g, dtype=torch.int32, device=dev)
        check(count_fn(ptr(data, torch.float32), n, self.x0, self.y0, self.cell, g, ptr(counts),
                       stream()), "grid count")
        self.offsets = torch.zeros(g * g + 1, dtype=torch.int32, device=dev)
        self.offsets[1:] = torch.cumsum(counts, 0)
        total = int(self.offsets[-1])
        self.items = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        cursor = torch.zeros(g * g, dtype=torch.int32, device=dev)
        check(fill_fn(ptr(data, torch.float32), n, self.x0, self.y0, self.cell, g, ptr(self.offsets),
                      ptr(cursor), ptr(self.items), stream()), "grid fill")
        self.data = data

    def args(self):
        return (self.x0, self.y0, self.cell, self.g, ptr(self.offsets), ptr(self.items))


def zray_cast(grid, faces_i32, origins, sign, self_vertex=None):
    """mesh_raycast.raycast(origin, (0,0,sign), mesh) for all origins (n,3) f32: returns
    (hit_count i32, t_near, face_near i32, t_far, face_far i32)."""
    origins = _f32c(origins)
    n = origins.shape[0]
    dev = origins.device
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    fn, ff = torch.empty_like(cnt), torch.empty_like(cnt)
    tn, tf = torch.empty(n, device=dev), torch.empty(n, device=dev)
    x0, y0, cell, g, off, items = grid.args()
    check(lib().dsu_zray_cast(ptr(grid.data, torch.float32), ptr(faces_i32, torch.int32),
                              grid.data.shape[0], x0, y0, cell, g, off, items, ptr(origins), n,
                              int(sign), ptr(self_vertex, torch.int32), ptr(cnt), ptr(tn), ptr(fn),
                              ptr(tf), ptr(ff), stream()), "dsu_zray_cast")
    return cnt, tn, fn, tf, ff


def raster_mask(tris, scale, res):
    mask = torch.zeros(res, res, dtype=torch.uint8, device=tris.device)
    check(lib().dsu_raster_mask(ptr(tris, torch.float32), tris.shape[0], float(scale), int(res),
                                ptr(mask), stream()), "dsu_raster_mask")
    return mask


def erode_ellipse_u8(mask, ksize):
    out = torch.empty_like(mask)
    check(lib().dsu_erode_ellipse_u8(ptr(mask, torch.uint8), mask.shape[0], mask.shape[1], int(ksize),
                                     ptr(out), stream()), "dsu_erode_ellipse_u8")
    return out


def knn8_blend(query_xy, known_xy, known_rgb):
    """interpolate_rgb: colours of the 8 nearest known points (xy distance, float64 like scipy's
    cKDTree), weights 1/(d+1e-6)."""
    q64 = query_xy.to(torch.float64).contiguous()
    k64 = known_xy.to(torch.float64).contiguous()
    known_rgb = _f32c(known_rgb)
    k32 = k64.to(torch.float32).contiguous()
    both = torch.cat([q64.to(torch.float32), k32], 0)
    grid = ZGrid(k32, both.amin(0).tolist(), both.amax(0).tolist(), points=True)
    out = torch.empty(q64.shape[0], 3, device=q64.device)
    x0, y0, cell, g, off, items = grid.args()
    check(lib().dsu_knn8_blend(ptr(q64, torch.float64), q64.shape[0], ptr(k64, torch.float64),
                               ptr(known_rgb), k64.shape[0], x0, y0, cell, g, off, items, ptr(out),
                               stream()), "dsu_knn8_blend")
    return out


# ------------------------------------------------------------------ thickness map (animate/rig.py)
THICKNESS_TILE = 16          # samples per side of a workgroup of dsu_mesh_thickness_ortho


def _thickness_lattice(x0, y0, h, W, H):
    x0, y0, h, W, H = float(x0), float(y0), float(h), int(W), int(H)
    side = _lib.DEFINES["DSU_THICKNESS_MAX_SIDE"]
    if not (0 <= W <= side and 0 <= H <= side):
        raise ValueError(f"a thickness lattice has 0 .. {side} samples per side")
    if not (h > 0.0 and all(abs(v) < float("inf") for v in (x0, y0, h))):
        raise ValueError("a thickness lattice needs finite x0, y0 and h > 0")
    return x0, y0, h, W, H


def mesh_thickness(verts, faces, x0, y0, h, W, H):
    """dsu_mesh_thickness_ortho: where along z the inside of the mesh lies under every sample of an xy
    lattice (sample (r, c) at (x0 + (c + 1/2) h, y0 + (r + 1/2) h)).  verts (V,3) f32 and faces (T,3)
    i32 on the device -> (mid (H,W) f64, thickness (H,W) f64, count (H,W) i32); the rule is stated in
    include/dsu_hip.h.  The triangles are binned by ZGrid's counting sort on cells of 16 x 16
    samples, so that a workgroup walks one list."""
    x0, y0, h, W, H = _thickness_lattice(x0, y0, h, W, H)
    verts, faces = _f32c(verts), faces.to(torch.int32).contiguous()
    dev = verts.device
    V, T = verts.shape[0], faces.shape[0]
    mid = torch.zeros((H, W), dtype=torch.float64, device=dev)
    thick = torch.zeros((H, W), dtype=torch.float64, device=dev)
    count = torch.zeros((H, W), dtype=torch.int32, device=dev)
    if not (V and T and W and H):
        return mid, thick, count
    # a face with an index outside [0, V) is ignored by the kernel; it is binned as if it named vertex 0
    tris = verts[faces.long().clamp(0, V - 1)].contiguous()
    g = max(1, -(-max(W, H) // THICKNESS_TILE))
    span = g * THICKNESS_TILE * h
    grid = ZGrid(tris, (x0, y0), (x0 + span, y0 + span), cells_per_axis=g)
    gx0, gy0, cell, g, off, items = grid.args()
    check(lib().dsu_mesh_thickness_ortho(ptr(verts, torch.float32), V, ptr(faces, torch.int32), T, gx0, gy0, cell, g,
                                         off, items, grid.items.shape[0], x0, y0, h, W, H, ptr(mid), ptr(thick),
                                         ptr(count), stream()), "dsu_mesh_thickness_ortho")
    return mid, thick, count


def mesh_thickness_host(verts, faces, x0, y0, h, W, H):
    """dsu_mesh_thickness_ortho_host: mesh_thickness on numpy arrays, without a device."""
    import numpy as np
    x0, y0, h, W, H = _thickness_lattice(x0, y0, h, W, H)
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    mid, thick = np.zeros((H, W), np.float64), np.zeros((H, W), np.float64)
    count = np.zeros((H, W), np.int32)
    p = [a.ctypes.data_as(C.c_void_p) for a in (v, f, mid, thick, count)]
    check(lib().dsu_mesh_thickness_ortho_host(p[0], len(v), p[1], len(f), x0, y0, h, W, H, p[2], p[3], p[4]),
          "dsu_mesh_thickness_ortho_host")
    return mid, thick, count


# ------------------------------------------------------------------ binning of the staged mesh entry points
class _BinnedPlan:
    """The binning half of a staged entry point (csrc/bin_sort.h): stage 0 counts the items per bin
    into the workspace, the prefix sum is taken here (torch), stage 1 fills the ids in.  A subclass
    names its entry point's two stage constants (COUNT, FILL), calls _alloc() from its constructor and
    states its entry point's argument list in _stage()."""
    COUNT = FILL = None

    def _alloc(self, nbytes, name, device):
        if nbytes < 0:
            check(int(nbytes), name)
        self.workspace = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        self.bins = (nbytes // 4 - 1) // 3          # counts (bins) | offsets (bins + 1) | cursor (bins)
        self.items = None

    def _bin_args(self):
        """workspace, workspace_bytes, items, n_items of the entry point."""
        items = self.items
        return (ptr(self.workspace), self.workspace.numel() * 4, ptr(items),
                0 if items is None else items.numel())

    def _stage(self, stage, *args):
        raise NotImplementedError

    def count(self):
        self._stage(self.COUNT)

    def scan(self):
        nb = self.bins
        self.workspace[nb] = 0
        self.workspace[nb + 1:2 * nb + 1] = torch.cumsum(self.workspace[:nb], 0).to(torch.int32)
        return int(self.workspace[2 * nb])

    def fill(self, total):
        self.items = torch.empty(max(total, 1), dtype=torch.int32, device=self.workspace.device)[:total]
        self._stage(self.FILL)

    def bin(self):
        self.count()
        self.fill(self.scan())
        return self


# ------------------------------------------------------------------ frame rendering (csrc/mesh_render.hip)
RENDER_COUNT, RENDER_FILL, RENDER_RASTER = (_lib.DEFINES["DSU_RENDER_" + k] for k in ("COUNT", "FILL", "RASTER"))
MIP_TRILINEAR = "trilinear"
TEXTURE_FILTERS = {k: _lib.DEFINES["DSU_TEX_" + k.upper()] for k in ("nearest", "bilinear", MIP_TRILINEAR)}
# the fourth filter carries a parameter of its own (max_anisotropy), so it is named beside the table
ANISOTROPIC = "anisotropic"
TEX_ANISOTROPIC = _lib.DEFINES["DSU_TEX_ANISOTROPIC"]
MAX_ANISOTROPY = 16
DEFAULT_ANISOTROPY = 8
PYRAMID_FILTERS = (MIP_TRILINEAR, ANISOTROPIC)              # the filters that read the mip pyramid


def check_texture_filter(filter, max_anisotropy=None):
    """Refuses an unknown texture filter, a max_anisotropy outside 1..16 and one given to another filter
    than "anisotropic"; -> the cap as an int (the default for None), or None for the other filters."""
    if filter != ANISOTROPIC:
        if filter not in TEXTURE_FILTERS:
            raise ValueError(f"filter must be one of {sorted([*TEXTURE_FILTERS, ANISOTROPIC])}")
        if max_anisotropy is not None:
            raise ValueError("max_anisotropy goes with filter 'anisotropic'")
        return None
    cap = DEFAULT_ANISOTROPY if max_anisotropy is None else max_anisotropy
    if isinstance(cap, bool) or int(cap) != cap or not 1 <= int(cap) <= MAX_ANISOTROPY:
        raise ValueError(f"max_anisotropy must be an integer in 1..{MAX_ANISOTROPY}")
    return int(cap)


class MeshRenderPlan(_BinnedPlan):
    """The binning half of dsu_mesh_render_ortho for one (screen, faces, window): (frame, triangle)
    pairs counted per 16x16-pixel tile, the prefix sum (torch), the triangle ids filled in.
    screen (F,V,3) f32, faces (M,3) i32 on the device; size a multiple of 4 (<= 2048), ss 1 | 2 | 4.
    halo: the reach of the pixel filter the plan will be rastered with, in sub-samples (0 .. 2 ss;
    animate.pixel_filter gives it with the taps): the tiles are grown by it when the pairs are listed."""
    COUNT, FILL = RENDER_COUNT, RENDER_FILL

    def __init__(self, screen, faces, cx, cy, span, size, ss, halo=0):
        self.screen, self.faces = _f32c(screen), faces.to(torch.int32).contiguous()
        self.halo = int(halo)                         # of the pixel filter, in sub-samples: the tiles grow by it
        if self.screen.dim() != 3 or self.screen.shape[2] != 3 or self.faces.dim() != 2:
            raise ValueError("screen (F,V,3) and faces (M,3) expected")
        self.F, self.V, self.M = self.screen.shape[0], self.screen.shape[1], self.faces.shape[0]
        self.cx, self.cy, self.span = float(cx), float(cy), float(span)
        self.size, self.ss = int(size), int(ss)
        self._alloc(lib().dsu_mesh_render_ortho_workspace_bytes(self.F, self.size),
                    "dsu_mesh_render_ortho_workspace_bytes", self.screen.device)

    def _stage(self, stage, colour=None, pos=None, tex=None, outs=(None,) * 6, taps=None):
        head = (stage, ptr(self.screen, torch.float32), ptr(self.faces, torch.int32), ptr(colour), ptr(pos),
                None if tex is None else C.byref(tex),
                self.F, self.V, self.M, self.cx, self.cy, self.span, self.size, self.ss)
        tail = (*self._bin_args(), *[ptr(o) for o in outs], stream())
        if taps is None and self.halo == 0:           # the unfiltered entry point; its bins are those of halo 0
            check(lib().dsu_mesh_render_ortho(*head, *tail), "dsu_mesh_render_ortho")
        else:                                         # taps: a host table, read at RASTER only
            check(lib().dsu_mesh_render_ortho_filtered(
                *head, None if taps is None else taps.ctypes.data_as(C.c_void_p), self.halo, *tail),
                "dsu_mesh_render_ortho_filtered")

    def raster(self, colour, pos, want=("color_u8", "pos_u8", "frames"), uv=None, texture=None,
               filter="bilinear", pyramid=None, taps=None, max_anisotropy=None):
        """Visibility + resolve.  Returns a dict of the requested outputs among color_u8, pos_u8
        (F,S,S,4) uint8, face_id (F,N,N) i32, depth (F,N,N) f32, frames (F,6,S,S) f32, pixels
        (F,S,S,8) f32.

        With uv (V,2) f32 and texture (T,T,3) or (T,T,4) uint8 (both or neither) the colour of every
        sample comes from the texture (the `tex` of dsu_mesh_render_ortho; filter "bilinear" or
        "nearest") and `colour` may be None; without them this is the vertex-colour call.
        filter "trilinear" reads the texture's mip pyramid: `pyramid`, a
        MipPyramid of this texture from mip_pyramid(), or None to build it here with every texel
        covered and the default gutter.  filter "anisotropic" reads the same pyramid with up to
        max_anisotropy (1..16, default 8) probes per sample along the long axis of the face's footprint
        (include/dsu_hip.h, "Anisotropic frames"); a pyramid built here gets max(2, max_anisotropy)
        gutter rounds.

        taps: None = the box over a pixel's own samples (dsu_mesh_render_ortho); otherwise the
        ss + 2 halo float64 taps of a separable pixel filter (animate.pixel_filter) for the halo this
        plan was binned with (dsu_mesh_render_ortho_filtered)."""
        if self.items is None:
            raise DsuError("MeshRenderPlan.raster before bin()")
        if taps is None:
            if self.halo:
                raise ValueError(f"this plan was binned for a pixel filter of halo {self.halo}: taps are needed")
        else:
            import numpy as np
            taps = np.ascontiguousarray(taps, np.float64).reshape(-1)
            if len(taps) != self.ss + 2 * self.halo:
                raise ValueError(f"{len(taps)} taps do not belong to ss {self.ss} and the halo {self.halo} this plan "
                                 f"was binned with ({self.ss + 2 * self.halo} expected)")
        if (uv is None) != (texture is None) or (texture is None and (filter in PYRAMID_FILTERS or pyramid is not None)):
            raise ValueError("uv and texture come together or not at all (and a trilinear or anisotropic read "
                             "needs both)")
        F, S, N, dev = self.F, self.size, self.size * self.ss, self.screen.device
        shapes = {"color_u8": ((F, S, S, 4), torch.uint8), "pos_u8": ((F, S, S, 4), torch.uint8),
                  "face_id": ((F, N, N), torch.int32), "depth": ((F, N, N), torch.float32),
                  "frames": ((F, 6, S, S), torch.float32), "pixels": ((F, S, S, 8), torch.float32)}
        bad = [w for w in want if w not in shapes]
        if bad:
            raise ValueError(f"unknown outputs {bad}")
        pos = _f32c(pos)
        if pos.shape != (self.V, 3):
            raise ValueError("colour and pos must be (V,3)")
        tex = None
        if texture is None:
            colour = _f32c(colour)
            if colour.shape != (self.V, 3):
                raise ValueError("colour and pos must be (V,3)")
        else:
            cap = check_texture_filter(filter, max_anisotropy)
            uv, texels = _f32c(uv), texture_rgba(texture)
            if uv.shape != (self.V, 2):
                raise ValueError("uv must be (V,2)")
            T = texels.shape[0]
            if filter in PYRAMID_FILTERS:
                if pyramid is None:
                    pyramid = mip_pyramid(texels) if cap is None else mip_pyramid(texels, gutter=max(2, cap))
                if not isinstance(pyramid, MipPyramid) or pyramid.T != T or pyramid.buffer.device != dev:
                    raise ValueError("pyramid must be the MipPyramid of this texture, on the mesh's device")
                texels = pyramid.buffer
            elif pyramid is not None:
                raise ValueError("a pyramid goes with filter 'trilinear' or 'anisotropic'")
            colour = None                             # not read
            if cap is None:
                tex = _lib.RenderTexture(ptr(uv), ptr(texels, torch.uint8), T, TEXTURE_FILTERS[filter])
            else:
                tex = _lib.RenderTexture(ptr(uv), ptr(texels, torch.uint8), T, TEX_ANISOTROPIC, cap)
        out = {k: torch.empty(shp, dtype=dt, device=dev) for k, (shp, dt) in shapes.items() if k in want}
        self._stage(RENDER_RASTER, colour, pos, tex, [out.get(k) for k in shapes], taps)
        return out


def texture_rgba(texture):
    """(T,T,3) or (T,T,4) uint8 on the device -> the contiguous (T,T,4) RGBA8 texture of
    dsu_render_texture (an opaque alpha is added to three channels; four are kept)."""
    if not torch.is_tensor(texture) or texture.dtype != torch.uint8 or texture.dim() != 3 or \
            texture.shape[0] != texture.shape[1] or texture.shape[2] not in (3, 4) or texture.shape[0] < 1:
        raise ValueError("texture (T,T,3) or (T,T,4) uint8 expected")
    if texture.shape[2] == 4:
        return texture.contiguous()
    rgba = torch.full((*texture.shape[:2], 4), 255, dtype=torch.uint8, device=texture.device)
    rgba[..., :3] = texture
    return rgba


class MipPyramid:
    """The mip pyramid of one atlas (dsu_mip_pyramid_build): buffer (dsu_mip_pyramid_texels(T), 4) uint8 on
    the device, T the side of level 0, L the number of levels."""

    def __init__(self, buffer, T, L):
        self.buffer, self.T, self.L = buffer, int(T), int(L)

    def size(self, k):
        """T_k = ceil(T / 2^k)."""
        if not 0 <= k < self.L:
            raise IndexError(f"level {k} of {self.L}")
        return (self.T + (1 << k) - 1) >> k

    def level(self, k):
        """(T_k, T_k, 4) uint8 view of level k."""
        at = sum(self.size(j) ** 2 for j in range(k))
        return self.buffer[at:at + self.size(k) ** 2].view(self.size(k), self.size(k), 4)


def mip_pyramid(texture, covered=None, gutter=2):
    """dsu_mip_pyramid_build (include/dsu_hip.h, "Mip-mapped frames"): texture (T,T,3|4) uint8 on the
    device; covered (T,T) bool / uint8 or None = every texel covered; `gutter` dilation rounds per level
    above 0 -> MipPyramid.  Level 0 is the texture (with an opaque alpha where it had three channels)."""
    rgba = texture_rgba(texture)
    T, dev = rgba.shape[0], rgba.device
    if covered is not None:
        if not torch.is_tensor(covered) or covered.shape != (T, T) or covered.device != dev:
            raise ValueError("covered (T,T) on the texture's device expected")
        covered = covered.to(torch.uint8).contiguous()
    texels = int(lib().dsu_mip_pyramid_texels(T))
    wbytes = int(lib().dsu_mip_workspace_bytes(T))
    if texels < 0 or wbytes < 0:
        check(min(texels, wbytes), "dsu_mip_pyramid_texels")
    buffer = torch.empty((texels, 4), dtype=torch.uint8, device=dev)
    work = torch.empty(max(wbytes, 16), dtype=torch.uint8, device=dev)
    check(lib().dsu_mip_pyramid_build(ptr(rgba, torch.uint8), ptr(covered), T, int(gutter), ptr(buffer), ptr(work),
                                      work.numel(), stream()), "dsu_mip_pyramid_build")
    return MipPyramid(buffer, T, int(lib().dsu_mip_levels(T)))


def mesh_render_ortho(screen, faces, colour, pos, cx, cy, span, size, ss=4,
                      want=("color_u8", "pos_u8", "frames"), uv=None, texture=None, filter="bilinear",
                      pyramid=None, pixel_filter=None, max_anisotropy=None):
    """Orthographic render of F frames of one mesh with two attribute sets (include/dsu_hip.h,
    dsu_mesh_render_ortho): bin, then rasterise and resolve.  The colours are the vertex colours,
    or with uv and texture the texture's (filter "trilinear": its mip `pyramid`, built from the
    texture when None; filter "anisotropic": the same pyramid, up to max_anisotropy probes per sample).
    pixel_filter: None = the box over a pixel's own samples, or the (taps, halo)
    of animate.pixel_filter for this ss (dsu_mesh_render_ortho_filtered)."""
    taps, halo = (None, 0) if pixel_filter is None else pixel_filter
    return MeshRenderPlan(screen, faces, cx, cy, span, size, ss, halo).bin().raster(colour, pos, want, uv, texture,
                                                                                    filter, pyramid, taps,
                                                                                    max_anisotropy)


def pos_edge_u8(pos_rgba):
    """run_render.py's pos2edge, stored inverted: pos_rgba (F,H,W,4) uint8 -> (F,H,W) uint8, 255 =
    no edge, 0 = edge."""
    if pos_rgba.dim() != 4 or pos_rgba.shape[3] != 4:
        raise ValueError("pos_rgba (F,H,W,4) expected")
    F, H, W = pos_rgba.shape[:3]
    out = torch.empty((F, H, W), dtype=torch.uint8, device=pos_rgba.device)
    check(lib().dsu_pos_edge_u8(ptr(pos_rgba, torch.uint8), F, H, W, ptr(out), stream()),
          "dsu_pos_edge_u8")
    return out


# ------------------------------------------------------------------ uv export (csrc/mesh_uv.hip)
UV_COUNT, UV_FILL, UV_RASTER = (_lib.DEFINES["DSU_UV_" + k] for k in ("COUNT", "FILL", "RASTER"))


def uv_face_labels(verts, faces):
    """dsu_uv_face_labels: verts (V,3) f32, faces (M,3) on the device -> normal (M,3) f64, label (M)
    i32 (2 axis + (n_axis < 0), -1 = degenerate), area (M) f64 projected along the axis."""
    verts, faces = _f32c(verts), faces.to(torch.int32).contiguous()
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("verts (V,3) and faces (M,3) expected")
    M, dev = faces.shape[0], verts.device
    normal = torch.empty((M, 3), dtype=torch.float64, device=dev)
    label = torch.empty(M, dtype=torch.int32, device=dev)
    area = torch.empty(M, dtype=torch.float64, device=dev)
    check(lib().dsu_uv_face_labels(ptr(verts, torch.float32), ptr(faces, torch.int32), verts.shape[0], M,
                                   ptr(normal), ptr(label), ptr(area), stream()), "dsu_uv_face_labels")
    return normal, label, area


def face_adjacency(faces):
    """(M,3) i32 on the faces' device: the face across edge (a,b), (b,c), (c,a); -1 on a boundary
    edge and on an edge used by more than two faces (torch sorts: plumbing for dsu_uv_components)."""
    f = faces.to(torch.int64)
    M = f.shape[0]
    if M == 0:
        return torch.empty((0, 3), dtype=torch.int32, device=f.device)
    a, b = f, f[:, [1, 2, 0]]
    nv = int(f.max()) + 1
    key = (torch.minimum(a, b) * nv + torch.maximum(a, b)).reshape(-1)      # slot = 3 face + edge
    skey, order = torch.sort(key, stable=True)
    first = torch.ones_like(skey, dtype=torch.bool)
    first[1:] = skey[1:] != skey[:-1]
    group = torch.cumsum(first.to(torch.int64), 0) - 1
    size = torch.bincount(group)[group]
    pos = torch.arange(len(skey), device=f.device) - torch.nonzero(first).reshape(-1)[group]
    partner = torch.where(pos == 0, torch.roll(order, -1), torch.roll(order, 1))
    adj = torch.full((3 * M,), -1, dtype=torch.int64, device=f.device)
    two = size == 2
    adj[order[two]] = torch.div(partner[two], 3, rounding_mode="floor")
    return adj.reshape(M, 3).to(torch.int32).contiguous()


def uv_components(adjacency, label, check_every=4, max_rounds=1 << 20):
    """dsu_uv_components -> (chart (M) i32: the smallest face index of each face's component,
    rounds launched)."""
    adjacency, label = adjacency.to(torch.int32).contiguous(), label.to(torch.int32).contiguous()
    M, dev = label.shape[0], label.device
    if adjacency.shape != (M, 3):
        raise ValueError("adjacency (M,3) and label (M) expected")
    chart = torch.arange(M, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    rounds = C.c_int32(0)
    check(lib().dsu_uv_components(ptr(adjacency, torch.int32), ptr(label, torch.int32), M, ptr(chart),
                                  ptr(flag), int(check_every), int(max_rounds), C.byref(rounds), stream()),
          "dsu_uv_components")
    return chart, int(rounds.value)


class UvBakePlan(_BinnedPlan):
    """The binning half of dsu_uv_bake for one (uvs, indices, size): faces counted per 16x16-texel
    tile, the prefix sum (torch), the ids filled in.  uvs (V,2) f32, indices (M,3) on the device."""
    COUNT, FILL = UV_COUNT, UV_FILL

    def __init__(self, uvs, indices, size):
        self.uvs, self.indices = _f32c(uvs), indices.to(torch.int32).contiguous()
        if self.uvs.dim() != 2 or self.uvs.shape[1] != 2 or self.indices.dim() != 2 or self.indices.shape[1] != 3:
            raise ValueError("uvs (V,2) and indices (M,3) expected")
        self.V, self.M, self.size = self.uvs.shape[0], self.indices.shape[0], int(size)
        self._alloc(lib().dsu_uv_bake_workspace_bytes(self.size), "dsu_uv_bake_workspace_bytes",
                    self.uvs.device)

    def _stage(self, stage, colours=None, depth=None, outs=(None, None, None)):
        check(lib().dsu_uv_bake(stage, ptr(self.uvs, torch.float32), ptr(self.indices, torch.int32),
                                ptr(colours), ptr(depth), self.V, self.M, self.size, *self._bin_args(),
                                *[ptr(o) for o in outs], stream()), "dsu_uv_bake")

    def raster(self, colours, depth=None):
        """-> image (S,S,3) u8, face_id (S,S) i32, demote (M) u8 (None without depth)."""
        if self.items is None:
            raise DsuError("UvBakePlan.raster before bin()")
        S, dev = self.size, self.uvs.device
        colours = _f32c(colours)
        if colours.shape != (self.V, 3):
            raise ValueError("colours must be (V',3)")
        image = torch.empty((S, S, 3), dtype=torch.uint8, device=dev)
        face_id = torch.empty((S, S), dtype=torch.int32, device=dev)
        demote = None
        if depth is not None:
            depth = depth.to(torch.float64).contiguous()
            if depth.shape != (self.M,):
                raise ValueError("depth must be (M,)")
            demote = torch.empty(self.M, dtype=torch.uint8, device=dev)
        self._stage(UV_RASTER, colours, depth, (image, face_id, demote))
        return image, face_id, demote


def uv_bake(uvs, indices, colours, size, depth=None):
    """dsu_uv_bake (include/dsu_hip.h): bin, then rasterise.  No gutter fill: see uv_dilate."""
    return UvBakePlan(uvs, indices, size).bin().raster(colours, depth)


def uv_dilate(image, covered, rounds):
    """`rounds` launches of dsu_uv_dilate, double-buffered -> (image (S,S,3) u8, covered (S,S) u8)."""
    image, covered = image.contiguous(), covered.to(torch.uint8).contiguous()
    S = image.shape[0]
    if image.shape != (S, S, 3) or covered.shape != (S, S) or image.dtype != torch.uint8:
        raise ValueError("image (S,S,3) uint8 and covered (S,S) expected")
    for _ in range(int(rounds)):
        img2, cov2 = torch.empty_like(image), torch.empty_like(covered)
        check(lib().dsu_uv_dilate(ptr(image, torch.uint8), ptr(covered, torch.uint8), S, ptr(img2), ptr(cov2),
                                  stream()), "dsu_uv_dilate")
        image, covered = img2, cov2
    return image, covered


def uv_project(uvs, indices, positions, face_id, color_front, mask_front, color_back, mask_back,
               z_tolerance, grid=None, cells_per_axis=None):
    """dsu_uv_project (include/dsu_hip.h): which pixel of the front / back drawing every atlas texel
    sees.  uvs (V',2) f32, indices (M,3), positions (V',3) f32 in color_projection's frame, face_id
    (S,S) i32 from uv_bake, color_* (res,res,3) u8 and the eroded masks (res,res) u8, all on the
    device.  `grid`: the ZGrid over positions[indices], built here when absent (`cells_per_axis`
    overrides its resolution).  -> image (S,S,3) u8, source (S,S) u8 (0 none, 1 front, 2 back).
    The kernel is uv_project_area's at one sample; the grid stays ZGrid's default, since the finer one
    of uv_area_cells costs more to build than this one launch gains (profiles/uv_project_unified_probe.json)."""
    return _uv_project(None, uvs, indices, positions, face_id, color_front, mask_front, color_back, mask_back,
                       z_tolerance, grid, cells_per_axis)


def uv_area_cells(n_faces):
    """Cells per axis of the z-grid uv_project_area builds when it is handed none: three times
    ZGrid's default.  The kernel's time goes into the edge functions of the listed triangles at
    every sub-sample, so shorter lists pay: on the ~50 000-face probe mesh 160 / 320 / 480 / 640
    cells give 1470 / 1141 / 977 / 1122 us at s = 4 (tools/uv_project_area_probe.py --cells); the
    result does not depend on the grid."""
    import math
    return int(min(1024, max(8, 3.0 * math.sqrt(max(n_faces, 1) / 2.0))))


UV_PIXEL_FILTERS = ("nearest", "bilinear")             # the `filter` argument of dsu_uv_project_area


def uv_project_area(uvs, indices, positions, face_id, color_front, mask_front, color_back, mask_back,
                    z_tolerance, samples, pixel_filter="nearest", grid=None, cells_per_axis=None):
    """dsu_uv_project_area (include/dsu_hip.h, UV export j.): uv_project with the drawings read at
    samples x samples points per texel (1..8), each at its nearest pixel or bilinearly, and averaged.
    Arguments as uv_project.  -> image (S,S,3) u8, source (S,S) u8, count (S,S) u8: the sub-samples
    that passed (0 with source > 0: the texel's own point decided)."""
    s = int(samples)
    if not 1 <= s <= 8:
        raise ValueError("samples must be 1..8")
    if pixel_filter not in UV_PIXEL_FILTERS:
        raise ValueError("pixel_filter must be 'nearest' or 'bilinear'")
    return _uv_project((s, UV_PIXEL_FILTERS.index(pixel_filter)), uvs, indices, positions, face_id, color_front,
                       mask_front, color_back, mask_back, z_tolerance, grid, cells_per_axis)


def _uv_project(area, uvs, indices, positions, face_id, color_front, mask_front, color_back, mask_back,
                z_tolerance, grid, cells_per_axis):
    """uv_project (area None) and uv_project_area (area = (s, filter)): one preparation of the arguments
    for the two C entries, which launch one kernel."""
    uvs, positions = _f32c(uvs), _f32c(positions)
    indices = indices.to(torch.int32).contiguous()
    V, M, S, dev = uvs.shape[0], indices.shape[0], face_id.shape[0], uvs.device
    if uvs.shape != (V, 2) or positions.shape != (V, 3) or indices.shape != (M, 3) or face_id.shape != (S, S):
        raise ValueError("uvs (V',2), positions (V',3), indices (M,3) and face_id (S,S) expected")
    res = color_front.shape[0]
    for img, shape in ((color_front, (res, res, 3)), (color_back, (res, res, 3)), (mask_front, (res, res)),
                       (mask_back, (res, res))):
        if tuple(img.shape) != shape or img.dtype != torch.uint8:
            raise ValueError("drawings (res,res,3) and masks (res,res) must be uint8 of one resolution")
    if grid is None and M:
        tris = positions[indices.long()].contiguous()
        xy = tris[..., :2].reshape(-1, 2)
        xy = xy[torch.isfinite(xy).all(1)]                   # a non-finite vertex must not set the extent
        lo, hi = (xy.amin(0).tolist(), xy.amax(0).tolist()) if xy.shape[0] else ([0.0, 0.0], [0.0, 0.0])
        if area is not None and cells_per_axis is None:
            cells_per_axis = uv_area_cells(M)
        grid = ZGrid(tris, lo, hi, cells_per_axis=cells_per_axis)
    image = torch.empty((S, S, 3), dtype=torch.uint8, device=dev)
    source = torch.empty((S, S), dtype=torch.uint8, device=dev)
    gargs = (ptr(grid.data, torch.float32),) + grid.args() if M else (None, 0.0, 0.0, 1.0, 1, None, None)
    args = (ptr(uvs), ptr(indices), ptr(positions), V, M, S, ptr(face_id.contiguous(), torch.int32), *gargs,
            ptr(color_front.contiguous()), ptr(mask_front.contiguous()), ptr(color_back.contiguous()),
            ptr(mask_back.contiguous()), res, float(z_tolerance))
    if area is None:
        check(lib().dsu_uv_project(*args, ptr(image), ptr(source), stream()), "dsu_uv_project")
        return image, source
    count = torch.empty((S, S), dtype=torch.uint8, device=dev)
    check(lib().dsu_uv_project_area(*args, area[0], area[1], ptr(image), ptr(source), ptr(count), stream()),
          "dsu_uv_project_area")
    return image, source, count


def uv_field_points(uvs, indices, positions, face_id, texels, samples):
    """dsu_uv_field_points (include/dsu_hip.h): the points at which the field bake evaluates the
    texture field.  uvs (V',2) f32, indices (M,3), positions (V',3) f32 in the field's frame,
    face_id (S,S) i32 from uv_bake, texels (T) i32 linear indices (ascending), all on the device;
    samples: sub-samples per axis, 1..8.  -> points (T, samples^2, 3) f32, valid (T, samples^2) u8."""
    uvs, positions = _f32c(uvs), _f32c(positions)
    indices, texels = indices.to(torch.int32).contiguous(), texels.to(torch.int32).contiguous()
    V, M, S, T, s, dev = uvs.shape[0], indices.shape[0], face_id.shape[0], texels.shape[0], int(samples), uvs.device
    if uvs.shape != (V, 2) or positions.shape != (V, 3) or indices.shape != (M, 3) or face_id.shape != (S, S) or \
            texels.dim() != 1:
        raise ValueError("uvs (V',2), positions (V',3), indices (M,3), face_id (S,S) and texels (T) expected")
    if not 1 <= s <= 8:
        raise ValueError("samples must be 1..8")
    points = torch.empty((T, s * s, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((T, s * s), dtype=torch.uint8, device=dev)
    if T == 0:                                               # empty tensors have no address to hand over
        return points, valid
    check(lib().dsu_uv_field_points(ptr(uvs), ptr(indices), ptr(positions), V, M, S,
                                    ptr(face_id.contiguous(), torch.int32), ptr(texels), T, s, ptr(points),
                                    ptr(valid), stream()), "dsu_uv_field_points")
    return points, valid


def uv_field_resolve(colours, valid, texels, image):
    """dsu_uv_field_resolve (include/dsu_hip.h): the mean of every listed texel's valid samples,
    quantised as uv_bake does, written into image (S,S,3) u8 IN PLACE; a texel without a valid
    sample keeps its bytes.  colours (T, samples^2, 3) f32, valid (T, samples^2) u8, texels (T) i32.
    -> image."""
    colours, texels = _f32c(colours), texels.to(torch.int32).contiguous()
    T, S = texels.shape[0], image.shape[0]
    if colours.dim() != 3 or colours.shape[0] != T or colours.shape[2] != 3 or valid.shape != colours.shape[:2] or \
            image.shape != (S, S, 3) or image.dtype != torch.uint8:
        raise ValueError("colours (T,n,3), valid (T,n), texels (T) and image (S,S,3) uint8 expected")
    s = int(round(colours.shape[1] ** 0.5))
    if s * s != colours.shape[1] or not 1 <= s <= 8:
        raise ValueError("colours must hold samples^2 colours per texel, samples 1..8")
    if T == 0:
        return image
    check(lib().dsu_uv_field_resolve(ptr(colours), ptr(valid.contiguous(), torch.uint8), ptr(texels), T, s, S,
                                     ptr(image, torch.uint8), stream()), "dsu_uv_field_resolve")
    return image


def _uv_seam_args(uvs, indices, group, face_id, source, proj, fallback):
    uvs = _f32c(uvs)
    indices, group = indices.to(torch.int32).contiguous(), group.to(torch.int32).contiguous()
    V, M, S = uvs.shape[0], indices.shape[0], face_id.shape[0]
    if uvs.shape != (V, 2) or indices.shape != (M, 3) or group.shape != (V,) or face_id.shape != (S, S):
        raise ValueError("uvs (V',2), indices (M,3), group (V') and face_id (S,S) expected")
    if face_id.dtype != torch.int32 or source.dtype != torch.uint8 or source.shape != (S, S):
        raise ValueError("face_id (S,S) int32 and source (S,S) uint8 expected")
    for img in (proj, fallback):
        if tuple(img.shape) != (S, S, 3) or img.dtype != torch.uint8:
            raise ValueError("proj and fallback must be (S,S,3) uint8")
    return (uvs, indices, group, face_id.contiguous(), source.contiguous(), proj.contiguous(),
            fallback.contiguous()), (V, M, S)


def uv_seam_gather(uvs, indices, group, face_id, source, proj, fallback, n_groups):
    """dsu_uv_seam_gather (include/dsu_hip.h, UV export h.): the projected texels' differences
    proj - fallback summed per welded vertex group in 64-bit fixed point.  uvs (V',2) f32, indices
    (M,3), group (V') i32 in [0, n_groups), face_id (S,S) i32 from uv_bake, source (S,S) u8 and proj
    (S,S,3) u8 from uv_project, fallback (S,S,3) u8 without gutter fill, all on the device.
    -> num (n_groups,3) i64, den (n_groups) i64."""
    (uvs, indices, group, face_id, source, proj, fallback), (V, M, S) = \
        _uv_seam_args(uvs, indices, group, face_id, source, proj, fallback)
    G = int(n_groups)
    if G < 0:
        raise ValueError("n_groups must not be negative")
    num = torch.zeros((G, 3), dtype=torch.int64, device=uvs.device)
    den = torch.zeros(G, dtype=torch.int64, device=uvs.device)
    if G == 0 or M == 0:                                     # empty tensors have no address to hand over
        return num, den
    check(lib().dsu_uv_seam_gather(ptr(uvs), ptr(indices), ptr(group), V, M, G, S, ptr(face_id), ptr(source),
                                   ptr(proj), ptr(fallback), ptr(num), ptr(den), stream()), "dsu_uv_seam_gather")
    return num, den


def uv_seam_apply(uvs, indices, group, face_id, source, proj, fallback, d):
    """dsu_uv_seam_apply (include/dsu_hip.h, UV export i.): the composed atlas — proj where source is
    set, elsewhere fallback plus the offsets d (G,3) f64 of the face's three groups interpolated with
    the texel's barycentrics, rounded to nearest and clipped.  Arguments as uv_seam_gather.
    -> image (S,S,3) u8."""
    (uvs, indices, group, face_id, source, proj, fallback), (V, M, S) = \
        _uv_seam_args(uvs, indices, group, face_id, source, proj, fallback)
    d = d.to(torch.float64).contiguous()
    if d.dim() != 2 or d.shape[1] != 3:
        raise ValueError("d must be (G,3)")
    G = d.shape[0]
    image = torch.empty((S, S, 3), dtype=torch.uint8, device=uvs.device)
    atlas = M > 0 and G > 0
    check(lib().dsu_uv_seam_apply(ptr(uvs) if atlas else None, ptr(indices) if atlas else None,
                                  ptr(group) if atlas else None, V, M, G, S, ptr(face_id), ptr(source), ptr(proj),
                                  ptr(fallback), ptr(d) if atlas else None, ptr(image), stream()),
          "dsu_uv_seam_apply")
    return image


# ------------------------------------------------------------------ rigging (csrc/mesh_skin.hip)
SKIN_COUNT, SKIN_FILL, SKIN_RUN = (_lib.DEFINES["DSU_SKIN_" + k] for k in ("COUNT", "FILL", "RUN"))


class BoneVisibilityPlan(_BinnedPlan):
    """The binning half of dsu_bone_visibility: the triangles of one mesh counted per cell of a
    uniform 3-D grid over the mesh and the bones, the prefix sum (torch), the ids filled in; and the
    vertex order (by cell) that keeps a workgroup's segments together.
    verts (V,3) f32, faces (M,3) i32, bones (B,2,3) f32 on the device."""
    COUNT, FILL = SKIN_COUNT, SKIN_FILL

    def __init__(self, verts, faces, bones, cells_per_axis=None):
        import math
        self.verts, self.faces = _f32c(verts), faces.to(torch.int32).contiguous()
        self.bones = _f32c(bones)
        if self.verts.dim() != 2 or self.verts.shape[1] != 3 or self.faces.dim() != 2 or \
                self.faces.shape[1] != 3 or self.bones.dim() != 3 or self.bones.shape[1:] != (2, 3):
            raise ValueError("verts (V,3), faces (M,3) and bones (B,2,3) expected")
        self.V, self.M, self.B = self.verts.shape[0], self.faces.shape[0], self.bones.shape[0]
        pts = torch.cat([self.verts, self.bones.reshape(-1, 3)], 0).to(torch.float64)
        lo, hi = pts.amin(0).tolist(), pts.amax(0).tolist()
        ext = [max(h - l, 0.0) for l, h in zip(lo, hi)]
        longest = max(max(ext), 1e-9)
        # about two triangles per occupied cell of a surface: cells ~ sqrt(M / 2) along the longest axis
        n = cells_per_axis or int(min(128, max(4, math.sqrt(max(self.M, 1) / 2.0))))
        self.cell = longest / n * (1.0 + 1e-6)
        self.g = [int(min(256, max(1, math.ceil(e / self.cell)))) for e in ext]
        self.lo = lo
        self._alloc(lib().dsu_bone_visibility_workspace_bytes(*self.g), "dsu_bone_visibility_workspace_bytes",
                    self.verts.device)
        self.cells = self.bins
        c = ((self.verts.to(torch.float64) - pts.new_tensor(lo)) / self.cell).floor().to(torch.int64)
        c = torch.minimum(c.clamp_(min=0), torch.tensor(self.g, device=c.device) - 1)
        key = (c[:, 2] * self.g[1] + c[:, 1]) * self.g[0] + c[:, 0]
        self.order = torch.argsort(key, stable=True).to(torch.int32).contiguous()

    def _stage(self, stage, dist=None, visible=None):
        check(lib().dsu_bone_visibility(
            stage, ptr(self.verts, torch.float32), ptr(self.faces, torch.int32), ptr(self.bones, torch.float32),
            self.V, self.M, self.B, ptr(self.order, torch.int32), self.lo[0], self.lo[1], self.lo[2],
            self.cell, self.g[0], self.g[1], self.g[2], *self._bin_args(), ptr(dist), ptr(visible), stream()),
            "dsu_bone_visibility")

    def run(self):
        if self.items is None:
            raise DsuError("BoneVisibilityPlan.run before bin()")
        dist = torch.empty((self.V, self.B), dtype=torch.float64, device=self.verts.device)
        visible = torch.empty((self.V, self.B), dtype=torch.uint8, device=self.verts.device)
        self._stage(SKIN_RUN, dist, visible)
        return dist, visible


def bone_visibility(verts, faces, bones, cells_per_axis=None):
    """For every (vertex, bone): the distance to the bone's segment (V,B) f64 and whether the open
    segment vertex -> closest point is free of triangles (V,B) uint8 (include/dsu_hip.h,
    dsu_bone_visibility)."""
    return BoneVisibilityPlan(verts, faces, bones, cells_per_axis).bin().run()


def spd_cg_block(rowptr, cols, vals, rhs, x0=None, tol=1e-10, max_iters=10000):
    """Jacobi-preconditioned conjugate gradients in float64 for a symmetric positive definite CSR
    matrix and all columns of rhs (n,B) at once (dsu_spd_cg_block).  Returns (x (n,B) f64,
    iterations, final relative residuals (B,) as a numpy array)."""
    import ctypes as C
    import numpy as np
    rhs = rhs.to(torch.float64).contiguous()
    if rhs.dim() != 2:
        raise ValueError("rhs (n,B) expected")
    n, B = rhs.shape
    rowptr, cols = rowptr.to(torch.int32).contiguous(), cols.to(torch.int32).contiguous()
    vals = vals.to(torch.float64).contiguous()
    if rowptr.numel() != n + 1 or cols.numel() != vals.numel():
        raise ValueError("CSR arrays do not match rhs")
    x = torch.zeros_like(rhs) if x0 is None else x0.to(torch.float64).clone().contiguous()
    nbytes = lib().dsu_spd_cg_block_workspace_bytes(n, B)
    if nbytes < 0:
        check(int(nbytes), "dsu_spd_cg_block_workspace_bytes")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=rhs.device)
    iters = C.c_int32(0)
    res = np.zeros(B, np.float64)
    check(lib().dsu_spd_cg_block(ptr(rowptr, torch.int32), ptr(cols, torch.int32), ptr(vals, torch.float64),
                                 n, vals.numel(), B, ptr(rhs, torch.float64), ptr(x, torch.float64),
                                 float(tol), int(max_iters), ptr(ws), ws.numel() * 8, C.byref(iters),
                                 res.ctypes.data_as(C.POINTER(C.c_double)), stream()), "dsu_spd_cg_block")
    return x, int(iters.value), res


def skin_lbs(rest, influences, weights, matrices):
    """Linear-blend skinning (dsu_skin_lbs): rest (V,3), influences (V,K) joint indices, weights
    (V,K), matrices (F,J,3,4) -> (F,V,3) f32 on the device."""
    rest, weights, matrices = _f32c(rest), _f32c(weights), _f32c(matrices)
    influences = influences.to(torch.int32).contiguous()
    if rest.dim() != 2 or rest.shape[1] != 3 or influences.dim() != 2 or weights.shape != influences.shape \
            or influences.shape[0] != rest.shape[0] or matrices.dim() != 4 or matrices.shape[2:] != (3, 4):
        raise ValueError("rest (V,3), influences / weights (V,K) and matrices (F,J,3,4) expected")
    V, K = influences.shape
    F, J = matrices.shape[:2]
    out = torch.empty((F, V, 3), dtype=torch.float32, device=rest.device)
    check(lib().dsu_skin_lbs(ptr(rest, torch.float32), ptr(influences, torch.int32), ptr(weights, torch.float32),
                             ptr(matrices, torch.float32), V, K, F, J, ptr(out), stream()), "dsu_skin_lbs")
    return out


def skin_dqs(rest, influences, weights, dualquats):
    """Dual-quaternion skinning (dsu_skin_dqs): rest (V,3), influences (V,K) joint indices, weights
    (V,K), dualquats (F,J,8) float64 (animate.dual_quaternions) -> (F,V,3) f32 on the device."""
    rest, weights = _f32c(rest), _f32c(weights)
    influences = influences.to(torch.int32).contiguous()
    dualquats = dualquats.to(torch.float64).contiguous()
    if rest.dim() != 2 or rest.shape[1] != 3 or influences.dim() != 2 or weights.shape != influences.shape \
            or influences.shape[0] != rest.shape[0] or dualquats.dim() != 3 or dualquats.shape[2] != 8:
        raise ValueError("rest (V,3), influences / weights (V,K) and dualquats (F,J,8) expected")
    V, K = influences.shape
    F, J = dualquats.shape[:2]
    out = torch.empty((F, V, 3), dtype=torch.float32, device=rest.device)
    check(lib().dsu_skin_dqs(ptr(rest, torch.float32), ptr(influences, torch.int32), ptr(weights, torch.float32),
                             ptr(dualquats, torch.float64), V, K, F, J, ptr(out), stream()), "dsu_skin_dqs")
    return out


def skin_cor_table(influences, weights, n_joints):
    """The canonical influence table of dsu_skin_cor_centres from any (influences (V,K), weights
    (V,K)), in numpy: an influence outside [0, n_joints) or with a weight that is not > 0 is dropped,
    duplicate joints are added in float64 in k order and rounded to f32, the joints of a row ascend
    and the padding after them is -1 / 0.  -> joints (V,K') int32, weights (V,K') float32 with K' the
    longest row (at least 1)."""
    import numpy as np
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    infl = to_np(influences).astype(np.int64)
    w = to_np(weights).astype(np.float32).astype(np.float64)
    if infl.ndim != 2 or w.shape != infl.shape:
        raise ValueError("influences / weights (V,K) expected")
    V, K = infl.shape
    J = int(n_joints)
    with np.errstate(invalid="ignore"):
        use = (infl >= 0) & (infl < J) & (w > 0.0)
    key = np.where(use, infl, J)
    order = np.argsort(key, axis=1, kind="stable")                   # by joint; k order within a joint
    sj, sw = np.take_along_axis(key, order, 1), np.take_along_axis(w, order, 1)
    first = np.ones((V, K), bool)
    first[:, 1:] = sj[:, 1:] != sj[:, :-1]
    slot = np.cumsum(first, 1) - 1
    acc = np.zeros((V, max(K, 1)))
    joints = np.full((V, max(K, 1)), -1, np.int32)
    for k in range(K):
        rows = np.flatnonzero(sj[:, k] < J)
        acc[rows, slot[rows, k]] = acc[rows, slot[rows, k]] + sw[rows, k]
        joints[rows, slot[rows, k]] = sj[rows, k]
    n = int((joints >= 0).sum(1).max()) if V else 0
    n = max(n, 1)
    return np.ascontiguousarray(joints[:, :n]), np.ascontiguousarray(acc[:, :n].astype(np.float32))


def skin_cor_centres(rest, faces, influences, weights, n_joints, sigma=0.1):
    """Centres of rotation of a rigged mesh (dsu_skin_cor_centres; Le & Hodgins 2016), once per
    character: rest (V,3) on the device, faces (T,3), any influences / weights (V,K) (the canonical
    table is made here, skin_cor_table) -> (centres (V,3) f64, valid (V,) uint8) on the device.  A
    vertex on one joint alone has no centre (valid 0): ops.skin_cor blends it linearly."""
    rest = _f32c(rest)
    if rest.dim() != 2 or rest.shape[1] != 3:
        raise ValueError("rest (V,3) expected")
    V = rest.shape[0]
    joints, w = skin_cor_table(influences, weights, n_joints)
    if joints.shape[0] != V:
        raise ValueError("influences / weights (V,K) of the rest mesh expected")
    faces = faces.to(device=rest.device, dtype=torch.int32).contiguous() if torch.is_tensor(faces) else \
        torch.as_tensor(faces, dtype=torch.int32).reshape(-1, 3).contiguous().to(rest.device)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces (T,3) expected")
    T, K = faces.shape[0], joints.shape[1]
    tj, tw = torch.from_numpy(joints).to(rest.device), torch.from_numpy(w).to(rest.device)
    centres = torch.zeros((V, 3), dtype=torch.float64, device=rest.device)
    valid = torch.zeros((V,), dtype=torch.uint8, device=rest.device)
    nbytes = lib().dsu_skin_cor_centres_workspace_bytes(V, T, K, int(n_joints))
    if nbytes < 0:
        check(int(nbytes), "dsu_skin_cor_centres_workspace_bytes")
    ws = torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.float64, device=rest.device)   # never short of nbytes
    check(lib().dsu_skin_cor_centres(ptr(rest, torch.float32), ptr(faces, torch.int32), ptr(tj, torch.int32),
                                     ptr(tw, torch.float32), V, T, K, int(n_joints), float(sigma), ptr(ws), nbytes,
                                     ptr(centres), ptr(valid), stream()), "dsu_skin_cor_centres")
    return centres, valid


def skin_cor(rest, influences, weights, matrices, quats, centres, valid):
    """Centre-of-rotation skinning (dsu_skin_cor): rest (V,3), influences / weights (V,K) as skin_dqs
    takes them, matrices (F,J,3,4) float64 (animate.skinning_matrices), quats (F,J,4) float64
    (animate.rotation_quaternions of their rotations), centres (V,3) f64 and valid (V,) uint8 from
    skin_cor_centres -> (F,V,3) f32 on the device."""
    rest, weights = _f32c(rest), _f32c(weights)
    influences = influences.to(torch.int32).contiguous()
    matrices, quats = matrices.to(torch.float64).contiguous(), quats.to(torch.float64).contiguous()
    centres, valid = centres.to(torch.float64).contiguous(), valid.to(torch.uint8).contiguous()
    if rest.dim() != 2 or rest.shape[1] != 3 or influences.dim() != 2 or weights.shape != influences.shape \
            or influences.shape[0] != rest.shape[0] or matrices.dim() != 4 or matrices.shape[2:] != (3, 4) \
            or quats.shape != matrices.shape[:2] + (4,) or centres.shape != rest.shape \
            or valid.shape != rest.shape[:1]:
        raise ValueError("rest (V,3), influences / weights (V,K), matrices (F,J,3,4), quats (F,J,4), centres (V,3) "
                         "and valid (V,) expected")
    V, K = influences.shape
    F, J = matrices.shape[:2]
    out = torch.empty((F, V, 3), dtype=torch.float32, device=rest.device)
    check(lib().dsu_skin_cor(ptr(rest, torch.float32), ptr(influences, torch.int32), ptr(weights, torch.float32),
                             ptr(matrices, torch.float64), ptr(quats, torch.float64), ptr(centres, torch.float64),
                             ptr(valid, torch.uint8), V, K, F, J, ptr(out), stream()), "dsu_skin_cor")
    return out


CORRECTIVE_KEYS = ("rep", "faces", "nbr_rowptr", "nbr_cols", "cor_rowptr", "cor_faces")


def corrective_topology(topology, device):
    """The arrays of animate.corrective.smoothing_topology as contiguous int32 tensors on `device`
    (a mapping that holds them already is returned as it is, so one upload serves bind and smooth)."""
    import numpy as np
    dev = torch.device(device)
    out = {}
    for k in CORRECTIVE_KEYS:
        a = topology[k]
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(a, np.int32))
        out[k] = a.to(device=dev, dtype=torch.int32).contiguous()
    V = out["rep"].numel()
    if out["rep"].dim() != 1 or out["nbr_rowptr"].shape != (V + 1,) or out["cor_rowptr"].shape != (V + 1,) \
            or out["faces"].dim() != 2 or out["faces"].shape[1] != 3 or out["nbr_cols"].dim() != 1 \
            or out["cor_faces"].dim() != 1:
        raise ValueError("topology: rep (V), faces (M,3), nbr_rowptr / cor_rowptr (V+1), nbr_cols, cor_faces expected")
    return out


def _corrective_args(t):
    return (ptr(t["nbr_rowptr"], torch.int32), ptr(t["nbr_cols"], torch.int32), t["nbr_cols"].numel(),
            ptr(t["cor_rowptr"], torch.int32), ptr(t["cor_faces"], torch.int32), t["cor_faces"].numel(),
            ptr(t["faces"], torch.int32), t["faces"].shape[0])


def _corrective_workspace(V, F, device):
    nbytes = lib().dsu_corrective_smooth_workspace_bytes(V, F)
    if nbytes < 0:
        check(int(nbytes), "dsu_corrective_smooth_workspace_bytes")
    return torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=device), nbytes


def corrective_bind(rest, topology, factor, iterations):
    """Bind of the corrective smoothing (dsu_corrective_bind): rest (V,3), topology as
    animate.corrective.smoothing_topology gives it -> (delta (V,3) f64, valid (V,) uint8) on the
    device: every representative's offset from its smoothed rest position in its local frame."""
    rest = _f32c(rest)
    if rest.dim() != 2 or rest.shape[1] != 3:
        raise ValueError("rest (V,3) expected")
    t = corrective_topology(topology, rest.device)
    V = rest.shape[0]
    if t["rep"].numel() != V:
        raise ValueError("the topology is of another mesh")
    delta = torch.zeros((V, 3), dtype=torch.float64, device=rest.device)
    valid = torch.zeros((V,), dtype=torch.uint8, device=rest.device)
    ws, nbytes = _corrective_workspace(V, 1, rest.device)
    check(lib().dsu_corrective_bind(ptr(rest, torch.float32), *_corrective_args(t), V, float(factor), int(iterations),
                                    ptr(ws), nbytes, ptr(delta), ptr(valid), stream()), "dsu_corrective_bind")
    return delta, valid


def corrective_smooth(skinned, topology, delta, valid, factor, iterations):
    """Corrective smoothing of skinned frames (dsu_corrective_smooth): skinned (F,V,3), delta and
    valid from corrective_bind with the same factor and iterations -> (F,V,3) f32 on the device.
    `skinned` is not written."""
    skinned = _f32c(skinned)
    if skinned.dim() != 3 or skinned.shape[2] != 3:
        raise ValueError("skinned (F,V,3) expected")
    t = corrective_topology(topology, skinned.device)
    F, V = skinned.shape[:2]
    delta, valid = delta.to(torch.float64).contiguous(), valid.to(torch.uint8).contiguous()
    if t["rep"].numel() != V or delta.shape != (V, 3) or valid.shape != (V,):
        raise ValueError("topology, delta (V,3) and valid (V,) of the skinned mesh expected")
    out = torch.empty((F, V, 3), dtype=torch.float32, device=skinned.device)
    ws, nbytes = _corrective_workspace(V, F, skinned.device)
    a = _corrective_args(t)
    check(lib().dsu_corrective_smooth(ptr(skinned, torch.float32), ptr(t["rep"], torch.int32), *a,
                                      ptr(delta, torch.float64), ptr(valid, torch.uint8), V, F, float(factor),
                                      int(iterations), ptr(ws), nbytes, ptr(out), stream()), "dsu_corrective_smooth")
    return out
