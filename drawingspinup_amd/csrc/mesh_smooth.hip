// Constrained smoothing of the export's binary volume: the weighted-Jacobi iteration of
// mcubes.smooth (MarchingCubeHelper.forward, instant_nsr/models/geometry.py:57-58) on the
// compacted band voxels (gfx950, float64 as PyMCubes).
//
// Unknowns: the nv voxels with |signed distance| <= band radius, compacted in x-major order.
// nbr[6][nv] (int32): slot of the -/+ neighbour along x, y, z, or -1 when that neighbour is
// outside the band (or the volume): it then folds onto the diagonal of the 1-D second difference
//     (F_a v)(i) = cd_a(i) v(i) + v(n-_a(i)) + v(n+_a(i)),   cd_a = -2 + [no n-] + [no n+].
// Energy |F v|^2, Q = sum_a F_a^T F_a.  One iteration (PyMCubes: weight 0.5, projection onto the
// per-voxel bounds lower[i] <= x <= upper[i]: the initial distance on the voxel's own side, 0 for
// the voxels next to the surface, +-inf on the other side) is
//     x  <- clamp(w * (-(Q x - d x) / d) + (1 - w) x)  with Q x = sum_a F_a^T (F_a x), d = diag Q
// as ONE kernel per step (smooth_fused_kernel): the three rows y_a = F_a x a voxel needs per axis —
// its own and its two neighbours' — are computed from x on the fly, so no row is written or read;
// x ping-pongs between the caller's x and the first nv doubles of the scratch y.
// Unique memory per iteration: slots 24 nv + x 8 nv in + 8 nv out + bounds 16 nv = 56 nv bytes (a
// row pass and an update pass over stored rows, the form of rounds 2-4, moved ~200 nv); the band
// of a 512^3 export is 2-5 M voxels, i.e. it lives in the Infinity Cache across iterations.
// Every tenth iteration the energy x . Q x / 2: smooth_rows_kernel, the energy's row pass, stores
// y_a = F_a x (3 nv doubles; the fused kernel's rows are the very expressions, same operands, same
// order: bit-identical values), smooth_energy_kernel sums x . sum_a F_a^T y_a into per-workgroup
// partials in a fixed order (the host adds the partials: the stopping test is deterministic).
//
// The export runs the iteration on the BRICK layout instead (dsu_smooth_bricks_*, second half of
// this file): the band compacted in 8^3 bricks, so that a neighbour is an address and neighbouring
// lanes read neighbouring doubles.  One 256-thread workgroup per active brick and iteration stages
// the brick and the 2-deep face slabs of its six neighbours (512 + 6 x 128 doubles; the stencil is
// +-1, +-2 along each axis: no edge or corner halo) and one presence bit per tile voxel in LDS, then
// runs the same per-voxel arithmetic from constant LDS offsets: no slot loads, no dependent loads.
// The bounds come from the initial distance, one byte per voxel into a table of the volume's
// distinct distances (a double per voxel when there are more than 255).  Set-up is two kernels
// (brick occupancy, gather) around a compaction of the 64^3 brick flags: no 512 MB slot volume, no
// per-voxel position list.  Results equal the slot layout's bit for bit
// (tests/test_gpu_smooth_bricks.py); the energy is summed per brick, so it may differ in the last bits.
// Measured on the band of tests' _shape(512) (2.54 M band voxels in 10 960 bricks, 45 % full;
// tools/smooth_probe.py, profiles/smooth_bricks_probe.json, medians of neighbouring profiled runs):
//     iteration   slots 55.7 us   bricks 46.4 us (x1.20)   [stored doubles 47.4-49.6; direct loads
//                 through L1/L2 instead of LDS 98-100; 512 threads x 1 voxel 55-57, 128 x 4 54]
//     energy pass slots 61-62 us (two kernels)   bricks 54-55 us (one)
//     set-up      slots 2.1-2.4 ms   bricks 0.50-0.60 ms (device events around the build)
// The brick kernel runs for every voxel of an active brick (5.6 M here), which is what holds the
// gain per iteration well under the ratio of the request counts.
// On the band of the bench's drawing, alone on the GPU: 225.8 -> 149.3 us per iteration, all smoothing
// kernels 124.9 -> 84.8 ms per drawing (profiles/smooth_bricks_alone_kernel_stats_{old,new}.csv).
#include "common.h"

namespace {

__device__ __forceinline__ double at_or_zero(const double* __restrict__ v, int s) {
  return s >= 0 ? v[s] : 0.0;
}

__global__ __launch_bounds__(256) void smooth_rows_kernel(const int32_t* __restrict__ nbr, int64_t nv,
                                                          const double* __restrict__ x,
                                                          double* __restrict__ y) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double xi = x[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int m = nbr[(size_t)(2 * a) * nv + i], p = nbr[(size_t)(2 * a + 1) * nv + i];
      const double cd = -2.0 + (m < 0 ? 1.0 : 0.0) + (p < 0 ? 1.0 : 0.0);
      y[(size_t)a * nv + i] = cd * xi + at_or_zero(x, m) + at_or_zero(x, p);
    }
  }
}

// (Q x)(i) and diag Q (i) from the rows y_a
__device__ __forceinline__ void q_and_diag(const int32_t* __restrict__ nbr, int64_t nv,
                                           const double* __restrict__ y, int64_t i, double& q,
                                           double& d) {
  q = 0.0;
  d = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int m = nbr[(size_t)(2 * a) * nv + i], p = nbr[(size_t)(2 * a + 1) * nv + i];
    const double hm = m < 0 ? 0.0 : 1.0, hp = p < 0 ? 0.0 : 1.0;
    const double cd = -2.0 + (1.0 - hm) + (1.0 - hp);
    const double* ya = y + (size_t)a * nv;
    q += cd * ya[i] + at_or_zero(ya, m) + at_or_zero(ya, p);
    d += cd * cd + hm + hp;
  }
}

// The per-voxel arithmetic of one iteration, shared by the slot kernel and the brick kernels (one
// text: both are compiled from the same expressions, same operands, same order).  A layout first
// gathers, per axis, what the voxel's own row and its two neighbours' rows read (AxisRows: who is
// present, and the values, 0.0 where absent); the arithmetic below then has no load and no branch.
struct AxisRows {
  bool m, p;                   // the - / + neighbour is present
  double xm, xp;               // x there
  bool mm, mp, pm, pp;         // the - / + neighbours of the - neighbour, of the + neighbour
  double xmm, xmp, xpm, xpp;
};

// cd_a = -2 + [no n-] + [no n+].  smooth_rows_kernel and q_and_diag add these up in float64; the
// terms and every partial sum are integers of magnitude <= 2, exact in any form, so the value is
// picked instead of summed (float64 adds run at a quarter of the rate of a select on gfx950).
__device__ __forceinline__ double row_diagonal(bool m, bool p) {
  return m ? (p ? -2.0 : -1.0) : (p ? -1.0 : 0.0);
}

// y_a(j) = cd_a(j) x(j) + x(n-_a(j)) + x(n+_a(j)): smooth_rows_kernel's expression for voxel j
__device__ __forceinline__ double row_of(bool m, bool p, double xj, double xm, double xp) {
  const double cd = row_diagonal(m, p);
  return cd * xj + xm + xp;
}

// (Q x)(i) and diag Q (i), Q x from rows recomputed on the fly (q_and_diag's sum, with
// y_a(.) = row_of(.)).  diag Q = sum_a cd_a^2 + [n-] + [n+] is an integer <= 18: counted, then
// converted once (q_and_diag's float64 sum of the same integers is exact too).
__device__ __forceinline__ void q_and_diag_of(const AxisRows (&rows)[3], double xi, double& q, double& d) {
  q = 0.0;
  int dn = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const AxisRows& r = rows[a];
    const int hm = r.m ? 1 : 0, hp = r.p ? 1 : 0;
    const int cdn = -2 + (1 - hm) + (1 - hp);
    const double cd = row_diagonal(r.m, r.p);
    const double ya_i = cd * xi + r.xm + r.xp;
    const double ya_m = r.m ? row_of(r.mm, r.mp, r.xm, r.xmm, r.xmp) : 0.0;
    const double ya_p = r.p ? row_of(r.pm, r.pp, r.xp, r.xpm, r.xpp) : 0.0;
    q += cd * ya_i + ya_m + ya_p;
    dn += cdn * cdn + hm + hp;
  }
  d = (double)dn;
}

// xo = clamp(w * (-(Q x - d x) / d) + (1 - w) x)
__device__ __forceinline__ double projected_step(double q, double d, double xi, double weight,
                                                 double lower, double upper) {
  const double x1 = -(1.0 / d) * (q - d * xi);                 // -D^-1 R x
  double xn = weight * x1 + (1.0 - weight) * xi;
  xn = fmin(fmax(xn, lower), upper);       // np.maximum(x, lower); np.minimum(x, upper)
  return xn;
}

// the compacted band: neighbours through the six slot arrays (-1 = absent), the neighbours' own
// neighbours through theirs
__device__ __forceinline__ void slot_rows(const int32_t* __restrict__ nbr, int64_t nv,
                                          const double* __restrict__ x, int64_t i, AxisRows (&rows)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    AxisRows& r = rows[a];
    const int32_t* nm = nbr + (size_t)(2 * a) * nv;
    const int32_t* np = nbr + (size_t)(2 * a + 1) * nv;
    const int m = nm[i], p = np[i];
    r.m = m >= 0;
    r.p = p >= 0;
    r.xm = at_or_zero(x, m);
    r.xp = at_or_zero(x, p);
    r.mm = r.mp = r.pm = r.pp = false;
    r.xmm = r.xmp = r.xpm = r.xpp = 0.0;
    if (m >= 0) {
      const int mm = nm[m], mp = np[m];
      r.mm = mm >= 0;
      r.mp = mp >= 0;
      r.xmm = at_or_zero(x, mm);
      r.xmp = at_or_zero(x, mp);
    }
    if (p >= 0) {
      const int pm = nm[p], pp = np[p];
      r.pm = pm >= 0;
      r.pp = pp >= 0;
      r.xpm = at_or_zero(x, pm);
      r.xpp = at_or_zero(x, pp);
    }
  }
}

// one whole iteration on the slot layout
__global__ __launch_bounds__(256) void smooth_fused_kernel(const int32_t* __restrict__ nbr, int64_t nv,
                                                           const double* __restrict__ x,
                                                           const double* __restrict__ lower,
                                                           const double* __restrict__ upper,
                                                           double weight, double* __restrict__ xo) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double xi = x[i];
    AxisRows rows[3];
    slot_rows(nbr, nv, x, i, rows);
    double q, d;
    q_and_diag_of(rows, xi, q, d);
    xo[i] = projected_step(q, d, xi, weight, lower[i], upper[i]);
  }
}

constexpr int EN_BLOCKS = 1024;

__global__ __launch_bounds__(256) void smooth_energy_kernel(const int32_t* __restrict__ nbr,
                                                            int64_t nv,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ x,
                                                            double* __restrict__ partials) {
  __shared__ double ws[4];
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * blockDim.x) {
    double q, d;
    q_and_diag(nbr, nv, y, i, q, d);
    acc += x[i] * q;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}


// ---------------------------------------------------------------------------------------------
// The brick layout: the band compacted brick by brick (BR^3 voxels, aligned to the volume grid;
// a brick is active when it holds a band voxel).  Per active brick s: x in two ping-pong copies
// (BV doubles each, z fastest), BR mask words (word lx, bit ly * BR + lz: the voxel is in the
// band and inside the volume), the slots of its six face neighbours (nbr6[s * 8 + 0..5] = -x, +x,
// -y, +y, -z, +z, or -1), and the initial distance (a double, or a byte indexing a table of the
// volume's distinct values).  A voxel is present when it is inside the volume, in an active brick
// and its mask bit is set; everything else is absent exactly as slot -1 is above.
constexpr int BR = 8;
constexpr int BV = BR * BR * BR;          // 512 voxels
constexpr int ITER_THREADS = 256;         // threads of the iteration's workgroup: two voxels each (512 x 1
                                          // and 128 x 4 measured 20 % slower: fewer bricks in flight per
                                          // CU, or fewer waves)
constexpr int TD = BR + 4;                // tile side: the brick and the 2-deep face slabs
constexpr int TZ = TD;                    // z stride of the tile

__device__ __forceinline__ int tile_index(int tx, int ty, int tz) { return (tx * TD + ty) * TZ + tz; }

// PyMCubes' bounds from the initial distance (smooth_constrained's four torch.where lines)
__device__ __forceinline__ void bounds_of(double x0, double& lower, double& upper) {
  lower = x0 > 0.0 ? x0 : -INFINITY;
  upper = x0 < 0.0 ? x0 : INFINITY;
  lower = fabs(lower) < 1.0 ? 0.0 : lower;
  upper = fabs(upper) < 1.0 ? 0.0 : upper;
}

// AxisRows of a brick voxel from fetch(a, k, v): is the voxel k = -2, -1, +1, +2 steps along axis a
// present, v = x there or 0.0.  The voxel itself is the + neighbour of its - neighbour (and the
// other way round), at distance 2 sits the neighbour's other neighbour.
template <class F>
__device__ __forceinline__ void brick_rows(const F& fetch, double xi, AxisRows (&rows)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    AxisRows& r = rows[a];
    r.m = fetch(a, -1, r.xm);
    r.p = fetch(a, 1, r.xp);
    r.mm = fetch(a, -2, r.xmm);
    r.pp = fetch(a, 2, r.xpp);
    r.mp = r.pm = true;
    r.xmp = r.xpm = xi;
  }
}

// brick + face slabs staged in LDS: every fetch is a load at a constant offset from the voxel
struct TileFetch {
  const double* tile;        // [TD][TD][TZ], at the voxel
  const uint32_t* prow;      // [TD][TD]: bit tz of row (tx, ty), at the voxel's row
  int tz;
  __device__ __forceinline__ bool operator()(int a, int k, double& v) const {
    const int rows = a == 0 ? k * TD : a == 1 ? k : 0, dz = a == 2 ? k : 0;
    const bool here = (prow[rows] >> (tz + dz)) & 1u;
    const double there = tile[rows * TZ + dz];         // (never a conditional load)
    v = here ? there : 0.0;
    return here;
  }
};

// the same without the staging: every fetch goes to the bricks in global memory
struct DirectFetch {
  const double* __restrict__ x;
  const uint64_t* __restrict__ mask;
  int own, lo[3], hi[3];     // slots: own brick, the - and the + neighbour along each axis
  int lx, ly, lz;
  __device__ __forceinline__ bool operator()(int a, int k, double& v) const {
    int c[3] = {lx, ly, lz};
    const int at = c[a] + k;
    const int s = at < 0 ? lo[a] : at >= BR ? hi[a] : own;
    c[a] = at & (BR - 1);
    bool here = false;
    v = 0.0;
    if (s >= 0) {
      here = (mask[(size_t)s * BR + c[0]] >> (c[1] * BR + c[2])) & 1ull;
      if (here) v = x[(size_t)s * BV + (c[0] * BR + c[1]) * BR + c[2]];
    }
    return here;
  }
};

// stage brick s and the 2-deep face slabs of its six neighbours (768 doubles) + the presence rows;
// BT threads, each with the voxels t, t + BT, ... of the brick
template <int BT>
__device__ __forceinline__ void stage_tile(const double* __restrict__ x, const uint64_t* __restrict__ mask,
                                           const int32_t* __restrict__ nbr6, int s,
                                           const double (&xi)[BV / BT], double* tile, uint32_t* prow) {
  const int t = threadIdx.x;
  const int32_t* n6 = nbr6 + (size_t)s * 8;
#pragma unroll
  for (int j = 0; j < BV / BT; ++j) {
    const int v = t + j * BT;
    const int lx = v >> 6, ly = (v >> 3) & 7, lz = v & 7;
    const int own = tile_index(lx + 2, ly + 2, lz + 2);
    tile[own] = xi[j];
    // The voxel with these coordinates in a neighbour brick lies in that brick's face slab when
    // its coordinate along the axis is 0, 1 (the + neighbour's slab) or 6, 7 (the - one's): the
    // same offset v inside the other brick, BR further along the axis in the tile.
    auto halo = [&](int c, int nm, int np, int stride) {
      if (c < 2 || c >= BR - 2) {
        const int ns = c < 2 ? np : nm;
        if (ns >= 0) tile[own + (c < 2 ? BR : -BR) * stride] = x[(size_t)ns * BV + v];
      }
    };
    halo(lx, n6[0], n6[1], TD * TZ);
    halo(ly, n6[2], n6[3], TZ);
    halo(lz, n6[4], n6[5], 1);
  }
  for (int r = t; r < TD * TD; r += BT) {
    const int tx = r / TD, ty = r % TD;
    const int fx = tx < 2 ? 0 : tx >= BR + 2 ? 1 : -1, fy = ty < 2 ? 2 : ty >= BR + 2 ? 3 : -1;
    uint32_t w = 0;
    if (fx < 0 || fy < 0) {
      const int f = fx >= 0 ? fx : fy;
      const int src = f < 0 ? s : n6[f];
      const int sh = ((ty - 2) & 7) * BR;
      if (src >= 0) w = (uint32_t)((mask[(size_t)src * BR + ((tx - 2) & 7)] >> sh) & 0xffu) << 2;
      if (f < 0) {                                     // a row of the brick itself: its z halo
        const int zm = n6[4], zp = n6[5];
        if (zm >= 0) w |= (uint32_t)((mask[(size_t)zm * BR + (tx - 2)] >> sh) & 0xffu) >> 6;
        if (zp >= 0) w |= (uint32_t)((mask[(size_t)zp * BR + (tx - 2)] >> sh) & 0x3u) << (BR + 2);
      }
    }
    prow[r] = w;
  }
}

// one whole iteration on the brick layout: one workgroup of BT threads per active brick
template <bool CODED, bool DIRECT, int BT>
__global__ __launch_bounds__(BT) void smooth_brick_kernel(const int32_t* __restrict__ nbr6,
                                                          const uint64_t* __restrict__ mask,
                                                          const double* __restrict__ x,
                                                          const double* __restrict__ x0,
                                                          const uint8_t* __restrict__ code,
                                                          const double* __restrict__ values, int nvalues,
                                                          double weight, double* __restrict__ xo) {
  constexpr int VPT = BV / BT;
  __shared__ double tile[DIRECT ? 1 : TD * TD * TZ];
  __shared__ uint32_t prow[DIRECT ? 1 : TD * TD];
  __shared__ double vals[CODED ? 256 : 1];
  const int s = blockIdx.x, t = threadIdx.x;
  const size_t g = (size_t)s * BV + t;
  double xi[VPT], b0[VPT];
  int cd0[VPT];
  bool here[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int v = t + j * BT;
    xi[j] = x[g + j * BT];
    here[j] = (mask[(size_t)s * BR + (v >> 6)] >> (v & 63)) & 1ull;
    if (CODED) cd0[j] = code[g + j * BT];
    else b0[j] = x0[g + j * BT];
  }
  if (CODED)
    for (int k = t; k < nvalues; k += BT) vals[k] = values[k];
  if (!DIRECT) stage_tile<BT>(x, mask, nbr6, s, xi, tile, prow);
  if (!DIRECT || CODED) __syncthreads();
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    if (!here[j]) continue;
    const int v = t + j * BT;
    const int lx = v >> 6, ly = (v >> 3) & 7, lz = v & 7;
    AxisRows rows[3];
    if (DIRECT) {
      const int32_t* n6 = nbr6 + (size_t)s * 8;
      brick_rows(DirectFetch{x, mask, s, {n6[0], n6[2], n6[4]}, {n6[1], n6[3], n6[5]}, lx, ly, lz},
                 xi[j], rows);
    } else {
      const int row = (lx + 2) * TD + ly + 2, tz = lz + 2;
      brick_rows(TileFetch{tile + row * TZ + tz, prow + row, tz}, xi[j], rows);
    }
    double q, d;
    q_and_diag_of(rows, xi[j], q, d);
    double lower, upper;
    bounds_of(CODED ? vals[cd0[j]] : b0[j], lower, upper);
    xo[g + j * BT] = projected_step(q, d, xi[j], weight, lower, upper);
  }
}

// x . Q x of one brick (the host adds the bricks in order and halves)
__global__ __launch_bounds__(BV) void smooth_brick_energy_kernel(const int32_t* __restrict__ nbr6,
                                                                 const uint64_t* __restrict__ mask,
                                                                 const double* __restrict__ x,
                                                                 double* __restrict__ partials) {
  __shared__ double tile[TD * TD * TZ];
  __shared__ uint32_t prow[TD * TD];
  __shared__ double ws[BV / 64];
  const int s = blockIdx.x, t = threadIdx.x;
  const double xi = x[(size_t)s * BV + t];
  const bool here = (mask[(size_t)s * BR + (t >> 6)] >> (t & 63)) & 1ull;
  stage_tile<BV>(x, mask, nbr6, s, {xi}, tile, prow);
  __syncthreads();
  double acc = 0.0;
  if (here) {
    const int row = ((t >> 6) + 2) * TD + ((t >> 3) & 7) + 2, tz = (t & 7) + 2;
    AxisRows rows[3];
    brick_rows(TileFetch{tile + row * TZ + tz, prow + row, tz}, xi, rows);
    double q, d;
    q_and_diag_of(rows, xi, q, d);
    acc = xi * q;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((t & 63) == 0) ws[t >> 6] = acc;
  __syncthreads();
  if (t == 0)
    partials[s] = ((ws[0] + ws[1]) + (ws[2] + ws[3])) + ((ws[4] + ws[5]) + (ws[6] + ws[7]));
}

// flags[brick] = 1 where the brick holds a band voxel: one thread per z-row segment of BR voxels
__global__ __launch_bounds__(256) void brick_flag_kernel(const uint8_t* __restrict__ band, int X, int Y,
                                                         int Z, int nby, int nbz, bool wide,
                                                         int32_t* __restrict__ flags) {
  const int64_t n = (int64_t)X * Y * nbz;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int bz = (int)(i % nbz);
    const int64_t xy = i / nbz;
    const int y = (int)(xy % Y), x = (int)(xy / Y);
    const uint8_t* row = band + (xy * Z + (int64_t)bz * BR);
    bool any = false;
    if (wide) {                                        // Z a multiple of BR, band 8-byte aligned
      any = *(const uint64_t*)row != 0;
    } else {
      const int zn = min(BR, Z - bz * BR);
      for (int k = 0; k < zn; ++k) any |= row[k] != 0;
    }
    if (any) flags[((int64_t)(x / BR) * nby + y / BR) * nbz + bz] = 1;
  }
}

// band / dist -> brick s: x (both the value the iteration starts from and the bounds' x0), mask,
// neighbour slots, and the byte codes (miss[0] = 1 when a band value is not in `values`)
__global__ __launch_bounds__(BV) void brick_gather_kernel(const uint8_t* __restrict__ band,
                                                          const double* __restrict__ dist, int X, int Y,
                                                          int Z, int nbx, int nby, int nbz,
                                                          const int32_t* __restrict__ table,
                                                          const int32_t* __restrict__ bcoord,
                                                          const double* __restrict__ values, int nvalues,
                                                          double* __restrict__ x, double* __restrict__ x0,
                                                          uint8_t* __restrict__ code,
                                                          uint64_t* __restrict__ mask,
                                                          int32_t* __restrict__ nbr6,
                                                          int32_t* __restrict__ miss) {
  const int s = blockIdx.x, t = threadIdx.x;
  const int b = bcoord[s];
  const int bz = b % nbz, by = (b / nbz) % nby, bx = b / (nbz * nby);
  const int gx = bx * BR + (t >> 6), gy = by * BR + ((t >> 3) & 7), gz = bz * BR + (t & 7);
  const bool inside = gx < X && gy < Y && gz < Z;
  const int64_t v = ((int64_t)gx * Y + gy) * Z + gz;
  const bool in_band = inside && band[v] != 0;
  const double val = in_band ? dist[v] : 0.0;
  const size_t g = (size_t)s * BV + t;
  x[g] = val;
  if (x0) x0[g] = val;
  if (code) {
    int lo = 0, hi = nvalues - 1;                      // values ascending: binary search
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (values[mid] < val) lo = mid + 1; else hi = mid;
    }
    if (in_band && !(nvalues > 0 && values[lo] == val)) miss[0] = 1;
    code[g] = (uint8_t)lo;
  }
  const uint64_t word = __ballot(in_band);             // wave = one x-plane, lane = ly * 8 + lz
  if ((t & 63) == 0) mask[(size_t)s * BR + (t >> 6)] = word;
  if (t < 8) {
    int ns = -1;
    if (t < 6) {
      const int a = t >> 1, step = (t & 1) ? 1 : -1;
      const int cx = bx + (a == 0 ? step : 0), cy = by + (a == 1 ? step : 0), cz = bz + (a == 2 ? step : 0);
      if (cx >= 0 && cx < nbx && cy >= 0 && cy < nby && cz >= 0 && cz < nbz)
        ns = table[((int64_t)cx * nby + cy) * nbz + cz];
    }
    nbr6[(size_t)s * 8 + t] = ns;
  }
}

// x -> dist where the mask is set, and nowhere else
__global__ __launch_bounds__(BV) void brick_scatter_kernel(const double* __restrict__ x,
                                                           const uint64_t* __restrict__ mask,
                                                           const int32_t* __restrict__ bcoord, int X, int Y,
                                                           int Z, int nby, int nbz,
                                                           double* __restrict__ dist) {
  const int s = blockIdx.x, t = threadIdx.x;
  if (!((mask[(size_t)s * BR + (t >> 6)] >> (t & 63)) & 1ull)) return;
  const int b = bcoord[s];
  const int bz = b % nbz, by = (b / nbz) % nby, bx = b / (nbz * nby);
  const int gx = bx * BR + (t >> 6), gy = by * BR + ((t >> 3) & 7), gz = bz * BR + (t & 7);
  dist[((int64_t)gx * Y + gy) * Z + gz] = x[(size_t)s * BV + t];
}

static inline bool brick_grid(int32_t X, int32_t Y, int32_t Z, int& nbx, int& nby, int& nbz) {
  if (X < 1 || Y < 1 || Z < 1) return false;
  nbx = (X + BR - 1) / BR; nby = (Y + BR - 1) / BR; nbz = (Z + BR - 1) / BR;
  return (int64_t)nbx * nby * nbz < (1ll << 31) / BV;  // slots * BV and brick ids stay in int32
}

}  // namespace

extern "C" {

int32_t dsu_smooth_energy_partials(void) { return EN_BLOCKS; }

int dsu_smooth_iterate(const int32_t* nbr, int64_t nv, const double* lower, const double* upper,
                       double weight, int32_t iters, double* x, double* y, void* stream) {
  if (nv < 0 || iters < 0 || (nv && (!nbr || !lower || !upper || !x || !y))) return DSU_EINVAL;
  if (nv == 0 || iters == 0) return DSU_OK;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = dsu_capped_blocks(nv, 256, 8192);
  double* cur = x;
  double* nxt = y;                                  // first nv doubles of the scratch
  for (int it = 0; it < iters; ++it) {
    smooth_fused_kernel<<<dim3(blocks), dim3(256), 0, s>>>(nbr, nv, cur, lower, upper, weight, nxt);
    double* t = cur; cur = nxt; nxt = t;
  }
  DSU_CHECK_LAUNCH();
  if (cur != x &&
      hipMemcpyAsync(x, cur, (size_t)nv * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return DSU_ELAUNCH;
  return DSU_OK;
}

int dsu_smooth_energy(const int32_t* nbr, int64_t nv, const double* x, double* y,
                      double* partials, void* stream) {
  if (nv < 0 || !partials || (nv && (!nbr || !x || !y))) return DSU_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = dsu_capped_blocks(nv > 0 ? nv : 1, 256, 8192);
  if (nv > 0) smooth_rows_kernel<<<dim3(blocks), dim3(256), 0, s>>>(nbr, nv, x, y);
  smooth_energy_kernel<<<dim3(EN_BLOCKS), dim3(256), 0, s>>>(nbr, nv, y, x, partials);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int32_t dsu_smooth_brick_side(void) { return BR; }

int dsu_smooth_bricks_flags(const uint8_t* band, int32_t X, int32_t Y, int32_t Z, int32_t* flags,
                            void* stream) {
  int nbx, nby, nbz;
  if (!brick_grid(X, Y, Z, nbx, nby, nbz)) return DSU_EUNSUP;
  if (!band || !flags) return DSU_EINVAL;
  const int64_t n = (int64_t)X * Y * nbz;
  brick_flag_kernel<<<dim3(dsu_capped_blocks(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream>>>(
      band, X, Y, Z, nby, nbz, Z % BR == 0 && ((uintptr_t)band & 7) == 0, flags);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_smooth_bricks_gather(const uint8_t* band, const double* dist, int32_t X, int32_t Y, int32_t Z,
                             const int32_t* table, const int32_t* bcoord, int32_t nb,
                             const double* values, int32_t nvalues, double* x, double* x0,
                             uint8_t* code, uint64_t* mask, int32_t* nbr6, int32_t* miss,
                             void* stream) {
  int nbx, nby, nbz;
  if (!brick_grid(X, Y, Z, nbx, nby, nbz)) return DSU_EUNSUP;
  if (nb < 0 || nb > nbx * nby * nbz || nvalues < 0 || nvalues > 255) return DSU_EINVAL;
  if (nb == 0) return DSU_OK;
  if (!band || !dist || !table || !bcoord || !x || !mask || !nbr6 || (!x0 && !code) ||
      (code && (!miss || (nvalues && !values))))
    return DSU_EINVAL;
  brick_gather_kernel<<<dim3(nb), dim3(BV), 0, (hipStream_t)stream>>>(
      band, dist, X, Y, Z, nbx, nby, nbz, table, bcoord, values, nvalues, x, x0, code, mask, nbr6, miss);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_smooth_bricks_iterate(const int32_t* nbr6, const uint64_t* mask, int32_t nb, const double* x0,
                              const uint8_t* code, const double* values, int32_t nvalues,
                              double weight, int32_t iters, int32_t direct, double* x, double* y,
                              void* stream) {
  if (nb < 0 || iters < 0 || nvalues < 0 || nvalues > 255) return DSU_EINVAL;
  if (nb == 0 || iters == 0) return DSU_OK;
  if (!nbr6 || !mask || !x || !y || (code ? (nvalues && !values) : !x0)) return DSU_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  double* cur = x;
  double* nxt = y;
#define DSU_BRICK_LAUNCH(CODED, DIRECT)                                                         \
  smooth_brick_kernel<CODED, DIRECT, ITER_THREADS>                                              \
      <<<dim3(nb), dim3(ITER_THREADS), 0, s>>>(nbr6, mask, cur, x0, code,                      \
                                               values, nvalues, weight, nxt)
  for (int it = 0; it < iters; ++it) {
    if (direct) {
      if (code) DSU_BRICK_LAUNCH(true, true); else DSU_BRICK_LAUNCH(false, true);
    } else {
      if (code) DSU_BRICK_LAUNCH(true, false); else DSU_BRICK_LAUNCH(false, false);
    }
    double* t = cur; cur = nxt; nxt = t;
  }
  DSU_CHECK_LAUNCH();
  if (cur != x &&
      hipMemcpyAsync(x, cur, (size_t)nb * BV * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return DSU_ELAUNCH;
  return DSU_OK;
}

int dsu_smooth_bricks_energy(const int32_t* nbr6, const uint64_t* mask, int32_t nb, const double* x,
                             double* partials, void* stream) {
  if (nb < 0) return DSU_EINVAL;
  if (nb == 0) return DSU_OK;
  if (!nbr6 || !mask || !x || !partials) return DSU_EINVAL;
  smooth_brick_energy_kernel<<<dim3(nb), dim3(BV), 0, (hipStream_t)stream>>>(nbr6, mask, x, partials);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_smooth_bricks_scatter(const double* x, const uint64_t* mask, const int32_t* bcoord, int32_t nb,
                              int32_t X, int32_t Y, int32_t Z, double* dist, void* stream) {
  int nbx, nby, nbz;
  if (!brick_grid(X, Y, Z, nbx, nby, nbz)) return DSU_EUNSUP;
  if (nb < 0 || nb > nbx * nby * nbz) return DSU_EINVAL;
  if (nb == 0) return DSU_OK;
  if (!x || !mask || !bcoord || !dist) return DSU_EINVAL;
  brick_scatter_kernel<<<dim3(nb), dim3(BV), 0, (hipStream_t)stream>>>(x, mask, bcoord, X, Y, Z, nby, nbz,
                                                                      dist);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

}  // extern "C"
