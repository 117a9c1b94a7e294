// Multi-resolution hash grid + fused SDF MLP for gfx950.
//
// Replaces tiny-cuda-nn's HashGrid encoding (reference call sites
// 2_charactor_reconstructor/instant_nsr/models/network_utils.py:46,55) and fuses it with
// the reference's own VanillaMLP geometry network (network_utils.py:94-138) and the
// finite-difference normal/laplacian logic of VolumeSDF.forward (geometry.py:135-187).
//
// Arithmetic contract (the oracle in oracle/hashgrid.py restates exactly this):
//   level l:  scale_l = (float)(exp2(l*log2(per_level_scale))*base_res - 1)   [double -> f32]
//             res_l   = (uint32)ceilf(scale_l) + 1
//             size_l  = min(round_up(res_l^3, 8), 2^log2_hashmap)   entries
//   point x in [0,1]^3:  pos = fmaf(scale, x, 0.5f); cell = floorf(pos); frac = pos - cell
//   corner c (bit d of c selects cell+1 in dim d), weight = prod_d (bit ? frac_d : 1-frac_d)
//             (f32 product in dim order 0,1,2 starting from 1.0f)
//   index:    dense  x + y*res + z*res^2   when res^3 <= size_l, else
//             (x*1) ^ (y*2654435761) ^ (z*805459861)   (uint32), both taken mod size_l
//   feature:  acc = fma((f16)weight, table[index], acc) in binary16 for c = 0..7 (f16 FMA,
//             one rounding per step), exactly tcnn's half-precision accumulation.
#define DSU_RELU_ONE_VMAX       // no matrix instructions in this file (common.h: dsu_relu)
#include "hashgrid_dev.h"
#include <utility>

using namespace dsu_hg;

namespace {

// ---------------------------------------------------------------- plain encode (tcnn shim)
template <int NL>
__global__ __launch_bounds__(256) void encode_fwd_kernel(const __half2* __restrict__ table,
                                                         GridMeta m,
                                                         const float* __restrict__ x, int64_t n,
                                                         uint32_t active,
                                                         __half2* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float px = x[i * 3 + 0], py = x[i * 3 + 1], pz = x[i * 3 + 2];
    __half2* o = out + i * NL;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      __half2 f = __float2half2_rn(0.0f);
      if ((uint32_t)l < active) f = lookup_level(table, m, l, px, py, pz);
      o[l] = f;
    }
  }
}

// grad wrt table: thread per (point, level); level = blockIdx.y keeps one level's slice of
// the gradient table hot in L2 while it is being scattered into.
__global__ __launch_bounds__(256) void encode_bwd_kernel(GridMeta m, int nl,
                                                         const float* __restrict__ x,
                                                         const float* __restrict__ dout,
                                                         int64_t n, float* __restrict__ gtable) {
  const int l = blockIdx.y;
  const uint32_t hsize = m.off[l + 1] - m.off[l];
  float* g = gtable + (size_t)m.off[l] * 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float d0 = dout[i * (2 * nl) + 2 * l], d1 = dout[i * (2 * nl) + 2 * l + 1];
    if (d0 == 0.0f && d1 == 0.0f) continue;
    CellPos p = cell_of(m.scale[l], x[i * 3], x[i * 3 + 1], x[i * 3 + 2]);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      uint32_t idx = grid_index(m.hashed[l], hsize, m.res[l], p.c[0] + (c & 1),
                                p.c[1] + ((c >> 1) & 1), p.c[2] + ((c >> 2) & 1));
      float w = corner_weight(p, c);
      unsafeAtomicAdd(g + (size_t)idx * 2, w * d0);
      unsafeAtomicAdd(g + (size_t)idx * 2 + 1, w * d1);
    }
  }
}

// ---------------------------------------------------------------- fused SDF network
// Encode one contracted point into the MLP input vector (xyz*2-1, masked features).
template <int NL, int LMAX = NL>
__device__ __forceinline__ void encode_input(const __half2* __restrict__ table,
                                             const GridMeta& m, uint32_t active, float x,
                                             float y, float z, float* in /*3+2NL*/) {
  in[0] = x * 2.0f + -1.0f;
  in[1] = y * 2.0f + -1.0f;
  in[2] = z * 2.0f + -1.0f;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    float2 f = make_float2(0.0f, 0.0f);
    if (l < LMAX && (uint32_t)l < active) f = __half22float2(lookup_level(table, m, l, x, y, z));
    in[3 + 2 * l] = f.x;
    in[4 + 2 * l] = f.y;
  }
}

// Both layers streamed over groups of four hidden units: pre-activation (k-ascending fma chain),
// Softplus, then the group's contribution to each of the NO outputs (j-ascending fma chain), so
// that the 64 hidden activations never exist at once (199 -> ~90 VGPRs: twice the resident waves
// to hide the table gathers).
// The weights are read through the SCALAR cache (constant address space, uniform
// addresses -> s_load into SGPR operands of the FMAs) instead of LDS broadcasts: a wave-wide
// ds_read_b128 occupies the CU's one LDS port for 8 clocks whether or not the lanes share the
// address, 368 of them per evaluation made the LDS port, shared by the four SIMDs, the kernel's
// bottleneck (measured on MI355X, 262 144 ray-ordered samples: forward 0.225 -> 0.173 ms at 4
// levels, 0.309 -> 0.236 ms at 7; 77 instead of 135-156 VGPRs, no LDS at all).
typedef __attribute__((address_space(4))) const float cfloat_t;
__device__ __forceinline__ const cfloat_t* as_const(const float* p) {
  return (const cfloat_t*)(uintptr_t)p;
}

template <int NL, int NO, int LMAX = NL>
__device__ __forceinline__ void mlp_stream_sgpr(const dsu_sdf_mlp& mlp, const float* in, int kmax,
                                                float* out /*NO*/) {
  constexpr int DIN = 3 + 2 * NL;
  const cfloat_t* w0 = as_const(mlp.w0);
  const cfloat_t* b0 = as_const(mlp.b0);
  const cfloat_t* w1 = as_const(mlp.w1);
  const cfloat_t* b1 = as_const(mlp.b1);
#pragma unroll
  for (int o = 0; o < NO; ++o) out[o] = b1[o];
#pragma unroll 1
  for (int j = 0; j < HID; j += 4) {
    float p0 = b0[j], p1 = b0[j + 1], p2 = b0[j + 2], p3 = b0[j + 3];
#pragma unroll
    for (int k = 0; k < 3 + 2 * LMAX; ++k) {
      if (k < kmax) {
        const float v = in[k];
        p0 = fmaf(w0[(j + 0) * DIN + k], v, p0);
        p1 = fmaf(w0[(j + 1) * DIN + k], v, p1);
        p2 = fmaf(w0[(j + 2) * DIN + k], v, p2);
        p3 = fmaf(w0[(j + 3) * DIN + k], v, p3);
      }
    }
    p0 = softplus100(p0); p1 = softplus100(p1); p2 = softplus100(p2); p3 = softplus100(p3);
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      float acc = out[o];
      acc = fmaf(w1[o * HID + j + 0], p0, acc);
      acc = fmaf(w1[o * HID + j + 1], p1, acc);
      acc = fmaf(w1[o * HID + j + 2], p2, acc);
      acc = fmaf(w1[o * HID + j + 3], p3, acc);
      out[o] = acc;
    }
  }
}

// no LDS, no barrier: any workgroup size works; one-wave workgroups (64 threads, finer balance of
// n / 64 waves over the SIMDs) measured no faster than 256 (0.1945 vs 0.187 ms)
constexpr int FWD_THREADS = 256;
// hidden units per group of the level-outer forward (scalar weight registers: JB x (DIN + 14))
constexpr int FWD_JB = 2;

// points of the export's lattice formed in the kernel (dsu_sdf_fwd_lattice): x-slabs from x0
struct SdfLattice {
  const float* lin;
  int32_t res, x0;
  float lo[3], span[3];
};

template <int NL, int NO, bool LAT = false>
__global__ __launch_bounds__(256) void sdf_fwd_kernel(const __half2* __restrict__ table,
                                                      GridMeta m, dsu_sdf_mlp mlp,
                                                      const float* __restrict__ pts, int64_t n,
                                                      float radius, uint32_t active,
                                                      float* __restrict__ out, SdfLattice lat) {
  const int kmax = 3 + 2 * (int)active;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float px, py, pz;
    if (LAT) {
      const int64_t r2 = (int64_t)lat.res * lat.res;
      const int ix = lat.x0 + (int)(i / r2), iy = (int)((i / lat.res) % lat.res), iz = (int)(i % lat.res);
      px = lat.lin[ix] * lat.span[0] + lat.lo[0];          // (-ffp-contract=off: two rounded operations)
      py = lat.lin[iy] * lat.span[1] + lat.lo[1];
      pz = lat.lin[iz] * lat.span[2] + lat.lo[2];
    } else {
      px = pts[i * 3 + 0]; py = pts[i * 3 + 1]; pz = pts[i * 3 + 2];
    }
    float x = contract(px, radius);
    float y = contract(py, radius);
    float z = contract(pz, radius);
    float in[3 + 2 * NL];
    encode_input<NL>(table, m, active, x, y, z, in);
    float o_[NO];
    mlp_stream_sgpr<NL, NO, NL>(mlp, in, kmax, o_);
#pragma unroll
    for (int o = 0; o < NO; ++o) out[i * NO + o] = o_[o];
  }
}

// VolumeSDF.forward with finite differences: 7 evaluations per point.
// LMAX: compile-time bound on the active levels (the 3000-step schedule uses 4..6 of the 10):
// levels >= LMAX, their metadata scalars and their share of the first-layer loop are compiled out.
template <int NL, int LMAX>
__global__ __launch_bounds__(256) void sdf_fd_fwd_kernel(
    const __half2* __restrict__ table, GridMeta m, dsu_sdf_mlp mlp,
    const float* __restrict__ pts, int64_t n, float radius, float eps, float eps2,
    uint32_t active, float* __restrict__ sdf, float* __restrict__ grad,
    float* __restrict__ feature, float* __restrict__ laplace, __half2* __restrict__ enc,
    const int32_t* __restrict__ perm) {
  const int kmax = 3 + 2 * (int)active;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // spatially sorted evaluation order (spatial_sort.hip): point i of `pts` is point perm[i] of
    // the caller's order; the per-point outputs go back to the caller's rows, the feature cache
    // stays in evaluation order (the backward pass walks it in the same order)
    const int64_t oi = perm ? (int64_t)perm[i] : i;
    const float p[3] = {pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2]};
    float s[7];
#pragma unroll 1
    for (int e = 0; e < 7; ++e) {
      float q[3] = {p[0], p[1], p[2]};
      if (e > 0) {
        const int ax = (e - 1) >> 1;
        const float d = ((e - 1) & 1) ? -eps : eps;
        // (points_ + offsets).clamp(-radius, radius)   (geometry.py:170)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          float v = q[a] + (a == ax ? d : 0.0f);
          q[a] = fminf(fmaxf(v, -radius), radius);
        }
      }
      float in[3 + 2 * NL];
      encode_input<NL, LMAX>(table, m, active, contract(q[0], radius), contract(q[1], radius),
                             contract(q[2], radius), in);
      if (enc != nullptr) {
        // interpolated f16 features of this evaluation, kept for the backward pass (exact: the
        // floats are widened halfs).  Layout [eval][point][active level].
        __half2* row = enc + ((size_t)e * n + i) * active;
#pragma unroll
        for (int l = 0; l < LMAX; ++l)
          if ((uint32_t)l < active) row[l] = __floats2half2_rn(in[3 + 2 * l], in[3 + 2 * l + 1]);
      }
      if (e == 0 && feature != nullptr) {
        float o_[NOUT];
        mlp_stream_sgpr<NL, NOUT, LMAX>(mlp, in, kmax, o_);
        s[0] = o_[0];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) feature[oi * NOUT + o] = o_[o];
      } else {
        float o_[1];
        mlp_stream_sgpr<NL, 1, LMAX>(mlp, in, kmax, o_);
        s[e] = o_[0];
      }
    }
    sdf[oi] = s[0];
    if (grad != nullptr) {
      // 0.5 * (sdf(+eps) - sdf(-eps)) / eps   (geometry.py:173)
      grad[oi * 3 + 0] = 0.5f * (s[1] - s[2]) / eps;
      grad[oi * 3 + 1] = 0.5f * (s[3] - s[4]) / eps;
      grad[oi * 3 + 2] = 0.5f * (s[5] - s[6]) / eps;
    }
    if (laplace != nullptr) {
      // (sdf(+)+sdf(-)-2 sdf).sum(-1) / eps^2   (geometry.py:176)
      float t0 = s[1] + s[2] - 2.0f * s[0];
      float t1 = s[3] + s[4] - 2.0f * s[0];
      float t2 = s[5] + s[6] - 2.0f * s[0];
      laplace[oi] = ((t0 + t1) + t2) / eps2;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The same 7 evaluations, level-outer: per active level the 8 corners of the centre's cell are
// gathered ONCE per point; an offset evaluation (+-eps along one axis: less than one cell on
// every active level, geometry.py:196-215 ties eps to the finest active level) stays in the
// centre's cell or moves to the neighbour that shares a face with it, so it reuses 8 or 4 of the
// centre's corners and gathers 0 or 4 new entries instead of 8.  Same table entries, same weights,
// same f16 FMA chain over corners 0..7 -> the features are bit-identical to lookup_level's.
// Gathers per point and level: 8 + 4 x (crossings) ~ 17-25 instead of 56.
//
// REGULAR points only: every evaluation inside the unit cube (then the other two axes keep their
// cell, cell coordinates stay in [0, res] and a dense index needs at most one subtraction of the
// level size instead of tcnn's modulo) and every offset within one cell of the centre.  A point
// that is not (outside the box, clamped, an eps of more than a cell: a few dozen of the 266 000
// of a step, the perturbed regulariser points next to the faces) is redone by its whole wave at
// the end of the wave's pass, evaluation by evaluation with the plain lookups (fd_point_by_wave:
// lanes = evaluations for the encoding, = hidden units for the MLP).  Handing such points to a
// second launch of the per-evaluation kernel cost as much as that whole kernel (0.12 ms measured:
// one wave's latency through 7 x (gathers + 16 weight groups) is the kernel's duration).  ND:
// levels below ND are dense, the others hashed (4 for the shipped grid; the launcher checks the
// level table against it).
//
// Then the MLP with the hidden units outer and the 7 evaluations inner: one set of scalar weight
// loads serves 7 evaluations; the interpolated features stay packed f16 in registers and enter
// the f32 FMAs through the mixed-precision form (widening is exact), the FMA chains (k ascending
// for the pre-activations, j ascending for the outputs) are those of mlp_stream_sgpr.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ __half2 interp8(const float (&fr)[3], const __half2* v) {
  __half2 acc = __float2half2_rn(0.0f);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float wf = 1.0f;                                   // corner_weight's product, same order
    wf *= (c & 1) ? fr[0] : 1.0f - fr[0];
    wf *= (c & 2) ? fr[1] : 1.0f - fr[1];
    wf *= (c & 4) ? fr[2] : 1.0f - fr[2];
    asm volatile("" : "+v"(wf));     // f32 product rounded before the f16 conversion (see lookup_level)
    const __half w = __float2half_rn(wf);
    acc = __hfma2(__half2(w, w), v[c], acc);
  }
  return acc;
}

// One level of the 7 evaluations of a regular point, as function templates so that the level
// index is a constant in every instance (a `#pragma unroll`ed loop over levels with this body is
// refused by the optimizer beyond a size limit, and f[][l] then lives in scratch).
// What one level keeps between issuing its requests and interpolating: the centre's fractions, the
// six offsets' fraction / cell step along their axis, the centre's corners, the new faces.
// (plain arrays with constant indices; a struct passed down by reference ended up in scratch
// memory)
struct FdLevelState {
  float (&fc)[3];
  float (&fa)[6];
  int (&rel)[6];
  __half2 (&v)[8];
  __half2 (&g)[6][4];
};

// Requests of one level for a regular point: 8 corners of the centre's cell + (per offset
// evaluation that leaves the cell) the 4 entries of the face the centre's cell does not have.
// Nothing here waits for a load: the new faces' registers are preset to zero, NOT to one of the
// centre's corners — `rel ? g : v` made the compiler copy v into g's register ahead of the
// conditional load, i.e. wait for the centre's corners before requesting the faces (two dependent
// round trips per level).
template <int l, int ND>
__device__ __forceinline__ void fd_level_issue(const __half2* __restrict__ table, const GridMeta& m,
                                               const float (&q)[7][3], FdLevelState& st, bool& bad) {
  constexpr bool HASHED = l >= ND;
  const uint32_t hsize = m.off[l + 1] - m.off[l];
  const __half2* lvl = table + m.off[l];
  const float scale = m.scale[l];
  const CellPos pc = cell_of(scale, q[0][0], q[0][1], q[0][2]);
  // index = combine(term of x, term of y, term of z); the term of coordinate c + 1 (c - 1) is the
  // term of c plus (minus) the axis' step: x, y * prime / y * res, z * prime / z * res^2
  const uint32_t res = m.res[l];
  const uint32_t step[3] = {1u, HASHED ? 2654435761u : res, HASHED ? 805459861u : res * res};
  uint32_t term[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    term[a][0] = pc.c[a] * step[a];
    term[a][1] = term[a][0] + step[a];
    st.fc[a] = pc.f[a];
  }
  auto index = [&](uint32_t tx, uint32_t ty, uint32_t tz) -> uint32_t {
    if (HASHED) return (tx ^ ty ^ tz) & (hsize - 1);
    const uint32_t idx = tx + ty + tz;                 // < 2 * hsize for coordinates in [0, res]
    return idx >= hsize ? idx - hsize : idx;
  };
#pragma unroll
  for (int c = 0; c < 8; ++c)
    st.v[c] = lvl[index(term[0][c & 1], term[1][(c >> 1) & 1], term[2][(c >> 2) & 1])];
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int ax = t >> 1, a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
    const float pa = fmaf(scale, q[t + 1][ax], 0.5f), fl = floorf(pa);
    st.fa[t] = pa - fl;
    st.rel[t] = (int)((uint32_t)(int)fl - pc.c[ax]);
    bad = bad || st.rel[t] < -1 || st.rel[t] > 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) st.g[t][k] = __float2half2_rn(0.0f);
    if (st.rel[t] != 0) {
      const uint32_t tn = st.rel[t] > 0 ? term[ax][1] + step[ax] : term[ax][0] - step[ax];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t tt[3];
        tt[ax] = tn;
        tt[a1] = term[a1][k & 1];
        tt[a2] = term[a2][k >> 1];
        st.g[t][k] = lvl[index(tt[0], tt[1], tt[2])];
      }
    }
  }
}

template <int l, int ACT>
__device__ __forceinline__ void fd_level_finish(const FdLevelState& st, __half2 (&f)[7][ACT]) {
  f[0][l] = interp8(st.fc, st.v);
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int ax = t >> 1, a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
    float fr[3];
    fr[ax] = st.fa[t];
    fr[a1] = st.fc[a1];
    fr[a2] = st.fc[a2];
    __half2 w[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int lo = ((k & 1) << a1) | ((k >> 1) << a2), hi = lo | (1 << ax);
      w[lo] = st.rel[t] == 0 ? st.v[lo] : (st.rel[t] > 0 ? st.v[hi] : st.g[t][k]);
      w[hi] = st.rel[t] == 0 ? st.v[hi] : (st.rel[t] > 0 ? st.g[t][k] : st.v[lo]);
    }
    f[t + 1][l] = interp8(fr, w);
  }
  // pin the level's features HERE: without a use before the `bad` exit of the kernel, the optimizer
  // sinks all the interpolation arithmetic behind that exit and keeps every gathered entry of every
  // level alive until then (396 VGPRs at 4 levels)
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    uint32_t bits = *reinterpret_cast<const uint32_t*>(&f[e][l]);
    asm volatile("" : "+v"(bits));
    f[e][l] = *reinterpret_cast<const __half2*>(&bits);
  }
}

// Level by level: the requests of level l + 1 go out after level l is interpolated (issuing them
// before, with two level states alive, lost its A/B).
template <int ACT, int ND, int... Ls>
__device__ __forceinline__ void fd_levels(const __half2* __restrict__ table, const GridMeta& m,
                                          const float (&q)[7][3], __half2 (&f)[7][ACT], bool& bad,
                                          std::integer_sequence<int, Ls...>) {
  float fc[3], fa[6];
  int rel[6];
  __half2 v[8], g[6][4];
  auto issue = [&](auto lc) {
    constexpr int l = decltype(lc)::value;
    FdLevelState st{fc, fa, rel, v, g};
    fd_level_issue<l, ND>(table, m, q, st, bad);
  };
  auto finish = [&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const FdLevelState st{fc, fa, rel, v, g};
    fd_level_finish<l, ACT>(st, f);
  };
  ((issue(std::integral_constant<int, Ls>{}), finish(std::integral_constant<int, Ls>{})), ...);
}

// One irregular point evaluated by a whole wave: same lookups (lookup_level), same FMA chains (k
// ascending for the pre-activations, j ascending for the outputs) as the per-evaluation kernel.
// p[] / i / oi are wave-uniform.  lds: 7 x DIN inputs + 7 x 64 hidden activations of this wave.
template <int NL, int ACT, bool FEAT>
__device__ __forceinline__ void fd_point_by_wave(
    const __half2* __restrict__ table, const GridMeta& m, const dsu_sdf_mlp& mlp, const float (&p)[3],
    int64_t i, int64_t oi, int64_t n, float radius, float eps, float eps2, float* __restrict__ sdf,
    float* __restrict__ grad, float* __restrict__ feature, float* __restrict__ laplace,
    __half2* __restrict__ enc, float* lds) {
  constexpr int DIN = 3 + 2 * NL, KIN = 3 + 2 * ACT;
  float* l_in = lds;                 // [7][KIN]
  float* l_h = lds + 7 * KIN;        // [7][64]
  const int lane = threadIdx.x & 63;
  // opaque copies of the pointers: the loads below are invariant in the caller's loops and would
  // be hoisted to the top of the kernel, where their ~30 registers are alive through everything
  const float *w0 = mlp.w0, *b0 = mlp.b0, *w1 = mlp.w1, *b1 = mlp.b1;
  asm volatile("" : "+v"(w0), "+v"(b0), "+v"(w1), "+v"(b1), "+v"(table));
  if (lane < 7) {
    const int e = lane, ax = (e - 1) >> 1;
    const float d = ((e - 1) & 1) ? -eps : eps;
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float v = p[a];
      if (e > 0) v = fminf(fmaxf(v + (a == ax ? d : 0.0f), -radius), radius);   // geometry.py:170
      x[a] = contract(v, radius);
      l_in[e * KIN + a] = x[a] * 2.0f + -1.0f;
    }
#pragma unroll
    for (int l = 0; l < ACT; ++l) {
      const __half2 f = lookup_level(table, m, l, x[0], x[1], x[2]);
      l_in[e * KIN + 3 + 2 * l] = __low2float(f);
      l_in[e * KIN + 4 + 2 * l] = __high2float(f);
      if (enc != nullptr) enc[((size_t)e * n + i) * ACT + l] = f;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  {
    const int j = lane;
#pragma unroll 1
    for (int e = 0; e < 7; ++e) {
      float acc = b0[j];
#pragma unroll
      for (int k = 0; k < KIN; ++k) acc = fmaf(w0[j * DIN + k], l_in[e * KIN + k], acc);
      l_h[e * HID + j] = softplus100(acc);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  // lanes 0..12: the 13 outputs of the centre; lanes 13..18: sdf of the offset evaluations 1..6
  float acc = 0.0f;
  if (lane < 19 && (FEAT || lane == 0 || lane >= NOUT)) {
    const int e = lane < NOUT ? 0 : lane - (NOUT - 1), o = lane < NOUT ? lane : 0;
    acc = b1[o];
#pragma unroll 4
    for (int j = 0; j < HID; ++j) acc = fmaf(w1[o * HID + j], l_h[e * HID + j], acc);
    if (FEAT && lane < NOUT) feature[oi * NOUT + lane] = acc;
  }
  float s[7];
  s[0] = __shfl(acc, 0);
#pragma unroll
  for (int e = 1; e < 7; ++e) s[e] = __shfl(acc, NOUT - 1 + e);
  if (lane == 0) {
    sdf[oi] = s[0];
    if (grad != nullptr) {
      grad[oi * 3 + 0] = 0.5f * (s[1] - s[2]) / eps;
      grad[oi * 3 + 1] = 0.5f * (s[3] - s[4]) / eps;
      grad[oi * 3 + 2] = 0.5f * (s[5] - s[6]) / eps;
    }
    if (laplace != nullptr) {
      const float t0 = s[1] + s[2] - 2.0f * s[0];
      const float t1 = s[3] + s[4] - 2.0f * s[0];
      const float t2 = s[5] + s[6] - 2.0f * s[0];
      laplace[oi] = ((t0 + t1) + t2) / eps2;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the LDS area is reused by the next point
}

// waves per SIMD the register allocation aims at: 4 (128 VGPRs) up to 4 active levels, 3 (168) beyond
constexpr int fwd_waves(int act) { return act <= 4 ? 4 : 3; }

template <int NL, int ACT, int ND, bool FEAT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(fwd_waves(ACT), fwd_waves(ACT))))
void sdf_fd_fwd_shared_kernel(
    const __half2* __restrict__ table, GridMeta m, dsu_sdf_mlp mlp,
    const float* __restrict__ pts, int64_t n, float radius, float eps, float eps2,
    float* __restrict__ sdf, float* __restrict__ grad, float* __restrict__ feature,
    float* __restrict__ laplace, __half2* __restrict__ enc, const int32_t* __restrict__ perm) {
  constexpr int DIN = 3 + 2 * NL;
  const cfloat_t* w0 = as_const(mlp.w0);
  const cfloat_t* b0 = as_const(mlp.b0);
  const cfloat_t* w1 = as_const(mlp.w1);
  const cfloat_t* b1 = as_const(mlp.b1);
  __shared__ float fix_lds[FWD_THREADS / 64][7 * (3 + 2 * ACT) + 7 * HID];
  // the wave iterates together: an irregular point is redone by all its lanes (fd_point_by_wave)
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < n;
       base += (int64_t)gridDim.x * blockDim.x) {
    const bool valid = base + threadIdx.x < n;
    const int64_t i = valid ? base + threadIdx.x : n - 1;
    const float p[3] = {pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2]};
    const int64_t oi = perm ? (int64_t)perm[i] : i;
    // contracted coordinates: q[0] the centre; evaluation e > 0 moves axis (e-1)/2 by +-eps and
    // clamps ALL axes to the box ((points_ + offsets).clamp(-radius, radius), geometry.py:170)
    float q[7][3];
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      q[0][a] = contract(p[a], radius);
      // inside the box: clamping leaves the unmoved axes alone, every evaluation stays in [0, 1]
      bad = bad || !(p[a] >= -radius && p[a] <= radius) || !(q[0][a] >= 0.0f && q[0][a] <= 1.0f);
    }
#pragma unroll
    for (int e = 1; e < 7; ++e) {
      const int ax = (e - 1) >> 1;
      const float d = ((e - 1) & 1) ? -eps : eps;
#pragma unroll
      for (int a = 0; a < 3; ++a) q[e][a] = q[0][a];
      q[e][ax] = contract(fminf(fmaxf(p[ax] + d, -radius), radius), radius);
      bad = bad || !(q[e][ax] >= 0.0f && q[e][ax] <= 1.0f);
    }
    if (bad) {                // addresses of an irregular point are not trusted: park it mid-cube
#pragma unroll
      for (int e = 0; e < 7; ++e)
#pragma unroll
        for (int a = 0; a < 3; ++a) q[e][a] = 0.5f;
    }
    __half2 f[7][ACT];
    fd_levels<ACT, ND>(table, m, q, f, bad, std::make_integer_sequence<int, ACT>{});
    const bool regular = valid && !bad;      // the others compute along and store nothing
    if (enc != nullptr && regular) {
      // interpolated f16 features kept for the backward pass, layout [eval][point][active level]
#pragma unroll
      for (int e = 0; e < 7; ++e) {
        __half2* row = enc + ((size_t)e * n + i) * ACT;
#pragma unroll
        for (int l = 0; l < ACT; ++l) row[l] = f[e][l];
      }
    }
    // ---- MLP: groups of hidden units outer, evaluations inner
    // The six offset evaluations as three (+eps, -eps) pairs in packed-f32 arithmetic (v_pk_fma_f32 /
    // v_pk_mul_f32 / v_pk_add_f32: two IEEE operations per lane and issue slot, the scalar weight
    // broadcast to both halves): the same operations in the same order per evaluation (k ascending
    // for the pre-activations, j ascending for the outputs), so the same bits — the kernel is bound
    // by VALU issue slots (~16 500 per wave and pass, two thirds of them here).
    constexpr int KIN = 3 + 2 * ACT;
    float in0[KIN];
    f32x2 inp[3][KIN];
#pragma unroll
    for (int a = 0; a < 3; ++a) in0[a] = q[0][a] * 2.0f + -1.0f;
#pragma unroll
    for (int l = 0; l < ACT; ++l) {
      in0[3 + 2 * l] = __low2float(f[0][l]);
      in0[4 + 2 * l] = __high2float(f[0][l]);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
        inp[t][a] = f32x2{q[2 * t + 1][a] * 2.0f + -1.0f, q[2 * t + 2][a] * 2.0f + -1.0f};
#pragma unroll
      for (int l = 0; l < ACT; ++l) {
        inp[t][3 + 2 * l] = f32x2{__low2float(f[2 * t + 1][l]), __low2float(f[2 * t + 2][l])};
        inp[t][4 + 2 * l] = f32x2{__high2float(f[2 * t + 1][l]), __high2float(f[2 * t + 2][l])};
      }
    }
    constexpr int NO0 = FEAT ? NOUT : 1;
    float o0[NO0], s[7];
    f32x2 sp[3];
#pragma unroll
    for (int o = 0; o < NO0; ++o) o0[o] = b1[o];
#pragma unroll
    for (int t = 0; t < 3; ++t) sp[t] = splat2(b1[0]);
#pragma unroll 1
    for (int j = 0; j < HID; j += FWD_JB) {
      {
        float h[FWD_JB];
#pragma unroll
        for (int r = 0; r < FWD_JB; ++r) {
          float acc = b0[j + r];
#pragma unroll
          for (int k = 0; k < KIN; ++k) acc = fmaf(w0[(j + r) * DIN + k], in0[k], acc);
          h[r] = softplus100(acc);
        }
#pragma unroll
        for (int o = 0; o < NO0; ++o)
#pragma unroll
          for (int r = 0; r < FWD_JB; ++r) o0[o] = fmaf(w1[o * HID + j + r], h[r], o0[o]);
      }
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        f32x2 h[FWD_JB];
#pragma unroll
        for (int r = 0; r < FWD_JB; ++r) {
          f32x2 acc = splat2(b0[j + r]);
#pragma unroll
          for (int k = 0; k < KIN; ++k)
            acc = __builtin_elementwise_fma(splat2(w0[(j + r) * DIN + k]), inp[t][k], acc);
          h[r] = softplus100_pair(acc);
        }
#pragma unroll
        for (int r = 0; r < FWD_JB; ++r)
          sp[t] = __builtin_elementwise_fma(splat2(w1[j + r]), h[r], sp[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      s[2 * t + 1] = sp[t].x;
      s[2 * t + 2] = sp[t].y;
    }
    s[0] = o0[0];
    if (regular) {
      if (FEAT) {
#pragma unroll
        for (int o = 0; o < NO0; ++o) feature[oi * NOUT + o] = o0[o];
      }
      sdf[oi] = s[0];
      if (grad != nullptr) {
        grad[oi * 3 + 0] = 0.5f * (s[1] - s[2]) / eps;     // geometry.py:173
        grad[oi * 3 + 1] = 0.5f * (s[3] - s[4]) / eps;
        grad[oi * 3 + 2] = 0.5f * (s[5] - s[6]) / eps;
      }
      if (laplace != nullptr) {
        float t0 = s[1] + s[2] - 2.0f * s[0];               // geometry.py:176
        float t1 = s[3] + s[4] - 2.0f * s[0];
        float t2 = s[5] + s[6] - 2.0f * s[0];
        laplace[oi] = ((t0 + t1) + t2) / eps2;
      }
    }
    // the wave's irregular points, one after the other, each by all 64 lanes
    uint64_t todo = __ballot(valid && bad);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t ib = base + (threadIdx.x & ~63) + src;
      const float pb[3] = {pts[ib * 3 + 0], pts[ib * 3 + 1], pts[ib * 3 + 2]};   // (not kept in registers)
      const int64_t oib = perm ? (int64_t)perm[ib] : ib;
      fd_point_by_wave<NL, ACT, FEAT>(table, m, mlp, pb, ib, oib, n, radius, eps, eps2, sdf, grad,
                                      feature, laplace, enc, fix_lds[threadIdx.x >> 6]);
    }
  }
}

// active-level counts the level-outer kernel is instantiated for
constexpr int FWD_SHARED_LO = 4, FWD_SHARED_HI = 7;

template <int... Ks>
void fd_shared_launch(uint32_t active, bool feat, int blocks, hipStream_t s, const __half2* table,
                      const GridMeta& m, const dsu_sdf_mlp& mlp, const float* pts, int64_t n,
                      float radius, float eps, float eps2, float* sdf, float* grad, float* feature,
                      float* laplace, __half2* enc, const int32_t* perm, bool& launched,
                      std::integer_sequence<int, Ks...>) {
  constexpr int ND = 4;        // dense levels of the shipped grid (32 * 1.32^l, 2^19 entries)
  for (int l = 0; l < (int)active; ++l)
    if ((m.hashed[l] != 0) != (l >= ND)) return;
  // the dense levels' index shortcut (one subtraction instead of a modulo) needs
  // x + y res + z res^2 < 2 hsize for every corner (coordinates <= res): checked here, not only by
  // the CPU test of the shipped configuration — another base resolution / table size takes the
  // per-evaluation kernel instead of reading out of range
  for (int l = 0; l < ND && l < (int)active; ++l) {
    const uint64_t res = m.res[l], hsize = (uint64_t)m.off[l + 1] - m.off[l];
    if (res + res * res + res * res * res >= 2 * hsize) return;
  }
  auto one = [&](auto act_c) {
    constexpr int ACT = FWD_SHARED_LO + decltype(act_c)::value;
    if ((int)active != ACT) return;
    if (feat)
      sdf_fd_fwd_shared_kernel<10, ACT, ND, true><<<dim3(blocks), dim3(FWD_THREADS), 0, s>>>(
          table, m, mlp, pts, n, radius, eps, eps2, sdf, grad, feature, laplace, enc, perm);
    else
      sdf_fd_fwd_shared_kernel<10, ACT, ND, false><<<dim3(blocks), dim3(FWD_THREADS), 0, s>>>(
          table, m, mlp, pts, n, radius, eps, eps2, sdf, grad, feature, laplace, enc, perm);
    launched = true;
  };
  (one(std::integral_constant<int, Ks>{}), ...);
}

}  // namespace

namespace dsu_hg {
int make_meta(const dsu_hashgrid_cfg* cfg, GridMeta* m) {
  dsu_hashgrid_levels lv;
  int rc = dsu_hashgrid_make_levels(cfg, &lv);
  if (rc) return rc;
  for (uint32_t l = 0; l <= cfg->n_levels; ++l) m->off[l] = lv.offsets[l];
  for (uint32_t l = 0; l < cfg->n_levels; ++l) {
    m->res[l] = lv.resolution[l];
    m->scale[l] = lv.scale[l];
    m->hashed[l] = lv.hashed[l];
  }
  return DSU_OK;
}
}  // namespace dsu_hg

#define DSU_DISPATCH_NL(nl, ...)          \
  switch (nl) {                            \
    case 10: { constexpr int NL = 10; __VA_ARGS__ } break; \
    case 12: { constexpr int NL = 12; __VA_ARGS__ } break; \
    default: return DSU_EUNSUP;            \
  }

extern "C" {

int dsu_hashgrid_make_levels(const dsu_hashgrid_cfg* cfg, dsu_hashgrid_levels* out) {
  if (!cfg || !out) return DSU_EINVAL;
  if (cfg->n_levels == 0 || cfg->n_levels > DSU_MAX_LEVELS) return DSU_EINVAL;
  if (cfg->n_features != 2) return DSU_EUNSUP;
  if (cfg->log2_hashmap_size < 3 || cfg->log2_hashmap_size > 28) return DSU_EINVAL;
  const double l2 = log2(cfg->per_level_scale);
  uint32_t offset = 0;
  for (uint32_t l = 0; l < cfg->n_levels; ++l) {
    const float scale = (float)(exp2((double)l * l2) * (double)cfg->base_resolution - 1.0);
    const uint32_t res = (uint32_t)ceilf(scale) + 1u;
    const uint32_t max_params = 0xFFFFFFFFu / 2;
    const double cube = (double)res * (double)res * (double)res;
    uint32_t params = cube > (double)max_params ? max_params : (uint32_t)cube;
    params = (params + 7u) / 8u * 8u;
    const uint32_t hsize = 1u << cfg->log2_hashmap_size;
    if (params > hsize) params = hsize;
    out->offsets[l] = offset;
    out->resolution[l] = res;
    out->scale[l] = scale;
    out->hashed[l] = cube > (double)params ? 1u : 0u;
    offset += params;
  }
  out->offsets[cfg->n_levels] = offset;
  return DSU_OK;
}

int dsu_hashgrid_encode_fwd(const dsu_hashgrid_cfg* cfg, const void* table_f16, const float* x,
                            int64_t n, uint32_t active_levels, void* out_f16, void* stream) {
  if (!cfg || !table_f16 || (!x && n) || (!out_f16 && n) || n < 0) return DSU_EINVAL;
  if (active_levels > cfg->n_levels) return DSU_EINVAL;
  GridMeta m;
  int rc = make_meta(cfg, &m);
  if (rc) return rc;
  if (n == 0) return DSU_OK;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = dsu_capped_blocks(n, 256, 8192);
  DSU_DISPATCH_NL(cfg->n_levels, {
    encode_fwd_kernel<NL><<<dim3(blocks), dim3(256), 0, s>>>(
        (const __half2*)table_f16, m, x, n, active_levels, (__half2*)out_f16);
  });
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_hashgrid_encode_bwd(const dsu_hashgrid_cfg* cfg, const float* x, const float* dout,
                            int64_t n, uint32_t active_levels, float* grad_table,
                            void* stream) {
  if (!cfg || (!x && n) || (!dout && n) || !grad_table || n < 0) return DSU_EINVAL;
  if (active_levels > cfg->n_levels) return DSU_EINVAL;
  GridMeta m;
  int rc = make_meta(cfg, &m);
  if (rc) return rc;
  if (n == 0 || active_levels == 0) return DSU_OK;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = dsu_capped_blocks(n, 256, 4096);
  encode_bwd_kernel<<<dim3(blocks, active_levels), dim3(256), 0, s>>>(
      m, (int)cfg->n_levels, x, dout, n, grad_table);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_sdf_fwd(const dsu_hashgrid_cfg* cfg, const void* table_f16, const dsu_sdf_mlp* mlp,
                const float* pts, int64_t n, float radius, uint32_t active_levels,
                uint32_t n_out, float* out, void* stream) {
  if (!cfg || !table_f16 || !mlp || (!pts && n) || (!out && n) || n < 0) return DSU_EINVAL;
  if (!mlp->w0 || !mlp->b0 || !mlp->w1 || !mlp->b1) return DSU_EINVAL;
  if (active_levels > cfg->n_levels) return DSU_EINVAL;
  if (n_out != 1 && n_out != NOUT) return DSU_EUNSUP;
  GridMeta m;
  int rc = make_meta(cfg, &m);
  if (rc) return rc;
  if (n == 0) return DSU_OK;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = dsu_capped_blocks(n, FWD_THREADS, 8192);
  DSU_DISPATCH_NL(cfg->n_levels, {
    if (n_out == 1)
      sdf_fwd_kernel<NL, 1><<<dim3(blocks), dim3(FWD_THREADS), 0, s>>>(
          (const __half2*)table_f16, m, *mlp, pts, n, radius, active_levels, out, SdfLattice{});
    else
      sdf_fwd_kernel<NL, NOUT><<<dim3(blocks), dim3(FWD_THREADS), 0, s>>>(
          (const __half2*)table_f16, m, *mlp, pts, n, radius, active_levels, out, SdfLattice{});
  });
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_sdf_fwd_lattice(const dsu_hashgrid_cfg* cfg, const void* table_f16, const dsu_sdf_mlp* mlp,
                        const float* lin, int32_t res, int32_t x0, int32_t nx, const float* lo3,
                        const float* span3, float radius, uint32_t active_levels, float* out,
                        void* stream) {
  if (!cfg || !table_f16 || !mlp || !lin || !lo3 || !span3 || !out || res < 1 || x0 < 0 || nx < 0 ||
      x0 + nx > res)
    return DSU_EINVAL;
  if (!mlp->w0 || !mlp->b0 || !mlp->w1 || !mlp->b1) return DSU_EINVAL;
  if (active_levels > cfg->n_levels) return DSU_EINVAL;
  GridMeta m;
  int rc = make_meta(cfg, &m);
  if (rc) return rc;
  const int64_t n = (int64_t)nx * res * res;
  if (n == 0) return DSU_OK;
  SdfLattice lat{lin, res, x0, {lo3[0], lo3[1], lo3[2]}, {span3[0], span3[1], span3[2]}};
  hipStream_t s = (hipStream_t)stream;
  const int blocks = dsu_capped_blocks(n, FWD_THREADS, 8192);
  DSU_DISPATCH_NL(cfg->n_levels, {
    sdf_fwd_kernel<NL, 1, true><<<dim3(blocks), dim3(FWD_THREADS), 0, s>>>(
        (const __half2*)table_f16, m, *mlp, nullptr, n, radius, active_levels, out, lat);
  });
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_sdf_fd_fwd_sorted(const dsu_hashgrid_cfg* cfg, const void* table_f16, const dsu_sdf_mlp* mlp,
                   const float* pts, const int32_t* perm, int64_t n, float radius, float eps,
                   uint32_t active_levels, float* sdf, float* grad, float* feature,
                   float* laplace, void* enc_cache, void* stream) {
  if (!cfg || !table_f16 || !mlp || (!pts && n) || (!sdf && n) || n < 0) return DSU_EINVAL;
  if (!mlp->w0 || !mlp->b0 || !mlp->w1 || !mlp->b1) return DSU_EINVAL;
  if (active_levels > cfg->n_levels || !(eps > 0.0f)) return DSU_EINVAL;
  GridMeta m;
  int rc = make_meta(cfg, &m);
  if (rc) return rc;
  if (n == 0) return DSU_OK;
  hipStream_t s = (hipStream_t)stream;
  const float eps2 = (float)((double)eps * (double)eps);
  const int blocks = dsu_capped_blocks(n, FWD_THREADS, 8192);
  // level-outer kernel with shared corners: one instance per number of active levels of the
  // shipped grid (10 levels; the 3000-step schedule runs 4..6 of them, geometry.py:196-215);
  // anything else takes the evaluation-by-evaluation kernel below
  if (cfg->n_levels == 10 && active_levels >= FWD_SHARED_LO && active_levels <= FWD_SHARED_HI) {
    bool launched = false;
    fd_shared_launch(active_levels, feature != nullptr, blocks, s, (const __half2*)table_f16, m, *mlp,
                     pts, n, radius, eps, eps2, sdf, grad, feature, laplace, (__half2*)enc_cache, perm,
                     launched, std::make_integer_sequence<int, FWD_SHARED_HI - FWD_SHARED_LO + 1>{});
    if (launched) {
      DSU_CHECK_LAUNCH();
      return DSU_OK;
    }
  }
  DSU_DISPATCH_NL(cfg->n_levels, {
    if (active_levels <= 6)
      sdf_fd_fwd_kernel<NL, 6><<<dim3(blocks), dim3(FWD_THREADS), 0, s>>>(
          (const __half2*)table_f16, m, *mlp, pts, n, radius, eps, eps2, active_levels, sdf, grad,
          feature, laplace, (__half2*)enc_cache, perm);
    else
      sdf_fd_fwd_kernel<NL, NL><<<dim3(blocks), dim3(FWD_THREADS), 0, s>>>(
          (const __half2*)table_f16, m, *mlp, pts, n, radius, eps, eps2, active_levels, sdf, grad,
          feature, laplace, (__half2*)enc_cache, perm);
  });
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

}  // extern "C"
