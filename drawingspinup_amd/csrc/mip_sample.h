// Level of detail and trilinear sampling of the atlas pyramid (include/dsu_hip.h, "Mip-mapped
// frames"): one text for the resolve of mesh_render.hip (device) and for dsu_mip_sample_host (host),
// so the non-GPU suite pins the arithmetic the kernel runs.  Everything is float64 in the operand
// order written here; the library is compiled with -ffp-contract=off, so no products are fused on
// either side.  tests/frame_render_mip_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#define DSU_MIP_HD __host__ __device__ __forceinline__

namespace dsu_mip {

constexpr int MAX_T = 8192;

// T_0 = T, T_k = ceil(T_{k-1} / 2) = ceil(T / 2^k); L levels down to and including size 1.
DSU_MIP_HD int level_size(int T, int k) { return (int)(((int64_t)T + (((int64_t)1 << k) - 1)) >> k); }
DSU_MIP_HD int levels(int T) {
  int L = 1;
  for (; T > 1; T = (T + 1) >> 1) ++L;
  return L;
}
// texel offset of level k in the pyramid buffer: sum of T_j^2 over j < k (below 2^27 for T <= 8192)
DSU_MIP_HD int64_t level_offset(int T, int k) {
  int64_t at = 0;
  for (int j = 0; j < k; ++j, T = (T + 1) >> 1) at += (int64_t)T * T;
  return at;
}

DSU_MIP_HD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// Texel footprint rho of one sub-sample on a face: screen vertices a, b, c (x, y), their uvs, the
// atlas side T and the sample spacing h = span / N.  0 where the face has no screen area.
DSU_MIP_HD double footprint(double ax, double ay, double bx, double by, double cx, double cy, float ua, float va,
                            float ub, float vb, float uc, float vc, int T, double h) {
  const double e1x = bx - ax, e1y = by - ay, e2x = cx - ax, e2y = cy - ay;
  const double p1 = ((double)ub - (double)ua) * (double)T, q1 = ((double)vb - (double)va) * (double)T;
  const double p2 = ((double)uc - (double)ua) * (double)T, q2 = ((double)vc - (double)va) * (double)T;
  const double det = e1x * e2y - e1y * e2x;
  if (det == 0.0) return 0.0;
  const double dpx = (p1 * e2y - p2 * e1y) / det, dpy = (p2 * e1x - p1 * e2x) / det;
  const double dqx = (q1 * e2y - q2 * e1y) / det, dqy = (q2 * e1x - q1 * e2x) / det;
  const double gx = dpx * dpx + dqx * dqx, gy = dpy * dpy + dqy * dqy;
  return sqrt((h * h) * (gx > gy ? gx : gy));
}

// rho -> level k and blend weight t in [0, 1): linear in rho inside an octave.
DSU_MIP_HD void lod(double rho, int L, int& k, double& t) {
  k = 0;
  t = 0.0;
  if (!finite(rho) || !(rho > 1.0)) return;
  const int e = ilogb(rho);                      // floor(log2 rho), from the exponent
  if (e >= L - 1) {
    k = L - 1;
    return;
  }
  k = e;
  t = ldexp(rho, -e) - 1.0;
}

// The four-term blend of one level, the bilinear filter's expression before its division and
// rounding.  level: T_j x T_j RGBA8 words; x, y already in that level's coordinates.
DSU_MIP_HD void blend(const uint32_t* __restrict__ level, int Tj, double x, double y, double B[3]) {
  const double top = (double)(Tj - 1);
  x = fmin(fmax(x, 0.0), top);
  y = fmin(fmax(y, 0.0), top);
  const int c0 = (int)floor(x), r0 = (int)floor(y);
  const int c1 = c0 + 1 < Tj ? c0 + 1 : Tj - 1, r1 = r0 + 1 < Tj ? r0 + 1 : Tj - 1;
  const double fx = x - (double)c0, fy = y - (double)r0;
  const uint32_t p00 = level[(int64_t)r0 * Tj + c0], p01 = level[(int64_t)r0 * Tj + c1];
  const uint32_t p10 = level[(int64_t)r1 * Tj + c0], p11 = level[(int64_t)r1 * Tj + c1];
  const double k00 = (1.0 - fx) * (1.0 - fy), k01 = fx * (1.0 - fy), k10 = (1.0 - fx) * fy, k11 = fx * fy;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    B[ch] = k00 * (double)(float)((p00 >> (8 * ch)) & 255u) + k01 * (double)(float)((p01 >> (8 * ch)) & 255u) +
            k10 * (double)(float)((p10 >> (8 * ch)) & 255u) + k11 * (double)(float)((p11 >> (8 * ch)) & 255u);
}

// Colour of one sample: tx, ty = uv T; (k, t) from lod(); at = level_offset(T, k).
DSU_MIP_HD void sample(const uint32_t* __restrict__ pyramid, int T, double tx, double ty, int k, double t,
                       int64_t at, float rgb[3]) {
  if (!finite(tx)) tx = 0.0;
  if (!finite(ty)) ty = 0.0;
  const double x0 = tx, y0 = (double)(T - 1) - ty;
  const int Tk = level_size(T, k);
  // a level-j texel sits at the centre of its block of level-0 points: x_j = (x_0 - (2^j - 1) / 2) / 2^j;
  // the division by a power of two is written as the (exact) product with its inverse
  const double half = ((double)(1 << k) - 1.0) * 0.5, inv = ldexp(1.0, -k);
  double B0[3];
  blend(pyramid + at, Tk, (x0 - half) * inv, (y0 - half) * inv, B0);
  if (t == 0.0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = (float)(B0[ch] / 255.0);
    return;
  }
  const double half1 = ((double)(2 << k) - 1.0) * 0.5, inv1 = ldexp(1.0, -(k + 1));
  double B1[3];
  blend(pyramid + at + (int64_t)Tk * Tk, (Tk + 1) >> 1, (x0 - half1) * inv1, (y0 - half1) * inv1, B1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) rgb[ch] = (float)(((1.0 - t) * B0[ch] + t * B1[ch]) / 255.0);
}

}  // namespace dsu_mip
