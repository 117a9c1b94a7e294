// Level of detail, trilinear and anisotropic sampling of the atlas pyramid (include/dsu_hip.h,
// "Mip-mapped frames" and "Anisotropic frames"): one text for the resolve of mesh_render.hip (device)
// and for dsu_mip_sample_host / dsu_aniso_sample_host (host), so the non-GPU suite pins the arithmetic
// the kernel runs.  Everything is float64 in the operand
// order written here; the library is compiled with -ffp-contract=off, so no products are fused on
// either side.  tests/frame_render_mip_ref.py and
// tests/frame_render_aniso_ref.py restate it in numpy.
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

// One trilinear read: tx, ty = uv T; (k, t) from lod(); at = level_offset(T, k).  V = B_k, or
// (1 - t) B_k + t B_{k+1}, per channel, goes to out[ch] through put(): divided by 255 and rounded once
// to f32 for the trilinear filter's colour (sample), as it is for the anisotropic filter's sum
// (sample_aniso).  A template over the output type and not a value array or a callback: with either of
// those the compiler schedules the plain trilinear kernels of mesh_render.hip differently.
DSU_MIP_HD void put(float& out, double V) { out = (float)(V / 255.0); }
DSU_MIP_HD void put(double& out, double V) { out = V; }

template <class Out>
DSU_MIP_HD void trilinear(const uint32_t* __restrict__ pyramid, int T, double tx, double ty, int k, double t,
                          int64_t at, Out out[3]) {
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
    for (int ch = 0; ch < 3; ++ch) put(out[ch], B0[ch]);
    return;
  }
  const double half1 = ((double)(2 << k) - 1.0) * 0.5, inv1 = ldexp(1.0, -(k + 1));
  double B1[3];
  blend(pyramid + at + (int64_t)Tk * Tk, (Tk + 1) >> 1, (x0 - half1) * inv1, (y0 - half1) * inv1, B1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) put(out[ch], (1.0 - t) * B0[ch] + t * B1[ch]);
}

// Colour of one sample under the trilinear rule.
DSU_MIP_HD void sample(const uint32_t* __restrict__ pyramid, int T, double tx, double ty, int k, double t,
                       int64_t at, float rgb[3]) {
  trilinear(pyramid, T, tx, ty, k, t, at, rgb);
}

// ---- anisotropic frames (include/dsu_hip.h, "Anisotropic frames"; tests/frame_render_aniso_ref.py)
constexpr int MAX_ANISO = 16;

// What one (frame, face) hands its samples: the major axis of the footprint (unit, in tx, ty), its
// length s1 in level-0 texels, the number of probes N along it, and the level (k, t) of one probe's
// footprint rho = s1 / N.
struct AnisoFace {
  double s1 = 0.0, ax = 1.0, ay = 0.0, rho = 0.0, t = 0.0;
  int N = 1, k = 0;
};

// The arguments of footprint(), the cap on N (1 .. MAX_ANISO) and the number of levels L.
DSU_MIP_HD AnisoFace footprint_aniso(double ax, double ay, double bx, double by, double cx, double cy, float ua,
                                     float va, float ub, float vb, float uc, float vc, int T, double h, int cap,
                                     int L) {
  AnisoFace f;
  const double e1x = bx - ax, e1y = by - ay, e2x = cx - ax, e2y = cy - ay;
  const double p1 = ((double)ub - (double)ua) * (double)T, q1 = ((double)vb - (double)va) * (double)T;
  const double p2 = ((double)uc - (double)ua) * (double)T, q2 = ((double)vc - (double)va) * (double)T;
  const double det = e1x * e2y - e1y * e2x;
  if (det == 0.0) return f;
  const double dpx = (p1 * e2y - p2 * e1y) / det, dpy = (p2 * e1x - p1 * e2x) / det;
  const double dqx = (q1 * e2y - q2 * e1y) / det, dqy = (q2 * e1x - q1 * e2x) / det;
  const double hh = h * h;
  const double A = hh * (dpx * dpx + dpy * dpy), C = hh * (dqx * dqx + dqy * dqy);
  const double B = hh * (dpx * dqx + dpy * dqy), D = hh * (dpx * dqy - dpy * dqx);
  const double m = (A + C) * 0.5, d = (A - C) * 0.5;
  const double r = sqrt(d * d + B * B);
  const double s1 = sqrt(m + r);
  if (!finite(A) || !finite(B) || !finite(C) || !finite(D) || !finite(r) || !finite(s1)) return f;
  const double s2 = fabs(D) / s1;                  // from the determinant: m - r cancels
  const double vx = d >= 0.0 ? d + r : B, vy = d >= 0.0 ? B : r - d;   // neither form cancels
  const double n = sqrt(vx * vx + vy * vy);
  if (n != 0.0 && finite(n)) {
    f.ax = vx / n;
    f.ay = vy / n;
  }
  f.s1 = s1;
  if (!(s1 > 1.0)) f.N = 1;
  else if (!(s2 > 0.0)) f.N = cap;
  else {
    const double q = ceil(s1 / s2);
    f.N = q < (double)cap ? (int)q : cap;
  }
  f.rho = s1 / (double)f.N;
  lod(f.rho, L, f.k, f.t);
  return f;
}

// Colour of one sample under the anisotropic rule: N probes along the axis, their unrounded trilinear
// values summed in ascending order, one rounding to f32.  at = level_offset(T, k).
DSU_MIP_HD void sample_aniso(const uint32_t* __restrict__ pyramid, int T, double tx, double ty, double s1, int N,
                             double ax, double ay, int k, double t, int64_t at, float rgb[3]) {
  double sum[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < N; ++i) {
    const double o = ((double)(2 * i + 1) / (double)(2 * N) - 0.5) * s1;
    double V[3];
    trilinear(pyramid, T, tx + o * ax, ty + o * ay, k, t, at, V);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sum[ch] += V[ch];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) rgb[ch] = (float)((sum[ch] / (double)N) / 255.0);
}

}  // namespace dsu_mip
