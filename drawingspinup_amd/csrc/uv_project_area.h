// The drawings projected into the atlas (include/dsu_hip.h, UV export e. and j.: e. is j. at s = 1,
// filter 0): everything one texel does, one text for the kernel of uv_project_area.hip (device) and
// for dsu_uv_project_area_host (host), so the non-GPU suite pins the arithmetic the kernel runs.  Float64 in the operand order
// written here; the library is compiled with -ffp-contract=off, so no products are fused on either
// side.  tests/uv_project_area_ref.py restates it in numpy.
//
// The cost is the occluder walk.  The s x s sub-samples of a texel are taken GROUP at a time, in
// ascending j: the points of a group sit in registers, the cells of the group's points are walked
// once each (a cell that an earlier point of the group already named is skipped) and every listed
// triangle is tested against all points of the group that are still unoccluded.  A triangle met
// through another point's cell, or twice, changes nothing: occlusion is an OR, and a triangle that
// covers a point is in that point's own list anyway.  A texel is about a quarter of a cell wide, so
// a group nearly always walks one list: s = 2 walks once, s = 4 four times instead of sixteen.
//
// What the sharing buys is the loads, and the loads are not where the time goes: measured on an
// MI355X (profiles/uv_project_area_probe.json) the kernel costs about as much per sub-sample as
// the one-point instantiation costs per texel.  The time is the float64 edge functions of every listed
// triangle at every point, on lanes that each walk a list of their own.  Tried and measured on the
// same probe, none kept: a box reject per triangle before the edge functions (12 % faster, with
// SGPR spills: some lane of a wave nearly always passes, so the wave runs the test anyway); eight
// points per group (197 VGPR, slower); one walk per texel for all sub-samples with the points
// recomputed where a triangle passes the box (three times slower, for the same reason).  What did
// pay is shorter lists: ops.uv_project_area builds a grid three times finer than ZGrid's default.
//
// s = 1 is texel<true>: one point, a group of one, no step 6.  It walks as the grouped text does, in
// 58 VGPR instead of 148 (8 waves per SIMD instead of 3): 62 us where the grouped text took 85 on
// the 160-cell grid of the 51 200-face probe (profiles/uv_project_unified_probe.json).
#pragma once
#include <math.h>
#include <stdint.h>
#include "mesh_geom.h"
#include "uv_field.h"

#define DSU_UVP_HD __host__ __device__ __forceinline__

namespace dsu_uvp {

constexpr int MAX_S = dsu_uvf::MAX_S;
constexpr int GROUP = 4;                             // points in registers at a time: 12 float64

// What every texel reads and writes.
struct Args {
  const float* __restrict__ uvs;
  const int32_t* __restrict__ indices;
  const float* __restrict__ pos;
  int64_t V, M;
  int32_t S;
  const int32_t* __restrict__ face_id;
  const float* __restrict__ tris;
  ZGrid gr;
  const int32_t* __restrict__ offsets;
  const int32_t* __restrict__ items;
  const uint8_t* __restrict__ colour_front;
  const uint8_t* __restrict__ mask_front;
  const uint8_t* __restrict__ colour_back;
  const uint8_t* __restrict__ mask_back;
  int32_t res;
  double tolerance;
  int32_t s, filter;
  uint8_t* __restrict__ image;
  uint8_t* __restrict__ source;
  uint8_t* __restrict__ count;                       // or NULL
};

DSU_UVP_HD double clamp(double v, double hi) { return v < 0.0 ? 0.0 : (v > hi ? hi : v); }

// e.'s pixel: nearest (half to even), clamped
DSU_UVP_HD int64_t nearest(double px, double py, bool back, int32_t res) {
  const double span = (double)(res - 1);
  const double X = clamp(rint(((back ? -px : px) + 0.5) * span), span);
  const double Y = clamp(rint((-py + 0.5) * span), span);
  return (int64_t)Y * res + (int64_t)X;
}

// floor(v + 0.5) clipped to [0, 255]
DSU_UVP_HD uint8_t round_byte(double v) {
  v = floor(v + 0.5);
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (uint8_t)(int)v;
}

// step 5: the three values of a passing sub-sample at p, added to sum
DSU_UVP_HD void add_value(const uint8_t* __restrict__ colour, int32_t res, int32_t filter, bool back, double px,
                          double py, double sum[3]) {
  if (filter == 0) {
    const uint8_t* __restrict__ q = colour + nearest(px, py, back, res) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sum[ch] += (double)q[ch];
    return;
  }
  const double span = (double)(res - 1);
  const double fx = clamp(((back ? -px : px) + 0.5) * span, span), fy = clamp((-py + 0.5) * span, span);
  const int32_t top = res >= 2 ? res - 2 : 0;
  int32_t x0 = (int32_t)floor(fx), y0 = (int32_t)floor(fy);
  x0 = x0 < top ? x0 : top;
  y0 = y0 < top ? y0 : top;
  const int32_t x1 = x0 + 1 < res - 1 ? x0 + 1 : res - 1, y1 = y0 + 1 < res - 1 ? y0 + 1 : res - 1;
  const double tx = fx - (double)x0, ty = fy - (double)y0;
  const uint8_t* __restrict__ r0 = colour + (int64_t)y0 * res * 3;
  const uint8_t* __restrict__ r1 = colour + (int64_t)y1 * res * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double c00 = (double)r0[x0 * 3 + ch], c10 = (double)r0[x1 * 3 + ch];
    const double c01 = (double)r1[x0 * 3 + ch], c11 = (double)r1[x1 * 3 + ch];
    sum[ch] += ((1.0 - ty) * ((1.0 - tx) * c00 + tx * c10)) + (ty * ((1.0 - tx) * c01 + tx * c11));
  }
}

// Sub-samples j0 .. j0 + nj - 1 (nj <= G) of the s x s grid about (x, y), on face m with atlas
// triangle t and positions A, B, C: steps 3 to 5, with G points in registers.  The passing ones add
// their values to sum in ascending j; -> how many passed.
template <int G>
DSU_UVP_HD int group(const Args& a, const TriXY& t, const double A[3], const double B[3], const double C[3],
                     int32_t m, bool back, double x, double y, int32_t s, int32_t j0, int32_t nj, double sum[3]) {
  const uint8_t* __restrict__ mask = back ? a.mask_back : a.mask_front;
  const double sign = back ? -1.0 : 1.0;
  double p[G][3];
  int32_t cell[G];
  unsigned todo = 0;                                 // bit k: point k has passed every test so far
#pragma unroll
  for (int k = 0; k < G; ++k) {
    p[k][0] = p[k][1] = p[k][2] = 0.0;
    cell[k] = 0;
    if (k >= nj) continue;
    const int32_t j = j0 + k, jy = j / s, jx = j - jy * s;
    double w0, w1, w2;
    uv_edges(t, x + dsu_uvf::offset(jx, s), y + dsu_uvf::offset(jy, s), w0, w1, w2);
    const double area = (w0 + w1) + w2;
    const double b0 = w0 / area, b1 = w1 / area, b2 = w2 / area;             // not clamped
#pragma unroll
    for (int i = 0; i < 3; ++i) p[k][i] = (b0 * A[i] + b1 * B[i]) + b2 * C[i];
    if (!(dsu_uvf::finite(p[k][0]) && dsu_uvf::finite(p[k][1]) && dsu_uvf::finite(p[k][2]))) continue;
    if (!(mask[nearest(p[k][0], p[k][1], back, a.res)] > 0)) continue;
    cell[k] = cell_of((float)p[k][1], a.gr.y0, a.gr.inv_cell, a.gr.g) * a.gr.g +
              cell_of((float)p[k][0], a.gr.x0, a.gr.inv_cell, a.gr.g);
    todo |= 1u << k;
  }
  unsigned walked = 0;                               // bit k: point k's cell has been walked
#pragma unroll
  for (int k = 0; k < G; ++k) {
    if (!((todo >> k) & 1u)) continue;               // failed or occluded by now: nobody needs its list
    bool seen = false;
#pragma unroll
    for (int e = 0; e < k; ++e) seen = seen || (((walked >> e) & 1u) && cell[e] == cell[k]);
    // an earlier walk of this cell ran to its end unless it ended with nothing left to test
    if (seen) continue;
    walked |= 1u << k;
    const int32_t end = a.offsets[cell[k] + 1];
    for (int32_t i = a.offsets[cell[k]]; i < end && todo; ++i) {
      const int32_t f = a.items[i];
      if (f == m || f < 0 || f >= a.M) continue;
      const float* __restrict__ tf = a.tris + (int64_t)f * 9;
      const TriXY xy{tf[0], tf[1], tf[3], tf[4], tf[6], tf[7]};
      // A group widens the triangle's z once for all its points.  A lone point reads it only under a
      // triangle that covers it: few do, and with the loads behind that branch the division stays
      // there too, which the compiler otherwise runs for every listed triangle (62 against 85 us)
      double z0 = 0.0, z1 = 0.0, z2 = 0.0;
      if (G > 1) z0 = (double)tf[2], z1 = (double)tf[5], z2 = (double)tf[8];
#pragma unroll
      for (int q = 0; q < G; ++q) {
        if (!((todo >> q) & 1u)) continue;
        double e0, e1, e2;
        edge_functions(xy, p[q][0], p[q][1], e0, e1, e2);
        const double ar = (e0 + e1) + e2;
        if (ar == 0.0 || !covers(e0, e1, e2)) continue;
        if (G == 1) z0 = (double)tf[2], z1 = (double)tf[5], z2 = (double)tf[8];
        const double z = ((e0 * z0 + e1 * z1) + e2 * z2) / ar;
        if ((z - p[q][2]) * sign > a.tolerance) todo &= ~(1u << q);
      }
    }
  }
  int n = 0;
  const uint8_t* __restrict__ colour = back ? a.colour_back : a.colour_front;
#pragma unroll
  for (int k = 0; k < G; ++k) {
    if (!((todo >> k) & 1u)) continue;
    add_value(colour, a.res, a.filter, back, p[k][0], p[k][1], sum);
    ++n;
  }
  return n;
}

// Which of the two instantiations of texel() a call runs: every entry asks here, the host entry
// included, so the host runs the instantiation the kernel runs.
inline bool one_point(const Args& a) { return a.s == 1; }

// Texel (row r, column c): its three bytes, its source and its count.  ONE: a.s is 1, so the
// texel's own point is its only sample (rule e. when the filter is 0), alone in its group, and
// step 6 has nothing to add.
template <bool ONE>
DSU_UVP_HD void texel(const Args& a, int32_t r, int32_t c) {
  constexpr int G = ONE ? 1 : GROUP;
  const int32_t s = ONE ? 1 : a.s;
  const int64_t at = (int64_t)r * a.S + c;
  uint8_t out[3] = {0, 0, 0}, src = 0, cnt = 0;
  const int32_t m = a.face_id[at];
  int ia, ib, ic;
  if (m >= 0 && m < a.M && face_indices(a.indices, m, a.V, ia, ib, ic)) {
    double A[3], B[3], C[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      A[k] = a.pos[(int64_t)ia * 3 + k];
      B[k] = a.pos[(int64_t)ib * 3 + k];
      C[k] = a.pos[(int64_t)ic * 3 + k];
    }
    const double nz = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0]);
    if (nz > 0.0 || nz < 0.0) {                      // a NaN faces neither view
      const bool back = nz < 0.0;
      const TriXY t = uv_tri(a.uvs, ia, ib, ic, (double)a.S);
      const double x = (double)c, y = (double)(a.S - 1 - r);
      double sum[3] = {0.0, 0.0, 0.0};
      int n = 0;
      const int32_t ss = s * s;
      for (int32_t j0 = 0; j0 < ss; j0 += G)
        n += group<G>(a, t, A, B, C, m, back, x, y, s, j0, ss - j0 < G ? ss - j0 : G, sum);
      cnt = (uint8_t)n;
      // step 6: the texel's own point; an odd grid has it as its centre sample already
      if (!ONE && n == 0 && !(s & 1)) n = group<1>(a, t, A, B, C, m, back, x, y, 1, 0, 1, sum);
      if (n > 0) {
        src = back ? 2 : 1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[ch] = round_byte(sum[ch] / (double)n);
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) a.image[at * 3 + ch] = out[ch];
  a.source[at] = src;
  if (a.count) a.count[at] = cnt;
}

}  // namespace dsu_uvp
