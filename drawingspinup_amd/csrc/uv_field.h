// The radiance field in the atlas (include/dsu_hip.h, UV export f. and g.): the point of one
// (texel, sub-sample) and the byte of one texel, one text for the kernels of mesh_uv.hip (device)
// and for dsu_uv_field_points_host / dsu_uv_field_resolve_host (host), so the non-GPU suite pins
// the arithmetic the kernels run.  Everything is float64 in the operand order written here; the
// library is compiled with -ffp-contract=off, so no products are fused on either side.
// tests/uv_field_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>
#include "mesh_geom.h"

#define DSU_UVF_HD __host__ __device__ __forceinline__

namespace dsu_uvf {

constexpr int MAX_S = 8;

DSU_UVF_HD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN
DSU_UVF_HD bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }

// o(i) = (2 i + 1 - s) / (2 s): the sub-sample's offset from the texel's own sample point
DSU_UVF_HD double offset(int i, int s) { return (double)(2 * i + 1 - s) / (double)(2 * s); }

// Sub-sample j of the texel with linear index `texel`: the point on (the affine extension of) the
// texel's face, in the frame of `positions`.  false: nothing to evaluate, out = (0, 0, 0).
DSU_UVF_HD bool point(const float* __restrict__ uvs, const int32_t* __restrict__ indices,
                      const float* __restrict__ positions, int64_t V, int64_t M, int32_t S,
                      const int32_t* __restrict__ face_id, int32_t texel, int32_t s, int32_t j, float out[3]) {
  out[0] = out[1] = out[2] = 0.0f;
  if (texel < 0 || (int64_t)texel >= (int64_t)S * S) return false;
  const int32_t m = face_id[texel];
  if (m < 0 || m >= M) return false;
  int ia, ib, ic;
  if (!face_indices(indices, m, V, ia, ib, ic)) return false;
  const int32_t r = texel / S, c = texel - r * S;
  const int32_t jy = j / s, jx = j - jy * s;
  const double px = (double)c + offset(jx, s), py = (double)(S - 1 - r) + offset(jy, s);
  const TriXY t = uv_tri(uvs, ia, ib, ic, (double)S);
  double w0, w1, w2;
  uv_edges(t, px, py, w0, w1, w2);                   // dsu_uv_bake's edge functions
  const double area = (w0 + w1) + w2;
  if (!finite(area) || !(area > 0.0)) return false;
  const double b0 = w0 / area, b1 = w1 / area, b2 = w2 / area;   // not clamped
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double v = (b0 * (double)positions[(int64_t)ia * 3 + k] + b1 * (double)positions[(int64_t)ib * 3 + k]) +
                     b2 * (double)positions[(int64_t)ic * 3 + k];
    p[k] = (float)v;
  }
  if (!finite_f(p[0]) || !finite_f(p[1]) || !finite_f(p[2])) return false;
  out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
  return true;
}

// dsu_uv_bake's quantisation
DSU_UVF_HD uint8_t quantise(double v) {
  v = v * 255.0;
  if (!(v == v)) return 0;                           // the reference's nan -> 0
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (uint8_t)(int)v;                            // truncation, as astype(np.uint8)
}

// Texel number t of the list: the mean of its valid samples into image, or nothing.
DSU_UVF_HD void resolve(const float* __restrict__ colours, const uint8_t* __restrict__ valid, int64_t t, int32_t ss,
                        int32_t S, int32_t texel, uint8_t* __restrict__ image) {
  if (texel < 0 || (int64_t)texel >= (int64_t)S * S) return;
  double sum[3] = {0.0, 0.0, 0.0};
  int n = 0;
  for (int j = 0; j < ss; ++j) {
    if (!valid[t * ss + j]) continue;
    const float* __restrict__ q = colours + (t * ss + j) * 3;
    sum[0] += (double)q[0];
    sum[1] += (double)q[1];
    sum[2] += (double)q[2];
    ++n;
  }
  if (n == 0) return;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) image[(int64_t)texel * 3 + ch] = quantise(sum[ch] / (double)n);
}

}  // namespace dsu_uvf
