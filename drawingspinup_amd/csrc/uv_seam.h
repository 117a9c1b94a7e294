// Seam levelling in the atlas (include/dsu_hip.h, UV export h. and i.): what one texel adds to the
// per-group sums and the bytes one texel of the composed image gets, one text for the kernels of
// mesh_uv.hip (device) and for dsu_uv_seam_gather_host / dsu_uv_seam_apply_host (host), so the
// non-GPU suite pins the arithmetic the kernels run.  Float64 and 64-bit integers in the operand
// order written here; the library is compiled with -ffp-contract=off, so no products are fused on
// either side.  tests/uv_seam_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>
#include "mesh_geom.h"
#include "uv_field.h"

#define DSU_UVS_HD __host__ __device__ __forceinline__

namespace dsu_uvs {

constexpr int64_t ONE = (int64_t)1 << 20;            // a barycentric of 1 in the gather's fixed point

// The atlas of both steps.
struct Atlas {
  const float* __restrict__ uvs;
  const int32_t* __restrict__ indices;
  const int32_t* __restrict__ group;
  int64_t V, M, G;
  int32_t S;
};

// The face under texel (r, c): its corners' groups and the barycentrics of the texel's sample point
// (c, S - 1 - r) as dsu_uv_project's step 1 has them.  false: the face is not sound.
DSU_UVS_HD bool corners(const Atlas& a, int32_t m, int32_t r, int32_t c, int g[3], double b[3]) {
  if (m < 0 || m >= a.M) return false;
  int ia, ib, ic;
  if (!face_indices(a.indices, m, a.V, ia, ib, ic)) return false;
  g[0] = a.group[ia]; g[1] = a.group[ib]; g[2] = a.group[ic];
  if (g[0] < 0 || g[1] < 0 || g[2] < 0 || g[0] >= a.G || g[1] >= a.G || g[2] >= a.G) return false;
  const TriXY t = uv_tri(a.uvs, ia, ib, ic, (double)a.S);
  double w0, w1, w2;
  uv_edges(t, (double)c, (double)(a.S - 1 - r), w0, w1, w2);
  const double area = (w0 + w1) + w2;
  if (!dsu_uvf::finite(area) || !(area > 0.0)) return false;
  b[0] = w0 / area; b[1] = w1 / area; b[2] = w2 / area;
  return true;
}

// floor(b 2^20 + 0.5) clipped to [0, 2^20]; a NaN gives 0
DSU_UVS_HD int64_t fixed(double b) {
  const double v = floor(b * (double)ONE + 0.5);
  if (!(v > 0.0)) return 0;
  return v > (double)ONE ? ONE : (int64_t)v;
}

// h.  Texel `at` = r S + c: add(g, q, n) is called for every corner the texel contributes through and
// stands for den[g] += q, num[g][ch] += n[ch] — the host does just that, the kernel sums a tile's
// contributions in LDS first.
template <class Add>
DSU_UVS_HD void gather(const Atlas& a, const int32_t* __restrict__ face_id, const uint8_t* __restrict__ source,
                       const uint8_t* __restrict__ proj, const uint8_t* __restrict__ fallback, int64_t at, Add add) {
  if (source[at] == 0) return;
  const int32_t r = (int32_t)(at / a.S), c = (int32_t)(at - (int64_t)r * a.S);
  int g[3];
  double b[3];
  if (!corners(a, face_id[at], r, c, g, b)) return;
  int64_t diff[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) diff[ch] = (int64_t)((int)proj[at * 3 + ch] - (int)fallback[at * 3 + ch]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int64_t q = fixed(b[i]);
    if (q <= 0) continue;
    const int64_t n[3] = {q * diff[0], q * diff[1], q * diff[2]};
    add(g[i], q, n);
  }
}

// floor(v + 0.5) clipped to [0, 255]; the caller has ruled out a non-finite v
DSU_UVS_HD uint8_t level(double v) {
  v = floor(v + 0.5);
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (uint8_t)(int)v;
}

// i.  The three bytes of texel `at` of the composed image.
DSU_UVS_HD void apply(const Atlas& a, const int32_t* __restrict__ face_id, const uint8_t* __restrict__ source,
                      const uint8_t* __restrict__ proj, const uint8_t* __restrict__ fallback,
                      const double* __restrict__ d, int64_t at, uint8_t* __restrict__ image) {
  const int32_t m = face_id[at];
  uint8_t out[3] = {0, 0, 0};
  if (m >= 0) {
    if (source[at] != 0) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = proj[at * 3 + ch];
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = fallback[at * 3 + ch];
      const int32_t r = (int32_t)(at / a.S), c = (int32_t)(at - (int64_t)r * a.S);
      int g[3];
      double b[3];
      if (corners(a, m, r, c, g, b)) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const double e = (b[0] * d[(int64_t)g[0] * 3 + ch] + b[1] * d[(int64_t)g[1] * 3 + ch]) +
                           b[2] * d[(int64_t)g[2] * 3 + ch];
          const double v = (double)out[ch] + e;
          if (dsu_uvf::finite(v)) out[ch] = level(v);
        }
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) image[at * 3 + ch] = out[ch];
}

}  // namespace dsu_uvs
