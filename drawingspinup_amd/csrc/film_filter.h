// The pixel filter of the frame rasteriser's resolve (include/dsu_hip.h, "Pixel filter"): one text
// for the filtered resolve of mesh_render.hip (device) and for dsu_pixel_filter_resolve_host (host),
// so the non-GPU suite pins the arithmetic the kernel runs.  Everything is float64 in the operand
// order written here; the library is compiled with -ffp-contract=off, so no products are fused on
// either side.  tests/frame_render_filter_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#define DSU_FILM_HD __host__ __device__ __forceinline__

namespace dsu_film {

constexpr int MAX_SS = 4;
constexpr int MAX_TAPS = MAX_SS + 2 * (2 * MAX_SS);   // ss + 2 halo at ss = 4, halo = 2 ss

// halo is counted in sub-samples; hp = ceil(halo / ss) is the same reach in whole pixels.
DSU_FILM_HD int halo_pixels(int halo, int ss) { return (halo + ss - 1) / ss; }

// What the entry points refuse: halo outside [0, 2 ss], a tap that is negative or not finite, central
// taps (the pixel's own ss samples) that sum to 0.  taps holds ss + 2 halo values.
inline bool taps_ok(const double* taps, int halo, int ss) {
  if (!taps || halo < 0 || halo > 2 * ss) return false;
  double centre = 0.0;
  for (int k = 0; k < ss + 2 * halo; ++k) {
    if (!(taps[k] >= 0.0) || !(taps[k] <= 1.7976931348623157e308)) return false;
    if (k >= halo && k < halo + ss) centre += taps[k];
  }
  return centre > 0.0;
}

// Pixel (i, j) of an S x S image over the N = S ss lattice: the samples at offsets qy, qx in
// [-halo, ss + halo) from the pixel's first sample, row-major; those outside the lattice do not exist.
// fetch(R, C, s) says whether sample (R, C) is covered and, if so, writes its six f32 attributes
// (colour rgb, position rgb) to s.  alpha = W_cov / W_all; v = A / W_cov, 0 where W_cov is 0.
template <class Fetch>
DSU_FILM_HD void gather(const double* taps, int halo, int ss, int N, int i, int j, Fetch fetch, double& alpha,
                        double v[6]) {
  double w_all = 0.0, w_cov = 0.0;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int qy = -halo; qy < ss + halo; ++qy) {
    const int R = i * ss + qy;
    if (R < 0 || R >= N) continue;
    const double wy = taps[qy + halo];
    for (int qx = -halo; qx < ss + halo; ++qx) {
      const int C = j * ss + qx;
      if (C < 0 || C >= N) continue;
      const double w = wy * taps[qx + halo];
      w_all += w;
      float s[6];
      if (!fetch(R, C, s)) continue;
      w_cov += w;
#pragma unroll
      for (int ch = 0; ch < 6; ++ch) acc[ch] += w * (double)s[ch];
    }
  }
  alpha = w_cov / w_all;
#pragma unroll
  for (int ch = 0; ch < 6; ++ch) v[ch] = w_cov > 0.0 ? acc[ch] / w_cov : 0.0;
}

// uint8 = floor(v 255 + 0.5), as the unfiltered resolve has it for its values in [0, 1]; a value that
// is not a number gives 0 and one outside [0, 1] the nearer end (the host entry takes any f32).
DSU_FILM_HD uint32_t quantise(double v) {
  const double q = floor(v * 255.0 + 0.5);
  if (!(q >= 0.0)) return 0u;
  return q > 255.0 ? 255u : (uint32_t)(int)q;
}

}  // namespace dsu_film
