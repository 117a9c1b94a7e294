// Classifier-free guidance around the multi-view UNet call (include/dsu_hip.h has the rule):
// the 2B-row UNet input in one pass, and guidance + DDIM step in one pass.  Both are elementwise
// over a few hundred KB, i.e. launch-bound: one grid-stride kernel each, V f16 per lane per access
// (16 bytes where the row length and the pointers allow it, else 8, else single elements), so no
// access is ever split across a row and there is no tail.  The C entries (argument checks) are in
// capi.hip.
#include "common.h"
#include <initializer_list>

namespace {

typedef _Float16 f16;

template <int V>
struct f16vec {
  typedef f16 type __attribute__((ext_vector_type(V)));
};
template <int V>
using f16v = typename f16vec<V>::type;          // V * 2 bytes, aligned to its size

inline int vec_width(int64_t row, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  if (row % 8 == 0 && bits % 16 == 0) return 8;
  if (row % 4 == 0 && bits % 8 == 0) return 4;
  return 1;
}

// out row r (2B rows of 2*row elements) = [lat[r % B] | (r < B ? 0 : img[r - B])]; `rowv`, the
// row length in vectors, and one index i per OUTPUT vector: i = (r * 2 + half) * rowv + j.
template <int V>
__global__ __launch_bounds__(256) void cfg_model_input_kernel(const f16v<V>* __restrict__ lat,
                                                              const f16v<V>* __restrict__ img,
                                                              int B, int64_t rowv,
                                                              f16v<V>* __restrict__ out) {
  const int64_t total = 4 * (int64_t)B * rowv;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t seg = i / rowv, j = i - seg * rowv;
    const int64_t r = seg >> 1;
    f16v<V> v = (f16)0.0f;
    if ((seg & 1) == 0) {
      v = lat[(r < B ? r : r - B) * rowv + j];
    } else if (r >= B) {
      v = img[(r - B) * rowv + j];
    }
    out[i] = v;
  }
}

// pred (2, nv) vectors: the unconditional half, then the conditional one.  The rule is evaluated in
// double: in f32 the two terms of `prev` (each of order 1, rounded to ~1e-7) can cancel to a value
// whose f16 spacing is 6e-8, and the result would no longer be the rounding of the rule; the
// launch is latency-bound either way.
template <int V>
__global__ __launch_bounds__(256) void ddim_cfg_step_kernel(
    const f16v<V>* __restrict__ pred, const f16v<V>* __restrict__ lat,
    const f16v<V>* __restrict__ noise, int64_t nv, double g, double sqrt_a_t, double sqrt_1m_a_t,
    double sqrt_a_prev, double dir, double std_dev, f16v<V>* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * blockDim.x) {
    const f16v<V> u = pred[i], c = pred[nv + i], x = lat[i];
    f16v<V> z = (f16)0.0f;
    if (noise) z = noise[i];
    f16v<V> o;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const double uf = (double)u[e];
      const double n = uf + g * ((double)c[e] - uf);
      const double x0 = ((double)x[e] - sqrt_1m_a_t * n) / sqrt_a_t;
      double prev = sqrt_a_prev * x0 + dir * n;
      if (noise) prev = prev + std_dev * (double)z[e];
      o[e] = (f16)prev;
    }
    out[i] = o;
  }
}

template <int V>
void launch_model_input(const void* lat, const void* img, int B, int64_t row, void* out,
                        hipStream_t s) {
  const int64_t rowv = row / V;
  cfg_model_input_kernel<V><<<dsu_capped_blocks(4 * (int64_t)B * rowv, 256), 256, 0, s>>>(
      (const f16v<V>*)lat, (const f16v<V>*)img, B, rowv, (f16v<V>*)out);
}

template <int V>
void launch_step(const void* pred, const void* lat, const void* noise, int64_t n, double g,
                 double sa, double sb, double sp, double dir, double sd, void* out, hipStream_t s) {
  ddim_cfg_step_kernel<V><<<dsu_capped_blocks(n / V, 256), 256, 0, s>>>(
      (const f16v<V>*)pred, (const f16v<V>*)lat, (const f16v<V>*)noise, n / V, g, sa, sb, sp, dir,
      sd, (f16v<V>*)out);
}

}  // namespace

int dsu_mv_cfg_model_input_launch(const void* latents, const void* image_latents, int32_t B,
                                  int64_t row_elems, void* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  // the second half of an output row starts row_elems in: part of the alignment question
  switch (vec_width(row_elems, {latents, image_latents, out})) {
    case 8: launch_model_input<8>(latents, image_latents, B, row_elems, out, s); break;
    case 4: launch_model_input<4>(latents, image_latents, B, row_elems, out, s); break;
    default: launch_model_input<1>(latents, image_latents, B, row_elems, out, s);
  }
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_mv_ddim_cfg_step_launch(const void* noise_pred, const void* latents,
                                const void* variance_noise, int64_t n, float guidance_scale,
                                float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev, double dir,
                                float std_dev, void* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  // the conditional half of noise_pred starts n elements in: n decides its alignment
  switch (vec_width(n, {noise_pred, latents, variance_noise, out})) {
    case 8:
      launch_step<8>(noise_pred, latents, variance_noise, n, guidance_scale, sqrt_a_t, sqrt_1m_a_t,
                     sqrt_a_prev, dir, std_dev, out, s);
      break;
    case 4:
      launch_step<4>(noise_pred, latents, variance_noise, n, guidance_scale, sqrt_a_t, sqrt_1m_a_t,
                     sqrt_a_prev, dir, std_dev, out, s);
      break;
    default:
      launch_step<1>(noise_pred, latents, variance_noise, n, guidance_scale, sqrt_a_t, sqrt_1m_a_t,
                     sqrt_a_prev, dir, std_dev, out, s);
  }
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}
