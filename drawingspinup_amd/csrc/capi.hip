// Error strings / ABI version of libdsu_hip.so.
#include "common.h"
#include <math.h>

// mv_guidance.hip: the launches behind dsu_cfg_model_input / dsu_ddim_cfg_step (arguments checked here)
int dsu_mv_cfg_model_input_launch(const void* latents, const void* image_latents, int32_t B,
                                  int64_t row_elems, void* out, void* stream);
int dsu_mv_ddim_cfg_step_launch(const void* noise_pred, const void* latents,
                                const void* variance_noise, int64_t n, float guidance_scale,
                                float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev, double dir,
                                float std_dev, void* out, void* stream);

extern "C" {

const char* dsu_strerror(int code) {
  switch (code) {
    case DSU_OK: return "ok";
    case DSU_EINVAL: return "invalid argument";
    case DSU_ELAUNCH: return "HIP launch/runtime error";
    case DSU_EUNSUP: return "configuration not supported by the gfx950 kernels";
    default: return "unknown dsu error";
  }
}

int dsu_abi_version(void) { return DSU_ABI_VERSION; }

int32_t dsu_onewave_grid_cap_value = 0;     // CUs; 0 = the resident count (geometry backward 512, texture backward 256 workgroups)
int32_t dsu_scatter_grid_cap_value = 0;     // 0 = the resident count (three 256-thread workgroups per CU: 768)
int dsu_set_scatter_grid_cap(int32_t workgroups) {
  if (workgroups < 0 || workgroups > 4096) return DSU_EINVAL;
  dsu_scatter_grid_cap_value = workgroups;
  return DSU_OK;
}
int32_t dsu_nsr_side_priority_value = 1;   // 1 high, 2 normal, 0 low (nsr_driver.hip)
int dsu_set_nsr_side_stream_priority(int32_t level) {
  if (level < 0 || level > 2) return DSU_EINVAL;
  dsu_nsr_side_priority_value = level;
  return DSU_OK;
}
int32_t dsu_nsr_side_pool_value = 0;   // 1: side streams handed from one step driver to the next (nsr_driver.hip)
int dsu_set_nsr_side_stream_pooling(int32_t on) {
  if (on < 0 || on > 1) return DSU_EINVAL;
  dsu_nsr_side_pool_value = on;
  return DSU_OK;
}
int dsu_set_onewave_grid_cap(int32_t cus) {
  if (cus < 0 || cus > 256) return DSU_EINVAL;
  dsu_onewave_grid_cap_value = cus;
  return DSU_OK;
}

int dsu_cfg_model_input(const void* latents, const void* image_latents, int32_t B,
                        int64_t row_elems, void* out, void* stream) {
  if (!latents || !image_latents || !out || B < 0 || row_elems < 0) return DSU_EINVAL;
  if (out == latents || out == image_latents) return DSU_EINVAL;
  if (B == 0 || row_elems == 0) return DSU_OK;
  if (row_elems > INT64_MAX / 4 / B) return DSU_EINVAL;
  return dsu_mv_cfg_model_input_launch(latents, image_latents, B, row_elems, out, stream);
}

int dsu_ddim_cfg_step(const void* noise_pred, const void* latents, const void* variance_noise,
                      int64_t n, float guidance_scale, float sqrt_a_t, float sqrt_1m_a_t,
                      float sqrt_a_prev, float std_dev, void* out, void* stream) {
  if (!noise_pred || !latents || !out || n < 0 || n > INT64_MAX / 2) return DSU_EINVAL;
  if (out == noise_pred || out == latents || out == variance_noise) return DSU_EINVAL;
  if (!(sqrt_a_t > 0.0f) || !(std_dev >= 0.0f) || !isfinite(guidance_scale) ||
      !isfinite(sqrt_1m_a_t) || !isfinite(sqrt_a_prev))
    return DSU_EINVAL;
  // the radicand of the "direction pointing to x_t" term, from the f32 scalars in double; eta = 1
  // at the last step leaves ~4e-4 of it, a rounding of the inputs must not make that a NaN
  const double rad = 1.0 - (double)sqrt_a_prev * sqrt_a_prev - (double)std_dev * std_dev;
  if (!(rad >= -1e-6)) return DSU_EINVAL;
  if (n == 0) return DSU_OK;
  return dsu_mv_ddim_cfg_step_launch(noise_pred, latents, variance_noise, n, guidance_scale,
                                     sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev,
                                     sqrt(rad > 0.0 ? rad : 0.0), std_dev, out, stream);
}

}  // extern "C"
