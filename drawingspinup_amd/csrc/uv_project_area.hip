// dsu_uv_project and dsu_uv_project_area (include/dsu_hip.h, UV export e. and j.): the drawings
// projected into the atlas, read at one point per texel (e., the default path) or at s x s points,
// nearest or bilinear.  The text of a texel is csrc/uv_project_area.h, compiled here for the kernel
// and for dsu_uv_project_area_host; tests/uv_project_ref.py and tests/uv_project_area_ref.py restate
// the two rules in float64 numpy.  s = 1 runs the one-point instantiation (58 VGPR, 8 waves per
// SIMD), any other s the grouped one (148 VGPR, 3 waves): dsu_uvp::one_point chooses for every entry.
//
// One thread per texel, one workgroup per 16x16-texel tile as in uv_raster_kernel: a wave's texels
// are neighbours in one chart, so their points fall into the same few grid cells and the lanes read
// the same list entries through L1.  Nothing is staged in LDS (a tile's cells cannot be bounded), no
// barrier, no atomics: two runs give the same bits.
#include <cmath>
#include <cstring>
#include "common.h"
#include "mesh_geom.h"
#include "uv_project_area.h"

namespace {

constexpr int UVP_TILE = 16;

template <bool ONE>
__global__ __launch_bounds__(256) void uv_project_area_kernel(dsu_uvp::Args a, int32_t tiles) {
  const int tid = threadIdx.x;
  const int bin = blockIdx.x;
  const int ty = bin / tiles, tx = bin - ty * tiles;
  const int x = tx * UVP_TILE + (tid & (UVP_TILE - 1)), y = ty * UVP_TILE + tid / UVP_TILE;
  if (x >= a.S || y >= a.S) return;
  dsu_uvp::texel<ONE>(a, a.S - 1 - y, x);            // image row r samples uv * size = (c, size - 1 - r)
}

template <bool ONE>
void uv_project_area_texels_host(const dsu_uvp::Args& a) {
  for (int32_t r = 0; r < a.S; ++r)
    for (int32_t c = 0; c < a.S; ++c) dsu_uvp::texel<ONE>(a, r, c);
}

// EINVAL / OK-and-zero (0) / "go on" (1) for the arguments the device and the host entry share
int uv_project_area_args(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                         int64_t n_faces, int32_t size, const int32_t* face_id, const float* tris, float x0, float y0,
                         float cell, int32_t g, const int32_t* offsets, const int32_t* items,
                         const uint8_t* color_front, const uint8_t* mask_front, const uint8_t* color_back,
                         const uint8_t* mask_back, int32_t res, double z_tolerance, int32_t s, int32_t filter,
                         uint8_t* image, uint8_t* source, uint8_t* count, dsu_uvp::Args& a) {
  if (size < 1 || size > 8192 || res < 1 || res > 16384 || g < 1 || g > 4096 || !(cell > 0.0f) ||
      !std::isfinite(cell) || !std::isfinite(x0) || !std::isfinite(y0) || !(z_tolerance >= 0.0) ||
      !std::isfinite(z_tolerance) || s < 1 || s > dsu_uvp::MAX_S || filter < 0 || filter > 1)
    return DSU_EINVAL;
  if (n_verts < 0 || n_faces < 0 || n_faces > (int64_t)1 << 30 || n_verts > (int64_t)1 << 30) return DSU_EINVAL;
  if (!image || !source) return DSU_EINVAL;
  if (n_faces == 0) return 0;
  if (!uvs || !indices || !positions || n_verts == 0 || !face_id || !tris || !offsets || !items || !color_front ||
      !mask_front || !color_back || !mask_back)
    return DSU_EINVAL;
  a = dsu_uvp::Args{uvs,     indices,     positions,  n_verts,    n_faces,    size,      face_id, tris,
                    ZGrid{x0, y0, 1.0f / cell, g},    offsets,    items,      color_front, mask_front,
                    color_back, mask_back, res,       z_tolerance, s,         filter,    image,   source, count};
  return 1;
}

}  // namespace

extern "C" {

int dsu_uv_project_area(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                        int64_t n_faces, int32_t size, const int32_t* face_id, const float* tris, float x0, float y0,
                        float cell, int32_t g, const int32_t* offsets, const int32_t* items,
                        const uint8_t* color_front, const uint8_t* mask_front, const uint8_t* color_back,
                        const uint8_t* mask_back, int32_t res, double z_tolerance, int32_t s, int32_t filter,
                        uint8_t* image, uint8_t* source, uint8_t* count, void* stream) {
  dsu_uvp::Args a;
  const int rc = uv_project_area_args(uvs, indices, positions, n_verts, n_faces, size, face_id, tris, x0, y0, cell, g,
                                      offsets, items, color_front, mask_front, color_back, mask_back, res, z_tolerance,
                                      s, filter, image, source, count, a);
  if (rc < 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t texels = (size_t)size * size;
  if (rc == 0) {
    if (hipMemsetAsync(image, 0, texels * 3, st) != hipSuccess || hipMemsetAsync(source, 0, texels, st) != hipSuccess ||
        (count && hipMemsetAsync(count, 0, texels, st) != hipSuccess))
      return DSU_ELAUNCH;
    return DSU_OK;
  }
  const int32_t tiles = (size + UVP_TILE - 1) / UVP_TILE;
  const auto kernel = dsu_uvp::one_point(a) ? uv_project_area_kernel<true> : uv_project_area_kernel<false>;
  kernel<<<(unsigned)(tiles * tiles), 256, 0, st>>>(a, tiles);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

// Rule e.: the one-point instantiation at the nearest pixel, without a count.
int dsu_uv_project(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                   int64_t n_faces, int32_t size, const int32_t* face_id, const float* tris, float x0, float y0,
                   float cell, int32_t g, const int32_t* offsets, const int32_t* items, const uint8_t* color_front,
                   const uint8_t* mask_front, const uint8_t* color_back, const uint8_t* mask_back, int32_t res,
                   double z_tolerance, uint8_t* image, uint8_t* source, void* stream) {
  return dsu_uv_project_area(uvs, indices, positions, n_verts, n_faces, size, face_id, tris, x0, y0, cell, g, offsets,
                             items, color_front, mask_front, color_back, mask_back, res, z_tolerance, 1, 0, image,
                             source, nullptr, stream);
}

// HOST: the same text on host arrays, texel after texel.
int dsu_uv_project_area_host(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                             int64_t n_faces, int32_t size, const int32_t* face_id, const float* tris, float x0,
                             float y0, float cell, int32_t g, const int32_t* offsets, const int32_t* items,
                             const uint8_t* color_front, const uint8_t* mask_front, const uint8_t* color_back,
                             const uint8_t* mask_back, int32_t res, double z_tolerance, int32_t s, int32_t filter,
                             uint8_t* image, uint8_t* source, uint8_t* count) {
  dsu_uvp::Args a;
  const int rc = uv_project_area_args(uvs, indices, positions, n_verts, n_faces, size, face_id, tris, x0, y0, cell, g,
                                      offsets, items, color_front, mask_front, color_back, mask_back, res, z_tolerance,
                                      s, filter, image, source, count, a);
  if (rc < 0) return rc;
  const size_t texels = (size_t)size * size;
  if (rc == 0) {
    memset(image, 0, texels * 3);
    memset(source, 0, texels);
    if (count) memset(count, 0, texels);
    return DSU_OK;
  }
  (dsu_uvp::one_point(a) ? uv_project_area_texels_host<true> : uv_project_area_texels_host<false>)(a);
  return DSU_OK;
}

}  // extern "C"
