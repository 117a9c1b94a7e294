// dsu_uv_project_area (include/dsu_hip.h, UV export j.): the drawings read at s x s points per texel
// instead of one, nearest or bilinear.  The text of a texel is csrc/uv_project_area.h, compiled here
// for the kernel and for dsu_uv_project_area_host; tests/uv_project_area_ref.py restates it in
// float64 numpy.  dsu_uv_project (mesh_uv.hip) stays the default path and is not touched.
//
// One thread per texel, one workgroup per 16x16-texel tile, as uv_project_kernel: a wave's texels
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

__global__ __launch_bounds__(256) void uv_project_area_kernel(dsu_uvp::Args a, int32_t tiles) {
  const int tid = threadIdx.x;
  const int bin = blockIdx.x;
  const int ty = bin / tiles, tx = bin - ty * tiles;
  const int x = tx * UVP_TILE + (tid & (UVP_TILE - 1)), y = ty * UVP_TILE + tid / UVP_TILE;
  if (x >= a.S || y >= a.S) return;
  dsu_uvp::texel(a, a.S - 1 - y, x);                 // image row r samples uv * size = (c, size - 1 - r)
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
  uv_project_area_kernel<<<(unsigned)(tiles * tiles), 256, 0, st>>>(a, tiles);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
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
  for (int32_t r = 0; r < size; ++r)
    for (int32_t c = 0; c < size; ++c) dsu_uvp::texel(a, r, c);
  return DSU_OK;
}

}  // extern "C"
