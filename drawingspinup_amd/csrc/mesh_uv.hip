// UV export of the reconstructed mesh (the export_uv branch of save_mesh, mesh_utils.py:65-67 and
// coloring_utils.py:140-167): axis-projection charts instead of xatlas, and the reference's
// compute_interpolation_map as a rasteriser of the mesh's own triangles.  Host side:
// drawingspinup_amd/nsr/uv.py; the rules are stated in full in include/dsu_hip.h and restated in
// float64 numpy in tests/uv_ref.py.
//
//   dsu_uv_face_labels   one thread per face: normal, dominant-axis label, projected area
//   dsu_uv_components    chart id = smallest face index of the component: every face takes the
//                        minimum over its same-label neighbours and jumps twice along its own
//                        pointer (chart[chart[m]]); only thread m writes chart[m], values only fall,
//                        so in-place updates between the launches' barriers can only be ahead of a
//                        synchronous sweep and the fixed point is the same
//   dsu_uv_bake          COUNT / FILL / RASTER: faces counting-sorted onto 16x16-texel tiles
//                        (bin_sort.h), one workgroup per tile and one thread per texel,
//                        the tile's faces walked through LDS 256 at a time (15 KB: ten workgroups
//                        fit a CU's LDS, the four waves of a workgroup cover the four SIMDs).  Every
//                        thread keeps its own lowest covering face, so no atomics and no dependence
//                        on the order of the tile's list
//   dsu_uv_dilate        one gutter round per launch, integer arithmetic
//   (dsu_uv_project and dsu_uv_project_area, the drawings into the atlas: uv_project_area.hip)
//   dsu_uv_field_points  the field bake's sample points: one thread per (texel, sub-sample) of the
//                        covered texels' list, the sub-sample fastest (uv_field.h has the text)
//   dsu_uv_field_resolve the mean of a texel's evaluated samples into its three bytes: one thread
//                        per listed texel
//   dsu_uv_seam_gather   seam levelling: one thread per texel, the projected texels' colour
//                        differences into per-group 64-bit integer sums (uv_seam.h has the text)
//   dsu_uv_seam_apply    the composed image: drawing texels copied, fallback texels plus the
//                        interpolated offset; one thread per texel
// No floating-point atomics anywhere (the seam gather's are integer adds): two runs give the same bits.
#include <cmath>
#include "common.h"
#include "bin_sort.h"
#include "mesh_geom.h"
#include "uv_field.h"
#include "uv_seam.h"

namespace {

constexpr int UV_TILE = 16;
constexpr int UV_BATCH = 256;

__global__ __launch_bounds__(256) void uv_face_labels_kernel(const float* __restrict__ verts,
                                                             const int32_t* __restrict__ faces, int64_t V,
                                                             int64_t M, double* __restrict__ normal,
                                                             int32_t* __restrict__ label,
                                                             double* __restrict__ area) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= M) return;
  int ia, ib, ic;
  double n[3] = {0.0, 0.0, 0.0};
  int lab = -1;
  double ar = 0.0;
  if (face_indices(faces, m, V, ia, ib, ic)) {
    double a[3], e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = verts[(int64_t)ia * 3 + k];
      e1[k] = (double)verts[(int64_t)ib * 3 + k] - a[k];
      e2[k] = (double)verts[(int64_t)ic * 3 + k] - a[k];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double m0 = fabs(n[0]), m1 = fabs(n[1]), m2 = fabs(n[2]);
    // a non-finite normal fails every comparison below and stays degenerate
    if (m0 > 0.0 || m1 > 0.0 || m2 > 0.0) {
      if (isfinite(m0) && isfinite(m1) && isfinite(m2)) {
        int ax = 0;
        double best = m0;
        if (m1 > best) { ax = 1; best = m1; }
        if (m2 > best) { ax = 2; best = m2; }
        lab = 2 * ax + (n[ax] < 0.0 ? 1 : 0);
        ar = 0.5 * best;
      }
    }
    if (lab < 0) n[0] = n[1] = n[2] = 0.0;
  }
  normal[m * 3] = n[0];
  normal[m * 3 + 1] = n[1];
  normal[m * 3 + 2] = n[2];
  label[m] = lab;
  area[m] = ar;
}

// chart values are read while other threads lower them: every value ever stored is a face of the
// same component, so either reading is valid
__device__ __forceinline__ int32_t chart_load(const int32_t* p) {
  return __atomic_load_n(p, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(256) void uv_components_round_kernel(const int32_t* __restrict__ adj,
                                                                  const int32_t* __restrict__ label, int64_t M,
                                                                  int32_t* chart, int32_t* flag) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int32_t lab = label[m];
  if (lab < 0) return;
  const int32_t old = chart_load(chart + m);
  int32_t c = old;
  if (c < 0 || c > m) return;                        // not the caller's initial state: leave it
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int32_t nb = adj[m * 3 + e];
    if (nb < 0 || nb >= M || label[nb] != lab) continue;
    const int32_t v = chart_load(chart + nb);
    if (v >= 0 && v < c) c = v;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int32_t v = chart_load(chart + c);
    if (v >= 0 && v < c) c = v;
  }
  if (c < old) {
    __atomic_store_n(chart + m, c, __ATOMIC_RELAXED);
    *flag = 1;
  }
}

// Texel range [x0, x1] x [y0, y1] (uv-texel coordinates, y up) of the samples the face can cover:
// floor / ceil of its bounds, clipped to the atlas.  false: non-finite, or outside.
__device__ __forceinline__ bool uv_range(const TriXY& t, int S, int& x0, int& x1, int& y0, int& y1) {
  if (!finite_xy(t)) return false;
  const double xmin = fmin(fmin(t.ax, t.bx), t.cx), xmax = fmax(fmax(t.ax, t.bx), t.cx);
  const double ymin = fmin(fmin(t.ay, t.by), t.cy), ymax = fmax(fmax(t.ay, t.by), t.cy);
  const double lim = (double)S + 4.0;
  x0 = (int)floor(fmin(fmax(xmin, -4.0), lim));
  x1 = (int)ceil(fmin(fmax(xmax, -4.0), lim));
  y0 = (int)floor(fmin(fmax(ymin, -4.0), lim));
  y1 = (int)ceil(fmin(fmax(ymax, -4.0), lim));
  if (x1 < 0 || y1 < 0 || x0 > S - 1 || y0 > S - 1) return false;
  x0 = max(x0, 0); y0 = max(y0, 0); x1 = min(x1, S - 1); y1 = min(y1, S - 1);
  return true;
}

// bin_sort.h source: face m goes to every tile its texel range touches.  tile = ty G + tx.
struct FaceTexelTiles {
  const float* __restrict__ uvs;
  const int32_t* __restrict__ faces;
  int64_t V;
  int32_t S, G;
  __device__ __forceinline__ int32_t id(int64_t m) const { return (int32_t)m; }
  template <class Emit>
  __device__ __forceinline__ void bins(int64_t m, Emit emit) const {
    int ia, ib, ic;
    if (!face_indices(faces, m, V, ia, ib, ic)) return;
    const TriXY t = uv_tri(uvs, ia, ib, ic, (double)S);
    int x0, x1, y0, y1;
    if (!uv_range(t, S, x0, x1, y0, y1)) return;
    for (int ty = y0 / UV_TILE; ty <= y1 / UV_TILE; ++ty)
      for (int tx = x0 / UV_TILE; tx <= x1 / UV_TILE; ++tx) emit(ty * G + tx);
  }
};

__global__ __launch_bounds__(256) void uv_raster_kernel(
    const float* __restrict__ uvs, const int32_t* __restrict__ faces, const float* __restrict__ colours,
    const double* __restrict__ depth, int64_t V, int64_t M, int32_t S, int32_t G,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ items, int64_t n_items,
    uint8_t* __restrict__ image, int32_t* __restrict__ face_id, uint8_t* __restrict__ demote) {
  __shared__ TriXY tri[UV_BATCH];
  __shared__ double dep[UV_BATCH];
  __shared__ int32_t idx[UV_BATCH];
  const int tid = threadIdx.x;
  const int bin = blockIdx.x;
  const int ty = bin / G, tx = bin - ty * G;
  const int x = tx * UV_TILE + (tid & (UV_TILE - 1)), y = ty * UV_TILE + tid / UV_TILE;
  const bool live = x < S && y < S;
  const double px = (double)x, py = (double)y;
  int32_t lowest = -1;                               // lowest face covering the sample (edges inclusive)
  int32_t front = -1;                                // front-most face strictly containing the sample
  double front_depth = 0.0;
  const int64_t beg = max((int64_t)offsets[bin], (int64_t)0), end = min((int64_t)offsets[bin + 1], n_items);
  for (int64_t base = beg; base < end; base += UV_BATCH) {
    const int n = (int)min((int64_t)UV_BATCH, end - base);
    __syncthreads();
    if (tid < n) {
      const int32_t m = items[base + tid];
      int ia, ib, ic;
      int32_t keep = -1;
      if (m >= 0 && m < M && face_indices(faces, m, V, ia, ib, ic)) {
        tri[tid] = uv_tri(uvs, ia, ib, ic, (double)S);
        dep[tid] = depth ? depth[m] : 0.0;
        keep = m;
      }
      idx[tid] = keep;
    }
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < n; ++k) {
      const int32_t m = idx[k];
      if (m < 0) continue;
      double w0, w1, w2;
      uv_edges(tri[k], px, py, w0, w1, w2);
      if (!(w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0)) continue;
      if (!((w0 + w1) + w2 > 0.0)) continue;
      if (lowest < 0 || m < lowest) lowest = m;
      if (demote && w0 > 0.0 && w1 > 0.0 && w2 > 0.0) {
        const double d = dep[k];
        if (front < 0) {
          front = m; front_depth = d;
        } else if (d > front_depth || (d == front_depth && m < front)) {
          demote[front] = 1;
          front = m; front_depth = d;
        } else {
          demote[m] = 1;
        }
      }
    }
  }
  if (!live) return;
  const int64_t at = (int64_t)(S - 1 - y) * S + x;   // image row r samples uv * size = (c, size - 1 - r)
  uint8_t q[3] = {0, 0, 0};
  if (lowest >= 0) {
    int ia, ib, ic;
    face_indices(faces, lowest, V, ia, ib, ic);           // validated when it was staged
    const TriXY t = uv_tri(uvs, ia, ib, ic, (double)S);
    double w0, w1, w2;
    uv_edges(t, px, py, w0, w1, w2);
    const double area = (w0 + w1) + w2;
    const double b0 = w0 / area, b1 = w1 / area, b2 = w2 / area;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      q[ch] = dsu_uvf::quantise((b0 * (double)colours[(int64_t)ia * 3 + ch] + b1 * (double)colours[(int64_t)ib * 3 + ch]) +
                          b2 * (double)colours[(int64_t)ic * 3 + ch]);
  }
  if (image) {
    image[at * 3] = q[0];
    image[at * 3 + 1] = q[1];
    image[at * 3 + 2] = q[2];
  }
  if (face_id) face_id[at] = lowest;
}

__global__ __launch_bounds__(256) void uv_dilate_kernel(const uint8_t* __restrict__ img_in,
                                                        const uint8_t* __restrict__ cov_in, int32_t S,
                                                        uint8_t* __restrict__ img_out,
                                                        uint8_t* __restrict__ cov_out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)S * S) return;
  const int r = (int)(i / S), c = (int)(i - (int64_t)r * S);
  uint32_t out[3] = {0, 0, 0};
  uint8_t cov = cov_in[i] ? 1 : 0;
  if (cov) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = img_in[i * 3 + ch];
  } else {
    uint32_t sum[3] = {0, 0, 0}, n = 0;
    for (int dr = -1; dr <= 1; ++dr)
      for (int dc = -1; dc <= 1; ++dc) {
        const int rr = r + dr, cc = c + dc;
        if ((dr == 0 && dc == 0) || rr < 0 || cc < 0 || rr >= S || cc >= S) continue;
        const int64_t j = (int64_t)rr * S + cc;
        if (!cov_in[j]) continue;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) sum[ch] += img_in[j * 3 + ch];
        ++n;
      }
    if (n) {
      cov = 1;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = (2u * sum[ch] + n) / (2u * n);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) img_out[i * 3 + ch] = (uint8_t)out[ch];
  cov_out[i] = cov;
}

// dsu_uv_field_points.  Neighbouring threads are the sub-samples of one texel, then the next listed
// texel (ascending, so mostly the next column of one chart): a wave reads a handful of faces and
// writes 64 consecutive points.  Nothing is shared, so no LDS and no barrier.
__global__ __launch_bounds__(256) void uv_field_points_kernel(
    const float* __restrict__ uvs, const int32_t* __restrict__ indices, const float* __restrict__ positions,
    int64_t V, int64_t M, int32_t S, const int32_t* __restrict__ face_id, const int32_t* __restrict__ texels,
    int64_t n_texels, int32_t s, float* __restrict__ points, uint8_t* __restrict__ valid) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int32_t ss = s * s;
  if (i >= n_texels * ss) return;
  const int64_t t = i / ss;
  float p[3];
  const bool ok = dsu_uvf::point(uvs, indices, positions, V, M, S, face_id, texels[t], s, (int32_t)(i - t * ss), p);
  points[i * 3] = p[0];
  points[i * 3 + 1] = p[1];
  points[i * 3 + 2] = p[2];
  valid[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void uv_field_resolve_kernel(const float* __restrict__ colours,
                                                               const uint8_t* __restrict__ valid,
                                                               const int32_t* __restrict__ texels, int64_t n_texels,
                                                               int32_t ss, int32_t S, uint8_t* __restrict__ image) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n_texels) return;
  dsu_uvf::resolve(colours, valid, t, ss, S, texels[t], image);
}

// dsu_uv_seam_gather.  Tiles as in uv_raster_kernel: a tile's texels are neighbours in one chart,
// so its up to 768 contributions go to the few groups of a handful of faces.  They are summed in LDS
// first, in an open-addressing table keyed by group (SEAM_SLOTS >= 3 x 256 keys, so linear probing
// always ends at the key or at a free slot; 36 KB, four workgroups per CU), and every used slot then
// adds its four sums to global memory once.  All sums are 64-bit integers and the adds relaxed
// atomics whose result nobody reads: the totals do not depend on any order.  A tile without a
// projected texel (two thirds of a 1024^2 atlas) leaves before touching the table.
constexpr int SEAM_BITS = 10;
constexpr int SEAM_SLOTS = 1 << SEAM_BITS;
static_assert(SEAM_SLOTS >= 3 * UV_TILE * UV_TILE, "the table must hold a key per corner of the tile's texels");

struct SeamTableAdd {
  int32_t* key;                    // SEAM_SLOTS, -1 = free
  unsigned long long* sum;         // SEAM_SLOTS x 4: den, num[0..2]
  __device__ __forceinline__ void operator()(int g, int64_t q, const int64_t n[3]) const {
    unsigned h = ((unsigned)g * 2654435761u) >> (32 - SEAM_BITS);
    for (int probe = 0; probe < SEAM_SLOTS; ++probe) {
      const int32_t k = atomicCAS(&key[h], -1, g);
      if (k == -1 || k == g) break;
      h = (h + 1) & (SEAM_SLOTS - 1);
    }
    atomicAdd(&sum[h * 4], (unsigned long long)q);                         // two's complement throughout
    atomicAdd(&sum[h * 4 + 1], (unsigned long long)n[0]);
    atomicAdd(&sum[h * 4 + 2], (unsigned long long)n[1]);
    atomicAdd(&sum[h * 4 + 3], (unsigned long long)n[2]);
  }
};

// the texel (linear index r S + c) of this thread in tile blockIdx.x of `tiles` per axis; -1 beyond the image
__device__ __forceinline__ int64_t uv_tile_texel(int32_t S, int32_t tiles) {
  const int tid = threadIdx.x;
  const int bin = blockIdx.x;
  const int ty = bin / tiles, tx = bin - ty * tiles;
  const int x = tx * UV_TILE + (tid & (UV_TILE - 1)), y = ty * UV_TILE + tid / UV_TILE;
  if (x >= S || y >= S) return -1;
  return (int64_t)(S - 1 - y) * S + x;
}

__global__ __launch_bounds__(256) void uv_seam_gather_kernel(dsu_uvs::Atlas a, int32_t tiles,
                                                             const int32_t* __restrict__ face_id,
                                                             const uint8_t* __restrict__ source,
                                                             const uint8_t* __restrict__ proj,
                                                             const uint8_t* __restrict__ fallback,
                                                             int64_t* __restrict__ num, int64_t* __restrict__ den) {
  __shared__ int32_t key[SEAM_SLOTS];
  __shared__ unsigned long long sum[SEAM_SLOTS * 4];
  const int tid = threadIdx.x;
  const int64_t at = uv_tile_texel(a.S, tiles);                    // -1 beyond the image: still at every barrier
  if (!__syncthreads_or(at >= 0 && source[at] != 0)) return;   // the whole workgroup leaves, or none of it
  for (int i = tid; i < SEAM_SLOTS; i += 256) {
    key[i] = -1;
    sum[i * 4] = sum[i * 4 + 1] = sum[i * 4 + 2] = sum[i * 4 + 3] = 0;
  }
  __syncthreads();
  if (at >= 0) dsu_uvs::gather(a, face_id, source, proj, fallback, at, SeamTableAdd{key, sum});
  __syncthreads();
  for (int i = tid; i < SEAM_SLOTS; i += 256) {
    const int32_t g = key[i];
    if (g < 0) continue;
    atomicAdd(reinterpret_cast<unsigned long long*>(den + g), sum[i * 4]);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      if (sum[i * 4 + 1 + ch])
        atomicAdd(reinterpret_cast<unsigned long long*>(num + (int64_t)g * 3 + ch), sum[i * 4 + 1 + ch]);
  }
}

// dsu_uv_seam_apply.  Every texel writes its own three bytes; nothing is shared.
__global__ __launch_bounds__(256) void uv_seam_apply_kernel(dsu_uvs::Atlas a, int32_t tiles,
                                                            const int32_t* __restrict__ face_id,
                                                            const uint8_t* __restrict__ source,
                                                            const uint8_t* __restrict__ proj,
                                                            const uint8_t* __restrict__ fallback,
                                                            const double* __restrict__ d, uint8_t* __restrict__ image) {
  const int64_t at = uv_tile_texel(a.S, tiles);
  if (at < 0) return;
  dsu_uvs::apply(a, face_id, source, proj, fallback, d, at, image);
}

bool uv_size_ok(int32_t size) { return size >= 1 && size <= 8192; }

int64_t uv_tiles(int32_t size) {
  const int64_t G = (size + UV_TILE - 1) / UV_TILE;
  return G * G;
}

// EINVAL / OK / "go on" (1) for the arguments the device and the host entries of the field bake share
int uv_field_points_args(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                         int64_t n_faces, int32_t size, const int32_t* face_id, const int32_t* texels,
                         int64_t n_texels, int32_t s, const float* points, const uint8_t* valid) {
  if (!uv_size_ok(size) || s < 1 || s > dsu_uvf::MAX_S) return DSU_EINVAL;
  if (n_verts < 0 || n_faces < 0 || n_texels < 0 || n_verts > (int64_t)1 << 30 || n_faces > (int64_t)1 << 30 ||
      n_texels > (int64_t)1 << 30)
    return DSU_EINVAL;
  if (!points || !valid) return DSU_EINVAL;
  if (n_texels == 0) return DSU_OK;
  if (!face_id || !texels) return DSU_EINVAL;
  if (n_faces && (!uvs || !indices || !positions || n_verts == 0)) return DSU_EINVAL;
  return 1;
}

int uv_field_resolve_args(const float* colours, const uint8_t* valid, const int32_t* texels, int64_t n_texels,
                          int32_t s, int32_t size, const uint8_t* image) {
  if (!uv_size_ok(size) || s < 1 || s > dsu_uvf::MAX_S || n_texels < 0 || n_texels > (int64_t)1 << 30)
    return DSU_EINVAL;
  if (!image) return DSU_EINVAL;
  if (n_texels == 0) return DSU_OK;
  if (!colours || !valid || !texels) return DSU_EINVAL;
  return 1;
}

// EINVAL / OK / "go on" (1) for the arguments the device and the host entries of the seam steps share
bool uv_seam_counts_ok(int64_t n_verts, int64_t n_faces, int64_t n_groups, int32_t size) {
  const int64_t cap = (int64_t)1 << 30;
  return uv_size_ok(size) && n_verts >= 0 && n_faces >= 0 && n_groups >= 0 && n_verts <= cap && n_faces <= cap &&
         n_groups <= cap;
}

int uv_seam_gather_args(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                        int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                        const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, const int64_t* num,
                        const int64_t* den) {
  if (!uv_seam_counts_ok(n_verts, n_faces, n_groups, size)) return DSU_EINVAL;
  if (!num || !den) return DSU_EINVAL;
  if (n_groups == 0 || n_faces == 0) return DSU_OK;
  if (!uvs || !indices || !group || n_verts == 0 || !face_id || !source || !proj || !fallback) return DSU_EINVAL;
  return 1;
}

// the atlas of apply: without faces or groups no face is sound and its arrays are not read
int uv_seam_apply_args(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                       int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                       const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, const double* d,
                       const uint8_t* image, dsu_uvs::Atlas& a) {
  if (!uv_seam_counts_ok(n_verts, n_faces, n_groups, size)) return DSU_EINVAL;
  if (!image) return DSU_EINVAL;
  if (!face_id || !source || !proj || !fallback) return DSU_EINVAL;
  const bool atlas = n_faces > 0 && n_groups > 0;
  if (atlas && (!uvs || !indices || !group || !d || n_verts == 0)) return DSU_EINVAL;
  a = dsu_uvs::Atlas{uvs, indices, group, n_verts, atlas ? n_faces : 0, atlas ? n_groups : 0, size};
  return 1;
}

}  // namespace

extern "C" {

int dsu_uv_face_labels(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces,
                       double* normal, int32_t* label, double* area, void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_verts > (int64_t)1 << 30 || n_faces > (int64_t)1 << 30) return DSU_EINVAL;
  if (n_faces == 0) return DSU_OK;
  if (!verts || !faces || !normal || !label || !area || n_verts == 0) return DSU_EINVAL;
  uv_face_labels_kernel<<<dsu_blocks_for(n_faces, 256), 256, 0, (hipStream_t)stream>>>(
      verts, faces, n_verts, n_faces, normal, label, area);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_uv_components(const int32_t* adjacency, const int32_t* label, int64_t n_faces, int32_t* chart,
                      int32_t* flag, int32_t check_every, int32_t max_rounds, int32_t* out_rounds,
                      void* stream) {
  if (n_faces < 0 || n_faces > (int64_t)1 << 30 || check_every < 1 || max_rounds < 1) return DSU_EINVAL;
  if (out_rounds) *out_rounds = 0;
  if (n_faces == 0) return DSU_OK;
  if (!adjacency || !label || !chart || !flag) return DSU_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int32_t rounds = 0, host_flag = 1;
  while (host_flag && rounds < max_rounds) {
    if (hipMemsetAsync(flag, 0, sizeof(int32_t), st) != hipSuccess) return DSU_ELAUNCH;
    for (int k = 0; k < check_every && rounds < max_rounds; ++k, ++rounds)
      uv_components_round_kernel<<<dsu_blocks_for(n_faces, 256), 256, 0, st>>>(adjacency, label, n_faces,
                                                                              chart, flag);
    DSU_CHECK_LAUNCH();
    if (hipMemcpyAsync(&host_flag, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return DSU_ELAUNCH;
  }
  if (out_rounds) *out_rounds = rounds;
  return host_flag ? DSU_EUNSUP : DSU_OK;
}

int64_t dsu_uv_bake_workspace_bytes(int32_t size) {
  if (!uv_size_ok(size)) return DSU_EINVAL;
  return dsu_bin::bytes(uv_tiles(size));
}

int dsu_uv_bake(int32_t stage, const float* uvs, const int32_t* indices, const float* colours,
                const double* depth, int64_t n_verts, int64_t n_faces, int32_t size, void* workspace,
                int64_t workspace_bytes, int32_t* items, int64_t n_items, uint8_t* image, int32_t* face_id,
                uint8_t* demote, void* stream) {
  if (stage < DSU_UV_COUNT || stage > DSU_UV_RASTER || !uv_size_ok(size)) return DSU_EINVAL;
  if (n_verts < 0 || n_faces < 0 || n_items < 0 || n_faces > (int64_t)1 << 30 || n_verts > (int64_t)1 << 30)
    return DSU_EINVAL;
  const int64_t nb = uv_tiles(size);
  if (!workspace || workspace_bytes < dsu_bin::bytes(nb)) return DSU_EINVAL;
  if (n_faces && (!uvs || !indices || n_verts == 0)) return DSU_EINVAL;
  if (stage != DSU_UV_COUNT && n_items && !items) return DSU_EINVAL;
  if (stage == DSU_UV_RASTER && ((n_faces && !colours) || (demote && !depth))) return DSU_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int32_t G = (size + UV_TILE - 1) / UV_TILE;
  if (stage != DSU_UV_RASTER)
    return dsu_bin::run_stage(stage, FaceTexelTiles{uvs, indices, n_verts, size, G}, n_faces, workspace, nb,
                              items, n_items, st);
  const int32_t* offsets = dsu_bin::split(workspace, nb).offsets;
  if (demote && n_faces && hipMemsetAsync(demote, 0, n_faces, st) != hipSuccess) return DSU_ELAUNCH;
  uv_raster_kernel<<<(unsigned)nb, 256, 0, st>>>(uvs, indices, colours, depth, n_verts, n_faces, size, G,
                                                 offsets, items, n_faces ? n_items : 0, image, face_id,
                                                 demote);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_uv_dilate(const uint8_t* image_in, const uint8_t* covered_in, int32_t size, uint8_t* image_out,
                  uint8_t* covered_out, void* stream) {
  if (!uv_size_ok(size) || !image_in || !covered_in || !image_out || !covered_out || image_in == image_out ||
      covered_in == covered_out)
    return DSU_EINVAL;
  uv_dilate_kernel<<<dsu_blocks_for((int64_t)size * size, 256), 256, 0, (hipStream_t)stream>>>(
      image_in, covered_in, size, image_out, covered_out);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_uv_field_points(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                        int64_t n_faces, int32_t size, const int32_t* face_id, const int32_t* texels,
                        int64_t n_texels, int32_t s, float* points, uint8_t* valid, void* stream) {
  const int rc = uv_field_points_args(uvs, indices, positions, n_verts, n_faces, size, face_id, texels, n_texels, s,
                                      points, valid);
  if (rc != 1) return rc;
  uv_field_points_kernel<<<dsu_blocks_for(n_texels * s * s, 256), 256, 0, (hipStream_t)stream>>>(
      uvs, indices, positions, n_verts, n_faces, size, face_id, texels, n_texels, s, points, valid);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_uv_field_resolve(const float* colours, const uint8_t* valid, const int32_t* texels, int64_t n_texels,
                         int32_t s, int32_t size, uint8_t* image, void* stream) {
  const int rc = uv_field_resolve_args(colours, valid, texels, n_texels, s, size, image);
  if (rc != 1) return rc;
  uv_field_resolve_kernel<<<dsu_blocks_for(n_texels, 256), 256, 0, (hipStream_t)stream>>>(
      colours, valid, texels, n_texels, s * s, size, image);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

// HOST: the same two texts (uv_field.h) on host arrays.
int dsu_uv_field_points_host(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                             int64_t n_faces, int32_t size, const int32_t* face_id, const int32_t* texels,
                             int64_t n_texels, int32_t s, float* points, uint8_t* valid) {
  const int rc = uv_field_points_args(uvs, indices, positions, n_verts, n_faces, size, face_id, texels, n_texels, s,
                                      points, valid);
  if (rc != 1) return rc;
  const int32_t ss = s * s;
  for (int64_t i = 0; i < n_texels * ss; ++i) {
    const int64_t t = i / ss;
    valid[i] = dsu_uvf::point(uvs, indices, positions, n_verts, n_faces, size, face_id, texels[t], s,
                              (int32_t)(i - t * ss), points + i * 3)
                   ? 1
                   : 0;
  }
  return DSU_OK;
}

int dsu_uv_field_resolve_host(const float* colours, const uint8_t* valid, const int32_t* texels, int64_t n_texels,
                              int32_t s, int32_t size, uint8_t* image) {
  const int rc = uv_field_resolve_args(colours, valid, texels, n_texels, s, size, image);
  if (rc != 1) return rc;
  for (int64_t t = 0; t < n_texels; ++t) dsu_uvf::resolve(colours, valid, t, s * s, size, texels[t], image);
  return DSU_OK;
}

int dsu_uv_seam_gather(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                       int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                       const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, int64_t* num,
                       int64_t* den, void* stream) {
  const int rc = uv_seam_gather_args(uvs, indices, group, n_verts, n_faces, n_groups, size, face_id, source, proj,
                                     fallback, num, den);
  if (rc != 1) return rc;
  const int32_t G = (size + UV_TILE - 1) / UV_TILE;
  uv_seam_gather_kernel<<<(unsigned)uv_tiles(size), 256, 0, (hipStream_t)stream>>>(
      dsu_uvs::Atlas{uvs, indices, group, n_verts, n_faces, n_groups, size}, G, face_id, source, proj, fallback, num,
      den);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_uv_seam_apply(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                      int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                      const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, const double* d,
                      uint8_t* image, void* stream) {
  dsu_uvs::Atlas a;
  const int rc = uv_seam_apply_args(uvs, indices, group, n_verts, n_faces, n_groups, size, face_id, source, proj,
                                    fallback, d, image, a);
  if (rc != 1) return rc;
  const int32_t G = (size + UV_TILE - 1) / UV_TILE;
  uv_seam_apply_kernel<<<(unsigned)uv_tiles(size), 256, 0, (hipStream_t)stream>>>(a, G, face_id, source, proj,
                                                                                 fallback, d, image);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

// HOST: the same two texts (uv_seam.h) on host arrays, texel after texel and a plain +=.
int dsu_uv_seam_gather_host(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                            int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                            const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, int64_t* num,
                            int64_t* den) {
  const int rc = uv_seam_gather_args(uvs, indices, group, n_verts, n_faces, n_groups, size, face_id, source, proj,
                                     fallback, num, den);
  if (rc != 1) return rc;
  const dsu_uvs::Atlas a{uvs, indices, group, n_verts, n_faces, n_groups, size};
  for (int64_t at = 0; at < (int64_t)size * size; ++at)
    dsu_uvs::gather(a, face_id, source, proj, fallback, at, [=](int g, int64_t q, const int64_t n[3]) {
      den[g] += q;
      for (int ch = 0; ch < 3; ++ch) num[(int64_t)g * 3 + ch] += n[ch];
    });
  return DSU_OK;
}

int dsu_uv_seam_apply_host(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                           int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                           const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, const double* d,
                           uint8_t* image) {
  dsu_uvs::Atlas a;
  const int rc = uv_seam_apply_args(uvs, indices, group, n_verts, n_faces, n_groups, size, face_id, source, proj,
                                    fallback, d, image, a);
  if (rc != 1) return rc;
  for (int64_t at = 0; at < (int64_t)size * size; ++at) dsu_uvs::apply(a, face_id, source, proj, fallback, d, at, image);
  return DSU_OK;
}

}  // extern "C"
