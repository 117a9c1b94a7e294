// Frame rendering between reconstruction and stylisation (3_style_translator/run_render.py +
// blender_animation.py): the reference hands the exported OBJ to Blender, which for the rig-free
// actions (rest_pose, rest_rotate) is an orthographic rasteriser of a vertex-coloured mesh, run
// once with the colours and once with the normalised positions; run_render.py:31-57 (pos2edge)
// then derives the edge map from the position pass.  Here: F frames of one mesh and both attribute
// sets in one call, on the device (gfx950).
//
// The rule (include/dsu_hip.h states it in full; tests/frame_render_ref.py restates it in float64):
//   * fine lattice N = S * ss; sample (R, C) at x = cx + ((C + 0.5) / N - 0.5) * span,
//     y = cy - ((R + 0.5) / N - 0.5) * span (float64, this order);
//   * coverage by the three edge functions of mesh_geom.h (float64 from the f32 vertices, both
//     orientations, edges inclusive), area = w0 + w1 + w2 at the sample, area == 0 skipped;
//   * z = (w0 za + w1 zb + w2 zc) / area rounded to f32: largest z wins, equal z -> lowest face;
//   * per pixel: alpha = covered / ss^2, attribute = mean over the covered samples.
//
// Shape of the work: (frame, triangle) pairs are binned onto 16x16-pixel tiles (the counting sort
// of bin_sort.h); one workgroup per (frame, tile)
// keeps the tile's (16 ss)^2 sub-samples in LDS as one 64-bit key each — depth as an ordered
// integer in the high word, the complemented face index in the low word — and walks the tile's
// list with LDS atomicMax, so the winner does not depend on the order of the list.  The same
// workgroup then resolves: no global atomics on the frame, no visibility buffer in HBM.
// LDS: 32 KB of keys + 1 KB of lattice coordinates at ss = 4.
//
// Textured frames (`tex` with filter NEAREST or BILINEAR): the same visibility, and in the resolve the three
// colour channels of a sample come from the UV atlas — the face's uvs interpolated with the sample's
// edge functions, then a nearest or bilinear read of the RGBA8 texture under the bake's convention
// (image row r, column c holds uv T = (c, T - 1 - r)).  The texels are read through L2: neighbouring
// samples share them.  The position pass is untouched.
//
// Mip-mapped frames (`tex` with filter TRILINEAR): the atlas is the pyramid of mesh_mip.hip and a sample
// blends the bilinear reads of two neighbouring levels (mip_sample.h).  The view is orthographic and
// uv is affine on a face, so the level is constant per (frame, face): it is computed where the
// face's attributes are loaded.  The two levels of a face lie near each other in the buffer.
//
// Anisotropic frames (`tex` with filter ANISOTROPIC): the same pyramid, read N times per sample along the
// major axis of the face's footprint, at the level of the footprint divided by N (mip_sample.h).  Axis,
// length, N and level are per (frame, face) like the trilinear level; the probes of a sample are a loop
// in the resolve, 4 or 8 texel loads each, on texels that neighbouring samples' probes share.
//
// Pixel filter (dsu_mesh_render_ortho_filtered): a pixel gathers the samples of its own square and of
// `halo` sub-samples around it, weighted by a separable table the caller hands in (film_filter.h
// holds the accumulation, for the kernel and for dsu_pixel_filter_resolve_host).  The workgroup's key
// tile grows by hp = ceil(halo / ss) pixels on every side, (frame, triangle) pairs are binned onto
// the grown tiles, and a sample's attributes are recomputed by every pixel that reaches it: staging
// six f32 per sample of the grown tile would not fit beside the keys.  The kernels of the unfiltered
// entry point are not touched by any of this.
#include "common.h"
#include "bin_sort.h"
#include "film_filter.h"
#include "mesh_geom.h"
#include "mip_sample.h"

namespace {

constexpr int RT_TILE = 16;   // output pixels per tile side

struct RenderView {
  double cx, cy, span;
  int32_t S, ss, N, G;        // output side, sub-samples per pixel side, N = S ss, tiles per side
};

__device__ __forceinline__ double lattice_x(const RenderView& v, int C) {
  return v.cx + (((double)C + 0.5) / (double)v.N - 0.5) * v.span;
}
__device__ __forceinline__ double lattice_y(const RenderView& v, int R) {
  return v.cy - (((double)R + 0.5) / (double)v.N - 0.5) * v.span;
}

// Samples whose centre can lie inside the triangle's xy bounding box: floor / ceil of the bounds'
// lattice coordinates, which already leaves up to one sample of margin on each side (the float64
// rounding of the lattice formula is many orders below one sample).
// false: non-finite vertex, or entirely outside the frame.  The range is clipped to the frame.
__device__ __forceinline__ bool sample_range(const RenderView& v, const TriXY& t, int& c0, int& c1,
                                             int& r0, int& r1) {
  if (!finite_xy(t)) return false;
  const double xmin = fmin(fmin(t.ax, t.bx), t.cx), xmax = fmax(fmax(t.ax, t.bx), t.cx);
  const double ymin = fmin(fmin(t.ay, t.by), t.cy), ymax = fmax(fmax(t.ay, t.by), t.cy);
  const double n = (double)v.N, lim = n + 4.0;
  const double tc0 = ((xmin - v.cx) / v.span + 0.5) * n - 0.5, tc1 = ((xmax - v.cx) / v.span + 0.5) * n - 0.5;
  const double tr0 = (0.5 - (ymax - v.cy) / v.span) * n - 0.5, tr1 = (0.5 - (ymin - v.cy) / v.span) * n - 0.5;
  c0 = (int)floor(fmin(fmax(tc0, -4.0), lim));
  c1 = (int)ceil(fmin(fmax(tc1, -4.0), lim));
  r0 = (int)floor(fmin(fmax(tr0, -4.0), lim));
  r1 = (int)ceil(fmin(fmax(tr1, -4.0), lim));
  if (c1 < 0 || r1 < 0 || c0 > v.N - 1 || r0 > v.N - 1) return false;
  c0 = max(c0, 0); r0 = max(r0, 0); c1 = min(c1, v.N - 1); r1 = min(r1, v.N - 1);
  return true;
}

__device__ __forceinline__ TriXY load_xy(const float* __restrict__ sv, int ia, int ib, int ic) {
  TriXY t;
  t.ax = sv[(int64_t)ia * 3]; t.ay = sv[(int64_t)ia * 3 + 1];
  t.bx = sv[(int64_t)ib * 3]; t.by = sv[(int64_t)ib * 3 + 1];
  t.cx = sv[(int64_t)ic * 3]; t.cy = sv[(int64_t)ic * 3 + 1];
  return t;
}

// bin_sort.h source: pair i = frame M + triangle goes to every tile the triangle may touch in that
// frame, stored as the triangle.  bin = (frame G + tile_row) G + tile_col.
struct FrameTriangleTiles {
  const float* __restrict__ screen;
  const int32_t* __restrict__ faces;
  int64_t V, M;
  RenderView view;
  __device__ __forceinline__ int32_t id(int64_t i) const { return (int32_t)(i - (int64_t)(int)(i / M) * M); }
  template <class Emit>
  __device__ __forceinline__ void bins(int64_t i, Emit emit) const {
    const int f = (int)(i / M);
    const int64_t m = i - (int64_t)f * M;
    int ia, ib, ic;
    if (!face_indices(faces, m, V, ia, ib, ic)) return;
    const TriXY t = load_xy(screen + (int64_t)f * V * 3, ia, ib, ic);
    int c0, c1, r0, r1;
    if (!sample_range(view, t, c0, c1, r0, r1)) return;
    const int T = RT_TILE * view.ss;
    for (int ty = r0 / T; ty <= r1 / T; ++ty)
      for (int tx = c0 / T; tx <= c1 / T; ++tx) emit((f * view.G + ty) * view.G + tx);
  }
};

// The same pairs for the filtered resolve: every tile whose rectangle, grown by `grow` samples on each
// side (hp pixels) and clipped to the frame, the triangle's sample range touches.
struct FrameTriangleGrownTiles {
  FrameTriangleTiles base;
  int32_t grow;
  __device__ __forceinline__ int32_t id(int64_t i) const { return base.id(i); }
  template <class Emit>
  __device__ __forceinline__ void bins(int64_t i, Emit emit) const {
    const RenderView& view = base.view;
    const int f = (int)(i / base.M);
    const int64_t m = i - (int64_t)f * base.M;
    int ia, ib, ic;
    if (!face_indices(base.faces, m, base.V, ia, ib, ic)) return;
    const TriXY t = load_xy(base.screen + (int64_t)f * base.V * 3, ia, ib, ic);
    int c0, c1, r0, r1;
    if (!sample_range(view, t, c0, c1, r0, r1)) return;
    const int T = RT_TILE * view.ss;
    const int ty0 = max(r0 - grow, 0) / T, ty1 = min((r1 + grow) / T, view.G - 1);
    const int tx0 = max(c0 - grow, 0) / T, tx1 = min((c1 + grow) / T, view.G - 1);
    for (int ty = ty0; ty <= ty1; ++ty)
      for (int tx = tx0; tx <= tx1; ++tx) emit((f * view.G + ty) * view.G + tx);
  }
};

// float -> unsigned with the same order (all finite values and infinities; never 0)
__device__ __forceinline__ uint32_t ordered_bits(float z) {
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__device__ __forceinline__ uint32_t quantise(double v) { return (uint32_t)(int)floor(v * 255.0 + 0.5); }

struct RenderOut {
  uint8_t* color_u8;    // (F,S,S,4)
  uint8_t* pos_u8;      // (F,S,S,4)
  int32_t* face_id;     // (F,N,N)
  float* depth;         // (F,N,N)
  float* frames;        // (F,6,S,S)
  float* pixels;        // (F,S,S,8)
};

// The atlas of the textured resolve: uv (V,2) f32, texels (T,T) RGBA8 as one 32-bit word each.
struct RenderTexture {
  const float* __restrict__ uv;
  const uint32_t* __restrict__ texels;
  int32_t T;
  int32_t max_aniso;          // TEX_ANISO: the cap on the probes of a sample
};

constexpr int TEX_NONE = -1, TEX_NEAREST = DSU_TEX_NEAREST, TEX_BILINEAR = DSU_TEX_BILINEAR,
              TEX_TRILINEAR = DSU_TEX_TRILINEAR, TEX_ANISO = DSU_TEX_ANISOTROPIC;

__device__ __forceinline__ float texel_channel(uint32_t p, int ch) { return (float)((p >> (8 * ch)) & 255u); }

// Colour of one sample from the atlas (include/dsu_hip.h, the textured rule): tx, ty = uv T.
template <int TEX>
__device__ __forceinline__ void sample_atlas(const RenderTexture& tex, double tx, double ty, float rgb[3]) {
  const double top = (double)(tex.T - 1);
  if (!isfinite(tx)) tx = 0.0;
  if (!isfinite(ty)) ty = 0.0;
  if constexpr (TEX == TEX_NEAREST) {
    const int c = (int)fmin(fmax(floor(tx + 0.5), 0.0), top);
    const int r = (int)fmin(fmax(top - floor(ty + 0.5), 0.0), top);
    const uint32_t p = tex.texels[(int64_t)r * tex.T + c];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = texel_channel(p, ch) / 255.0f;
  } else {
    const double x = fmin(fmax(tx, 0.0), top), y = fmin(fmax(top - ty, 0.0), top);
    const int c0 = (int)floor(x), r0 = (int)floor(y);
    const int c1 = min(c0 + 1, tex.T - 1), r1 = min(r0 + 1, tex.T - 1);
    const double fx = x - (double)c0, fy = y - (double)r0;
    const uint32_t p00 = tex.texels[(int64_t)r0 * tex.T + c0], p01 = tex.texels[(int64_t)r0 * tex.T + c1];
    const uint32_t p10 = tex.texels[(int64_t)r1 * tex.T + c0], p11 = tex.texels[(int64_t)r1 * tex.T + c1];
    const double k00 = (1.0 - fx) * (1.0 - fy), k01 = fx * (1.0 - fy), k10 = (1.0 - fx) * fy, k11 = fx * fy;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      rgb[ch] = (float)((k00 * (double)texel_channel(p00, ch) + k01 * (double)texel_channel(p01, ch) +
                         k10 * (double)texel_channel(p10, ch) + k11 * (double)texel_channel(p11, ch)) / 255.0);
  }
}

// One workgroup of four waves per (frame, tile).  TEX: where the colour channels of a sample come
// from — TEX_NONE the vertex colours, TEX_NEAREST / TEX_BILINEAR the atlas, TEX_TRILINEAR / TEX_ANISO its
// pyramid (tex.texels is then the pyramid buffer, tex.T the side of level 0).
template <int SS, int TEX>
__device__ __forceinline__ void raster_resolve_tile(
    unsigned long long* keys, double* xs, double* ys,
    const float* __restrict__ screen, const int32_t* __restrict__ faces,
    const float* __restrict__ colour, const float* __restrict__ pos, int64_t V, int64_t M,
    const RenderView& view, const int32_t* __restrict__ offsets, const int32_t* __restrict__ items,
    int64_t n_items, const RenderTexture& tex, const RenderOut& out) {
  constexpr int T = RT_TILE * SS;
  constexpr int CH0 = TEX == TEX_NONE ? 0 : 3;   // first interpolated channel
  const int tid = threadIdx.x;
  const int bin = blockIdx.x;
  const int f = bin / (view.G * view.G);
  const int ty = (bin - f * view.G * view.G) / view.G, tx = bin - (f * view.G + ty) * view.G;
  const int R0 = ty * T, C0 = tx * T;
  const float* __restrict__ sv = screen + (int64_t)f * V * 3;
  for (int s = tid; s < T * T; s += 256) keys[s] = 0ull;
  if (tid < T) xs[tid] = lattice_x(view, C0 + tid);
  else if (tid < 2 * T) ys[tid - T] = lattice_y(view, R0 + tid - T);
  __syncthreads();

  // ---- visibility: one triangle per wave, its lanes stride over the triangle's samples in the tile
  const int wave = tid >> 6, lane = tid & 63;
  const int64_t beg = offsets[bin], end = min((int64_t)offsets[bin + 1], n_items);
  for (int64_t k = max(beg, (int64_t)0) + wave; k < end; k += 4) {
    const int m = items[k];
    if (m < 0 || m >= M) continue;
    int ia, ib, ic;
    if (!face_indices(faces, m, V, ia, ib, ic)) continue;
    const TriXY t = load_xy(sv, ia, ib, ic);
    int c0, c1, r0, r1;
    if (!sample_range(view, t, c0, c1, r0, r1)) continue;
    c0 = max(c0, C0); r0 = max(r0, R0); c1 = min(c1, C0 + T - 1); r1 = min(r1, R0 + T - 1);
    if (c1 < c0 || r1 < r0) continue;
    const double za = sv[(int64_t)ia * 3 + 2], zb = sv[(int64_t)ib * 3 + 2], zc = sv[(int64_t)ic * 3 + 2];
    const int w = c1 - c0 + 1, n = w * (r1 - r0 + 1);
    const uint32_t low = ~(uint32_t)m;
    for (int i = lane; i < n; i += 64) {
      const int rr = i / w;
      const int lr = r0 - R0 + rr, lc = c0 - C0 + (i - rr * w);
      double w0, w1, w2;
      edge_functions(t, xs[lc], ys[lr], w0, w1, w2);
      const double area = w0 + w1 + w2;
      if (area == 0.0 || !covers(w0, w1, w2)) continue;
      float z = (float)((w0 * za + w1 * zb + w2 * zc) / area);
      if (!(z == z)) continue;
      if (z == 0.0f) z = 0.0f;                       // -0 and +0 are the same depth
      atomicMax(&keys[lr * T + lc], ((unsigned long long)ordered_bits(z) << 32) | low);
    }
  }
  __syncthreads();

  // ---- per-sample outputs
  if (out.face_id || out.depth) {
    for (int s = tid; s < T * T; s += 256) {
      const int lr = s / T, lc = s - lr * T;
      const int R = R0 + lr, C = C0 + lc;
      if (R >= view.N || C >= view.N) continue;
      const unsigned long long key = keys[s];
      const int64_t at = ((int64_t)f * view.N + R) * view.N + C;
      if (out.face_id) out.face_id[at] = key ? (int32_t)~(uint32_t)key : -1;
      if (out.depth) out.depth[at] = key ? ordered_float((uint32_t)(key >> 32)) : 0.0f;
    }
  }

  // ---- resolve: one pixel per thread, its samples in row-major order
  const int py = tid / RT_TILE, px = tid - py * RT_TILE;
  const int Y = ty * RT_TILE + py, X = tx * RT_TILE + px;
  if (Y >= view.S || X >= view.S) return;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int covered = 0;
  uint32_t last = 0xffffffffu;
  TriXY t = {};
  float a0[6], a1[6], a2[6];
#pragma unroll
  for (int ch = 0; ch < 6; ++ch) a0[ch] = a1[ch] = a2[ch] = 0.0f;
  float ua = 0.0f, va = 0.0f, ub = 0.0f, vb = 0.0f, uc = 0.0f, vc = 0.0f;
  int lod_k = 0, lod_at = 0;                        // TEX_TRILINEAR: the face's level, its texel offset
  double lod_t = 0.0;                               // and the weight of level lod_k + 1
  dsu_mip::AnisoFace an;                            // TEX_ANISO: the face's axis, probes and level
  for (int sy = 0; sy < SS; ++sy)
    for (int sx = 0; sx < SS; ++sx) {
      const int lr = py * SS + sy, lc = px * SS + sx;
      const unsigned long long key = keys[lr * T + lc];
      if (!key) continue;
      const uint32_t m = ~(uint32_t)key;
      if (m != last) {
        int ia, ib, ic;
        face_indices(faces, m, V, ia, ib, ic);      // validated when the key was written
        t = load_xy(sv, ia, ib, ic);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          if constexpr (TEX == TEX_NONE) {
            a0[ch] = clamp01(colour[(int64_t)ia * 3 + ch]);
            a1[ch] = clamp01(colour[(int64_t)ib * 3 + ch]);
            a2[ch] = clamp01(colour[(int64_t)ic * 3 + ch]);
          }
          a0[3 + ch] = clamp01(pos[(int64_t)ia * 3 + ch]);
          a1[3 + ch] = clamp01(pos[(int64_t)ib * 3 + ch]);
          a2[3 + ch] = clamp01(pos[(int64_t)ic * 3 + ch]);
        }
        if constexpr (TEX != TEX_NONE) {
          ua = tex.uv[(int64_t)ia * 2]; va = tex.uv[(int64_t)ia * 2 + 1];
          ub = tex.uv[(int64_t)ib * 2]; vb = tex.uv[(int64_t)ib * 2 + 1];
          uc = tex.uv[(int64_t)ic * 2]; vc = tex.uv[(int64_t)ic * 2 + 1];
        }
        if constexpr (TEX == TEX_TRILINEAR) {
          const double rho = dsu_mip::footprint(t.ax, t.ay, t.bx, t.by, t.cx, t.cy, ua, va, ub, vb, uc, vc,
                                                tex.T, view.span / (double)view.N);
          dsu_mip::lod(rho, dsu_mip::levels(tex.T), lod_k, lod_t);
          lod_at = (int)dsu_mip::level_offset(tex.T, lod_k);
        }
        if constexpr (TEX == TEX_ANISO) {
          an = dsu_mip::footprint_aniso(t.ax, t.ay, t.bx, t.by, t.cx, t.cy, ua, va, ub, vb, uc, vc, tex.T,
                                        view.span / (double)view.N, tex.max_aniso, dsu_mip::levels(tex.T));
          lod_at = (int)dsu_mip::level_offset(tex.T, an.k);
        }
        last = m;
      }
      double w0, w1, w2;
      edge_functions(t, xs[lc], ys[lr], w0, w1, w2);
      const double area = w0 + w1 + w2;
      if constexpr (TEX != TEX_NONE) {
        const double u = (w0 * (double)ua + w1 * (double)ub + w2 * (double)uc) / area;
        const double v = (w0 * (double)va + w1 * (double)vb + w2 * (double)vc) / area;
        float rgb[3];
        if constexpr (TEX == TEX_TRILINEAR)
          dsu_mip::sample(tex.texels, tex.T, u * (double)tex.T, v * (double)tex.T, lod_k, lod_t, lod_at, rgb);
        else if constexpr (TEX == TEX_ANISO)
          dsu_mip::sample_aniso(tex.texels, tex.T, u * (double)tex.T, v * (double)tex.T, an.s1, an.N, an.ax, an.ay,
                                an.k, an.t, lod_at, rgb);
        else
          sample_atlas<TEX>(tex, u * (double)tex.T, v * (double)tex.T, rgb);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] += (double)rgb[ch];
      }
#pragma unroll
      for (int ch = CH0; ch < 6; ++ch)
        acc[ch] += (double)(float)((w0 * (double)a0[ch] + w1 * (double)a1[ch] + w2 * (double)a2[ch]) / area);
      ++covered;
    }
  double v[6];
#pragma unroll
  for (int ch = 0; ch < 6; ++ch) v[ch] = covered ? acc[ch] / (double)covered : 0.0;
  const double alpha = (double)covered / (double)(SS * SS);
  const uint32_t a8 = quantise(alpha);
  uint32_t q[6];
#pragma unroll
  for (int ch = 0; ch < 6; ++ch) q[ch] = quantise(v[ch]);
  const int64_t pix = ((int64_t)f * view.S + Y) * view.S + X;
  if (out.color_u8)
    reinterpret_cast<uint32_t*>(out.color_u8)[pix] = q[0] | (q[1] << 8) | (q[2] << 16) | (a8 << 24);
  if (out.pos_u8)
    reinterpret_cast<uint32_t*>(out.pos_u8)[pix] = q[3] | (q[4] << 8) | (q[5] << 16) | (a8 << 24);
  if (out.pixels) {
    float4* p = reinterpret_cast<float4*>(out.pixels) + pix * 2;
    p[0] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)alpha);
    p[1] = make_float4((float)v[3], (float)v[4], (float)v[5], (float)alpha);
  }
  if (out.frames) {
    // DatasetFullImages (entry/data.py): ToTensor = u8 / 255 in f32, Normalize(0.5, 0.5) on the
    // colour and position channels, the mask as it is — from the uint8 values, like a PNG read back
    const int64_t plane = (int64_t)view.S * view.S;
    float* fr = out.frames + (int64_t)f * 6 * plane + (int64_t)Y * view.S + X;
    fr[0] = ((float)q[0] / 255.0f - 0.5f) / 0.5f;
    fr[plane] = ((float)q[1] / 255.0f - 0.5f) / 0.5f;
    fr[2 * plane] = ((float)q[2] / 255.0f - 0.5f) / 0.5f;
    fr[3 * plane] = (float)a8 / 255.0f;
    fr[4 * plane] = ((float)q[3] / 255.0f - 0.5f) / 0.5f;
    fr[5 * plane] = ((float)q[4] / 255.0f - 0.5f) / 0.5f;
  }
}

template <int SS>
__global__ __launch_bounds__(256) void mesh_raster_resolve_kernel(
    const float* __restrict__ screen, const int32_t* __restrict__ faces,
    const float* __restrict__ colour, const float* __restrict__ pos, int64_t V, int64_t M,
    RenderView view, const int32_t* __restrict__ offsets, const int32_t* __restrict__ items,
    int64_t n_items, RenderOut out) {
  constexpr int T = RT_TILE * SS;
  __shared__ unsigned long long keys[T * T];
  __shared__ double xs[T], ys[T];
  raster_resolve_tile<SS, TEX_NONE>(keys, xs, ys, screen, faces, colour, pos, V, M, view, offsets, items,
                                    n_items, RenderTexture{nullptr, nullptr, 0, 0}, out);
}

template <int SS, int FILTER>
__global__ __launch_bounds__(256) void mesh_raster_resolve_textured_kernel(
    const float* __restrict__ screen, const int32_t* __restrict__ faces, const float* __restrict__ pos,
    int64_t V, int64_t M, RenderView view, const int32_t* __restrict__ offsets,
    const int32_t* __restrict__ items, int64_t n_items, RenderTexture tex, RenderOut out) {
  constexpr int T = RT_TILE * SS;
  __shared__ unsigned long long keys[T * T];
  __shared__ double xs[T], ys[T];
  raster_resolve_tile<SS, FILTER>(keys, xs, ys, screen, faces, nullptr, pos, V, M, view, offsets, items,
                                  n_items, tex, out);
}

// ---- the filtered resolve (include/dsu_hip.h, "Pixel filter")
// The visibility loop, the face's attributes and the pixel's stores are written out again below, not
// shared with raster_resolve_tile: with them factored into common functions the compiler unrolls and
// schedules the twelve unfiltered kernels differently (up to four times the instructions at ss 4), and
// those are to stay the code they were.
struct FilmTaps {
  double t[dsu_film::MAX_TAPS];   // ss + 2 halo of them
  int32_t halo;
};

// The winning face of a sample and what the resolve reads of it: loaded when the face changes.
template <int TEX>
struct FaceAttributes {
  uint32_t face = 0xffffffffu;
  TriXY t = {};
  float a0[6], a1[6], a2[6];
  float ua = 0.0f, va = 0.0f, ub = 0.0f, vb = 0.0f, uc = 0.0f, vc = 0.0f;
  int lod_k = 0, lod_at = 0;
  double lod_t = 0.0;
  dsu_mip::AnisoFace an;

  __device__ __forceinline__ void load(uint32_t m, const float* __restrict__ sv, const int32_t* __restrict__ faces,
                                       const float* __restrict__ colour, const float* __restrict__ pos, int64_t V,
                                       const RenderView& view, const RenderTexture& tex) {
    int ia, ib, ic;
    face_indices(faces, m, V, ia, ib, ic);          // validated when the key was written
    t = load_xy(sv, ia, ib, ic);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if constexpr (TEX == TEX_NONE) {
        a0[ch] = clamp01(colour[(int64_t)ia * 3 + ch]);
        a1[ch] = clamp01(colour[(int64_t)ib * 3 + ch]);
        a2[ch] = clamp01(colour[(int64_t)ic * 3 + ch]);
      }
      a0[3 + ch] = clamp01(pos[(int64_t)ia * 3 + ch]);
      a1[3 + ch] = clamp01(pos[(int64_t)ib * 3 + ch]);
      a2[3 + ch] = clamp01(pos[(int64_t)ic * 3 + ch]);
    }
    if constexpr (TEX != TEX_NONE) {
      ua = tex.uv[(int64_t)ia * 2]; va = tex.uv[(int64_t)ia * 2 + 1];
      ub = tex.uv[(int64_t)ib * 2]; vb = tex.uv[(int64_t)ib * 2 + 1];
      uc = tex.uv[(int64_t)ic * 2]; vc = tex.uv[(int64_t)ic * 2 + 1];
    }
    if constexpr (TEX == TEX_TRILINEAR) {
      const double rho = dsu_mip::footprint(t.ax, t.ay, t.bx, t.by, t.cx, t.cy, ua, va, ub, vb, uc, vc, tex.T,
                                            view.span / (double)view.N);
      dsu_mip::lod(rho, dsu_mip::levels(tex.T), lod_k, lod_t);
      lod_at = (int)dsu_mip::level_offset(tex.T, lod_k);
    }
    if constexpr (TEX == TEX_ANISO) {
      an = dsu_mip::footprint_aniso(t.ax, t.ay, t.bx, t.by, t.cx, t.cy, ua, va, ub, vb, uc, vc, tex.T,
                                    view.span / (double)view.N, tex.max_aniso, dsu_mip::levels(tex.T));
      lod_at = (int)dsu_mip::level_offset(tex.T, an.k);
    }
    face = m;
  }

  // the six f32 attributes of the sample at (x, y): the unfiltered resolve's per-sample values
  __device__ __forceinline__ void at(double x, double y, const RenderTexture& tex, float s[6]) const {
    constexpr int CH0 = TEX == TEX_NONE ? 0 : 3;
    double w0, w1, w2;
    edge_functions(t, x, y, w0, w1, w2);
    const double area = w0 + w1 + w2;
    if constexpr (TEX != TEX_NONE) {
      const double u = (w0 * (double)ua + w1 * (double)ub + w2 * (double)uc) / area;
      const double v = (w0 * (double)va + w1 * (double)vb + w2 * (double)vc) / area;
      if constexpr (TEX == TEX_TRILINEAR)
        dsu_mip::sample(tex.texels, tex.T, u * (double)tex.T, v * (double)tex.T, lod_k, lod_t, lod_at, s);
      else if constexpr (TEX == TEX_ANISO)
        dsu_mip::sample_aniso(tex.texels, tex.T, u * (double)tex.T, v * (double)tex.T, an.s1, an.N, an.ax, an.ay,
                              an.k, an.t, lod_at, s);
      else
        sample_atlas<TEX>(tex, u * (double)tex.T, v * (double)tex.T, s);
    }
#pragma unroll
    for (int ch = CH0; ch < 6; ++ch)
      s[ch] = (float)((w0 * (double)a0[ch] + w1 * (double)a1[ch] + w2 * (double)a2[ch]) / area);
  }
};

// One workgroup of four waves per (frame, tile), as above, over the tile grown by hp pixels per side.
// Dynamic LDS: keys (TG^2) | xs (TG) | ys (TG) | taps (MAX_TAPS), TG = (16 + 2 hp) SS.
template <int SS, int TEX>
__global__ __launch_bounds__(256) void mesh_raster_resolve_filtered_kernel(
    const float* __restrict__ screen, const int32_t* __restrict__ faces, const float* __restrict__ colour,
    const float* __restrict__ pos, int64_t V, int64_t M, RenderView view, const int32_t* __restrict__ offsets,
    const int32_t* __restrict__ items, int64_t n_items, RenderTexture tex, FilmTaps film, RenderOut out) {
  extern __shared__ unsigned long long film_lds[];
  constexpr int T = RT_TILE * SS;
  const int halo = film.halo;
  const int grow = dsu_film::halo_pixels(halo, SS) * SS;
  const int TG = T + 2 * grow;
  unsigned long long* keys = film_lds;
  double* xs = reinterpret_cast<double*>(film_lds + TG * TG);
  double* ys = xs + TG;
  double* taps = ys + TG;
  const int tid = threadIdx.x;
  const int bin = blockIdx.x;
  const int f = bin / (view.G * view.G);
  const int ty = (bin - f * view.G * view.G) / view.G, tx = bin - (f * view.G + ty) * view.G;
  const int R0 = ty * T - grow, C0 = tx * T - grow;   // first sample of the grown tile; may lie outside the frame
  const float* __restrict__ sv = screen + (int64_t)f * V * 3;
  for (int s = tid; s < TG * TG; s += 256) keys[s] = 0ull;
  if (tid < TG) xs[tid] = lattice_x(view, C0 + tid);
  else if (tid < 2 * TG) ys[tid - TG] = lattice_y(view, R0 + tid - TG);
  if (tid == 255) {
#pragma unroll
    for (int k = 0; k < dsu_film::MAX_TAPS; ++k) taps[k] = film.t[k];
  }
  __syncthreads();

  // ---- visibility over the grown tile (sample_range has clipped the triangle to the frame)
  const int wave = tid >> 6, lane = tid & 63;
  const int64_t beg = offsets[bin], end = min((int64_t)offsets[bin + 1], n_items);
  for (int64_t k = max(beg, (int64_t)0) + wave; k < end; k += 4) {
    const int m = items[k];
    if (m < 0 || m >= M) continue;
    int ia, ib, ic;
    if (!face_indices(faces, m, V, ia, ib, ic)) continue;
    const TriXY t = load_xy(sv, ia, ib, ic);
    int c0, c1, r0, r1;
    if (!sample_range(view, t, c0, c1, r0, r1)) continue;
    c0 = max(c0, C0); r0 = max(r0, R0); c1 = min(c1, C0 + TG - 1); r1 = min(r1, R0 + TG - 1);
    if (c1 < c0 || r1 < r0) continue;
    const double za = sv[(int64_t)ia * 3 + 2], zb = sv[(int64_t)ib * 3 + 2], zc = sv[(int64_t)ic * 3 + 2];
    const int w = c1 - c0 + 1, n = w * (r1 - r0 + 1);
    const uint32_t low = ~(uint32_t)m;
    for (int i = lane; i < n; i += 64) {
      const int rr = i / w;
      const int lr = r0 - R0 + rr, lc = c0 - C0 + (i - rr * w);
      double w0, w1, w2;
      edge_functions(t, xs[lc], ys[lr], w0, w1, w2);
      const double area = w0 + w1 + w2;
      if (area == 0.0 || !covers(w0, w1, w2)) continue;
      float z = (float)((w0 * za + w1 * zb + w2 * zc) / area);
      if (!(z == z)) continue;
      if (z == 0.0f) z = 0.0f;                       // -0 and +0 are the same depth
      atomicMax(&keys[lr * TG + lc], ((unsigned long long)ordered_bits(z) << 32) | low);
    }
  }
  __syncthreads();

  // ---- per-sample outputs: the tile's own samples, not the margin (its owners write those)
  if (out.face_id || out.depth) {
    for (int s = tid; s < T * T; s += 256) {
      const int lr = s / T, lc = s - lr * T;
      const int R = ty * T + lr, C = tx * T + lc;
      if (R >= view.N || C >= view.N) continue;
      const unsigned long long key = keys[(lr + grow) * TG + lc + grow];
      const int64_t at = ((int64_t)f * view.N + R) * view.N + C;
      if (out.face_id) out.face_id[at] = key ? (int32_t)~(uint32_t)key : -1;
      if (out.depth) out.depth[at] = key ? ordered_float((uint32_t)(key >> 32)) : 0.0f;
    }
  }

  // ---- resolve: one pixel per thread gathers its footprint (film_filter.h)
  const int py = tid / RT_TILE, px = tid - py * RT_TILE;
  const int Y = ty * RT_TILE + py, X = tx * RT_TILE + px;
  if (Y >= view.S || X >= view.S) return;
  FaceAttributes<TEX> face;
  double alpha, v[6];
  dsu_film::gather(taps, halo, SS, view.N, Y, X, [&](int R, int C, float s[6]) {
    const int lr = R - R0, lc = C - C0;
    const unsigned long long key = keys[lr * TG + lc];
    if (!key) return false;
    const uint32_t m = ~(uint32_t)key;
    if (m != face.face) face.load(m, sv, faces, colour, pos, V, view, tex);
    face.at(xs[lc], ys[lr], tex, s);
    return true;
  }, alpha, v);
  const uint32_t a8 = dsu_film::quantise(alpha);
  uint32_t q[6];
#pragma unroll
  for (int ch = 0; ch < 6; ++ch) q[ch] = dsu_film::quantise(v[ch]);
  const int64_t pix = ((int64_t)f * view.S + Y) * view.S + X;
  if (out.color_u8)
    reinterpret_cast<uint32_t*>(out.color_u8)[pix] = q[0] | (q[1] << 8) | (q[2] << 16) | (a8 << 24);
  if (out.pos_u8)
    reinterpret_cast<uint32_t*>(out.pos_u8)[pix] = q[3] | (q[4] << 8) | (q[5] << 16) | (a8 << 24);
  if (out.pixels) {
    float4* p = reinterpret_cast<float4*>(out.pixels) + pix * 2;
    p[0] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)alpha);
    p[1] = make_float4((float)v[3], (float)v[4], (float)v[5], (float)alpha);
  }
  if (out.frames) {                                  // the DatasetFullImages tensor, as in the unfiltered resolve
    const int64_t plane = (int64_t)view.S * view.S;
    float* fr = out.frames + (int64_t)f * 6 * plane + (int64_t)Y * view.S + X;
    fr[0] = ((float)q[0] / 255.0f - 0.5f) / 0.5f;
    fr[plane] = ((float)q[1] / 255.0f - 0.5f) / 0.5f;
    fr[2 * plane] = ((float)q[2] / 255.0f - 0.5f) / 0.5f;
    fr[3 * plane] = (float)a8 / 255.0f;
    fr[4 * plane] = ((float)q[3] / 255.0f - 0.5f) / 0.5f;
    fr[5 * plane] = ((float)q[4] / 255.0f - 0.5f) / 0.5f;
  }
}

// pos2edge (run_render.py:31-57) + the inversion of :120 on the RGBA8 position image: channels
// u8 -> f32 / 255, every channel 2 where alpha8 < 255 (alpha < 1), 3x3 Sobel per channel in
// float64 (cv2.Sobel(..., CV_64F, ksize=3), default border BORDER_REFLECT_101), magnitude, maximum
// over the three colour channels, > 0.3 = edge; stored 255 - edge (255 = no edge).
__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(256) void pos_edge_kernel(const uint8_t* __restrict__ pos_rgba, int32_t H,
                                                       int32_t W, uint8_t* __restrict__ edge) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
  if (x >= W) return;
  const uint32_t* __restrict__ img = reinterpret_cast<const uint32_t*>(pos_rgba) + (int64_t)f * H * W;
  uint32_t px[3][3];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
      px[dy][dx] = img[(int64_t)reflect101(y + dy - 1, H) * W + reflect101(x + dx - 1, W)];
  double best = 0.0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double p[3][3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const uint32_t w = px[dy][dx];
        p[dy][dx] = (w >> 24) < 255u ? 2.0 : (double)((float)((w >> (8 * ch)) & 255u) / 255.0f);
      }
    const double gx = (p[0][2] - p[0][0]) + 2.0 * (p[1][2] - p[1][0]) + (p[2][2] - p[2][0]);
    const double gy = (p[2][0] - p[0][0]) + 2.0 * (p[2][1] - p[0][1]) + (p[2][2] - p[0][2]);
    best = fmax(best, sqrt(gx * gx + gy * gy));
  }
  edge[((int64_t)f * H + y) * W + x] = best > 0.3 ? 0 : 255;
}

bool view_ok(int32_t F, int32_t S, int32_t ss, double span) {
  return F >= 1 && F <= 4096 && S >= 4 && S <= 2048 && S % 4 == 0 && (ss == 1 || ss == 2 || ss == 4) &&
         span > 0.0 && span == span && span < 1e30;
}

int64_t bins_of(int32_t F, int32_t S) {
  const int64_t G = (S + RT_TILE - 1) / RT_TILE;
  return (int64_t)F * G * G;
}

bool texture_ok(const dsu_render_texture& t) {
  return t.uv && t.texels && (uintptr_t)t.texels % 4 == 0 &&   // a texel is one 32-bit load
         t.tex_size >= 1 && t.tex_size <= dsu_mip::MAX_T && t.filter >= TEX_NEAREST && t.filter <= TEX_ANISO &&
         (t.filter != TEX_ANISO || (t.max_aniso >= 1 && t.max_aniso <= dsu_mip::MAX_ANISO));   // read with ANISO only
}

// The arguments of the RASTER launch, and the kernel of a (SS, colour source) pair.
struct RasterCall {
  unsigned bins;
  hipStream_t st;
  const float* screen;
  const int32_t* faces;
  const float* colour;
  const float* pos;
  int64_t V, M;
  RenderView view;
  const int32_t* offsets;
  const int32_t* items;
  int64_t n_items;
  RenderTexture tex;
  RenderOut out;

  template <int SS, int TEX>
  void go() const {
    if constexpr (TEX == TEX_NONE)
      mesh_raster_resolve_kernel<SS><<<bins, 256, 0, st>>>(screen, faces, colour, pos, V, M, view, offsets,
                                                           items, n_items, out);
    else
      mesh_raster_resolve_textured_kernel<SS, TEX><<<bins, 256, 0, st>>>(screen, faces, pos, V, M, view, offsets,
                                                                         items, n_items, tex, out);
  }
  template <int TEX>
  void launch(int ss) const {
    if (ss == 1) go<1, TEX>();
    else if (ss == 2) go<2, TEX>();
    else go<4, TEX>();
  }

  // the filtered resolve of the same pair; at most 52 640 B of dynamic LDS (ss 4, halo 8)
  template <int SS, int TEX>
  void go_filtered(const FilmTaps& film) const {
    const int TG = (RT_TILE + 2 * dsu_film::halo_pixels(film.halo, SS)) * SS;
    const size_t lds = sizeof(double) * ((size_t)TG * TG + 2 * TG + dsu_film::MAX_TAPS);
    mesh_raster_resolve_filtered_kernel<SS, TEX><<<bins, 256, lds, st>>>(screen, faces, colour, pos, V, M, view,
                                                                         offsets, items, n_items, tex, film, out);
  }
  template <int TEX>
  void launch_filtered(int ss, const FilmTaps& film) const {
    if (ss == 1) go_filtered<1, TEX>(film);
    else if (ss == 2) go_filtered<2, TEX>(film);
    else go_filtered<4, TEX>(film);
  }
};

// Both entry points.  filtered == false is dsu_mesh_render_ortho: taps and halo are not looked at.
int render_ortho(bool filtered, int32_t stage, const float* screen, const int32_t* faces, const float* colour,
                 const float* pos, const dsu_render_texture* tex, int32_t n_frames, int64_t n_verts,
                 int64_t n_faces, double cx, double cy, double span, int32_t size, int32_t ss, const double* taps,
                 int32_t halo, void* workspace, int64_t workspace_bytes, int32_t* items, int64_t n_items,
                 const RenderOut& out, void* stream) {
  if (stage < DSU_RENDER_COUNT || stage > DSU_RENDER_RASTER) return DSU_EINVAL;
  if (!view_ok(n_frames, size, ss, span) || !(cx == cx) || !(cy == cy)) return DSU_EINVAL;
  if (n_verts < 0 || n_faces < 0 || n_items < 0 || (int64_t)n_frames * n_faces > (int64_t)1 << 31 ||
      n_verts > (int64_t)1 << 30)
    return DSU_EINVAL;
  if (filtered && (halo < 0 || halo > 2 * ss)) return DSU_EINVAL;
  const int64_t nb = bins_of(n_frames, size);
  if (!workspace || workspace_bytes < dsu_bin::bytes(nb)) return DSU_EINVAL;
  if (n_faces && (!screen || !faces || n_verts == 0)) return DSU_EINVAL;
  if (stage != DSU_RENDER_COUNT && n_items && !items) return DSU_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  RenderView view{cx, cy, span, size, ss, size * ss, (size + RT_TILE - 1) / RT_TILE};
  if (stage != DSU_RENDER_RASTER) {
    const FrameTriangleTiles tiles{screen, faces, n_verts, n_faces, view};
    const int64_t n = (int64_t)n_frames * n_faces;
    if (!filtered) return dsu_bin::run_stage(stage, tiles, n, workspace, nb, items, n_items, st);
    return dsu_bin::run_stage(stage, FrameTriangleGrownTiles{tiles, dsu_film::halo_pixels(halo, ss) * ss}, n,
                              workspace, nb, items, n_items, st);
  }
  if (n_faces && !pos) return DSU_EINVAL;
  if (tex ? !texture_ok(*tex) : (n_faces && !colour)) return DSU_EINVAL;
  if (filtered && !dsu_film::taps_ok(taps, halo, ss)) return DSU_EINVAL;
  const RasterCall call{(unsigned)nb, st, screen, faces, colour, pos, n_verts, n_faces, view,
                        dsu_bin::split(workspace, nb).offsets, items, n_faces ? n_items : 0,
                        tex ? RenderTexture{tex->uv, reinterpret_cast<const uint32_t*>(tex->texels), tex->tex_size,
                                            tex->filter == TEX_ANISO ? tex->max_aniso : 0}
                            : RenderTexture{nullptr, nullptr, 0, 0},
                        out};
  const int source = tex ? tex->filter : TEX_NONE;
  if (!filtered) {
    switch (source) {   // source first, then ss: the order the kernels have in the code object
      case TEX_NONE: call.launch<TEX_NONE>(ss); break;
      case TEX_NEAREST: call.launch<TEX_NEAREST>(ss); break;
      case TEX_BILINEAR: call.launch<TEX_BILINEAR>(ss); break;
      case TEX_TRILINEAR: call.launch<TEX_TRILINEAR>(ss); break;
      case TEX_ANISO: call.launch<TEX_ANISO>(ss); break;
    }
  } else {
    FilmTaps film = {};
    for (int k = 0; k < ss + 2 * halo; ++k) film.t[k] = taps[k];
    film.halo = halo;
    switch (source) {
      case TEX_NONE: call.launch_filtered<TEX_NONE>(ss, film); break;
      case TEX_NEAREST: call.launch_filtered<TEX_NEAREST>(ss, film); break;
      case TEX_BILINEAR: call.launch_filtered<TEX_BILINEAR>(ss, film); break;
      case TEX_TRILINEAR: call.launch_filtered<TEX_TRILINEAR>(ss, film); break;
      case TEX_ANISO: call.launch_filtered<TEX_ANISO>(ss, film); break;
    }
  }
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

}  // namespace

extern "C" {

int64_t dsu_mesh_render_ortho_workspace_bytes(int32_t n_frames, int32_t size) {
  if (n_frames < 1 || n_frames > 4096 || size < 4 || size > 2048 || size % 4) return DSU_EINVAL;
  return dsu_bin::bytes(bins_of(n_frames, size));
}

int dsu_mesh_render_ortho(int32_t stage, const float* screen, const int32_t* faces,
                          const float* colour, const float* pos, const dsu_render_texture* tex,
                          int32_t n_frames, int64_t n_verts, int64_t n_faces, double cx, double cy,
                          double span, int32_t size, int32_t ss, void* workspace, int64_t workspace_bytes,
                          int32_t* items, int64_t n_items, uint8_t* color_u8, uint8_t* pos_u8,
                          int32_t* face_id, float* depth, float* frames, float* pixels, void* stream) {
  return render_ortho(false, stage, screen, faces, colour, pos, tex, n_frames, n_verts, n_faces, cx, cy, span, size,
                      ss, nullptr, 0, workspace, workspace_bytes, items, n_items,
                      RenderOut{color_u8, pos_u8, face_id, depth, frames, pixels}, stream);
}

int dsu_mesh_render_ortho_filtered(int32_t stage, const float* screen, const int32_t* faces, const float* colour,
                                   const float* pos, const dsu_render_texture* tex, int32_t n_frames,
                                   int64_t n_verts, int64_t n_faces, double cx, double cy, double span,
                                   int32_t size, int32_t ss, const double* taps, int32_t halo, void* workspace,
                                   int64_t workspace_bytes, int32_t* items, int64_t n_items, uint8_t* color_u8,
                                   uint8_t* pos_u8, int32_t* face_id, float* depth, float* frames, float* pixels,
                                   void* stream) {
  return render_ortho(true, stage, screen, faces, colour, pos, tex, n_frames, n_verts, n_faces, cx, cy, span, size,
                      ss, taps, halo, workspace, workspace_bytes, items, n_items,
                      RenderOut{color_u8, pos_u8, face_id, depth, frames, pixels}, stream);
}

// HOST: the filtered resolve evaluated on the CPU by the text the kernel compiles (film_filter.h) —
// colour, pos (F,N,N,3) f32 and covered (F,N,N) u8 per sample, N = size ss; every array is host memory.
int dsu_pixel_filter_resolve_host(const float* colour, const float* pos, const uint8_t* covered, int32_t n_frames,
                                  int32_t size, int32_t ss, const double* taps, int32_t halo, float* pixels,
                                  uint8_t* color_u8, uint8_t* pos_u8) {
  if (!view_ok(n_frames, size, ss, 1.0) || !colour || !pos || !covered) return DSU_EINVAL;
  if (!dsu_film::taps_ok(taps, halo, ss)) return DSU_EINVAL;
  const int N = size * ss;
  for (int f = 0; f < n_frames; ++f) {
    const int64_t base = (int64_t)f * N * N;
    for (int i = 0; i < size; ++i)
      for (int j = 0; j < size; ++j) {
        double alpha, v[6];
        dsu_film::gather(taps, halo, ss, N, i, j, [&](int R, int C, float s[6]) {
          const int64_t at = base + (int64_t)R * N + C;
          if (!covered[at]) return false;
          for (int ch = 0; ch < 3; ++ch) {
            s[ch] = colour[at * 3 + ch];
            s[3 + ch] = pos[at * 3 + ch];
          }
          return true;
        }, alpha, v);
        const int64_t pix = ((int64_t)f * size + i) * size + j;
        const uint8_t a8 = (uint8_t)dsu_film::quantise(alpha);
        for (int ch = 0; ch < 3; ++ch) {
          if (pixels) {
            pixels[pix * 8 + ch] = (float)v[ch];
            pixels[pix * 8 + 4 + ch] = (float)v[3 + ch];
          }
          if (color_u8) color_u8[pix * 4 + ch] = (uint8_t)dsu_film::quantise(v[ch]);
          if (pos_u8) pos_u8[pix * 4 + ch] = (uint8_t)dsu_film::quantise(v[3 + ch]);
        }
        if (pixels) pixels[pix * 8 + 3] = pixels[pix * 8 + 7] = (float)alpha;
        if (color_u8) color_u8[pix * 4 + 3] = a8;
        if (pos_u8) pos_u8[pix * 4 + 3] = a8;
      }
  }
  return DSU_OK;
}

int dsu_pos_edge_u8(const uint8_t* pos_rgba, int32_t n_frames, int32_t H, int32_t W, uint8_t* edge,
                    void* stream) {
  if (n_frames < 1 || n_frames > 65535 || H < 2 || W < 2 || H > 65535 || W > 16384 || !pos_rgba || !edge)
    return DSU_EINVAL;
  pos_edge_kernel<<<dim3((W + 255) / 256, H, n_frames), dim3(256), 0, (hipStream_t)stream>>>(pos_rgba, H,
                                                                                             W, edge);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

}  // extern "C"
