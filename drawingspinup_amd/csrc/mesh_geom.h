// Device helpers shared by the mesh stages (mesh_post, mesh_render, mesh_skin, mesh_uv).
#pragma once
#include "common.h"

// The three vertex indices of face m, or false when one of them is outside [0, V).  (Host as well:
// uv_field.h compiles its text for both.)
__host__ __device__ __forceinline__ bool face_indices(const int32_t* __restrict__ faces, int64_t m, int64_t V,
                                             int& ia, int& ib, int& ic) {
  ia = faces[m * 3];
  ib = faces[m * 3 + 1];
  ic = faces[m * 3 + 2];
  return ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V;
}

struct TriXY {
  double ax, ay, bx, by, cx, cy;
};

// fmin / fmax drop a NaN operand, so a bounding box cannot tell: ask the six coordinates
__device__ __forceinline__ bool finite_xy(const TriXY& t) {
  return isfinite(t.ax) && isfinite(t.ay) && isfinite(t.bx) && isfinite(t.by) && isfinite(t.cx) && isfinite(t.cy);
}

// 2-D edge functions in float64: w0 weighs vertex a (edge b->c), w1 b (c->a), w2 c (a->b).  The
// operand order is part of the result (-ffp-contract=off): every user gets the same bits.
__host__ __device__ __forceinline__ void edge_functions(const TriXY& t, double px, double py, double& w0,
                                               double& w1, double& w2) {
  w0 = (px - t.bx) * (t.cy - t.by) - (py - t.by) * (t.cx - t.bx);
  w1 = (px - t.cx) * (t.ay - t.cy) - (py - t.cy) * (t.ax - t.cx);
  w2 = (px - t.ax) * (t.by - t.ay) - (py - t.ay) * (t.bx - t.ax);
}

// inside or on the boundary, either orientation
__host__ __device__ __forceinline__ bool covers(double w0, double w1, double w2) {
  return (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0);
}

// Uniform xy grid of the z-parallel queries (mesh_post.hip builds it, mesh_uv.hip reads it too).
struct ZGrid {
  float x0, y0, inv_cell;
  int32_t g;   // cells per axis
};

__host__ __device__ __forceinline__ int cell_of(float v, float v0, float inv_cell, int g) {
  int c = (int)floorf((v - v0) * inv_cell);
  return min(max(c, 0), g - 1);
}

// uv * size in float64 from the f32 uv
__host__ __device__ __forceinline__ TriXY uv_tri(const float* __restrict__ uvs, int ia, int ib, int ic, double S) {
  TriXY t;
  t.ax = (double)uvs[(int64_t)ia * 2] * S; t.ay = (double)uvs[(int64_t)ia * 2 + 1] * S;
  t.bx = (double)uvs[(int64_t)ib * 2] * S; t.by = (double)uvs[(int64_t)ib * 2 + 1] * S;
  t.cx = (double)uvs[(int64_t)ic * 2] * S; t.cy = (double)uvs[(int64_t)ic * 2 + 1] * S;
  return t;
}

// The atlas raster's edge functions.  Not edge_functions above: the operands are in the other order,
// every value is the exact negation of that form, and the uv kernels accept this orientation only.
__host__ __device__ __forceinline__ void uv_edges(const TriXY& t, double px, double py, double& w0,
                                                  double& w1, double& w2) {
  w0 = (t.cx - t.bx) * (py - t.by) - (t.cy - t.by) * (px - t.bx);
  w1 = (t.ax - t.cx) * (py - t.cy) - (t.ay - t.cy) * (px - t.cx);
  w2 = (t.bx - t.ax) * (py - t.ay) - (t.by - t.ay) * (px - t.ax);
}
