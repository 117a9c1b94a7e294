// Device helpers shared by the mesh stages (mesh_post, mesh_render, mesh_skin, mesh_uv).
#pragma once
#include "common.h"

// The three vertex indices of face m, or false when one of them is outside [0, V).
__device__ __forceinline__ bool face_indices(const int32_t* __restrict__ faces, int64_t m, int64_t V,
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
__device__ __forceinline__ void edge_functions(const TriXY& t, double px, double py, double& w0,
                                               double& w1, double& w2) {
  w0 = (px - t.bx) * (t.cy - t.by) - (py - t.by) * (t.cx - t.bx);
  w1 = (px - t.cx) * (t.ay - t.cy) - (py - t.cy) * (t.ax - t.cx);
  w2 = (px - t.ax) * (t.by - t.ay) - (py - t.ay) * (t.bx - t.ax);
}

// inside or on the boundary, either orientation
__device__ __forceinline__ bool covers(double w0, double w1, double w2) {
  return (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0);
}
