// The thickness map's rule (include/dsu_hip.h, "Thickness map"), stated once: compiled for the
// kernel (mesh_thickness.hip) and for dsu_mesh_thickness_ortho_host, restated in float64 numpy by
// tests/mesh_thickness_ref.py.  Float64 from the f32 inputs, one operand order (-ffp-contract=off).
#pragma once
#include "common.h"

namespace dsu_mt {

// One triangle as the samples see it: its f32 coordinates and its face index (< 0: ignored).
struct Tri {
  float ax, ay, az, bx, by, bz, cx, cy, cz;
  int32_t face;
};

// x - x is 0 for a finite x and NaN for an infinity or a NaN (host and device alike)
__host__ __device__ __forceinline__ bool finite3(float x, float y, float z) {
  return x - x == 0.0f && y - y == 0.0f && z - z == 0.0f;
}

// Face f of the mesh; face = -1 when f is outside [0, T), an index is outside [0, V) or a
// coordinate is not finite.
__host__ __device__ __forceinline__ Tri load_tri(const float* __restrict__ verts, int64_t V,
                                                 const int32_t* __restrict__ faces, int64_t T, int64_t f) {
  Tri t;
  t.face = -1;
  t.ax = t.ay = t.az = t.bx = t.by = t.bz = t.cx = t.cy = t.cz = 0.0f;
  if (f < 0 || f >= T) return t;
  const int64_t ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return t;
  t.ax = verts[ia * 3]; t.ay = verts[ia * 3 + 1]; t.az = verts[ia * 3 + 2];
  t.bx = verts[ib * 3]; t.by = verts[ib * 3 + 1]; t.bz = verts[ib * 3 + 2];
  t.cx = verts[ic * 3]; t.cy = verts[ic * 3 + 1]; t.cz = verts[ic * 3 + 2];
  if (finite3(t.ax, t.ay, t.az) && finite3(t.bx, t.by, t.bz) && finite3(t.cx, t.cy, t.cz)) t.face = (int32_t)f;
  return t;
}

// Centre of sample `i` (a column or a row) of a lattice that starts at v0 with step h.
__host__ __device__ __forceinline__ double sample_at(double v0, int32_t i, double h) {
  return v0 + ((double)i + 0.5) * h;
}

// E(p -> q) at s, and whether the sample is on the inner side of the edge: E > 0, or E == 0 on a
// top-left edge of the counter-clockwise triangle.
__host__ __device__ __forceinline__ bool edge_covers(double px, double py, double qx, double qy, double sx,
                                                     double sy, double& E) {
  const double dx = qx - px, dy = qy - py;
  E = dx * (sy - py) - dy * (sx - px);
  return E > 0.0 || (E == 0.0 && (dy < 0.0 || (dy == 0.0 && dx < 0.0)));
}

// Does the ray through (sx, sy) cross the triangle, and at which z.
__host__ __device__ __forceinline__ bool crossing(const Tri& t, double sx, double sy, double& z) {
  if (t.face < 0) return false;
  const double ax = t.ax, ay = t.ay, az = t.az;
  double bx = t.bx, by = t.by, bz = t.bz, cx = t.cx, cy = t.cy, cz = t.cz;
  double area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
  if (area2 == 0.0) return false;
  if (area2 < 0.0) {                          // make it counter-clockwise: swap b and c
    double s;
    s = bx; bx = cx; cx = s;
    s = by; by = cy; cy = s;
    s = bz; bz = cz; cz = s;
    area2 = -area2;                           // exactly the swapped triangle's area2
  }
  double eab, ebc, eca;
  if (!edge_covers(ax, ay, bx, by, sx, sy, eab)) return false;
  if (!edge_covers(bx, by, cx, cy, sx, sy, ebc)) return false;
  if (!edge_covers(cx, cy, ax, ay, sx, sy, eca)) return false;
  z = ((ebc / area2) * az + (eca / area2) * bz) + (eab / area2) * cz;
  return true;
}

// The crossings of one sample are visited in the order (z, face), one pair per walk over its
// triangles: `cur` is the crossing last visited, `lo` and `hi` the two lowest ones above it met so
// far in this walk.
struct Key {
  double z;
  int32_t face;   // < 0: none
};

__host__ __device__ __forceinline__ bool above(double z, int32_t face, const Key& k) {
  return k.face < 0 || z > k.z || (z == k.z && face > k.face);
}
__host__ __device__ __forceinline__ bool below(double z, int32_t face, const Key& k) {
  return k.face < 0 || z < k.z || (z == k.z && face < k.face);
}

// One triangle of a walk.  FIRST: the walk that starts below every crossing and also counts them.
template <bool FIRST>
__host__ __device__ __forceinline__ void visit(const Tri& t, double sx, double sy, const Key& cur, Key& lo, Key& hi,
                                               int32_t& count) {
  double z;
  if (!crossing(t, sx, sy, z)) return;
  if (FIRST) ++count;
  if (!FIRST && !above(z, t.face, cur)) return;
  if (below(z, t.face, lo)) {
    hi = lo;
    lo.z = z;
    lo.face = t.face;
  } else if (below(z, t.face, hi)) {
    hi.z = z;
    hi.face = t.face;
  }
}

// The pairing: crossings (0,1), (2,3), ... in visiting order; the thickest pair wins, ties go to the
// lower z (the earlier pair).
struct Pairs {
  double z0, mid, thickness;
  int32_t taken;   // crossings visited
  bool any;
};

__host__ __device__ __forceinline__ Pairs no_pairs() { return Pairs{0.0, 0.0, 0.0, 0, false}; }

__host__ __device__ __forceinline__ void take(Pairs& p, double z) {
  if ((p.taken & 1) == 0) {
    p.z0 = z;
  } else {
    const double th = z - p.z0;
    if (!p.any || th > p.thickness) {
      p.thickness = th;
      p.mid = (p.z0 + z) / 2.0;
      p.any = true;
    }
  }
  ++p.taken;
}

}  // namespace dsu_mt
