// The float64 arithmetic of the quadric edge-collapse decimation, one text for the serial queue
// (mesh_decimate.hip, host) and the device rounds (mesh_decimate_gpu.hip): the queue finishes what the
// rounds began, from the quadrics they accumulated, so both must price an edge, place its target
// and refuse a flip by the same rule to the bit.  The library is compiled with -ffp-contract=off: no
// products are fused on either side, and the operand order is the one written here.
// How a file finds its triangles, boundary edges and links stays in that file.
#pragma once
#include <math.h>

#define DSU_DQ_HD __host__ __device__ __forceinline__

namespace dsu_dq {

struct V3 {
  double x, y, z;
};
DSU_DQ_HD V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
DSU_DQ_HD V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
DSU_DQ_HD V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
DSU_DQ_HD double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DSU_DQ_HD V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
DSU_DQ_HD double norm(V3 a) { return sqrt(dot(a, a)); }
DSU_DQ_HD V3 unit(V3 a, double l) { return a * (1.0 / l); }        // l = norm(a) > 0

struct Row4 {
  double c[4];
};
DSU_DQ_HD void swap_if(Row4& a, Row4& b, bool s) {
  if (s) { const Row4 t = a; a = b; b = t; }
}
DSU_DQ_HD void eliminate(Row4& r, const Row4& piv, int col) {
  const double f = r.c[col] / piv.c[col];
  for (int k = 0; k < 4; ++k) r.c[k] -= f * piv.c[k];
}

// symmetric 4x4 [A b; b^T c]: error(v) = v^T A v + 2 b^T v + c, as the ten doubles of the C ABI:
// a00 a01 a02 a11 a12 a22 b0 b1 b2 c.  Zero when made.
struct Quadric {
  double q[10] = {};

  DSU_DQ_HD void add(const Quadric& o) {
    for (int i = 0; i < 10; ++i) q[i] += o.q[i];
  }
  // w x the quadric of the plane n . x + d = 0
  DSU_DQ_HD void add_plane(V3 n, double d, double w) {
    q[0] += w * n.x * n.x; q[1] += w * n.x * n.y; q[2] += w * n.x * n.z;
    q[3] += w * n.y * n.y; q[4] += w * n.y * n.z; q[5] += w * n.z * n.z;
    q[6] += w * n.x * d; q[7] += w * n.y * d; q[8] += w * n.z * d;
    q[9] += w * d * d;
  }
  DSU_DQ_HD double eval(V3 v) const {
    return v.x * (q[0] * v.x + 2 * q[1] * v.y + 2 * q[2] * v.z) + v.y * (q[3] * v.y + 2 * q[4] * v.z) +
           q[5] * v.z * v.z + 2 * (q[6] * v.x + q[7] * v.y + q[8] * v.z) + q[9];
  }
  // minimiser -A^-1 b when A is well conditioned relative to its own scale, as o + d with
  // A d = -(b + A o) for a point o near the answer (the edge's midpoint), by elimination with
  // partial pivoting.  Not the cofactor inverse: on a near-planar quadric (eigenvalues l1 >> l2 of
  // A) every 2x2 minor cancels to ~l1 l2 with rounding eps l1^2, which puts a factor l1 / l2 on top
  // of the eps cond(A) |x| a stable solve loses — 8e-8 on marching-cubes vertices at |x| ~ 20,
  // cond(A) = 3e4.  About o the right-hand side is small, so what is left is eps cond(A) |x| from
  // its rounding.  The determinant still decides whether to solve at all.
  DSU_DQ_HD bool minimum(V3 o, V3& out) const {
    const double a00 = q[0], a01 = q[1], a02 = q[2], a11 = q[3], a12 = q[4], a22 = q[5];
    const double b0 = q[6], b1 = q[7], b2 = q[8];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double tr = a00 + a11 + a22;
    if (!(tr > 0.0) || !(fabs(det) > 1e-9 * tr * tr * tr)) return false;
    Row4 r0 = {{a00, a01, a02, -(b0 + (a00 * o.x + a01 * o.y + a02 * o.z))}};
    Row4 r1 = {{a01, a11, a12, -(b1 + (a01 * o.x + a11 * o.y + a12 * o.z))}};
    Row4 r2 = {{a02, a12, a22, -(b2 + (a02 * o.x + a12 * o.y + a22 * o.z))}};
    swap_if(r0, r1, fabs(r1.c[0]) > fabs(r0.c[0]));
    swap_if(r0, r2, fabs(r2.c[0]) > fabs(r0.c[0]));
    if (!(fabs(r0.c[0]) > 0.0)) return false;
    eliminate(r1, r0, 0);
    eliminate(r2, r0, 0);
    swap_if(r1, r2, fabs(r2.c[1]) > fabs(r1.c[1]));
    if (!(fabs(r1.c[1]) > 0.0)) return false;
    eliminate(r2, r1, 1);
    if (!(fabs(r2.c[2]) > 0.0)) return false;
    const double z = r2.c[3] / r2.c[2];
    const double y = (r1.c[3] - r1.c[2] * z) / r1.c[1];
    const double x = (r0.c[3] - r0.c[1] * y - r0.c[2] * z) / r0.c[0];
    out = {o.x + x, o.y + y, o.z + z};
    return true;
  }
};

// Collapsing the edge between p0 and p1, q the sum of their quadrics: where the merged vertex goes
// and what that costs.  The minimiser of q when its 3x3 block is well conditioned, otherwise the
// best of {p0, p1, midpoint}.  (The sum and not its two terms: a caller adds them before it loads the
// positions, the order the rounds' kernels were generated in; see
// profiles/decimate_one_text_asm_identity.txt for this and the shapes of the functions below.)
DSU_DQ_HD void edge_target(const Quadric& q, V3 p0, V3 p1, double& cost, V3& vbar) {
  const V3 mid = (p0 + p1) * 0.5;
  if (q.minimum(mid, vbar)) {
    // a minimiser far outside the edge's neighbourhood means the conditioning test was too kind
    const double len = norm(p1 - p0);
    if (norm(vbar - mid) <= 4.0 * len) {
      cost = q.eval(vbar);
      return;
    }
  }
  const V3 cand[3] = {p0, p1, (p0 + p1) * 0.5};
  cost = q.eval(cand[0]);
  vbar = cand[0];
  for (int i = 1; i < 3; ++i) {
    const double c = q.eval(cand[i]);
    if (c < cost) { cost = c; vbar = cand[i]; }
  }
}

// The planes of the initial quadrics, as what add_plane takes.
struct Plane {
  V3 n;
  double d, w;
};
// A triangle's own plane, weighted by its area: cr = cross(pb - pa, pc - pa), l = norm(cr) > 0.
DSU_DQ_HD Plane face_plane(V3 cr, double l, V3 pa) {
  const V3 n = unit(cr, l);
  return {n, -dot(n, pa), 0.5 * l};
}
// The plane through a boundary edge perpendicular to its triangle, weighted by boundary_weight x the
// triangle's area: plo, phi the end points of the lower and the higher vertex index, n = unit(cr, l)
// the triangle's normal (face_plane's).  In two steps with the caller's test between them, as for
// the face: en = boundary_cross(plo, phi, n), el = norm(en) > 0 (the edge has a length).
DSU_DQ_HD V3 boundary_cross(V3 plo, V3 phi, V3 n) { return cross(phi - plo, n); }
DSU_DQ_HD Plane boundary_plane(V3 en, double el, V3 plo, double l, double boundary_weight) {
  en = unit(en, el);
  return {en, -dot(en, plo), boundary_weight * 0.5 * l};
}

// Does the triangle p turn its normal over when its corners go to q?
DSU_DQ_HD bool flips(const V3 (&p)[3], const V3 (&q)[3]) {
  const V3 before = cross(p[1] - p[0], p[2] - p[0]);
  const V3 after = cross(q[1] - q[0], q[2] - q[0]);
  return dot(before, after) < 0.0;
}

}  // namespace dsu_dq
