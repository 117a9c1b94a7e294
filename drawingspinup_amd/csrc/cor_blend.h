// Centre-of-rotation skinning (include/dsu_hip.h, "Centre-of-rotation skinning"; Le & Hodgins 2016):
// the per-triangle, per-pair and per-vertex text, once, for the kernels of mesh_skin.hip (device) and
// for dsu_skin_cor_centres_host / dsu_skin_cor_host (host), so the non-GPU suite pins the arithmetic
// the kernels run.  Everything is float64 in the operand order written here; the library is compiled
// with -ffp-contract=off, so no products are fused on either side.  tests/skin_cor_ref.py restates it
// in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#define DSU_COR_HD __host__ __device__ __forceinline__

namespace dsu_cor {

DSU_COR_HD bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// entries of a canonical row: those before the first joint outside [0, J)
DSU_COR_HD int row_length(const int32_t* __restrict__ j, int K, int J) {
  int n = 0;
  while (n < K && j[n] >= 0 && j[n] < J) ++n;
  return n;
}

// The canonical row of triangle t: its ascending (joint, w^) pairs into tj / tw (at most cap of them),
// geo = (centroid, area).  -> the number of pairs; 0 for a triangle that is skipped (an index outside
// [0, V), an area that is zero or not finite, three vertices without a joint).
DSU_COR_HD int triangle_row(const float* __restrict__ rest, const int32_t* __restrict__ faces, int64_t t, int64_t V,
                            const int32_t* __restrict__ joints, const float* __restrict__ weights, int K, int J,
                            int cap, int32_t* __restrict__ tj, double* __restrict__ tw, double geo[4]) {
  geo[0] = geo[1] = geo[2] = geo[3] = 0.0;
  const int64_t ia = faces[t * 3], ib = faces[t * 3 + 1], ic = faces[t * 3 + 2];
  if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return 0;
  const double ax = rest[ia * 3], ay = rest[ia * 3 + 1], az = rest[ia * 3 + 2];
  const double bx = rest[ib * 3], by = rest[ib * 3 + 1], bz = rest[ib * 3 + 2];
  const double cx = rest[ic * 3], cy = rest[ic * 3 + 1], cz = rest[ic * 3 + 2];
  const double ux = bx - ax, uy = by - ay, uz = bz - az;
  const double vx = cx - ax, vy = cy - ay, vz = cz - az;
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const double area = sqrt((nx * nx + ny * ny) + nz * nz) / 2.0;
  if (!(area > 0.0 && finite(area))) return 0;
  const int32_t* __restrict__ ja = joints + ia * K;
  const int32_t* __restrict__ jb = joints + ib * K;
  const int32_t* __restrict__ jc = joints + ic * K;
  const int na = row_length(ja, K, J), nb = row_length(jb, K, J), nc = row_length(jc, K, J);
  int pa = 0, pb = 0, pc = 0, n = 0;
  while (n < cap && (pa < na || pb < nb || pc < nc)) {
    int32_t j = 0x7fffffff;
    if (pa < na && ja[pa] < j) j = ja[pa];
    if (pb < nb && jb[pb] < j) j = jb[pb];
    if (pc < nc && jc[pc] < j) j = jc[pc];
    double wa = 0.0, wb = 0.0, wc = 0.0;
    if (pa < na && ja[pa] == j) wa = (double)weights[ia * K + pa++];
    if (pb < nb && jb[pb] == j) wb = (double)weights[ib * K + pb++];
    if (pc < nc && jc[pc] == j) wc = (double)weights[ic * K + pc++];
    tj[n] = j;
    tw[n] = ((wa + wb) + wc) / 3.0;
    ++n;
  }
  if (n == 0) return 0;
  geo[0] = ((ax + bx) + cx) / 3.0;
  geo[1] = ((ay + by) + cy) / 3.0;
  geo[2] = ((az + bz) + cz) / 3.0;
  geo[3] = area;
  return n;
}

// One joint pair j < k of the similarity: W_i(j), W_i(k), w^_t(j), w^_t(k), all non-zero; s2 = sigma^2.
DSU_COR_HD double pair_term(double wj, double wk, double tj, double tk, double s2) {
  const double d = wj * tk - wk * tj;
  return (((wj * wk) * tj) * tk) * exp(-(d * d) / s2);
}

// s(i, t) of a vertex row (vj, vw; nv entries) and a triangle row (tj, tw; nt entries), both
// ascending: the pairs of shared joints in ascending (j, k) order, added from 0.  A pair with a zero
// factor contributes nothing (a canonical table has none; one made elsewhere may), and no exponential
// is evaluated when fewer than two joints are shared.
DSU_COR_HD double similarity(const int32_t* __restrict__ vj, const float* __restrict__ vw, int nv,
                             const int32_t* __restrict__ tj, const double* __restrict__ tw, int nt, double s2) {
  double s = 0.0;
  int ea = 0;
  for (int a = 0; a + 1 < nv; ++a) {
    while (ea < nt && tj[ea] < vj[a]) ++ea;
    if (ea >= nt) break;
    if (tj[ea] != vj[a]) continue;
    const double wa = (double)vw[a], ta = tw[ea];
    if (wa == 0.0 || ta == 0.0) continue;
    int eb = ea + 1;
    for (int b = a + 1; b < nv; ++b) {
      while (eb < nt && tj[eb] < vj[b]) ++eb;
      if (eb >= nt) break;
      if (tj[eb] != vj[b]) continue;
      const double wb = (double)vw[b], tb = tw[eb];
      if (wb == 0.0 || tb == 0.0) continue;
      s = s + pair_term(wa, wb, ta, tb, s2);
    }
  }
  return s;
}

// acc = (num_x, num_y, num_z, den) += one triangle
DSU_COR_HD void add_triangle(double acc[4], double s, const double* __restrict__ geo) {
  const double sa = s * geo[3];
  acc[0] = acc[0] + sa * geo[0];
  acc[1] = acc[1] + sa * geo[1];
  acc[2] = acc[2] + sa * geo[2];
  acc[3] = acc[3] + sa;
}

DSU_COR_HD void finish(const double acc[4], double* __restrict__ centre, uint8_t* __restrict__ valid) {
  const bool ok = acc[3] > 0.0 && finite(acc[3]) && finite(acc[0]) && finite(acc[1]) && finite(acc[2]);
  centre[0] = ok ? acc[0] / acc[3] : 0.0;
  centre[1] = ok ? acc[1] / acc[3] : 0.0;
  centre[2] = ok ? acc[2] / acc[3] : 0.0;
  *valid = ok ? 1 : 0;
}

// L(p) of the contributing influences (an influence outside [0, J) or with a weight that is not > 0
// contributes nothing); mats: the (J, 12) matrices [R | t] of the frame.
DSU_COR_HD void linear(const int32_t* __restrict__ infl, const float* __restrict__ w, int K,
                       const double* __restrict__ mats, int J, double px, double py, double pz, double L[3]) {
  L[0] = L[1] = L[2] = 0.0;
  for (int k = 0; k < K; ++k) {
    const int jn = infl[k];
    if (jn < 0 || jn >= J) continue;
    const double wk = (double)w[k];
    if (!(wk > 0.0)) continue;
    const double* __restrict__ m = mats + (int64_t)jn * 12;
    L[0] = L[0] + wk * (((m[0] * px + m[1] * py) + m[2] * pz) + m[3]);
    L[1] = L[1] + wk * (((m[4] * px + m[5] * py) + m[6] * pz) + m[7]);
    L[2] = L[2] + wk * (((m[8] * px + m[9] * py) + m[10] * pz) + m[11]);
  }
}

// One vertex in one frame.  quats: the (J, 4) unit quaternions (w, x, y, z) of the frame; centre,
// valid: the vertex's centre of rotation.
DSU_COR_HD void blend(const int32_t* __restrict__ infl, const float* __restrict__ w, int K,
                      const double* __restrict__ mats, const double* __restrict__ quats, int J, float xf, float yf,
                      float zf, const double* __restrict__ centre, uint8_t valid, float out[3]) {
  const double x = xf, y = yf, z = zf;
  double L[3];
  if (!valid) {
    linear(infl, w, K, mats, J, x, y, z, L);
    out[0] = (float)L[0]; out[1] = (float)L[1]; out[2] = (float)L[2];
    return;
  }
  const double px = centre[0], py = centre[1], pz = centre[2];
  double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;   // the pivot's rotation
  bool has = false;
  // M = sum_k w_k (y_k - p*), y_k = R_k p* + t_k: the displacement of the centre under the linear blend
  L[0] = L[1] = L[2] = 0.0;
  for (int k = 0; k < K; ++k) {
    const int jn = infl[k];
    if (jn < 0 || jn >= J) continue;
    const double wk = (double)w[k];
    if (!(wk > 0.0)) continue;
    const double* __restrict__ m = mats + (int64_t)jn * 12;
    L[0] = L[0] + wk * ((((m[0] * px + m[1] * py) + m[2] * pz) + m[3]) - px);
    L[1] = L[1] + wk * ((((m[4] * px + m[5] * py) + m[6] * pz) + m[7]) - py);
    L[2] = L[2] + wk * ((((m[8] * px + m[9] * py) + m[10] * pz) + m[11]) - pz);
    const double* __restrict__ q = quats + (int64_t)jn * 4;
    if (!has) {
      p0 = q[0]; p1 = q[1]; p2 = q[2]; p3 = q[3];
      has = true;
    }
    const double dot = ((q[0] * p0 + q[1] * p1) + q[2] * p2) + q[3] * p3;
    const double sw = dot < 0.0 ? -wk : wk;
    b0 = b0 + sw * q[0]; b1 = b1 + sw * q[1]; b2 = b2 + sw * q[2]; b3 = b3 + sw * q[3];
  }
  const double n2 = ((b0 * b0 + b1 * b1) + b2 * b2) + b3 * b3;
  // no contributing influence, rotations that cancel, NaN or overflow: the linear blend of x
  if (!(n2 > 0.0 && finite(n2))) {
    linear(infl, w, K, mats, J, x, y, z, L);
    out[0] = (float)L[0]; out[1] = (float)L[1]; out[2] = (float)L[2];
    return;
  }
  const double n = sqrt(n2);
  const double rw = b0 / n, rx = b1 / n, ry = b2 / n, rz = b3 / n;
  // the rotation moves d = x - p* by 2 r_w (r_v x d) + 2 r_v x (r_v x d); x itself is the leading term,
  // so identity transforms (M = 0, r_v = 0) return x bit for bit
  const double dx = x - px, dy = y - py, dz = z - pz;
  const double ax = ry * dz - rz * dy, ay = rz * dx - rx * dz, az = rx * dy - ry * dx;
  const double cx = ry * az - rz * ay, cy = rz * ax - rx * az, cz = rx * ay - ry * ax;
  const double w2 = 2.0 * rw;
  out[0] = (float)(x + (L[0] + (w2 * ax + 2.0 * cx)));
  out[1] = (float)(y + (L[1] + (w2 * ay + 2.0 * cy)));
  out[2] = (float)(z + (L[2] + (w2 * az + 2.0 * cz)));
}

}  // namespace dsu_cor
