// Corrective smoothing ("delta mush") of one vertex in one frame (include/dsu_hip.h, "Corrective
// smoothing"): one text for the three kernels of mesh_corrective.hip (device) and for
// dsu_corrective_bind_host / dsu_corrective_smooth_host (host), so the non-GPU suite pins the
// arithmetic the kernels run.  Everything is float64 from the f32 inputs in the operand order
// written here; the library is compiled with -ffp-contract=off, so no products are fused on either
// side.  tests/corrective_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#define DSU_CS_HD __host__ __device__ __forceinline__

namespace dsu_cs {

// The welded mesh graph (animate/corrective.py, smoothing_topology).  Every index read from it is
// checked against its range before it is used: an entry outside its range is left out of its row.
struct Topology {
  const int32_t* __restrict__ rep;          // (V): representative of each vertex
  const int32_t* __restrict__ nbr_rowptr;   // (V + 1)
  const int32_t* __restrict__ nbr_cols;     // (n_nbr): neighbour representatives, ascending per row
  const int32_t* __restrict__ cor_rowptr;   // (V + 1)
  const int32_t* __restrict__ cor_faces;    // (n_cor): faces that contain the vertex, ascending per row
  const int32_t* __restrict__ faces;        // (M, 3): faces over representatives
  int64_t n_nbr, n_cor, M, V;
};

DSU_CS_HD void row_of(const int32_t* __restrict__ rowptr, int64_t nnz, int64_t v, int64_t& k0, int64_t& k1) {
  k0 = rowptr[v];
  k1 = rowptr[v + 1];
  if (k0 < 0) k0 = 0;
  if (k1 > nnz) k1 = nnz;
}

constexpr int SMOOTH_CHUNK = 8;   // a vertex of a triangle mesh has 6 neighbours on average

DSU_CS_HD bool positive_finite(double x) { return x > 0.0 && x <= 1.7976931348623157e308; }

// One smoothing step of vertex v: q is the (V, 3) f32 buffer of the frame, out the vertex's 3 floats.
DSU_CS_HD void smooth_step(const Topology& T, const float* __restrict__ q, int64_t v, double lam, float* out) {
  int64_t k0, k1;
  row_of(T.nbr_rowptr, T.n_nbr, v, k0, k1);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int64_t deg = 0;
  // SMOOTH_CHUNK entries at a time: first their indices, then their values, then the sums in row
  // order.  The loads are unconditional — an entry past the row's end re-reads the row's last one,
  // an entry that is left out reads the vertex itself — so they are in flight together instead of
  // one dependent chain per neighbour; what is added, and in which order, is the rule's.
  for (int64_t k = k0; k < k1; k += SMOOTH_CHUNK) {
    int64_t j[SMOOTH_CHUNK];
    bool use[SMOOTH_CHUNK];
    float px[SMOOTH_CHUNK], py[SMOOTH_CHUNK], pz[SMOOTH_CHUNK];
#pragma unroll
    for (int u = 0; u < SMOOTH_CHUNK; ++u) j[u] = T.nbr_cols[k + u < k1 ? k + u : k1 - 1];
#pragma unroll
    for (int u = 0; u < SMOOTH_CHUNK; ++u) {
      use[u] = k + u < k1 && j[u] >= 0 && j[u] < T.V;
      const float* __restrict__ p = q + (use[u] ? j[u] : v) * 3;
      px[u] = p[0]; py[u] = p[1]; pz[u] = p[2];
    }
#pragma unroll
    for (int u = 0; u < SMOOTH_CHUNK; ++u) {
      if (!use[u]) continue;
      sx = sx + (double)px[u];
      sy = sy + (double)py[u];
      sz = sz + (double)pz[u];
      ++deg;
    }
  }
  const float* __restrict__ p = q + v * 3;
  if (deg == 0) {
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
    return;
  }
  const double d = (double)deg;
  const double x = p[0], y = p[1], z = p[2];
  out[0] = (float)(x + lam * (sx / d - x));
  out[1] = (float)(y + lam * (sy / d - y));
  out[2] = (float)(z + lam * (sz / d - z));
}

// The local frame (t, b, n) at representative r from the fully smoothed (V, 3) buffer s of the
// frame.  false: there is no frame (t, b, n are then unspecified).
DSU_CS_HD bool frame_at(const Topology& T, const float* __restrict__ s, int64_t r, double t[3], double b[3],
                        double n[3]) {
  int64_t k0, k1;
  row_of(T.nbr_rowptr, T.n_nbr, r, k0, k1);
  int64_t first = -1;
  for (int64_t k = k0; k < k1 && first < 0; ++k) {
    const int64_t j = T.nbr_cols[k];
    if (j >= 0 && j < T.V) first = j;
  }
  if (first < 0) return false;
  row_of(T.cor_rowptr, T.n_cor, r, k0, k1);
  double Nx = 0.0, Ny = 0.0, Nz = 0.0;
  int64_t corners = 0;
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t m = T.cor_faces[k];
    if (m < 0 || m >= T.M) continue;
    const int64_t ia = T.faces[m * 3], ib = T.faces[m * 3 + 1], ic = T.faces[m * 3 + 2];
    if (ia < 0 || ia >= T.V || ib < 0 || ib >= T.V || ic < 0 || ic >= T.V) continue;
    const double ax = s[ia * 3], ay = s[ia * 3 + 1], az = s[ia * 3 + 2];
    const double ux = (double)s[ib * 3] - ax, uy = (double)s[ib * 3 + 1] - ay, uz = (double)s[ib * 3 + 2] - az;
    const double wx = (double)s[ic * 3] - ax, wy = (double)s[ic * 3 + 1] - ay, wz = (double)s[ic * 3 + 2] - az;
    Nx = Nx + (uy * wz - uz * wy);
    Ny = Ny + (uz * wx - ux * wz);
    Nz = Nz + (ux * wy - uy * wx);
    ++corners;
  }
  if (corners == 0) return false;
  const double n2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
  if (!positive_finite(n2)) return false;
  const double nl = sqrt(n2);
  n[0] = Nx / nl; n[1] = Ny / nl; n[2] = Nz / nl;
  const double ex = (double)s[first * 3] - (double)s[r * 3];
  const double ey = (double)s[first * 3 + 1] - (double)s[r * 3 + 1];
  const double ez = (double)s[first * 3 + 2] - (double)s[r * 3 + 2];
  const double en = (ex * n[0] + ey * n[1]) + ez * n[2];
  const double tx = ex - en * n[0], ty = ey - en * n[1], tz = ez - en * n[2];
  const double t2 = (tx * tx + ty * ty) + tz * tz;
  if (!positive_finite(t2)) return false;
  const double tl = sqrt(t2);
  t[0] = tx / tl; t[1] = ty / tl; t[2] = tz / tl;
  b[0] = n[1] * t[2] - n[2] * t[1];
  b[1] = n[2] * t[0] - n[0] * t[2];
  b[2] = n[0] * t[1] - n[1] * t[0];
  return true;
}

// Bind of vertex v (F = 1): rest and s are the rest mesh and its smoothed copy.
DSU_CS_HD void bind_vertex(const Topology& T, const float* __restrict__ rest, const float* __restrict__ s,
                           int64_t v, double* delta, uint8_t* valid) {
  double t[3], b[3], n[3];
  if (!frame_at(T, s, v, t, b, n)) {
    delta[0] = 0.0; delta[1] = 0.0; delta[2] = 0.0;
    *valid = 0;
    return;
  }
  const double dx = (double)rest[v * 3] - (double)s[v * 3];
  const double dy = (double)rest[v * 3 + 1] - (double)s[v * 3 + 1];
  const double dz = (double)rest[v * 3 + 2] - (double)s[v * 3 + 2];
  delta[0] = (t[0] * dx + t[1] * dy) + t[2] * dz;
  delta[1] = (b[0] * dx + b[1] * dy) + b[2] * dz;
  delta[2] = (n[0] * dx + n[1] * dy) + n[2] * dz;
  *valid = 1;
}

// Apply of vertex v in one frame: in and s are the frame's input and fully smoothed buffers.
DSU_CS_HD void apply_vertex(const Topology& T, const float* __restrict__ in, const float* __restrict__ s,
                            const double* __restrict__ delta, const uint8_t* __restrict__ valid, int64_t v,
                            float* out) {
  const int64_t r = T.rep[v];
  double t[3], b[3], n[3];
  if (r < 0 || r >= T.V || !valid[r] || !frame_at(T, s, r, t, b, n)) {
    out[0] = in[v * 3]; out[1] = in[v * 3 + 1]; out[2] = in[v * 3 + 2];
    return;
  }
  const double d0 = delta[r * 3], d1 = delta[r * 3 + 1], d2 = delta[r * 3 + 2];
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (float)((double)s[r * 3 + c] + ((t[c] * d0 + b[c] * d1) + n[c] * d2));
}

}  // namespace dsu_cs
