// Dual-quaternion blend of one vertex in one frame (include/dsu_hip.h, "Dual-quaternion skinning"):
// one text for skin_dqs_kernel of mesh_skin.hip (device) and for dsu_skin_dqs_host (host), so the
// non-GPU suite pins the arithmetic the kernel runs.  Everything is float64 in the operand order
// written here; the library is compiled with -ffp-contract=off, so no products are fused on either
// side.  tests/skin_dqs_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#define DSU_DQS_HD __host__ __device__ __forceinline__

namespace dsu_dqs {

// infl, w: the K influences of the vertex; table: the (J, 8) dual quaternions of the frame,
// [r_w r_x r_y r_z | d_w d_x d_y d_z]; x, y, z: the rest position; out: the skinned position.
DSU_DQS_HD void blend(const int32_t* __restrict__ infl, const float* __restrict__ w, int K,
                      const double* __restrict__ table, int J, float xf, float yf, float zf, float out[3]) {
  double b[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;   // the pivot's rotation
  bool has = false;
  for (int k = 0; k < K; ++k) {
    const int jn = infl[k];
    if (jn < 0 || jn >= J) continue;
    const double wk = (double)w[k];
    if (!(wk > 0.0)) continue;
    const double* __restrict__ q = table + (int64_t)jn * 8;
    if (!has) {
      p0 = q[0]; p1 = q[1]; p2 = q[2]; p3 = q[3];
      has = true;
    }
    // q and -q are the same transform: take the one on the pivot's side (the pivot itself: +1)
    const double dot = ((q[0] * p0 + q[1] * p1) + q[2] * p2) + q[3] * p3;
    const double sw = dot < 0.0 ? -wk : wk;
#pragma unroll
    for (int c = 0; c < 8; ++c) b[c] = b[c] + sw * q[c];
  }
  const double n2 = ((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) + b[3] * b[3];
  // no contributing influence, rotations that cancel, NaN or overflow: the rest position
  if (!(n2 > 0.0 && n2 <= 1.7976931348623157e308)) {
    out[0] = xf; out[1] = yf; out[2] = zf;
    return;
  }
  const double n = sqrt(n2);
  const double rw = b[0] / n, rx = b[1] / n, ry = b[2] / n, rz = b[3] / n;
  const double dw = b[4] / n, dx = b[5] / n, dy = b[6] / n, dz = b[7] / n;
  // t = 2 (r_w d_v - d_w r_v + r_v x d_v)
  const double tx = 2.0 * ((rw * dx - dw * rx) + (ry * dz - rz * dy));
  const double ty = 2.0 * ((rw * dy - dw * ry) + (rz * dx - rx * dz));
  const double tz = 2.0 * ((rw * dz - dw * rz) + (rx * dy - ry * dx));
  // x' = x + 2 r_w (r_v x x) + 2 r_v x (r_v x x)
  const double x = xf, y = yf, z = zf;
  const double ax = ry * z - rz * y, ay = rz * x - rx * z, az = rx * y - ry * x;
  const double cx = ry * az - rz * ay, cy = rz * ax - rx * az, cz = rx * ay - ry * ax;
  const double w2 = 2.0 * rw;
  out[0] = (float)(((x + w2 * ax) + 2.0 * cx) + tx);
  out[1] = (float)(((y + w2 * ay) + 2.0 * cy) + ty);
  out[2] = (float)(((z + w2 * az) + 2.0 * cz) + tz);
}

}  // namespace dsu_dqs
