// Rigging of the reconstructed mesh (blender_animation.py:38-44 binds it to the armature with
// Blender's automatic bone-heat weights, then Blender skins it per frame): the three device steps
// of drawingspinup_amd/animate/skin.py (gfx950).
//
//   dsu_bone_visibility   for every (vertex, bone): distance to the bone's segment and whether the
//                         open segment vertex -> closest point is crossed by a triangle
//   dsu_spd_cg_block      (L + M H) W = M H P, all bones at once: Jacobi-preconditioned CG, float64
//   dsu_skin_lbs          out[f, v] = sum_k w_k (R_k x + t_k)
//   dsu_skin_dqs          out[f, v] = the rigid transform of the blended unit dual quaternion
//                         (dqs_blend.h; dsu_skin_dqs_host runs the same text on host arrays)
//   dsu_skin_cor_centres  once per character: every vertex's centre of rotation, a sum over all
//                         (vertex, triangle) pairs (cor_blend.h; brute force, the hot one of this blend)
//   dsu_skin_cor          out[f, v] = x + the linear blend's displacement of the centre p* + the blended
//                         rotation's displacement of (x - p*)
//
// The rules (include/dsu_hip.h states them in full; tests/skin_ref.py restates them in float64).
//
// Shape of the visibility work (the hot one: V * B segments against M triangles): triangles are
// binned on a uniform 3-D grid by the cells their bounding box touches (the counting sort of
// bin_sort.h).  One workgroup takes 256
// vertices (in the caller's order: sorted by cell, so that they are neighbours) and ONE bone:
// their segments run side by side, so the union of their boxes is slim.  The workgroup walks the
// rows of cells of that union box — a row along x is one contiguous range of the item list —
// stages 256 triangles at a time in LDS (9 f32 coordinates + 3 indices each, 12 KB, structure of
// arrays: every lane reads the same address, a broadcast) and every lane tests its own segment
// against each staged triangle whose box meets its segment's box.  A triangle listed in several
// cells is tested several times; the answer is an OR, so the order and the repeats do not matter.
// The walk stops as soon as every segment of the workgroup is blocked.
#include <new>
#include <vector>

#include "common.h"
#include "bin_sort.h"
#include "mesh_geom.h"
#include "partial_reduce.h"
#include "dqs_blend.h"
#include "cor_blend.h"

namespace {

// ------------------------------------------------------------------ grid
struct SkinGrid {
  double x0, y0, z0, cell;
  int32_t gx, gy, gz;
};

// floor((x - lo) / cell) clamped to [0, g - 1]; monotone in x, NaN -> 0
__device__ __forceinline__ int cell_of(double x, double lo, double cell, int g) {
  const double t = floor((x - lo) / cell);
  return (int)fmin(fmax(t, 0.0), (double)(g - 1));
}

// bin_sort.h source: triangle m goes to every cell its 3-D box touches.  cell = (cz gy + cy) gx + cx.
struct TriangleCells3 {
  const float* __restrict__ verts;
  const int32_t* __restrict__ faces;
  int64_t V;
  SkinGrid g;
  __device__ __forceinline__ int32_t id(int64_t m) const { return (int32_t)m; }
  template <class Emit>
  __device__ __forceinline__ void bins(int64_t m, Emit emit) const {
    int ia, ib, ic;
    if (!face_indices(faces, m, V, ia, ib, ic)) return;
    int lo[3], hi[3];
    const double o[3] = {g.x0, g.y0, g.z0};
    const int n[3] = {g.gx, g.gy, g.gz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double u = verts[(int64_t)ia * 3 + a], v = verts[(int64_t)ib * 3 + a], w = verts[(int64_t)ic * 3 + a];
      if (!(isfinite(u) && isfinite(v) && isfinite(w))) return;
      lo[a] = cell_of(fmin(fmin(u, v), w), o[a], g.cell, n[a]);
      hi[a] = cell_of(fmax(fmax(u, v), w), o[a], g.cell, n[a]);
    }
    for (int cz = lo[2]; cz <= hi[2]; ++cz)
      for (int cy = lo[1]; cy <= hi[1]; ++cy)
        for (int cx = lo[0]; cx <= hi[0]; ++cx) emit((cz * g.gy + cy) * g.gx + cx);
  }
};

// ------------------------------------------------------------------ distance and visibility
// a . (b x c), in this order; no products are fused (-ffp-contract=off)
__device__ __forceinline__ double triple(double ax, double ay, double az, double bx, double by, double bz,
                                         double cx, double cy, double cz) {
  return (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
}

constexpr int VIS_CHUNK = 256;

__global__ __launch_bounds__(256) void bone_visibility_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ faces, const float* __restrict__ bones,
    int64_t V, int64_t M, int32_t B, const int32_t* __restrict__ order, SkinGrid g,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ items, int64_t n_items,
    double* __restrict__ dist, uint8_t* __restrict__ visible) {
  __shared__ float tc[9][VIS_CHUNK];     // staged triangles: ux uy uz vx vy vz wx wy wz
  __shared__ int32_t ti[3][VIS_CHUNK];   // their vertex indices (-1: skip)
  __shared__ int32_t ubox[6];            // union of the workgroup's segment boxes, in cells
  const int tid = threadIdx.x;
  const int j = blockIdx.y;
  const int64_t slot = blockIdx.x * (int64_t)blockDim.x + tid;
  int64_t vi = -1;
  if (slot < V) {
    vi = order ? (int64_t)order[slot] : slot;
    if (vi < 0 || vi >= V) vi = -1;
  }
  if (tid < 3) ubox[tid] = 0x7fffffff;
  else if (tid < 6) ubox[tid] = -1;
  __syncthreads();

  double px = 0, py = 0, pz = 0, qx = 0, qy = 0, qz = 0, ex = 0, ey = 0, ez = 0;
  double lox = 0, loy = 0, loz = 0, hix = 0, hiy = 0, hiz = 0;
  bool alive = false;
  if (vi >= 0) {
    px = verts[vi * 3]; py = verts[vi * 3 + 1]; pz = verts[vi * 3 + 2];
    const float* bj = bones + (int64_t)j * 6;
    const double ax = bj[0], ay = bj[1], az = bj[2];
    const double abx = (double)bj[3] - ax, aby = (double)bj[4] - ay, abz = (double)bj[5] - az;
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double den = (abx * abx + aby * aby) + abz * abz;
    const double num = (apx * abx + apy * aby) + apz * abz;
    double t = den > 0.0 ? num / den : 0.0;
    t = fmin(fmax(t, 0.0), 1.0);
    qx = ax + t * abx; qy = ay + t * aby; qz = az + t * abz;
    ex = qx - px; ey = qy - py; ez = qz - pz;
    const double d = sqrt((ex * ex + ey * ey) + ez * ez);
    dist[vi * B + j] = d;
    alive = isfinite(d);
    if (alive) {
      lox = fmin(px, qx); loy = fmin(py, qy); loz = fmin(pz, qz);
      hix = fmax(px, qx); hiy = fmax(py, qy); hiz = fmax(pz, qz);
      atomicMin(&ubox[0], cell_of(lox, g.x0, g.cell, g.gx));
      atomicMin(&ubox[1], cell_of(loy, g.y0, g.cell, g.gy));
      atomicMin(&ubox[2], cell_of(loz, g.z0, g.cell, g.gz));
      atomicMax(&ubox[3], cell_of(hix, g.x0, g.cell, g.gx));
      atomicMax(&ubox[4], cell_of(hiy, g.y0, g.cell, g.gy));
      atomicMax(&ubox[5], cell_of(hiz, g.z0, g.cell, g.gz));
    }
  }
  __syncthreads();
  const int cx0 = ubox[0], cy0 = ubox[1], cz0 = ubox[2], cx1 = ubox[3], cy1 = ubox[4], cz1 = ubox[5];
  const bool valid = alive;
  bool done = false;                     // uniform: every segment of the workgroup is blocked

  for (int cz = cz0; cz <= cz1 && !done; ++cz)
    for (int cy = cy0; cy <= cy1 && !done; ++cy) {
      const int row = (cz * g.gy + cy) * g.gx;
      const int64_t beg = max((int64_t)offsets[row + cx0], (int64_t)0);
      const int64_t end = min((int64_t)offsets[row + cx1 + 1], n_items);
      for (int64_t base = beg; base < end; base += VIS_CHUNK) {
        // the previous chunk is consumed; stop when nobody is left
        if (!__syncthreads_or(alive ? 1 : 0)) { done = true; break; }
        const int64_t k = base + tid;
        int ia = -1, ib = -1, ic = -1;
        if (k < end) {
          const int m = items[k];
          if (m >= 0 && m < M && face_indices(faces, m, V, ia, ib, ic)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              tc[a][tid] = verts[(int64_t)ia * 3 + a];
              tc[3 + a][tid] = verts[(int64_t)ib * 3 + a];
              tc[6 + a][tid] = verts[(int64_t)ic * 3 + a];
            }
          } else {
            ia = -1;
          }
        }
        ti[0][tid] = ia; ti[1][tid] = ib; ti[2][tid] = ic;
        __syncthreads();
        if (alive) {
          const int n = (int)min((int64_t)VIS_CHUNK, end - base);
          for (int s = 0; s < n; ++s) {
            const int a0 = ti[0][s];
            if (a0 < 0 || a0 == vi || ti[1][s] == vi || ti[2][s] == vi) continue;
            const double ux = tc[0][s], uy = tc[1][s], uz = tc[2][s];
            const double vx = tc[3][s], vy = tc[4][s], vz = tc[5][s];
            const double wx = tc[6][s], wy = tc[7][s], wz = tc[8][s];
            // boxes apart: no point in common, the volumes below cannot say otherwise
            if (fmax(fmax(ux, vx), wx) < lox || fmin(fmin(ux, vx), wx) > hix ||
                fmax(fmax(uy, vy), wy) < loy || fmin(fmin(uy, vy), wy) > hiy ||
                fmax(fmax(uz, vz), wz) < loz || fmin(fmin(uz, vz), wz) > hiz)
              continue;
            const double Ax = ux - px, Ay = uy - py, Az = uz - pz;
            const double Bx = vx - px, By = vy - py, Bz = vz - pz;
            const double Cx = wx - px, Cy = wy - py, Cz = wz - pz;
            const double s1 = triple(Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz);
            const double s2 = triple(ux - qx, uy - qy, uz - qz, vx - qx, vy - qy, vz - qz, wx - qx,
                                     wy - qy, wz - qz);
            if (!((s1 > 0.0 && s2 < 0.0) || (s1 < 0.0 && s2 > 0.0))) continue;
            const double t1 = triple(ex, ey, ez, Ax, Ay, Az, Bx, By, Bz);
            const double t2 = triple(ex, ey, ez, Bx, By, Bz, Cx, Cy, Cz);
            const double t3 = triple(ex, ey, ez, Cx, Cy, Cz, Ax, Ay, Az);
            if ((t1 >= 0.0 && t2 >= 0.0 && t3 >= 0.0) || (t1 <= 0.0 && t2 <= 0.0 && t3 <= 0.0)) {
              alive = false;
              break;
            }
          }
        }
      }
    }
  if (vi >= 0) visible[vi * B + j] = (valid && alive) ? 1 : 0;
}

// ------------------------------------------------------------------ block conjugate gradients
// Layout of every launch: n_rhs = B columns, G = 256 / B row groups per workgroup, RB rows per
// workgroup (a multiple of G), NB = ceil(n / RB) <= 256 workgroups.  Thread t < G B owns column
// t % B of the rows blk RB + t / B, + G, ...: element (row, column) is visited by the same thread
// in the same order in every kernel and every run, and per-workgroup partial sums are added in
// workgroup order (dsu_red::column_sum), so two runs give the same bits.
struct CgPlan {
  int64_t n;
  int32_t B, G, RB, NB;
};

struct CgBuf {
  double *r, *p, *q, *minv, *pq, *rz0, *rz1, *rr, *bb, *bnorm, *res;
  int32_t* flag;
};

__device__ __forceinline__ double sq_or_one(double s) { return s > 0.0 ? sqrt(s) : 1.0; }

#define CG_THREAD_ROWS()                                                          \
  const int tid = threadIdx.x, blk = blockIdx.x;                                  \
  const bool act = tid < pl.G * pl.B;                                             \
  const int c = act ? tid % pl.B : 0, gq = tid / pl.B;                            \
  const int64_t r_end = min((int64_t)(blk + 1) * pl.RB, pl.n);                    \
  const int64_t r_beg = act ? (int64_t)blk * pl.RB + gq : r_end

__device__ __forceinline__ double csr_row_dot(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                              const double* __restrict__ vals, int64_t nnz, int64_t n,
                                              int64_t row, const double* __restrict__ x, int B, int c,
                                              double* diag) {
  double s = 0.0, d = 0.0;
  const int64_t k0 = max((int64_t)rowptr[row], (int64_t)0), k1 = min((int64_t)rowptr[row + 1], nnz);
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t jn = cols[k];
    if (jn < 0 || jn >= n) continue;
    const double a = vals[k];
    if (jn == row) d += a;
    s += a * x[jn * B + c];
  }
  if (diag) *diag = d;
  return s;
}

// r = b - A x, p = z = r / diag, partials of r.z (parity 0), r.r and b.b
__global__ __launch_bounds__(256) void cg_init_kernel(const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ cols,
                                                      const double* __restrict__ vals, int64_t nnz,
                                                      const double* __restrict__ rhs,
                                                      const double* __restrict__ x, CgPlan pl, CgBuf w) {
  __shared__ double red[256];
  CG_THREAD_ROWS();
  double a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int64_t row = r_beg; row < r_end; row += pl.G) {
    double d;
    const double ax = csr_row_dot(rowptr, cols, vals, nnz, pl.n, row, x, pl.B, c, &d);
    const double mi = d > 0.0 ? 1.0 / d : 1.0;
    if (c == 0) w.minv[row] = mi;
    const int64_t e = row * pl.B + c;
    const double b = rhs[e], r0 = b - ax, z = mi * r0;
    w.r[e] = r0;
    w.p[e] = z;
    a1 += r0 * z; a2 += r0 * r0; a3 += b * b;
  }
  dsu_red::block_column_partials(a1, red, pl.B, pl.G, w.rz0 + (int64_t)blk * pl.B);
  dsu_red::block_column_partials(a2, red, pl.B, pl.G, w.rr + (int64_t)blk * pl.B);
  dsu_red::block_column_partials(a3, red, pl.B, pl.G, w.bb + (int64_t)blk * pl.B);
}

// one workgroup: |b| per column, the starting residuals and the flag
__global__ __launch_bounds__(256) void cg_norms_kernel(CgPlan pl, CgBuf w, double tol) {
  __shared__ int32_t bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int c = threadIdx.x; c < pl.B; c += blockDim.x) {
    const double bn = sq_or_one(dsu_red::column_sum(w.bb, pl.NB, pl.B, c));
    w.bnorm[c] = bn;
    const double res = sqrt(dsu_red::column_sum(w.rr, pl.NB, pl.B, c)) / bn;
    w.res[c] = res;
    if (!(res <= tol)) atomicOr(&bad, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) w.flag[0] = bad ? 0 : 1;
}

// q = A p, partials of p.q
__global__ __launch_bounds__(256) void cg_spmv_kernel(const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ cols,
                                                      const double* __restrict__ vals, int64_t nnz, CgPlan pl,
                                                      CgBuf w) {
  __shared__ double red[256];
  CG_THREAD_ROWS();
  double acc = 0.0;
  for (int64_t row = r_beg; row < r_end; row += pl.G) {
    const double s = csr_row_dot(rowptr, cols, vals, nnz, pl.n, row, w.p, pl.B, c, nullptr);
    const int64_t e = row * pl.B + c;
    w.q[e] = s;
    acc += w.p[e] * s;
  }
  dsu_red::block_column_partials(acc, red, pl.B, pl.G, w.pq + (int64_t)blk * pl.B);
}

// alpha = r.z / p.q;  x += alpha p;  r -= alpha q;  partials of the new r.z and r.r
__global__ __launch_bounds__(256) void cg_update_kernel(double* __restrict__ x, CgPlan pl, CgBuf w,
                                                        const double* __restrict__ rz_old,
                                                        double* __restrict__ rz_new) {
  __shared__ double red[256];
  __shared__ double alpha_s[256];
  CG_THREAD_ROWS();
  if (tid < pl.B) {
    const double pq = dsu_red::column_sum(w.pq, pl.NB, pl.B, tid);
    const double rz = dsu_red::column_sum(rz_old, pl.NB, pl.B, tid);
    alpha_s[tid] = pq > 0.0 ? rz / pq : 0.0;
  }
  __syncthreads();
  const double alpha = alpha_s[c];
  double a1 = 0.0, a2 = 0.0;
  for (int64_t row = r_beg; row < r_end; row += pl.G) {
    const int64_t e = row * pl.B + c;
    x[e] = x[e] + alpha * w.p[e];
    const double rn = w.r[e] - alpha * w.q[e];
    w.r[e] = rn;
    const double z = w.minv[row] * rn;
    a1 += rn * z; a2 += rn * rn;
  }
  dsu_red::block_column_partials(a1, red, pl.B, pl.G, rz_new + (int64_t)blk * pl.B);
  dsu_red::block_column_partials(a2, red, pl.B, pl.G, w.rr + (int64_t)blk * pl.B);
}

// beta = r.z new / r.z old;  p = z + beta p;  workgroup 0 also writes the residuals and the flag
__global__ __launch_bounds__(256) void cg_direction_kernel(CgPlan pl, CgBuf w, const double* __restrict__ rz_old,
                                                           const double* __restrict__ rz_new, double tol) {
  __shared__ double beta_s[256];
  __shared__ int32_t bad;
  CG_THREAD_ROWS();
  if (tid == 0) bad = 0;
  __syncthreads();
  if (tid < pl.B) {
    const double rn = dsu_red::column_sum(rz_new, pl.NB, pl.B, tid);
    const double ro = dsu_red::column_sum(rz_old, pl.NB, pl.B, tid);
    beta_s[tid] = ro > 0.0 ? rn / ro : 0.0;
    if (blk == 0) {
      const double res = sqrt(dsu_red::column_sum(w.rr, pl.NB, pl.B, tid)) / w.bnorm[tid];
      w.res[tid] = res;
      if (!(res <= tol)) atomicOr(&bad, 1);
    }
  }
  __syncthreads();
  if (blk == 0 && tid == 0) w.flag[0] = bad ? 0 : 1;
  const double beta = beta_s[c];
  for (int64_t row = r_beg; row < r_end; row += pl.G) {
    const int64_t e = row * pl.B + c;
    w.p[e] = w.minv[row] * w.r[e] + beta * w.p[e];
  }
}

bool cg_plan(int64_t n, int32_t B, CgPlan& pl) {
  if (n < 1 || n > (int64_t)1 << 26 || B < 1 || B > 256 || n * B > (int64_t)1 << 31) return false;
  pl.n = n;
  pl.B = B;
  pl.G = 256 / B;
  int64_t rb = (n + 255) / 256;
  rb = (rb + pl.G - 1) / pl.G * pl.G;
  pl.RB = (int32_t)rb;
  pl.NB = (int32_t)((n + rb - 1) / rb);
  return true;
}

// doubles of the workspace: r, p, q (n B each), 1 / diag (n), five partial tables (NB B), |b| and
// the residuals (B); then the flag
int64_t cg_doubles(const CgPlan& pl) {
  return 3 * pl.n * pl.B + pl.n + 5 * (int64_t)pl.NB * pl.B + 2 * (int64_t)pl.B;
}

// ------------------------------------------------------------------ linear-blend skinning
__global__ __launch_bounds__(256) void skin_lbs_kernel(const float* __restrict__ rest,
                                                       const int32_t* __restrict__ infl,
                                                       const float* __restrict__ wts,
                                                       const float* __restrict__ mats, int64_t V, int32_t K,
                                                       int32_t F, int32_t J, float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)F * V) return;
  const int64_t f = i / V, v = i - f * V;
  const float x = rest[v * 3], y = rest[v * 3 + 1], z = rest[v * 3 + 2];
  float ox = 0.0f, oy = 0.0f, oz = 0.0f;
  for (int k = 0; k < K; ++k) {
    const int jn = infl[v * K + k];
    if (jn < 0 || jn >= J) continue;
    const float w = wts[v * K + k];
    const float* __restrict__ m = mats + (f * J + jn) * 12;
    ox = ox + w * (((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
    oy = oy + w * (((m[4] * x + m[5] * y) + m[6] * z) + m[7]);
    oz = oz + w * (((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
  }
  out[i * 3] = ox;
  out[i * 3 + 1] = oy;
  out[i * 3 + 2] = oz;
}

// ------------------------------------------------------------------ dual-quaternion skinning
// One thread per (frame, vertex), vertex fastest: the 12 B stores of a wave are contiguous, a wave's
// influences and weights are contiguous rows, and the frame's table (J * 64 B) is shared by every
// thread of the frame and stays in L2.
__global__ __launch_bounds__(256) void skin_dqs_kernel(const float* __restrict__ rest,
                                                       const int32_t* __restrict__ infl,
                                                       const float* __restrict__ wts,
                                                       const double* __restrict__ dq, int64_t V, int32_t K,
                                                       int32_t F, int32_t J, float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)F * V) return;
  const int64_t f = i / V, v = i - f * V;
  float o[3];
  dsu_dqs::blend(infl + v * K, wts + v * K, K, dq + f * J * 8, J, rest[v * 3], rest[v * 3 + 1], rest[v * 3 + 2], o);
  out[i * 3] = o[0];
  out[i * 3 + 1] = o[1];
  out[i * 3 + 2] = o[2];
}

// ------------------------------------------------------------------ centre-of-rotation skinning
// Centres, once per character (V * T pairs).  cor_rows_kernel writes every triangle's canonical row
// (its ascending (joint, w^) pairs, centroid and area) once.  cor_centres_kernel: one thread per
// vertex with its <= COR_KR pairs in registers; the rows stream through LDS DSU_COR_TILE triangles
// at a time and every lane reads the same triangle (a broadcast).  A (vertex, triangle) pair looks
// the vertex's joints up in the triangle's row and leaves before any exponential when fewer than two
// are shared.  V / 256 workgroups do not fill the device, so blockIdx.y splits the triangle range
// into runs of whole tiles; cor_reduce_kernel adds the partial sums in ascending order: no atomics,
// two runs give the same bits.  K above COR_KR: cor_centres_wide_kernel, the same sums with both
// rows read from memory.
constexpr int COR_TILE = DSU_COR_TILE;
constexpr int COR_KR = 4;
constexpr int COR_RW = 3 * COR_KR;

struct CorRows {
  int32_t* n;      // (T) pairs of the row, 0: skipped
  int32_t* j;      // (T, rw)
  double* w;       // (T, rw)
  double* geo;     // (T, 4) centroid, area
  int32_t rw;
};

struct CorPlan {
  int32_t rw, parts;
  int64_t tiles_per_part;
};

bool cor_shape_ok(int64_t V, int64_t T, int32_t K, int32_t J, double sigma) {
  return V >= 0 && V <= (int64_t)1 << 26 && T >= 0 && T <= (int64_t)1 << 28 && K >= 1 && K <= 4096 && J >= 1 &&
         V * K <= (int64_t)1 << 31 && sigma > 0.0 && sigma * sigma > 0.0 &&
         sigma * sigma <= 1.7976931348623157e308;
}

CorPlan cor_plan(int64_t V, int64_t T, int32_t K, int32_t J) {
  CorPlan pl;
  pl.rw = (int32_t)min((int64_t)3 * K, (int64_t)J);
  const int64_t nbx = max((V + 255) / 256, (int64_t)1);
  pl.parts = (int32_t)min((int64_t)DSU_COR_MAX_PARTS, (1024 + nbx - 1) / nbx);
  const int64_t tiles = (T + COR_TILE - 1) / COR_TILE;
  pl.tiles_per_part = max((tiles + pl.parts - 1) / pl.parts, (int64_t)1);
  return pl;
}

// doubles first (partials, geo, w), then the int32 arrays; rounded up to whole doubles
int64_t cor_bytes(const CorPlan& pl, int64_t V, int64_t T) {
  const int64_t ints = T + T * pl.rw;
  return ((int64_t)pl.parts * V * 4 + T * 4 + T * pl.rw + (ints + 1) / 2) * 8;
}

__global__ __launch_bounds__(256) void cor_rows_kernel(const float* __restrict__ rest,
                                                       const int32_t* __restrict__ faces,
                                                       const int32_t* __restrict__ joints,
                                                       const float* __restrict__ weights, int64_t V, int64_t T,
                                                       int32_t K, int32_t J, CorRows r) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= T) return;
  double geo[4];
  r.n[t] = dsu_cor::triangle_row(rest, faces, t, V, joints, weights, K, J, r.rw, r.j + t * r.rw, r.w + t * r.rw, geo);
  r.geo[t * 4] = geo[0]; r.geo[t * 4 + 1] = geo[1]; r.geo[t * 4 + 2] = geo[2]; r.geo[t * 4 + 3] = geo[3];
}

__global__ __launch_bounds__(256) void cor_centres_kernel(const int32_t* __restrict__ joints,
                                                          const float* __restrict__ weights, int64_t V, int32_t K,
                                                          int32_t J, CorRows r, int64_t T, int64_t tiles_per_part,
                                                          double s2, double* __restrict__ partial) {
  __shared__ double s_geo[COR_TILE * 4];
  __shared__ double s_w[COR_TILE * COR_RW];
  __shared__ int32_t s_j[COR_TILE * COR_RW];
  __shared__ int32_t s_n[COR_TILE];
  const int tid = threadIdx.x;
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + tid;
  const int rw = r.rw;                       // <= COR_RW here
  int32_t vj[COR_KR];
  double vw[COR_KR];
  int nv = 0;
#pragma unroll
  for (int a = 0; a < COR_KR; ++a) { vj[a] = -1; vw[a] = 0.0; }
  if (v < V) {
    nv = dsu_cor::row_length(joints + v * K, K, J);
#pragma unroll
    for (int a = 0; a < COR_KR; ++a)
      if (a < nv) { vj[a] = joints[v * K + a]; vw[a] = (double)weights[v * K + a]; }
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int64_t t_beg = min((int64_t)blockIdx.y * tiles_per_part * COR_TILE, T);
  const int64_t t_end = min(((int64_t)blockIdx.y + 1) * tiles_per_part * COR_TILE, T);
  for (int64_t base = t_beg; base < t_end; base += COR_TILE) {
    const int nt = (int)min((int64_t)COR_TILE, t_end - base);
    __syncthreads();                         // the previous tile is consumed
    if (tid < nt * 4) s_geo[tid] = r.geo[base * 4 + tid];
    if (tid < nt) s_n[tid] = r.n[base + tid];
    for (int i = tid; i < nt * rw; i += 256) {
      s_w[i] = r.w[base * rw + i];
      s_j[i] = r.j[base * rw + i];
    }
    __syncthreads();
    if (nv < 2) continue;
    for (int s = 0; s < nt; ++s) {
      const int n = s_n[s];
      if (n < 2) continue;
      double th[COR_KR];
#pragma unroll
      for (int a = 0; a < COR_KR; ++a) th[a] = 0.0;
      int shared = 0;
      for (int e = 0; e < n; ++e) {
        const int32_t je = s_j[s * rw + e];
        const double we = s_w[s * rw + e];
#pragma unroll
        for (int a = 0; a < COR_KR; ++a)
          if (je == vj[a] && we != 0.0 && vw[a] != 0.0) { th[a] = we; ++shared; }
      }
      if (shared < 2) continue;
      double sim = 0.0;
#pragma unroll
      for (int a = 0; a < COR_KR; ++a)
#pragma unroll
        for (int b = a + 1; b < COR_KR; ++b)
          if (th[a] != 0.0 && th[b] != 0.0) sim = sim + dsu_cor::pair_term(vw[a], vw[b], th[a], th[b], s2);
      if (sim != 0.0) dsu_cor::add_triangle(acc, sim, s_geo + s * 4);
    }
  }
  if (v < V) {
    double* __restrict__ o = partial + ((int64_t)blockIdx.y * V + v) * 4;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
  }
}

__global__ __launch_bounds__(256) void cor_centres_wide_kernel(const int32_t* __restrict__ joints,
                                                               const float* __restrict__ weights, int64_t V,
                                                               int32_t K, int32_t J, CorRows r, int64_t T,
                                                               int64_t tiles_per_part, double s2,
                                                               double* __restrict__ partial) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int32_t* __restrict__ vj = joints + v * K;
  const float* __restrict__ vw = weights + v * K;
  const int nv = dsu_cor::row_length(vj, K, J);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int64_t t_beg = min((int64_t)blockIdx.y * tiles_per_part * COR_TILE, T);
  const int64_t t_end = min(((int64_t)blockIdx.y + 1) * tiles_per_part * COR_TILE, T);
  if (nv >= 2)
    for (int64_t t = t_beg; t < t_end; ++t) {
      const int n = r.n[t];
      if (n < 2) continue;
      const double sim = dsu_cor::similarity(vj, vw, nv, r.j + t * r.rw, r.w + t * r.rw, n, s2);
      if (sim != 0.0) dsu_cor::add_triangle(acc, sim, r.geo + t * 4);
    }
  double* __restrict__ o = partial + ((int64_t)blockIdx.y * V + v) * 4;
  o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
}

__global__ __launch_bounds__(256) void cor_reduce_kernel(const double* __restrict__ partial, int64_t V, int32_t parts,
                                                         double* __restrict__ centres, uint8_t* __restrict__ valid) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v >= V) return;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < parts; ++p) {
    const double* __restrict__ q = partial + ((int64_t)p * V + v) * 4;
    acc[0] = acc[0] + q[0]; acc[1] = acc[1] + q[1]; acc[2] = acc[2] + q[2]; acc[3] = acc[3] + q[3];
  }
  dsu_cor::finish(acc, centres + v * 3, valid + v);
}

// Apply: skin_dqs_kernel's shape, one thread per (frame, vertex), vertex fastest; the frame's tables
// (J * 128 B) are shared by every thread of the frame.
__global__ __launch_bounds__(256) void skin_cor_kernel(const float* __restrict__ rest,
                                                       const int32_t* __restrict__ infl,
                                                       const float* __restrict__ wts,
                                                       const double* __restrict__ mats,
                                                       const double* __restrict__ quats,
                                                       const double* __restrict__ centres,
                                                       const uint8_t* __restrict__ valid, int64_t V, int32_t K,
                                                       int32_t F, int32_t J, float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)F * V) return;
  const int64_t f = i / V, v = i - f * V;
  float o[3];
  dsu_cor::blend(infl + v * K, wts + v * K, K, mats + f * J * 12, quats + f * J * 4, J, rest[v * 3], rest[v * 3 + 1],
                 rest[v * 3 + 2], centres + v * 3, valid[v], o);
  out[i * 3] = o[0];
  out[i * 3 + 1] = o[1];
  out[i * 3 + 2] = o[2];
}

bool skin_shape_ok(int64_t n_verts, int32_t K, int32_t n_frames, int32_t n_joints) {
  return !(n_verts < 0 || K < 1 || K > 4096 || n_frames < 1 || n_frames > 65535 || n_joints < 1 ||
           (int64_t)n_frames * n_verts > (int64_t)1 << 31 || n_verts * K > (int64_t)1 << 31);
}

bool grid_ok(int32_t gx, int32_t gy, int32_t gz) {
  return gx >= 1 && gy >= 1 && gz >= 1 && gx <= 256 && gy <= 256 && gz <= 256 &&
         (int64_t)gx * gy * gz <= (int64_t)1 << 22;
}

}  // namespace

extern "C" {

int64_t dsu_bone_visibility_workspace_bytes(int32_t gx, int32_t gy, int32_t gz) {
  if (!grid_ok(gx, gy, gz)) return DSU_EINVAL;
  return dsu_bin::bytes((int64_t)gx * gy * gz);
}

int dsu_bone_visibility(int32_t stage, const float* verts, const int32_t* faces, const float* bones,
                        int64_t n_verts, int64_t n_faces, int32_t n_bones, const int32_t* order, double x0,
                        double y0, double z0, double cell, int32_t gx, int32_t gy, int32_t gz,
                        void* workspace, int64_t workspace_bytes, int32_t* items, int64_t n_items,
                        double* dist, uint8_t* visible, void* stream) {
  if (stage < DSU_SKIN_COUNT || stage > DSU_SKIN_RUN || !grid_ok(gx, gy, gz)) return DSU_EINVAL;
  if (!(cell > 0.0) || !(cell < 1e30) || !(x0 == x0) || !(y0 == y0) || !(z0 == z0)) return DSU_EINVAL;
  if (n_verts < 1 || n_verts > (int64_t)1 << 30 || n_faces < 0 || n_faces > (int64_t)1 << 30 || n_items < 0 ||
      n_bones < 1 || n_bones > 65535 || n_verts * n_bones > (int64_t)1 << 31)
    return DSU_EINVAL;
  const int64_t nc = (int64_t)gx * gy * gz;
  if (!workspace || workspace_bytes < dsu_bin::bytes(nc)) return DSU_EINVAL;
  if (!verts || (n_faces && !faces)) return DSU_EINVAL;
  if (stage != DSU_SKIN_COUNT && n_items && !items) return DSU_EINVAL;
  if (stage == DSU_SKIN_RUN && (!bones || !dist || !visible)) return DSU_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const SkinGrid g{x0, y0, z0, cell, gx, gy, gz};
  if (stage != DSU_SKIN_RUN)
    return dsu_bin::run_stage(stage, TriangleCells3{verts, faces, n_verts, g}, n_faces, workspace, nc, items,
                              n_items, st);
  const int32_t* offsets = dsu_bin::split(workspace, nc).offsets;
  bone_visibility_kernel<<<dim3((unsigned)dsu_blocks_for(n_verts, 256), (unsigned)n_bones), dim3(256), 0, st>>>(
      verts, faces, bones, n_verts, n_faces, n_bones, order, g, offsets, items, n_faces ? n_items : 0, dist,
      visible);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int64_t dsu_spd_cg_block_workspace_bytes(int64_t n, int32_t n_rhs) {
  CgPlan pl;
  if (!cg_plan(n, n_rhs, pl)) return DSU_EINVAL;
  return cg_doubles(pl) * (int64_t)sizeof(double) + 8;
}

int dsu_spd_cg_block(const int32_t* rowptr, const int32_t* cols, const double* vals, int64_t n, int64_t nnz,
                     int32_t n_rhs, const double* rhs, double* x, double tol, int32_t max_iters,
                     void* workspace, int64_t workspace_bytes, int32_t* out_iters, double* out_residuals,
                     void* stream) {
  CgPlan pl;
  if (!cg_plan(n, n_rhs, pl) || nnz < 0 || nnz > (int64_t)1 << 31 || max_iters < 0 || !(tol >= 0.0))
    return DSU_EINVAL;
  if (!rowptr || (nnz && (!cols || !vals)) || !rhs || !x || !workspace) return DSU_EINVAL;
  if (workspace_bytes < cg_doubles(pl) * (int64_t)sizeof(double) + 8) return DSU_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = pl.n * pl.B, pb = (int64_t)pl.NB * pl.B;
  double* d = (double*)workspace;
  CgBuf w;
  w.r = d; w.p = d + nb; w.q = d + 2 * nb; w.minv = d + 3 * nb;
  double* t = w.minv + pl.n;
  w.pq = t; w.rz0 = t + pb; w.rz1 = t + 2 * pb; w.rr = t + 3 * pb; w.bb = t + 4 * pb;
  w.bnorm = t + 5 * pb; w.res = w.bnorm + pl.B;
  w.flag = (int32_t*)(w.res + pl.B);
  cg_init_kernel<<<pl.NB, 256, 0, st>>>(rowptr, cols, vals, nnz, rhs, x, pl, w);
  cg_norms_kernel<<<1, 256, 0, st>>>(pl, w, tol);
  DSU_CHECK_LAUNCH();
  int32_t flag = 0, it = 0;
  if (hipMemcpyAsync(&flag, w.flag, sizeof(flag), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return DSU_ELAUNCH;
  while (!flag && it < max_iters) {
    ++it;
    const double* rz_old = (it & 1) ? w.rz0 : w.rz1;
    double* rz_new = (it & 1) ? w.rz1 : w.rz0;
    cg_spmv_kernel<<<pl.NB, 256, 0, st>>>(rowptr, cols, vals, nnz, pl, w);
    cg_update_kernel<<<pl.NB, 256, 0, st>>>(x, pl, w, rz_old, rz_new);
    cg_direction_kernel<<<pl.NB, 256, 0, st>>>(pl, w, rz_old, rz_new, tol);
    DSU_CHECK_LAUNCH();
    if (hipMemcpyAsync(&flag, w.flag, sizeof(flag), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return DSU_ELAUNCH;
  }
  if (out_iters) *out_iters = it;
  if (out_residuals &&
      (hipMemcpyAsync(out_residuals, w.res, pl.B * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipStreamSynchronize(st) != hipSuccess))
    return DSU_ELAUNCH;
  return DSU_OK;
}

int dsu_skin_lbs(const float* rest, const int32_t* influences, const float* weights, const float* matrices,
                 int64_t n_verts, int32_t K, int32_t n_frames, int32_t n_joints, float* out, void* stream) {
  if (n_verts < 0 || K < 1 || K > 4096 || n_frames < 1 || n_frames > 65535 || n_joints < 1 ||
      (int64_t)n_frames * n_verts > (int64_t)1 << 31 || n_verts * K > (int64_t)1 << 31)
    return DSU_EINVAL;
  if (n_verts == 0) return DSU_OK;
  if (!rest || !influences || !weights || !matrices || !out) return DSU_EINVAL;
  const int64_t total = (int64_t)n_frames * n_verts;
  skin_lbs_kernel<<<dsu_blocks_for(total, 256), 256, 0, (hipStream_t)stream>>>(
      rest, influences, weights, matrices, n_verts, K, n_frames, n_joints, out);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_skin_dqs(const float* rest, const int32_t* influences, const float* weights, const double* dualquats,
                 int64_t n_verts, int32_t K, int32_t n_frames, int32_t n_joints, float* out, void* stream) {
  if (!skin_shape_ok(n_verts, K, n_frames, n_joints)) return DSU_EINVAL;
  if (n_verts == 0) return DSU_OK;
  if (!rest || !influences || !weights || !dualquats || !out) return DSU_EINVAL;
  const int64_t total = (int64_t)n_frames * n_verts;
  skin_dqs_kernel<<<dsu_blocks_for(total, 256), 256, 0, (hipStream_t)stream>>>(
      rest, influences, weights, dualquats, n_verts, K, n_frames, n_joints, out);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

// HOST: the same blend (dqs_blend.h) on host arrays.
int dsu_skin_dqs_host(const float* rest, const int32_t* influences, const float* weights,
                      const double* dualquats, int64_t n_verts, int32_t K, int32_t n_frames, int32_t n_joints,
                      float* out) {
  if (!skin_shape_ok(n_verts, K, n_frames, n_joints)) return DSU_EINVAL;
  if (n_verts == 0) return DSU_OK;
  if (!rest || !influences || !weights || !dualquats || !out) return DSU_EINVAL;
  for (int64_t f = 0; f < n_frames; ++f)
    for (int64_t v = 0; v < n_verts; ++v)
      dsu_dqs::blend(influences + v * K, weights + v * K, K, dualquats + f * n_joints * 8, n_joints, rest[v * 3],
                     rest[v * 3 + 1], rest[v * 3 + 2], out + (f * n_verts + v) * 3);
  return DSU_OK;
}

int64_t dsu_skin_cor_centres_workspace_bytes(int64_t n_verts, int64_t n_faces, int32_t K, int32_t n_joints) {
  if (!cor_shape_ok(n_verts, n_faces, K, n_joints, 1.0)) return DSU_EINVAL;
  return cor_bytes(cor_plan(n_verts, n_faces, K, n_joints), n_verts, n_faces);
}

int dsu_skin_cor_centres(const float* rest, const int32_t* faces, const int32_t* joints, const float* weights,
                         int64_t n_verts, int64_t n_faces, int32_t K, int32_t n_joints, double sigma,
                         void* workspace, int64_t workspace_bytes, double* centres, uint8_t* valid, void* stream) {
  if (!cor_shape_ok(n_verts, n_faces, K, n_joints, sigma)) return DSU_EINVAL;
  if (n_verts == 0) return DSU_OK;
  const CorPlan pl = cor_plan(n_verts, n_faces, K, n_joints);
  if (!rest || (n_faces && !faces) || !joints || !weights || !centres || !valid || !workspace ||
      workspace_bytes < cor_bytes(pl, n_verts, n_faces))
    return DSU_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t V = n_verts, T = n_faces;
  double* partial = (double*)workspace;
  CorRows r;
  r.geo = partial + (int64_t)pl.parts * V * 4;
  r.w = r.geo + T * 4;
  r.n = (int32_t*)(r.w + T * pl.rw);
  r.j = r.n + T;
  r.rw = pl.rw;
  if (T) cor_rows_kernel<<<dsu_blocks_for(T, 256), 256, 0, st>>>(rest, faces, joints, weights, V, T, K, n_joints, r);
  const dim3 grid((unsigned)dsu_blocks_for(V, 256), (unsigned)pl.parts);
  if (K <= COR_KR)
    cor_centres_kernel<<<grid, dim3(256), 0, st>>>(joints, weights, V, K, n_joints, r, T, pl.tiles_per_part,
                                                   sigma * sigma, partial);
  else
    cor_centres_wide_kernel<<<grid, dim3(256), 0, st>>>(joints, weights, V, K, n_joints, r, T, pl.tiles_per_part,
                                                        sigma * sigma, partial);
  cor_reduce_kernel<<<dsu_blocks_for(V, 256), 256, 0, st>>>(partial, V, pl.parts, centres, valid);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

// HOST: the same text (cor_blend.h) on host arrays, the triangles in one ascending run.
int dsu_skin_cor_centres_host(const float* rest, const int32_t* faces, const int32_t* joints, const float* weights,
                              int64_t n_verts, int64_t n_faces, int32_t K, int32_t n_joints, double sigma,
                              double* centres, uint8_t* valid) {
  if (!cor_shape_ok(n_verts, n_faces, K, n_joints, sigma)) return DSU_EINVAL;
  if (n_verts == 0) return DSU_OK;
  if (!rest || (n_faces && !faces) || !joints || !weights || !centres || !valid) return DSU_EINVAL;
  const int64_t V = n_verts, T = n_faces;
  // the rows are host memory of this call: running out of it is an unsupported size, not an exception
  try {
    const int rw = cor_plan(V, T, K, n_joints).rw;
    std::vector<int32_t> tn(T), tj(T * rw);
    std::vector<double> tw(T * rw), geo(T * 4);
    for (int64_t t = 0; t < T; ++t)
      tn[t] = dsu_cor::triangle_row(rest, faces, t, V, joints, weights, K, n_joints, rw, tj.data() + t * rw,
                                    tw.data() + t * rw, geo.data() + t * 4);
    const double s2 = sigma * sigma;
    for (int64_t v = 0; v < V; ++v) {
      const int nv = dsu_cor::row_length(joints + v * K, K, n_joints);
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      if (nv >= 2)
        for (int64_t t = 0; t < T; ++t) {
          if (tn[t] < 2) continue;
          const double sim = dsu_cor::similarity(joints + v * K, weights + v * K, nv, tj.data() + t * rw,
                                                 tw.data() + t * rw, tn[t], s2);
          if (sim != 0.0) dsu_cor::add_triangle(acc, sim, geo.data() + t * 4);
        }
      dsu_cor::finish(acc, centres + v * 3, valid + v);
    }
  } catch (const std::bad_alloc&) {
    return DSU_EINVAL;
  }
  return DSU_OK;
}

int dsu_skin_cor(const float* rest, const int32_t* influences, const float* weights, const double* matrices,
                 const double* quats, const double* centres, const uint8_t* valid, int64_t n_verts, int32_t K,
                 int32_t n_frames, int32_t n_joints, float* out, void* stream) {
  if (!skin_shape_ok(n_verts, K, n_frames, n_joints)) return DSU_EINVAL;
  if (n_verts == 0) return DSU_OK;
  if (!rest || !influences || !weights || !matrices || !quats || !centres || !valid || !out) return DSU_EINVAL;
  const int64_t total = (int64_t)n_frames * n_verts;
  skin_cor_kernel<<<dsu_blocks_for(total, 256), 256, 0, (hipStream_t)stream>>>(
      rest, influences, weights, matrices, quats, centres, valid, n_verts, K, n_frames, n_joints, out);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

// HOST: the same blend (cor_blend.h) on host arrays.
int dsu_skin_cor_host(const float* rest, const int32_t* influences, const float* weights, const double* matrices,
                      const double* quats, const double* centres, const uint8_t* valid, int64_t n_verts, int32_t K,
                      int32_t n_frames, int32_t n_joints, float* out) {
  if (!skin_shape_ok(n_verts, K, n_frames, n_joints)) return DSU_EINVAL;
  if (n_verts == 0) return DSU_OK;
  if (!rest || !influences || !weights || !matrices || !quats || !centres || !valid || !out) return DSU_EINVAL;
  for (int64_t f = 0; f < n_frames; ++f)
    for (int64_t v = 0; v < n_verts; ++v)
      dsu_cor::blend(influences + v * K, weights + v * K, K, matrices + f * n_joints * 12, quats + f * n_joints * 4,
                     n_joints, rest[v * 3], rest[v * 3 + 1], rest[v * 3 + 2], centres + v * 3, valid[v],
                     out + (f * n_verts + v) * 3);
  return DSU_OK;
}

}  // extern "C"
