// Thickness map of a mesh along z on a lattice of xy samples (gfx950): per sample the middle and
// the thickness of the thickest inside interval and the number of crossings.  What
// drawingspinup_amd/animate/rig.py lifts 2-D joint marks into the mesh with; an extension of the
// reference, which gets its skeleton already fitted from Mixamo.
//
//   dsu_mesh_thickness_ortho        the kernel, over the triangle grid of dsu_zgrid_count / _fill
//   dsu_mesh_thickness_ortho_host   the same text on host arrays
//
// The rule is stated in include/dsu_hip.h, its text is csrc/mesh_thickness.h (compiled here for
// both), tests/mesh_thickness_ref.py restates it in float64 numpy.
//
// One thread per sample, a workgroup of 256 = 16 x 16 samples (a wave is 4 rows of 16: its stores
// are four 128 B runs).  The workgroup walks the triangle lists of the grid cells its samples fall
// in, usually one (ops.mesh_thickness sizes a cell as 16 x 16 samples), 256 triangles at a time
// through LDS: a thread gathers one triangle, every thread then reads each of them from LDS at one
// address (a broadcast, no bank conflict).  A thread keeps no list of its crossings, which would
// live in scratch: walk k finds the k-th pair of crossings in the order (z, face) as the two lowest
// ones above the pair before, and the first walk counts them, so that the workgroup walks as often
// as its deepest sample has pairs (1-3 on a character).  No cap, no atomics: two runs give the same
// bits, and so does the host entry.
#include <vector>

#include "common.h"
#include "mesh_geom.h"
#include "mesh_thickness.h"

namespace {

using dsu_mt::Key;
using dsu_mt::Pairs;
using dsu_mt::Tri;

constexpr int SIDE = 16;                 // samples per workgroup side
constexpr int THREADS = SIDE * SIDE;     // = triangles per LDS tile

struct Lattice {
  double x0, y0, h;
  int32_t W, H;
};

struct Mesh {
  const float* __restrict__ verts;
  const int32_t* __restrict__ faces;
  int64_t V, T;
};

// One walk of a sample over the lists of the workgroup's cells; every thread of the workgroup
// comes here, `want` or not.
template <bool FIRST>
__device__ __forceinline__ void walk(Tri* tile, const Mesh& m, const ZGrid& gr, const int32_t* __restrict__ offsets,
                                     const int32_t* __restrict__ items, int64_t n_items, int cx_lo, int cx_hi,
                                     int cy_lo, int cy_hi, bool want, int own, double sx, double sy, const Key& cur,
                                     Key& lo, Key& hi, int32_t& count) {
  const int tid = threadIdx.x;
  for (int cy = cy_lo; cy <= cy_hi; ++cy) {
    for (int cx = cx_lo; cx <= cx_hi; ++cx) {
      const int cell = cy * gr.g + cx;
      int64_t k0 = offsets[cell], k1 = offsets[cell + 1];
      if (k0 < 0) k0 = 0;
      if (k1 > n_items) k1 = n_items;
      const bool mine = want && cell == own;
      for (int64_t base = k0; base < k1; base += THREADS) {
        const int n = (int)(k1 - base < THREADS ? k1 - base : THREADS);
        __syncthreads();                                    // the tile before is read
        if (tid < n) tile[tid] = dsu_mt::load_tri(m.verts, m.V, m.faces, m.T, items[base + tid]);
        __syncthreads();
        if (mine)
          for (int j = 0; j < n; ++j) dsu_mt::visit<FIRST>(tile[j], sx, sy, cur, lo, hi, count);
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void mesh_thickness_kernel(Mesh m, ZGrid gr, const int32_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ items, int64_t n_items,
                                                                 Lattice lt, double* __restrict__ out_mid,
                                                                 double* __restrict__ out_thickness,
                                                                 int32_t* __restrict__ out_count) {
  __shared__ Tri tile[THREADS];
  const int tid = threadIdx.x;
  const int c_first = blockIdx.x * SIDE, r_first = blockIdx.y * SIDE;
  const int c = c_first + (tid & (SIDE - 1)), r = r_first + tid / SIDE;
  const bool live = c < lt.W && r < lt.H;
  const double sx = dsu_mt::sample_at(lt.x0, c, lt.h), sy = dsu_mt::sample_at(lt.y0, r, lt.h);
  // cell_of is monotone, so the cells of the corner samples bound every sample's, and a triangle
  // that covers a sample is listed in the sample's cell (its f32 box contains the f32 sample)
  const int c_last = min(c_first + SIDE, lt.W) - 1, r_last = min(r_first + SIDE, lt.H) - 1;
  const int cx_lo = cell_of((float)dsu_mt::sample_at(lt.x0, c_first, lt.h), gr.x0, gr.inv_cell, gr.g);
  const int cx_hi = cell_of((float)dsu_mt::sample_at(lt.x0, c_last, lt.h), gr.x0, gr.inv_cell, gr.g);
  const int cy_lo = cell_of((float)dsu_mt::sample_at(lt.y0, r_first, lt.h), gr.y0, gr.inv_cell, gr.g);
  const int cy_hi = cell_of((float)dsu_mt::sample_at(lt.y0, r_last, lt.h), gr.y0, gr.inv_cell, gr.g);
  const int own = cell_of((float)sy, gr.y0, gr.inv_cell, gr.g) * gr.g + cell_of((float)sx, gr.x0, gr.inv_cell, gr.g);

  Key cur{0.0, -1};
  Pairs p = dsu_mt::no_pairs();
  int32_t count = 0, paired = 0;
  bool want = live;
  {
    Key lo{0.0, -1}, hi{0.0, -1};
    walk<true>(tile, m, gr, offsets, items, n_items, cx_lo, cx_hi, cy_lo, cy_hi, want, own, sx, sy, cur, lo, hi, count);
    paired = count & ~1;
    want = want && paired > 0;
    if (want) {
      dsu_mt::take(p, lo.z);
      dsu_mt::take(p, hi.z);
      cur = hi;
    }
  }
  while (__syncthreads_or(want && p.taken < paired)) {
    want = want && p.taken < paired;
    Key lo{0.0, -1}, hi{0.0, -1};
    int32_t unused = 0;
    walk<false>(tile, m, gr, offsets, items, n_items, cx_lo, cx_hi, cy_lo, cy_hi, want, own, sx, sy, cur, lo, hi,
                unused);
    if (want) {
      if (hi.face < 0) {
        want = false;                                       // a list that names a face twice: stop here
      } else {
        dsu_mt::take(p, lo.z);
        dsu_mt::take(p, hi.z);
        cur = hi;
      }
    }
  }
  if (live) {
    const int64_t at = (int64_t)r * lt.W + c;
    out_mid[at] = p.mid;
    out_thickness[at] = p.thickness;
    out_count[at] = count;
  }
}

bool finite_d(double v) { return v - v == 0.0; }

bool args_ok(int64_t n_verts, int64_t n_faces, double x0, double y0, double h, int32_t W, int32_t H) {
  const int64_t lim = ((int64_t)1 << 31) - 1;
  return n_verts >= 0 && n_verts <= lim && n_faces >= 0 && n_faces <= lim && finite_d(x0) && finite_d(y0) &&
         finite_d(h) && h > 0.0 && W >= 0 && W <= DSU_THICKNESS_MAX_SIDE && H >= 0 && H <= DSU_THICKNESS_MAX_SIDE;
}

// HOST: the lattice's 16 x 16 tiles as bins, each triangle listed where its xy box may reach a
// sample (one sample of margin on every side for the division's rounding).
int tile_range(double lo, double hi, double v0, double h, int32_t n, int& t0, int& t1) {
  double a = floor((lo - v0) / h - 0.5) - 1.0, b = ceil((hi - v0) / h - 0.5) + 1.0;
  if (!(b >= 0.0) || !(a <= (double)(n - 1))) return 0;
  if (a < 0.0) a = 0.0;
  if (b > (double)(n - 1)) b = (double)(n - 1);
  t0 = (int)a / SIDE;
  t1 = (int)b / SIDE;
  return 1;
}

}  // namespace

extern "C" {

int dsu_mesh_thickness_ortho(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, float grid_x0,
                             float grid_y0, float grid_cell, int32_t g, const int32_t* offsets, const int32_t* items,
                             int64_t n_items, double x0, double y0, double h, int32_t W, int32_t H, double* mid,
                             double* thickness, int32_t* count, void* stream) {
  if (!args_ok(n_verts, n_faces, x0, y0, h, W, H) || g < 1 || g > 4096 || !(grid_cell > 0.0f) || n_items < 0)
    return DSU_EINVAL;
  if (W == 0 || H == 0) return DSU_OK;
  if (!offsets || (n_items && !items) || (n_verts && !verts) || (n_faces && !faces) || !mid || !thickness || !count)
    return DSU_EINVAL;
  const Mesh m{verts, faces, n_verts, n_faces};
  const ZGrid gr{grid_x0, grid_y0, 1.0f / grid_cell, g};
  const Lattice lt{x0, y0, h, W, H};
  const dim3 grid((unsigned)dsu_blocks_for(W, SIDE), (unsigned)dsu_blocks_for(H, SIDE));
  mesh_thickness_kernel<<<grid, THREADS, 0, (hipStream_t)stream>>>(m, gr, offsets, items, n_items, lt, mid, thickness,
                                                                   count);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_mesh_thickness_ortho_host(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, double x0,
                                  double y0, double h, int32_t W, int32_t H, double* mid, double* thickness,
                                  int32_t* count) {
  if (!args_ok(n_verts, n_faces, x0, y0, h, W, H)) return DSU_EINVAL;
  if (W == 0 || H == 0) return DSU_OK;
  if ((n_verts && !verts) || (n_faces && !faces) || !mid || !thickness || !count) return DSU_EINVAL;
  const int tw = dsu_blocks_for(W, SIDE), th = dsu_blocks_for(H, SIDE);
  std::vector<int64_t> offsets((size_t)tw * th + 1, 0);
  std::vector<int32_t> items;
  for (int pass = 0; pass < 2; ++pass) {                     // count, then fill
    std::vector<int64_t> cursor(offsets.begin(), offsets.end() - 1);
    for (int64_t f = 0; f < n_faces; ++f) {
      const Tri t = dsu_mt::load_tri(verts, n_verts, faces, n_faces, f);
      if (t.face < 0) continue;
      int tx0, tx1, ty0, ty1;
      if (!tile_range(fmin(fmin(t.ax, t.bx), t.cx), fmax(fmax(t.ax, t.bx), t.cx), x0, h, W, tx0, tx1) ||
          !tile_range(fmin(fmin(t.ay, t.by), t.cy), fmax(fmax(t.ay, t.by), t.cy), y0, h, H, ty0, ty1))
        continue;
      for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
          const size_t bin = (size_t)ty * tw + tx;
          if (pass == 0) ++offsets[bin + 1];
          else items[(size_t)cursor[bin]++] = t.face;
        }
    }
    if (pass == 0) {
      for (size_t b = 1; b < offsets.size(); ++b) offsets[b] += offsets[b - 1];
      items.resize((size_t)offsets.back());
    }
  }
  for (int32_t r = 0; r < H; ++r) {
    for (int32_t c = 0; c < W; ++c) {
      const double sx = dsu_mt::sample_at(x0, c, h), sy = dsu_mt::sample_at(y0, r, h);
      const size_t bin = (size_t)(r / SIDE) * tw + c / SIDE;
      const int64_t k0 = offsets[bin], k1 = offsets[bin + 1];
      Key cur{0.0, -1};
      Pairs p = dsu_mt::no_pairs();
      int32_t n = 0;
      for (bool first = true;; first = false) {
        Key lo{0.0, -1}, hi{0.0, -1};
        for (int64_t k = k0; k < k1; ++k) {
          const Tri t = dsu_mt::load_tri(verts, n_verts, faces, n_faces, items[(size_t)k]);
          if (first) dsu_mt::visit<true>(t, sx, sy, cur, lo, hi, n);
          else dsu_mt::visit<false>(t, sx, sy, cur, lo, hi, n);
        }
        if (p.taken >= (n & ~1) || hi.face < 0) break;
        dsu_mt::take(p, lo.z);
        dsu_mt::take(p, hi.z);
        cur = hi;
      }
      const int64_t at = (int64_t)r * W + c;
      mid[at] = p.mid;
      thickness[at] = p.thickness;
      count[at] = n;
    }
  }
  return DSU_OK;
}

}  // extern "C"
