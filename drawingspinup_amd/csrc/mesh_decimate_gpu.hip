// Parallel quadric edge-collapse decimation on the device: the bulk of `remesh()` of the
// reference's export (instant_nsr/utils/mesh_utils.py:10-22, geometry.py:63-64: the 512^3
// marching-cubes mesh, 1-3 M triangles, down to face_count = 50 000).
//
// The reference hands this to Open3D's serial priority-queue algorithm (host).  The serial form
// (csrc/mesh_decimate.hip, same file header: Garland & Heckbert quadrics, boundary planes,
// minimiser-or-endpoints target, normal-flip rejection, link condition) costs ~13 s of one host
// core at that size — three times the whole NSR optimisation.  Here the same admissible-collapse
// rules run as ROUNDS of independent collapses:
//   1. vertex -> triangle lists (CSR) of the live mesh; one "owner" half-edge per edge;
//   2. cost + target of every edge;
//   3. the cheapest `budget` edges are candidates, ranked by (cost, edge order);
//   4. every candidate writes a (hashed, unique) priority into all vertices of its closed
//      neighbourhood (v0, v1 and their one-rings) with atomicMin; a candidate whose two END POINTS
//      still carry its priority is selected: no selected collapse has an end point equal or
//      adjacent to another's, so their flip tests, link conditions and updates cannot see each
//      other (see collapse_kernel);
//   5. selected + admissible collapses are applied in place; dead triangles are compacted away.
// A collapse rejected by the flip / link tests is remembered (direct-mapped table keyed by the
// edge, valid while neither end point's neighbourhood changed) so that it does not keep winning
// its neighbourhood round after round.
// How the four selection passes of a round are run (claim_kernel / collapse_kernel, one launch per
// pass and kernel; none of it changes which collapses are taken):
//   * records: pass 0 reads a candidate's rank, edge and end points once and writes (r, v0, v1);
//     the later kernels of the round read records, handed on through two lists that keep only the
//     candidates still undecided (see Cand);
//   * stamping: a candidate writes each vertex of its closed neighbourhood once per fan, not once
//     per triangle, and only where a plain read of the word shows it could still lower it
//     (see fan_ring, stamp);
//   * marks: the end points of an applied collapse get round * 16 + pass in ONE array; a pass takes a
//     vertex for dirty when its mark is of an earlier pass of the same round
//     (see DSU_MARK_ROUND_BITS);
//   * the round's three counters and the list appends take one atomic per wave.
// The rounds stop above the target (`stop_faces`) and never go below `floor_faces`; the caller
// finishes the last stretch with the serial code seeded with the accumulated quadrics
// (dsu_mesh_decimate_quadric_q), which also lands on the exact face count.
//
// Everything is float64 (positions, quadrics, costs): near-planar regions have costs ~1e-20 that
// float32 quadrics cannot order.  Deterministic: vertex lists are sorted, ranks are unique, sums
// run in list order; atomics only take minima of unique integers.
// Scans / compaction / radix sort: hipCUB device primitives (header-only), on the caller's stream
// with the caller's workspace.
// The arithmetic of the quadrics, the edge's target, the initial planes and the flip test is
// decimate_quadric.h, shared with the serial queue (mesh_decimate.hip).
#include "common.h"
#include "decimate_quadric.h"

#include <math.h>
#include <stdint.h>

#include <hipcub/hipcub.hpp>

namespace {

using dsu_dq::Quadric;
using dsu_dq::V3;

struct Mesh {
  double* P;        // (nv,3)
  double* Q;        // (nv,10)
  int32_t* F;       // (nf,3) live triangles
  int32_t* voff;    // (nv+1) CSR offsets
  int32_t* vfaces;  // (3 nf)
  int64_t nv, nf;
};

__device__ inline V3 ldP(const Mesh& m, int32_t v) { return {m.P[3 * v], m.P[3 * v + 1], m.P[3 * v + 2]}; }
__device__ inline Quadric ldQ(const Mesh& m, int32_t v) {
  Quadric a;
  for (int i = 0; i < 10; ++i) a.q[i] = m.Q[10 * (int64_t)v + i];
  return a;
}
__device__ inline bool tri_has(const Mesh& m, int32_t t, int32_t v) {
  return m.F[3 * t] == v || m.F[3 * t + 1] == v || m.F[3 * t + 2] == v;
}
__device__ inline void edge_target(const Mesh& m, int32_t v0, int32_t v1, double& cost, V3& vbar) {
  Quadric q = ldQ(m, v0);
  q.add(ldQ(m, v1));
  dsu_dq::edge_target(q, ldP(m, v0), ldP(m, v1), cost, vbar);
}

// ------------------------------------------------------------------------------------ CSR
__global__ void flag_nondegenerate_kernel(const int32_t* F, int64_t nf, uint8_t* flag) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nf; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t a = F[3 * t], b = F[3 * t + 1], c = F[3 * t + 2];
    flag[t] = (a != b && b != c && a != c) ? 1 : 0;
  }
}

__global__ void degree_kernel(const int32_t* F, int64_t nf, int32_t* deg) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 3 * nf; i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&deg[F[i]], 1);
}

__global__ void fill_kernel(const int32_t* F, int64_t nf, const int32_t* voff, int32_t* cursor, int32_t* vfaces) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 3 * nf; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = F[i];
    vfaces[voff[v] + atomicAdd(&cursor[v], 1)] = (int32_t)(i / 3);
  }
}

// insertion sort of every vertex's triangle list: list order (hence every later sum and scan) does
// not depend on the order the atomics above happened to run in
__global__ void sort_lists_kernel(const int32_t* voff, int32_t* vfaces, int64_t nv) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
    const int32_t b = voff[v], e = voff[v + 1];
    for (int32_t i = b + 1; i < e; ++i) {
      const int32_t x = vfaces[i];
      int32_t j = i - 1;
      while (j >= b && vfaces[j] > x) { vfaces[j + 1] = vfaces[j]; --j; }
      vfaces[j + 1] = x;
    }
  }
}

// does some live triangle hold the half-edge a -> b ?
__device__ inline bool has_half_edge(const Mesh& m, int32_t a, int32_t b) {
  for (int32_t i = m.voff[a]; i < m.voff[a + 1]; ++i) {
    const int32_t t = m.vfaces[i];
    for (int k = 0; k < 3; ++k)
      if (m.F[3 * t + k] == a && m.F[3 * t + (k + 1) % 3] == b) return true;
  }
  return false;
}

// ------------------------------------------------------------------------------------ quadrics
__global__ void init_quadrics_kernel(Mesh m, double boundary_weight) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < m.nv; v += (int64_t)gridDim.x * blockDim.x) {
    Quadric q;
    for (int32_t i = m.voff[v]; i < m.voff[v + 1]; ++i) {
      const int32_t t = m.vfaces[i];
      const int32_t a = m.F[3 * t], b = m.F[3 * t + 1], c = m.F[3 * t + 2];
      const V3 pa = ldP(m, a), pb = ldP(m, b), pc = ldP(m, c);
      const V3 cr = cross(pb - pa, pc - pa);
      const double l = norm(cr);
      if (!(l > 0.0)) continue;
      const dsu_dq::Plane fp = dsu_dq::face_plane(cr, l, pa);
      q.add_plane(fp.n, fp.d, fp.w);
      if (boundary_weight > 0.0) {
        // the two edges of t at v; an edge with no opposite half-edge is a boundary edge
        for (int k = 0; k < 3; ++k) {
          const int32_t e0 = m.F[3 * t + k], e1 = m.F[3 * t + (k + 1) % 3];
          if (e0 != (int32_t)v && e1 != (int32_t)v) continue;
          if (has_half_edge(m, e1, e0)) continue;
          // a second triangle with the SAME half-edge (non-manifold fan): not a boundary
          int same = 0;
          for (int32_t j = m.voff[e0]; j < m.voff[e0 + 1]; ++j) {
            const int32_t t2 = m.vfaces[j];
            for (int kk = 0; kk < 3; ++kk)
              if (m.F[3 * t2 + kk] == e0 && m.F[3 * t2 + (kk + 1) % 3] == e1) ++same;
          }
          if (same != 1) continue;
          const int32_t lo = e0 < e1 ? e0 : e1, hi = e0 < e1 ? e1 : e0;
          const V3 phi = ldP(m, hi), plo = ldP(m, lo);     // hi first: the order the kernel was generated in
          const V3 en = dsu_dq::boundary_cross(plo, phi, fp.n);
          const double el = norm(en);
          if (!(el > 0.0)) continue;
          const dsu_dq::Plane bp = dsu_dq::boundary_plane(en, el, plo, l, boundary_weight);
          q.add_plane(bp.n, bp.d, bp.w);
        }
      }
    }
    for (int i = 0; i < 10; ++i) m.Q[10 * v + i] = q.q[i];
  }
}

// ------------------------------------------------------------------------------------ edges
// half-edge i = 3 t + k (a -> b) owns its edge when a < b, or when a > b and no triangle holds b -> a
__global__ void owner_flags_kernel(Mesh m, uint8_t* flag) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 3 * m.nf; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / 3;
    const int k = (int)(i % 3);
    const int32_t a = m.F[3 * t + k], b = m.F[3 * t + (k + 1) % 3];
    flag[i] = (a < b || (a > b && !has_half_edge(m, b, a))) ? 1 : 0;
  }
}

// Direct-mapped memory of rejected collapses, one 64-bit word per slot:
//   [63:48] round of the rejection | [47:0] hash of (edge, version of v0, version of v1)
// written with atomicMax: a later round replaces an earlier one, and when several rejections of one
// round fall into one slot the larger hash stays — the same one on every run (a plain store would
// keep whichever writer came last).  A look-up compares the low 48 bits with the hash of the
// edge's CURRENT versions.
typedef unsigned long long Reject;

__device__ inline unsigned long long ekey(int32_t a, int32_t b) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  return ((unsigned long long)lo << 32) | hi;
}
__device__ inline unsigned long long mix64(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}
__device__ inline uint32_t slot_of(unsigned long long key, uint32_t n_slots) {
  return (uint32_t)(mix64(key) % n_slots);
}
__device__ inline unsigned long long reject_tag(unsigned long long key, uint32_t ver0, uint32_t ver1) {
  return mix64(key ^ mix64(((unsigned long long)ver0 << 32) | ver1)) & 0xffffffffffffull;
}

// cost of every owner half-edge, as the float32 bit pattern of max(cost, 0) (monotone as an
// unsigned integer); remembered rejections get +inf
__global__ void edge_cost_kernel(Mesh m, const int32_t* edges, int64_t ne, const Reject* rej, uint32_t n_slots,
                                 const uint32_t* vver, uint32_t* cost_bits, uint32_t* edge_idx) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t h = edges[e];
    const int32_t t = h / 3, k = h % 3;
    const int32_t a = m.F[3 * t + k], b = m.F[3 * t + (k + 1) % 3];
    const int32_t v0 = a < b ? a : b, v1 = a < b ? b : a;
    double cost; V3 vb;
    edge_target(m, v0, v1, cost, vb);
    float c = (float)(cost > 0.0 ? cost : 0.0);
    const unsigned long long key = ekey(v0, v1);
    if ((rej[slot_of(key, n_slots)] & 0xffffffffffffull) == reject_tag(key, vver[v0], vver[v1])) c = INFINITY;
    cost_bits[e] = __float_as_uint(c);
    edge_idx[e] = (uint32_t)e;
  }
}

__device__ inline void edge_ends(const Mesh& m, int32_t h, int32_t& v0, int32_t& v1) {
  const int32_t t = h / 3, k = h % 3;
  const int32_t a = m.F[3 * t + k], b = m.F[3 * t + (k + 1) % 3];
  v0 = a < b ? a : b;
  v1 = a < b ? b : a;
}

// Priority of a candidate inside the independent-set selection: a hash of (edge, round) — NOT its
// cost rank.  Costs vary smoothly over the surface (and tie on regular meshes), so "the cheapest
// edge of its neighbourhood wins" leaves one winner per monotone chain: a few dozen collapses per
// round on a 150 k-triangle sphere.  The cost decides who is a candidate (the cheapest `ncand`
// edges); a locally random, globally unique 64-bit priority decides which non-conflicting subset
// of them goes first.
__device__ inline unsigned long long priority_of(int32_t v0, int32_t v1, uint32_t round, uint32_t r) {
  unsigned long long k = ekey(v0, v1) ^ ((unsigned long long)round * 0x9e3779b97f4a7c15ull);
  k ^= k >> 31; k *= 0xbf58476d1ce4e5b9ull; k ^= k >> 29; k *= 0x94d049bb133111ebull; k ^= k >> 32;
  return (k << 32) | r;                                      // unique: r is the candidate's index
}

// Several selection passes share one round's lists, edge list and cost order.  After a pass, the
// lists of the end points of applied collapses are stale (v1 is gone, v0 gained triangles) and so
// is every triangle that held a v1: a candidate is `dirty` — skipped until the next round — when
// any vertex of its closed neighbourhood was an end point of a collapse applied in an earlier pass
// of this round (its mark in `touched`).  Everything a clean candidate reads is as it was at round
// start.
//
// ONE array of marks serves all passes: a collapse applied in pass p of round R writes
// mark_base(R) + p on its two end points, and pass q tests `mark - mark_base(R) < q` (unsigned):
// true exactly for the marks of earlier passes of this round.  Marks of earlier rounds lie below
// mark_base(R) and wrap to huge values, the initial 0xffffffff stays >= 2^31 above any base, and
// the marks the running pass itself writes (difference == q) do not count — what the second array
// and the copy after every pass were for.  mark_base(R) = (R mod 2^27) * 16; the host refills the
// array whenever R mod 2^27 returns to 0, so no mark of an earlier epoch can alias.
#define DSU_MARK_ROUND_BITS 27
#define DSU_MARK_PASS_SLOTS 16u

// A candidate of the round: its rank r in the cost order (the low word of its priority, see
// priority_of) and the end points of its edge.  Pass 0 reads sorted_cost[r], edges[sorted_idx[r]] and
// the edge's end points ONCE and writes the record; every later kernel of the round reads records.
// The records still undecided travel from kernel to kernel through two lists: a candidate leaves
// when it is dirty (marks are never taken back inside a round: dirty once, dirty in every later
// pass) or when its collapse was applied (its end points then carry a mark: it would be dirty).
// A REJECTED candidate stays, also while the table remembers it: the table is direct-mapped, another
// rejection of the round may take its slot in any pass, and the candidate is then tested (and
// counted as rejected) again, as it was when every pass asked every candidate.  Each pass after the
// first therefore makes that code's probe for every record.  The order of a list depends on the order the waves
// appended in; nothing computed depends on that order: r travels with the record, claim[] takes
// minima, the counters are integer sums, the table takes maxima.
typedef uint4 Cand;                                           // x = r, y = v0, z = v1

#define DSU_FAN 8
// The corners of the triangles around v, as at most 2 * DSU_FAN vertex ids in registers (-1: none),
// each DISTINCT vertex other than v at least once.  Triangle j of the list gives u[j], the corner
// after v, and u[DSU_FAN + j], the corner before v, unless that vertex is the corner after v of one
// of these triangles.  In a closed fan every ring vertex is the corner after v of one triangle and
// the corner before v of another, so the second half empties; on an open fan, a fan of mixed
// orientation or a non-manifold one a vertex that is nobody's `after` stays in the second half
// (and one held by three triangles may stay twice: more stamps than needed, never fewer vertices).
// Triangles past the DSU_FAN-th (the poles) are left to the caller, corner by corner.
// A triangle of a stale list may no longer hold v (v was collapsed away in an earlier pass): then
// two of its corners are returned, and the caller's test of v's own mark decides (claim_kernel).
__device__ inline void fan_ring(const Mesh& m, int32_t v, int32_t (&u)[2 * DSU_FAN]) {
  const int32_t b = m.voff[v], e = m.voff[v + 1];
#pragma unroll
  for (int j = 0; j < DSU_FAN; ++j) {
    int32_t nx = -1, pv = -1;
    if (b + j < e) {
      const int32_t t = m.vfaces[b + j];
      const int32_t a0 = m.F[3 * t], a1 = m.F[3 * t + 1], a2 = m.F[3 * t + 2];
      if (a0 == v) { nx = a1; pv = a2; }
      else if (a1 == v) { nx = a2; pv = a0; }
      else { nx = a0; pv = a1; }
    }
    u[j] = nx;
    u[DSU_FAN + j] = pv;
  }
#pragma unroll
  for (int j = 0; j < DSU_FAN; ++j) {                         // a `before` that is somebody's `after` goes
    int32_t same = 0;
#pragma unroll
    for (int i = 0; i < DSU_FAN; ++i) same |= (int32_t)(u[i] == u[DSU_FAN + j]);
    u[DSU_FAN + j] = same ? -1 : u[DSU_FAN + j];
  }
}

__device__ inline bool mark_earlier_pass(const uint32_t* touched, int32_t u, uint32_t mark_base, uint32_t pass) {
  return touched[u] - mark_base < pass;
}

// `claim[u]` only falls while the kernel runs, so whatever a plain load returns (a stale line of
// the vector cache included) is >= the word's current value: when it is already <= pr, the
// atomicMin could not have changed the word, and leaving it out leaves the final claim[] — the
// minimum over the same set of (vertex, priority) pairs — as it was.
__device__ inline void stamp(unsigned long long* claim, int32_t u, unsigned long long pr) {
  if (claim[u] > pr) atomicMin(&claim[u], pr);
}

// one record per lane with `keep` -> out[*n_out ...]; one atomic per wave.  Whole waves call this.
__device__ inline void wave_append(bool keep, Cand c, Cand* out, int32_t* n_out) {
  const unsigned long long mask = __ballot(keep);
  if (mask == 0) return;
  const int lane = threadIdx.x & (DSU_WAVE - 1);
  int32_t base = 0;
  if (lane == 0) base = atomicAdd(n_out, (int32_t)__popcll(mask));
  base = __shfl(base, 0);
  if (keep) out[base + __popcll(mask & ((1ull << lane) - 1ull))] = c;
}

__device__ inline int wave_sum(int x) {
#pragma unroll
  for (int o = DSU_WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// Every candidate stamps its priority on all vertices of its closed neighbourhood (v0, v1, rings).
// What is stamped is the SET of vertices the earlier kernel reached by writing every corner of
// every triangle around v0 and around v1 (about 36 atomics for about 10 vertices): v0 and v1 once
// (each lies in a triangle of the edge), the ring of each fan through fan_ring, every corner of the
// triangles past DSU_FAN.  The same set of pairs under a minimum: the same claim[].
// FIRST (pass 0 of a round): reads the cost order and writes the records; no mark of this round
// exists yet (nothing dirty), and the table was probed by edge_cost_kernel a moment ago with the
// same versions (remembered == +inf cost), so neither test is made.
template <bool FIRST>
__global__ void claim_kernel(Mesh m, const int32_t* edges, const uint32_t* sorted_idx, const uint32_t* sorted_cost,
                             int64_t ncand, const Cand* in, const int32_t* n_in, Cand* out, int32_t* n_out,
                             uint32_t mark_base, uint32_t pass, uint32_t seed, const uint32_t* touched,
                             const Reject* rej, uint32_t n_slots, const uint32_t* vver,
                             unsigned long long* claim) {
  const int64_t n = FIRST ? ncand : (int64_t)*n_in;
  const int lane = threadIdx.x & (DSU_WAVE - 1);
  // whole waves go round the loop together (wave_append)
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x - lane); base < n;
       base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + lane;
    bool keep = false, remembered = false;
    Cand c = make_uint4(0u, 0u, 0u, 0u);
    if (i < n) {
      int32_t v0, v1;
      if (FIRST) {
        keep = sorted_cost[i] != 0x7f800000u;               // +inf: remembered rejection
        if (keep) {
          edge_ends(m, edges[sorted_idx[i]], v0, v1);
          c = make_uint4((uint32_t)i, (uint32_t)v0, (uint32_t)v1, 0u);
        }
      } else {
        c = in[i];
        v0 = (int32_t)c.y; v1 = (int32_t)c.z;
        // rejected in an earlier pass of this round and still remembered: sits this pass out, but
        // stays on the list (the table may have forgotten it by the next pass)
        const unsigned long long key = ekey(v0, v1);
        remembered = (rej[slot_of(key, n_slots)] & 0xffffffffffffull) == reject_tag(key, vver[v0], vver[v1]);
        keep = true;
      }
      if (keep && !remembered) {
        int32_t u0[2 * DSU_FAN], u1[2 * DSU_FAN];
        fan_ring(m, v0, u0);
        fan_ring(m, v1, u1);
        const int32_t t0 = m.voff[v0] + DSU_FAN, e0 = m.voff[v0 + 1];
        const int32_t t1 = m.voff[v1] + DSU_FAN, e1 = m.voff[v1 + 1];
        if (!FIRST) {
          // dirty: a mark of an earlier pass on any vertex the earlier walk read, i.e. on any corner
          // of any triangle of the two lists (fan_ring drops only repeats), or on v0 / v1
          bool dirty = mark_earlier_pass(touched, v0, mark_base, pass) | mark_earlier_pass(touched, v1, mark_base, pass);
#pragma unroll
          for (int j = 0; j < 2 * DSU_FAN; ++j) {
            if (u0[j] >= 0) dirty |= mark_earlier_pass(touched, u0[j], mark_base, pass);
            if (u1[j] >= 0) dirty |= mark_earlier_pass(touched, u1[j], mark_base, pass);
          }
          for (int32_t q = t0; q < e0; ++q)
            for (int k = 0; k < 3; ++k) dirty |= mark_earlier_pass(touched, m.F[3 * m.vfaces[q] + k], mark_base, pass);
          for (int32_t q = t1; q < e1; ++q)
            for (int k = 0; k < 3; ++k) dirty |= mark_earlier_pass(touched, m.F[3 * m.vfaces[q] + k], mark_base, pass);
          keep = !dirty;
        }
        if (keep) {
          const unsigned long long pr = priority_of(v0, v1, seed, c.x);
          stamp(claim, v0, pr);
          stamp(claim, v1, pr);
#pragma unroll
          for (int j = 0; j < 2 * DSU_FAN; ++j) {
            if (u0[j] >= 0 && u0[j] != v1) stamp(claim, u0[j], pr);
            if (u1[j] >= 0 && u1[j] != v0) stamp(claim, u1[j], pr);
          }
          for (int32_t q = t0; q < e0; ++q)
            for (int k = 0; k < 3; ++k) stamp(claim, m.F[3 * m.vfaces[q] + k], pr);
          for (int32_t q = t1; q < e1; ++q)
            for (int k = 0; k < 3; ++k) stamp(claim, m.F[3 * m.vfaces[q] + k], pr);
        }
      }
    }
    wave_append(keep, c, out, n_out);
  }
}

// Selected = both END POINTS still carry this candidate's priority.  If an end point of another
// candidate B lies in the closed neighbourhood of A, A stamped it and B stamped one of A's end
// points (adjacency is symmetric), so at most one of the two keeps both of its end points: selected
// collapses never have an end point equal or adjacent to another's.  That is all they need: a
// collapse moves v0, deletes v1 and rewrites only triangles around v1; its tests read the
// positions of ring vertices (not moved: not end points of a selected collapse) and the triangles
// around v0 / v1 (not rewritten: they would have to contain another collapse's v1, which would
// then be a ring vertex).  Rings may overlap.
// selected -> admissibility tests of the serial code -> apply
struct Outcome {
  int what;      // 0 = not selected, 1 = rejected (remembered), 2 = applied
  int removed;   // triangles the collapse removed
};
__device__ inline Outcome test_and_apply(const Mesh& m, int32_t v0, int32_t v1, uint32_t round, int link_test,
                                     uint8_t* f_alive, Reject* rej, uint32_t n_slots, uint32_t* vver,
                                     uint32_t* touched, uint32_t mark) {
  {
    double cost; V3 vbar;
    edge_target(m, v0, v1, cost, vbar);
    const int32_t b0 = m.voff[v0], e0 = m.voff[v0 + 1], b1 = m.voff[v1], e1 = m.voff[v1 + 1];
    int shared = 0;
    bool bad = false;
    for (int pass = 0; pass < 2 && !bad; ++pass) {
      const int32_t mv = pass ? v0 : v1, other = pass ? v1 : v0;
      for (int32_t i = m.voff[mv]; i < m.voff[mv + 1]; ++i) {
        const int32_t t = m.vfaces[i];
        if (tri_has(m, t, other)) { if (!pass) ++shared; continue; }
        V3 p[3], q[3];
        for (int k = 0; k < 3; ++k) {
          p[k] = ldP(m, m.F[3 * t + k]);
          q[k] = m.F[3 * t + k] == mv ? vbar : p[k];
        }
        if (flips(p, q)) { bad = true; break; }
      }
    }
    if (!bad && shared == 0) bad = true;
    if (!bad && link_test) {
      // |N(v0) ∩ N(v1)| must equal the number of triangles on the edge
      int common = 0;
      for (int32_t i = b0; i < e0; ++i) {
        const int32_t t = m.vfaces[i];
        for (int k = 0; k < 3; ++k) {
          const int32_t u = m.F[3 * t + k];
          if (u == v0 || u == v1) continue;
          // first occurrence of u in the ring of v0 ?
          bool first = true;
          for (int32_t j = b0; j < i && first; ++j)
            if (tri_has(m, m.vfaces[j], u)) first = false;
          if (first)
            for (int kk = 0; kk < k; ++kk)
              if (m.F[3 * t + kk] == u) first = false;
          if (!first) continue;
          bool in1 = false;
          for (int32_t j = b1; j < e1 && !in1; ++j)
            if (tri_has(m, m.vfaces[j], u)) in1 = true;
          if (in1) ++common;
        }
      }
      if (common != shared) bad = true;
      // no triangle (v1, x, y) next to a triangle (v0, x, y)
      for (int32_t j = b1; j < e1 && !bad; ++j) {
        const int32_t t1 = m.vfaces[j];
        if (tri_has(m, t1, v0)) continue;
        int32_t x = -1, y = -1, k2 = 0;                       // (two scalars: an indexed pair went to LDS)
        for (int k = 0; k < 3; ++k) {
          const int32_t c = m.F[3 * t1 + k];
          if (c != v1 && k2 < 2) { if (k2 == 0) x = c; else y = c; ++k2; }
        }
        if (k2 < 2) continue;
        for (int32_t i = b0; i < e0; ++i) {
          const int32_t t0 = m.vfaces[i];
          if (!tri_has(m, t0, v1) && tri_has(m, t0, x) && tri_has(m, t0, y)) { bad = true; break; }
        }
      }
    }
    if (bad) {
      const unsigned long long key = ekey(v0, v1);
      atomicMax(&rej[slot_of(key, n_slots)],
                ((unsigned long long)(round & 0xffffu) << 48) | reject_tag(key, vver[v0], vver[v1]));
      return {1, 0};
    }
    // ---- collapse v1 into v0 (this thread owns every vertex and triangle it touches)
    for (int pass = 0; pass < 2; ++pass) {                  // the neighbourhood changed: versions
      const int32_t v = pass ? v1 : v0;
      for (int32_t i = m.voff[v]; i < m.voff[v + 1]; ++i) {
        const int32_t t = m.vfaces[i];
        for (int k = 0; k < 3; ++k) atomicAdd(&vver[m.F[3 * t + k]], 1u);   // rings may be shared
      }
    }
    int removed = 0;
    for (int32_t j = b1; j < e1; ++j) {
      const int32_t t = m.vfaces[j];
      if (tri_has(m, t, v0)) {
        f_alive[t] = 0;
        ++removed;
      } else {
        for (int k = 0; k < 3; ++k)
          if (m.F[3 * t + k] == v1) m.F[3 * t + k] = v0;
      }
    }
    m.P[3 * v0] = vbar.x; m.P[3 * v0 + 1] = vbar.y; m.P[3 * v0 + 2] = vbar.z;
    for (int i = 0; i < 10; ++i) m.Q[10 * (int64_t)v0 + i] += m.Q[10 * (int64_t)v1 + i];
    touched[v0] = mark;                                      // dirty for the LATER passes of this round only
    touched[v1] = mark;                                      // (see DSU_MARK_ROUND_BITS)
    return {2, removed};
  }
}

// A candidate whose two end points carry its priority did stamp them: the low word of a priority
// is the rank r, which no other candidate writes.  So it passed claim_kernel's tests in this same
// pass (not remembered, not dirty), and the marks it read there are the ones it would read here:
// the walk the earlier kernel repeated at this point could never find anything.
// Records that stay undecided (not selected, or rejected: see Cand) go to `out` for the next pass;
// out == nullptr in the last pass.  counters[0..2] (collapses, rejections, triangles removed) get
// one add per wave: integer sums, the same totals.
__global__ void collapse_kernel(Mesh m, const Cand* in, const int32_t* n_in, Cand* out, int32_t* n_out,
                                uint32_t round, uint32_t mark, uint32_t seed, const unsigned long long* claim,
                                int link_test, uint8_t* f_alive, Reject* rej, uint32_t n_slots, uint32_t* vver,
                                uint32_t* touched, int32_t* counters) {
  const int32_t n = *n_in;                                  // <= ncand <= 2^28: 32-bit arithmetic below
  const int lane = threadIdx.x & (DSU_WAVE - 1);
  // Every wave of the grid takes one contiguous run of the list, so that the few records of a late
  // pass spread over all waves instead of filling a few: the selected lanes of a wave make their
  // walks in lockstep, every load touching as many cache lines as lanes take part, and the launch
  // lasts as long as its slowest wave (last pass of a round on a 465 k-face mesh: ~190 us with the
  // list packed 64 to the wave, ~85 us spread out; on the export's own, larger mesh the two forms
  // come out even over a call: profiles/remesh_rounds_ab.txt).
  const int32_t waves = (int32_t)(gridDim.x * (blockDim.x / DSU_WAVE));   // <= 2048 * 4
  const int32_t wave = (int32_t)(blockIdx.x * (blockDim.x / DSU_WAVE) + threadIdx.x / DSU_WAVE);
  const int32_t per_wave = (n + waves - 1) / waves;
  const int32_t end = (wave + 1) * per_wave < n ? (wave + 1) * per_wave : n;
  int n_applied = 0, n_rejected = 0, n_removed = 0;
  for (int32_t base = wave * per_wave; base < end; base += DSU_WAVE) {
    const int32_t i = base + lane;
    Outcome o = {0, 0};
    bool stay = false;
    Cand c = make_uint4(0u, 0u, 0u, 0u);
    if (i < end) {
      c = in[i];
      const int32_t v0 = (int32_t)c.y, v1 = (int32_t)c.z;
      const unsigned long long pr = priority_of(v0, v1, seed, c.x);
      if (claim[v0] == pr && claim[v1] == pr)
        o = test_and_apply(m, v0, v1, round, link_test, f_alive, rej, n_slots, vver, touched, mark);
      stay = o.what != 2;
    }
    const int applied = (int)__popcll(__ballot(o.what == 2));
    n_applied += applied;
    n_rejected += (int)__popcll(__ballot(o.what == 1));
    if (applied) n_removed += wave_sum(o.removed);
    if (out) wave_append(stay, c, out, n_out);
  }
  if (lane == 0) {
    if (n_applied) atomicAdd(&counters[0], n_applied);
    if (n_rejected) atomicAdd(&counters[1], n_rejected);
    if (n_removed) atomicAdd(&counters[2], n_removed);
  }
}

struct Tri {
  int32_t a, b, c;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Layout {
  size_t off_Q, off_F2, off_voff, off_cursor, off_vfaces, off_flag, off_edges, off_iota, off_cost, off_cost2,
      off_idx, off_idx2, off_claim, off_vver, off_touched, off_rej, off_counters, off_nsel, off_cub, cub_bytes, total;
  uint32_t n_slots;
};

Layout make_layout(int64_t nv, int64_t nf) {
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
  L.off_Q = take((size_t)nv * 10 * sizeof(double));
  L.off_F2 = take((size_t)nf * 3 * sizeof(int32_t));
  L.off_voff = take((size_t)(nv + 1) * sizeof(int32_t));
  L.off_cursor = take((size_t)(nv + 1) * sizeof(int32_t));
  L.off_vfaces = take((size_t)nf * 3 * sizeof(int32_t));
  L.off_flag = take((size_t)nf * 3);
  L.off_edges = take((size_t)nf * 3 * sizeof(int32_t));
  L.off_iota = take((size_t)nf * 3 * sizeof(int32_t));
  L.off_cost = take((size_t)nf * 3 * sizeof(uint32_t));
  L.off_cost2 = take((size_t)nf * 3 * sizeof(uint32_t));
  L.off_idx = take((size_t)nf * 3 * sizeof(uint32_t));
  L.off_idx2 = take((size_t)nf * 3 * sizeof(uint32_t));
  L.off_claim = take((size_t)nv * sizeof(unsigned long long));
  L.off_vver = take((size_t)nv * sizeof(uint32_t));
  L.off_touched = take((size_t)nv * sizeof(uint32_t));
  L.n_slots = (uint32_t)(nv * 2 + 1024);
  L.off_rej = take((size_t)L.n_slots * sizeof(Reject));
  L.off_counters = take(64);
  L.off_nsel = take(64);
  // hipCUB temporary storage: the largest of the calls below at the largest sizes
  size_t b_scan = 0, b_sel_i = 0, b_sel_t = 0, b_sort = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, b_scan, (int32_t*)nullptr, (int32_t*)nullptr, (int)(nv + 1));
  hipcub::DeviceSelect::Flagged(nullptr, b_sel_i, (int32_t*)nullptr, (uint8_t*)nullptr, (int32_t*)nullptr,
                                (int32_t*)nullptr, (int)(3 * nf));
  hipcub::DeviceSelect::Flagged(nullptr, b_sel_t, (Tri*)nullptr, (uint8_t*)nullptr, (Tri*)nullptr, (int32_t*)nullptr,
                                (int)nf);
  hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                     (uint32_t*)nullptr, (int)(3 * nf));
  L.cub_bytes = std::max(std::max(b_scan, b_sel_i), std::max(b_sel_t, b_sort)) + 256;
  L.off_cub = take(L.cub_bytes);
  L.total = o;
  return L;
}

__global__ void iota_kernel(int32_t* p, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = (int32_t)i;
}

}  // namespace

#define DSU_HIP_TRY(expr)                       \
  do {                                          \
    if ((expr) != hipSuccess) return DSU_ELAUNCH; \
  } while (0)

extern "C" {

int64_t dsu_mesh_decimate_parallel_workspace_bytes(int64_t n_verts, int64_t n_faces) {
  if (n_verts < 0 || n_faces < 0 || n_verts > (1 << 30) || n_faces > (1 << 29)) return DSU_EINVAL;
  return (int64_t)make_layout(n_verts, n_faces).total;
}

int dsu_mesh_decimate_parallel(double* verts, int64_t n_verts, int32_t* faces, int64_t n_faces,
                               int64_t stop_faces, int64_t floor_faces, double boundary_weight, int32_t flags,
                               int32_t max_rounds, double* out_quadrics, int64_t* out_n_faces,
                               int32_t* out_stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_verts < 0 || n_faces < 0 || stop_faces < floor_faces || floor_faces < 0 || !out_n_faces ||
      (n_verts && !verts) || (n_faces && !faces) || !(boundary_weight >= 0.0) || max_rounds < 0 ||
      n_verts > (1 << 30) || n_faces > (1 << 29))
    return DSU_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (out_stats) out_stats[0] = out_stats[1] = out_stats[2] = 0;
  *out_n_faces = n_faces;
  if (n_faces == 0 || n_verts == 0) return DSU_OK;
  const Layout L = make_layout(n_verts, n_faces);
  if (!workspace || workspace_bytes < (int64_t)L.total) return DSU_EINVAL;
  char* w = (char*)workspace;
  double* Q = (double*)(w + L.off_Q);
  int32_t* F2 = (int32_t*)(w + L.off_F2);
  int32_t* voff = (int32_t*)(w + L.off_voff);
  int32_t* cursor = (int32_t*)(w + L.off_cursor);
  int32_t* vfaces = (int32_t*)(w + L.off_vfaces);
  uint8_t* flag = (uint8_t*)(w + L.off_flag);
  int32_t* edges = (int32_t*)(w + L.off_edges);
  int32_t* iota = (int32_t*)(w + L.off_iota);
  uint32_t* cost = (uint32_t*)(w + L.off_cost);
  uint32_t* cost2 = (uint32_t*)(w + L.off_cost2);
  uint32_t* idx = (uint32_t*)(w + L.off_idx);
  uint32_t* idx2 = (uint32_t*)(w + L.off_idx2);
  unsigned long long* claim = (unsigned long long*)(w + L.off_claim);
  uint32_t* vver = (uint32_t*)(w + L.off_vver);
  uint32_t* touched = (uint32_t*)(w + L.off_touched);
  Reject* rej = (Reject*)(w + L.off_rej);
  int32_t* counters = (int32_t*)(w + L.off_counters);
  int32_t* nsel = (int32_t*)(w + L.off_nsel);
  void* cub = (void*)(w + L.off_cub);
  const int T = 256;
  const int PASSES = 4;                     // selection passes per round (see claim_kernel)
  static_assert(PASSES <= (int)DSU_MARK_PASS_SLOTS && 4 + 2 * PASSES <= 16, "marks and list counts of a round");
  // The two candidate lists of the passes live in the radix sort's INPUT arrays, which nothing reads
  // between the sort of a round and the edge costs of the next: a round has ncand <= budget <=
  // nf / 2 records of 16 bytes (or the single one of `ncand < 1`, with nf >= 2), the arrays hold
  // 3 nf words of 4 bytes each.
  Cand* list_a = (Cand*)cost;
  Cand* list_b = (Cand*)idx;
  const int link_test = !(flags & 1);

  int32_t* F = faces;                       // live triangles, compacted in place (through F2)
  int64_t nf = n_faces;
  int32_t host_n = 0;
  auto compact_faces = [&]() -> int {       // flag[0..nf) marks the survivors
    size_t b = L.cub_bytes;
    if (hipcub::DeviceSelect::Flagged(cub, b, (Tri*)F, flag, (Tri*)F2, nsel, (int)nf, s) != hipSuccess)
      return DSU_ELAUNCH;
    if (hipMemcpyAsync(&host_n, nsel, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess) return DSU_ELAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return DSU_ELAUNCH;
    nf = host_n;
    if (nf && hipMemcpyAsync(F, F2, (size_t)nf * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return DSU_ELAUNCH;
    return DSU_OK;
  };
  auto build_csr = [&]() -> int {
    DSU_HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)(n_verts + 1) * sizeof(int32_t), s));
    degree_kernel<<<dsu_capped_blocks(3 * nf, T), T, 0, s>>>(F, nf, cursor);
    size_t b = L.cub_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(cub, b, cursor, voff, (int)(n_verts + 1), s) != hipSuccess)
      return DSU_ELAUNCH;
    DSU_HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)(n_verts + 1) * sizeof(int32_t), s));
    fill_kernel<<<dsu_capped_blocks(3 * nf, T), T, 0, s>>>(F, nf, voff, cursor, vfaces);
    sort_lists_kernel<<<dsu_capped_blocks(n_verts, T), T, 0, s>>>(voff, vfaces, n_verts);
    DSU_CHECK_LAUNCH();
    return DSU_OK;
  };

  // triangles with a repeated vertex carry no surface
  flag_nondegenerate_kernel<<<dsu_capped_blocks(nf, T), T, 0, s>>>(F, nf, flag);
  DSU_CHECK_LAUNCH();
  int rc = compact_faces();
  if (rc) return rc;
  DSU_HIP_TRY(hipMemsetAsync(vver, 0, (size_t)n_verts * sizeof(uint32_t), s));
  DSU_HIP_TRY(hipMemsetAsync(touched, 0xff, (size_t)n_verts * sizeof(uint32_t), s));
  DSU_HIP_TRY(hipMemsetAsync(rej, 0, (size_t)L.n_slots * sizeof(Reject), s));
  iota_kernel<<<dsu_capped_blocks(3 * nf, T), T, 0, s>>>(iota, 3 * nf);
  if ((rc = build_csr())) return rc;
  Mesh m{verts, Q, F, voff, vfaces, n_verts, nf};
  init_quadrics_kernel<<<dsu_capped_blocks(n_verts, T), T, 0, s>>>(m, boundary_weight);
  DSU_CHECK_LAUNCH();

  int rounds = 0, applied_total = 0, rejected_total = 0, stall = 0;
  while (nf > stop_faces && rounds < max_rounds) {
    const int64_t budget = (nf - floor_faces) / 2;
    if (budget < 1) break;
    m.nf = nf;
    // owner half-edges -> edge list
    owner_flags_kernel<<<dsu_capped_blocks(3 * nf, T), T, 0, s>>>(m, flag);
    DSU_CHECK_LAUNCH();
    size_t b = L.cub_bytes;
    if (hipcub::DeviceSelect::Flagged(cub, b, iota, flag, edges, nsel, (int)(3 * nf), s) != hipSuccess)
      return DSU_ELAUNCH;
    DSU_HIP_TRY(hipMemcpyAsync(&host_n, nsel, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DSU_HIP_TRY(hipStreamSynchronize(s));
    const int64_t ne = host_n;
    if (ne == 0) break;
    edge_cost_kernel<<<dsu_capped_blocks(ne, T), T, 0, s>>>(m, edges, ne, rej, L.n_slots, vver, cost, idx);
    DSU_CHECK_LAUNCH();
    b = L.cub_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(cub, b, cost, cost2, idx, idx2, (int)ne, 0, 32, s) != hipSuccess)
      return DSU_ELAUNCH;
    int64_t ncand = budget < ne / 2 ? budget : ne / 2;
    if (ncand < 1) ncand = 1;
    DSU_HIP_TRY(hipMemsetAsync(counters, 0, 64, s));
    DSU_HIP_TRY(hipMemsetAsync(flag, 1, (size_t)nf, s));
    // counters (16 words, zeroed above): [0..2] collapses, rejections, triangles removed;
    // [4 + 2 p] records claim_kernel of pass p passed on, [5 + 2 p] records collapse_kernel did
    const uint32_t mark_round = (uint32_t)rounds & ((1u << DSU_MARK_ROUND_BITS) - 1u);
    if (rounds > 0 && mark_round == 0)      // the marks start over: none of the last epoch may stay
      DSU_HIP_TRY(hipMemsetAsync(touched, 0xff, (size_t)n_verts * sizeof(uint32_t), s));
    const uint32_t mark_base = mark_round * DSU_MARK_PASS_SLOTS;
    const int blocks = dsu_capped_blocks(ncand, T);
    for (int pass = 0; pass < PASSES; ++pass) {
      const uint32_t seed = (uint32_t)rounds * 16u + (uint32_t)pass;
      int32_t* n_claimed = counters + 4 + 2 * pass;
      int32_t* n_left = counters + 5 + 2 * pass;
      DSU_HIP_TRY(hipMemsetAsync(claim, 0xff, (size_t)n_verts * sizeof(unsigned long long), s));
      if (pass == 0)
        claim_kernel<true><<<blocks, T, 0, s>>>(m, edges, idx2, cost2, ncand, nullptr, nullptr, list_b, n_claimed,
                                                mark_base, 0u, seed, touched, rej, L.n_slots, vver, claim);
      else
        claim_kernel<false><<<blocks, T, 0, s>>>(m, edges, idx2, cost2, ncand, list_a, n_left - 2, list_b, n_claimed,
                                                 mark_base, (uint32_t)pass, seed, touched, rej, L.n_slots, vver,
                                                 claim);
      collapse_kernel<<<blocks, T, 0, s>>>(m, list_b, n_claimed, pass + 1 < PASSES ? list_a : nullptr, n_left,
                                           (uint32_t)rounds, mark_base + (uint32_t)pass, seed, claim, link_test, flag,
                                           rej, L.n_slots, vver, touched, counters);
      DSU_CHECK_LAUNCH();
    }
    int32_t hc[3];
    DSU_HIP_TRY(hipMemcpyAsync(hc, counters, sizeof(hc), hipMemcpyDeviceToHost, s));
    DSU_HIP_TRY(hipStreamSynchronize(s));
    ++rounds;
    applied_total += hc[0];
    rejected_total += hc[1];
    if (hc[0] == 0) {
      // nothing admissible among the winners: their rejections are remembered, the next round sees
      // other winners; give up when that does not help either
      if (++stall >= 4) break;
      continue;
    }
    stall = 0;
    const int64_t before = nf;
    if ((rc = compact_faces())) return rc;
    // a round that removes under 0.5 % of a mesh already within 4x of the target (candidates
    // clustered in one place): the serial queue is the faster way from here
    if ((before - nf) * 200 < before && nf <= 4 * stop_faces) break;
    if (nf == 0) break;
    if ((rc = build_csr())) return rc;
  }
  if (out_quadrics)
    DSU_HIP_TRY(hipMemcpyAsync(out_quadrics, Q, (size_t)n_verts * 10 * sizeof(double), hipMemcpyDeviceToDevice, s));
  DSU_HIP_TRY(hipStreamSynchronize(s));
  *out_n_faces = nf;
  if (out_stats) { out_stats[0] = rounds; out_stats[1] = applied_total; out_stats[2] = rejected_total; }
  return DSU_OK;
}

}  // extern "C"
