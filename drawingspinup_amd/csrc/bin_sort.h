// The counting sort every mesh stage bins with (gfx950): items are sorted onto bins in two launches
// around the caller's exclusive prefix sum.
//   COUNT   counts[bin] += 1 for every (item, bin) pair
//   (the caller writes offsets[0 .. nb] = exclusive prefix sum of counts)
//   FILL    items[offsets[bin] + cursor[bin]++] = id, for the same pairs
// Order within a bin comes from the atomics and is free; the consumers do not depend on it.
//
// What differs between the stages is only how an item enumerates the bins it touches: a "source"
// functor, passed to the kernel by value, with
//   __device__ int32_t id(int64_t i) const;                 the id stored for launch index i
//   template <class Emit> __device__ void bins(int64_t i, Emit emit) const;
//                                                           emit(bin) once per bin i touches
// both __forceinline__, so that the kernel below is one straight piece of code per source.
#pragma once
#include "common.h"

namespace dsu_bin {

// n_items of an entry point whose ABI has no item count (dsu_zgrid_fill, dsu_point_bin_fill): the
// write is guarded all the same, and for offsets that are a prefix sum of the counts the guard
// never fires.
constexpr int64_t NO_LIMIT = INT64_MAX;

// MODE 0: `tally` is counts.  MODE 1: `tally` is the zeroed cursor.
template <int MODE, class Source>
__global__ __launch_bounds__(256) void bin_kernel(Source src, int64_t n, int32_t* __restrict__ tally,
                                                  const int32_t* __restrict__ offsets,
                                                  int32_t* __restrict__ items, int64_t n_items) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t id = src.id(i);
  src.bins(i, [&](int bin) {
    const int k = atomicAdd(&tally[bin], 1);
    if (MODE == 1) {
      const int64_t at = (int64_t)offsets[bin] + k;
      if (at >= 0 && at < n_items) items[at] = id;
    }
  });
}

template <int MODE, class Source>
inline void launch(const Source& src, int64_t n, int32_t* tally, const int32_t* offsets, int32_t* items,
                   int64_t n_items, hipStream_t st) {
  bin_kernel<MODE><<<dsu_blocks_for(n, 256), 256, 0, st>>>(src, n, tally, offsets, items, n_items);
}

// ---- the staged entry points' workspace: counts (nb) | offsets (nb + 1) | cursor (nb), int32
struct Workspace {
  int32_t *counts, *offsets, *cursor;
};

inline Workspace split(void* base, int64_t nb) {
  int32_t* counts = (int32_t*)base;
  return {counts, counts + nb, counts + 2 * nb + 1};
}

inline int64_t bytes(int64_t nb) { return (3 * nb + 1) * (int64_t)sizeof(int32_t); }

constexpr int32_t COUNT = 0, FILL = 1;   // = DSU_RENDER_* = DSU_UV_* = DSU_SKIN_*

// Stage COUNT or FILL of a staged entry point over n launch indices.  offsets is written by the
// caller between the two.
template <class Source>
inline int run_stage(int32_t stage, const Source& src, int64_t n, void* workspace, int64_t nb,
                     int32_t* items, int64_t n_items, hipStream_t st) {
  const Workspace w = split(workspace, nb);
  if (hipMemsetAsync(stage == COUNT ? w.counts : w.cursor, 0, nb * sizeof(int32_t), st) != hipSuccess)
    return DSU_ELAUNCH;
  if (stage == COUNT) {
    if (n) launch<0>(src, n, w.counts, nullptr, nullptr, 0, st);
  } else if (n && n_items) {
    launch<1>(src, n, w.cursor, w.offsets, items, n_items, st);
  }
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

}  // namespace dsu_bin
