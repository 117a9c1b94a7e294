// Who does which 32-sample half of the texture backward (texture_mlp.hip), for host and device.
//
// A half whose d_rgb rows are all zero is DEAD: the kernel writes its d_feature = 0 and its d_grad from
// d_normal alone, and that is all.  A LIVE half costs the recompute, seven bf16 x 3 products and the
// staging.  So the halves are handed out by their live count: with L live halves among H, part k of P
// takes the contiguous run of halves that holds the live ranks [k L / P, (k + 1) L / P) — from the live
// half of its first rank up to (not including) the live half of the next part's first rank; the first
// part starts at half 0, the last ends at H.  Live counts of two parts differ by at most one, every
// half belongs to exactly one part, parts are in order.  A run without a live half (L = 0) is cut into
// equal numbers of halves instead.  The rule is applied twice: [0, H) over the launched workgroups, a
// workgroup's run over its waves.  Nothing in it depends on timing: two launches over the same
// bitmap group the parameter-gradient partial sums the same way.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSU_TEXPART_HD __host__ __device__ __forceinline__
#else
#define DSU_TEXPART_HD static inline
#endif

namespace texpart {

// the scan the kernel keeps in LDS: at most this many bitmap words (32 halves = 1024 samples each)
constexpr int MAX_WORDS = 2048;                    // 2 097 152 samples

// bits[w]: the bitmap, bits at or beyond `halves` cleared; pre[w]: live halves before word w, pre[words] = all
struct Scan {
  const uint32_t* bits;
  const uint32_t* pre;
  int words;
  int halves;
};

struct Run {
  int h0, h1;     // halves [h0, h1)
  int l0, l1;     // their live ranks [l0, l1)
};

DSU_TEXPART_HD int popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

// the bitmap word with the bits at or beyond `halves` cleared (a stale or foreign bit there is nobody's half)
DSU_TEXPART_HD uint32_t clip_word(uint32_t word, int w, int halves) {
  const int left = halves - 32 * w;
  return left >= 32 ? word : (left <= 0 ? 0u : word & ((1u << left) - 1u));
}

// the half with live rank `rank` (0 <= rank < pre[words])
DSU_TEXPART_HD int select(const Scan& s, int rank) {
  int lo = 0, hi = s.words - 1;                    // the last word w with pre[w] <= rank
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)s.pre[mid] <= rank) lo = mid;
    else hi = mid - 1;
  }
  uint32_t word = s.bits[lo];
  for (int k = rank - (int)s.pre[lo]; k > 0; --k) word &= word - 1u;   // drop the k lowest set bits
  int bit = 0;
  while (bit < 31 && !((word >> bit) & 1u)) ++bit;
  return 32 * lo + bit;
}

// part k of P of the run r
DSU_TEXPART_HD Run split(const Scan& s, const Run& r, int P, int k) {
  Run o;
  const int64_t live = r.l1 - r.l0, len = r.h1 - r.h0;
  if (live == 0) {
    o.l0 = o.l1 = r.l0;
    o.h0 = r.h0 + (int)(k * len / P);
    o.h1 = r.h0 + (int)((k + 1) * len / P);
    return o;
  }
  o.l0 = r.l0 + (int)(k * live / P);
  o.l1 = r.l0 + (int)((k + 1) * live / P);
  o.h0 = k == 0 ? r.h0 : select(s, o.l0);
  o.h1 = k == P - 1 ? r.h1 : select(s, o.l1);
  return o;
}

DSU_TEXPART_HD Run whole(const Scan& s) {
  Run r;
  r.h0 = 0; r.h1 = s.halves; r.l0 = 0; r.l1 = (int)s.pre[s.words];
  return r;
}

}  // namespace texpart
