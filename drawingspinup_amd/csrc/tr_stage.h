// Per-wave LDS images of the backward kernels' contractions over the points (or samples):
//   image[point 0..31][column 0..COLS-1] bf16, one image for the hi part and one for the mid part.
// A lane whose MFMA accumulator holds registers 4g .. 4g+3 of the point in its column stores them
// packed, four bf16 = 8 bytes = one SLOT of the point's row (ds_write_b64); the A or B fragment of the
// 32x32x16 MFMA that sums over the points is read back with ds_read_b64_tr_b16 (gfx950), which hands
// lane i of a 16-lane group column i of a block of 4 rows x 16 columns — the transpose for free.
//
// Layout.  Rows are dense (2 COLS bytes); slot s of point p sits at slot s ^ swz(p) of the row:
//   off(p, s) = p * 2 COLS + 8 * (s ^ swz(p))
//   COLS = 64 (16 slots, 128-byte rows): swz(p) = (p & 7) | (((p >> 3) ^ (p >> 1)) & 1) << 3
//   COLS = 32 ( 8 slots,  64-byte rows): swz(p) = (p >> 1) & 7
// Every offset is a multiple of 8; the image base must be a multiple of 2 COLS bytes, so that the
// slot bits of a lane's address can be changed with one XOR (store_base ^ 8 s, read_base ^ read_xor).
//
// Bank conflicts, computed by the functions below and asserted at compile time:
//   ds_write_b64  (4 groups of 16 consecutive lanes, bank = (a / 4) mod 32, 2 banks per lane): the 16
//     lanes of a group store the SAME slot of 16 consecutive points.  COLS = 64: a row is the 32 banks,
//     swz is a bijection of p & 15 -> 16 different slots: 0 extra cycles.  COLS = 32: two rows are the
//     32 banks, (p & 1, swz) is a bijection of p & 15: 0 extra cycles.
//   ds_read_b64_tr_b16 (2 groups of 32 lanes, bank = (a / 4) mod 64, 2 banks per lane): a lane half
//     reads 4 consecutive points (4-aligned) x 8 consecutive slots (8-aligned).  COLS = 32: that is four
//     whole rows = 256 contiguous bytes: 0 extra cycles.  COLS = 64: points q = 0..3 fall on the 128-byte
//     half q & 1 of the 64 banks, and bit 3 of swz differs between q and q ^ 2, which puts their 8 slots
//     in different halves of the row: 0 extra cycles.
// The transposed read needs EXEC all ones (masked lanes' addresses still take part): call it in
// wave-uniform control flow only, and pad rows without a point with zeros instead of masking.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TRS_HD __host__ __device__
#else
#define TRS_HD
#endif

namespace trs {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int COLS>
struct Img {
  static_assert(COLS == 32 || COLS == 64, "8 or 16 slots per row");
  static constexpr int ROW_B = 2 * COLS;          // bytes per point row
  static constexpr int SLOTS = COLS / 4;
  static constexpr int PART_B = 32 * ROW_B;       // bytes of one part (hi or mid)

  TRS_HD static constexpr int swz(int p) {
    return COLS == 64 ? ((p & 7) | ((((p >> 3) ^ (p >> 1)) & 1) << 3)) : ((p >> 1) & 7);
  }
  // byte offset of columns 4 s .. 4 s + 3 of point p
  TRS_HD static constexpr int off(int p, int s) { return p * ROW_B + 8 * (s ^ swz(p)); }

  // ---- stores: the lane of point p stores slot s at store_base(p) ^ (8 s)
  TRS_HD static constexpr int store_base(int p) { return off(p, 0); }

  // ---- transposed reads.  Operand fragment of k-step ks (points 16 ks + 8 h + j, j = 0..7, of lane
  // half h) for the 32 rows (A) or columns (B) 32 tile .. 32 tile + 31: two reads jj = 0, 1 of four
  // points each.  Lane l = 32 h + 16 c + 4 q + p supplies the address of point 16 ks + 8 h + 4 jj + q,
  // slot 8 tile + 4 c + p:
  //   read_off = (read_base(l) ^ read_xor(jj, tile)) + read_add(ks, jj)
  TRS_HD static constexpr int read_base(int l) {
    return off(8 * (l >> 5) + ((l >> 2) & 3), 4 * ((l >> 4) & 1) + (l & 3));
  }
  TRS_HD static constexpr int read_xor(int jj, int tile) {
    return COLS == 64 ? (32 * jj) ^ (64 * tile) : 16 * jj;
  }
  TRS_HD static constexpr int read_add(int ks, int jj) { return (16 * ks + 4 * jj) * ROW_B; }
  TRS_HD static constexpr int read_off(int l, int ks, int jj, int tile) {
    return (read_base(l) ^ read_xor(jj, tile)) + read_add(ks, jj);
  }

  // ---- column reads (COLS = 64): lane l of the wave receives column l of the four points P0 .. P0 + 3
  // (P0 a multiple of 4) — what a sum over the points of each column needs.  Lane l = 16 c + 4 q + p
  // supplies the address of point P0 + q, slot 4 c + p; swz is linear in the bits of the point, so
  //   col_off = (col_base(l) ^ col_xor(P0)) + P0 * ROW_B
  // The lanes of a half read 4 points x 8 consecutive slots like a fragment read: 0 extra cycles.
  TRS_HD static constexpr int col_base(int l) { return off((l >> 2) & 3, 4 * (l >> 4) + (l & 3)); }
  TRS_HD static constexpr int col_xor(int P0) { return 8 * swz(P0); }
  TRS_HD static constexpr int col_off(int l, int P0) { return (col_base(l) ^ col_xor(P0)) + P0 * ROW_B; }

  // ---- checks (compile time)
  // the decomposition above addresses what the instruction wants
  static constexpr bool read_map_ok() {
    for (int l = 0; l < 64; ++l)
      for (int ks = 0; ks < 2; ++ks)
        for (int jj = 0; jj < 2; ++jj)
          for (int tile = 0; tile < COLS / 32; ++tile) {
            const int h = l >> 5, c = (l >> 4) & 1, q = (l >> 2) & 3, p = l & 3;
            if (read_off(l, ks, jj, tile) != off(16 * ks + 8 * h + 4 * jj + q, 8 * tile + 4 * c + p)) return false;
          }
    for (int p = 0; p < 32; ++p)
      for (int s = 0; s < SLOTS; ++s)
        if ((store_base(p) ^ (8 * s)) != off(p, s)) return false;
    if (COLS == 64)
      for (int l = 0; l < 64; ++l)
        for (int P0 = 0; P0 < 32; P0 += 4)
          if (col_off(l, P0) != off(P0 + ((l >> 2) & 3), 4 * (l >> 4) + (l & 3))) return false;
    return true;
  }
  // extra LDS cycles of one wave instruction: `n` lanes per group, 8 bytes per lane, `banks` banks
  static constexpr int extra_cycles(const int (&a)[64], int n, int banks) {
    int extra = 0;
    for (int g = 0; g < 64 / n; ++g) {
      int worst = 1;
      for (int b = 0; b < banks; ++b) {
        int cnt = 0, seen[64] = {};
        for (int i = 0; i < n; ++i)
          for (int d = 0; d < 2; ++d) {
            const int dw = a[g * n + i] / 4 + d;
            if (dw % banks != b) continue;
            bool dup = false;
            for (int k = 0; k < cnt; ++k) dup = dup || seen[k] == dw;
            if (!dup) seen[cnt++] = dw;
          }
        worst = cnt > worst ? cnt : worst;
      }
      extra += worst - 1;
    }
    return extra;
  }
  // ds_write_b64 of slot s by the lanes of points p = l & 31 (both lane halves store the same rows)
  static constexpr int store_conflicts() {
    int worst = 0;
    for (int s = 0; s < SLOTS; ++s) {
      int a[64] = {};
      for (int l = 0; l < 64; ++l) a[l] = store_base(l & 31) ^ (8 * s);
      const int e = extra_cycles(a, 16, 32);
      worst = e > worst ? e : worst;
    }
    return worst;
  }
  static constexpr int read_conflicts() {
    int worst = 0;
    for (int ks = 0; ks < 2; ++ks)
      for (int jj = 0; jj < 2; ++jj)
        for (int tile = 0; tile < COLS / 32; ++tile) {
          int a[64] = {};
          for (int l = 0; l < 64; ++l) a[l] = read_off(l, ks, jj, tile);
          const int e = extra_cycles(a, 32, 64);
          worst = e > worst ? e : worst;
        }
    if (COLS == 64)
      for (int P0 = 0; P0 < 32; P0 += 4) {
        int a[64] = {};
        for (int l = 0; l < 64; ++l) a[l] = col_off(l, P0);
        const int e = extra_cycles(a, 32, 64);
        worst = e > worst ? e : worst;
      }
    return worst;
  }
  static_assert(read_map_ok(), "lane addresses of the transposed read");
  static_assert(store_conflicts() == 0, "ds_write_b64: 0 extra cycles per instruction");
  static_assert(read_conflicts() == 0, "ds_read_b64_tr_b16: 0 extra cycles per instruction");
};

#if defined(__HIPCC__)
#define TRS_LDS __attribute__((address_space(3)))
// 32-bit LDS byte address of a pointer into __shared__ memory
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(TRS_LDS const char*)p;
}
// ds_read_b64_tr_b16 at LDS byte address a: element q = row q of the block, this lane's column
__device__ __forceinline__ bf16x4 read_tr(uint32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((TRS_LDS bf16x4*)(uintptr_t)a);
#else
  return bf16x4{};
#endif
}
// the fragment of k-step ks, tile `tile`: rd = image address (a multiple of 2 COLS) + read_base(lane);
// `add` = a compile-time byte offset behind the XOR (the mid part: PART_B)
template <int COLS>
__device__ __forceinline__ bf16x8 frag_tr(uint32_t rd, int ks, int tile, int add = 0) {
  const bf16x4 lo = read_tr((rd ^ (uint32_t)Img<COLS>::read_xor(0, tile)) + Img<COLS>::read_add(ks, 0) + add);
  const bf16x4 hi = read_tr((rd ^ (uint32_t)Img<COLS>::read_xor(1, tile)) + Img<COLS>::read_add(ks, 1) + add);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// four bf16 -> slot s of the lane's point row: st = image address + store_base(point) (^ lane-dependent
// slot bits, if any); `add` as above
__device__ __forceinline__ void store_slot(uint32_t st, int s, int add, bf16x4 v) {
  *(TRS_LDS bf16x4*)(uintptr_t)((st ^ (uint32_t)(8 * s)) + add) = v;
}
#endif

}  // namespace trs
