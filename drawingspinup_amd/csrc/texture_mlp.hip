// Radiance ("texture") MLP of the NeuS model, forward and backward, on the matrix pipes of gfx950.
//
// Replaces VolumeRadiance.forward (2_charactor_reconstructor/instant_nsr/models/texture.py:9-30)
// = VanillaMLP 16 -> 64 -> 64 -> 3 with ReLU (models/network_utils.py:94-138, no weight norm for
// this network) followed by sigmoid, and its autograd backward.  The reference runs it as three
// library GEMMs + elementwise kernels forward and ~10 GEMMs / reductions backward over N ~ 2.6e5
// samples with 16..64 columns: tall-skinny shapes the library handles at a few percent of peak.
//
// One wave = 64 samples.  Activations live transposed in MFMA accumulators
//   H^T[64 hidden x 32 samples] per sample half:  lane = sample, register quad = 4 hidden units,
// and are fed straight back as the B operand of the next layer (the k-pair of one register is
// (unit, unit+4) across the two lane halves; the weight operand is permuted to match, exactly as
// in hashgrid_mfma.hip).
//
// Which pipe runs what:
//   exact f32 (v_mfma_f32_32x32x2_f32): layers 0 and 1 of the forward kernel and of the backward's
//     recompute, with their biases as one more k-pair.  Layer 2 (3 outputs), dPre1 = W2^T dz and the
//     bias gradients gb1 / gb2 are plain VALU arithmetic.
//   bf16 x 3 (v_mfma_f32_32x32x16_bf16, x = hi + mid, three products: 2^-16 relative): every GEMM
//     of the backward proper.  dH0 = W1^T dPre1 and dIn = W0^T dPre0 take the accumulator of the
//     previous phase as the B operand as it stands and read the weights from images in LDS; the
//     parameter-gradient GEMMs gW2, gW1, gW0 (contraction over samples = lanes) go through
//     per-wave [sample][unit] images in LDS, 32 samples at a time: packed 8-byte stores of an
//     accumulator's register quads, operand fragments through ds_read_b64_tr_b16, which transposes
//     (tr_stage.h).  When the forward handed over the
//     ReLU pattern of layer 1 (L1_MASK), the recompute of layer 1 runs this way too.
#include <vector>
#include "common.h"
#include "tr_stage.h"
#include "tex_partition.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// x = hi + mid + O(2^-16 |x|), hi and mid in bf16: operands of the "bf16 x 3" products
// a b ~ a_hi b_hi + a_hi b_mid + a_mid b_hi on v_mfma_f32_32x32x16_bf16 (16x the f32 MFMA's rate),
// used for the backward's GEMMs (see the file header)
__device__ __forceinline__ void bf16_split8(const float* x, bf16x8& hi, bf16x8& mid) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const __bf16 hh = (__bf16)x[i];
    hi[i] = hh;
    mid[i] = (__bf16)(x[i] - (float)hh);
  }
}

constexpr int TIN = 16, THID = 64, TOUT = 3;
// LDS map of the backward kernel, in floats (the forward kernel has the weights only):
//   [0, L_WEND)             5 576   weights and biases in f32 (load_weights)
//   [L_WEND, L_STAGE)          24   padding: the staging images start on a multiple of 128 bytes
//   [L_STAGE, L_IMG1)  4 x 5 120   per-wave staging: the [sample][column] bf16 images X, Y, S
//   [L_IMG1, L_IMG0)        4 096   W1 image of dH0
//   [L_IMG0, L_IMGF)        2 048   W0 image of dIn
//   [L_IMGF, BWD_LDS_F)     4 096   W1 image of the recompute of layer 1 (written by L1_MASK kernels)
//   BWD_LDS_F = 36 320 floats = 142 KB of the CU's 160: one workgroup per CU.  (+ 16 KB behind it: L_SCAN)
// The workgroup reduction at the end of the kernel reuses [0, 4 PART_STRIDE) for four partial images.
constexpr int W1_ROW = 65;                       // padded row: conflict-free by row AND by column
constexpr int W0_ROW = 17;
constexpr int L_W1 = 0;
constexpr int L_W0 = L_W1 + THID * W1_ROW;       // 4160
constexpr int L_W2P = L_W0 + THID * W0_ROW;      // 5248: w2perm[h][o][32]
constexpr int L_B0 = L_W2P + 2 * TOUT * 32;      // 5440
constexpr int L_B1 = L_B0 + THID;
constexpr int L_B2 = L_B1 + THID;                // 5568
constexpr int L_WEND = L_B2 + 8;                 // 5576
// per-wave staging (backward): bf16 images of the contraction-over-samples GEMMs (gW2, gW1, gW0 as
// bf16 x 3), tr_stage.h:
// [part hi | mid][sample of the 32-sample half][column = unit (or output / input column)] bf16.  A lane
// stores the four units of an accumulator register quad of its sample packed (8 bytes); the operand
// fragments — 8 consecutive samples of one column per lane — come back through the transposing read.
// Stores and reads are conflict-free (computed in tr_stage.h).  Two 64-column images (X, Y) and one
// 32-column image (S: dz in columns 0..2, then In in columns 0..15 and the ones column 16) per wave.
typedef trs::Img<64> ImgU;
typedef trs::Img<32> ImgS;
constexpr int SB_X = 0, SB_Y = 2 * ImgU::PART_B, SB_S = 4 * ImgU::PART_B;     // byte offsets
constexpr int STAGE_F = (4 * ImgU::PART_B + 2 * ImgS::PART_B) / 4;            // 5120 floats
constexpr int L_STAGE = (L_WEND + 31) / 32 * 32;                              // 5600
static_assert(STAGE_F * 4 % ImgU::ROW_B == 0 && SB_S % ImgS::ROW_B == 0, "image bases: multiples of the row");
// bf16 images of the backward GEMMs' weight operands, one 16-byte fragment per lane and MFMA:
//   W1 image [hi|mid][To][Tin][g][lane] : 8 values t -> w1[feat_of(Tin, 8 g + t, h)][32 To + l31]
//   W0 image [hi|mid][T][g][lane]       : 8 values t -> w0[feat_of(T, 8 g + t, h)][l31] (0 for l31 >= 16)
constexpr int IMG1_F = 2 * 8 * 64 * 4, IMG0_F = 2 * 4 * 64 * 4;       // floats (16 B = 4 floats per fragment)
constexpr int L_IMG1 = L_STAGE + 4 * STAGE_F;
constexpr int L_IMG0 = L_IMG1 + IMG1_F;
//   W1 image of the backward's forward RECOMPUTE (L1_MASK kernels) [hi|mid][To][Tin][g][lane] :
//   8 values t -> w1[32 To + l31][feat_of(Tin, 8 g + t, h)]
constexpr int L_IMGF = L_IMG0 + IMG0_F;
constexpr int BWD_LDS_F = L_IMGF + IMG1_F;       // 36 320 floats = 142 KB
//   [L_SCAN, BWD_LDS_ALL_F)  the liveness bitmap of the halves and its scan (tex_partition.h): 16 KB more,
//   158 KB in all.  Not part of what the final reduction reuses.
constexpr int L_SCAN = BWD_LDS_F;
constexpr int BWD_LDS_ALL_F = L_SCAN + 2 * texpart::MAX_WORDS + 8;
static_assert(BWD_LDS_ALL_F * 4 <= 160 * 1024, "the backward kernel's LDS fits the CU");
// per-workgroup partial vector
constexpr int P_GW1 = 0, P_GW0 = 64 * 64, P_GW2 = P_GW0 + 64 * 32, P_GB1 = P_GW2 + 64 * 32,
              P_GB2 = P_GB1 + 64, PART_N = P_GB2 + 3, PART_STRIDE = 8320;
constexpr int TEX_MAX_BLOCKS = 256;

__device__ __forceinline__ int feat_of(int T, int r, int h) {
  return 32 * T + (r & 3) + 8 * (r >> 2) + 4 * h;
}

__device__ __forceinline__ void swap_halves(float a, float b, float& o0, float& o1) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  o0 = __uint_as_float(r[0]);
  o1 = __uint_as_float(r[1]);
}

__device__ __forceinline__ void load_weights(float* lds, const dsu_tex_mlp& m) {
  for (int i = threadIdx.x; i < THID * THID; i += blockDim.x)
    lds[L_W1 + (i >> 6) * W1_ROW + (i & 63)] = m.w1[i];
  for (int i = threadIdx.x; i < THID * TIN; i += blockDim.x)
    lds[L_W0 + (i >> 4) * W0_ROW + (i & 15)] = m.w0[i];
  for (int i = threadIdx.x; i < 2 * TOUT * 32; i += blockDim.x) {
    const int h = i / (TOUT * 32), o = (i / 32) % TOUT, tr = i & 31;
    lds[L_W2P + i] = m.w2[o * THID + feat_of(tr >> 4, tr & 15, h)];
  }
  for (int i = threadIdx.x; i < THID; i += blockDim.x) {
    lds[L_B0 + i] = m.b0[i];
    lds[L_B1 + i] = m.b1[i];
  }
  for (int i = threadIdx.x; i < TOUT; i += blockDim.x) lds[L_B2 + i] = m.b2[i];
}

// Hidden activations of ONE sample half `a` (0: samples of lanes 0-31, 1: lanes 32-63).
// in: the lane's OWN sample (16 inputs).  H0/H1: [hidden tile T] accumulators, post-ReLU.
// L1_BF16 (the backward's recompute when the forward handed over its ReLU pattern of layer 1): layer 1
// as bf16 x 3 on v_mfma_f32_32x32x16_bf16 — the post-ReLU accumulators of layer 0 are the B operand
// as they stand (registers 8 g + t of tile Tin = units feat_of(Tin, 8 g + t, h) of the lane's sample
// column), the A fragments come from the image at L_IMGF: 24 MFMAs of 32 clocks instead of 64 of 64.
template <bool L1_BF16 = false>
__device__ __forceinline__ void forward_half(const float* lds, const float* in, int a, int l31,
                                             int h, f32x16 (&H0)[2], f32x16 (&H1)[2]) {
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int r = 0; r < 16; ++r) H0[T][r] = 0.0f;
  // layer 0: H0^T = W0 . In^T (+ b0 as the k-pair (1, 0))
#pragma unroll
  for (int t = 0; t < TIN / 2; ++t) {
    float b0v, b1v;
    swap_halves(in[2 * t], in[2 * t + 1], b0v, b1v);
    const float b = a == 0 ? b0v : b1v;
#pragma unroll
    for (int T = 0; T < 2; ++T)
      H0[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[L_W0 + (32 * T + l31) * W0_ROW + 2 * t + h],
                                                   b, H0[T], 0, 0, 0);
  }
  {
    const float one = h == 0 ? 1.0f : 0.0f;
#pragma unroll
    for (int T = 0; T < 2; ++T)
      H0[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(h == 0 ? lds[L_B0 + 32 * T + l31] : 0.0f, one,
                                                   H0[T], 0, 0, 0);
  }
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      H0[T][r] = fmaxf(H0[T][r], 0.0f);
      H1[T][r] = 0.0f;
    }
  // layer 1: H1^T = W1 . H0^T ; register (T, r) of H0 is the k-pair (feat_of(T,r,0), +4).
  // The weight operands of the NEXT four k-pairs are requested from LDS before the eight MFMAs of
  // the current four are issued (written per k-pair, the compiler put every `ds_read` right in
  // front of its MFMA with `s_waitcnt lgkmcnt(0)` in between: one MFMA per LDS round trip).
  if constexpr (L1_BF16) {
    // (one B fragment pair at a time: the kernel has no registers for all four)
    const bf16x8* imgf = reinterpret_cast<const bf16x8*>(lds + L_IMGF);
    const int lane = l31 + 32 * h;
#pragma unroll
    for (int Tin = 0; Tin < 2; ++Tin)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        float v[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = H0[Tin][8 * g + t];
        bf16x8 bh, bm;
        bf16_split8(v, bh, bm);
#pragma unroll
        for (int To = 0; To < 2; ++To) {
          const int f = ((To * 2 + Tin) * 2 + g) * 64 + lane;
          const bf16x8 ah = imgf[f], am = imgf[8 * 64 + f];
          H1[To] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, H1[To], 0, 0, 0);
          H1[To] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, H1[To], 0, 0, 0);
          H1[To] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, H1[To], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);        // (keeps the next pair's fragments out of this one's registers)
      }
  } else {
    float a[2][8];
    auto load = [&](int s_, float* dst) {
      const int T = s_ >> 2, rq = s_ & 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = feat_of(T, 4 * rq + j, h);
        dst[2 * j + 0] = lds[L_W1 + l31 * W1_ROW + k];
        dst[2 * j + 1] = lds[L_W1 + (32 + l31) * W1_ROW + k];
      }
    };
    load(0, a[0]);
#pragma unroll
    for (int s_ = 0; s_ < 8; ++s_) {
      if (s_ + 1 < 8) load(s_ + 1, a[(s_ + 1) & 1]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float b = H0[s_ >> 2][4 * (s_ & 3) + j];
        H1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s_ & 1][2 * j + 0], b, H1[0], 0, 0, 0);
        H1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s_ & 1][2 * j + 1], b, H1[1], 0, 0, 0);
      }
    }
  }
  {
    const float one = h == 0 ? 1.0f : 0.0f;
#pragma unroll
    for (int To = 0; To < 2; ++To)
      H1[To] = __builtin_amdgcn_mfma_f32_32x32x2f32(h == 0 ? lds[L_B1 + 32 * To + l31] : 0.0f,
                                                    one, H1[To], 0, 0, 0);
  }
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int r = 0; r < 16; ++r) H1[T][r] = fmaxf(H1[T][r], 0.0f);
}

// partial dot products of the 3 outputs over the 32 hidden units this lane holds (sample l31 of
// half a); the other 32 units sit in lane ^ 32
__device__ __forceinline__ void layer2_partial(const float* lds, const f32x16 (&H1)[2], int h,
                                               float (&p)[TOUT]) {
#pragma unroll
  for (int o = 0; o < TOUT; ++o) {
    const float4* w4 = reinterpret_cast<const float4*>(lds + L_W2P + (h * TOUT + o) * 32);
    float s = 0.0f;
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 w = w4[T * 4 + q];
        s = fmaf(w.x, H1[T][4 * q + 0], s);
        s = fmaf(w.y, H1[T][4 * q + 1], s);
        s = fmaf(w.z, H1[T][4 * q + 2], s);
        s = fmaf(w.w, H1[T][4 * q + 3], s);
      }
    p[o] = s;
  }
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// SHADE: the input row is not read from a (n,16) buffer but built here from the geometry network's
// outputs — cat(feature(13), normalize(sdf_grad)(3)) (neus.py:143, texture.py:22): what
// shade_prep_fwd_kernel materialised in a separate launch.  `normal_out` (n,3) is written for the
// compositing kernels.
struct ShadeIn {
  const float* feature;   // (n,13)
  const float* grad;      // (n,3)
};

__device__ __forceinline__ void load_shaded(const ShadeIn& si, int64_t ii, float (&in)[TIN],
                                            float& inv_len) {
#pragma unroll
  for (int k = 0; k < 13; ++k) in[k] = si.feature[ii * 13 + k];
  const float g0 = si.grad[ii * 3], g1 = si.grad[ii * 3 + 1], g2 = si.grad[ii * 3 + 2];
  inv_len = 1.0f / fmaxf(sqrtf(g0 * g0 + g1 * g1 + g2 * g2), 1e-12f);
  in[13] = g0 * inv_len; in[14] = g1 * inv_len; in[15] = g2 * inv_len;
}

template <bool SHADE>
__global__ __launch_bounds__(256) void texture_fwd_kernel(dsu_tex_mlp m,
                                                          const float* __restrict__ x, ShadeIn sh,
                                                          float* __restrict__ normal_out, int64_t n,
                                                          float* __restrict__ rgb,
                                                          uint32_t* __restrict__ h1_mask) {
  __shared__ __attribute__((aligned(16))) float lds[L_WEND];
  const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
  load_weights(lds, m);
  __syncthreads();
  // one contiguous range of samples per workgroup: the remainder of n over 256 x 256 samples
  // becomes a short last iteration everywhere (one wave, one sample half) instead of a full extra
  // round on a few CUs
  const int wave = threadIdx.x >> 6;
  const int64_t per = ((n + gridDim.x - 1) / gridDim.x + 31) / 32 * 32;
  const int64_t r0 = blockIdx.x * per;
  const int64_t r1 = r0 + per < n ? r0 + per : n;
  for (int64_t base = r0; base < r1; base += blockDim.x) {
    const int64_t i = base + threadIdx.x;
    const bool valid = i < r1;
    const int64_t ii = valid ? i : r1 - 1;
    const int64_t wave_first = base + wave * 64;
    if (wave_first >= r1) continue;                    // wave-uniform, no barrier in the loop
    float in[TIN];
    if (SHADE) {
      float inv_len;
      load_shaded(sh, ii, in, inv_len);
      if (valid) {
        normal_out[i * 3] = in[13]; normal_out[i * 3 + 1] = in[14]; normal_out[i * 3 + 2] = in[15];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(x + ii * TIN + 4 * q);
        in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
      }
    }
    float out[TOUT] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int a = 0; a < 2; ++a) {
      if (wave_first + a * 32 >= r1) continue;
      f32x16 H0[2], H1[2];
      forward_half(lds, in, a, l31, h, H0, H1);
      if (h1_mask) {
        // the ReLU pattern of layer 1 for the backward (bit 16 T + r = unit feat_of(T, r, h) of the
        // sample in column l31): its recompute may then round differently without moving a mask
        uint32_t mk = 0u;
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
          for (int r = 0; r < 16; ++r) mk |= (H1[T][r] > 0.0f ? 1u : 0u) << (16 * T + r);
        const int64_t si = wave_first + a * 32 + l31;
        if (si < r1) h1_mask[si * 2 + h] = mk;
      }
      float p[TOUT];
      layer2_partial(lds, H1, h, p);
#pragma unroll
      for (int o = 0; o < TOUT; ++o) {
        const float tot = p[o] + __shfl_xor(p[o], 32);     // both lanes of the pair get the sum
        if (h == a) out[o] = tot;                          // the lane whose OWN sample is in half a
      }
    }
    if (valid) {
#pragma unroll
      for (int o = 0; o < TOUT; ++o) rgb[i * TOUT + o] = sigmoidf(out[o] + lds[L_B2 + o]);
    }
  }
}

// columns = hidden units: the lane's 32 values X[T][r] (unit 32 T + (r & 3) + 8 (r >> 2) + 4 h of the
// sample in column l31) -> bf16 hi / mid in the sample's row of a 64-column image: registers
// 4 g .. 4 g + 3 of tile T are slot 8 T + 2 g + h.  st = image address + (store_base(l31) ^ 8 h)
__device__ __forceinline__ void stage_units_T(uint32_t st, const f32x16 (&X)[2]) {
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      trs::bf16x4 hi, mid;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float x = X[T][4 * g + c];
        const __bf16 hh = (__bf16)x;
        hi[c] = hh;
        mid[c] = (__bf16)(x - (float)hh);
      }
      trs::store_slot(st, 8 * T + 2 * g, 0, hi);
      trs::store_slot(st, 8 * T + 2 * g, ImgU::PART_B, mid);
    }
}
// four columns of the lane's own sample -> slot s of its row of the 32-column image, hi and mid
__device__ __forceinline__ void stage_cols_S(uint32_t st, int s, float v0, float v1, float v2, float v3) {
  const float v[4] = {v0, v1, v2, v3};
  trs::bf16x4 hi, mid;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const __bf16 hh = (__bf16)v[c];
    hi[c] = hh;
    mid[c] = (__bf16)(v[c] - (float)hh);
  }
  trs::store_slot(st, s, 0, hi);
  trs::store_slot(st, s, ImgS::PART_B, mid);
}
// acc[Ti][Tj] += A^T B over the 32 samples of the half, bf16 x 3: A / B images with 64 / (32 NJ) columns,
// rdA / rdB = image address + read_base(lane): k index 8 h + j of k-step ks = sample 16 ks + 8 h + j.
// (`cols_b` columns of B are real: lanes beyond them read like the others and feed zeros)
template <int NJ>
__device__ __forceinline__ void gemm_samples_T(f32x16 (&acc0)[NJ], f32x16 (&acc1)[NJ], uint32_t rdA,
                                               uint32_t rdB, int cols_b, int l31) {
  constexpr int CB = 32 * NJ;
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.0f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8 ah[2], am[2], bh[NJ], bm[NJ];
#pragma unroll
    for (int Ti = 0; Ti < 2; ++Ti) {
      ah[Ti] = trs::frag_tr<64>(rdA, ks, Ti);
      am[Ti] = trs::frag_tr<64>(rdA, ks, Ti, ImgU::PART_B);
    }
#pragma unroll
    for (int Tj = 0; Tj < NJ; ++Tj) {
      const bool real = 32 * Tj + l31 < cols_b;
      const bf16x8 vh = trs::frag_tr<CB>(rdB, ks, Tj), vm = trs::frag_tr<CB>(rdB, ks, Tj, trs::Img<CB>::PART_B);
      bh[Tj] = real ? vh : z;
      bm[Tj] = real ? vm : z;
    }
#pragma unroll
    for (int Tj = 0; Tj < NJ; ++Tj) {
      acc0[Tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[0], bh[Tj], acc0[Tj], 0, 0, 0);
      acc1[Tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[1], bh[Tj], acc1[Tj], 0, 0, 0);
      acc0[Tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[0], bm[Tj], acc0[Tj], 0, 0, 0);
      acc1[Tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[1], bm[Tj], acc1[Tj], 0, 0, 0);
      acc0[Tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[0], bh[Tj], acc0[Tj], 0, 0, 0);
      acc1[Tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[1], bh[Tj], acc1[Tj], 0, 0, 0);
    }
  }
}

// SHADE (backward): the gradient of the input row is not stored as (n,16) but pulled back through
// cat / normalize right here (what shade_prep_bwd_kernel did in a separate launch):
//   d_feature[s] = d_x[0:13];  dn = d_x[13:16] + d_normal[s];  d_grad[s] = (dn - n (n.dn)) / |grad|
struct ShadeOut {
  const float* d_normal;  // (n,3) from the compositing backward
  float* d_grad;          // (n,3)
  float* d_feature;       // (n + tail,13): rows n .. n + tail - 1 are set to zero (points that are
  int64_t tail;           // not ray samples: the regulariser points of the same geometry launch)
};

// a value every lane of the wave holds alike, moved to scalar registers (loop bounds read from LDS)
__device__ __forceinline__ int64_t dsu_uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// d_grad of sample si from the gradient (d0, d1, d2) of its normal, d_normal added: normalize's backward
__device__ __forceinline__ void shade_grad_out(const ShadeIn& sh, const ShadeOut& so, int64_t si,
                                               float d0, float d1, float d2) {
  const float g0 = sh.grad[si * 3], g1 = sh.grad[si * 3 + 1], g2 = sh.grad[si * 3 + 2];
  const float len = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
  const float inv = 1.0f / fmaxf(len, 1e-12f);
  const float n0 = g0 * inv, n1 = g1 * inv, n2 = g2 * inv;
  if (so.d_normal) {
    d0 += so.d_normal[si * 3]; d1 += so.d_normal[si * 3 + 1]; d2 += so.d_normal[si * 3 + 2];
  }
  const float dot = n0 * d0 + n1 * d1 + n2 * d2;
  const bool ok = len > 1e-12f;
  so.d_grad[si * 3] = ok ? (d0 - n0 * dot) * inv : d0 * inv;
  so.d_grad[si * 3 + 1] = ok ? (d1 - n1 * dot) * inv : d1 * inv;
  so.d_grad[si * 3 + 2] = ok ? (d2 - n2 * dot) * inv : d2 * inv;
}

// the rows of a sample in a dead half: what the live path writes for dIn = 0
template <bool SHADE>
__device__ __forceinline__ void dead_sample_out(const ShadeIn& sh, const ShadeOut& so, float* __restrict__ d_x,
                                                int64_t i) {
  if (SHADE) {
#pragma unroll
    for (int k = 0; k < 13; ++k) so.d_feature[i * 13 + k] = 0.0f;
    shade_grad_out(sh, so, i, 0.0f, 0.0f, 0.0f);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(d_x + i * TIN + 4 * q) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// One bit per 32-sample half: some d_rgb of the half is not zero.  What the compositing backward of the
// NSR step fills on its way (nsr_render.hip); the stand-alone entry points launch this in front of the
// backward kernel.  One 1024-thread workgroup = one word: no atomics on memory, nothing to clear.
__global__ __launch_bounds__(1024) void texture_live_kernel(const float* __restrict__ d_rgb, int64_t n,
                                                            uint32_t* __restrict__ live_halves) {
  __shared__ uint32_t word;
  if (threadIdx.x == 0) word = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  const bool lit = i < n && (d_rgb[i * 3] != 0.0f || d_rgb[i * 3 + 1] != 0.0f || d_rgb[i * 3 + 2] != 0.0f);
  const uint64_t m = __ballot(lit);
  if ((threadIdx.x & 63) == 0) {
    const uint32_t two = ((uint32_t)m != 0u ? 1u : 0u) | ((uint32_t)(m >> 32) != 0u ? 2u : 0u);
    if (two) atomicOr(&word, two << (2 * (threadIdx.x >> 6)));
  }
  __syncthreads();
  if (threadIdx.x == 0) live_halves[blockIdx.x] = word;
}

// DEAD HALVES.  A 32-sample half whose d_rgb rows are all zero (samples behind the front surface: the
// f32 transmittance has underflowed, w = 0 and d_rgb = w dc = 0 exactly) has dz = 0, hence dPre1, dH0,
// dPre0, dIn and its share of every parameter gradient exactly zero: it is not recomputed, staged or
// multiplied — its d_feature rows are written as zeros and its d_grad from d_normal alone, by a sweep of
// the whole grid over the dead halves in front of the waves' walks.  Work is handed out by the live halves
// (tex_partition.h, live_halves = one bit per half): a workgroup, and each of its waves, takes a
// contiguous run of halves with an equal share of the live ones.  The BIT decides what is dead: a set
// bit on a half of zeros only costs its time (the live path computes the same zeros), a clear bit on a
// half with a colour gradient would lose it — both producers set the bit of every such half.  Rays the
// colour loss gives no gradient (dc = 0) are dead from end to end, as are the samples behind the surface:
// three halves of four in the bench's fits (profiles/texture_dead_halves_share.txt).  Without a bitmap (n beyond
// texpart::MAX_WORDS x 1024 samples, which the LDS scan does not hold) the runs are the static ones:
// equal numbers of halves per workgroup and wave, and a wave finds its dead halves by a ballot over the
// d_rgb it has just loaded and writes their rows itself.
template <bool SHADE, bool L1_MASK = false>
__global__ __launch_bounds__(256) void texture_bwd_kernel(
    dsu_tex_mlp m, const float* __restrict__ x, ShadeIn sh, ShadeOut so,
    const float* __restrict__ rgb, const float* __restrict__ d_rgb, int64_t n,
    float* __restrict__ d_x, float* __restrict__ partials,
    const uint32_t* __restrict__ h1_mask, const uint32_t* __restrict__ live_halves) {
  extern __shared__ __attribute__((aligned(128))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
  // The kernel is written for one wave per SIMD and is to HAVE the SIMD (nsr_driver.hip: the ray marcher of
  // the side stream beside it delays its last workgroups).  The compiler needs 464 registers here, which would
  // leave the 48 a marching wave takes; the kernel before needed 474, an allocation of 480, which does not.
  // Naming accumulation register 223 keeps the allocation at 480 whatever the compiler needs (the effect of
  // 464 on the step has not been measured).
  asm volatile("" ::: "a223");
  // ---- dead halves: the bitmap and its scan (live halves before every word) in an LDS area of their own
  const int64_t halves = (n + 31) / 32;
  const bool scanned = live_halves != nullptr && halves <= 32 * (int64_t)texpart::MAX_WORDS;   // (per launch)
  uint32_t* sbits = reinterpret_cast<uint32_t*>(lds + L_SCAN);
  uint32_t* spre = sbits + texpart::MAX_WORDS;
  const int words = scanned ? (int)((halves + 31) / 32) : 0;
  for (int w = threadIdx.x; w < words; w += blockDim.x)
    sbits[w] = texpart::clip_word(live_halves[w], w, (int)halves);
  // the wave's images X, Y, S (tr_stage.h) as LDS byte addresses: st* = where the lane stores the row
  // of the sample in its column (X, Y: its lane half's unit quad), rd* = where it reads the fragments,
  // colY = where it reads the column `lane` of Y
  const uint32_t stg = trs::lds_addr(lds + L_STAGE + wave * STAGE_F);
  const uint32_t stX = stg + SB_X + (ImgU::store_base(l31) ^ (8 * h)), stY = stX + (SB_Y - SB_X);
  const uint32_t stS = stg + SB_S + ImgS::store_base(l31);
  const uint32_t rdX = stg + SB_X + ImgU::read_base(lane), rdY = rdX + (SB_Y - SB_X);
  const uint32_t rdS = stg + SB_S + ImgS::read_base(lane);
  const uint32_t colY = stg + SB_Y + ImgU::col_base(lane);
  load_weights(lds, m);
  __syncthreads();
  if (scanned && wave == 0) {     // a chunk of words per lane, scan over the lanes; the other waves start on the images
    const int chunk = (words + 63) / 64, w0 = lane * chunk;
    int sum = 0;
    for (int k = 0; k < chunk; ++k)
      if (w0 + k < words) sum += __popc(sbits[w0 + k]);
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    int before = incl - sum;
    for (int k = 0; k < chunk; ++k)
      if (w0 + k < words) {
        spre[w0 + k] = (uint32_t)before;
        before += __popc(sbits[w0 + k]);
      }
    if (lane == 63) spre[words] = (uint32_t)incl;
  }
  {   // bf16 hi / mid fragments of W1 and W0 in the order the backward MFMAs consume them
    bf16x8* img1 = reinterpret_cast<bf16x8*>(lds + L_IMG1);
    bf16x8* img0 = reinterpret_cast<bf16x8*>(lds + L_IMG0);
    for (int f = threadIdx.x; f < 8 * 64; f += blockDim.x) {
      const int ln = f & 63, c = f >> 6, g = c & 1, Tin = (c >> 1) & 1, To = c >> 2;
      float w[8];
#pragma unroll
      for (int t = 0; t < 8; ++t)
        w[t] = lds[L_W1 + feat_of(Tin, 8 * g + t, ln >> 5) * W1_ROW + 32 * To + (ln & 31)];
      bf16_split8(w, img1[f], img1[8 * 64 + f]);
    }
    for (int f = threadIdx.x; f < 4 * 64; f += blockDim.x) {
      const int ln = f & 63, c = f >> 6, g = c & 1, T = c >> 1;
      float w[8];
#pragma unroll
      for (int t = 0; t < 8; ++t)
        w[t] = (ln & 31) < TIN ? lds[L_W0 + feat_of(T, 8 * g + t, ln >> 5) * W0_ROW + (ln & 31)] : 0.0f;
      bf16_split8(w, img0[f], img0[4 * 64 + f]);
    }
    if constexpr (L1_MASK) {
      bf16x8* imgf = reinterpret_cast<bf16x8*>(lds + L_IMGF);
      for (int f = threadIdx.x; f < 8 * 64; f += blockDim.x) {
        const int ln = f & 63, c = f >> 6, g = c & 1, Tin = (c >> 1) & 1, To = c >> 2;
        float w[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)
          w[t] = lds[L_W1 + (32 * To + (ln & 31)) * W1_ROW + feat_of(Tin, 8 * g + t, ln >> 5)];
        bf16_split8(w, imgf[f], imgf[8 * 64 + f]);
      }
    }
  }
  __syncthreads();

  if (SHADE) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < so.tail * 13;
         t += (int64_t)gridDim.x * blockDim.x)
      so.d_feature[n * 13 + t] = 0.0f;
  }
  f32x16 gw1[2][2], gw0[2], gw2[2];     // D[i = row unit][j]: W1[i][j], W0[i][k | bias], W2^T[i][o]
  float gb1row = 0.0f;                 // gb1[unit = lane]: row sums of the transposed dPre1 image (see gW1)
  float gb2[TOUT] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      gw1[T][0][r] = gw1[T][1][r] = 0.0f;
      gw0[T][r] = gw2[T][r] = 0.0f;
    }

  // ---- the dead halves' rows, by all threads of the grid side by side: independent iterations, where the
  // walk below is one chain of memory latencies per 64 samples for a single wave per SIMD — as part of that
  // walk the longest stretch of dead rays (tens of halves) set the kernel's time: 104 instead of 70 us
  if (scanned) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
      const int64_t hf = t >> 5;
      if (!((sbits[hf >> 5] >> (hf & 31)) & 1u)) dead_sample_out<SHADE>(sh, so, d_x, t);
    }
  }
  // ---- the wave's run of halves [wh0, wh1)
  int64_t wh0, wh1;
  if (scanned) {
    const texpart::Scan sc{sbits, spre, words, (int)halves};
    const texpart::Run wg = texpart::split(sc, texpart::whole(sc), (int)gridDim.x, (int)blockIdx.x);
    const texpart::Run wr = texpart::split(sc, wg, 4, wave);
    wh0 = wr.h0; wh1 = wr.h1;
  } else {
    const int64_t per = (halves + gridDim.x - 1) / gridDim.x;
    const int64_t b0 = blockIdx.x * per < halves ? blockIdx.x * per : halves;
    const int64_t len = (b0 + per < halves ? b0 + per : halves) - b0;
    wh0 = b0 + wave * len / 4; wh1 = b0 + (wave + 1) * len / 4;
  }
  // the wave's samples [32 wh0, r1), 64 per iteration (wave-uniform bounds, no workgroup barrier in the loop)
  const int64_t r0 = 32 * dsu_uniform64(wh0);
  const int64_t r1 = 32 * dsu_uniform64(wh1) < n ? 32 * dsu_uniform64(wh1) : n;
  for (int64_t wave_first = r0; wave_first < r1; wave_first += 64) {
    const int64_t i = wave_first + lane;
    const bool valid = i < r1;
    const int64_t ii = valid ? i : r1 - 1;
    // which of the two halves carry a colour gradient at all: the bitmap says so before anything is loaded
    // (their rows are written by the sweep above); without a bitmap, a ballot over the d_rgb just loaded
    bool live0 = true, live1 = true;
    if (scanned) {
      const int64_t hf = wave_first >> 5;
      const uint32_t b0 = sbits[hf >> 5] >> (hf & 31), b1 = hf + 1 < halves ? sbits[(hf + 1) >> 5] >> ((hf + 1) & 31) : 0u;
      live0 = (__builtin_amdgcn_readfirstlane(b0) & 1u) != 0u;
      live1 = (__builtin_amdgcn_readfirstlane(b1) & 1u) != 0u;
      if (!live0 && !live1) continue;
    }
    float dr[TOUT];
#pragma unroll
    for (int o = 0; o < TOUT; ++o) dr[o] = d_rgb[ii * TOUT + o];
    if (!scanned) {
      const uint64_t lit = __ballot(valid && (dr[0] != 0.0f || dr[1] != 0.0f || dr[2] != 0.0f));
      live0 = (uint32_t)lit != 0u;
      live1 = (uint32_t)(lit >> 32) != 0u;
      if (valid && !(h ? live1 : live0)) dead_sample_out<SHADE>(sh, so, d_x, i);
      if (lit == 0ull) continue;
    }
    float in[TIN];
    if (SHADE) {
      float inv_len;
      load_shaded(sh, ii, in, inv_len);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(x + ii * TIN + 4 * q);
        in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
      }
    }
    // gradient on the pre-sigmoid outputs of the lane's own sample (0 for padding lanes)
    float dz[TOUT];
#pragma unroll
    for (int o = 0; o < TOUT; ++o) {
      const float s = rgb[ii * TOUT + o];
      dz[o] = valid ? dr[o] * s * (1.0f - s) : 0.0f;
      gb2[o] += dz[o];
    }
    uint32_t mk2[2] = {0u, 0u};         // layer 1's ReLU pattern of the samples in column l31 of both halves
    if constexpr (L1_MASK) {
#pragma unroll
      for (int a_ = 0; a_ < 2; ++a_) {
        int64_t si = wave_first + a_ * 32 + l31;
        si = si < r1 ? si : r1 - 1;
        mk2[a_] = h1_mask[si * 2 + h];
      }
    }
#pragma unroll 1
    for (int a = 0; a < 2; ++a) {
      if (wave_first + a * 32 >= r1 || !(a ? live1 : live0)) continue;
      f32x16 H0[2], H1[2];
      forward_half<L1_MASK>(lds, in, a, l31, h, H0, H1);
      const uint32_t mk = a ? mk2[1] : mk2[0];
      if constexpr (L1_MASK) {
        // the forward's pattern decides which units are live; the bf16 x 3 recompute only supplies
        // their values (2^-16 relative)
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
          for (int r = 0; r < 16; ++r) H1[T][r] = ((mk >> (16 * T + r)) & 1u) ? H1[T][r] : 0.0f;
      }
      // dz of the samples of half a, in every lane of the pair
      float dza[TOUT];
#pragma unroll
      for (int o = 0; o < TOUT; ++o) {
        const float other = __shfl_xor(dz[o], 32);
        dza[o] = h == a ? dz[o] : other;
      }
      // dPre1 = (W2^T dz) * relu'(H1)
      f32x16 D1[2];
#pragma unroll
      for (int T = 0; T < 2; ++T)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = 0.0f;
#pragma unroll
          for (int o = 0; o < TOUT; ++o)
            v = fmaf(lds[L_W2P + (h * TOUT + o) * 32 + T * 16 + r], dza[o], v);
          D1[T][r] = (L1_MASK ? ((mk >> (16 * T + r)) & 1u) != 0u : H1[T][r] > 0.0f) ? v : 0.0f;
        }
      // ---- gW2^T[unit][o] += sum_samples H1[sample][unit] * dz[sample][o]
      // bf16 x 3 on v_mfma_f32_32x32x16_bf16 (K = 16 samples per MFMA): H1 and dz go to LDS as
      // [sample][unit] images (bf16 hi / mid, packed 8-byte stores), and a lane's operand fragment —
      // 8 consecutive samples of one unit — comes back through two transposing reads.
      // 12 MFMAs of 32 clocks instead of 32 of 64.
      __builtin_amdgcn_wave_barrier();
      stage_units_T(stX, H1);
      if (h == a) stage_cols_S(stS, 0, dz[0], dz[1], dz[2], 0.0f);
      __builtin_amdgcn_wave_barrier();
      {
        f32x16 (&g0)[1] = *reinterpret_cast<f32x16 (*)[1]>(&gw2[0]);
        f32x16 (&g1)[1] = *reinterpret_cast<f32x16 (*)[1]>(&gw2[1]);
        gemm_samples_T<1>(g0, g1, rdX, rdS, TOUT, l31);
      }
      // ---- gW1[i][j] += sum_samples dPre1[sample][i] * H0[sample][j]
      __builtin_amdgcn_wave_barrier();           // (the gW2 reads of X are done: in-order LDS queue of the wave)
      stage_units_T(stY, D1);
      stage_units_T(stX, H0);
      __builtin_amdgcn_wave_barrier();
      {   // gb1[unit] += sum over the half's samples of dPre1: lane u adds up column u of the image it was
          // just staged into (hi + mid: 2^-16 relative, like the products), samples 0 .. 31 in order — one
          // accumulator per lane instead of 32 per-column partial sums
        float srow = 0.0f;
#pragma unroll
        for (int P0 = 0; P0 < 32; P0 += 4) {
          const uint32_t a4 = (colY ^ (uint32_t)ImgU::col_xor(P0)) + P0 * ImgU::ROW_B;
          const trs::bf16x4 vh = trs::read_tr(a4), vm = trs::read_tr(a4 + ImgU::PART_B);
#pragma unroll
          for (int e = 0; e < 4; ++e) srow += (float)vh[e] + (float)vm[e];
        }
        gb1row += srow;
      }
      gemm_samples_T<2>(gw1[0], gw1[1], rdY, rdX, 64, l31);   // 24 MFMAs instead of 64
      // ---- dH0^T = W1^T . dPre1^T, then dPre0 = dH0 * relu'(H0)
      f32x16 D0[2];
#pragma unroll
      for (int T = 0; T < 2; ++T)
#pragma unroll
        for (int r = 0; r < 16; ++r) D0[T][r] = 0.0f;
      {   // on the bf16 matrix pipe (bf16 x 3): registers 8 g + t of a lane's dPre1 accumulator hold
          // units feat_of(Tin, 8 g + t, h) of ITS sample — the B operand of one
          // v_mfma_f32_32x32x16_bf16 as they stand; the A fragment is W1 in the same order (image
          // above).  2 x 2 x 2 x 3 = 24 MFMAs of 32 clocks instead of 64 of 64.
        const bf16x8* img1 = reinterpret_cast<const bf16x8*>(lds + L_IMG1);
        bf16x8 bh[2][2], bm[2][2];
#pragma unroll
        for (int Tin = 0; Tin < 2; ++Tin)
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            float v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = D1[Tin][8 * g + t];
            bf16_split8(v, bh[Tin][g], bm[Tin][g]);
          }
#pragma unroll
        for (int To = 0; To < 2; ++To)
#pragma unroll
          for (int Tin = 0; Tin < 2; ++Tin)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
              const int f = ((To * 2 + Tin) * 2 + g) * 64 + lane;
              const bf16x8 ah = img1[f], am = img1[8 * 64 + f];
              D0[To] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[Tin][g], D0[To], 0, 0, 0);
              D0[To] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm[Tin][g], D0[To], 0, 0, 0);
              D0[To] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh[Tin][g], D0[To], 0, 0, 0);
            }
      }
#pragma unroll
      for (int T = 0; T < 2; ++T)
#pragma unroll
        for (int r = 0; r < 16; ++r) D0[T][r] = H0[T][r] > 0.0f ? D0[T][r] : 0.0f;
      // ---- gW0[i][k] += sum_samples dPre0[sample][i] * In[sample][k]  (k = 16: ones -> gb0)
      __builtin_amdgcn_wave_barrier();
      stage_units_T(stY, D0);
      if (h == a) {
#pragma unroll
        for (int s = 0; s < TIN / 4; ++s) stage_cols_S(stS, s, in[4 * s], in[4 * s + 1], in[4 * s + 2], in[4 * s + 3]);
        stage_cols_S(stS, TIN / 4, 1.0f, 0.0f, 0.0f, 0.0f);  // the ones column -> gb0
      }
      __builtin_amdgcn_wave_barrier();
      {
        f32x16 (&g0)[1] = *reinterpret_cast<f32x16 (*)[1]>(&gw0[0]);
        f32x16 (&g1)[1] = *reinterpret_cast<f32x16 (*)[1]>(&gw0[1]);
        gemm_samples_T<1>(g0, g1, rdY, rdS, TIN + 1, l31);   // 12 MFMAs instead of 32
      }
      // ---- dIn^T = W0^T . dPre0^T : row k = (r&3) + 8(r>>2) + 4h of the sample in column l31
      f32x16 din;
#pragma unroll
      for (int r = 0; r < 16; ++r) din[r] = 0.0f;
      {   // bf16 x 3 as above: 2 x 2 x 3 = 12 MFMAs instead of 32
        const bf16x8* img0 = reinterpret_cast<const bf16x8*>(lds + L_IMG0);
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            float v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = D0[T][8 * g + t];
            bf16x8 bh, bm;
            bf16_split8(v, bh, bm);
            const int f = (T * 2 + g) * 64 + lane;
            const bf16x8 ah = img0[f], am = img0[4 * 64 + f];
            din = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, din, 0, 0, 0);
            din = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, din, 0, 0, 0);
            din = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, din, 0, 0, 0);
          }
      }
      const int64_t si = wave_first + a * 32 + l31;              // the sample of column l31
      if (si < r1) {
        if (SHADE) {
          // lane h holds components 8q + 4h + {0..3}: h = 0 -> 0-3, 8-11; h = 1 -> 4-7, 12-15
#pragma unroll
          for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int comp = 8 * q + 4 * h + e;
              if (comp < 13) so.d_feature[si * 13 + comp] = din[4 * q + e];
            }
          if (h == 1) shade_grad_out(sh, so, si, din[5], din[6], din[7]);   // components 13, 14, 15
        } else {
#pragma unroll
          for (int q = 0; q < 2; ++q)
            *reinterpret_cast<float4*>(d_x + si * TIN + 8 * q + 4 * h) =
                make_float4(din[4 * q], din[4 * q + 1], din[4 * q + 2], din[4 * q + 3]);
        }
      }
    }
  }

  // ---- workgroup reduction of the parameter-gradient tiles -> one partial vector per workgroup.
  // Every wave stores its tiles into an image of its own, one barrier, then all 256 threads sum the
  // four images element by element (fixed order) and write the partial vector.  The first form added
  // all four waves' tiles into ONE image with LDS float atomics (160 per lane, every address hit by
  // all four waves): 112 k of the kernel's 332 k clocks per wave (phase clocks,
  // profiles/round6_texture_phase_clocks.txt).  The whole LDS is free here.
  __syncthreads();
  static_assert(4 * PART_STRIDE <= BWD_LDS_F, "four partial images fit the kernel's LDS");
  float gb2s[TOUT];
#pragma unroll
  for (int o = 0; o < TOUT; ++o) {
    float s_ = gb2[o];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) s_ += __shfl_xor(s_, k);
    gb2s[o] = s_;
  }
  auto store_own = [&](float* dst) {
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = feat_of(T, r, h);
        dst[P_GW1 + row * 64 + l31] = gw1[T][0][r];
        dst[P_GW1 + row * 64 + 32 + l31] = gw1[T][1][r];
        dst[P_GW0 + row * 32 + l31] = gw0[T][r];
        dst[P_GW2 + row * 32 + l31] = gw2[T][r];
      }
    dst[P_GB1 + lane] = gb1row;
    if (lane == 0) {
#pragma unroll
      for (int o = 0; o < TOUT; ++o) dst[P_GB2 + o] = gb2s[o];
    }
  };
  store_own(lds + wave * PART_STRIDE);
  __syncthreads();
  float* part = partials + (size_t)blockIdx.x * PART_STRIDE;
  for (int v = threadIdx.x; v < PART_N; v += blockDim.x)
    part[v] = (lds[v] + lds[PART_STRIDE + v]) + (lds[2 * PART_STRIDE + v] + lds[3 * PART_STRIDE + v]);
}

__global__ void texture_reduce_kernel(const float* __restrict__ partials, int nblocks,
                                      float* __restrict__ g_w0, float* __restrict__ g_b0,
                                      float* __restrict__ g_w1, float* __restrict__ g_b1,
                                      float* __restrict__ g_w2, float* __restrict__ g_b2) {
  // 64 elements x 16 slices of the workgroup range per 1024-thread workgroup
  __shared__ float red[16][64];
  const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int v = blockIdx.x * 64 + e;
  const bool in_range = v < PART_N;
  float acc = 0.0f;
  if (in_range)
    for (int b = sl; b < nblocks; b += 16) acc += partials[(size_t)b * PART_STRIDE + v];
  red[sl][e] = acc;
  __syncthreads();
  if (sl != 0 || !in_range) return;
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += red[k][e];
  if (v < P_GW0) {
    g_w1[v] += s;                                   // [i][j] row-major = W1's layout
  } else if (v < P_GW2) {
    const int i = (v - P_GW0) >> 5, k = (v - P_GW0) & 31;
    if (k < TIN) g_w0[i * TIN + k] += s;
    else if (k == TIN) g_b0[i] += s;
  } else if (v < P_GB1) {
    const int i = (v - P_GW2) >> 5, o = (v - P_GW2) & 31;
    if (o < TOUT) g_w2[o * THID + i] += s;
  } else if (v < P_GB2) {
    g_b1[v - P_GB1] += s;
  } else {
    g_b2[v - P_GB2] += s;
  }
}

// words of the liveness bitmap of n samples: 32 halves of 32 samples each
int64_t live_words(int64_t n) { return (n + 1023) / 1024; }

bool mlp_ok(const dsu_tex_mlp* m) {
  return m && m->w0 && m->b0 && m->w1 && m->b1 && m->w2 && m->b2;
}

// One launch of texture_bwd_kernel<SHADE, L1_MASK> for n > 0 validated samples: workspace check, one
// workgroup per CU it is given, the whole dynamic LDS.  A template and not a run-time branch:
// DSU_ENSURE_DYN_LDS keeps its high-water mark per expansion, i.e. per kernel instantiation.
// The caller checks the launch; *blocks is the number of partial vectors left in the workspace.
// live: the liveness bitmap of the halves (see DEAD HALVES above); null = found here from d_rgb, into
// the words behind the partial vectors of the workspace.
template <bool SHADE, bool L1_MASK>
int launch_bwd(const dsu_tex_mlp* mlp, const float* x, ShadeIn sh, ShadeOut so, const float* rgb,
               const float* d_rgb, int64_t n, float* d_x, const uint32_t* h1_mask, const uint32_t* live,
               void* workspace, int64_t workspace_bytes, hipStream_t s, int* blocks) {
  if (!workspace || workspace_bytes < dsu_texture_bwd_workspace_bytes(n)) return DSU_EINVAL;
  *blocks = dsu_onewave_blocks(n, 256, TEX_MAX_BLOCKS, 1);
  const int64_t words = live_words(n);
  if (words > texpart::MAX_WORDS) {
    live = nullptr;                                  // the kernel's static ranges
  } else if (!live) {
    uint32_t* own = reinterpret_cast<uint32_t*>((float*)workspace +
                                                (size_t)dsu_capped_blocks(n, 256, TEX_MAX_BLOCKS) * PART_STRIDE);
    texture_live_kernel<<<(unsigned)words, 1024, 0, s>>>(d_rgb, n, own);
    live = own;
  }
  const size_t shm = (size_t)BWD_LDS_ALL_F * sizeof(float);
  DSU_ENSURE_DYN_LDS((texture_bwd_kernel<SHADE, L1_MASK>), shm);
  texture_bwd_kernel<SHADE, L1_MASK><<<*blocks, 256, shm, s>>>(*mlp, x, sh, so, rgb, d_rgb, n, d_x,
                                                              (float*)workspace, h1_mask, live);
  return DSU_OK;
}

void launch_reduce(const void* workspace, int blocks, float* g_w0, float* g_b0, float* g_w1,
                   float* g_b1, float* g_w2, float* g_b2, hipStream_t s) {
  texture_reduce_kernel<<<(PART_N + 63) / 64, 1024, 0, s>>>((const float*)workspace, blocks, g_w0,
                                                           g_b0, g_w1, g_b1, g_w2, g_b2);
}

}  // namespace

extern "C" {

int dsu_texture_fwd(const dsu_tex_mlp* mlp, const float* tex_in, int64_t n, float* rgb,
                    void* stream) {
  if (!mlp_ok(mlp) || n < 0 || (n && (!tex_in || !rgb))) return DSU_EINVAL;
  if (n == 0) return DSU_OK;
  texture_fwd_kernel<false><<<dsu_capped_blocks(n, 256, 2048), 256, 0, (hipStream_t)stream>>>(
      *mlp, tex_in, ShadeIn{nullptr, nullptr}, nullptr, n, rgb, nullptr);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_texture_fwd_shaded_m(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                             int64_t n, float* normal, float* rgb, uint32_t* h1_mask, void* stream) {
  if (!mlp_ok(mlp) || n < 0 || (n && (!feature || !grad || !normal || !rgb))) return DSU_EINVAL;
  if (n == 0) return DSU_OK;
  texture_fwd_kernel<true><<<dsu_capped_blocks(n, 256, 2048), 256, 0, (hipStream_t)stream>>>(
      *mlp, nullptr, ShadeIn{feature, grad}, normal, n, rgb, h1_mask);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int64_t dsu_texture_bwd_workspace_bytes(int64_t n) {
  if (n < 0) return DSU_EINVAL;
  // the partial vectors, then the liveness bitmap the stand-alone entry points build (launch_bwd)
  const int64_t words = live_words(n) <= texpart::MAX_WORDS ? live_words(n) : 0;
  return ((int64_t)dsu_capped_blocks(n, 256, TEX_MAX_BLOCKS) * PART_STRIDE + words) * (int64_t)sizeof(float);
}

int dsu_texture_bwd(const dsu_tex_mlp* mlp, const float* tex_in, const float* rgb,
                    const float* d_rgb, int64_t n, float* d_tex_in, float* g_w0, float* g_b0,
                    float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  if (!mlp_ok(mlp) || n < 0) return DSU_EINVAL;
  if (!g_w0 || !g_b0 || !g_w1 || !g_b1 || !g_w2 || !g_b2) return DSU_EINVAL;
  if (n && (!tex_in || !rgb || !d_rgb || !d_tex_in)) return DSU_EINVAL;
  if (n == 0) return DSU_OK;
  int blocks;
  const int rc = launch_bwd<false, false>(mlp, tex_in, ShadeIn{nullptr, nullptr},
                                          ShadeOut{nullptr, nullptr, nullptr, 0}, rgb, d_rgb, n, d_tex_in,
                                          nullptr, nullptr, workspace, workspace_bytes, (hipStream_t)stream,
                                          &blocks);
  if (rc != DSU_OK) return rc;
  launch_reduce(workspace, blocks, g_w0, g_b0, g_w1, g_b1, g_w2, g_b2, (hipStream_t)stream);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_texture_bwd_shaded(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                           const float* rgb, const float* d_rgb, const float* d_normal, int64_t n,
                           int64_t tail_rows, float* d_grad, float* d_feature, float* g_w0,
                           float* g_b0, float* g_w1,
                           float* g_b1, float* g_w2, float* g_b2, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  if (!mlp_ok(mlp) || n < 0) return DSU_EINVAL;
  if (!g_w0 || !g_b0 || !g_w1 || !g_b1 || !g_w2 || !g_b2) return DSU_EINVAL;
  if (tail_rows < 0 || (n && (!feature || !grad || !rgb || !d_rgb || !d_grad || !d_feature)))
    return DSU_EINVAL;
  if (n == 0) return DSU_EUNSUP;                    // the caller zeroes the tail itself
  int blocks;
  const int rc = launch_bwd<true, false>(mlp, nullptr, ShadeIn{feature, grad},
                                         ShadeOut{d_normal, d_grad, d_feature, tail_rows}, rgb, d_rgb, n,
                                         nullptr, nullptr, nullptr, workspace, workspace_bytes,
                                         (hipStream_t)stream, &blocks);
  if (rc != DSU_OK) return rc;
  launch_reduce(workspace, blocks, g_w0, g_b0, g_w1, g_b1, g_w2, g_b2, (hipStream_t)stream);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int32_t dsu_texture_partial_map(int32_t* map_host) {
  if (map_host) {
    // offsets into one contiguous gradient block [w0 (64,16) | b0 | w1 (64,64) | b1 | w2 (3,64) | b2]
    constexpr int O_W0 = 0, O_B0 = THID * TIN, O_W1 = O_B0 + THID, O_B1 = O_W1 + THID * THID,
                  O_W2 = O_B1 + THID, O_B2 = O_W2 + TOUT * THID;
    for (int v = 0; v < PART_N; ++v) {
      int d = -1;
      if (v < P_GW0) {
        d = O_W1 + v;
      } else if (v < P_GW2) {
        const int i = (v - P_GW0) >> 5, k = (v - P_GW0) & 31;
        if (k < TIN) d = O_W0 + i * TIN + k;
        else if (k == TIN) d = O_B0 + i;
      } else if (v < P_GB1) {
        const int i = (v - P_GW2) >> 5, o = (v - P_GW2) & 31;
        if (o < TOUT) d = O_W2 + o * THID + i;
      } else if (v < P_GB2) {
        d = O_B1 + (v - P_GB1);
      } else {
        d = O_B2 + (v - P_GB2);
      }
      map_host[v] = d;
    }
  }
  return PART_N;
}

static int shaded_partials(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                           const float* rgb, const float* d_rgb, const float* d_normal,
                           int64_t n, int64_t tail_rows, float* d_grad, float* d_feature,
                           const uint32_t* h1_mask, const uint32_t* live, void* workspace,
                           int64_t workspace_bytes, dsu_partial_reduce* red, void* stream) {
  if (!mlp_ok(mlp) || n < 0 || !red) return DSU_EINVAL;
  if (tail_rows < 0 || (n && (!feature || !grad || !rgb || !d_rgb || !d_grad || !d_feature)))
    return DSU_EINVAL;
  if (n == 0) return DSU_EUNSUP;                    // the caller zeroes the tail itself
  const ShadeIn sh{feature, grad};
  const ShadeOut so{d_normal, d_grad, d_feature, tail_rows};
  int blocks;
  const int rc = h1_mask ? launch_bwd<true, true>(mlp, nullptr, sh, so, rgb, d_rgb, n, nullptr, h1_mask, live,
                                                  workspace, workspace_bytes, (hipStream_t)stream, &blocks)
                         : launch_bwd<true, false>(mlp, nullptr, sh, so, rgb, d_rgb, n, nullptr, nullptr, live,
                                                   workspace, workspace_bytes, (hipStream_t)stream, &blocks);
  if (rc != DSU_OK) return rc;
  DSU_CHECK_LAUNCH();
  red->partials = (const float*)workspace;
  red->nblocks = blocks;
  red->stride = PART_STRIDE;
  red->n = PART_N;
  return DSU_OK;
}

int dsu_texture_bwd_shaded_partials_live(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                                         const float* rgb, const float* d_rgb, const float* d_normal,
                                         int64_t n, int64_t tail_rows, float* d_grad, float* d_feature,
                                         const uint32_t* h1_mask, const uint32_t* live_halves,
                                         void* workspace, int64_t workspace_bytes,
                                         dsu_partial_reduce* red, void* stream) {
  if (!live_halves) return DSU_EINVAL;
  return shaded_partials(mlp, feature, grad, rgb, d_rgb, d_normal, n, tail_rows, d_grad, d_feature, h1_mask,
                         live_halves, workspace, workspace_bytes, red, stream);
}

int dsu_texture_bwd_shaded_partials_m(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                                      const float* rgb, const float* d_rgb, const float* d_normal,
                                      int64_t n, int64_t tail_rows, float* d_grad, float* d_feature,
                                      const uint32_t* h1_mask, void* workspace, int64_t workspace_bytes,
                                      dsu_partial_reduce* red, void* stream) {
  return shaded_partials(mlp, feature, grad, rgb, d_rgb, d_normal, n, tail_rows, d_grad, d_feature, h1_mask,
                         nullptr, workspace, workspace_bytes, red, stream);
}

int dsu_texture_live_partition(const uint32_t* live_halves, int64_t n_halves, int32_t parts,
                               int32_t waves, int32_t* runs) {
  if (!live_halves || !runs || n_halves < 1 || parts < 1 || waves < 1) return DSU_EINVAL;
  const int64_t words = (n_halves + 31) / 32;
  if (words > texpart::MAX_WORDS) return DSU_EUNSUP;
  std::vector<uint32_t> bits((size_t)words), pre((size_t)words + 1);
  pre[0] = 0;
  for (int64_t w = 0; w < words; ++w) {
    bits[w] = texpart::clip_word(live_halves[w], (int)w, (int)n_halves);
    pre[w + 1] = pre[w] + (uint32_t)texpart::popc(bits[w]);
  }
  const texpart::Scan sc{bits.data(), pre.data(), (int)words, (int)n_halves};
  const texpart::Run all = texpart::whole(sc);
  for (int b = 0; b < parts; ++b) {
    const texpart::Run wg = texpart::split(sc, all, parts, b);
    for (int w = 0; w < waves; ++w) {
      const texpart::Run r = texpart::split(sc, wg, waves, w);
      runs[2 * (b * waves + w)] = r.h0;
      runs[2 * (b * waves + w) + 1] = r.h1;
    }
  }
  return DSU_OK;
}

}  // extern "C"
