// GroupNorm(+SiLU) on NHWC f16, LayerNorm, GEGLU for the diffusion UNet (K4 of SURVEY.md
// §2.3: the GroupNorm/SiLU/LayerNorm/GEGLU kernels the reference runs through diffusers'
// ResnetBlock2D (norm1/norm2 + nonlinearity), TransformerMV2DModel.norm
// (mvdiffusion/models/transformer_mv2d.py:304), BasicMVTransformerBlock.norm1/2/3/norm_joint_mid
// (:532-625) and FeedForward(GEGLU) (:483)).  All HBM-bound: every kernel reads its input once
// with 16-byte accesses and keeps statistics in f32; no variance is taken as E[x^2] - E[x]^2 of
// the raw values (GroupNorm: centred or shifted per kernel, see each; LayerNorm: centred).
#include "common.h"

namespace {

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- GroupNorm statistics: per (image, channel) partial sums over a slab of pixels, folded
// to per-(image, group) sum / sum-of-squares with one atomic pair per workgroup and group.
// Both sums are taken of x - K, K = gn_shift() being the group's own first element.  Sums of x and
// x*x lose mean^2/var of their digits (at mean 1000, std 2 the f32 result is noise and clamps to
// 0); the shifted ones lose (K - mean)^2/var instead, which is what the group's offset from zero
// no longer enters.  The limit: K is ONE element.  Tens of standard deviations from the mean cost
// a few hundred of f32's 1.7e7 and are harmless; an element thousands of standard deviations out,
// sitting exactly at pixel 0 of the group's first channel, would cancel as the raw sums did.
// out must not alias x: gn_apply_kernel reads K from x while other threads write out.
__device__ __forceinline__ float gn_shift(const f16* __restrict__ x, int n, int HW, int C, int cpg,
                                          int g) {
  return (float)x[(size_t)n * HW * C + g * cpg];
}

// grid = (pixel slabs, B); block = 256 threads; thread t owns 8-channel group (t % C8) of
// pixels t / C8, t / C8 + 256 / C8 ...   (C8 = C/8 <= 256)
__global__ __launch_bounds__(256) void gn_stats_kernel(const f16* __restrict__ x, int HW, int C,
                                                       int G, int pix_per_block,
                                                       float* __restrict__ stats /*(B,G,2)*/) {
  extern __shared__ float sh[];   // [2][C]
  const int n = blockIdx.y;
  const int C8 = C >> 3;
  const int nsplit = (C8 + 255) / 256;               // channel range split when C/8 > 256
  const int lanes_per_pix = C8 / nsplit;             // host guarantees divisibility
  const int pix_par = 256 / lanes_per_pix;           // pixels processed concurrently
  const int pl = threadIdx.x / lanes_per_pix;
  for (int i = threadIdx.x; i < 2 * C; i += 256) sh[i] = 0.0f;
  __syncthreads();
  const int p0 = blockIdx.x * pix_per_block;
  const int p1 = min(p0 + pix_per_block, HW);
  const int cpg = C / G;
  for (int sp = 0; sp < nsplit; ++sp) {
    const int cg = sp * lanes_per_pix + threadIdx.x % lanes_per_pix;
    float s[8], q[8], K[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.0f;
    if (pl < pix_par) {
#pragma unroll
      for (int e = 0; e < 8; ++e) K[e] = gn_shift(x, n, HW, C, cpg, (cg * 8 + e) / cpg);
      for (int p = p0 + pl; p < p1; p += pix_par) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(x + ((size_t)n * HW + p) * C + cg * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = (float)v[e] - K[e];
          s[e] += f;
          q[e] += f * f;
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        atomicAdd(&sh[cg * 8 + e], s[e]);
        atomicAdd(&sh[C + cg * 8 + e], q[e]);
      }
    }
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) {
    float ss = 0.0f, qq = 0.0f;
    for (int c = 0; c < cpg; ++c) {
      ss += sh[g * cpg + c];
      qq += sh[C + g * cpg + c];
    }
    unsafeAtomicAdd(&stats[((size_t)n * G + g) * 2], ss);
    unsafeAtomicAdd(&stats[((size_t)n * G + g) * 2 + 1], qq);
  }
}

__device__ __forceinline__ float silu(float v) { return v / (1.0f + __expf(-v)); }

__global__ __launch_bounds__(256) void gn_apply_kernel(const f16* __restrict__ x,
                                                       const float* __restrict__ stats,
                                                       const f16* __restrict__ gamma,
                                                       const f16* __restrict__ beta, int HW,
                                                       int C, int G, float eps, int do_silu,
                                                       int64_t total8, f16* __restrict__ out) {
  const int cpg = C / G;
  const float inv_cnt = 1.0f / ((float)HW * (float)cpg);
  const int C8 = C >> 3;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total8;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % C8) * 8;
    const int n = (int)(i / ((int64_t)C8 * HW));
    const f16x8 v = *reinterpret_cast<const f16x8*>(x + i * 8);
    const f16x8 gm = *reinterpret_cast<const f16x8*>(gamma + c0);
    const f16x8 bt = *reinterpret_cast<const f16x8*>(beta + c0);
    f16x8 o;
    int g_cur = -1;
    float mean = 0.0f, rstd = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int g = (c0 + e) / cpg;
      if (g != g_cur) {   // the shifted sums of gn_stats_kernel: mean = K + S/n, var = Q/n - (S/n)^2
        g_cur = g;
        const float ds = stats[((size_t)n * G + g) * 2] * inv_cnt;
        const float var = fmaxf(stats[((size_t)n * G + g) * 2 + 1] * inv_cnt - ds * ds, 0.0f);
        mean = gn_shift(x, n, HW, C, cpg, g) + ds;
        rstd = rsqrtf(var + eps);
      }
      float y = ((float)v[e] - mean) * rstd * (float)gm[e] + (float)bt[e];
      if (do_silu) y = silu(y);
      o[e] = (f16)y;
    }
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
  }
}

// ---- small tensors (every GroupNorm of the UNet): ONE launch, one workgroup per (image, group).
// The memset + statistics + apply sequence above costs three dependent launches (25-60 us of
// mostly launch latency on 0.1-6 MB tensors); here the group's HW x cpg elements (<= 64 KB, L2
// resident) are read twice by the same workgroup.  Variance: where the group's values stay in
// registers, the centred sum of (x - mean)^2 over them once the mean is known; where they are read
// a second time, the shifted sums of x - K as in gn_stats_kernel.
__global__ __launch_bounds__(256) void gn_fused_small_kernel(const f16* __restrict__ x,
                                                             const f16* __restrict__ gamma,
                                                             const f16* __restrict__ beta, int HW,
                                                             int C, int G, float eps, int do_silu,
                                                             f16* __restrict__ out) {
  // channels per group are even for every layer (10..80), so the group's rows are walked as
  // half2 pairs; up to GN_KEEP pairs per thread stay in registers between the two passes
  constexpr int GN_KEEP = 16;
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  __shared__ float red[3][4];
  const int n = blockIdx.x / G, g = blockIdx.x % G;
  const int cpg = C / G, cp2 = cpg >> 1;
  const int cnt2 = HW * cp2;
  const f16* xb = x + (size_t)n * HW * C + g * cpg;
  f16* ob = out + (size_t)n * HW * C + g * cpg;
  const bool keep = cnt2 <= GN_KEEP * 256;
  f16x2 kv[GN_KEEP];
  float s = 0.0f, q = 0.0f, shift = 0.0f;
  if (keep) {
#pragma unroll
    for (int k = 0; k < GN_KEEP; ++k) {
      const int e = threadIdx.x + 256 * k;
      f16x2 v;
      v[0] = (f16)0.0f; v[1] = (f16)0.0f;
      if (e < cnt2) {
        const int p = e / cp2, c = e - p * cp2;
        v = *reinterpret_cast<const f16x2*>(xb + (size_t)p * C + 2 * c);
      }
      kv[k] = v;
      s += (float)v[0] + (float)v[1];
    }
  } else {
    shift = (float)xb[0];
    for (int e = threadIdx.x; e < cnt2; e += 256) {
      const int p = e / cp2, c = e - p * cp2;
      const f16x2 v = *reinterpret_cast<const f16x2*>(xb + (size_t)p * C + 2 * c);
      const float f0 = (float)v[0] - shift, f1 = (float)v[1] - shift;
      s += f0 + f1;
      q += f0 * f0 + f1 * f1;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    q += __shfl_xor(q, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s;
    red[1][threadIdx.x >> 6] = q;
  }
  __syncthreads();
  s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  const float inv_cnt = 1.0f / ((float)HW * (float)cpg);
  const float ds = s * inv_cnt;
  const float mean = shift + ds;
  float var;
  if (keep) {
    q = 0.0f;
#pragma unroll
    for (int k = 0; k < GN_KEEP; ++k) {
      if (threadIdx.x + 256 * k < cnt2) {          // the zero padding is no part of the group
        const float d0 = (float)kv[k][0] - mean, d1 = (float)kv[k][1] - mean;
        q += d0 * d0 + d1 * d1;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if ((threadIdx.x & 63) == 0) red[2][threadIdx.x >> 6] = q;
    __syncthreads();
    var = ((red[2][0] + red[2][1]) + (red[2][2] + red[2][3])) * inv_cnt;
  } else {
    q = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    var = fmaxf(q * inv_cnt - ds * ds, 0.0f);
  }
  const float rstd = rsqrtf(var + eps);
  auto apply = [&](int e, f16x2 v) {
    const int p = e / cp2, c = e - p * cp2;
    const int ch = g * cpg + 2 * c;
    const f16x2 gm = *reinterpret_cast<const f16x2*>(gamma + ch);
    const f16x2 bt = *reinterpret_cast<const f16x2*>(beta + ch);
    float y0 = ((float)v[0] - mean) * rstd * (float)gm[0] + (float)bt[0];
    float y1 = ((float)v[1] - mean) * rstd * (float)gm[1] + (float)bt[1];
    if (do_silu) { y0 = silu(y0); y1 = silu(y1); }
    f16x2 o;
    o[0] = (f16)y0; o[1] = (f16)y1;
    *reinterpret_cast<f16x2*>(ob + (size_t)p * C + 2 * c) = o;
  };
  if (keep) {
#pragma unroll
    for (int k = 0; k < GN_KEEP; ++k) {
      const int e = threadIdx.x + 256 * k;
      if (e < cnt2) apply(e, kv[k]);
    }
  } else {
    for (int e = threadIdx.x; e < cnt2; e += 256) {
      const int p = e / cp2, c = e - p * cp2;
      apply(e, *reinterpret_cast<const f16x2*>(xb + (size_t)p * C + 2 * c));
    }
  }
}

// ---- the same with 16-byte accesses: one 1024-thread workgroup per (image, SUPER-group), a
// super-group being the smallest run of whole groups that is also a whole number of 8-channel
// chunks (10 channels per group -> 4 groups = 40 channels = 5 chunks).  The kernel above reads a
// group's 10..80 channels of a pixel as half2 pairs, 20..160 bytes out of every 640..5120-byte
// pixel row: 13 cache lines per wave instruction, each line fetched again by the 3-6 other
// workgroups whose groups share it (28.7 us for the 7.9 MB of a (12, 32x32, 320) tensor = 0.55 TB/s).
// Here a thread keeps its <= GS_KEEP chunks in registers between the statistics and the apply pass.
constexpr int GS_KEEP = 16;
constexpr int GS_THREADS = 1024;

// sum over each row of 16 lanes, in all of its lanes, on the VALU's lane-permute path (DPP): the
// LDS permutes behind __shfl_xor were 80 LDS instructions per wave of gn_super_kernel, 16 waves deep
template <int CTRL>
__device__ __forceinline__ float dpp_add(float t) {
  return t + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row_sum(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]: lane ^ 1
  v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]: lane ^ 2
  v = dpp_add<0x141>(v);   // row_half_mirror: 7 - lane within 8
  v = dpp_add<0x140>(v);   // row_mirror: 15 - lane within 16
  return v;
}
// sum over the wave, uniform
__device__ __forceinline__ float wave_sum(float v) {
  const int r = __float_as_int(row_sum(v));
  return (__int_as_float(__builtin_amdgcn_readlane(r, 0)) + __int_as_float(__builtin_amdgcn_readlane(r, 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(r, 32)) + __int_as_float(__builtin_amdgcn_readlane(r, 48)));
}
__global__ __launch_bounds__(GS_THREADS) void gn_super_kernel(const f16* __restrict__ x,
                                                              const f16* __restrict__ gamma,
                                                              const f16* __restrict__ beta, int HW,
                                                              int C, int cpg, int SG, float eps,
                                                              int do_silu, f16* __restrict__ out) {
  static_assert(GS_THREADS / 64 == 16, "the cross-wave sums below fold 16 partials");
  __shared__ float red[GS_THREADS / 64][8];       // per wave: shifted sum[4] | shifted sum of squares[4]
  const int nsg = C / SG, CH = SG >> 3;
  const int n = blockIdx.x / nsg, c_base = (blockIdx.x % nsg) * SG;
  const int total = HW * CH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const f16* xb = x + (size_t)n * HW * C + c_base;
  f16* ob = out + (size_t)n * HW * C + c_base;
  f16x8 kv[GS_KEEP];
  auto pick = [](const float (&t)[4], int g) {
    return g == 0 ? t[0] : (g == 1 ? t[1] : (g == 2 ? t[2] : t[3]));
  };
  // sums of x - K, K the group's own first element (see gn_shift): nothing cancels off zero, and
  // the statistics stay one pass over the registers with one workgroup-wide reduction
  float K[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    // workgroup-uniform, so read through the scalar unit as the aligned 32-bit word that holds it
    // (as vector loads these were 64 wave instructions per workgroup, beside 16-80 for the chunks);
    // unconditional: a group the super-group lacks reads group 0's
    const size_t i = (size_t)n * HW * C + c_base + (g * cpg < SG ? g * cpg : 0);
    const uint32_t w = reinterpret_cast<const uint32_t*>(x)[i >> 1];
    const uint16_t h = (uint16_t)(i & 1 ? w >> 16 : w);
    f16 hv;
    __builtin_memcpy(&hv, &h, sizeof(hv));
    K[g] = (float)hv;
  }
  float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
  // chunk e = threadIdx.x + GS_THREADS k is chunk c of pixel p.  One division per thread; from k
  // to k + 1 the pair moves by a workgroup-uniform step, and a channel's group (at most 4 per
  // super-group) comes from compares: the kernel is bound by its instruction count, not by HBM
  const int dp = GS_THREADS / CH, dc = GS_THREADS - dp * CH;
  const int p_first = (int)threadIdx.x / CH, c_first = (int)threadIdx.x - p_first * CH;
  auto step = [&](int& p, int& c) {
    p += dp;
    c += dc;
    if (c >= CH) { c -= CH; ++p; }
  };
  auto group_of = [&](int c8) { return (c8 >= cpg) + (c8 >= 2 * cpg) + (c8 >= 3 * cpg); };
  // every chunk is requested before the first is used: the loads overlap instead of each being
  // waited for in turn
  int p = p_first, c = c_first;
#pragma unroll
  for (int k = 0; k < GS_KEEP; ++k) {
    if ((int)threadIdx.x + GS_THREADS * k < total) {
      kv[k] = *reinterpret_cast<const f16x8*>(xb + (p * C + 8 * c));
      step(p, c);
    }
  }
  p = p_first;
  c = c_first;
#pragma unroll
  for (int k = 0; k < GS_KEEP; ++k) {
    const int e = threadIdx.x + GS_THREADS * k;
    if (e < total) {
      const int c8 = 8 * c;
      const f16x8 v = kv[k];
      // cpg >= 8: a chunk touches at most two groups, g0 for its first `split` channels
      const int g0 = group_of(c8), split = (g0 + 1) * cpg - c8;
      step(p, c);
      const float K0 = pick(K, g0), K1 = pick(K, g0 + 1);
      float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[j] - (j < split ? K0 : K1);
        if (j < split) { s0 += f; q0 += f * f; } else { s1 += f; q1 += f * f; }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        s[g] += g == g0 ? s0 : (g == g0 + 1 ? s1 : 0.0f);
        q[g] += g == g0 ? q0 : (g == g0 + 1 ? q1 : 0.0f);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    s[g] = wave_sum(s[g]);
    q[g] = wave_sum(q[g]);
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      red[wave][g] = s[g];
      red[wave][4 + g] = q[g];
    }
  }
  __syncthreads();
  // every wave folds the 16 wave partials itself (same additions in the same order everywhere, so
  // all waves hold the same bits): no second barrier, no serial loop
  const float inv_cnt = 1.0f / ((float)HW * (float)cpg);
  auto uniform = [](float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
  };
  float mean[4], rstd[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float ss = row_sum(red[lane & 15][g]), qq = row_sum(red[lane & 15][4 + g]);
    const float ds = ss * inv_cnt;
    // uniform across the workgroup: kept in scalar registers (the kept chunks fill the vector file)
    mean[g] = uniform(K[g] + ds);
    rstd[g] = uniform(rsqrtf(fmaxf(qq * inv_cnt - ds * ds, 0.0f) + eps));
  }
  p = p_first;
  c = c_first;
#pragma unroll
  for (int k = 0; k < GS_KEEP; ++k) {
    if ((int)threadIdx.x + GS_THREADS * k >= total) continue;
    const int c8 = 8 * c, off = p * C + c8;        // the same walk as above: nothing kept per chunk
    const int g0 = group_of(c8), split = (g0 + 1) * cpg - c8;
    step(p, c);
    const float m0 = pick(mean, g0), r0 = pick(rstd, g0);
    const float m1 = pick(mean, g0 + 1), r1 = pick(rstd, g0 + 1);
    const f16x8 gm = *reinterpret_cast<const f16x8*>(gamma + c_base + c8);
    const f16x8 bt = *reinterpret_cast<const f16x8*>(beta + c_base + c8);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float mu = j < split ? m0 : m1, rs = j < split ? r0 : r1;
      float y = ((float)kv[k][j] - mu) * rs * (float)gm[j] + (float)bt[j];
      if (do_silu) y = silu(y);
      o[j] = (f16)y;
    }
    *reinterpret_cast<f16x8*>(ob + off) = o;
  }
}

// ---- LayerNorm over the last dimension: one wave per row, C % 8 == 0, C <= 64*8*4
__global__ __launch_bounds__(256) void layernorm_kernel(const f16* __restrict__ x,
                                                        const f16* __restrict__ gamma,
                                                        const f16* __restrict__ beta,
                                                        int64_t rows, int C, float eps,
                                                        f16* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int C8 = C >> 3;
  f16x8 v[4];
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int g = lane + 64 * i;
    if (g < C8) {
      v[i] = *reinterpret_cast<const f16x8*>(x + row * C + g * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += (float)v[i][e];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)C;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int g = lane + 64 * i;
    if (g < C8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = (float)v[i][e] - mean;
        q += d * d;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = rsqrtf(q / (float)C + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int g = lane + 64 * i;
    if (g < C8) {
      const f16x8 gm = *reinterpret_cast<const f16x8*>(gamma + g * 8);
      const f16x8 bt = *reinterpret_cast<const f16x8*>(beta + g * 8);
      f16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        o[e] = (f16)(((float)v[i][e] - mean) * rstd * (float)gm[e] + (float)bt[e]);
      *reinterpret_cast<f16x8*>(out + row * C + g * 8) = o;
    }
  }
}

// ---- GEGLU: out[r][j] = h[r][j] * gelu(h[r][D + j])   (diffusers GEGLU: exact erf GELU)
__global__ __launch_bounds__(256) void geglu_kernel(const f16* __restrict__ h, int64_t rows,
                                                    int D, f16* __restrict__ out) {
  const int D8 = D >> 3;
  const int64_t total = rows * D8;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D8;
    const int j = (int)(i % D8) * 8;
    const f16x8 a = *reinterpret_cast<const f16x8*>(h + r * 2 * D + j);
    const f16x8 g = *reinterpret_cast<const f16x8*>(h + r * 2 * D + D + j);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gv = (float)g[e];
      const float gelu = 0.5f * gv * (1.0f + erff(gv * 0.70710678118654752f));
      o[e] = (f16)((float)a[e] * gelu);
    }
    *reinterpret_cast<f16x8*>(out + r * D + j) = o;
  }
}

}  // namespace

extern "C" {

int dsu_groupnorm_nhwc_f16(const void* x, const void* gamma, const void* beta, int32_t B,
                           int32_t HW, int32_t C, int32_t G, float eps, int32_t silu,
                           float* stats_ws, void* out, void* stream) {
  if (!x || !gamma || !beta || !stats_ws || !out) return DSU_EINVAL;
  if (B <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G != 0) return DSU_EINVAL;
  if (C % 8 != 0 || C / 8 > 1024 || (C / 8) % ((C / 8 + 255) / 256) != 0) return DSU_EUNSUP;
  hipStream_t s = (hipStream_t)stream;
  {
    // super-group form: groups of >= 8 channels whose super-group has <= 4 groups and fits the
    // registers of one 1024-thread workgroup
    const int cpg = C / G;
    int SG = cpg;
    while (SG % 8 != 0) SG += cpg;
    // (measured per UNet shape, tools/gn_time.py: 19-47 us instead of 26-58 at 32x32, 15.6 instead of
    // 20.1 at 16x16x1280, a tie at 16x16x640, 2-3 us SLOWER on the 8x8 / 4x4 levels — few, fat workgroups)
    if (HW >= 256 && cpg >= 8 && SG / cpg <= 4 && C % SG == 0 &&
        (int64_t)HW * (SG / 8) <= (int64_t)GS_KEEP * GS_THREADS && (int64_t)HW * C < ((int64_t)1 << 31)) {
      gn_super_kernel<<<B * (C / SG), GS_THREADS, 0, s>>>((const f16*)x, (const f16*)gamma,
                                                          (const f16*)beta, HW, C, cpg, SG, eps, silu,
                                                          (f16*)out);
      DSU_CHECK_LAUNCH();
      return DSU_OK;
    }
  }
  if ((int64_t)HW * (C / G) <= 32768 && (int64_t)B * G >= 64 && (C / G) % 2 == 0) {
    gn_fused_small_kernel<<<B * G, 256, 0, s>>>((const f16*)x, (const f16*)gamma,
                                                (const f16*)beta, HW, C, G, eps, silu, (f16*)out);
    DSU_CHECK_LAUNCH();
    return DSU_OK;
  }
  if (hipMemsetAsync(stats_ws, 0, (size_t)B * G * 2 * sizeof(float), s) != hipSuccess)
    return DSU_ELAUNCH;
  const int pix_per_block = 64;
  dim3 grid((HW + pix_per_block - 1) / pix_per_block, B);
  gn_stats_kernel<<<grid, 256, 2 * C * sizeof(float), s>>>((const f16*)x, HW, C, G,
                                                           pix_per_block, stats_ws);
  const int64_t total8 = (int64_t)B * HW * (C / 8);
  gn_apply_kernel<<<dsu_capped_blocks(total8, 256, 4096), 256, 0, s>>>(
      (const f16*)x, stats_ws, (const f16*)gamma, (const f16*)beta, HW, C, G, eps, silu, total8,
      (f16*)out);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_layernorm_f16(const void* x, const void* gamma, const void* beta, int64_t rows,
                      int32_t C, float eps, void* out, void* stream) {
  if (!gamma || !beta || rows < 0 || C <= 0) return DSU_EINVAL;
  if (C % 8 != 0 || C > 2048) return DSU_EUNSUP;
  if (rows == 0) return DSU_OK;   // an empty tensor has no storage: x and out may be null here
  if (!x || !out) return DSU_EINVAL;
  layernorm_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      (const f16*)x, (const f16*)gamma, (const f16*)beta, rows, C, eps, (f16*)out);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

int dsu_geglu_f16(const void* h, int64_t rows, int32_t D, void* out, void* stream) {
  if (rows < 0 || D <= 0) return DSU_EINVAL;
  if (D % 8 != 0) return DSU_EUNSUP;
  if (rows == 0) return DSU_OK;
  if (!h || !out) return DSU_EINVAL;
  geglu_kernel<<<dsu_capped_blocks(rows * (D / 8), 256, 4096), 256, 0, (hipStream_t)stream>>>(
      (const f16*)h, rows, D, (f16*)out);
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

}  // extern "C"
