// The mip pyramid of the UV atlas behind the trilinear filter of the frame rasteriser
// (DSU_TEX_TRILINEAR of dsu_mesh_render_ortho, mesh_render.hip).  The rule is stated in full in include/dsu_hip.h
// ("Mip-mapped frames"); tests/frame_render_mip_ref.py restates it by brute force.
//
//   level 0      the atlas, byte for byte
//   level k >= 1 texel (r, c) = rounded mean of the COVERED level-0 texels of its 2^k x 2^k block,
//                taken from exact sums: every level carries (sum_r, sum_g, sum_b, n) per texel in
//                64 bits to the next, so rounding does not compound; then `gutter` rounds of
//                dsu_uv_dilate's rule on that level, alpha = 255 covered / 0 uncovered.
//
// One thread per output texel, its 2 x 2 children read directly; no atomics, no LDS.  The sums of
// two consecutive levels ping-pong between the two halves of the workspace, the gutter rounds between
// the level's place in the pyramid and a third workspace region.
#include "common.h"
#include "mip_sample.h"

namespace {

struct MipSum {
  uint64_t r, g, b, n;
};

__device__ __forceinline__ uint32_t mip_mean(const MipSum& s) {
  if (!s.n) return 0u;
  const uint64_t d = 2ull * s.n;
  return (uint32_t)((2ull * s.r + s.n) / d) | ((uint32_t)((2ull * s.g + s.n) / d) << 8) |
         ((uint32_t)((2ull * s.b + s.n) / d) << 16) | 0xff000000u;
}

// FIRST: children are level-0 texels (atlas words, optional coverage bytes); else the sums of the
// level below.  Children past the clipped edge of an odd level are absent.
template <bool FIRST>
__global__ __launch_bounds__(256) void mip_reduce_kernel(const uint32_t* __restrict__ atlas,
                                                         const uint8_t* __restrict__ covered,
                                                         const MipSum* __restrict__ below, int32_t Tin,
                                                         int32_t Tout, MipSum* __restrict__ sums,
                                                         uint32_t* __restrict__ image) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)Tout * Tout) return;
  const int r = (int)(i / Tout), c = (int)(i - (int64_t)r * Tout);
  MipSum s{0, 0, 0, 0};
#pragma unroll
  for (int dr = 0; dr < 2; ++dr)
#pragma unroll
    for (int dc = 0; dc < 2; ++dc) {
      const int rr = 2 * r + dr, cc = 2 * c + dc;
      if (rr >= Tin || cc >= Tin) continue;
      const int64_t j = (int64_t)rr * Tin + cc;
      if constexpr (FIRST) {
        if (covered && !covered[j]) continue;
        const uint32_t p = atlas[j];
        s.r += p & 255u; s.g += (p >> 8) & 255u; s.b += (p >> 16) & 255u; s.n += 1;
      } else {
        const MipSum q = below[j];
        s.r += q.r; s.g += q.g; s.b += q.b; s.n += q.n;
      }
    }
  sums[i] = s;
  image[i] = mip_mean(s);
}

// dsu_uv_dilate's round on RGBA8 words whose alpha byte is the coverage (255 / 0).
__global__ __launch_bounds__(256) void mip_dilate_kernel(const uint32_t* __restrict__ in, int32_t S,
                                                         uint32_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)S * S) return;
  const uint32_t own = in[i];
  if (own >> 24) {
    out[i] = own;
    return;
  }
  const int r = (int)(i / S), c = (int)(i - (int64_t)r * S);
  uint32_t sum[3] = {0, 0, 0}, n = 0;
  for (int dr = -1; dr <= 1; ++dr)
    for (int dc = -1; dc <= 1; ++dc) {
      const int rr = r + dr, cc = c + dc;
      if ((dr == 0 && dc == 0) || rr < 0 || cc < 0 || rr >= S || cc >= S) continue;
      const uint32_t p = in[(int64_t)rr * S + cc];
      if (!(p >> 24)) continue;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) sum[ch] += (p >> (8 * ch)) & 255u;
      ++n;
    }
  out[i] = n ? ((2u * sum[0] + n) / (2u * n)) | (((2u * sum[1] + n) / (2u * n)) << 8) |
                   (((2u * sum[2] + n) / (2u * n)) << 16) | 0xff000000u
             : 0u;
}

constexpr int MIP_MAX_GUTTER = 64;

bool size_ok(int32_t T) { return T >= 1 && T <= dsu_mip::MAX_T; }

// workspace: sums of the odd levels | sums of the even levels >= 2 | one level-1 image
struct MipWorkspace {
  int64_t odd, even, image, bytes;
};
MipWorkspace split(int32_t T) {
  const int64_t t1 = dsu_mip::level_size(T, 1), t2 = dsu_mip::level_size(T, 2);
  MipWorkspace w;
  w.odd = 0;
  w.even = t1 * t1 * (int64_t)sizeof(MipSum);
  w.image = w.even + t2 * t2 * (int64_t)sizeof(MipSum);
  w.bytes = T > 1 ? w.image + t1 * t1 * 4 : 0;
  return w;
}

}  // namespace

extern "C" {

int32_t dsu_mip_levels(int32_t tex_size) { return size_ok(tex_size) ? dsu_mip::levels(tex_size) : DSU_EINVAL; }

int64_t dsu_mip_pyramid_texels(int32_t tex_size) {
  if (!size_ok(tex_size)) return DSU_EINVAL;
  return dsu_mip::level_offset(tex_size, dsu_mip::levels(tex_size));
}

int64_t dsu_mip_workspace_bytes(int32_t tex_size) {
  if (!size_ok(tex_size)) return DSU_EINVAL;
  return split(tex_size).bytes;
}

int dsu_mip_pyramid_build(const uint8_t* texture, const uint8_t* covered, int32_t tex_size, int32_t gutter,
                          uint8_t* pyramid, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!size_ok(tex_size) || gutter < 0 || gutter > MIP_MAX_GUTTER || !texture || !pyramid) return DSU_EINVAL;
  if ((uintptr_t)texture % 4 || (uintptr_t)pyramid % 4) return DSU_EINVAL;      // a texel is one 32-bit word
  const MipWorkspace w = split(tex_size);
  if (w.bytes && (!workspace || workspace_bytes < w.bytes || (uintptr_t)workspace % 16)) return DSU_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int32_t T = tex_size, L = dsu_mip::levels(T);
  if (pyramid != texture &&
      hipMemcpyAsync(pyramid, texture, (size_t)T * T * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return DSU_ELAUNCH;
  const uint32_t* atlas = reinterpret_cast<const uint32_t*>(texture);
  uint32_t* pyr = reinterpret_cast<uint32_t*>(pyramid);
  char* ws = static_cast<char*>(workspace);
  uint32_t* spare = w.bytes ? reinterpret_cast<uint32_t*>(ws + w.image) : nullptr;
  const MipSum* below = nullptr;
  int64_t at = (int64_t)T * T;
  for (int k = 1, Tin = T; k < L; ++k) {
    const int Tout = (Tin + 1) >> 1;
    const int blocks = dsu_blocks_for((int64_t)Tout * Tout, 256);
    MipSum* sums = reinterpret_cast<MipSum*>(ws + (k & 1 ? w.odd : w.even));
    uint32_t* level = pyr + at;
    // the rounds alternate between the level's place and the spare image and must end in place
    uint32_t* src = (gutter & 1) ? spare : level;
    if (k == 1)
      mip_reduce_kernel<true><<<blocks, 256, 0, st>>>(atlas, covered, nullptr, Tin, Tout, sums, src);
    else
      mip_reduce_kernel<false><<<blocks, 256, 0, st>>>(nullptr, nullptr, below, Tin, Tout, sums, src);
    for (int g = 0; g < gutter; ++g) {
      uint32_t* dst = src == level ? spare : level;
      mip_dilate_kernel<<<blocks, 256, 0, st>>>(src, Tout, dst);
      src = dst;
    }
    below = sums;
    at += (int64_t)Tout * Tout;
    Tin = Tout;
  }
  DSU_CHECK_LAUNCH();
  return DSU_OK;
}

// HOST: the sampling of the trilinear resolve evaluated on the CPU — pyramid, tx, ty, rho, rgb_out
// are host arrays.  rgb_out (n, 3) f32.
int dsu_mip_sample_host(const uint8_t* pyramid, int32_t tex_size, const double* tx, const double* ty,
                        const double* rho, int64_t n, float* rgb_out) {
  if (!size_ok(tex_size) || n < 0 || !pyramid || (uintptr_t)pyramid % 4) return DSU_EINVAL;
  if (n && (!tx || !ty || !rho || !rgb_out)) return DSU_EINVAL;
  const uint32_t* pyr = reinterpret_cast<const uint32_t*>(pyramid);
  const int L = dsu_mip::levels(tex_size);
  for (int64_t i = 0; i < n; ++i) {
    int k;
    double t;
    dsu_mip::lod(rho[i], L, k, t);
    dsu_mip::sample(pyr, tex_size, tx[i], ty[i], k, t, dsu_mip::level_offset(tex_size, k), rgb_out + 3 * i);
  }
  return DSU_OK;
}

// HOST: the anisotropic resolve's per-face and per-sample text (include/dsu_hip.h, "Anisotropic frames")
// on host arrays, one (face, sample) pair per item.
int dsu_aniso_sample_host(const uint8_t* pyramid, int32_t tex_size, const double* tri, const float* uv, double h,
                          const double* tx, const double* ty, int32_t max_aniso, int64_t n, float* rgb_out,
                          int32_t* probes_out, double* rho_out, double* axis_out) {
  if (!size_ok(tex_size) || n < 0 || max_aniso < 1 || max_aniso > dsu_mip::MAX_ANISO || !dsu_mip::finite(h))
    return DSU_EINVAL;
  if (n && (!pyramid || (uintptr_t)pyramid % 4 || !tri || !uv || !tx || !ty || !rgb_out)) return DSU_EINVAL;
  const uint32_t* pyr = reinterpret_cast<const uint32_t*>(pyramid);
  const int L = dsu_mip::levels(tex_size);
  for (int64_t i = 0; i < n; ++i) {
    const double* p = tri + 6 * i;
    const float* q = uv + 6 * i;
    const dsu_mip::AnisoFace f = dsu_mip::footprint_aniso(p[0], p[1], p[2], p[3], p[4], p[5], q[0], q[1], q[2], q[3],
                                                          q[4], q[5], tex_size, h, max_aniso, L);
    dsu_mip::sample_aniso(pyr, tex_size, tx[i], ty[i], f.s1, f.N, f.ax, f.ay, f.k, f.t,
                          dsu_mip::level_offset(tex_size, f.k), rgb_out + 3 * i);
    if (probes_out) probes_out[i] = f.N;
    if (rho_out) rho_out[i] = f.rho;
    if (axis_out) {
      axis_out[2 * i] = f.ax;
      axis_out[2 * i + 1] = f.ay;
    }
  }
  return DSU_OK;
}

}  // extern "C"
