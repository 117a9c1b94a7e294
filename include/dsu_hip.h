/*
 * dsu_hip.h — C ABI of libdsu_hip.so, the MI355X (gfx950) hot path of DrawingSpinUp.
 *
 * Every entry point replaces one third-party native op that the reference reaches
 * through a Python import (the reference ships no native code of its own).  The
 * reference call site each function stands in for is cited as
 * `<path under /root/reference>:<line>`.
 *
 * Conventions
 *   - plain C, no torch types: device pointers, element counts, a hipStream_t passed
 *     as void*.  The caller owns every buffer; nothing is allocated inside.
 *   - all kernels are stream-ordered on `stream`; no internal synchronisation.
 *   - return value: 0 = ok, <0 = DSU_E* error code (dsu_strerror gives the text).
 *   - "f16" buffers hold IEEE binary16, "f32" IEEE binary32, row-major, contiguous.
 */
#ifndef DSU_HIP_H
#define DSU_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSU_OK 0
#define DSU_EINVAL (-1)   /* bad argument (null pointer, unsupported size) */
#define DSU_ELAUNCH (-2)  /* hipLaunch / runtime error */
#define DSU_EUNSUP (-3)   /* configuration not supported by the kernels */

#define DSU_MAX_LEVELS 16

const char* dsu_strerror(int code);
/* ABI version of this header: DSU_ABI_VERSION, bumped by any change to an exported signature or to the
 * layout of a struct declared here.  dsu_abi_version() returns the value the library was compiled with;
 * a caller that binds from this header (drawingspinup_amd/_lib.py) compares the two before the first call. */
#define DSU_ABI_VERSION 3
int dsu_abi_version(void);
/* CUs given to the two whole-SIMD kernels of the NSR step (the MLP part of the geometry backward,
 * the texture backward: their waves fill every SIMD of a CU they run on, nothing else fits beside
 * them).  Each kernel launches cus x its resident workgroups per CU: one for the texture backward
 * (450-510 registers per lane) and for the geometry backward at 7 active levels, two for the
 * geometry backward at 4..6 active levels (<= 256 registers, two waves per SIMD).  0 = every CU (a
 * single optimisation alone on the GPU); with several drawings in flight on one GPU fewer CUs
 * leave the rest to the other drawings' kernels while such a kernel runs (bench.py --inflight: 192).
 * Process-wide; workspaces stay sized for the resident count. */
int dsu_set_onewave_grid_cap(int32_t cus);
/* The same for the table-gradient scatter of the geometry backward (0 = its resident count: three
 * 256-thread workgroups of 45 KB LDS per CU). */
int dsu_set_scatter_grid_cap(int32_t workgroups);
/* Priority of the side stream on which the NSR step driver marches and packs the next step's samples
 * (dsu_nsr_driver_create reads it): 1 = high (default: what several drawings in flight measured best
 * with), 2 = normal (one drawing at a time: streams of non-default priority put every fourth and later
 * drawing of a process into a 0.8 s slower mode, profiles/round6_side_stream_priority.txt), 0 = low.
 * Process-wide. */
int dsu_set_nsr_side_stream_priority(int32_t level);
/* 1: a destroyed step driver hands its (drained) side stream to the next driver created on the same
 * device with the same priority, so that a process creates as many side streams as it has drawings
 * in flight instead of one per drawing.  0 (default): one stream per driver.  Prepared at the end of
 * round 6: six of six back-to-back reconstructions fast at high priority with it (un-pooled: slow from
 * the fourth on); the bench line with drawings in flight is not measured with it yet.  Process-wide. */
int dsu_set_nsr_side_stream_pooling(int32_t on);

/* ------------------------------------------------------------------------------------
 * Multi-resolution hash grid (replaces tiny-cuda-nn `tcnn.Encoding(3, {otype:HashGrid})`
 * constructed at 2_charactor_reconstructor/instant_nsr/models/network_utils.py:46 and
 * called at :55; hyper-parameters from configs/neuralangelo-ortho-wmask.yaml:52-62).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  uint32_t n_levels;           /* 10 */
  uint32_t n_features;         /* 2 (the kernels are specialised for 2) */
  uint32_t log2_hashmap_size;  /* 19 */
  uint32_t base_resolution;    /* 32 */
  double per_level_scale;      /* 1.3195079107728942 */
} dsu_hashgrid_cfg;

/* Per-level derived quantities.  offsets[l] = first table ENTRY of level l (an entry is
 * n_features values); offsets[n_levels] = total entries.  scale/resolution follow
 * tcnn's grid_scale()/grid_resolution(); hashed[l]=1 when the level is addressed by the
 * coherent-prime hash instead of the dense x+y*res+z*res^2 index. */
typedef struct {
  uint32_t offsets[DSU_MAX_LEVELS + 1];
  uint32_t resolution[DSU_MAX_LEVELS];
  float scale[DSU_MAX_LEVELS];
  uint32_t hashed[DSU_MAX_LEVELS];
} dsu_hashgrid_levels;

/* Host-only: fill `out` for `cfg`.  Pure function; safe without a GPU. */
int dsu_hashgrid_make_levels(const dsu_hashgrid_cfg* cfg, dsu_hashgrid_levels* out);

/* tcnn.Encoding.__call__ (network_utils.py:55) fused with the progressive level mask
 * (network_utils.py:56): out[n, 2*l..2*l+1] = trilinear lookup for l < active_levels,
 * 0 for the masked levels.  x: (n,3) f32 in [0,1]; table: (total_entries,2) f16;
 * out: (n, 2*n_levels) f16. */
int dsu_hashgrid_encode_fwd(const dsu_hashgrid_cfg* cfg, const void* table_f16,
                            const float* x, int64_t n, uint32_t active_levels,
                            void* out_f16, void* stream);

/* Backward of the above w.r.t. the table only (the reference never needs dL/dx:
 * grad_type=finite_difference, neuralangelo-ortho-wmask.yaml:42).  dout: (n, 2*n_levels)
 * f32; grad_table: (total_entries,2) f32, ACCUMULATED into (caller zeroes it). */
int dsu_hashgrid_encode_bwd(const dsu_hashgrid_cfg* cfg, const float* x, const float* dout,
                            int64_t n, uint32_t active_levels, float* grad_table,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * Fused SDF network: contract -> hash grid -> cat(xyz*2-1, enc*mask) -> Linear(23,64) ->
 * Softplus(beta=100) -> Linear(64,13).  Replaces VolumeSDF.forward_level
 * (instant_nsr/models/geometry.py:189-194) and the per-point body of VolumeSDF.forward
 * (geometry.py:135-187): N1-N5 of SURVEY.md §8(a).
 * Weights are the EFFECTIVE (weight-norm already applied) row-major nn.Linear matrices.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const float* w0; /* (64, 23) */
  const float* b0; /* (64) */
  const float* w1; /* (13, 64) */
  const float* b1; /* (13) */
} dsu_sdf_mlp;

/* pts: (n,3) f32 world coordinates in [-radius, radius]; out: (n, n_out) f32 where
 * n_out = 1 (sdf only: forward_level / occupancy / export) or 13 (sdf + feature). */
int dsu_sdf_fwd(const dsu_hashgrid_cfg* cfg, const void* table_f16, const dsu_sdf_mlp* mlp,
                const float* pts, int64_t n, float radius, uint32_t active_levels,
                uint32_t n_out, float* out, void* stream);
/* The same network on the export's lattice (BaseImplicitGeometry.isosurface_, geometry.py:83-106:
 * `scale_anything(meshgrid(linspace(0,1,res)), (0,1), (vmin,vmax))` -> forward_level, chunk by
 * chunk): the points are formed in the kernel, x-slabs [x0, x0 + nx) of the res^3 lattice,
 * p = lin[i] * span + lo per axis (two rounded f32 operations, as the reference's tensor
 * expression).  lin: (res) f32 on the device (the caller's linspace); out: (nx * res * res) f32,
 * x-major / y / z-minor. */
int dsu_sdf_fwd_lattice(const dsu_hashgrid_cfg* cfg, const void* table_f16, const dsu_sdf_mlp* mlp,
                        const float* lin, int32_t res, int32_t x0, int32_t nx, const float* lo3,
                        const float* span3, float radius, uint32_t active_levels, float* out,
                        void* stream);

/* VolumeSDF.forward(points, with_grad, with_feature, with_laplace) with
 * grad_type=finite_difference (geometry.py:158-176): 7 network evaluations per point
 * (centre + 6 clamped +-eps offsets), and its backward w.r.t. table and MLP parameters:
 * dsu_sdf_fd_fwd_sorted / dsu_sdf_fd_bwd_sorted, declared below with the evaluation order they
 * take.  Forward outputs (any may be NULL except sdf): sdf (n), grad (n,3), feature (n,13),
 * laplace (n).  Upstream gradients of the backward (NULL = zero): d_sdf (n), d_grad (n,3),
 * d_feature (n,13), d_laplace (n).  It accumulates into grad_table (entries,2) f32 and g_w0 (64,23),
 * g_b0 (64), g_w1 (13,64), g_b1 (13) f32 — caller zeroes them.  `workspace` is caller-owned device
 * scratch of at least dsu_sdf_fd_bwd_workspace_bytes(cfg, n) bytes (contents undefined on return).
 * A feature cache may sit between the two calls: the forward pass stores the interpolated f16
 * hash-grid features of all 7 evaluations ([eval][point][active level] half2,
 * dsu_sdf_fd_enc_cache_bytes(n, active_levels) bytes) and the backward pass reads them back
 * instead of repeating the 7 x active_levels x 8 table gathers per point.  Same results bit
 * for bit (the cached values ARE the forward's features); enc_cache NULL = no cache. */
int64_t dsu_sdf_fd_enc_cache_bytes(int64_t n, uint32_t active_levels);

/* Spatially sorted evaluation order for one optimisation step.  VolumeSDF.forward is pointwise
 * (geometry.py:135-187), but its callers hand it the samples ray by ray (neus.py:119-129 ->
 * nerfacc.ray_marching order) and the rays are random pixels of six views, so neighbouring
 * lanes touch unrelated table neighbourhoods.  dsu_spatial_sort bins the points on a
 * 2^bits-per-axis lattice of the [-radius, radius]^3 cube in Morton order (counting sort;
 * bits 4..7): pts_sorted[i] = pts[perm[i]].  The *_sorted calls take the sorted points plus
 * perm and read / write every per-point array (sdf, grad, feature, laplace, d_*) in the
 * CALLER'S row order through it; the feature cache is kept in sorted order.  perm NULL = the
 * points as they are, in the caller's order.  Same per-point arithmetic, bit for bit. */
int64_t dsu_spatial_sort_workspace_bytes(int64_t n, int32_t bits);
int dsu_spatial_sort(const float* pts, int64_t n, float radius, int32_t bits, int32_t* perm,
                     float* pts_sorted, void* workspace, int64_t workspace_bytes, void* stream);
/* Prefetch-path variants: the sample total of the next step is still on the device when the side
 * stream packs and sorts its points.  dsu_ray_compact_points_cap = dsu_ray_compact_points into
 * fixed-capacity outputs (rows beyond out_capacity are dropped: the caller checks the total
 * later); dsu_points_tail writes the 2 x n_random random / perturbed points of neus.py:155-162
 * behind the ray samples (row total_dev[0]); dsu_spatial_sort_dev sorts n_dev[0] + n_add points
 * (at most n_capacity). */
int dsu_points_tail(float* points, int64_t capacity_rows, const int32_t* total_dev,
                    const float* pts_random, const float* perturb, int64_t n_random, float alpha,
                    void* stream);
int dsu_spatial_sort_dev(const float* pts, int64_t n_capacity, const int32_t* n_dev, int64_t n_add,
                         float radius, int32_t bits, int32_t* perm, float* pts_sorted,
                         void* workspace, int64_t workspace_bytes, void* stream);
int dsu_sdf_fd_fwd_sorted(const dsu_hashgrid_cfg* cfg, const void* table_f16,
                          const dsu_sdf_mlp* mlp, const float* pts_sorted, const int32_t* perm,
                          int64_t n, float radius, float eps, uint32_t active_levels, float* sdf,
                          float* grad, float* feature, float* laplace, void* enc_cache,
                          void* stream);
int dsu_sdf_fd_bwd_sorted(const dsu_hashgrid_cfg* cfg, const void* table_f16,
                          const dsu_sdf_mlp* mlp, const float* pts_sorted, const int32_t* perm,
                          int64_t n, float radius, float eps, uint32_t active_levels,
                          const float* d_sdf, const float* d_grad, const float* d_feature,
                          const float* d_laplace, float* grad_table, float* g_w0, float* g_b0,
                          float* g_w1, float* g_b1, void* workspace, int64_t workspace_bytes,
                          const void* enc_cache, void* stream);

/* A deferred sum of per-workgroup partial vectors: element v of the result is
 * sum_b partials[b * stride + v] (b < nblocks, v < n), added to base[map[v]] (map[v] < 0: a padding
 * element, dropped).  The partial reductions of the backward kernels are carried out by extra
 * workgroups of the scatter launch of dsu_sdf_fd_bwd_sorted_fold instead of launches of their own. */
typedef struct dsu_partial_reduce {
  const float* partials;
  const int32_t* map;   /* device, n entries */
  float* base;
  int32_t nblocks, stride, n;
} dsu_partial_reduce;

/* dsu_sdf_fd_bwd_sorted with two optional extras (dsu_sdf_fd_bwd_sorted passes NULL for both).
 * `mid_event`: a hipEvent_t (as void*, may be NULL) recorded on `stream` between the two kernels of
 * the backward: behind the MLP part, which fills every SIMD, and in front of the table-gradient
 * scatter, which leaves room.  Work a caller wants to overlap with the backward (the next step's ray
 * march) waits for it.  `extra` (may be NULL): a deferred partial sum of ANOTHER kernel that precedes
 * this call on `stream` (the native NSR step passes the texture backward's:
 * dsu_texture_bwd_shaded_partials_m), carried out by the scatter launch.  The backward's own partial
 * sums always ride in that launch.  DSU_EUNSUP with `extra` and n == 0. */
int dsu_sdf_fd_bwd_sorted_fold(const dsu_hashgrid_cfg* cfg, const void* table_f16,
                               const dsu_sdf_mlp* mlp, const float* pts_sorted, const int32_t* perm,
                               int64_t n, float radius, float eps, uint32_t active_levels,
                               const float* d_sdf, const float* d_grad, const float* d_feature,
                               const float* d_laplace, float* grad_table, float* g_w0, float* g_b0,
                               float* g_w1, float* g_b1, void* workspace, int64_t workspace_bytes,
                               const void* enc_cache, void* mid_event,
                               const dsu_partial_reduce* extra, void* stream);

/* Bytes of device scratch dsu_sdf_fd_bwd_sorted needs for n points (per-workgroup partial MLP
 * gradients, summed by a second kernel: deterministic, no same-address atomics).  <0 = error. */
int64_t dsu_sdf_fd_bwd_workspace_bytes(const dsu_hashgrid_cfg* cfg, int64_t n);

/* ------------------------------------------------------------------------------------
 * nerfacc 0.3.3 replacements (call sites instant_nsr/models/neus.py:53-57,84,119-129,
 * 147-152).
 * ---------------------------------------------------------------------------------- */

/* ray_aabb_intersect + optional stratified jitter: t_min += jitter*step (jitter may be
 * NULL).  rays_o/rays_d (n,3) f32; aabb 6 floats (host values). */
int dsu_ray_aabb(const float* rays_o, const float* rays_d, int64_t n_rays, const float* aabb6,
                 const float* jitter, float step, float* t_min, float* t_max, void* stream);

/* ray_marching through the binary occupancy grid (res^3 uint8, index x*res*res + y*res + z; NULL:
 * no grid), in one pass: each ray's samples go into a fixed-capacity scratch row (ray r at
 * scratch[r*capacity ...]) and its count into num_steps (n_rays) int32; dsu_ray_compact* then
 * pack the rows at the exclusive prefix sum of the counts (dsu_ray_offsets).  A ray with more
 * than `capacity` samples keeps the first `capacity` and is reported through num_steps (the
 * caller checks max(num_steps) <= capacity). */
int dsu_ray_march_scratch(const float* rays_o, const float* rays_d, const float* t_min,
                          const float* t_max, int64_t n_rays, const float* aabb6,
                          const uint8_t* occ_binary, int32_t res, float step, int32_t capacity,
                          int32_t* num_steps, float* scratch_t_starts, float* scratch_t_ends,
                          void* stream);
int dsu_ray_compact(const float* scratch_t_starts, const float* scratch_t_ends, int32_t capacity,
                    const int32_t* offsets, const int32_t* counts, int64_t n_rays,
                    int64_t* ray_indices, float* t_starts, float* t_ends, void* stream);

/* dsu_ray_compact that also writes the sample positions
 * rays_o[r] + rays_d[r] * ((t_start + t_end) / 2)  (neus.py:131-134: t_origins, t_dirs,
 * midpoints, positions) and no ray_indices — the fused step addresses samples by (offsets,
 * counts) only. */
int dsu_ray_compact_points(const float* scratch_t_starts, const float* scratch_t_ends,
                           int32_t capacity, const int32_t* offsets, const int32_t* counts,
                           int64_t n_rays, const float* rays_o, const float* rays_d,
                           float* t_starts, float* t_ends, float* positions, void* stream);
int dsu_ray_compact_points_cap(const float* scratch_t_starts, const float* scratch_t_ends,
                           int32_t capacity, const int32_t* offsets, const int32_t* counts,
                           int64_t n_rays, const float* rays_o, const float* rays_d,
                           float* t_starts, float* t_ends, float* positions, int64_t out_capacity,
                               void* stream);
/* offsets = exclusive prefix sum of counts; stats[0] = total, stats[1] = max(counts)
 * (nerfacc's packed_info construction; one launch, read back with ONE host copy). */
int dsu_ray_offsets(const int32_t* counts, int64_t n_rays, int32_t* offsets, int32_t* stats,
                    void* stream);

/* render_weight_from_alpha (neus.py:147): per ray segment [offsets[r], offsets[r]+cnt[r])
 * w_i = alpha_i * prod_{j<i}(1-alpha_j).  One ray per thread. */
int dsu_weights_from_alpha_fwd(const float* alpha, const int32_t* offsets, const int32_t* counts,
                               int64_t n_rays, float* weights, void* stream);
int dsu_weights_from_alpha_bwd(const float* alpha, const float* weights, const float* d_weights,
                               const int32_t* offsets, const int32_t* counts, int64_t n_rays,
                               float* d_alpha, void* stream);

/* accumulate_along_rays (neus.py:148-152): out[r, c] = sum_i w_i * v[i, c]  (v NULL -> 1). */
int dsu_accumulate_fwd(const float* weights, const float* values, int32_t channels,
                       const int32_t* offsets, const int32_t* counts, int64_t n_rays,
                       float* out, void* stream);

/* OccupancyGrid._update tail (nerfacc 0.3.3 grid.py): occs[idx] = max(occs[idx]*decay, occ).
 * idx may be NULL (= all cells, warm-up; scratch unused).  With idx, every old value is read
 * before any is written (the indexed assignment gathers first) and a cell listed several times
 * keeps the largest of its candidates: scratch = n floats of the caller.  occ are opacities (>= 0):
 * a negative candidate is stored as 0. */
int dsu_occgrid_ema(float* occs, const int64_t* idx, const float* occ, int64_t n, float decay,
                    float* scratch, void* stream);
/* binary = occs > thre  (thre = min(mean(occs), occ_thre) computed by the caller). */
int dsu_occgrid_binarize(const float* occs, int64_t n_cells, float thre, uint8_t* binary,
                         void* stream);

/* The whole refresh (nerfacc 0.3.3 OccupancyGrid._update with NeuSModel's occ_eval_fn,
 * instant_nsr/models/neus.py:61-88) as one stream-ordered sequence without host round trips:
 * cells (all of them while all_cells = 1, i.e. step < warm-up; otherwise res^3/4 uniform draws + the
 * occupied cells, subsampled to res^3/4 with replacement when there are more) -> points
 * (cell + U[0,1)^3) / res in the aabb -> dsu_sdf_fwd -> occ = clip((sigmoid(prev inv_s) -
 * sigmoid(next inv_s) + 1e-5) / (sigmoid(prev inv_s) + 1e-5)), prev / next = sdf +- render_step_size/2
 * -> occs[c] = max(occs[c] ema_decay, occ) -> binary = occs > min(mean(occs), occ_thre).
 * A cell drawn several times is decayed once and keeps the largest of its occ values (one of the
 * outcomes of nerfacc's indexed assignment, whose winner among duplicates is unspecified; the old
 * values are all gathered before any is written, as there).
 * Draws: Philox4x32-10 keyed (seed, step), streams 8-10.  inj_cells / inj_rand (device, inj_count
 * cells and inj_count x 3 uniforms; tests) replace the draws.  thre_out (device, may be NULL)
 * receives the threshold.  cells_out / rand_out (device, may be NULL; capacity res^3 cells while
 * all_cells, else 2 (res^3 / 4), x 3 uniforms): the cells (-1 = unused slot) and uniforms the call
 * evaluated, so that a caller can replay the update.  workspace:
 * dsu_occgrid_refresh_workspace_bytes(res) (< 0: invalid). */
typedef struct dsu_occgrid_refresh_args {
  float* occs;               /* (res^3) f32, updated in place */
  uint8_t* binary;           /* (res^3) u8: read (occupied cells), then rewritten */
  int32_t res, all_cells;
  const float* aabb;         /* HOST: min xyz, max xyz */
  uint64_t seed;
  int64_t step;
  const dsu_hashgrid_cfg* grid;
  const void* table_img;
  const dsu_sdf_mlp* mlp;    /* effective (weight-normed) weights */
  const float* inv_s;        /* device scalar exp(10 variance) */
  float radius, render_step_size, ema_decay, occ_thre;
  uint32_t active_levels;
  int32_t inj_count;
  const int32_t* inj_cells;
  const float* inj_rand;
  float* thre_out;
  void* workspace;
  int64_t workspace_bytes;
  int32_t* cells_out;
  float* rand_out;
} dsu_occgrid_refresh_args;
int64_t dsu_occgrid_refresh_workspace_bytes(int32_t res);
int dsu_occgrid_refresh(const dsu_occgrid_refresh_args* args, void* stream);

/* Fused NeuS shading + compositing of one ray batch (neus.py:90-112 get_alpha, :143-153
 * render_weight_from_alpha + the four accumulate_along_rays): per sample
 *   alpha = clip((sigmoid(prev*inv_s) - sigmoid(next*inv_s) + 1e-5) / (sigmoid(prev*inv_s) + 1e-5))
 * with the cos-anneal of neus.py:97-104, w = alpha * prod_{j<i}(1-alpha_j); per ray
 * comp[r] = {opacity, depth, rgb(3), sum w*normal (3)}.  sdf (n), normal (n,3), rgb (n,3),
 * rays_d (n_rays,3) unit directions, t_starts/t_ends (n); alpha/weights (n) are written for
 * the backward pass.  inv_s: DEVICE pointer to the scalar exp(10*variance) (clipped to
 * [1e-6,1e6] inside, neus.py:91), so no host synchronisation is needed. */
int dsu_neus_composite_fwd(const float* sdf, const float* normal, const float* rgb,
                           const float* rays_d, const float* t_starts, const float* t_ends,
                           const int32_t* offsets, const int32_t* counts, int64_t n_rays,
                           const float* inv_s, float cos_anneal_ratio, float* alpha,
                           float* weights, float* comp, void* stream);
/* Backward: d_comp (n_rays,8), optional d_weights (n) -> d_sdf (n), d_normal (n,3), d_rgb (n,3);
 * d_inv_s (1 float, caller zeroes) accumulates the gradient of the variance scalar. */
int dsu_neus_composite_bwd(const float* sdf, const float* normal, const float* rgb,
                           const float* rays_d, const float* t_starts, const float* t_ends,
                           const int32_t* offsets, const int32_t* counts, int64_t n_rays,
                           const float* inv_s, float cos_anneal_ratio, const float* alpha,
                           const float* weights, const float* d_comp, const float* d_weights,
                           float* d_sdf, float* d_normal, float* d_rgb, float* d_inv_s,
                           void* stream);
/* The same, and the liveness bitmap of the texture backward on the way: bit (i >> 5) & 31 of word
 * i >> 10 of live_halves is set where some d_rgb of sample i is not zero (behind the front surface
 * the weights are exactly 0.0f).  (n + 1023) / 1024 words, zeroed by the caller. */
int dsu_neus_composite_bwd_live(const float* sdf, const float* normal, const float* rgb,
                                const float* rays_d, const float* t_starts, const float* t_ends,
                                const int32_t* offsets, const int32_t* counts, int64_t n_rays,
                                const float* inv_s, float cos_anneal_ratio, const float* alpha,
                                const float* weights, const float* d_comp, const float* d_weights,
                                float* d_sdf, float* d_normal, float* d_rgb, float* d_inv_s,
                                uint32_t* live_halves, void* stream);
/* normal = F.normalize(sdf_grad) and the texture-MLP input cat(feature, normal) (neus.py:143,
 * texture.py:22) in one pass; and its backward. */
int dsu_shade_prep_fwd(const float* grad, const float* feature, int64_t n, float* normal,
                       float* tex_in, void* stream);
int dsu_shade_prep_bwd(const float* grad, const float* d_normal, const float* d_tex_in, int64_t n,
                       float* d_grad, float* d_feature, void* stream);

/* VolumeRadiance (2_charactor_reconstructor/instant_nsr/models/texture.py:9-30): VanillaMLP
 * 16 -> 64 -> 64 -> 3, ReLU, no weight norm (models/network_utils.py:94-138), then sigmoid.
 * Weights row-major (out, in) f32 as nn.Linear stores them (texture.network.layers.{0,2,4}).
 *   dsu_texture_fwd: rgb (n,3) = sigmoid(MLP(tex_in (n,16)))
 *   dsu_texture_bwd: d_tex_in (n,16) written; g_* accumulated (+=) with the parameter
 *     gradients; `rgb` is the forward output (sigmoid' = rgb (1 - rgb)); hidden activations are
 *     recomputed.  workspace: dsu_texture_bwd_workspace_bytes(n) bytes of device memory. */
typedef struct dsu_tex_mlp {
  const float *w0, *b0, *w1, *b1, *w2, *b2;
} dsu_tex_mlp;
int dsu_texture_fwd(const dsu_tex_mlp* mlp, const float* tex_in, int64_t n, float* rgb,
                    void* stream);
int64_t dsu_texture_bwd_workspace_bytes(int64_t n);
int dsu_texture_bwd(const dsu_tex_mlp* mlp, const float* tex_in, const float* rgb,
                    const float* d_rgb, int64_t n, float* d_tex_in, float* g_w0, float* g_b0,
                    float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* The same two calls with the shading glue of neus.py:143 / texture.py:22 inside: the input row is
 * cat(feature (n,13), normalize(sdf_grad (n,3))) built in the kernel (`normal` (n,3) is written for
 * the compositing kernels), and the backward pulls the row's gradient back through cat / normalize
 * itself: d_feature (n + tail_rows, 13) (the tail rows zeroed), d_grad (n,3) =
 * (dn - n (n.dn)) / |sdf_grad| with dn = d_row[13:16] + d_normal (d_normal may be NULL).  Replaces
 * dsu_shade_prep_fwd + dsu_texture_fwd and dsu_texture_bwd + dsu_shade_prep_bwd.
 * h1_mask (may be NULL): the forward also writes the ReLU pattern of hidden layer 1, (n, 2) uint32,
 * word h of a sample = its hidden units 32 T + (r & 3) + 8 (r >> 2) + 4 h, bit 16 T + r. */
int dsu_texture_fwd_shaded_m(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                             int64_t n, float* normal, float* rgb, uint32_t* h1_mask, void* stream);
int dsu_texture_bwd_shaded(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                           const float* rgb, const float* d_rgb, const float* d_normal, int64_t n,
                           int64_t tail_rows, float* d_grad, float* d_feature, float* g_w0,
                           float* g_b0, float* g_w1, float* g_b1, float* g_w2, float* g_b2,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* dsu_texture_bwd_shaded without its final launch: the per-workgroup partial parameter gradients
 * stay in `workspace` and `red` receives partials / nblocks / stride / n of the deferred sum; the
 * caller sets red->map (device copy of dsu_texture_partial_map) and red->base (a contiguous
 * [w0 | b0 | w1 | b1 | w2 | b2] gradient block, accumulated +=) and hands the record to a launch that
 * carries it out (dsu_sdf_fd_bwd_sorted_fold).  dsu_texture_partial_map fills map_host (may be NULL)
 * and returns the number of entries.
 * h1_mask (may be NULL): the pattern dsu_texture_fwd_shaded_m wrote.  The backward then recomputes
 * layer 1 with three bf16 products per f32 product (2^-16 relative on the activations) while the
 * masks stay the forward's, bit for bit.  NULL = exact f32 recompute, as in dsu_texture_bwd_shaded. */
int32_t dsu_texture_partial_map(int32_t* map_host);
int dsu_texture_bwd_shaded_partials_m(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                                      const float* rgb, const float* d_rgb, const float* d_normal,
                                      int64_t n, int64_t tail_rows, float* d_grad, float* d_feature,
                                      const uint32_t* h1_mask, void* workspace, int64_t workspace_bytes,
                                      dsu_partial_reduce* red, void* stream);
/* Dead halves.  A 32-sample half of [0, n) whose d_rgb rows are all zero contributes exact zeros to
 * d_feature, to the MLP's part of d_grad and to every parameter gradient: the backward kernels skip
 * its recompute and products, write d_feature = 0 and d_grad from d_normal alone, and hand every
 * workgroup (and every wave of it) a contiguous run of halves with an equal share of the LIVE ones
 * (csrc/tex_partition.h).  The entry points above find the live halves from d_rgb themselves (one small
 * launch; the bitmap sits behind the partial vectors in `workspace`); this one takes the bitmap
 * dsu_neus_composite_bwd_live filled.  The bit decides: a set bit on a dead half only costs its time, a
 * clear bit on a half with a non-zero d_rgb loses that half's gradients.  Beyond 2 097 152 samples the
 * bitmap is not read (static ranges, dead halves found from d_rgb). */
int dsu_texture_bwd_shaded_partials_live(const dsu_tex_mlp* mlp, const float* feature, const float* grad,
                                         const float* rgb, const float* d_rgb, const float* d_normal,
                                         int64_t n, int64_t tail_rows, float* d_grad, float* d_feature,
                                         const uint32_t* h1_mask, const uint32_t* live_halves,
                                         void* workspace, int64_t workspace_bytes,
                                         dsu_partial_reduce* red, void* stream);
/* Host only: the runs of halves the backward kernel gives its workgroups and waves for a bitmap of
 * n_halves bits (host memory) and a grid of `parts` workgroups of `waves` waves.  runs: parts x waves
 * pairs (first half, one past the last), in order. */
int dsu_texture_live_partition(const uint32_t* live_halves, int64_t n_halves, int32_t parts,
                               int32_t waves, int32_t* runs);

/* OrthoNeuSSystem.preprocess_data (systems/neus_ortho.py:26-82) for n sampled (view, y, x)
 * triples (int64, drawn by the caller): c2w gather, get_ortho_rays (models/ray_utils.py:36-58),
 * colour / normal / mask / view-weight gathers, cosines = cosine_similarity(rays_d, normal,
 * eps=1e-6), rays = [rays_o | normalize(rays_d)].  Dataset tensors are the resident
 * (V,H,W,*) f32 arrays of OrthoDatasetBase.setup (datasets/ortho.py:99-151). */
int dsu_ortho_ray_batch(const int64_t* index, const int64_t* x, const int64_t* y, int64_t n,
                        const float* c2w, const float* origins, const float* directions,
                        const float* images, int32_t image_channels, const float* normals,
                        const float* masks, const float* view_weights, int32_t H, int32_t W,
                        float* rays, float* rgb, float* normal, float* mask, float* cosines,
                        float* vw, void* stream);

/* The same launch also writing rays[:, :3] and rays[:, 3:] as two contiguous (n,3) arrays (both or
 * neither may be NULL). */
int dsu_ortho_ray_batch_split(const int64_t* index, const int64_t* x, const int64_t* y, int64_t n,
                              const float* c2w, const float* origins, const float* directions,
                              const float* images, int32_t image_channels, const float* normals,
                              const float* masks, const float* view_weights, int32_t H, int32_t W,
                              float* rays, float* rgb, float* normal, float* mask, float* cosines,
                              float* vw, float* rays_o, float* rays_d, void* stream);

/* Ray-level loss terms of OrthoNeuSSystem.training_step
 * (2_charactor_reconstructor/instant_nsr/systems/neus_ortho.py:94-133 with
 * systems/criterions.py:4-27) and their gradient w.r.t. the raw composite
 * comp (R,8) = [opacity, depth, rgb(3), sum w*normal(3)], in ONE launch:
 *   terms[0] rgb_mse  = ranking(sum_c (rgb-gt)^2 | fg, rgb_p_ratio, mean) * lambda_rgb_mse
 *   terms[1] rgb_l1   = ranking(sum_c |rgb-gt|   | fg, rgb_p_ratio, mean) * lambda_rgb_l1
 *   terms[2] normal   = ranking(1-cos(normalize(n), gt) [* exp|cos'| / sum exp|cos'| if
 *                       geo_aware] | fg, normal_p_ratio, view_weights, sum|mean) * lambda_normal
 *   terms[3] mask     = ranking(BCE(clamp(opacity,1e-3,1-1e-3), mask) | all, mask_p_ratio,
 *                       view_weights, mean) * lambda_mask
 * fg = mask > 0 and cosines < -0.1.  ranking() reproduces criterions.py:16-27 exactly,
 * including its selection rule (sorted errors indexed with the original positions of the k
 * smallest; k = int(ratio * count)).  n_rays <= DSU_RAY_LOSS_MAX_RAYS. */
#define DSU_RAY_LOSS_MAX_RAYS 8192
typedef struct dsu_ray_loss_cfg {
  double rgb_p_ratio, normal_p_ratio, mask_p_ratio;
  float lambda_rgb_mse, lambda_rgb_l1, lambda_normal, lambda_mask;
  int32_t geo_aware;
  int32_t reserved;
} dsu_ray_loss_cfg;
int dsu_ray_losses(const float* comp, const float* rgb, const float* normal, const float* mask,
                   const float* cosines, const float* view_weights, int32_t n_rays,
                   const dsu_ray_loss_cfg* cfg, float* terms, float* d_comp, void* stream);

/* Sample-level terms (neus_ortho.py:118-151) over the concatenated evaluation
 * [n_samples ray samples | n_random random points | n_random perturbed copies]:
 *   terms[0] eikonal       = mean_i (|grad_i| - 1)^2            * lambda_eikonal   (samples)
 *   terms[1] sparsity      = mean_r exp(-scale |sdf_r|)         * lambda_sparsity  (random)
 *   terms[2] normal_smooth = mean_{r,c} |grad_r - grad_perturbed_r| * lambda_smooth
 * and their gradients: d_grad_all[:n_samples] += eikonal part when accumulate_prefix != 0
 * (the compositing/shading backward has already written it; d_sdf_all[:n_samples] is left
 * untouched) or = when 0 (then d_sdf_all[:n_samples] = 0); the random / perturbed rows of
 * d_sdf_all and d_grad_all are written.  accumulate_prefix bit 1 (value 2): `terms` was zeroed by
 * the caller (otherwise this call zeroes it first). */
int dsu_sample_losses(const float* sdf_all, const float* grad_all, int64_t n_samples,
                      int64_t n_random, float lambda_eikonal, float lambda_sparsity,
                      float sparsity_scale, float lambda_smooth, int32_t accumulate_prefix,
                      float* d_sdf_all, float* d_grad_all, float* terms, void* stream);

/* ------------------------------------------------------------------------------------
 * Style translator (3_style_translator/training/models.py).
 * ---------------------------------------------------------------------------------- */

/* generate_coordinates (models.py:551-604): the 18-channel fixed offset map for an (H,W)
 * image, written as (18,H,W) f32 (batch broadcast is the caller's view). */
int dsu_ric_offsets(int32_t H, int32_t W, float* offsets, void* stream);

/* torchvision.ops.deform_conv2d(input, offset, weight, padding=(1,1)) for a 3x3 kernel,
 * stride 1, dilation 1, one offset group, no bias, no mask (call sites models.py:302-351).
 * input (B,C,H,W) f32; offset (18,H,W) f32 shared over the batch (offset_batch_stride=0)
 * or per image; weight (O,C,3,3); out (B,O,H,W).
 * Optional fused epilogue (scale/shift per output channel = folded eval BatchNorm, then
 * act: 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 tanh), optional residual added last.
 * in_relu != 0 applies ReLU to the input as it is read (the resnet blocks' leading
 * nonlinearity_0, models.py:321) without a separate pass. */
int dsu_deform_conv3x3_fwd(const float* input, const float* offset, int64_t offset_batch_stride,
                           const float* weight, int32_t B, int32_t C, int32_t H, int32_t W,
                           int32_t O, int32_t in_relu, const float* ep_scale,
                           const float* ep_shift, int32_t act, const float* residual, float* out,
                           void* stream);

/* nn.Conv2d forward, NCHW f32, square kernel k in {1,3,7} with stride in {1,2} (GeneratorJ,
 * models.py:41-129; PerceptualVGG19 features 0/2/5, models.py:536-544) or k = 4 with stride in
 * {1,2} (DiscriminatorN_IN, models.py:441-462), zero padding, same fused epilogue.  bias may be
 * NULL. */
int dsu_conv2d_fwd(const float* input, const float* weight, const float* bias, int32_t B,
                   int32_t C, int32_t H, int32_t W, int32_t O, int32_t k, int32_t stride,
                   int32_t pad, int32_t in_relu, const float* ep_scale, const float* ep_shift,
                   int32_t act, const float* residual, float* out, void* stream);

/* Evaluation-time variants of the two convolutions above on the bf16 MFMA with "bf16 x 3"
 * operands (x = x_hi + x_mid + O(2^-16 |x|); products a_hi b_hi + a_hi b_mid + a_mid b_hi with
 * f32 accumulation: relative error ~2^-15 per product — finer than the TF32 arithmetic
 * torch.backends.cudnn.allow_tf32 = True gives the reference's nn.Conv2d by default).  Same
 * tensors, epilogue and argument meaning; the weight comes packed:
 *   dsu_conv_x3_packed_elems(O, C, k)   number of uint16 elements of EACH of w_hi / w_mid,
 *   dsu_conv_x3_pack_weights            (O,C,k,k) f32 -> (roundup(O,32), ceil(C/16), k*k, 16) bf16
 *                                       hi and mid parts, zero padded; 16-byte aligned buffers.
 * k in {1,3,7} (stride 2 for k = 3 only); others DSU_EUNSUP.  Used by GeneratorJ / GeneratorJ_RIC
 * in eval mode (models.py:41-129, :302-351); training keeps the exact-f32 kernels. */
int64_t dsu_conv_x3_packed_elems(int32_t O, int32_t C, int32_t k);
int dsu_conv_x3_pack_weights(const float* weight, int32_t O, int32_t C, int32_t k, uint16_t* w_hi,
                             uint16_t* w_mid, void* stream);
int dsu_deform_conv3x3_fwd_x3(const float* input, const float* offset, int64_t offset_batch_stride,
                              const uint16_t* w_hi, const uint16_t* w_mid, int32_t B, int32_t C,
                              int32_t H, int32_t W, int32_t O, int32_t in_relu,
                              const float* ep_scale, const float* ep_shift, int32_t act,
                              const float* residual, float* out, void* stream);
int dsu_conv2d_fwd_x3(const float* input, const uint16_t* w_hi, const uint16_t* w_mid,
                      const float* bias, int32_t B, int32_t C, int32_t H, int32_t W, int32_t O,
                      int32_t k, int32_t stride, int32_t pad, int32_t in_relu,
                      const float* ep_scale, const float* ep_shift, int32_t act,
                      const float* residual, float* out, void* stream);

/* Exact-f32 evaluation variants on the same im2col-in-registers structure (f32 MFMA,
 * v_mfma_f32_32x32x2_f32: every product and sum an f32 fmaf, the arithmetic of
 * torchvision.ops.deform_conv2d's im2col + f32 addmm with TF32 off, which is PyTorch's default
 * for matmuls: models.py:302-351 via test_stage1.py:42-71; and of the f32 ONNX session behind
 * mv.py:17-18,134-150).  Same tensors, epilogue and argument meaning as dsu_deform_conv3x3_fwd /
 * dsu_conv2d_fwd; the weight comes packed as (roundup(O,32), ceil(C/16), k*k, 16) f32, zero padded
 * (dsu_conv_x3_packed_elems(O, C, k) floats, 16-byte aligned).  C % 8 == 0 (callers pad with zero
 * channels); k in {1,3} (stride 2 for k = 3 only), others DSU_EUNSUP -> dsu_conv2d_fwd. */
int dsu_conv_f32p_pack_weights(const float* weight, int32_t O, int32_t C, int32_t k, float* w_packed,
                               void* stream);
int dsu_deform_conv3x3_fwd_f32p(const float* input, const float* offset, int64_t offset_batch_stride,
                                const float* w_packed, int32_t B, int32_t C, int32_t H, int32_t W,
                                int32_t O, int32_t in_relu, const float* ep_scale,
                                const float* ep_shift, int32_t act, const float* residual, float* out,
                                void* stream);
int dsu_conv2d_fwd_f32p(const float* input, const float* w_packed, const float* bias, int32_t B,
                        int32_t C, int32_t H, int32_t W, int32_t O, int32_t k, int32_t stride,
                        int32_t pad, int32_t in_relu, const float* ep_scale, const float* ep_shift,
                        int32_t act, const float* residual, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Style translator, per-character TRAINING (3_style_translator/training/trainers.py:140-192:
 * autograd through GeneratorJ / GeneratorJ_RIC, DiscriminatorN_IN and PerceptualVGG19 on
 * batch_size x C x 32 x 32 patches, configs/config_stage{1,2}.yaml).  SURVEY.md 8f-1.
 * The data gradient of nn.Conv2d is dsu_conv2d_fwd on dout with flipped/transposed weights.
 * ---------------------------------------------------------------------------------- */

/* Fixed sampling table of the 3x3 deformable convolution for an (18,H,W) offset map shared by
 * the batch (models.py:297-300: coords_k depend on the resolution only): 9 records per pixel
 * with the four clamped corner offsets and bilinear weights, computed with the forward
 * kernel's own arithmetic.  table: caller-owned device buffer of dsu_deform_tap_table_bytes
 * (0 = invalid arguments). */
int64_t dsu_deform_tap_table_bytes(int32_t H, int32_t W);
int dsu_deform_tap_table(const float* offset, int32_t H, int32_t W, void* table, void* stream);

/* Weight gradient of nn.Conv2d (tap_table == NULL; k in {1,3,4,7}, any stride/pad) or of
 * torchvision.ops.deform_conv2d with the fixed offsets of tap_table (k = 3, stride 1, pad 1):
 *   dweight[o][c][ty][tx] (= or +=, accumulate) sum_{b,pixel} dout[b][o][pixel] * col[b][c][tap][pixel]
 * input (B,C,H,W), dout (B,O,OH,OW), O <= 128.  workspace: per-slice partial sums, size from
 * dsu_conv2d_wgrad_workspace_bytes (same B,C,O,k and the OUTPUT size OH,OW); summed in a
 * fixed order, so results are run-to-run identical. */
int64_t dsu_conv2d_wgrad_workspace_bytes(int32_t deform, int32_t B, int32_t C, int32_t O,
                                         int32_t OH, int32_t OW, int32_t k);
int dsu_conv2d_wgrad(const float* input, const float* dout, const void* tap_table, int32_t B,
                     int32_t C, int32_t H, int32_t W, int32_t O, int32_t k, int32_t stride,
                     int32_t pad, float* workspace, float* dweight, int32_t accumulate,
                     void* stream);

/* Input gradient of the fixed-offset deformable convolution, second half: dcol (planes = B*C,
 * 9, npix) = W^T dout (a 1x1 dsu_conv2d_fwd with the (C*9, O) transposed weight) is pulled back
 * through the transposed sampling operator given as CSR over INPUT pixels: row q lists
 * src = tap * npix + output_pixel and the bilinear weight of every sample that read q.
 *   dx[plane][q] = sum_e wgt[e] * dcol[plane][src[e]],  e in [rowptr[q], rowptr[q+1]) */
int dsu_deform_conv3x3_dgrad_gather(const float* dcol, const int32_t* rowptr, const int32_t* src,
                                    const float* wgt, int64_t planes, int32_t npix, float* dx,
                                    void* stream);

/* nn.BatchNorm2d in training mode (instance = 0: statistics over (batch, hw) per channel;
 * running_mean/var, when given, take `stat_updates` momentum updates with the unbiased batch
 * variance) or nn.InstanceNorm2d without affine/running stats (instance = 1, DiscriminatorN_IN
 * models.py:436-439), followed by act (0 none, 1 ReLU, 2 LeakyReLU(0.2)).  x,y (B,C,HW) f32;
 * save_mean/save_invstd: one value per channel (instance = 0) or per (image, channel). */
typedef struct dsu_norm_cfg {
  int32_t batch, channels, hw;
  int32_t instance;
  int32_t act;
  int32_t stat_updates;
  float eps;
  float momentum;
} dsu_norm_cfg;
int dsu_norm_train_fwd(const dsu_norm_cfg* cfg, const float* x, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, float* y,
                       float* save_mean, float* save_invstd, void* stream);
/* Backward of the above through the activation (derivative taken from the output y):
 * dx, and for instance = 0 dgamma/dbeta (C) when non-NULL. */
int dsu_norm_train_bwd(const dsu_norm_cfg* cfg, const float* x, const float* y, const float* dy,
                       const float* gamma, const float* save_mean, const float* save_invstd,
                       float* dx, float* dgamma, float* dbeta, void* stream);

/* out[c] = sum over (b, hw) of x[b][c][hw]: the bias gradient of a convolution. */
int dsu_channel_sum(const float* x, int32_t B, int32_t C, int32_t HW, float* out, void* stream);

/* Activations (act: 1 ReLU, 2 LeakyReLU(0.2), 3 tanh) and their backward from the OUTPUT y. */
int dsu_act_fwd(const float* x, float* y, int64_t n, int32_t act, void* stream);
int dsu_act_bwd(const float* dy, const float* y, float* dx, int64_t n, int32_t act, void* stream);

/* nn.MaxPool2d(2,2) (GeneratorJ_RIC.maxpool models.py:214, VGG19 features[4]) on `planes`
 * images of H x W (H, W even); backward routes to the first maximum of each window. */
int dsu_maxpool2_fwd(const float* x, float* y, int64_t planes, int32_t H, int32_t W, void* stream);
int dsu_maxpool2_bwd(const float* x, const float* dy, float* dx, int64_t planes, int32_t H,
                     int32_t W, void* stream);

/* nn.Upsample(scale_factor=2) nearest (UpsamplingLayer, models.py:8-14): H x W -> 2H x 2W. */
int dsu_upsample2_fwd(const float* x, float* y, int64_t planes, int32_t H, int32_t W,
                      void* stream);
int dsu_upsample2_bwd(const float* dy, float* dx, int64_t planes, int32_t H, int32_t W,
                      void* stream);

/* nn.L1Loss (kind 0) / nn.MSELoss (kind 1) terms of trainers.py:97-135 before the division by
 * n: partial256[256] partial sums of |x - t| or (x - t)^2 (t = target[i], or target_const when
 * target is NULL); grad (may be NULL) = d/dx of (grad_scale * sum). */
int dsu_pair_loss(const float* x, const float* target, float target_const, int64_t n,
                  int32_t kind, float grad_scale, float* grad, float* partial256, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-view diffusion UNet (2_charactor_reconstructor/mvdiffusion/models).
 * ---------------------------------------------------------------------------------- */

/* xformers.ops.memory_efficient_attention(q, k, v, attn_bias=None) as called by
 * XFormersMVAttnProcessor (transformer_mv2d.py:802) and XFormersJointAttnProcessor (:890),
 * WITHOUT materialising the repeated / concatenated K,V (transformer_mv2d.py:785-786,
 * 878-883): the key/value sequence of query batch b is the concatenation of S segments of
 * seg_len tokens; segment s of query batch b lives at batch index seg_batch[b*S + s] of K/Vt.
 *   q, out : f16, element strides q_strides/o_strides = {batch, token, head}, d contiguous
 *   k      : f16, strides {batch, token, head}, d contiguous
 *   vt     : f16 V TRANSPOSED per head, strides {batch, head, d}, token contiguous
 *   d in {40, 64, 80, 160}; scale = softmax scale (1/sqrt(d) for xformers' default).
 * f32 accumulation, f16 output. */
int dsu_mv_attention_fwd(const void* q, const void* k, const void* vt, void* out,
                         const int32_t* seg_batch, int32_t Bq, int32_t H, int32_t Nq, int32_t d,
                         int32_t S, int32_t seg_len, const int64_t* q_strides,
                         const int64_t* k_strides, const int64_t* vt_strides,
                         const int64_t* o_strides, float scale, void* stream);

/* nn.Conv2d forward on NHWC f16 activations with f32 accumulation (diffusers ResnetBlock2D /
 * Downsample2D / Upsample2D / conv_in / conv_out convolutions, unet_mv2d_blocks.py:528,649,
 * 688,798,839; unet_mv2d_condition.py:290,623).
 *   input (B,H,W,C) f16; weight_okc (O, k*k, C) f16 = the nn.Conv2d weight (O,C,k,k)
 *   permuted to (O,k,k,C) once by the caller; bias (O) f16 or NULL.
 *   upsample2x != 0: the convolution reads the nearest-neighbour x2 upsampled input
 *   (Upsample2D = F.interpolate(scale 2, nearest) + conv) without materialising it.
 *   addvec (B,O) f16 or NULL: added per image and channel (time-embedding projection of
 *   ResnetBlock2D); residual (B,OH,OW,O) f16 or NULL: added last.  C % 8 == 0.
 * Split-K: the k*k*C reduction is divided over `split_k` workgroups per output tile (f32 partials
 * in `workspace`, summed by a second kernel that also applies bias / addvec / residual).  For the
 * 8x8 and 4x4 levels of the UNet the output tiles alone occupy 20-120 of the 256 CUs.
 * dsu_conv2d_nhwc_f16_split_k returns the factor the library would pick (1 = plain kernel: no
 * workspace needed), dsu_conv2d_nhwc_f16_workspace_bytes the f32 scratch it needs. */
int32_t dsu_conv2d_nhwc_f16_split_k(int32_t B, int32_t H, int32_t W, int32_t C, int32_t O,
                                    int32_t k, int32_t stride, int32_t pad, int32_t upsample2x);
int64_t dsu_conv2d_nhwc_f16_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t O, int32_t k,
                                            int32_t stride, int32_t pad, int32_t upsample2x,
                                            int32_t split_k);
/* The reduction can also run inside the kernel: `tile_counters` is a caller-owned, ZEROED int32
 * buffer of at least (output tiles) entries that stays allocated between calls; the last workgroup
 * of a tile to finish sums the split_k partial tiles (in z order) and runs the epilogue, then
 * resets the tile's counter — no separate reduce launch.  One buffer serves every launch issued
 * on ONE stream (launches on different streams need their own).  NULL = the reduce kernel. */
int dsu_conv2d_nhwc_f16_fwd_fx(const void* input, const void* weight_okc, const void* bias,
                               int32_t B, int32_t H, int32_t W, int32_t C, int32_t O, int32_t k,
                               int32_t stride, int32_t pad, int32_t upsample2x,
                               const void* addvec, const void* residual, void* out,
                               int32_t split_k, void* workspace, int64_t workspace_bytes,
                               int32_t* tile_counters, int64_t n_counters, void* stream);

/* nn.Linear forward of the UNet's transformer blocks and embedding MLPs on the same MFMA kernel
 * (a 1x1 convolution over M rows): Attention.to_q / to_k / to_out, FeedForward.net.2,
 * TransformerMV2DModel.proj_in / proj_out, TimestepEmbedding, ResnetBlock2D.time_emb_proj
 * (transformer_mv2d.py:447-483, 304-370; unet_mv2d_condition.py:313-319,374).
 *   x (M, K) f16 row-major, w (N, K) f16 = the nn.Linear weight as stored, bias (N) or NULL,
 *   residual (M, N) or NULL (added last), out (M, N) f16, f32 accumulation.  K % 8 == 0.
 *   tokens_per_image > 0 (M a multiple of it): out is written TRANSPOSED per image,
 *   out[(m / tokens) * N * tokens + n * tokens + m % tokens] — Attention.to_v, so that
 *   dsu_mv_attention_fwd reads V^T rows in place; no residual / split-K in that form.
 *   split_k / workspace / tile_counters as for dsu_conv2d_nhwc_f16_fwd_fx (dsu_gemm_f16_split_k =
 *   the library's choice, dsu_gemm_f16_workspace_bytes = f32 scratch). */
int32_t dsu_gemm_f16_split_k(int64_t M, int32_t K, int32_t N);
int64_t dsu_gemm_f16_workspace_bytes(int64_t M, int32_t N, int32_t split_k);
int dsu_gemm_f16_fwd_fx(const void* x, const void* w, const void* bias, int64_t M, int32_t K,
                        int32_t N, const void* residual, void* out, int32_t tokens_per_image,
                        int32_t split_k, void* workspace, int64_t workspace_bytes,
                        int32_t* tile_counters, int64_t n_counters, void* stream);
/* diffusers FeedForward(activation_fn="geglu") first layer fused with its activation
 * (transformer_mv2d.py:483 -> GEGLU.forward): w (2N, K), bias (2N) or NULL;
 * out (M, N) = (x w[:N]^T + b[:N]) * gelu_erf(x w[N:]^T + b[N:]); both halves are rounded to f16
 * before the product, as the unfused nn.Linear output is.  K % 8 == 0, N % 4 == 0. */
int dsu_gemm_geglu_fwd(const void* x, const void* w, const void* bias, int64_t M, int32_t K,
                       int32_t N, void* out, void* stream);

/* nn.GroupNorm(G, C, eps) on NHWC f16 (+ optional fused SiLU): diffusers ResnetBlock2D
 * norm1/norm2 + nonlinearity, TransformerMV2DModel.norm (transformer_mv2d.py:304),
 * conv_norm_out + conv_act (unet_mv2d_condition.py:1046-1048).  x/out (B,HW,C) f16;
 * gamma/beta (C) f16; stats_ws: caller-owned f32 scratch of B*G*2 floats.  out must not alias
 * x: the statistics are sums of x - K, K being x[n, 0, g*C/G], and the apply pass reads K from x
 * while other threads write out. */
int dsu_groupnorm_nhwc_f16(const void* x, const void* gamma, const void* beta, int32_t B,
                           int32_t HW, int32_t C, int32_t G, float eps, int32_t silu,
                           float* stats_ws, void* out, void* stream);

/* nn.LayerNorm(C) over the last dimension of (rows, C) f16 (BasicMVTransformerBlock
 * norm1 / norm_joint_mid / norm2 / norm3, transformer_mv2d.py:447-519). */
int dsu_layernorm_f16(const void* x, const void* gamma, const void* beta, int64_t rows,
                      int32_t C, float eps, void* out, void* stream);

/* diffusers GEGLU (FeedForward activation_fn="geglu", transformer_mv2d.py:483):
 * h (rows, 2*D) f16 = proj output; out[r][j] = h[r][j] * gelu_erf(h[r][D+j]). */
int dsu_geglu_f16(const void* h, int64_t rows, int32_t D, void* out, void* stream);

/* Classifier-free guidance around the UNet call of MVDiffusionImagePipeline.__call__
 * (2_charactor_reconstructor/mvdiffusion/pipelines/pipeline_mvdiffusion_image.py, guidance_scale != 1).
 *
 * dsu_cfg_model_input — the UNet input of one step (:180 and :465-468: `cat([latents] * 2)`,
 * `cat([.., cat([zeros_like(image_latents), image_latents])], dim=1)`) in one pass:
 *   latents, image_latents (B, row_elems) f16, row_elems = C*h*w of one latent (C = 4);
 *   out (2B, 2*row_elems) f16: rows 0..B-1 = [latents[b] | 0], rows B..2B-1 =
 *   [latents[b] | image_latents[b]].  out must not alias an input.  Any row_elems >= 0.
 *
 * dsu_ddim_cfg_step — guidance (:476-477) and DDIMScheduler.step (diffusers 0.19.3, epsilon
 * prediction, clip_sample False) in one pass over n = B*C*h*w elements:
 *   noise_pred (2n) f16 = the UNet output, unconditional rows first; latents (n) f16;
 *   variance_noise (n) f16 or NULL (NULL: no noise term, whatever std_dev is);
 *   sqrt_a_t = sqrt(alphas_cumprod[t]), sqrt_1m_a_t = sqrt(1 - alphas_cumprod[t]),
 *   sqrt_a_prev = sqrt(alphas_cumprod[t_prev]), std_dev = eta * sqrt(variance): the host's, as f32.
 *   Per element, from the f16 inputs and the f32 scalars, in this operand order:
 *     n    = u + g * (c - u)                        u = noise_pred[i], c = noise_pred[n + i]
 *     x0   = (x - sqrt_1m_a_t * n) / sqrt_a_t       x = latents[i]
 *     prev = sqrt_a_prev * x0 + dir * n             dir = sqrt(1 - sqrt_a_prev^2 - std_dev^2)
 *     prev = prev + std_dev * variance_noise[i]
 *     out[i] = (f16)prev                            the only rounding to f16
 *   evaluated in double, so that out is the rounding of the rule's exact value to within the f16
 *   conversion: the two terms of prev are of order 1 each and can cancel, and f32 roundings of them
 *   (~1e-7) would exceed the f16 spacing of a result near zero (6e-8).  (The reference forms n in
 *   f16 on its GPU and rounds it before the step, whose arithmetic is f32; here n is not rounded.)
 *   DSU_EINVAL: sqrt_a_t <= 0, std_dev < 0, a radicand below -1e-6 (between that and 0: dir = 0),
 *   out aliasing an input.  Any n >= 0. */
int dsu_cfg_model_input(const void* latents, const void* image_latents, int32_t B,
                        int64_t row_elems, void* out, void* stream);
int dsu_ddim_cfg_step(const void* noise_pred, const void* latents, const void* variance_noise,
                      int64_t n, float guidance_scale, float sqrt_a_t, float sqrt_1m_a_t,
                      float sqrt_a_prev, float std_dev, void* out, void* stream);

/* cv2.inpaint(img, mask, radius, cv2.INPAINT_TELEA) on an 8-bit 3-channel HOST image
 * (1_lama_contour_remover/predict.py:63: the predicted contour pixels and the background are
 * filled from the character's own pixels).  Host code, as in the reference: fast marching is a
 * strictly ordered front propagation.  img/out (rows, cols, 3) u8, mask (rows, cols) u8
 * (non-zero = fill); rows, cols >= 3. */
int dsu_inpaint_telea_u8c3(const uint8_t* img, const uint8_t* mask, int32_t rows, int32_t cols,
                           int32_t radius, uint8_t* out);

/* torch.optim.AdamW step on a range of the hash-table parameters (the optimizer the reference
 * configures in configs/neuralangelo-ortho-wmask.yaml:96-110 -> systems/utils.py parse_optimizer;
 * torch's update: p -= lr*wd*p; m = lerp(m, g, 1-b1); v = b2*v + (1-b2)*g*g;
 * p -= (lr / bias_correction1) * m / (sqrt(v) / bias_correction2_sqrt + eps)), fused with the f16
 * image rewrite (img_f16[i] = half(p[i])) and the gradient reset (g = 0).  n floats, n % 4 == 0,
 * 16-byte aligned pointers.  dsu_table_decay: p *= factor (+ image) — the accumulated
 * `1 - lr*wd` factors of steps in which a level of the progressive grid was still masked. */
int dsu_table_adamw(float* p, float* g, float* m, float* v, void* img_f16, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, float bias_correction1,
                    float bias_correction2_sqrt, void* stream);
int dsu_table_decay(float* p, void* img_f16, int64_t n, float factor, void* stream);
/* The same AdamW update for up to DSU_ADAMW_MAX_TENSORS small tensors in one launch (the SDF MLP,
 * texture MLP and variance parameters of the three optimizer groups, each with its group's lr and
 * its own bias corrections); `tensors` is a HOST array. */
#define DSU_ADAMW_MAX_TENSORS 24
typedef struct {
  float* p; float* g; float* m; float* v;
  int64_t n;
  float lr, bias_correction1, bias_correction2_sqrt, reserved;
} dsu_adamw_tensor;
int dsu_adamw_multi(const dsu_adamw_tensor* tensors, int32_t count, float beta1, float beta2,
                    float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------------------------
 * Native driver of ONE NSR optimisation step: OrthoNeuSSystem.training_step
 * (2_charactor_reconstructor/instant_nsr/systems/neus_ortho.py:79-169) over
 * NeuSModelTextureMLP.forward_ (instant_nsr/models/neus.py:114-196), the ray batch of
 * preprocess_data (neus_ortho.py:26-77) and the AdamW update of the SDF-MLP / texture-MLP /
 * variance groups (configs/neuralangelo-ortho-wmask.yaml:96-127) sequenced by the library
 * itself: the host-side cost of a step is ~20 kernel launches issued from C instead of ~1.4 ms
 * of interpreter work (as long as the step's device time).  The hash table's own update stays the
 * caller's bookkeeping (levels, lazy decay) with the launch itself inside the step; the occupancy-grid
 * refresh of every 16th step is dsu_nsr_driver_occ_refresh, called by the caller before that step.
 *
 * All device memory is the caller's: parameters, dataset tensors and ONE workspace of
 * dsu_nsr_driver_workspace_bytes(cfg) bytes.  The driver object owns a side stream, three
 * events and 16 bytes of pinned host memory (the next step's rays are drawn, marched, packed
 * and Morton-sorted on the side stream while this step's backward runs; the sample total
 * reaches the host through the pinned words).  Random draws: counter-based Philox4x32-10 keyed
 * by (seed, step) — reproducible, independent of the step's timing; tests inject their own.
 * ---------------------------------------------------------------------------------- */
typedef struct dsu_nsr_driver dsu_nsr_driver;
typedef struct dsu_nsr_driver_cfg {
  dsu_hashgrid_cfg grid;
  float radius;              /* model.radius (1.0) */
  float render_step_size;    /* 1.732 * 2 * radius / num_samples_per_ray (neus.py:59) */
  int32_t cap_points;        /* capacity of the packed sample buffers (2^19: 2x the target) */
  int32_t cap_rays;          /* max_train_num_rays (8192), <= DSU_RAY_LOSS_MAX_RAYS */
  int32_t n_random;          /* 2048 regulariser points (neus.py:155) */
  int32_t sort_bits;         /* Morton bits per axis for the evaluation order (0 = ray-major) */
  int32_t dynamic_ray_sampling; /* neus_ortho.py:88-92 */
  int32_t train_num_samples; /* train_num_rays * num_samples_per_ray (2^18) */
  /* resident dataset (datasets/ortho.py:99-151), f32 contiguous */
  const float *c2w, *origins, *directions, *images, *normals, *masks, *view_weights;
  int32_t V, H, W, image_channels;
  /* parameters (f32, device): SDF MLP with weight norm (network_utils.py:113-138), texture MLP,
   * variance scalar; updated in place */
  float *w0_v, *w0_g, *b0, *w1_v, *w1_g, *b1;
  float* tex[6];
  float* variance;
  /* losses and optimizer (neuralangelo-ortho-wmask.yaml:86-127) */
  dsu_ray_loss_cfg ray_loss;
  float lambda_eikonal, lambda_sparsity, sparsity_scale, lambda_smooth;
  float beta1, beta2, adam_eps, weight_decay;
  uint64_t seed;
  void* workspace;
  int64_t workspace_bytes;
} dsu_nsr_driver_cfg;

typedef struct dsu_nsr_step_args {
  int64_t step;              /* global step: RNG counter and buffer parity */
  int32_t n_rays;            /* rays of this step */
  int32_t prefetch_next;     /* 1: enqueue step+1's samples on the side stream */
  uint32_t active_levels;    /* ProgressiveBandHashGrid.current_level */
  float eps;                 /* finite-difference step (geometry.py:196-215) */
  float cos_anneal_ratio;
  float lr_geometry, lr_texture, lr_variance;
  int32_t adam_step;         /* 1-based count of small-tensor updates (bias corrections) */
  int32_t randomized;        /* stratified jitter on (model.randomized) */
  int32_t refresh_effective; /* 1: parameters were written from outside since the last step */
  int32_t occ_res;
  const uint8_t* occ_binary; /* current occupancy grid (NULL = no pruning) */
  const void* table_img;     /* f16 image of the hash table */
  float* table_grad;         /* (entries,2) f32, accumulated into */
  /* injected draws for THIS step (tests; any NULL = the driver's own draw) */
  const int64_t *inj_index, *inj_x, *inj_y;
  const float *inj_jitter, *inj_pts_random, *inj_perturb;
  /* tests: a whole ray batch as OrthoNeuSSystem.preprocess_data returns it (neus_ortho.py:26-82) in
   * place of the (index, x, y) gathers: rays (n,6) = [origin | direction], rgb (n,3), normal (n,3),
   * mask, cosines, view_weights (n); inj_rays NULL = the dataset path; with it the other five are
   * required */
  const float *inj_rays, *inj_rgb, *inj_normal, *inj_mask, *inj_cosines, *inj_view_weights;
  /* the hash table's AdamW step (dsu_table_adamw), launched by the driver behind the backward:
   * master parameters and moments, number of floats of the active levels, this step's lr and
   * bias corrections (the caller keeps the level / decay bookkeeping); table_p NULL = skip */
  float *table_p, *table_m, *table_v;
  int64_t table_n;
  float table_lr, table_bc1, table_bc2_sqrt, table_eps, table_wd;
  /* outputs (host) */
  int32_t out_n_samples, out_max_count, out_next_n_rays;
  /* optional: 8 floats of DEVICE memory that receive a copy of this step's loss terms (the
   * driver's own two sets are reused two steps later); written by the step's last kernel */
  float* terms_out;
} dsu_nsr_step_args;

/* The random draws of step `step` (neus_ortho.py:31-41: view / pixel triples of the ray batch;
 * nerfacc's stratified jitter; neus.py:155-160: n_random points in [-1,1)^3 and their N(0,1)
 * perturbation) from Philox4x32-10 with key `seed` and counter (element, stream, step): the
 * same (seed, step) gives the same draws whatever ran before.  index in [0,V), x in [0,W), y in
 * [0,H) as int64 (what dsu_ortho_ray_batch takes), jitter in [0,1). */
int dsu_nsr_draws(uint64_t seed, int64_t step, int32_t n_rays, int32_t V, int32_t H, int32_t W,
                  int64_t* index, int64_t* x, int64_t* y, float* jitter, int32_t n_random,
                  float* pts_random, float* perturb, void* stream);
int64_t dsu_nsr_driver_workspace_bytes(const dsu_nsr_driver_cfg* cfg);
int dsu_nsr_driver_create(const dsu_nsr_driver_cfg* cfg, dsu_nsr_driver** out);
void dsu_nsr_driver_destroy(dsu_nsr_driver* d);
/* One step on `main_stream`.  DSU_EUNSUP: the step produced more samples than cap_points (or a
 * ray more than the march scratch row holds); out_n_samples / out_max_count say how many. */
int dsu_nsr_driver_step(dsu_nsr_driver* d, dsu_nsr_step_args* args, void* main_stream);
/* Device pointer to two sets of 8 floats; the set of step s starts at 8 * (s & 1) and holds its 7
 * loss terms: rgb_mse, rgb_l1, normal, mask, eikonal, sparsity, normal_smooth (each already
 * multiplied by its lambda).  A set is reused (zeroed) at the end of the following step. */
const float* dsu_nsr_driver_terms(const dsu_nsr_driver* d);
/* Device pointer to the liveness bitmap of step `step`'s texture backward (one bit per 32-sample half of
 * its out_n_samples ray samples, see dsu_neus_composite_bwd_live): valid from that step's return until
 * the end of the following step. */
const uint32_t* dsu_nsr_driver_live_halves(const dsu_nsr_driver* d, int64_t step);
/* Device pointer to the first (second = 0) or second (1) AdamW moments of the 13 small tensors,
 * 7 902 floats in the order lin0.weight_v (64x23), lin0.weight_g (64), lin0.bias (64),
 * lin1.weight_v (13x64), lin1.weight_g (13), lin1.bias (13), the texture MLP's w0 b0 w1 b1 w2 b2,
 * variance (1).  After ONE step from zeroed moments m / (1 - beta1) is that step's gradient per
 * parameter — how tests/test_gpu_nsr_native.py compares the library-sequenced step with the
 * reference's loss.backward() (systems/neus_ortho.py:79-169). */
const float* dsu_nsr_driver_adam_moments(const dsu_nsr_driver* d, int32_t second);
/* HIP-event timing of the two geometry launches of a step (family 0: dsu_sdf_fd_fwd_sorted,
 * 1: dsu_sdf_fd_bwd_sorted) on the stream they run on: enable = n > 0 times the steps whose index
 * is a multiple of n (resets; 1 = every step — the four event records cost ~28 us of main-queue time
 * per step), 0 disables; then read the number of timed launches, their summed duration and their
 * algorithmic bytes (points x (7 x active_levels x 8 x 4 + 84)). */
int dsu_nsr_driver_timing(dsu_nsr_driver* d, int32_t enable);
int dsu_nsr_driver_timing_read(dsu_nsr_driver* d, int32_t family, int64_t* launches,
                               double* total_ms, double* alg_bytes);
/* Algorithmic MLP flops of the same launches (points x 2 x (7 x 64 x (3 + 2 active_levels) + 64 x 19),
 * three times that for the backward family): these kernels are bound by the f32 arithmetic of
 * VanillaMLP (network_utils.py:107-138), not by the table traffic the contract prices them on. */
int dsu_nsr_driver_timing_flops(dsu_nsr_driver* d, int32_t family, double* mlp_flops);
/* dsu_occgrid_refresh with the driver's own effective weights, inv_s, grid, radius, step size, aabb
 * and seed filled in (args->grid / mlp / inv_s / aabb / seed / radius / render_step_size are
 * ignored): the refresh of every 16th step without leaving the native path. */
int dsu_nsr_driver_occ_refresh(dsu_nsr_driver* d, const dsu_occgrid_refresh_args* args,
                               void* main_stream);

/* mcubes.smooth on the export's binary volume (MarchingCubeHelper.forward,
 * instant_nsr/models/geometry.py:57-58 -> PyMCubes' constrained smoothing): the weighted-Jacobi
 * iteration on the compacted band voxels, float64.  nbr (6, nv) int32: slot of the -x,+x,-y,+y,
 * -z,+z neighbour or -1 (outside the band: folds onto the diagonal); lower / upper (nv) f64: the
 * per-voxel bounds of PyMCubes' projection (`np.maximum(x, lower)` then `np.minimum(x, upper)`;
 * +-infinity = unbounded); x (nv) in/out; y caller-owned scratch of 3*nv doubles.
 * dsu_smooth_iterate runs `iters` iterations x <- proj(w * (-D^-1 R x) + (1 - w) x);
 * dsu_smooth_energy writes dsu_smooth_energy_partials() partial sums of x . Q x (the caller adds
 * them in order and halves: the energy of the stopping test). */
int32_t dsu_smooth_energy_partials(void);
int dsu_smooth_iterate(const int32_t* nbr, int64_t nv, const double* lower, const double* upper,
                       double weight, int32_t iters, double* x, double* y, void* stream);
int dsu_smooth_energy(const int32_t* nbr, int64_t nv, const double* x, double* y,
                      double* partials, void* stream);

/* The same iteration (geometry.py:57-58) with the band compacted brick by brick instead of voxel by
 * voxel: a brick is dsu_smooth_brick_side()^3 voxels (8^3) aligned to the volume grid and is active
 * when it holds a band voxel; partial bricks at the far faces simply lack the voxels outside the
 * volume.  Inside a brick a neighbour is an address, not a slot load.  Per active brick s (nb of them,
 * in ascending order of the linear brick id (bx * nby + by) * nbz + bz, nb* = ceil(side / 8)):
 *   x, y       (nb, 512) f64   the unknowns, z fastest, in two ping-pong copies (absent voxels: 0)
 *   mask       (nb, 8)   u64   word lx, bit ly * 8 + lz: the voxel is a band voxel
 *   nbr6       (nb, 8)   i32   slots of the -x,+x,-y,+y,-z,+z bricks or -1 (entries 6, 7 unused)
 *   x0         (nb, 512) f64   the initial distance, from which the kernel derives PyMCubes' bounds
 *                              (own-side bound = x0, 0 where |x0| < 1, unbounded on the other side)
 *   code       (nb, 512) u8    or instead: index of x0 in values (nvalues <= 255 ascending doubles)
 * A voxel is present when it is inside the volume, in an active brick and its mask bit is set;
 * every other voxel is absent exactly as slot -1 is in dsu_smooth_iterate, and the per-voxel
 * arithmetic is that function's, operand for operand: the results are equal bit for bit.
 *   dsu_smooth_bricks_flags    flags[brick id] = 1 where band (X,Y,Z bytes) has a voxel (flags zeroed
 *                              by the caller, who compacts them: table[brick id] = slot or -1,
 *                              bcoord[slot] = brick id)
 *   dsu_smooth_bricks_gather   band, dist -> x, mask, nbr6 and x0 and / or code (either may be NULL;
 *                              miss[0] is set to 1 when a band value is not in values)
 *   dsu_smooth_bricks_iterate  `iters` iterations in place on x (y: scratch of the same size), one
 *                              launch each; code != NULL selects the byte-coded bounds; direct != 0
 *                              reads neighbours straight from global memory instead of staging the
 *                              brick and its six 2-deep face slabs in LDS (the measured comparison)
 *   dsu_smooth_bricks_energy   partials[s] = sum over brick s of x . Q x, fixed order (the caller
 *                              adds the nb partials in order and halves)
 *   dsu_smooth_bricks_scatter  dist[v] = x where the mask is set, and nowhere else
 * EUNSUP: a volume of 2^22 or more bricks. */
int32_t dsu_smooth_brick_side(void);
int dsu_smooth_bricks_flags(const uint8_t* band, int32_t X, int32_t Y, int32_t Z, int32_t* flags,
                            void* stream);
int dsu_smooth_bricks_gather(const uint8_t* band, const double* dist, int32_t X, int32_t Y, int32_t Z,
                             const int32_t* table, const int32_t* bcoord, int32_t nb,
                             const double* values, int32_t nvalues, double* x, double* x0,
                             uint8_t* code, uint64_t* mask, int32_t* nbr6, int32_t* miss,
                             void* stream);
int dsu_smooth_bricks_iterate(const int32_t* nbr6, const uint64_t* mask, int32_t nb, const double* x0,
                              const uint8_t* code, const double* values, int32_t nvalues,
                              double weight, int32_t iters, int32_t direct, double* x, double* y,
                              void* stream);
int dsu_smooth_bricks_energy(const int32_t* nbr6, const uint64_t* mask, int32_t nb, const double* x,
                             double* partials, void* stream);
int dsu_smooth_bricks_scatter(const double* x, const uint64_t* mask, const int32_t* bcoord, int32_t nb,
                              int32_t X, int32_t Y, int32_t Z, double* dist, void* stream);

/* The signed distance transform mcubes.smooth starts from (PyMCubes: scipy's
 * distance_transform_edt on both classes, +-0.5 at the boundary voxels; geometry.py:57-58), in the
 * band that matters: exact wherever the other class is within R voxels (1 <= R <= 8).
 * binary (X,Y,Z) bytes (non-zero = inside), z minor.  Per voxel d2 = min(squared distance to the
 * nearest voxel of the OTHER class, (R+1)^2) as an integer; the outputs go through two caller-built
 * tables: dist[v] = value_table[(inside ? 0 : (R+1)^2 + 1) + d2] (f64: the caller applies sqrt,
 * the far-field value, the half-voxel shift and the sign on the host), band[v] = band_table[d2].
 * workspace: dsu_volume_band_distance_workspace_bytes(X, Y, Z) bytes of device scratch. */
int64_t dsu_volume_band_distance_workspace_bytes(int32_t X, int32_t Y, int32_t Z);
int dsu_volume_band_distance(const uint8_t* binary, int32_t X, int32_t Y, int32_t Z, int32_t R,
                             const double* value_table, const uint8_t* band_table, double* dist,
                             uint8_t* band, void* workspace, int64_t workspace_bytes, void* stream);
/* mcubes.marching_cubes' configuration byte per cube (PyMCubes marchingcubes.h: `if (v[m] <=
 * isovalue) cubeindex |= 1 << m`, geometry.py:59): volume (X,Y,Z) f64 -> cube (X-1,Y-1,Z-1) bytes. */
int dsu_mc_cube_index(const double* volume, int32_t X, int32_t Y, int32_t Z, double isovalue,
                      uint8_t* cube, void* stream);

/* ------------------------------------------------------------------------------------
 * Mesh post-processing of the export (save_mesh, instant_nsr/utils/mesh_utils.py:25-73): the
 * geometric queries of color_projection (utils/coloring_utils.py:91-138) and get_offset_mask
 * (utils/thinning_utils.py:96-193).  SURVEY.md 8f-2.
 * ---------------------------------------------------------------------------------- */

/* Uniform xy grid over the triangles (tris: (n_faces, 3 vertices, 3) f32): cell (cx, cy) =
 * floor((x - x0) / cell), clamped to [0, g); a triangle is listed in every cell its xy bounding
 * box overlaps.  Counting sort in two launches around the caller's exclusive prefix sum:
 * dsu_zgrid_count adds to counts (g*g int32, zeroed by the caller); dsu_zgrid_fill writes the
 * face ids into items at offsets[cell] (+ a zeroed cursor array it increments). */
int dsu_zgrid_count(const float* tris, int64_t n_faces, float x0, float y0, float cell, int32_t g,
                    int32_t* counts, void* stream);
int dsu_zgrid_fill(const float* tris, int64_t n_faces, float x0, float y0, float cell, int32_t g,
                   const int32_t* offsets, int32_t* cursor, int32_t* items, void* stream);
/* mesh_raycast.raycast(origin, (0, 0, sign), mesh=triangles) for n_rays origins (coloring_utils.py:
 * 107-130, thinning_utils.py:101-193): per ray the number of hits, the nearest and the farthest
 * hit (distance t >= 0 along the ray and face id; ties -> smaller face id; no hit: id -1, t 0).
 * A hit = (x, y) inside or on the boundary of the triangle's xy projection and not behind the
 * origin.  self_vertex (optional, with faces (n_faces,3) int32): the mesh vertex a ray starts at;
 * triangles incident to it count as hits at distance exactly 0. */
int dsu_zray_cast(const float* tris, const int32_t* faces, int64_t n_faces, float x0, float y0,
                  float cell, int32_t g, const int32_t* offsets, const int32_t* items,
                  const float* origins, int64_t n_rays, int32_t sign, const int32_t* self_vertex,
                  int32_t* hit_count, float* t_near, int32_t* face_near, float* t_far,
                  int32_t* face_far, void* stream);
/* MaskRenderer.render (coloring_utils.py:22-41; pytorch3d orthographic rasteriser, zbuf > -1):
 * silhouette of `scale` x the mesh seen from +z on a res x res image, 255 where a pixel centre
 * (x = (2 col + 1) / res - 1, y = 1 - (2 row + 1) / res) is covered; mask zeroed by the caller. */
int dsu_raster_mask(const float* tris, int64_t n_faces, float scale, int32_t res, uint8_t* mask,
                    void* stream);
/* cv2.erode(src, cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (ksize, ksize))) (coloring_utils.py:
 * 61-64), single channel uint8, default border. */
int dsu_erode_ellipse_u8(const uint8_t* src, int32_t H, int32_t W, int32_t ksize, uint8_t* dst,
                         void* stream);
/* interpolate_rgb (coloring_utils.py:43-58): for every query point the 8 nearest known points in
 * the xy plane (scipy cKDTree.query(k=8); coordinates float64), colours blended with weights
 * 1 / (d + 1e-6).  The
 * known points are binned on an xy grid by dsu_point_bin_count / _fill (same protocol as the
 * triangle grid). */
int dsu_point_bin_count(const float* xy, int64_t n, float x0, float y0, float cell, int32_t g,
                        int32_t* counts, void* stream);
int dsu_point_bin_fill(const float* xy, int64_t n, float x0, float y0, float cell, int32_t g,
                       const int32_t* offsets, int32_t* cursor, int32_t* items, void* stream);
int dsu_knn8_blend(const double* query_xy, int64_t n_query, const double* known_xy,
                   const float* known_rgb, int64_t n_known, float x0, float y0, float cell,
                   int32_t g, const int32_t* offsets, const int32_t* items, float* out_rgb,
                   void* stream);

/* ------------------------------------------------------------------------------------
 * Frame rendering between reconstruction and stylisation (3_style_translator/run_render.py +
 * blender_animation.py; csrc/mesh_render.hip): for the rig-free actions the reference's renderer
 * is an orthographic rasteriser of a vertex-coloured mesh, run once with the colours and once with
 * the normalised positions.  n_frames frames of one mesh, both attribute sets, in one call.
 *
 * Inputs: screen (n_frames, n_verts, 3) f32 per-frame vertices (x right, y up, z towards the
 * viewer); faces (n_faces, 3) i32; colour, pos (n_verts, 3) f32, clamped to [0, 1]; the window
 * centre (cx, cy) and world width span; output side `size` (a multiple of 4, at most 2048);
 * ss in {1, 2, 4} sub-samples per pixel side.  tex: NULL = the colours are the vertex colours, and
 * colour is required at DSU_RENDER_RASTER; otherwise the colours come from the atlas or the pyramid
 * that *tex names ("Textured frames" and "Mip-mapped frames" below), and colour is not read and may
 * be NULL.  tex is read and validated at DSU_RENDER_RASTER only: COUNT and FILL ignore it, as they
 * ignore colour and pos.
 *
 * Rule.  Fine lattice N = size * ss: sample (R, C) sits at x = cx + ((C + 0.5) / N - 0.5) * span,
 * y = cy - ((R + 0.5) / N - 0.5) * span, in float64 in this order (it depends on N only).  With the
 * edge functions of dsu_zray_cast (float64 from the f32 vertices a, b, c)
 *     w0 = (x - bx)(cy - by) - (y - by)(cx - bx),  w1 = (x - cx)(ay - cy) - (y - cy)(ax - cx),
 *     w2 = (x - ax)(by - ay) - (y - ay)(bx - ax),  area = w0 + w1 + w2,
 * a sample is covered when all three are >= 0 or all three are <= 0 and area != 0.  Its depth is
 * z = (w0 za + w1 zb + w2 zc) / area rounded to f32; the largest z wins, equal z goes to the lowest
 * face index.  The attributes of the winning face are (w0 va + w1 vb + w2 vc) / area per sample
 * (rounded to f32).  Per pixel over its ss^2 samples: alpha = covered / ss^2, rgb = the float64
 * mean over the covered samples in row-major order (straight alpha; 0 where nothing is covered),
 * uint8 = floor(v * 255 + 0.5).  No products are fused.  This box over the pixel's own samples stands
 * in for Blender's pixel filter; dsu_mesh_render_ortho_filtered ("Pixel filter" below) puts a
 * reconstruction window that reaches into the neighbouring pixels in its place.
 *
 * Outputs, each optional (NULL): color_u8, pos_u8 (n_frames, size, size, 4) RGBA; face_id
 * (n_frames, N, N) i32, -1 = empty; depth (n_frames, N, N) f32, 0 where empty; frames
 * (n_frames, 6, size, size) f32 = the DatasetFullImages tensor with mask and pos on, formed from the
 * uint8 values ((u8 / 255 - 0.5) / 0.5 for colour rgb and pos rg, a8 / 255 for the mask: what a PNG
 * round trip gives); pixels (n_frames, size, size, 8) f32 = colour rgb, alpha, pos rgb, alpha
 * before quantisation.
 *
 * (frame, triangle) pairs are binned onto 16x16-pixel tiles by a counting sort around the
 * caller's prefix sum, one stage per call on the same arguments:
 *   DSU_RENDER_COUNT   counts per (frame, tile) bin -> workspace int32 [0, bins)
 *   (caller)           exclusive prefix sum of the counts -> workspace int32 [bins, 2 bins + 1);
 *                      its last entry is n_items, the length of `items` (int32, caller-owned)
 *   DSU_RENDER_FILL    triangle ids into items
 *   DSU_RENDER_RASTER  one workgroup per bin: visibility in LDS, resolve, all outputs
 * bins = n_frames * ceil(size / 16)^2; workspace_bytes = (3 bins + 1) * 4.
 *
 * Textured frames (tex with DSU_TEX_NEAREST or DSU_TEX_BILINEAR): the colour of every sample is taken
 * from a UV atlas instead of the vertex colours (the reference's Blender reads the OBJ's map_Kd).
 * uv (n_verts, 2) f32; texels (tex_size, tex_size, 4) uint8 RGBA, 4-byte aligned (a texel is one
 * 32-bit load; the fourth byte is not read); 1 <= tex_size <= 8192.  DSU_EINVAL before any launch:
 * uv or texels NULL, texels misaligned, tex_size out of range, filter not one of DSU_TEX_*, or
 * DSU_TEX_ANISOTROPIC with max_aniso outside 1..16.
 *
 * Rule.  Visibility, depth, alpha, the position pass, frames, the layout of pixels and everything
 * downstream of pos_u8 are as without tex: the texture enters through the three colour
 * channels and in no other way.  For a covered sample whose winner is face (a, b, c), with w0, w1,
 * w2 and area as above and the vertex uvs widened from f32 to float64:
 *     u = (w0 ua + w1 ub + w2 uc) / area,  v likewise,  tx = u T,  ty = v T  (T = tex_size);
 *     a non-finite tx or ty is taken as 0.
 * The texel convention is the bake's (dsu_uv_bake): image row r, column c holds uv T = (c, T - 1 - r).
 *   nearest:   c = clamp(floor(tx + 0.5), 0, T - 1),  r = clamp(T - 1 - floor(ty + 0.5), 0, T - 1),
 *              channel = (float)u8 / 255.0f.
 *   bilinear:  x = clamp(tx, 0, T - 1),  y = clamp(T - 1 - ty, 0, T - 1),  c0 = floor(x),
 *              c1 = min(c0 + 1, T - 1),  r0, r1 likewise from y,  fx = x - c0,  fy = y - r0,
 *              channel = (((1 - fx)(1 - fy)) p00 + (fx (1 - fy)) p01 + ((1 - fx) fy) p10 + (fx fy) p11) / 255
 *              in float64, summed left to right (p01 = row r0, column c1; p10 = row r1, column c0),
 *              rounded to f32.  T = 1 is legal.
 * The per-sample value goes where the interpolated vertex colour goes: accumulated in float64 over
 * the pixel's covered samples in row-major order, divided by their count, uint8 = floor(v 255 + 0.5).
 * These two filters read level 0 only: a texture much finer than the sample lattice aliases under
 * them.  DSU_TEX_TRILINEAR ("Mip-mapped frames" below) is the filtered read and DSU_TEX_ANISOTROPIC
 * ("Anisotropic frames" below) the one that follows the footprint's long axis; there is no area
 * sampling.  The library cannot tell a level-0 image from a pyramid: texels that hold only the
 * former, passed with DSU_TEX_TRILINEAR or DSU_TEX_ANISOTROPIC, are read past their end. */
#define DSU_RENDER_COUNT 0
#define DSU_RENDER_FILL 1
#define DSU_RENDER_RASTER 2
#define DSU_TEX_NEAREST   0
#define DSU_TEX_BILINEAR  1
#define DSU_TEX_TRILINEAR 2
#define DSU_TEX_ANISOTROPIC 3
typedef struct dsu_render_texture {
  const float*   uv;        /* (n_verts, 2) f32 */
  const uint8_t* texels;    /* NEAREST / BILINEAR: (T, T, 4) RGBA8.  TRILINEAR / ANISOTROPIC: the pyramid
                               buffer of dsu_mip_pyramid_build for a level 0 of side T.  4-byte aligned. */
  int32_t tex_size;         /* T, 1 .. 8192 */
  int32_t filter;           /* DSU_TEX_* */
  int32_t max_aniso;        /* ANISOTROPIC: the cap on the probes of a sample, 1 .. 16; not read otherwise */
} dsu_render_texture;
int64_t dsu_mesh_render_ortho_workspace_bytes(int32_t n_frames, int32_t size);
int dsu_mesh_render_ortho(int32_t stage, const float* screen, const int32_t* faces,
                          const float* colour, const float* pos, const dsu_render_texture* tex,
                          int32_t n_frames, int64_t n_verts, int64_t n_faces, double cx, double cy,
                          double span, int32_t size, int32_t ss, void* workspace, int64_t workspace_bytes,
                          int32_t* items, int64_t n_items, uint8_t* color_u8, uint8_t* pos_u8,
                          int32_t* face_id, float* depth, float* frames, float* pixels, void* stream);
/* Mip-mapped frames: the pyramid of the atlas (csrc/mesh_mip.hip) and the trilinear read of it in
 * the resolve (csrc/mesh_render.hip; the arithmetic of both sides is csrc/mip_sample.h).
 *
 * a. The pyramid.  texture (T, T, 4) RGBA8 as above, 1 <= T <= 8192, any T; covered (T, T) u8 or
 * NULL = every texel is covered.  Levels: T_0 = T, T_k = ceil(T_{k-1} / 2), L = the number of levels
 * down to and including size 1 (dsu_mip_levels).  Storage: one RGBA8 buffer, level k at texel offset
 * sum_{j<k} T_j^2; dsu_mip_pyramid_texels(T) texels in all.
 *   Level 0 is the input byte for byte (its alpha is not rewritten; pyramid == texture skips the copy).
 *   Level k >= 1, reduction: texel (r, c) owns the level-0 rows [2^k r, 2^k (r + 1)) clipped to
 *   [0, T) and the columns likewise.  n = the covered level-0 texels of the block, sum_ch their
 *   channel sum.  n > 0: the texel is covered and channel = (2 sum_ch + n) / (2 n) in integer
 *   arithmetic (round half up, the form of dsu_uv_dilate's mean).  The means come from the exact sums,
 *   not from rounded children: every level hands (sum_r, sum_g, sum_b, n), 64 bits each (255 4^13
 *   does not fit 32), to the next; one thread per output texel adds its 2 x 2 children, and the
 *   clipped edge of an odd level is absent children, not zeros.
 *   Level k >= 1, gutter: `gutter` rounds (0..64; the export's 2) of exactly dsu_uv_dilate's rule on
 *   the covered / uncovered texels of that level.  A texel still uncovered is 0.  The alpha byte is
 *   255 where the texel is covered after the rounds and 0 otherwise; sampling never reads alpha.
 * No atomics: two builds give the same bytes.  workspace (16-byte aligned):
 * dsu_mip_workspace_bytes(T) = 32 (T_1^2 + T_2^2) + 4 T_1^2 for T > 1 — the sums of two consecutive
 * levels and one spare level image for the gutter rounds (T = 8192: 704 MB; T = 1024: 11 MB) —, 0
 * (workspace may be NULL) for T = 1.  DSU_EINVAL before any launch: T or gutter out of range,
 * texture or pyramid NULL or not 4-byte aligned, workspace NULL, short or misaligned.
 *
 * b. dsu_mesh_render_ortho, tex with DSU_TEX_TRILINEAR: texels is the pyramid buffer of a, tex_size
 * the side of its level 0.  Visibility, depth, alpha, the position pass, frames and pixels are
 * untouched; tx, ty of a sample are formed as in "Textured frames".
 *   Level of detail.  The view is orthographic and uv is affine on a face, so the texel footprint
 *   of one sub-sample is constant per (frame, face).  Float64 from the f32 screen vertices a, b, c
 *   and the f32 uvs, in this operand order, no products fused:
 *       e1 = b - a,  e2 = c - a (screen x, y);
 *       p1 = (ub - ua) T,  q1 = (vb - va) T;  p2, q2 likewise from c;
 *       det = e1x e2y - e1y e2x;   h = span / N, the sample spacing;
 *       dpx = (p1 e2y - p2 e1y) / det,  dpy = (p2 e1x - p1 e2x) / det;  dqx, dqy likewise from q;
 *       gx = dpx dpx + dqx dqx,  gy = dpy dpy + dqy dqy;
 *       rho = sqrt((h h) (gx > gy ? gx : gy))       (IEEE sqrt; det == 0: rho = 0).
 *   rho not finite or !(rho > 1): k = 0, t = 0.  Otherwise k = floor(log2 rho), read from the
 *   exponent (ilogb; no transcendental call); k >= L - 1: k = L - 1, t = 0; otherwise
 *   t = rho 2^-k - 1 (ldexp, exact), t in [0, 1).
 *   Sample.  x_0 = tx, y_0 = (T - 1) - ty (non-finite tx, ty -> 0 first).  At level j:
 *   x_j = (x_0 - (2^j - 1) / 2) / 2^j, y_j likewise — a level-j texel sits at the centre of its block
 *   of level-0 sample points under the bake's point convention —, clamped to [0, T_j - 1].  B_j is
 *   the bilinear filter's four-term expression at level j, same operand order, float64, not divided
 *   and not rounded.  channel = (float)(((1 - t) B_k + t B_{k+1}) / 255), one rounding to f32; with
 *   t = 0 level k + 1 is not read and channel = (float)(B_k / 255): at k = 0, t = 0 this is the
 *   bilinear rule bit for bit.
 * Deviations from the textbook filter.  The blend weight is linear in rho inside an octave where
 * log2 rho would be the usual choice (they differ by at most 0.086 of a level); in exchange the rule
 * is reproducible bit for bit on the host.  rho is the isotropic (max) rule: a face seen edge-on is
 * blurred along both axes; DSU_TEX_ANISOTROPIC ("Anisotropic frames" below) is the filter that is not.
 *
 * c. dsu_mip_sample_host: HOST function on HOST arrays — the sampling above (level and weight from
 * rho[i], then the sample at tx[i], ty[i]) evaluated on the CPU by the text the kernel compiles:
 * rgb_out (n, 3) f32. */
int32_t dsu_mip_levels(int32_t tex_size);
int64_t dsu_mip_pyramid_texels(int32_t tex_size);
int64_t dsu_mip_workspace_bytes(int32_t tex_size);
int dsu_mip_pyramid_build(const uint8_t* texture, const uint8_t* covered, int32_t tex_size, int32_t gutter,
                          uint8_t* pyramid, void* workspace, int64_t workspace_bytes, void* stream);
int dsu_mip_sample_host(const uint8_t* pyramid, int32_t tex_size, const double* tx, const double* ty,
                        const double* rho, int64_t n, float* rgb_out);
/* Anisotropic frames: dsu_mesh_render_ortho (and _filtered), tex with DSU_TEX_ANISOTROPIC and max_aniso
 * = cap in 1..16.  texels is the pyramid buffer as for DSU_TEX_TRILINEAR; visibility, depth, alpha, the
 * position pass, frames and pixels are untouched.  Where the trilinear rule takes one isotropic
 * footprint, this one takes the footprint's two axes: up to `cap` trilinear probes are spread along
 * the long axis, each at the level of the footprint divided by their number, so a face seen edge-on
 * keeps its detail along the axis that is not compressed.  (csrc/mip_sample.h is the text of both
 * sides; tests/frame_render_aniso_ref.py restates it.)
 *
 * Rule.  Everything is float64 in the operand order written, no products fused, no transcendental:
 * IEEE sqrt and division only.  Per (frame, face), from the f32 screen vertices and the f32 uvs, with
 * dpx, dpy, dqx, dqy, det and h exactly as in "Mip-mapped frames":
 *     A = (h h)(dpx dpx + dpy dpy),  C = (h h)(dqx dqx + dqy dqy),
 *     B = (h h)(dpx dqx + dpy dqy),  D = (h h)(dpx dqy - dpy dqx)
 * — the entries and the determinant's root of M M^T, M the texel-per-sample Jacobian —,
 *     m = (A + C) 0.5,  d = (A - C) 0.5,  r = sqrt(d d + B B),  s1 = sqrt(m + r),  s2 = |D| / s1
 * (s2 from the determinant: m - r cancels).  Major axis in (tx, ty): (d + r, B) when d >= 0, else
 * (B, r - d) — neither form cancels —, divided by its norm sqrt(x x + y y); (1, 0) where the norm is 0
 * or not finite.
 *   det == 0, or one of A, B, C, D, r, s1 not finite: N = 1, rho' = 0, s1 taken as 0, axis (1, 0).
 *   Otherwise !(s1 > 1): N = 1;  else !(s2 > 0): N = cap;  else N = min(ceil(s1 / s2), cap) (the
 *   comparison is made in float64, before the conversion to int);  rho' = s1 / N;
 *   (k, t) = the level and weight of "Mip-mapped frames" for rho'.
 * Per sample, with tx, ty as in "Textured frames": probe i = 0 .. N - 1 sits at
 *     o_i = ((double)(2 i + 1) / (double)(2 N) - 0.5) s1,   (tx + o_i ax, ty + o_i ay)
 * (a non-finite coordinate is taken as 0, per probe); V_i is the unrounded trilinear value there at
 * (k, t): B_k, or (1 - t) B_k + t B_{k+1};
 *     channel = (float)(((sum_i V_i) / (double)N) / 255.0),
 * the sum started at 0 and taken in ascending i, one rounding to f32.
 *   The gutter.  2^k <= rho' = s1 / N, so |o_i| <= (N - 1) s1 / (2 N) < (N - 1) 2^k: the outermost
 *   probe lies less than N - 1 texels of level k from the sample, and its bilinear read reaches one
 *   texel further.  A chart therefore needs max(2, cap) texels of margin on every level for no probe
 *   to read its neighbour: animate.render_frames builds the pyramid with that many gutter rounds (and
 *   dilates level 0 by as many).  This entry point does not dilate: it reads the pyramid it is given.
 * What follows from the rule (and the tests assert):
 *   (a) s1 <= 1: N = 1, k = 0, t = 0, o_0 = 0 — the bilinear rule bit for bit;
 *   (b) an axis-aligned map of equal scale on both axes (dpy = dqx = 0, |dpx| = |dqy|): A = C has the
 *       bits of the trilinear (h h) gx, so s1 has the bits of the trilinear rho; where s1 / s2 does not
 *       exceed 1 in float64 (every scale whose square root is exact) N = 1 and the output is the
 *       trilinear one bit for bit;
 *   (c) cap = 1 is a trilinear filter on s1 (the larger singular value where "Mip-mapped frames" takes
 *       the larger screen-axis gradient).
 * Deviations from the textbook filter.  The probes have equal weights: no Gaussian, no EWA.  The blend
 * is linear in rho', as the trilinear rule's is in rho.  A probe may leave its chart: nothing clips it
 * to the face's uv triangle, the gutter above is what it then reads.  Beyond the cap the probes are
 * spaced wider than their footprint (rho' > s2): the remainder of the ratio is blurred isotropically.
 *
 * dsu_aniso_sample_host: HOST function on HOST arrays — the rule above evaluated on the CPU by the text
 * the kernel compiles, item by item.  tri (n, 6) f64: screen x, y of a, b, c (the f32 vertices widened);
 * uv (n, 6) f32: u, v of a, b, c; h the sample spacing; tx, ty (n) f64 the sample's texel coordinates;
 * max_aniso the cap.  rgb_out (n, 3) f32; optional (NULL): probes_out (n) i32 = N, rho_out (n) f64 =
 * rho', axis_out (n, 2) f64.  DSU_EINVAL: tex_size or max_aniso out of range, n < 0, h not finite, or
 * with n > 0 a required pointer NULL or pyramid not 4-byte aligned. */
int dsu_aniso_sample_host(const uint8_t* pyramid, int32_t tex_size, const double* tri, const float* uv, double h,
                          const double* tx, const double* ty, int32_t max_aniso, int64_t n, float* rgb_out,
                          int32_t* probes_out, double* rho_out, double* axis_out);
/* Pixel filter: dsu_mesh_render_ortho_filtered is dsu_mesh_render_ortho with the reconstruction
 * filter of the reference's renderer in the resolve (Blender's EEVEE and Cycles weight the samples
 * of a pixel with a Blackman-Harris window that reaches beyond the pixel's own square) where
 * dsu_mesh_render_ortho has a box over the pixel's own ss^2 samples.  The arguments are those of
 * dsu_mesh_render_ortho with `taps` and `halo` after ss; the three stages, the workspace and
 * dsu_mesh_render_ortho_workspace_bytes are the same; dsu_mesh_render_ortho itself is unchanged.
 *
 * The library calls no transcendental: the caller hands in the 1-D window as a table (HOST memory),
 * so host and device agree bit for bit and any separable window is the caller's matter
 * (animate.pixel_filter makes the tables).  taps holds ss + 2 halo f64 values; halo is counted in
 * sub-samples, 0 <= halo <= 2 ss.  Tap index q + halo belongs to sub-sample offset q in
 * [-halo, ss + halo) from the pixel's first sample; its distance from the pixel centre is
 * d_q = (q + 0.5) / ss - 0.5 px.
 *
 * Rule.  Visibility and the per-sample attributes v (f32: the interpolated vertex colour, or the
 * nearest, bilinear or trilinear read; the interpolated position) are those of dsu_mesh_render_ortho.
 * For pixel (i, j): rows R = i ss + qy, columns C = j ss + qx.  A sample with R or C outside [0, N)
 * does not exist and enters no sum: the weights are renormalised at the image border.  The samples
 * are walked row-major over (qy, qx), everything in float64, no products fused:
 *     w = taps[qy + halo] * taps[qx + halo];   W_all += w;
 *     covered sample:  W_cov += w,  A_ch += w * (double)v_ch  for the six channels;
 *     alpha = W_cov / W_all;   channel = W_cov > 0 ? A_ch / W_cov : 0;
 * both rounded to f32 in `pixels`; uint8 = floor(v 255 + 0.5) of the float64 values, `frames` from the
 * uint8 values, as in dsu_mesh_render_ortho.  face_id and depth are per sample and do not depend on
 * the filter.  With halo = 0 and all taps 1.0 every output is byte-equal to dsu_mesh_render_ortho.
 * A pixel all of whose existing samples are covered has alpha exactly 1 (W_cov and W_all are the
 * same sum), which is what pos2edge asks of the interior.
 *
 * hp = ceil(halo / ss).  COUNT / FILL list a (frame, triangle) pair in every tile whose 16x16-pixel
 * rectangle, grown by hp pixels and clipped to the image, the triangle's sample range touches; RASTER
 * keeps the keys of the grown tile, ((16 + 2 hp) ss)^2 of them, in LDS (at most 51 200 B).  halo is
 * read at all three stages and must be the same in each; taps is read at RASTER only.
 * DSU_EINVAL before any launch: everything dsu_mesh_render_ortho refuses; halo out of range (every
 * stage); at RASTER taps NULL, a tap negative or not finite, the ss central taps summing to 0.
 *
 * dsu_pixel_filter_resolve_host: HOST function on HOST arrays — the accumulation above evaluated on
 * the CPU by the text the kernel compiles (csrc/film_filter.h), from per-sample colour and pos
 * (n_frames, N, N, 3) f32 and covered (n_frames, N, N) u8, N = size ss.  Outputs, each optional:
 * pixels (n_frames, size, size, 8) f32, color_u8 and pos_u8 (n_frames, size, size, 4).  The inputs
 * are any f32: a uint8 is 0 for a value that is not a number and clamped to 0..255 otherwise (on the
 * device every v lies in [0, 1]).  DSU_EINVAL: n_frames, size or ss out of dsu_mesh_render_ortho's
 * range, an input NULL, taps or halo as above. */
int dsu_mesh_render_ortho_filtered(int32_t stage, const float* screen, const int32_t* faces,
                                   const float* colour, const float* pos, const dsu_render_texture* tex,
                                   int32_t n_frames, int64_t n_verts, int64_t n_faces, double cx, double cy,
                                   double span, int32_t size, int32_t ss, const double* taps, int32_t halo,
                                   void* workspace, int64_t workspace_bytes, int32_t* items, int64_t n_items,
                                   uint8_t* color_u8, uint8_t* pos_u8, int32_t* face_id, float* depth,
                                   float* frames, float* pixels, void* stream);
int dsu_pixel_filter_resolve_host(const float* colour, const float* pos, const uint8_t* covered,
                                  int32_t n_frames, int32_t size, int32_t ss, const double* taps, int32_t halo,
                                  float* pixels, uint8_t* color_u8, uint8_t* pos_u8);
/* pos2edge (run_render.py:31-57) and the inversion of run_render.py:120 on RGBA8 position images
 * (n_frames, H, W, 4): channels u8 -> f32 / 255, every channel 2 where alpha8 < 255, per-channel 3x3
 * Sobel in float64 with reflect-101 borders, magnitude, maximum over the three colour channels,
 * > 0.3 = edge.  edge (n_frames, H, W) uint8: 255 = no edge, 0 = edge — the edge PNG and the
 * stylisation path's edge tensor at once. */
int dsu_pos_edge_u8(const uint8_t* pos_rgba, int32_t n_frames, int32_t H, int32_t W, uint8_t* edge,
                    void* stream);

/* ------------------------------------------------------------------------------------
 * Rigging of the reconstructed mesh (blender_animation.py:38-44: the mesh is bound to the armature
 * with Blender's automatic bone-heat weights and skinned per frame; csrc/mesh_skin.hip).  The
 * weighting follows the published bone-heat form (Baran & Popovic, "Automatic rigging and animation
 * of 3D characters", 2007), not Blender's source.  Host side: drawingspinup_amd/animate/skin.py.
 *
 * a. dsu_bone_visibility.  Inputs: verts (n_verts, 3) f32; faces (n_faces, 3) i32; bones
 * (n_bones, 2, 3) f32, head a and tail b of each bone; order (n_verts) i32 or NULL: the vertex that
 * thread k takes (a permutation; spatially sorted vertices keep a workgroup's segments together —
 * the outputs do not depend on it).
 *
 * Rule, for vertex p (index i) and bone (a, b), everything in float64 from the f32 inputs, sums of
 * three terms taken as (x + y) + z, no products are fused:
 *     ab = b - a,  ap = p - a,  den = ab.ab,  num = ap.ab,
 *     t = num / den clamped to [0, 1] (t = 0 when den is not > 0),
 *     q = a + t ab (per coordinate),  e = q - p,  d = sqrt(e.e).
 * With  [x, y, z] = (x0 (y1 z2 - y2 z1) + x1 (y2 z0 - y0 z2)) + x2 (y0 z1 - y1 z0)  for three vectors
 * x, y, z (components 0, 1, 2), a triangle (u, v, w) none of whose three indices equals i crosses the
 * open segment p -> q when, with A = u - p, B = v - p, C = w - p,
 *     s1 = [A, B, C],  s2 = [u - q, v - q, w - q]:  (s1 > 0 and s2 < 0) or (s1 < 0 and s2 > 0)
 *                                                   (both ends strictly off the plane, on opposite sides)
 *     t1 = [e, A, B],  t2 = [e, B, C],  t3 = [e, C, A]:  all three >= 0 or all three <= 0
 *                                                   (the closed triangle).
 * visible = no such triangle.  A non-finite d gives visible = 0.  Triangles with an index outside
 * [0, n_verts) are ignored.
 * Outputs: dist (n_verts, n_bones) f64 = d; visible (n_verts, n_bones) u8.
 *
 * Triangles are binned on a uniform grid — cell (cx, cy, cz) = floor((x - x0) / cell) per axis,
 * clamped to [0, g - 1], list index (cz gy + cy) gx + cx — into every cell their bounding box
 * touches, by the counting sort of dsu_mesh_render_ortho, one stage per call on the same arguments:
 *   DSU_SKIN_COUNT   counts per cell -> workspace int32 [0, cells)
 *   (caller)         exclusive prefix sum -> workspace int32 [cells, 2 cells + 1); its last entry
 *                    is n_items, the length of `items` (int32, caller-owned)
 *   DSU_SKIN_FILL    triangle ids into items
 *   DSU_SKIN_RUN     one workgroup per (256 vertices, bone): only the cells that the boxes of its
 *                    segments touch are walked, 256 triangles at a time through LDS; a triangle
 *                    whose box is apart from a segment's box is not tested against it (they have
 *                    no point in common).
 * cells = gx gy gz (each at most 256, at most 2^22 in all); workspace_bytes = (3 cells + 1) * 4. */
#define DSU_SKIN_COUNT 0
#define DSU_SKIN_FILL 1
#define DSU_SKIN_RUN 2
int64_t dsu_bone_visibility_workspace_bytes(int32_t gx, int32_t gy, int32_t gz);
int dsu_bone_visibility(int32_t stage, const float* verts, const int32_t* faces, const float* bones,
                        int64_t n_verts, int64_t n_faces, int32_t n_bones, const int32_t* order, double x0,
                        double y0, double z0, double cell, int32_t gx, int32_t gy, int32_t gz,
                        void* workspace, int64_t workspace_bytes, int32_t* items, int64_t n_items,
                        double* dist, uint8_t* visible, void* stream);
/* c. The bone-heat system (L + M H) W = M H P (assembled on the host, once per character) for all
 * bones at once: Jacobi-preconditioned conjugate gradients in float64 on a symmetric positive
 * definite matrix in CSR form (rowptr (n + 1) i32, cols (nnz) i32, vals (nnz) f64: device arrays),
 * rhs and x (n, n_rhs) f64 row-major (a matrix row reads n_rhs contiguous values per neighbour).
 * x holds the starting guess on entry and the solution on return.  Every column runs its own
 * recurrence (alpha = r.z / p.Ap, beta = r.z new / r.z old, z = r / diag; a diagonal that is not
 * > 0 counts as 1; a row's products are added in the order of its entries); the inner products are
 * fixed-order partial sums — per workgroup in row order, then over the workgroups in order — so
 * two runs give the same bits.  After every iteration the relative residuals |r| / |b| of the
 * recurrence (|b| = 0 counts as 1) are compared with tol: the solve stops when every column is
 * <= tol, or after max_iters iterations.  out_iters (HOST int32) = iterations run; out_residuals
 * (HOST, n_rhs f64) = the final relative residuals.  Synchronises the stream (one flag per
 * iteration is read back).  n_rhs <= 256.
 * workspace_bytes: three (n, n_rhs) vectors, the inverse diagonal and the partial sums. */
int64_t dsu_spd_cg_block_workspace_bytes(int64_t n, int32_t n_rhs);
int dsu_spd_cg_block(const int32_t* rowptr, const int32_t* cols, const double* vals, int64_t n, int64_t nnz,
                     int32_t n_rhs, const double* rhs, double* x, double tol, int32_t max_iters,
                     void* workspace, int64_t workspace_bytes, int32_t* out_iters, double* out_residuals,
                     void* stream);
/* Linear-blend skinning: rest (n_verts, 3) f32, influences (n_verts, K) i32 joint indices, weights
 * (n_verts, K) f32, matrices (n_frames, n_joints, 3, 4) f32 = [R | t] per frame and joint ->
 * out (n_frames, n_verts, 3) f32, the `screen` tensor of dsu_mesh_render_ortho:
 *     y_k = ((R_c0 x + R_c1 y) + R_c2 z) + t_c per coordinate c,  out = sum_k w_k y_k,
 * accumulated in f32 from 0 in the order k = 0 .. K-1, no products are fused.  An influence
 * outside [0, n_joints) contributes nothing. */
int dsu_skin_lbs(const float* rest, const int32_t* influences, const float* weights, const float* matrices,
                 int64_t n_verts, int32_t K, int32_t n_frames, int32_t n_joints, float* out, void* stream);
/* Dual-quaternion skinning ("Preserve Volume" of Blender's armature modifier; Kavan et al.,
 * "Geometric skinning with approximate dual quaternion blending", 2008): where linear blending
 * averages matrices — a vertex shared half and half by two joints that differ by a turn of theta
 * lands at cos(theta / 2) of its distance from the axis —, this blends unit dual quaternions and
 * applies the rigid transform of the normalised blend, so the distance is kept.  An extension of
 * the reference (blender_animation.py leaves Blender's linear default on); csrc/dqs_blend.h holds
 * the text, compiled for the kernel and for the host entry.
 *
 * rest, influences, weights, out: as dsu_skin_lbs.  dualquats (n_frames, n_joints, 8) FLOAT64 =
 * [r_w r_x r_y r_z | d_w d_x d_y d_z] per frame and joint: a unit rotation quaternion r and the dual
 * part d = 1/2 (0, t) (x) r of the joint's rigid skinning transform [R | t] (float64: the table is
 * n_frames n_joints 64 B, the arithmetic is float64 anyway, and an f32 table alone would cost about
 * 13 f32 ulps against the rigid transform).
 *
 * Rule per (frame, vertex), everything in float64 from the f32 / f64 inputs, sums of four terms
 * taken as ((a + b) + c) + d, no products are fused:
 *   1. k = 0 .. K-1 in order; an influence outside [0, n_joints) or with a weight that is not > 0
 *      contributes nothing.  The first contributing influence is the pivot, r_p its rotation.
 *   2. dot_k = ((r_k.w r_p.w + r_k.x r_p.x) + r_k.y r_p.y) + r_k.z r_p.z;  s_k = -1 if dot_k < 0,
 *      else +1 (q and -q are the same transform; the pivot itself gets +1).
 *   3. b_c = b_c + (s_k w_k) q_k,c for the 8 components c, accumulated from 0.
 *   4. n2 = ((b_0 b_0 + b_1 b_1) + b_2 b_2) + b_3 b_3.  Unless n2 > 0 and finite, out = rest (no
 *      contributing influence, rotations that cancel, NaN in a rotation part).
 *   5. n = sqrt(n2);  r = b_0..3 / n,  d = b_4..7 / n  (component by component).
 *   6. t = 2 ((r_w d_v - d_w r_v) + r_v x d_v)  with  (u x v)_x = u_y v_z - u_z v_y  (cyclic); the d_w
 *      term removes the part of the blended dual that is no longer orthogonal to r.
 *   7. a = r_v x x,  c = r_v x a,  x' = (x + (2 r_w) a) + 2 c  per coordinate.
 *   8. out = (float)(x' + t), the one rounding to f32.
 * The rotation is applied in this form, not as a 3x3 matrix built from r, because under identity
 * transforms the blend is (W, 0, 0, 0 | 0): r_v = 0, d = 0 and x' = x + 0 + 0 exactly — the skinned
 * rest mesh is the rest mesh bit for bit for any positive weights (dsu_skin_lbs: only at K = 1).
 * Negating any table entry, the pivot's included, leaves the output bits unchanged.
 * Kernel: one thread per (frame, vertex), vertex fastest, 256 threads; no LDS, no atomics: two runs
 * give the same bits.  Skinning transforms here are rigid, so Blender's separate treatment of bone
 * scale does not arise; the known bulge of dual-quaternion blending on the outside of a sharp bend
 * is not corrected (by this blend: dsu_skin_cor below rotates about per-vertex centres instead).
 * dsu_skin_dqs_host: HOST function on HOST arrays, the same text evaluated on the CPU.
 * Both return -1 on a null pointer with work to do and 0 for n_verts = 0. */
int dsu_skin_dqs(const float* rest, const int32_t* influences, const float* weights, const double* dualquats,
                 int64_t n_verts, int32_t K, int32_t n_frames, int32_t n_joints, float* out, void* stream);
int dsu_skin_dqs_host(const float* rest, const int32_t* influences, const float* weights,
                      const double* dualquats, int64_t n_verts, int32_t K, int32_t n_frames, int32_t n_joints,
                      float* out);
/* Centre-of-rotation skinning (Le & Hodgins, "Real-time skeletal skinning with optimized centers of
 * rotation", SIGGRAPH 2016): the third blend.  Linear blending collapses a bent or twisted limb;
 * dual-quaternion blending keeps the radius but swings every vertex near a joint about the joint's
 * axis, which bulges the outside of a sharp bend.  Here every vertex gets, once per character, a
 * centre of rotation p*: the area-weighted mean of the centroids of the triangles whose skinning
 * weights resemble its own.  Per frame the normalised blend of the joints' rotation quaternions is
 * applied about p*, and p* itself moves by the linear blend.  An extension of the reference;
 * csrc/cor_blend.h holds the text, compiled for the kernels and for the host entries.
 * Everything is float64 from the f32 / f64 inputs, no products are fused, sums of three are taken as
 * (a + b) + c and sums of four as ((a + b) + c) + d.
 *
 * a. Centres, once per character: dsu_skin_cor_centres.
 * Inputs: rest (n_verts, 3) f32; faces (n_faces, 3) i32; a CANONICAL influence table joints
 * (n_verts, K) i32 and weights (n_verts, K) f32; n_joints; sigma (f64, > 0; the paper's 0.1 is the
 * default of every Python layer).  Canonical, per row: the contributing joints strictly ascending,
 * each once, with weights > 0; the padding after them is -1 / 0 (a row ends at its first joint outside
 * [0, n_joints)).  ops.skin_cor_centres makes this table from any (influences, weights), in numpy: an
 * influence outside [0, n_joints) or with a weight that is not > 0 is dropped, duplicate joints are
 * added in float64 in k order and rounded to f32 once.
 *   W_i(j) = vertex i's weight on joint j, 0 where absent.
 *   Triangle t = (a, b, c), vertices in stored order:  w^_t(j) = ((W_a(j) + W_b(j)) + W_c(j)) / 3 for the
 *     joints of its three rows (ascending: its canonical row, at most min(3K, n_joints) pairs);
 *     c_t = ((a + b) + c) / 3 per coordinate;  n = (b - a) x (c - a) with (u x v)_x = u_y v_z - u_z v_y
 *     (cyclic);  a_t = sqrt((n_x n_x + n_y n_y) + n_z n_z) / 2.  A triangle with an index outside
 *     [0, n_verts) or whose area is zero or not finite is skipped (so a NaN or infinite vertex removes
 *     its triangles and reaches no sum).
 *   Similarity:  s(i, t) = sum over the joint pairs j < k, in ascending (j, k) order, from 0, of
 *       (((W_i(j) W_i(k)) w^_t(j)) w^_t(k)) exp(-(d d) / sigma^2),   d = W_i(j) w^_t(k) - W_i(k) w^_t(j),
 *     sigma^2 = sigma sigma.  A pair with a zero factor contributes nothing and its exponential is not
 *     evaluated (every entry tests the four factors, so a table made elsewhere with a weight of 0 inside
 *     a row follows the same rule); with fewer than two shared joints s = 0.
 *   Sums:  den_i = sum_t s a_t,  num_i = sum_t (s a_t) c_t per coordinate, each from 0.  Within one
 *     partition of the triangle range the triangles are added in ascending order; the partitions are
 *     combined in ascending order by a second pass.  No floating-point atomics: two runs give the same
 *     bits, and two vertices with equal rows get equal bits.
 *   valid_i = den_i > 0 and den_i, num_i finite;  centre_i = num_i / den_i, or 0 where not valid.  A
 *     vertex on one joint alone has s = 0 everywhere and is not valid: the paper's case for the plain
 *     linear blend.
 * Outputs: centres (n_verts, 3) f64, valid (n_verts) u8.
 * The partition is the implementation's choice — the device entry cuts the triangle range into
 * `parts` runs of whole tiles of DSU_COR_TILE triangles, parts = min(DSU_COR_MAX_PARTS,
 * ceil(1024 / ceil(n_verts / 256))), ceil(ceil(n_faces / tile) / parts) tiles each (the last runs may
 * be empty); the host entry takes one run — and exp is each side's own.  The result is therefore
 * held to a bound, not to bits: per coordinate 2 (n_faces + 1 / sigma^2 + 64) 2^-52 times the
 * bounding-box diagonal (a centre is a convex combination of centroids; a weight carries the
 * relative error of its exponential's argument, at most 1 / sigma^2 of them, plus a few roundings;
 * the sums add n_faces roundings).
 * Kernels (csrc/mesh_skin.hip): one thread per triangle writes the rows; one thread per vertex, 256
 * per workgroup, the partition in blockIdx.y, walks them (K <= 4: the vertex's pairs in registers,
 * the rows through LDS, every lane on the same triangle; above: both from memory); a third adds
 * the partitions.  workspace_bytes: the partial sums (parts, n_verts, 4) f64 and the rows, rounded up
 * to a multiple of 8.
 * n_verts <= 2^26, n_faces <= 2^28, K <= 4096.
 *
 * b. Apply, per (frame, vertex): dsu_skin_cor.
 * rest, influences, weights, out: as dsu_skin_dqs takes them (any table, not only a canonical one),
 * with its skipping rule — an influence outside [0, n_joints) or with a weight that is not > 0
 * contributes nothing, to either part — and its pivot and sign rule.  matrices (n_frames, n_joints,
 * 3, 4) FLOAT64 = [R | t];  quats (n_frames, n_joints, 4) FLOAT64 unit quaternions (w, x, y, z) of R
 * (animate.rotation_quaternions);  centres, valid: of a.
 *   With y_k(p) = ((R_c0 p_x + R_c1 p_y) + R_c2 p_z) + t_c per coordinate c of influence k's transform:
 *   Linear blend:  L(x) = sum_k w_k y_k(x), accumulated from 0 in k order over the contributing
 *     influences.  The weights are used as given, not renormalised, as in dsu_skin_lbs.
 *   Not valid:  out = (float) L(x).
 *   Valid:  M = sum_k w_k (y_k(p*) - p*_c), accumulated from 0 in k order: the displacement of the centre
 *     under the linear blend;  b = sum_k (s_k w_k) r_k, with the first contributing influence as the
 *     pivot and s_k = -1 where ((r_k.w r_p.w + r_k.x r_p.x) + r_k.y r_p.y) + r_k.z r_p.z < 0, else +1 (step
 *     2 of the dual-quaternion rule);  n2 = ((b_0 b_0 + b_1 b_1) + b_2 b_2) + b_3 b_3.  Unless n2 > 0 and
 *     finite (no contributing influence, rotations that cancel, NaN in a quaternion), out = (float) L(x).
 *     r = b / sqrt(n2) component by component;  d = x - p*;  a = r_v x d,  c = r_v x a;
 *     out = (float)(x + (M + ((2 r_w) a + 2 c))), the one rounding to f32.
 * This is p* + M + r d r^-1 — the centre moved by the linear blend, the offset turned by the blended
 * rotation — with the rotation in the form of step 7 there, r d r^-1 = d + (2 r_w) a + 2 c, and p* + d
 * collected into x.  Written as L(p*) + r d r^-1 with L(p*) = sum_k w_k y_k(p*), the same value when the
 * weights sum to 1, the f32 weights' sum leaves (sum w - 1) p* in every coordinate: under identity
 * transforms a coordinate x_c = 0 would come out as (sum w - 1) p*_c, outside any bound relative to
 * |x_c|, and the blend would depend on where the origin lies.  In the form above identity transforms
 * give M = 0 and r_v = 0 exactly, so a vertex with a centre returns its rest position bit for bit; a
 * vertex without one takes L(x) and is reproduced within the linear blend's bound, (2K + 4) 2^-24
 * (|R||x| + |t|), bit for bit only where its weights sum to 1 in float64 (one influence of weight 1).
 * So the rest clip need not render byte-equal to rest_pose in this mode; the other two blends keep
 * their guarantees.
 * The two forms differ by more than rounding where a row's weights do NOT sum to 1 (a caller's table,
 * influences dropped by the skipping rule): L scales the whole position by S = sum w, the form above
 * does not.  Under one transform [R | t] on every joint a vertex with a centre comes out as
 * R x + S t + (S - 1)(R - I) p*, a vertex on the L(x) branches (not valid, n2 not > 0) as S (R x + t); under
 * identity the first returns x and the second S x.  Two neighbouring vertices with the same row can
 * land on different branches (one without a centre, one with), so with S far from 1 the surface tears
 * there by about |S - 1| |x|: the blend is meant for rows that sum to 1 up to their f32 rounding, as
 * animate.bone_heat_weights makes them, and a caller with other rows should normalise them first.  Negating any quaternion, the pivot's included, leaves the output bits unchanged.
 * Kernel: skin_dqs_kernel's shape, one thread per (frame, vertex), vertex fastest, 256 threads; no
 * LDS, no atomics: two runs give the same bits.
 * dsu_skin_cor_centres_host / dsu_skin_cor_host: HOST functions on HOST arrays, the same text
 * evaluated on the CPU (the centres without a workspace; -1 too when the host memory for the rows, about
 * 52 + 12 min(3K, n_joints) bytes per face, cannot be had).  All return -1 on a null pointer with work
 * to do (faces may be null when n_faces = 0) or a short workspace, and 0 for n_verts = 0. */
#define DSU_COR_TILE 64
#define DSU_COR_MAX_PARTS 16
int64_t dsu_skin_cor_centres_workspace_bytes(int64_t n_verts, int64_t n_faces, int32_t K, int32_t n_joints);
int dsu_skin_cor_centres(const float* rest, const int32_t* faces, const int32_t* joints, const float* weights,
                         int64_t n_verts, int64_t n_faces, int32_t K, int32_t n_joints, double sigma,
                         void* workspace, int64_t workspace_bytes, double* centres, uint8_t* valid, void* stream);
int dsu_skin_cor_centres_host(const float* rest, const int32_t* faces, const int32_t* joints, const float* weights,
                              int64_t n_verts, int64_t n_faces, int32_t K, int32_t n_joints, double sigma,
                              double* centres, uint8_t* valid);
int dsu_skin_cor(const float* rest, const int32_t* influences, const float* weights, const double* matrices,
                 const double* quats, const double* centres, const uint8_t* valid, int64_t n_verts, int32_t K,
                 int32_t n_frames, int32_t n_joints, float* out, void* stream);
int dsu_skin_cor_host(const float* rest, const int32_t* influences, const float* weights, const double* matrices,
                      const double* quats, const double* centres, const uint8_t* valid, int64_t n_verts, int32_t K,
                      int32_t n_frames, int32_t n_joints, float* out);
/* Corrective smoothing of skinned frames ("delta mush", Mancewicz et al., "Delta Mush: smoothing
 * deformations while preserving detail", 2014; Blender's Corrective Smooth modifier).  Skinning moves
 * every vertex by its own influences alone, so wrong or abruptly changing weights shear and crease
 * the surface at a joint.  At bind time the rest mesh is smoothed and every vertex remembers, in a
 * local surface frame, its offset from its smoothed position; per frame the skinned mesh is smoothed
 * (which removes the creases) and the offsets are put back in that frame's local frames (which
 * restores the detail).  Invariant under rigid motion; an extension of the reference, off by default;
 * csrc/corrective_smooth.h holds the text, compiled for the kernels and for the host entries.
 *
 * Topology (device arrays, int32; drawingspinup_amd/animate/corrective.py builds it once per
 * character on the WELDED mesh, so a seam-split export does not tear):
 *   rep (n_verts)             the lowest index of each cluster of coincident vertices
 *   faces (n_faces, 3)        the faces over representatives, degenerate ones dropped
 *   nbr_rowptr (n_verts + 1), nbr_cols (n_nbr)    CSR: the row of a representative is the ascending,
 *                             duplicate-free list of the other representatives it shares a face with;
 *                             the row of a non-representative or of a vertex without a face is empty
 *   cor_rowptr (n_verts + 1), cor_faces (n_cor)   CSR: the ascending indices into `faces` of the
 *                             faces that contain the representative
 * A row is rowptr[v] .. rowptr[v + 1] clamped to [0, n]; an entry outside its range (a neighbour or a
 * face vertex outside [0, n_verts), a face outside [0, n_faces)) is left out of its row, as if it
 * were not listed.
 *
 * Rule.  All arithmetic is float64 from the f32 inputs, sums of three terms are (a + b) + c, no
 * products are fused.
 *   Smoothing step, per (frame, vertex v) on an (n_frames, n_verts, 3) f32 buffer q: the neighbours'
 *     q are added in row order to a sum that starts at 0; deg = the row's length; m = sum / deg;
 *     out = (float)(q_v + factor (m - q_v)) per coordinate — one rounding to f32 per step, the
 *     buffers between steps are f32.  deg = 0 copies the value.  `iterations` steps run, the first
 *     from the input, the others between the two halves of the workspace; the input is never written.
 *   Frame at a representative r from the fully smoothed buffer s:
 *     N = sum over the corner row, in row order, from 0, of (b - a) x (c - a), with (a, b, c) the
 *     face's vertices in stored order and (u x w)_x = u_y w_z - u_z w_y (cyclic);
 *     n2 = (N_x N_x + N_y N_y) + N_z N_z; unless n2 > 0 and finite there is no frame; n = N / sqrt(n2)
 *     component by component;  e = s[first neighbour] - s[r];  en = (e_x n_x + e_y n_y) + e_z n_z;
 *     t = e - en n;  t2 = (t_x t_x + t_y t_y) + t_z t_z; unless t2 > 0 and finite there is no frame;
 *     t = t / sqrt(t2);  b = n x t, not renormalised.  An empty neighbour row or an empty corner row:
 *     no frame.
 *   Bind (one frame, the rest mesh): d = rest[r] - s_rest[r];  delta[r] = (t.d, b.d, n.d), each dot
 *     product (x + y) + z: (n_verts, 3) FLOAT64;  valid[r] = 1 if and only if a frame exists:
 *     (n_verts) uint8.  Without a frame delta is 0.
 *   Apply, per (frame, vertex v), r = rep[v]: if valid[r] and a frame exists at r in this frame,
 *     out = (float)(s_r + ((t delta_0 + b delta_1) + n delta_2)) per coordinate; otherwise
 *     out = in[frame, v] unchanged (also when r is outside [0, n_verts)).  All members of a welded
 *     class receive the same position, computed from their representative's input.
 * 0 <= factor <= 1, 1 <= iterations <= 255.  Deviations from Blender's modifier: uniform ("simple")
 * neighbour weights only; one frame per vertex from the area-weighted normal and one edge (the
 * paper's form, not Blender's per-corner accumulation); no boundary pinning and no vertex-group mask
 * (an open boundary shrinks under the smoothing; the stored offsets put it back).  The rest pose is
 * NOT returned byte for byte: R (R^T d) differs from d by about 2^-53 |d|, which shows in a
 * coordinate far smaller than the offset; tests/test_corrective_host.py holds it to a bound.
 * Kernels (csrc/mesh_corrective.hip): one thread per (frame, vertex), vertex fastest, 256 threads,
 * the frame in blockIdx.y; no LDS, no atomics: two runs give the same bits.  dsu_corrective_smooth
 * launches `iterations` smoothing steps and one apply (the apply reads the neighbours' final
 * values, so it cannot be fused into the last step).
 * workspace_bytes: two (n_frames, n_verts, 3) f32 buffers (dsu_corrective_bind: n_frames = 1).
 * `out` may not be the input.  DSU_EINVAL before any launch: factor or iterations out of range,
 * n_verts or n_faces negative or above 2^30, n_frames negative or above 65535, n_frames n_verts above
 * 2^31, n_nbr or n_cor negative or above 2^31 - 1; and, with work to do, a null pointer (nbr_cols,
 * cor_faces and faces may be null when their count is 0), out == skinned, or a short workspace.
 * n_verts = 0 or n_frames = 0: DSU_OK, nothing read or written.
 * dsu_corrective_bind_host / dsu_corrective_smooth_host: HOST functions on HOST arrays (workspace
 * included), the same text evaluated on the CPU, the same argument checks. */
int64_t dsu_corrective_smooth_workspace_bytes(int64_t n_verts, int32_t n_frames);
int dsu_corrective_bind(const float* rest, const int32_t* nbr_rowptr, const int32_t* nbr_cols, int64_t n_nbr,
                        const int32_t* cor_rowptr, const int32_t* cor_faces, int64_t n_cor, const int32_t* faces,
                        int64_t n_faces, int64_t n_verts, double factor, int32_t iterations, void* workspace,
                        int64_t workspace_bytes, double* delta, uint8_t* valid, void* stream);
int dsu_corrective_smooth(const float* skinned, const int32_t* rep, const int32_t* nbr_rowptr,
                          const int32_t* nbr_cols, int64_t n_nbr, const int32_t* cor_rowptr,
                          const int32_t* cor_faces, int64_t n_cor, const int32_t* faces, int64_t n_faces,
                          const double* delta, const uint8_t* valid, int64_t n_verts, int32_t n_frames,
                          double factor, int32_t iterations, void* workspace, int64_t workspace_bytes, float* out,
                          void* stream);
int dsu_corrective_bind_host(const float* rest, const int32_t* nbr_rowptr, const int32_t* nbr_cols, int64_t n_nbr,
                             const int32_t* cor_rowptr, const int32_t* cor_faces, int64_t n_cor,
                             const int32_t* faces, int64_t n_faces, int64_t n_verts, double factor,
                             int32_t iterations, void* workspace, int64_t workspace_bytes, double* delta,
                             uint8_t* valid);
int dsu_corrective_smooth_host(const float* skinned, const int32_t* rep, const int32_t* nbr_rowptr,
                               const int32_t* nbr_cols, int64_t n_nbr, const int32_t* cor_rowptr,
                               const int32_t* cor_faces, int64_t n_cor, const int32_t* faces, int64_t n_faces,
                               const double* delta, const uint8_t* valid, int64_t n_verts, int32_t n_frames,
                               double factor, int32_t iterations, void* workspace, int64_t workspace_bytes,
                               float* out);

/* ------------------------------------------------------------------------------------
 * UV export (the export_uv branch of save_mesh, mesh_utils.py:65-67; coloring_utils.py:140-167;
 * csrc/mesh_uv.hip).  The reference parametrises with xatlas and bakes the vertex colours with
 * scipy's griddata; here the charts are axis projections and the bake rasterises the mesh's own
 * triangles.  Host side (projection, packing, the split loop): drawingspinup_amd/nsr/uv.py.
 * Everything below is float64 from the f32 inputs, no products are fused, and no kernel uses a
 * floating-point atomic: two runs give the same bits.
 *
 * a. dsu_uv_face_labels.  verts (n_verts, 3) f32, faces (n_faces, 3) i32.  With e1 = b - a,
 * e2 = c - a:  n = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x);
 * axis = argmax |n_c| (the lowest axis on a tie);  label = 2 axis + (n_axis < 0);
 * area = |n_axis| / 2, the area of the face projected along its axis.  A face whose normal is zero
 * or not finite, or with an index outside [0, n_verts), gets n = 0, label = -1, area = 0.
 * Outputs: normal (n_faces, 3) f64, label (n_faces) i32, area (n_faces) f64.
 * (|n_axis| >= |n| / sqrt(3) follows from the argmax: the `min_cos` of the parametrisation.)
 *
 * b. dsu_uv_components.  adjacency (n_faces, 3) i32: the face across edge (a,b), (b,c), (c,a), or
 * -1 where the edge is on a boundary or used by more than two faces; label (n_faces) i32.  Two
 * faces are joined when they are adjacent and carry the same label >= 0; a face with a negative
 * label joins nothing.  chart (n_faces) i32 holds chart[m] = m on entry and the smallest face index
 * of m's component on return.  One round = every face takes the minimum of its own value and its
 * joined neighbours' values, then twice replaces its value c by chart[c] (pointer jumping); a face
 * that lowered its value raises `flag` (device int32).  Rounds are launched check_every at a time;
 * after each group the flag is read back (the stream is synchronised) and the loop ends when no
 * face changed, or after max_rounds rounds (then DSU_EUNSUP).  out_rounds (HOST int32) = rounds
 * launched.  Values only fall and only thread m writes chart[m], so the in-place rounds are never
 * behind a synchronous sweep; on a strip numbered along its length the distance covered at least
 * doubles per round.
 *
 * c. dsu_uv_bake.  uvs (n_verts, 2) f32 in [0, 1]; indices (n_faces, 3) i32; colours (n_verts, 3)
 * f32; depth (n_faces) f64 or NULL.  Texel convention of compute_interpolation_map (points =
 * tcoords * shape, X = arange, Y = flip(arange)): image row r, column c samples the point
 * (x, y) = (c, size - 1 - r) of uv * size — NOT the half-texel centre.  Vertex positions are
 * (double)u * size, (double)v * size.  With
 *     w0 = (cx - bx)(y - by) - (cy - by)(x - bx),  w1 = (ax - cx)(y - cy) - (ay - cy)(x - cx),
 *     w2 = (bx - ax)(y - ay) - (by - ay)(x - ax),  area = (w0 + w1) + w2
 * (positive inside a counter-clockwise face: the sign opposite to dsu_mesh_render_ortho's),
 * a face covers the sample when w0 >= 0, w1 >= 0, w2 >= 0 and area > 0 (counter-clockwise faces
 * only; a face with an index outside [0, n_verts) or a non-finite uv covers nothing).  The lowest
 * covering face index wins: face_id (size, size) i32, -1 where no face covers.  Its colour is
 *     ((w0 / area) c_a + (w1 / area) c_b) + (w2 / area) c_c   per channel, summed as written,
 * uint8 = the value * 255 clipped to [0, 255] and truncated (NaN -> 0): image (size, size, 3) u8,
 * 0 where uncovered.  demote (n_faces) u8 or NULL (needs depth): a face STRICTLY contains the
 * sample when w0, w1, w2 > 0; among the faces strictly containing one sample the one with the
 * largest depth (the lowest index on a tie) is in front, every other one gets demote = 1; faces
 * never behind another stay 0.  (The packing keeps charts apart, so two such faces belong to one
 * chart: the chart overlaps itself there.)
 * Faces are binned onto 16x16-texel tiles (tile (ty, tx) holds x in [16 tx, 16 tx + 15], y
 * likewise; bin = ty G + tx, G = ceil(size / 16)) by the counting sort of dsu_mesh_render_ortho:
 *   DSU_UV_COUNT    counts per tile -> workspace int32 [0, tiles)
 *   (caller)        exclusive prefix sum -> workspace int32 [tiles, 2 tiles + 1); its last entry is
 *                   n_items, the length of `items` (int32, caller-owned)
 *   DSU_UV_FILL     face ids into items
 *   DSU_UV_RASTER   one workgroup per tile, one thread per texel, the tile's faces through LDS 256
 *                   at a time; every thread keeps its own winners, so the outputs do not depend on
 *                   the order of the lists
 * size <= 8192; workspace_bytes = (3 tiles + 1) * 4.
 *
 * d. dsu_uv_dilate: one round of the gutter fill.  image_in (size, size, 3) u8, covered_in
 * (size, size) u8.  A covered texel is copied.  An uncovered texel with at least one covered
 * texel among its eight neighbours inside the image takes, per channel, the rounded mean
 * (2 sum + n) / (2 n) in integer arithmetic over those n neighbours and is covered in the output;
 * any other texel is 0 and uncovered.  In and out must be different buffers.
 *
 * e. dsu_uv_project: per-texel back-projection of the front and back drawings into the atlas (an
 * extension: the reference projects the drawings onto the vertices only, coloring_utils.py:91-138).
 * The atlas is (uvs, indices, size) and face_id (size, size) i32 as dsu_uv_bake wrote it; positions
 * (n_verts, 3) f32 are the atlas vertices in color_projection's frame (x right, y up, z front,
 * inside [-0.5, 0.5]); tris (n_faces, 3, 3) f32 = positions[indices] with its z-parallel grid (x0,
 * y0, cell, g, offsets, items) exactly as dsu_zray_cast takes it; per view a colour image (res,
 * res, 3) u8 and an eroded mask (res, res) u8.  Outputs image (size, size, 3) u8 and source (size,
 * size) u8: 0 = not projected (image 0), 1 = front, 2 = back.  One thread per texel, one workgroup
 * per 16x16 tile.  Everything in float64 from the f32 inputs, in this operand order:
 *   1. the texel (row r, column c) with m = face_id >= 0 (a face with an index outside [0, n_verts)
 *      projects nothing) samples (x, y) = (c, size - 1 - r); w0, w1, w2 and area as in c. above,
 *      b_i = w_i / area.
 *   2. p = (b0 Pa + b1 Pb) + b2 Pc per coordinate, Pa, Pb, Pc the positions of m's vertices.  A
 *      non-finite p projects nothing.
 *   3. the front view (sign +1) is tested, then the back view (sign -1); the first that passes
 *      gives source and colour.  A view passes when
 *      facing:      ((Pbx - Pax)(Pcy - Pay) - (Pby - Pay)(Pcx - Pax)) sign > 0;
 *      pixel:       X = rint((+-px + 0.5)(res - 1)), px negated for the back view,
 *                   Y = rint((-py + 0.5)(res - 1)), half to even, both clamped to [0, res - 1]
 *                   (get_color_from_image, coloring_utils.py:67-86); mask[Y][X] > 0;
 *      unoccluded:  the grid cell of ((float)px, (float)py) is walked; for every listed triangle
 *                   f != m with dsu_zray_cast's edge functions e0, e1, e2 at (px, py),
 *                   ar = (e0 + e1) + e2 != 0 and (all e >= 0 or all e <= 0):
 *                   z_f = ((e0 z0 + e1 z1) + e2 z2) / ar; the texel is occluded when
 *                   (z_f - pz) sign > z_tolerance for any such f.
 *   4. the colour is the drawing's uint8 pixel [Y][X] of that view, copied.
 * No atomics: two runs give the same bits.  A triangle that covers (px, py) has a box that
 * contains the float casts, so the result does not depend on the grid's resolution.
 * DSU_EINVAL before any launch: size outside 1..8192, res outside 1..16384, g outside 1..4096,
 * cell <= 0 or not finite, x0 or y0 not finite, z_tolerance negative or not finite, n_verts or
 * n_faces negative or above 2^30, image or source NULL; and, with n_faces > 0, n_verts == 0 or any
 * other pointer NULL.  n_faces == 0: DSU_OK, image and source zeroed, the other pointers unread.
 * The mesh must be wound outward in this frame (as marching cubes leaves it): the facing test reads
 * the winding, and a mesh wound inward projects nothing its views can see.
 * It is computed by j.'s text at s = 1, filter 0, count = NULL (csrc/uv_project_area.h).
 *
 * f. dsu_uv_field_points: the sample points of the field bake (an extension: the reference bakes
 * vertex colours, which hold no more detail than the vertices do; here the optimised texture field
 * is evaluated per texel).  uvs, indices, size and face_id (size, size) i32 as dsu_uv_bake wrote
 * them; positions (n_verts, 3) f32 are the atlas vertices IN THE FIELD'S FRAME (the world-frame
 * vertices the export receives, before halving, axis swap, thinning, smoothing and shear, which
 * move vertices but keep their order); texels (n_texels) i32: linear indices r size + c of the
 * texels to sample, ascending (the caller lists nonzero(face_id >= 0)); s: sub-samples per axis,
 * 1..8.  Outputs points (n_texels, s s, 3) f32 and valid (n_texels, s s) u8.  One thread per
 * (texel, sub-sample), the sub-sample index fastest.  Everything in float64 from the f32 inputs, in
 * this operand order.  Per texel (r, c) with m = face_id[r][c], sub-sample j = jy s + jx:
 *   1. (x, y) = (c + o(jx), (size - 1 - r) + o(jy)),  o(i) = (2 i + 1 - s) / (2 s): an s x s grid
 *      centred on the texel's own sample point and one texel wide.  For s = 1 it is that point,
 *      the one dsu_uv_bake tests.
 *   2. w0, w1, w2 and area exactly as in c. (vertex positions (double)u * size), b_i = w_i / area.
 *      The b_i are NOT clamped: a sub-sample outside face m is evaluated on the affine extension of
 *      m (no second raster, no dependence on neighbouring faces; the field is defined off the
 *      surface too).
 *   3. p = (b0 Pa + b1 Pb) + b2 Pc per coordinate, rounded once to f32.  For s = 1 the b_i and p
 *      are those of e., steps 1-2.
 *   4. valid = 1 when m is in [0, n_faces), its three indices are in [0, n_verts), area is finite
 *      and > 0 and the three f32 coordinates of p are finite (a float64 p beyond the f32 range is
 *      not); otherwise valid = 0 and the point is (0, 0, 0): the evaluator never sees a NaN.  A
 *      texel index outside [0, size size) reads nothing and is invalid.
 * DSU_EINVAL before any launch: size outside 1..8192, s outside 1..8, n_verts, n_faces or n_texels
 * negative or above 2^30, points or valid NULL; and, with n_texels > 0, face_id or texels NULL, or
 * with n_faces > 0 as well, n_verts == 0 or uvs, indices or positions NULL.  n_texels == 0: DSU_OK,
 * nothing read or written.
 *
 * g. dsu_uv_field_resolve: colours (n_texels, s s, 3) f32 (the field evaluated at the points of
 * f.), valid and texels as above -> image (size, size, 3) u8, written ONLY at the listed texels.
 * Per texel and channel: sum = the (double)colour of the valid samples added in ascending j, n =
 * their count.  n == 0: the texel is left untouched (the caller's fallback stays).  Otherwise the
 * byte is dsu_uv_bake's quantisation of sum / n: times 255, clipped to [0, 255], truncated, NaN ->
 * 0.  One thread per listed texel; a texel index outside [0, size size) writes nothing; the list
 * must not name a texel twice.  No atomics: two runs give the same bits.
 * DSU_EINVAL before any launch: size outside 1..8192, s outside 1..8, n_texels negative or above
 * 2^30, image NULL; and, with n_texels > 0, colours, valid or texels NULL.  n_texels == 0: DSU_OK.
 *
 * dsu_uv_field_points_host / dsu_uv_field_resolve_host: HOST functions on HOST arrays — the same
 * two texts (csrc/uv_field.h) compiled for the CPU, with the same argument checks, so that the
 * rule can be held bit for bit without a device.
 *
 * h. / i. Seam levelling (an extension; Lempitsky & Ivanov 2007): where the drawings of e. are
 * composed over a fallback bake (the vertex bake of c. or the field bake of g.), the two disagree in
 * tone and a step runs along every border between them.  The drawing texels are left alone; the
 * fallback texels get a colour offset that equals drawing - fallback at the border and is the
 * harmonic extension of that over the MESH elsewhere (not over the texture: the border crosses the
 * charts).  Inputs of both steps: the atlas (uvs, indices, size) and face_id (size, size) i32 as
 * dsu_uv_bake wrote it; source (size, size) u8 and proj (size, size, 3) u8 as dsu_uv_project wrote
 * them; fallback (size, size, 3) u8, the vertex or field bake BEFORE the gutter fill; group
 * (n_verts) i32, the welded class of every atlas vertex in [0, n_groups) — the chart copies of one
 * mesh vertex, and the coincident vertices marching cubes leaves behind, are one unknown
 * (nsr/uv.seam_groups).  A face m is SOUND at a texel (row r, column c) when m is in [0, n_faces),
 * its three indices are in [0, n_verts), the three groups g_0, g_1, g_2 of its corners are in
 * [0, n_groups), and, with w0, w1, w2 and area at (x, y) = (c, size - 1 - r) exactly as in e. step
 * 1, area is finite and > 0; then b_i = w_i / area.
 *
 * h. dsu_uv_seam_gather.  One thread per texel, one workgroup per 16x16 tile.  A texel with
 * source == 0, or whose face m = face_id[r][c] is not sound, adds nothing.  Otherwise, per corner i:
 *     q_i = (int64) floor(b_i 2^20 + 0.5), clipped to [0, 2^20]  (a NaN counts as 0);
 * and for each corner with q_i > 0
 *     den[g_i] += q_i,    num[g_i][ch] += q_i ((int) proj[ch] - (int) fallback[ch])   ch = 0, 1, 2
 * as 64-bit INTEGER atomic adds into the caller-zeroed den (n_groups) i64 and num (n_groups, 3) i64
 * (the kernel first sums a tile's contributions per group in LDS, also in 64-bit integers, and adds
 * each group's four sums once).  Integer sums do not depend on the order of arrival or on how they
 * are grouped: two runs give the same bits.  |num| is at most size^2 2^20 255 < 2^54 for
 * size <= 8192.
 * DSU_EINVAL before any launch: size outside 1..8192, n_verts, n_faces or n_groups negative or
 * above 2^30, num or den NULL.  Then n_groups == 0 or n_faces == 0: DSU_OK, nothing read or
 * written.  Then DSU_EINVAL for n_verts == 0 or any input pointer NULL.
 *
 * The host (nsr/uv.seam_offsets) turns the sums into one offset d (n_groups, 3) f64 per group: a
 * group with den >= 2^20 (one whole texel's weight) is KNOWN and has d = num / den; the others are
 * the unknowns of the uniform graph Laplacian over the welded mesh's edges, deg(u) d_u - sum of the
 * unknown neighbours' d = sum of the known neighbours' d, solved for the three channels at once
 * with dsu_spd_cg_block; an unknown in a component without a known group has d = 0.  Uniform
 * weights keep the matrix an M-matrix: no offset leaves the range of the known ones.
 *
 * i. dsu_uv_seam_apply.  One thread per texel, tiles as above; every texel of image (size, size, 3)
 * u8 is written.  In this order:
 *   face_id < 0:       0, 0, 0;
 *   source != 0:       the bytes of proj;
 *   the face is sound: per channel  e = (b0 d[g_0][ch] + b1 d[g_1][ch]) + b2 d[g_2][ch],
 *                      v = (double) fallback[ch] + e;  the byte is floor(v + 0.5) clipped to
 *                      [0, 255], or the fallback byte when v is not finite;
 *   otherwise:         the bytes of fallback.
 * No atomics.  The gutter fill (d.) runs over the result.
 * DSU_EINVAL before any launch: size outside 1..8192, n_verts, n_faces or n_groups negative or
 * above 2^30, image, face_id, source, proj or fallback NULL; and, with n_faces > 0 and
 * n_groups > 0, n_verts == 0 or uvs, indices, group or d NULL.  With n_faces == 0 or n_groups == 0
 * no face is sound and uvs, indices, group and d are not read.
 *
 * dsu_uv_seam_gather_host / dsu_uv_seam_apply_host: HOST functions on HOST arrays — the same two
 * texts (csrc/uv_seam.h) compiled for the CPU (a plain loop over the texels and a plain +=), with
 * the same argument checks.
 *
 * j. dsu_uv_project_area: e. with the drawings read at s x s points per texel instead of one (an
 * extension; csrc/uv_project_area.hip).  At 1024^2 texels over 2048^2 drawings a texel is about
 * three pixels wide and e. reads one pixel in ten: ink lines alias before any later filter sees
 * them.  The inputs are exactly e.'s, plus s (sub-samples per axis, 1..8) and filter (0 nearest, 1
 * bilinear).  Outputs image (size, size, 3) u8, source (size, size) u8 as in e., and count (size,
 * size) u8, which may be NULL.  One thread per texel, one workgroup per 16x16 tile.  Everything in
 * float64 from the f32 / u8 inputs, in this operand order:
 *   1. the texel (row r, column c) with m = face_id[r][c]; m outside [0, n_faces), or an index of m
 *      outside [0, n_verts), projects nothing.
 *   2. the view is a property of the face: with nz = (Pbx - Pax)(Pcy - Pay) - (Pby - Pay)(Pcx - Pax)
 *      as in e. step 3, front (sign +1) if nz > 0, back (sign -1) if nz < 0, otherwise none (this is
 *      e.'s "front, then back, first that passes": a face passes the facing test of at most one
 *      view).
 *   3. sub-sample j = jy s + jx sits at (x, y) = (c + o(jx), (size - 1 - r) + o(jy)), o(i) =
 *      (2 i + 1 - s) / (2 s): the grid of f.  w0, w1, w2, area and b_i = w_i / area as in c., NOT
 *      clamped: a sub-sample outside face m lies on the affine extension of m (no second raster).
 *      p = (b0 Pa + b1 Pb) + b2 Pc per coordinate.
 *   4. a sub-sample PASSES when p is finite; the mask of its NEAREST pixel (X, Y of e., half to even,
 *      clamped) is > 0; and it is unoccluded by e.'s test at (px, py, pz): the cell of ((float)px,
 *      (float)py), f != m skipped, the same z_tolerance.
 *   5. a passing sub-sample's value per channel: filter 0, the byte at [Y][X].  Filter 1, with
 *      fx = (+-px + 0.5)(res - 1) and fy = (-py + 0.5)(res - 1), both clamped to [0, res - 1],
 *      x0 = min(floor(fx), max(res - 2, 0)), x1 = min(x0 + 1, res - 1), tx = fx - x0, likewise y0, y1,
 *      ty:  value = ((1 - ty)((1 - tx) c00 + tx c10)) + (ty ((1 - tx) c01 + tx c11)), c_xy the byte at
 *      [y_][x_].  The mask is still tested at the nearest pixel only (the erosion keeps the other
 *      three inside the drawing).
 *   6. n = the number of passing sub-samples; count = n.  If n = 0, one more sample at the texel's
 *      own point (o = 0) is put through steps 3-5 (for odd s it would repeat the centre sample and
 *      change nothing); if that fails as well, source = 0 and image = 0.
 *   7. otherwise source = 1 (front) or 2 (back); per channel the values are summed in ascending j and
 *      the byte is floor(sum / n + 0.5) clipped to [0, 255], n being 1 when the extra sample was used.
 * It follows that (a) s = 1, filter = 0 is e. byte for byte; (b) wherever e. gives source != 0 this
 * entry gives the same source for any s and filter (the texel's own point is a sample of every odd
 * grid and the extra sample of every even one), so the projected set can only grow; (c) the result
 * does not depend on the grid, for e.'s reason.  The kernel takes the sub-samples four at a time,
 * walks each cell the four points name once and tests every listed triangle against all of them: a
 * triangle met through another point's cell, or twice, changes nothing, since occlusion is an OR
 * and a triangle that covers a point is in that point's own list.  At s = 1 every entry, the host
 * entry included, runs the one-point instantiation of the same text instead: the texel's own point,
 * alone in its group.  No atomics: two runs give the same bits.
 * DSU_EINVAL before any launch: as e., and s outside 1..8 or filter outside {0, 1}.  n_faces == 0:
 * DSU_OK, image, source and count (when given) zeroed, the other pointers unread.
 *
 * dsu_uv_project_area_host: a HOST function on HOST arrays (tris and the grid arrays included; a
 * grid of one cell, g = 1 with offsets [0, n_faces] and items 0 .. n_faces - 1, is valid by (c)) —
 * the same text (csrc/uv_project_area.h) compiled for the CPU, with the same argument checks.  At
 * s = 1, filter 0, count = NULL this call is the host statement of dsu_uv_project. */
#define DSU_UV_COUNT 0
#define DSU_UV_FILL 1
#define DSU_UV_RASTER 2
int dsu_uv_face_labels(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces,
                       double* normal, int32_t* label, double* area, void* stream);
int dsu_uv_components(const int32_t* adjacency, const int32_t* label, int64_t n_faces, int32_t* chart,
                      int32_t* flag, int32_t check_every, int32_t max_rounds, int32_t* out_rounds,
                      void* stream);
int64_t dsu_uv_bake_workspace_bytes(int32_t size);
int dsu_uv_bake(int32_t stage, const float* uvs, const int32_t* indices, const float* colours,
                const double* depth, int64_t n_verts, int64_t n_faces, int32_t size, void* workspace,
                int64_t workspace_bytes, int32_t* items, int64_t n_items, uint8_t* image, int32_t* face_id,
                uint8_t* demote, void* stream);
int dsu_uv_dilate(const uint8_t* image_in, const uint8_t* covered_in, int32_t size, uint8_t* image_out,
                  uint8_t* covered_out, void* stream);
int dsu_uv_project(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                   int64_t n_faces, int32_t size, const int32_t* face_id, const float* tris, float x0, float y0,
                   float cell, int32_t g, const int32_t* offsets, const int32_t* items, const uint8_t* color_front,
                   const uint8_t* mask_front, const uint8_t* color_back, const uint8_t* mask_back, int32_t res,
                   double z_tolerance, uint8_t* image, uint8_t* source, void* stream);
int dsu_uv_field_points(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                        int64_t n_faces, int32_t size, const int32_t* face_id, const int32_t* texels,
                        int64_t n_texels, int32_t s, float* points, uint8_t* valid, void* stream);
int dsu_uv_field_resolve(const float* colours, const uint8_t* valid, const int32_t* texels, int64_t n_texels,
                         int32_t s, int32_t size, uint8_t* image, void* stream);
int dsu_uv_field_points_host(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                             int64_t n_faces, int32_t size, const int32_t* face_id, const int32_t* texels,
                             int64_t n_texels, int32_t s, float* points, uint8_t* valid);
int dsu_uv_field_resolve_host(const float* colours, const uint8_t* valid, const int32_t* texels, int64_t n_texels,
                              int32_t s, int32_t size, uint8_t* image);
int dsu_uv_seam_gather(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                       int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                       const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, int64_t* num,
                       int64_t* den, void* stream);
int dsu_uv_seam_apply(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                      int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                      const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, const double* d,
                      uint8_t* image, void* stream);
int dsu_uv_seam_gather_host(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                            int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                            const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, int64_t* num,
                            int64_t* den);
int dsu_uv_seam_apply_host(const float* uvs, const int32_t* indices, const int32_t* group, int64_t n_verts,
                           int64_t n_faces, int64_t n_groups, int32_t size, const int32_t* face_id,
                           const uint8_t* source, const uint8_t* proj, const uint8_t* fallback, const double* d,
                           uint8_t* image);
int dsu_uv_project_area(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                        int64_t n_faces, int32_t size, const int32_t* face_id, const float* tris, float x0, float y0,
                        float cell, int32_t g, const int32_t* offsets, const int32_t* items,
                        const uint8_t* color_front, const uint8_t* mask_front, const uint8_t* color_back,
                        const uint8_t* mask_back, int32_t res, double z_tolerance, int32_t s, int32_t filter,
                        uint8_t* image, uint8_t* source, uint8_t* count, void* stream);
int dsu_uv_project_area_host(const float* uvs, const int32_t* indices, const float* positions, int64_t n_verts,
                             int64_t n_faces, int32_t size, const int32_t* face_id, const float* tris, float x0,
                             float y0, float cell, int32_t g, const int32_t* offsets, const int32_t* items,
                             const uint8_t* color_front, const uint8_t* mask_front, const uint8_t* color_back,
                             const uint8_t* mask_back, int32_t res, double z_tolerance, int32_t s, int32_t filter,
                             uint8_t* image, uint8_t* source, uint8_t* count);

/* remesh() (instant_nsr/utils/mesh_utils.py:10-22, called by models/geometry.py:63-64 with
 * face_count 50000): quadric edge-collapse decimation of a triangle mesh down to `target_faces`
 * triangles.  HOST function on HOST arrays (as in the reference, where trimesh hands the mesh to
 * Open3D's simplify_quadric_decimation): verts (n_verts,3) float64, faces (n_faces,3) int32.
 * out_verts / out_faces must hold n_verts / n_faces rows; the counts come back through
 * out_n_verts / out_n_faces.  boundary_weight: weight of the boundary-edge planes (Open3D: 1.0).
 * flags bit 0: skip the link-condition test (collapses may then create non-manifold edges, as
 * Open3D's can).  Collapses stop at the first face count <= target_faces (a collapse removes two
 * triangles, one on a boundary edge); more remain when no admissible collapse is left. */
int dsu_mesh_decimate_quadric(const double* verts, int64_t n_verts, const int32_t* faces,
                              int64_t n_faces, int64_t target_faces, double boundary_weight,
                              int32_t flags, double* out_verts, int64_t* out_n_verts,
                              int32_t* out_faces, int64_t* out_n_faces);

/* The same, seeded with per-vertex quadrics (n_verts,10: a00 a01 a02 a11 a12 a22 b0 b1 b2 c of
 * [A b; b^T c]) instead of computing them from the input triangles — the finishing pass after
 * dsu_mesh_decimate_parallel, whose collapses have accumulated them. */
int dsu_mesh_decimate_quadric_q(const double* verts, int64_t n_verts, const int32_t* faces,
                                int64_t n_faces, int64_t target_faces, double boundary_weight,
                                int32_t flags, const double* vertex_quadrics, double* out_verts,
                                int64_t* out_n_verts, int32_t* out_faces, int64_t* out_n_faces);

/* The bulk of the same `remesh` call (mesh_utils.py:10-22; geometry.py:63-64 hands it the 512^3
 * marching-cubes mesh, 1-3 M triangles) ON THE DEVICE: rounds of independent quadric edge collapses
 * with the serial function's admissibility rules (csrc/mesh_decimate_gpu.hip).  verts (n_verts,3)
 * f64 and faces (n_faces,3) i32 are DEVICE arrays updated in place: surviving vertices keep their
 * index (positions move), the live triangles are compacted to the first *out_n_faces rows.
 * Rounds run while the live count is above stop_faces (at most max_rounds) and a round never takes
 * the count below floor_faces (<= stop_faces); the caller finishes with
 * dsu_mesh_decimate_quadric_q(out_quadrics) which lands on the exact target.  out_quadrics:
 * (n_verts,10) f64 device or NULL.  out_stats: host int32[3] = rounds, collapses, rejections, or
 * NULL.  Synchronises the stream (one count per round is read back).  flags as above. */
int64_t dsu_mesh_decimate_parallel_workspace_bytes(int64_t n_verts, int64_t n_faces);
int dsu_mesh_decimate_parallel(double* verts, int64_t n_verts, int32_t* faces, int64_t n_faces,
                               int64_t stop_faces, int64_t floor_faces, double boundary_weight,
                               int32_t flags, int32_t max_rounds, double* out_quadrics,
                               int64_t* out_n_faces, int32_t* out_stats, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* One implicit step of trimesh.smoothing.filter_laplacian (save_mesh, mesh_utils.py:42-45):
 * solves (I + lamb (I - L)) X = rhs for the umbrella operator L given as CSR neighbour lists
 * (offsets (n_verts+1), neighbours: int32 device), rhs / x / tmp (n_verts,3) float64 device.
 * x holds the starting guess on entry (rhs itself is a good one) and the solution on return;
 * `sweeps` Jacobi sweeps (even; the error contracts by lamb / (1 + lamb) per sweep). */
int dsu_umbrella_implicit_solve(const int32_t* offsets, const int32_t* neighbours, int64_t n_verts,
                                double lamb, const double* rhs, double* x, double* tmp,
                                int32_t sweeps, void* stream);

/* Image-side host steps of thinning_processing (instant_nsr/utils/thinning_utils.py:205-218) on
 * HOST arrays (H,W) uint8, non-zero = character:
 *   cv2.distanceTransform(mask, cv2.DIST_L2, 5)            -> out (H,W) float32
 *   skimage.morphology.skeletonize(mask, method='lee')     -> out (H,W) uint8, 0 / 255 */
int dsu_distance_transform_l2_5x5(const uint8_t* mask, int32_t H, int32_t W, float* out);
int dsu_skeletonize_lee_2d(const uint8_t* img, int32_t H, int32_t W, uint8_t* out);

/* ------------------------------------------------------------------------------------
 * Thickness map: where along z the inside of a mesh lies under every sample of an xy lattice.
 * An extension of the reference (its skeletons come fitted from Mixamo):
 * drawingspinup_amd/animate/rig.py lifts 2-D joint marks into the mesh with it.
 * csrc/mesh_thickness.h holds the text, compiled for the kernel and for the host entry;
 * tests/mesh_thickness_ref.py restates it in float64 numpy.
 *
 * verts (n_verts,3) f32, faces (n_faces,3) i32.  Lattice x0, y0, h > 0 (finite), W x H samples
 * (0 .. DSU_THICKNESS_MAX_SIDE each): sample (r, c) is the point s = (x0 + (c + 1/2) h,
 * y0 + (r + 1/2) h), its ray runs along z.
 *
 * Rule per sample, in float64 from the f32 inputs, in one operand order, no fused products.  A
 * triangle with an index outside [0, n_verts) or a non-finite coordinate is ignored.  For triangle
 * (a, b, c): area2 = (b.x - a.x)(c.y - a.y) - (b.y - a.y)(c.x - a.x); area2 == 0 skips it; area2 < 0
 * swaps b and c (and negates area2).  E(p->q) = (q.x - p.x)(s.y - p.y) - (q.y - p.y)(s.x - p.x) for
 * the edges a->b, b->c, c->a.  The sample is covered when every E > 0, or E == 0 on a top-left
 * edge of the counter-clockwise triangle (dy < 0, or dy == 0 and dx < 0, with d = q - p): a sample
 * on an edge that two triangles share is counted once where they face the same way, 0 or 2 times on
 * a silhouette.  The crossing's z = ((E(b->c) / area2) a.z + (E(c->a) / area2) b.z) + (E(a->b) /
 * area2) c.z.
 * The crossings are ordered by (z, face index) and paired (0,1), (2,3), ...; an odd last one is
 * dropped.  The thickest pair wins (z1 - z0), ties go to the lower z.
 *   mid (H,W) f64        (z0 + z1) / 2 of that pair, 0 without a pair
 *   thickness (H,W) f64  z1 - z0, 0 without a pair
 *   count (H,W) i32      the number of crossings (odd: the mesh is open there)
 * Deviation from a winding-number inside test: parity.  Closed components that interpenetrate
 * cancel where they overlap; a marching-cubes export has none.
 *
 * dsu_mesh_thickness_ortho: device arrays.  The triangles come through the xy grid of
 * dsu_zgrid_count / dsu_zgrid_fill over verts[faces] (grid_x0, grid_y0, grid_cell, g, offsets
 * (g*g + 1), items (n_items)); any such grid gives the same result, a cell of 16 x 16 samples
 * (ops.mesh_thickness) lets a workgroup walk one list.  One thread per sample, 256 = 16 x 16 per
 * workgroup, the lists staged through LDS 256 triangles at a time; a thread holds no array of its
 * crossings: walk k finds pair k as the two lowest (z, face) above pair k - 1.  No atomics:
 * two runs give the same bits, and the bits of the host entry.
 * dsu_mesh_thickness_ortho_host: a HOST function on HOST arrays, the same text; it bins the
 * triangles itself. */
#define DSU_THICKNESS_MAX_SIDE 4096
int dsu_mesh_thickness_ortho(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                             float grid_x0, float grid_y0, float grid_cell, int32_t g,
                             const int32_t* offsets, const int32_t* items, int64_t n_items, double x0,
                             double y0, double h, int32_t W, int32_t H, double* mid, double* thickness,
                             int32_t* count, void* stream);
int dsu_mesh_thickness_ortho_host(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                  double x0, double y0, double h, int32_t W, int32_t H, double* mid,
                                  double* thickness, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* DSU_HIP_H */
