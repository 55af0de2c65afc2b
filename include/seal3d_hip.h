/*
 * seal3d_hip.h — C ABI of libseal3d_hip.so, the MI355X (gfx950) replacement for
 * the five CUDA extension modules on Seal-3D's render/train hot path.
 *
 * One entry point per function the reference binds with pybind11
 * (`_raymarching`, `_gridencoder`, `_shencoder`, `_freqencoder`, `_ffmlp`); the
 * reference declaration each one replaces is cited above it.  Conventions:
 *   - plain device pointers + explicit sizes, no torch types;
 *   - every function takes the HIP stream to launch on and returns 0 on
 *     success, non-zero on error (message: s3d_last_error(), thread-local);
 *   - the CALLER allocates every output (and zero-initialises those the
 *     reference zero-initialises: xyzs/dirs/deltas, grad_embeddings,
 *     grad_sigmas/grad_rgbs, SH grad_inputs) — raymarching.py:205-207,
 *     grid.py:77, raymarching.py:283-284, sphere_harmonics.py:50;
 *   - kernels never allocate; functions that need scratch take a caller-owned
 *     workspace whose size the matching *_workspace_size() reports;
 *   - dtype: S3D_F32 / S3D_F16 select the element type of `void*` tensors;
 *   - n_valid (grid encoder, ffmlp, NGP head; NULL = off): DEVICE pointer to the sample count the ray marcher
 *     left in `counter[0]` (raymarching.cu:431-437).  The training step marches into buffers of a static extent
 *     B (raymarching.py:205-207 sizes them from a running mean) and only the first *n_valid rows hold samples;
 *     with the pointer, rows [round_up(*n_valid, 128), B) are absent for the call — neither read nor written,
 *     their outputs keep whatever the caller's buffer held — so the per-sample work follows the samples without
 *     a host read-back (the step stays HIP-graph capturable with one generous B).  Strides and layouts are
 *     those of B.  Results for the valid rows and every reduced gradient are identical to a call without it on
 *     the same buffers with zero gradient in the tail.
 * INTEGRATION.md shows the pybind / ctypes stub a maintainer of the reference
 * would add on top of this header.
 */
#ifndef SEAL3D_HIP_H
#define SEAL3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* s3d_stream_t; /* hipStream_t */

enum { S3D_F32 = 0, S3D_F16 = 1 };
enum { S3D_OK = 0, S3D_ERR_INVALID = 1, S3D_ERR_HIP = 2, S3D_ERR_UNSUPPORTED = 3 };

const char* s3d_last_error(void);
/* "seal3d-hip <version> gfx950" */
const char* s3d_version(void);

/* ------------------------------------------------------------------ raymarching
 * raymarching/src/raymarching.h:7-18 (bindings.cpp:6-17) */

/* raymarching.h:7  void near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars)
 * Build extension (all optional, NULL/0 = the reference call): noises [N] receives the per-ray jitter of march_rays_train's
 * `perturb` (raymarching.py:211 draws it with torch.rand) as a counter-based uniform u01(noise_key, *noise_step, ray) —
 * the step number lives in device memory, so a graph-replayed step draws fresh jitter without host-side RNG state. */
int s3d_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N,
                           float min_near, float* nears, float* fars, float* noises, const int32_t* noise_step,
                           uint32_t noise_key, s3d_stream_t stream);

/* raymarching.h:8  void sph_from_ray(rays_o, rays_d, radius, N, coords) */
int s3d_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords,
                     s3d_stream_t stream);

/* Test hook (no reference entry point): the cascade selection of the marching kernels, `mip_from_pos` / `mip_from_dt`
 * (raymarching.cu:42-54), on arrays: xyz [N,3] -> mip_pos [N], dt [N] -> mip_dt [N]; either output may be NULL. */
int s3d_mip_levels(const float* xyz, const float* dt, uint32_t N, uint32_t H, uint32_t C, int32_t* mip_pos, int32_t* mip_dt,
                   s3d_stream_t stream);

/* raymarching.h:9  void morton3D(coords, N, indices) */
int s3d_morton3D(const int32_t* coords, uint32_t N, int32_t* indices, s3d_stream_t stream);

/* raymarching.h:10 void morton3D_invert(indices, N, coords) */
int s3d_morton3D_invert(const int32_t* indices, uint32_t N, int32_t* coords, s3d_stream_t stream);

/* raymarching.h:11 void packbits(grid, N, density_thresh, bitfield); N = output bytes */
int s3d_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield,
                 s3d_stream_t stream);

/* Build extension — the steady-state occupancy sweep of NeRFRenderer.update_extra_state (nerf/renderer.py:497-538: H^3/4
 * uniform cells + H^3/4 uniform picks among the occupied cells per cascade, jittered inside the cell, density queried by the
 * caller, then density_grid = max(density_grid * decay, sample) where both are >= 0) without host syncs or index tensors:
 * s3d_sweep_draw: u_uniform / u_occupied [N] doubles in [0, 1) (ascending order makes the queries walk the Z-curve),
 *   occ_csum [H^3] = inclusive prefix count of cells with density > 0 -> cells [2N] (morton index = density_grid index)
 *   and xyzs [2N, 3] (jitter = counter-based u01(noise_key, *noise_step, 3 i + d); noise_step may be NULL = 0).
 * s3d_sweep_update: one cascade's density_grid [n_cells] updated in place from (cells, sigma * density_scale) [n]; of the
 *   samples that fall in one cell the largest is kept (the reference's indexed assignment keeps an arbitrary one);
 *   *grid_sum = sum(max(density_grid, 0)) afterwards (fixed summation order); step_counter (optional) += 1. */
int s3d_sweep_draw(const double* u_uniform, const double* u_occupied, const int32_t* occ_csum, uint32_t N, uint32_t H,
                   float bound, float half_cell, uint32_t noise_key, const int32_t* noise_step, int32_t* cells,
                   float* xyzs, s3d_stream_t stream);
size_t s3d_sweep_update_workspace_size(uint32_t n_cells);
int s3d_sweep_update(float* density_grid, uint32_t n_cells, const int32_t* cells, const void* sigma, int sigma_dtype,
                     uint32_t n, float density_scale, float decay, void* workspace, size_t workspace_bytes,
                     float* grid_sum, int32_t* step_counter, s3d_stream_t stream);

/* The same sweep without a host value between its launches (what a graph-replayed trainer runs).
 * s3d_sweep_draw_native: s3d_sweep_draw without the [H^3] prefix array.  Three launches: per block of 1,024 cells the count and
 *   the bit mask of the cells with density > 0, and tmp[H^3] = -1; a one-workgroup scan of the block counts; the draw (cells
 *   [2N], xyzs [2N, 3], jitter as in s3d_sweep_draw).  The occupied half is searchsorted(cumsum(grid > 0),
 *   floor(u_occupied * #occupied), right=True) clamped to H^3 - 1, found in the scanned block counts and the block's mask.
 * s3d_sweep_scatter_update: tmp (filled by the draw) <- max over the samples, density_grid <- EMA-max; partial
 *   [s3d_sweep_partial_stride()] receives the per-block sums of max(density_grid, 0); sigma is read `sigma_stride` elements apart.
 * s3d_sweep_tail: one workgroup; partial [cascades, s3d_sweep_partial_stride()] -> record = {float mean(max(grid, 0)), float
 *   min(mean, density_thresh), uint32 lo, hi of the int64 sum of step_ring[r, 0], r < min(16, *local_step)} (16 bytes);
 *   *sweep_step (optional) += 1.
 * s3d_packbits_record: s3d_packbits with the threshold taken from such a record. */
size_t s3d_sweep_draw_native_workspace_size(uint32_t H);
int s3d_sweep_draw_native(const double* u_uniform, const double* u_occupied, const float* density_grid, uint32_t N, uint32_t H,
                          float bound, float half_cell, uint32_t noise_key, const int32_t* noise_step, float* tmp, int32_t* cells,
                          float* xyzs, void* workspace, size_t workspace_bytes, s3d_stream_t stream);
uint32_t s3d_sweep_partial_stride(void);
int s3d_sweep_scatter_update(float* density_grid, uint32_t n_cells, const int32_t* cells, const void* sigma, int sigma_dtype,
                             uint32_t sigma_stride, uint32_t n, float density_scale, float decay, float* tmp, float* partial,
                             s3d_stream_t stream);
int s3d_sweep_tail(const float* partial, uint32_t cascades, uint32_t n_cells, float density_thresh, const int32_t* step_ring,
                   const int32_t* local_step, int32_t* sweep_step, void* record, s3d_stream_t stream);
int s3d_packbits_record(const float* grid, uint32_t N, const void* record, uint8_t* bitfield, s3d_stream_t stream);

/* raymarching.h:13 void march_rays_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M,
 *                                        nears, fars, xyzs, dirs, deltas, rays, counter, noises)
 * Spans are packed in RAY ORDER (deterministic; one valid outcome of the reference's atomic
 * reservation, raymarching.cu:405-406).  counter[0] += total samples, counter[1] += N.
 * path (kernel choice, same results): 0 = auto (wave-per-ray up to 16,384 rays), 1 = lane-per-ray, 2 = wave-per-ray,
 *   3 = wave-per-ray without the single-cascade fast path (its morton table, batched probes and voxel-run shortcut).
 * Rows no ray fills are written as zeros where a consumer bounded by the device-side count (`n_valid`: the count rounded
 * up to 128 rows, at most M) still reads them: [total, round_up(total, 128)) and, for the one ray that straddles the
 * budget (offset < M < offset + steps, dropped like in the reference), [offset, M).  The reference zero-fills all M rows
 * beforehand (raymarching.py:205-207); callers that read every row must still do so.  s3d_composite_rays_train_backward
 * does the same for grad_sigmas / grad_rgbs (plus the samples behind a ray's early termination).
 * aabb != NULL (build extension): s3d_near_far_from_aabb(aabb, min_near, noise_step, noise_key) is part of this call —
 * nears / fars and, with noise_step, noises are then OUTPUTS (written before they are used; same values). */
size_t s3d_march_rays_train_workspace_size(uint32_t N, uint32_t max_steps);
int s3d_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound,
                         float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                         uint32_t M, const float* nears, const float* fars, float* xyzs, float* dirs,
                         float* deltas, int32_t* rays, int32_t* counter, const float* noises,
                         void* workspace, size_t workspace_bytes, int path, const float* aabb, float min_near,
                         const int32_t* noise_step, uint32_t noise_key, s3d_stream_t stream);

/* raymarching.h:14 void composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh,
 *                                                    weights_sum, depth, image)
 * path (both directions): 0 = wave-per-ray compositing, 1 = lane-per-ray (serial chain, the reference's order). */
int s3d_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas,
                                     const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                     float* weights_sum, float* depth, float* image, int path,
                                     s3d_stream_t stream);

/* raymarching.h:15 void composite_rays_train_backward(grad_weights_sum, grad_image, sigmas, rgbs, deltas,
 *                       rays, weights_sum, image, M, N, T_thresh, grad_sigmas, grad_rgbs) */
int s3d_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image,
                                      const float* sigmas, const float* rgbs, const float* deltas,
                                      const int32_t* rays, const float* weights_sum, const float* image,
                                      uint32_t M, uint32_t N, float T_thresh, float* grad_sigmas,
                                      float* grad_rgbs, int path, s3d_stream_t stream);

/* Build extension — s3d_composite_rays_train_forward, s3d_bg_mse_forward(grad_loss) and s3d_composite_rays_train_backward of
 * one training ray batch as ONE launch (raymarching.py:238-291 + nerf/renderer.py:316 + nerf/utils.py:484-489): the wave that
 * composites a ray forms that ray's loss gradient (k = *grad_loss * 2 / (3N), the announced upstream gradient of the loss) and
 * walks its samples again for grad_sigmas / grad_rgbs; the loss value is summed by a one-workgroup launch behind it in
 * s3d_bg_mse_forward's order (two launches instead of three, the second off the backward's critical data).  Every output equals
 * the three-call sequence (wave-per-ray paths) bit for bit.  gt [N,3], bg_rgb = 3 HOST floats, gt_depth [N] or NULL (value-only
 * depth term), grad_image [N,3] / grad_weights_sum [N]: optional outputs (both or neither), workspace: 4N floats (scratch).
 * loss = NULL (also s3d_composite_rays_train_loss_bg): the one-workgroup launch is left out; the per-ray terms stay in `workspace`
 * until s3d_loss_terms_reduce, or a step tail of s3d_grid_encode_backward_adam_tail, sums them in the same order. */
int s3d_composite_rays_train_loss(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                  uint32_t M, uint32_t N, float T_thresh, const float* gt, const float* bg_rgb,
                                  const float* grad_loss, const float* gt_depth, float depth_weight,
                                  float* weights_sum, float* depth, float* image, float* grad_sigmas, float* grad_rgbs,
                                  float* grad_image, float* grad_weights_sum, float* loss, float* workspace,
                                  s3d_stream_t stream);
/* the one-workgroup sum of s3d_composite_rays_train_loss's per-ray terms on its own: workspace = that call's, with_depth = it
 * was given a gt_depth.  *loss = sum(sq) / 3N (+ depth_weight * sum(dabs) / N). */
int s3d_loss_terms_reduce(const float* workspace, uint32_t N, int with_depth, float depth_weight, float* loss, s3d_stream_t stream);

/* raymarching.h:17 void march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma,
 *                       max_steps, C, H, grid, nears, fars, xyzs, dirs, deltas, noises)
 * noises may be NULL (= all zero: no perturbation).  zero_unfilled (build extension): the reference's wrapper zero-fills
 * xyzs / dirs / deltas before every call (raymarching.py:324-326: unfilled slots must read as zeros, deltas == 0 ends a
 * ray's chunk); with zero_unfilled != 0 the kernel writes those zeros itself — the slots a ray does not fill and the rows
 * behind the last ray up to rows_total (up to the next multiple of 128 of the live rows when n_alive_dev is given) — and
 * the caller passes uninitialised buffers of rows_total rows.
 * Two launches on `stream` (a walk that records (t, previous t) per emitted sample in the sample's own `deltas` row — one
 * lane per ray with lane refill, or sixteen lanes per ray once few rays are alive — then one lane per row expanding it to
 * xyz / dir / (dt, t' - previous t)); n_alive * n_step must fit 32 bits. */
int s3d_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                   const float* rays_o, const float* rays_d, float bound, float dt_gamma,
                   uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* grid, const float* nears,
                   const float* fars, float* xyzs, float* dirs, float* deltas, const float* noises,
                   const int32_t* n_alive_dev, int32_t* n_rows_out, uint32_t rows_total, int zero_unfilled,
                   s3d_stream_t stream);

/* raymarching.h:18 void composite_rays(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs,
 *                       deltas, weights_sum, depth, image) — in place */
int s3d_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* rays_alive,
                       float* rays_t, const void* sigmas, const void* rgbs, const float* deltas,
                       float* weights_sum, float* depth, float* image, const int32_t* n_alive_dev,
                       int sigmas_dtype /* S3D_F32 | S3D_F16: the network's outputs as they come */, int rgbs_dtype,
                       s3d_stream_t stream);

/* Device-side replacement of the host compaction `rays_alive = rays_alive[rays_alive >= 0]`
 * (nerf/renderer.py:363): stable wave-ballot compaction of `in[0..n)` into `out`, count -> *n_out
 * (device int32).  Not in the reference's native surface; used by the build's renderer. */
size_t s3d_compact_alive_workspace_size(uint32_t n);
int s3d_compact_alive(const int32_t* in, uint32_t n, int32_t* out, int32_t* n_out, void* workspace,
                      size_t workspace_bytes, const int32_t* n_in_dev, s3d_stream_t stream);
/* Sync-free inference loop (nerf/renderer.py:341-367 reads the alive count back on every iteration): `n_alive` / `n` of
 * march_rays, composite_rays and compact_alive are then the host's UPPER BOUND (launch geometry, buffer extents) and the
 * optional `n_alive_dev` / `n_in_dev` point at the real count in device memory (NULL: the bound is the count); entries
 * past it are ignored.  march_rays leaves `*n_alive_dev * n_step` in `n_rows_out` (optional) — the `n_valid` of the
 * network kernels that follow.  The host refreshes its bound every few iterations only. */

/* ------------------------------------------------------------------ gridencoder
 * gridencoder/src/gridencoder.h:12-15 (bindings.cpp:6-8).
 * `S` and `H` as in the reference (S = log2(per_level_scale)); the per-level scale table
 * exp2f(l*S)*H-1 (gridencoder.cu:138) is evaluated ONCE ON THE HOST inside the call so that all
 * implementations agree on cell boundaries bit-for-bit; s3d_grid_level_scales exposes it. */
void s3d_grid_level_scales(uint32_t L, float S, uint32_t H, float* scales_out /* host, [L] */);

/* gridencoder.h:12 void grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H,
 *                        dy_dx, gridtype, align_corners, interp)
 * inputs [B,D] f32 in [0,1]; embeddings [sO,C] dtype; offsets [L+1] i32; outputs [L,B,C] dtype;
 * dy_dx [B,L,D,C] dtype or NULL.
 * bound: 0 = inputs already in [0,1] (the reference's native contract); > 0 = raw coordinates in [-bound, bound],
 * normalised in the kernel exactly like GridEncoder.forward does in torch (grid.py:146), dy_dx must be NULL.
 * live (optional, inference): device fp32, row b is live iff live[b * live_stride] != 0; other rows are written as zeros
 * without touching the table.  The inference loop passes `deltas` (nerf/renderer.py:355-360: march_rays leaves the
 * unused slots of a ray's chunk zero-filled and composite_rays stops at the first deltas == 0, raymarching.cu:740). */
int s3d_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets,
                            void* outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                            uint32_t H, void* dy_dx, uint32_t gridtype, int align_corners,
                            uint32_t interp, int dtype, float bound, const int32_t* n_valid,
                            const float* live, uint32_t live_stride, s3d_stream_t stream);
/* Build extension: TWO tables of identical geometry (offsets, C, L, S, H, gridtype, ...) encoded for the same points in one
 * launch — the density and the colour encoder of the network Seal-3D trains (nerf/network.py:99-128 calls them on the same x):
 * outputs_a / outputs_b [L, B, C] as s3d_grid_encode_forward writes them; no input Jacobian.  Same values as two calls. */
int s3d_grid_encode_forward_pair(const float* inputs, const void* embeddings_a, const void* embeddings_b, const int32_t* offsets,
                                 void* outputs_a, void* outputs_b, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                 uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype, float bound,
                                 const int32_t* n_valid, const float* live, uint32_t live_stride, s3d_stream_t stream);

/* Test hook: table row of every corner, corner_idx [B,L,2^D] u32 (0xffffffff for out-of-range points). */
int s3d_grid_corner_indices(const float* inputs, const int32_t* offsets, uint32_t* corner_idx, uint32_t B,
                            uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                            int align_corners, s3d_stream_t stream);

/* gridencoder.h:13 void grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C,
 *                        L, S, H, dy_dx, grad_inputs, gridtype, align_corners, interp)
 * grad [L,B,C]; grad_embeddings [table_rows,C] zero-initialised by the caller, accumulated into.
 * max_level_rows = max over levels of offsets[l+1]-offsets[l] (the module builds `offsets` on the host,
 * grid.py:104-112, so it knows it; 0 = unknown).
 * workspace (s3d_grid_encode_backward_workspace_size bytes; 0 = configuration not supported) enables the
 * binned path used for B >= 8192: contributions are partitioned by table slice and summed in LDS as 64-bit
 * fixed point — deterministic, no global atomics.  Without it (NULL) direct atomics are used.
 * path: 0 = auto, 1 = direct atomics, 2 = binned (an error when the workspace is missing).
 * found_inf (optional, build extension): a device float raised to 1 when grad_embeddings holds a non-finite value after
 * the call (torch.amp.GradScaler's check, nerf/utils.py:495-537, made where the gradient is produced: the binned fp16 path
 * reports while it writes the sums, the other paths scan the table once).  Never cleared here.
 * control (optional, build extension): s3d_grid_encode_backward_control_size() bytes of device memory (a few hundred KB,
 * independent of B) that the CALLER zero-fills once after allocating it; every call finds it all-zero and leaves it all-zero
 * (the accumulate kernel clears the bucket cursors it has consumed), so the binned path needs no clearing launch of its
 * own.  Not to be shared by calls that may run concurrently.  NULL: the words live in `workspace` and are cleared per call. */
size_t s3d_grid_encode_backward_workspace_size(uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                               uint32_t max_level_rows, int dtype);
size_t s3d_grid_encode_backward_control_size(uint32_t D, uint32_t C, uint32_t L, uint32_t max_level_rows, int dtype);
int s3d_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings,
                             const int32_t* offsets, void* grad_embeddings, uint32_t max_level_rows,
                             uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners,
                             uint32_t interp, int dtype, void* workspace, size_t workspace_bytes,
                             float bound, const int32_t* n_valid, int path, float* found_inf,
                             void* control, size_t control_bytes, s3d_stream_t stream);

/* Build extension: the backward of a table WITH its parameter update (single replica, fp16 C = 2 tables).  The binned path's
 * accumulate kernel holds every row's gradient sum in registers at its write-out; given the optimizer's state it applies
 * torch.optim.Adam's update (betas, eps as passed; the reference: main_SealNeRF.py:283-288) there — fp32 master row, both
 * moments and the fp16 copy the next forward reads — for EVERY row of the table (rows without records take g = 0), and the
 * gradient table is neither written nor read: the separate update's 30 B per parameter become 26 B, overlapped with the
 * records' streaming.  The row's gradient is the exact sum rounded to binary16 (what the unfused path stores), so both routes
 * update to the same bits; where that rounding would overflow the fp32 sum is used.  GradScaler: `found_inf` must hold the
 * step's decision so far when the call is issued (every other gradient producer of the step has run: the table's backward is
 * the last node of the graph); a non-finite dL/dy seen by this call's scatter raises it and skips the update as a whole.
 * step / grad_scale / lr_scale: device floats (step count BEFORE this update; loss scale or NULL; schedule factor or NULL).
 * *applied (host) = 1 when the update was made here; 0 when the call fell back to the plain backward (direct-atomics sizes,
 * more than one level pass, other dtypes): grad_embeddings then holds the gradient and the caller's optimizer applies it. */
typedef struct s3d_grid_adam {
    float* param;
    float* exp_avg;
    float* exp_avg_sq;
    void* param_half; /* fp16 [rows, C] or NULL */
    float lr, beta1, beta2, eps;
    const float* step;
    const float* grad_scale;
    const float* lr_scale;
} s3d_grid_adam;
int s3d_grid_encode_backward_adam(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                  void* grad_embeddings, uint32_t max_level_rows, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                  float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                  void* workspace, size_t workspace_bytes, float bound, const int32_t* n_valid, float* found_inf,
                                  void* control, size_t control_bytes, const s3d_grid_adam* adam, int* applied, s3d_stream_t stream);

/* s3d_grid_encode_backward_adam with a STEP TAIL: small work of the training step that is independent of the table's backward
 * and would otherwise queue behind it as four launches of 4 - 10 us each.  It runs inside the backward's own two binned launches:
 *  (a) S3D_TAIL_WGRAD_REDUCE  s3d_ffmlp_wgrad_reduce_pair's work (its arguments: *_a, *_b; workspace_a = NULL: none) and
 *  (b) S3D_TAIL_LOSS          s3d_loss_terms_reduce's work (loss_workspace = NULL: none) as extra workgroups of the scatter
 *                             launch — both are complete before the accumulate launch starts;
 *  (c) S3D_TAIL_ADAM          s3d_adam_step_multi's work on `tensors` (host array, at most four non-empty ones), with the step /
 *                             grad_scale / lr_scale of `adam`, the call's found_inf and the skip decision of the table's own
 *                             update (found_inf at entry, or-ed with the poison words of every level), and
 *  (d) S3D_TAIL_EPILOGUE      s3d_scaler_update on the call's found_inf (scale = NULL: none), followed by s3d_step_ring_push
 *                             (counter = NULL: none), by the workgroup of the accumulate launch that finishes last.
 * Same arithmetic and order of additions as the separate entry points: every value is bit-identical.  *tail_applied (host)
 * receives the S3D_TAIL_* bits of the parts that ran there.  A call that falls back (*applied = 0) issues (a) and (b) as their
 * ordinary launches in front of the backward and reports no bit; the caller then runs (c) and (d) as it would without a tail.
 * (d) is applied only together with every tensor of (c): it clears found_inf and advances the step count, so the caller hands
 * it in only when no other update of the step is left to launch. */
enum { S3D_TAIL_WGRAD_REDUCE = 1, S3D_TAIL_LOSS = 2, S3D_TAIL_ADAM = 4, S3D_TAIL_EPILOGUE = 8 };
struct s3d_adam_tensor;
typedef struct s3d_step_tail {
    const void* workspace_a; uint32_t B_a, input_dim_a, hidden_dim_a, num_layers_a; uint16_t* grad_weights_a; int accumulate_a; float* found_inf_a;
    const void* workspace_b; uint32_t B_b, input_dim_b, hidden_dim_b, num_layers_b; uint16_t* grad_weights_b; int accumulate_b; float* found_inf_b;
    const float* loss_workspace; /* [3N squared errors | N depth terms] of s3d_composite_rays_train_loss(loss = NULL) */
    uint32_t loss_N;
    int loss_with_depth;
    float loss_depth_weight;
    float* loss;
    const struct s3d_adam_tensor* tensors;
    int32_t n_tensors;
    float* scale;
    int32_t* growth_tracker;
    float growth_factor, backoff_factor;
    int32_t growth_interval;
    float* adam_step;
    const float* ring_loss;
    int32_t* counter;
    float* loss_ring;
    int32_t* counter_ring;
    int32_t* cursor;
    int32_t ring, loss_slots;
} s3d_step_tail;
int s3d_grid_encode_backward_adam_tail(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                       void* grad_embeddings, uint32_t max_level_rows, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                       float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                       void* workspace, size_t workspace_bytes, float bound, const int32_t* n_valid, float* found_inf,
                                       void* control, size_t control_bytes, const s3d_grid_adam* adam, const s3d_step_tail* tail,
                                       int* applied, uint32_t* tail_applied, s3d_stream_t stream);

/* gridencoder.h:15 void grad_total_variation(inputs, embeddings, grad, offsets, weight, B, D, C, L, S, H,
 *                        gridtype, align_corners) — fp32 only (grid.py:162 disables autocast) */
int s3d_grad_total_variation(const float* inputs, const float* embeddings, float* grad,
                             const int32_t* offsets, float weight, uint32_t B, uint32_t D, uint32_t C,
                             uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                             s3d_stream_t stream);

/* ------------------------------------------------------------------ shencoder
 * shencoder/src/shencoder.h:9-10.  fp32 (the wrapper casts inputs to f32, sphere_harmonics.py:16). */
int s3d_sh_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D, uint32_t degree,
                          float* dy_dx /* [B,3,deg^2] or NULL */, s3d_stream_t stream);
int s3d_sh_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D, uint32_t degree,
                           const float* dy_dx, float* grad_inputs, s3d_stream_t stream);

/* ------------------------------------------------------------------ freqencoder
 * freqencoder/src/freqencoder.h:7,10.  C = D + 2*D*deg. */
int s3d_freq_encode_forward(const float* inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                            float* outputs, s3d_stream_t stream);
int s3d_freq_encode_backward(const float* grad, const float* outputs, uint32_t B, uint32_t D, uint32_t deg,
                             uint32_t C, float* grad_inputs, s3d_stream_t stream);
/* Build extension — two frequency encodings side by side in one fp16 row: out[b] = [freq(a[b]) (D1 + 2 D1 deg1 columns) |
 * freq(d[b]) (D2 + 2 D2 deg2) | zeros up to ld] — TensoRF's colour MLP input cat([encoder(feat), encoder_dir(d)]) as the fp16
 * autocast Linear sees it (tensoRF/network.py:48-51, 160-166): s3d_freq_encode_forward's fp32 values of float(a) and d, rounded
 * to binary16 once.  a: fp16 [B, D1], d: fp32 [B, D2], out: fp16 [B, ld], ld even.  _backward: the gradient w.r.t. a from the
 * row's fp16 gradient (s3d_freq_encode_backward's expression, sin / cos re-computed), fp16 [B, ldg] with the columns behind D1
 * zero (ldg = 32: the row layout s3d_vm_color_backward reads); d takes no gradient (view directions). */
int s3d_freq_encode_pack_forward(const uint16_t* a, const float* d, uint32_t B, uint32_t D1, uint32_t deg1, uint32_t D2,
                                 uint32_t deg2, uint32_t ld, uint16_t* out, const int32_t* n_valid, s3d_stream_t stream);
int s3d_freq_encode_pack_backward(const uint16_t* grad, const uint16_t* a, uint32_t B, uint32_t D1, uint32_t deg1, uint32_t ld,
                                  uint32_t ldg, uint16_t* grad_a, const int32_t* n_valid, s3d_stream_t stream);

/* ------------------------------------------------------------------ ffmlp
 * ffmlp/src/ffmlp.h:8-14.  All tensors fp16 (uint16_t bit patterns).
 * weights: [W,in] | (n-1) x [W,W] | [out,W], row-major [out,in] per layer (ffmlp.cu:631-634).
 * forward_buffer / backward_buffer: [n, B, W] post-activation / pre-activation-gradient scratch.
 * B must be a multiple of 128 (ffmlp.py:156-159 pads); in % 16 == 0; out == 16; W in {16,32,64,128,256} (ffmlp.cu:40-44).
 * W in {32,64} with in <= 64 (every network of the BASELINE configs) run on the register-resident MFMA kernels and have all
 * the extensions below; the other shapes take a layer-by-layer path (hand-written MFMA kernels k_layer / k_wgrad_tile / k_wgrad_finish, fp16
 * storage / fp32 accumulation, csrc/ffmlp_generic.hip; the library links no BLAS) that implements the reference's interface only: forward_buffer / backward_buffer
 * are then REQUIRED for training (plain row-major [n, B, W]) and inference_buffer must hold [2, B, W].
 * input_layout: 0 = inputs [B,in] row-major (the reference); 1 = level-major [in/2][B][2], i.e. the grid
 * encoder's own output layout read in place (and grad_inputs written in it) — no permute copies in between.
 * rgb_head (optional, build extension): fp32 [B, 3] = sigmoid(output[:, 0:3]) written INSTEAD of `outputs` (which may then
 * be NULL) — the colour network's `torch.sigmoid(h)` (nerf/network_ff.py:103) folded into the last layer's store, with the
 * fp16 roundings of the op sequence.  s3d_ffmlp_backward then takes grad_rgb (fp32 [B, 3], gradient w.r.t. that output)
 * and rgb_head instead of `grad`.
 * mid_* (optional, build extension; mid_color_in != NULL switches it on): the density network's head of
 * nerf/network_ff.py:55-96 folded into the last layer — mid_sigma [B] f32 = trunc_exp(output[:, 0]), mid_color_in [B, 32] f16
 * = [half(SH_4(mid_dirs)) | output[:, 1:16] | 0] (the colour network's input), mid_h0 [B] f16 = output[:, 0]; `outputs` may
 * then be NULL.  s3d_ffmlp_backward takes mid_grad_sigma [B] f32 (may be NULL), mid_grad_color_in [B, 32] f16 and mid_h0
 * instead of `grad`.  Same arithmetic and roundings as s3d_ngp_mid_forward / _backward. */
int s3d_ffmlp_forward(const uint16_t* inputs, const uint16_t* weights, uint32_t B, uint32_t input_dim,
                      uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                      uint32_t output_activation, uint16_t* forward_buffer, uint16_t* outputs,
                      int input_layout, const int32_t* n_valid, float* rgb_head, const float* mid_dirs,
                      float* mid_sigma, uint16_t* mid_color_in, uint16_t* mid_h0, s3d_stream_t stream);
/* ffmlp.h:9: same network without storing intermediates (inference_buffer: unused by the MFMA kernels, [2, B, W] ping-pong
 * scratch for the layer-by-layer shapes) */
int s3d_ffmlp_inference(const uint16_t* inputs, const uint16_t* weights, uint32_t B, uint32_t input_dim,
                        uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                        uint32_t output_activation, uint16_t* inference_buffer, uint16_t* outputs,
                        int input_layout, const int32_t* n_valid, float* rgb_head, const float* mid_dirs,
                      float* mid_sigma, uint16_t* mid_color_in, uint16_t* mid_h0, s3d_stream_t stream);
/* Build extension for the inference loop (nerf/renderer.py:341-367 calls density and colour network back to back on the same
 * rows; nerf/network_ff.py:55-105): both fused MLPs and the two heads in ONE launch — inputs [B, 32] fp16 (or level-major
 * [16][B][2]), dirs [B, 3] fp32 -> sigma [B] fp32 = trunc_exp(h[:, 0]), rgb [B, 3] fp32 = sigmoid(colour(...)[:, :3]);
 * color_in (optional) [B, 32] fp16 receives the colour-net input rows and h0 (optional) [B] fp16 the pre-activation of
 * sigma — what the two networks' backward calls need (s3d_ffmlp_backward: colour head on color_in, density head on h0), so a
 * training forward takes the same launch.  Same arithmetic and rounding points as s3d_ffmlp_inference(density head) +
 * s3d_ffmlp_inference(colour head).  hidden_dim 64, ReLU, 16-column outputs.  enc_color (optional) fp16 level-major [16][B][2]:
 * the network Seal-3D trains (nerf/network.py:99-128) — the colour network then takes the 64-wide row of s3d_ngp_mid2_forward,
 * [half(SH_4(d)) | h1..h15 | enc_color | 0], built on chip (weights_color [64*64 | ...], color_in [B, 64]). */
int s3d_ffmlp_ngp_pair_inference(const uint16_t* inputs, const uint16_t* weights_sigma, const uint16_t* weights_color,
                                 uint32_t B, uint32_t hidden_dim, uint32_t num_layers_sigma, uint32_t num_layers_color,
                                 int input_layout, const int32_t* n_valid, const float* dirs, float* sigma, float* rgb,
                                 uint16_t* color_in, uint16_t* h0, const uint16_t* enc_color, s3d_stream_t stream);
/* ffmlp.h:11; grad_weights fp16 [same layout as weights]: every element is written (accumulate_grad_weights = 0,
 * the reference zero-fills it first, ffmlp.py:72) or added to (accumulate_grad_weights = 1).
 * workspace: fp32 accumulation of the weight gradient (s3d_ffmlp_backward_workspace_size).
 * forward_buffer == backward_buffer == NULL selects the fused backward: the activations are re-computed from
 * `inputs` inside one kernel that also forms the data and weight gradients, so a training forward may skip
 * forward_buffer altogether (call s3d_ffmlp_forward with forward_buffer = NULL).  Shapes it covers:
 * s3d_ffmlp_fused_backward_supported() != 0 (hidden 32/64, <= 3 hidden matrices, no sine).
 * found_inf (optional, build extension): device float raised to 1 when a written grad_weights element is non-finite
 * (GradScaler's check made by the kernel that writes the gradient).  Never cleared here. */
int s3d_ffmlp_fused_backward_supported(uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim,
                                       uint32_t num_layers, uint32_t activation);
size_t s3d_ffmlp_backward_workspace_size(uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim,
                                         uint32_t num_layers);
int s3d_ffmlp_backward(const uint16_t* grad, const uint16_t* inputs, const uint16_t* weights,
                       const uint16_t* forward_buffer, uint32_t B, uint32_t input_dim, uint32_t output_dim,
                       uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                       uint32_t output_activation, int calc_grad_inputs, uint16_t* backward_buffer,
                       uint16_t* grad_inputs, uint16_t* grad_weights, void* workspace,
                       size_t workspace_bytes, int input_layout, int accumulate_grad_weights,
                       const int32_t* n_valid, float* found_inf, const float* grad_rgb, const float* rgb_head,
                       const float* mid_grad_sigma, const uint16_t* mid_grad_color_in, const uint16_t* mid_h0,
                       s3d_stream_t stream);
/* Build extension: s3d_ffmlp_backward with accumulate_grad_weights = 2 (fused backward only) leaves the per-workgroup partial
 * sums of the weight gradient in `workspace` and skips its reduce launch; this call finishes TWO such networks (the colour and
 * the density network of one step, each with its own workspace) in one launch: grad_weights_x fp16 written (accumulate_x = 0)
 * or added to (1), found_inf_x raised like s3d_ffmlp_backward's.  B_x etc.: the arguments of the backward call it finishes. */
int s3d_ffmlp_wgrad_reduce_pair(const void* workspace_a, uint32_t B_a, uint32_t input_dim_a, uint32_t hidden_dim_a,
                                uint32_t num_layers_a, uint16_t* grad_weights_a, int accumulate_a, float* found_inf_a,
                                const void* workspace_b, uint32_t B_b, uint32_t input_dim_b, uint32_t hidden_dim_b,
                                uint32_t num_layers_b, uint16_t* grad_weights_b, int accumulate_b, float* found_inf_b,
                                s3d_stream_t stream);
/* ffmlp.h:13-14: the reference allocates split-K side streams here; this build fuses the weight
 * gradient into the backward launch sequence on the caller's stream, so these are no-ops kept for
 * surface compatibility. */
int s3d_ffmlp_allocate_splitk(size_t n);
int s3d_ffmlp_free_splitk(void);

/* ------------------------------------------------------------------ TensoRF vector-matrix features
 * tensoRF/network.py:112-153 get_sigma_feat / get_color_feat (12 F.grid_sample calls, bilinear, zeros padding,
 * align_corners=True, + stack / cat / mul / sum) in one pass, csrc/tensorf.hip.
 * x [N,3] fp32 in [-1,1] (normalised like network.py:160); planes / lines / rank / resolution: HOST arrays of 3:
 * planes[i] device fp32 [rank[i], res[m1], res[m0]] with (m0,m1) = mat_ids[i] = (0,1),(0,2),(1,2); lines[i] device fp32
 * [rank[i], res[vec_ids[i]]], vec_ids = 2,1,0 (network.py:37-38, :105-106).
 * reduce = 1: out [N] = sum_i sum_r plane*line (sigma_feat); reduce = 0: out [rank0+rank1+rank2, N] = the products
 * (the tensor the reference transposes into basis_mat, network.py:147). */
int s3d_vm_features_forward(const float* x, uint32_t N, const float* const* planes, const float* const* lines,
                            const uint32_t* rank, const uint32_t* resolution, int reduce, float* out,
                            const float* const* planes_t, const float* const* lines_t, const int32_t* n_valid,
                            s3d_stream_t stream);
/* Parameter gradients of the same op (what autograd derives from the grid_sample calls: F.grid_sample's backward
 * scatter-adds every corner with a global atomic).  Binned instead: s3d_vm_backward_keys writes keys [6,N] i32 (rows 0-2
 * the 8x8-cell plane tile of component i, rows 3-5 its 64-row line chunk; 0x7fffffff = contributes nothing); the caller
 * sorts each row, passes perm [6,N] i32 (point ids in key order) and start [6,n_bounds] i32 (first sorted position with
 * key >= t, n_bounds > s3d_vm_backward_max_bins(resolution) + 1), a scratch gm [N, sum rank] (no initialisation needed) and
 * zero-initialised gradient buffers shaped like the factors.  grad: [N] (reduce = 1) or [N, sum rank] (reduce = 0: the
 * gradient of the products, point-major — the memory layout autograd hands back through the reference's `.T`).
 * bound_words: four zero-initialised device words per call — the kernels sum a tile's contributions in LDS as 64-bit fixed
 * point (integer LDS atomics retire ~10x faster than float ones on MI355X) and keep the bounds that fix its scale there
 * (max |grad|, max |line parameter|, max |g m|, max column sum of |basis|); a non-finite bound poisons the gradients.
 * line_scratch: sum_i rank_i * resolution[vec_ids[i]] floats, no initialisation: the bound pass leaves the line factors there
 * transposed ([Dn][rank]) for the plane pass, whose lanes are rank channels.
 * found_inf (optional device float): set to 1 when a bound is not finite — the condition under which these kernels write a
 * non-finite gradient — so a GradScaler need not read the 69 MB of factor gradients again to find out.
 * planes_t / lines_t (optional, round 6): rank-fastest shadows of the factors — planes_t[i] [H][W][rank_i], lines_t[i] [Dn][rank_i],
 * 16-byte aligned, written by s3d_vm_transpose_factors from the current parameters (the caller refreshes them when the parameters
 * change).  With them a corner's rank channels are one contiguous run instead of rank_i words H * W * 4 bytes apart: the forwards
 * (ranks that are multiples of four) read four ranks per 16-byte load, the plane passes of the backward load a tile's window as 81
 * runs.  Same values, same arithmetic, same results bit for bit; NULL: the parameters' own layout.
 * n_valid (optional, round 6; every s3d_vm_* entry point that walks the points, and s3d_freq_encode_pack_*): the device-side
 * sample count of a padded batch — rows [round_up(*n_valid, 128), N) are absent: the forwards do not write them, the binning
 * sorts them behind every bin (the backward passes then never see them) and the bound pass does not look at their gradients.
 * stage / stage_bytes (optional, round 6): s3d_vm_backward_stage_bytes(N, rank, resolution) bytes of 16-byte aligned device
 * scratch, no initialisation.  With it the cells several workgroups add to (the border of a whole tile's 9x9 window, a line
 * chunk's 65 cells) leave as plain stores into per-tile / per-workgroup rows and one extra launch adds the rows in a FIXED
 * order; NULL (or too small): those cells take global atomics, as before.  Same sums within fp32 summation order. */
size_t s3d_vm_backward_stage_bytes(uint32_t N, const uint32_t* rank, const uint32_t* resolution);
int s3d_vm_transpose_factors(const float* const* planes, const float* const* lines, const uint32_t* rank, const uint32_t* resolution,
                             float* const* planes_t, float* const* lines_t, s3d_stream_t stream);
uint32_t s3d_vm_backward_max_bins(const uint32_t* resolution);
int s3d_vm_backward_keys(const float* x, uint32_t N, const uint32_t* rank, const uint32_t* resolution, int32_t* keys,
                         s3d_stream_t stream);
/* The whole binning in one call: perm [6,N] i32 and start [6,n_bounds] i32 (n_bounds >= max_bins + 2) as described above, by a
 * counting sort (keys + wave-aggregated bin counts, scan, scatter); the order of the points inside a bin is unspecified (the
 * backward kernels sum a bin exactly, in fixed point).  workspace: s3d_vm_backward_bins_workspace_size(N, n_bounds) bytes. */
size_t s3d_vm_backward_bins_workspace_size(uint32_t N, uint32_t n_bounds);
int s3d_vm_backward_bins(const float* x, uint32_t N, const uint32_t* rank, const uint32_t* resolution, int32_t* perm,
                         int32_t* start, uint32_t n_bounds, void* workspace, size_t workspace_bytes, const int32_t* n_valid,
                         s3d_stream_t stream);
int s3d_vm_features_backward(const float* x, uint32_t N, const float* const* planes, const float* const* lines,
                             const uint32_t* rank, const uint32_t* resolution, int reduce, const float* grad,
                             const int32_t* perm, const int32_t* start, uint32_t n_bounds, float* gm,
                             float* const* grad_planes, float* const* grad_lines, uint32_t* bound_words, float* line_scratch,
                             void* stage, size_t stage_bytes, float* found_inf, const float* const* planes_t, const int32_t* n_valid,
                             s3d_stream_t stream);

/* The colour features with basis_mat applied inside the kernel (tensoRF/network.py:149-153: `basis_mat((mat * vec).T)`, an
 * nn.Linear(sum rank, basis_rows, bias=False) that runs under fp16 autocast): out [N, basis_rows] fp16 =
 * half(sum_row half(basis[c][row]) * half(product[row][n])) with fp32 accumulation; the [sum rank, N] products are never
 * written.  basis: fp16 [basis_rows, sum rank] (the Linear's weight), basis_rows <= 32.
 * s3d_vm_color_backward: from grad_out fp16 [N, 32] (the gradient of that output, rows zero-padded to 32 columns = 64 bytes,
 * 16-byte aligned) the factor gradients as
 * s3d_vm_features_backward writes them (same perm / start / gm / zero-initialised buffers) and grad_basis fp32
 * [basis_rows, sum rank] (zero-initialised; accumulated with atomics). */
int s3d_vm_color_forward(const float* x, uint32_t N, const float* const* planes, const float* const* lines,
                         const uint32_t* rank, const uint32_t* resolution, const uint16_t* basis, uint32_t basis_rows,
                         uint16_t* out, const float* const* planes_t, const float* const* lines_t, const int32_t* n_valid,
                         s3d_stream_t stream);
int s3d_vm_color_backward(const float* x, uint32_t N, const float* const* planes, const float* const* lines,
                          const uint32_t* rank, const uint32_t* resolution, const uint16_t* basis, uint32_t basis_rows,
                          const uint16_t* grad_out, const int32_t* perm, const int32_t* start, uint32_t n_bounds,
                          float* gm, float* const* grad_planes, float* const* grad_lines, float* grad_basis,
                          uint32_t* bound_words, float* line_scratch, void* stage, size_t stage_bytes, float* found_inf,
                          const float* const* planes_t, const int32_t* n_valid, s3d_stream_t stream);

/* ------------------------------------------------------------------ TensoRF CP features (line factors only)
 * tensoRF/network_cp.py:78-111 get_sigma_feat / get_color_feat (3 F.grid_sample calls on "fake 2-D" [1,R,D,1] tensors, two
 * products of [R,N] tensors, a sum or basis_mat) in one pass, csrc/tensorf_cp.hip.
 * x [N,3] fp32 in [-1,1]; lines / rank / resolution: HOST arrays of 3: lines[i] device fp32 [rank, res[vec_ids[i]]],
 * vec_ids = 2,1,0 (network_cp.py:35).  The three ranks must be equal (the product runs over ONE rank index; anything else is
 * refused).  Per line: p = ((u + 1) / 2) * (D - 1), i0 = floor(p), value = v[i0] * ((i0 + 1) - p) + v[i0 + 1] * (p - i0), a
 * tap outside [0, D - 1] counts as zero; f[r][n] = (l0 * l1) * l2.
 * reduce = 1: out [N] = sum_r f[r][n] (sigma_feat); reduce = 0: out [rank, N] (the tensor the reference transposes into
 * basis_mat).  Any N >= 1.
 * lines_t (optional): rank-fastest shadows lines_t[i] [D_i][rank] written by s3d_cp_transpose_lines from the current parameters;
 * a tap's channels are then one contiguous run (four per 16-byte load when rank % 4 == 0 and the shadows are 16-byte aligned).
 * Same values, same arithmetic; NULL: the parameters' own layout.
 * n_valid (optional): as for the s3d_vm_* entry points — rows [round_up(*n_valid, 128), N) are absent: the forwards do not write
 * them, the backwards do not read them (the binning sorts them behind every bin). */
int s3d_cp_transpose_lines(const float* const* lines, const uint32_t* rank, const uint32_t* resolution, float* const* lines_t,
                           s3d_stream_t stream);
int s3d_cp_features_forward(const float* x, uint32_t N, const float* const* lines, const uint32_t* rank,
                            const uint32_t* resolution, int reduce, float* out, const float* const* lines_t,
                            const int32_t* n_valid, s3d_stream_t stream);
/* The products with basis_mat applied inside the kernel (network_cp.py:109), the fp16-autocast Linear's arithmetic exactly as
 * s3d_vm_color_forward defines it: out [N, basis_rows] fp16 = half(sum_r half(basis[c][r]) * half(f[r][n])), fp32 accumulation.
 * basis: fp16 [basis_rows <= 32, rank], rank <= 512 (the weight sits in LDS). */
int s3d_cp_color_forward(const float* x, uint32_t N, const float* const* lines, const uint32_t* rank,
                         const uint32_t* resolution, const uint16_t* basis, uint32_t basis_rows, uint16_t* out,
                         const float* const* lines_t, const int32_t* n_valid, s3d_stream_t stream);
/* Parameter gradients: grad_lines[i] fp32 [rank, D_i], ZERO-INITIALISED by the caller (the kernels add).  grad: [N]
 * (reduce = 1) or [N, rank] point-major (reduce = 0).  perm / start / n_bounds: the result of s3d_vm_backward_bins for the same
 * x, resolution and n_valid (its rows 3-5, the 64-row line chunks, are read; no further workspace).  A workgroup sums up to
 * 1,024 sorted points of one chunk and one 32-rank slice in LDS in fp32 and adds each of its 65 cells to grad_lines with one
 * atomic; the order of those few adds is the only thing that varies between runs.  Non-finite gradients travel through the
 * sums; one that belongs to a point outside every line's range (which reaches no cell) makes grad_lines[0][0] NaN and raises
 * found_inf (optional device float, set to 1).  The coordinates' gradient is not computed.
 * s3d_cp_color_backward: from grad_out fp16 [N, 32] (rows zero-padded to 32 columns, 16-byte aligned) the line gradients and
 * grad_basis fp32 [basis_rows, rank] (zero-initialised; one atomic per entry and workgroup). */
int s3d_cp_features_backward(const float* x, uint32_t N, const float* const* lines, const uint32_t* rank,
                             const uint32_t* resolution, int reduce, const float* grad, const int32_t* perm,
                             const int32_t* start, uint32_t n_bounds, float* const* grad_lines, float* found_inf,
                             const float* const* lines_t, const int32_t* n_valid, s3d_stream_t stream);
int s3d_cp_color_backward(const float* x, uint32_t N, const float* const* lines, const uint32_t* rank,
                          const uint32_t* resolution, const uint16_t* basis, uint32_t basis_rows, const uint16_t* grad_out,
                          const int32_t* perm, const int32_t* start, uint32_t n_bounds, float* const* grad_lines,
                          float* grad_basis, float* found_inf, const float* const* lines_t, const int32_t* n_valid,
                          s3d_stream_t stream);

/* ------------------------------------------------------------------ CCNeRF features (rank-residual TensoRF)
 * tensoRF/network_cc.py:128-250 compute_features_density / compute_features and the SH contraction of :287-291, in one pass per
 * call, csrc/tensorf_cc.hip.  The components are cut into n_groups <= 8 groups; a group holds a vector component (three lines,
 * one rank index: l0[r] * l1[r] * l2[r]) and / or a matrix component (three planes, one rank index: p0[r] * p1[r] * p2[r]) and
 * one matrix S per component.  groups: HOST array of n_groups records; an absent component is NULL / rank 0:
 *   line[i]  device fp32 [rank_vec, res[vec_ids[i]]], vec_ids = 2,1,0;
 *   plane[i] device fp32 [rank_mat, res[m1], res[m0]], (m0, m1) = mat_ids[i] = (0,1), (0,2), (1,2): x[m0] runs along the last axis;
 *   s_vec / s_mat device fp32 [rows, rank]: rows = 1 (features) or 3 * degree^2 (colour).
 * Level k is the sum over the groups g <= k of S_vec_g (l0 l1 l2) + S_mat_g (p0 p1 p2).  residual = 1: every level is returned
 * (K_out = n_groups); residual = 0: the last one only (K_out = 1).
 *   s3d_cc_features_forward: out fp32 [K_out, N].
 *   s3d_cc_color_forward:    out fp32 [K_out, N, 3] = sum_j level[ch * degree^2 + j] * SH_j(dirs[n]) — the logits in front of the
 *                            sigmoid; degree 1 .. 4, dirs [N,3] fp32.  The [K, N, 3 degree^2] tensor is never written.
 * Arithmetic contract.  Sampling is grid_sample's bilinear, zeros padding, align_corners = FALSE: per axis of D cells
 * p = ((u + 1) * D - 1) / 2 in fp32, i0 = floor(p), weights (i0 + 1) - p and p - i0, a tap outside [0, D - 1] counts as zero (a
 * point up to one cell outside [-1, 1] still reads a value); plane taps in the order nw, ne, sw, se with weight wx * wy; the
 * products are (a * b) * c in fp32.  half = 0: everything is fp32; a level is (vec + mat) + previous level.  half = 1 (the fp16
 * autocast sequence): every S @ f is the autocast Linear's arithmetic as s3d_vm_color_forward defines it,
 * half(sum_r half(S[c][r]) * half(f[r])) with fp32 accumulation; the level sums are fp16 adds in the reference's order (vec, then
 * mat, then the previous level); the SH contraction and everything behind it is fp32.
 * Limits (anything else is refused): n_groups <= 8, (rank_vec + rank_mat) * rows <= 7168 per group (the group's S sits in LDS),
 * rank * extent < 2^31 per factor.
 * n_valid (optional): as for the s3d_vm_* entry points — rows [round_up(*n_valid, 128), N) are neither written nor read.
 *
 * Backward (parameter gradients only; the coordinates' and directions' gradients are not computed).  grad: fp32 [K_out, N] /
 * [K_out, N, 3].  The level gradients are folded into per-group gradients by a suffix sum over the levels in registers (group g
 * receives every level >= g).  grads: HOST array of n_groups records of device fp32 buffers shaped like the factors and the S
 * matrices, ZERO-INITIALISED by the caller (the kernels add).  half = 1: the gradient that reaches S @ f and the operands of
 * both products are rounded to binary16, sums are fp32.  Factor gradients leave by global fp32 atomics: adjacent points of a
 * wave that fall into the same cell (consecutive samples of a ray) are summed first and leave by one atomic per tap and rank, any
 * other point by its own; the S gradients are summed over the 128 points of a workgroup in LDS and leave by one atomic per entry
 * and workgroup.  The order of the adds is the only thing that varies between runs.
 * A non-finite gradient of any live point — inside or outside the factors — raises found_inf (optional device float, set to 1)
 * and makes the first S gradient's first entry NaN; inside the factors it also travels through the sums. */
typedef struct s3d_cc_group {
    const float* line[3];
    const float* plane[3];
    const float* s_vec;
    const float* s_mat;
    uint32_t rank_vec, rank_mat;
} s3d_cc_group;
typedef struct s3d_cc_group_grad {
    float* line[3];
    float* plane[3];
    float* s_vec;
    float* s_mat;
} s3d_cc_group_grad;
int s3d_cc_features_forward(const float* x, uint32_t N, const s3d_cc_group* groups, uint32_t n_groups, const uint32_t* resolution,
                            int residual, int half, float* out, const int32_t* n_valid, s3d_stream_t stream);
int s3d_cc_color_forward(const float* x, const float* dirs, uint32_t N, const s3d_cc_group* groups, uint32_t n_groups,
                         const uint32_t* resolution, uint32_t degree, int residual, int half, float* out, const int32_t* n_valid,
                         s3d_stream_t stream);
int s3d_cc_features_backward(const float* x, uint32_t N, const s3d_cc_group* groups, uint32_t n_groups, const uint32_t* resolution,
                             int residual, int half, const float* grad, const s3d_cc_group_grad* grads, float* found_inf,
                             const int32_t* n_valid, s3d_stream_t stream);
int s3d_cc_color_backward(const float* x, const float* dirs, uint32_t N, const s3d_cc_group* groups, uint32_t n_groups,
                          const uint32_t* resolution, uint32_t degree, int residual, int half, const float* grad,
                          const s3d_cc_group_grad* grads, float* found_inf, const int32_t* n_valid, s3d_stream_t stream);

/* Build extensions for the TensoRF step (chains of tiny launches otherwise):
 * s3d_aabb_normalize: out[n][a] = 2 (x[n][a] - aabb[a]) / (aabb[3 + a] - aabb[a]) - 1 (tensoRF/network.py:155-157, the reference's
 *   operation order; aabb = 6 DEVICE floats);
 * s3d_weighted_abs_sum: *out = sum_i weights[i] * sum |tensors[i]| over up to 8 fp32 tensors (host arrays of device pointers /
 *   element counts / weights) — density_loss() of tensoRF/network.py:259-263 with weights 1 / numel; workspace:
 *   s3d_weighted_abs_sum_workspace_size() bytes of scratch; fixed summation order. */
int s3d_aabb_normalize(const float* x, const float* aabb, uint32_t N, float* out, s3d_stream_t stream);
size_t s3d_weighted_abs_sum_workspace_size(void);
int s3d_weighted_abs_sum(const float* const* tensors, const uint64_t* numel, const float* weights, int32_t count, float* out,
                         float* workspace, s3d_stream_t stream);

/* s3d_pack_linear_chain: the fp32 [rows_i, cols_i] weights of a bias-free nn.Linear chain into the flat fp16 vector s3d_ffmlp_*
 * take ([W, in_pad] | (n - 1) x [W, W] | [16, W]: matrix i at its running offset, row stride ld[i] >= cols[i], padded_rows[i] >=
 * rows[i] rows, padding zero) in one launch; s3d_unpack_linear_chain: the flat fp16 gradient back into fp32 matrices of the
 * parameters' shapes.  Host arrays of `count` <= 8 entries. */
int s3d_pack_linear_chain(const float* const* mats, const uint32_t* rows, const uint32_t* cols, const uint32_t* padded_rows,
                          const uint32_t* ld, int32_t count, uint16_t* flat, s3d_stream_t stream);
int s3d_unpack_linear_chain(const uint16_t* flat, float* const* mats, const uint32_t* rows, const uint32_t* cols,
                            const uint32_t* padded_rows, const uint32_t* ld, int32_t count, s3d_stream_t stream);

/* ------------------------------------------------------------------ NGP head glue
 * The elementwise steps between the two MLPs of nerf/network_ff.py:55-96 (slice / trunc_exp / SH / cat / cast /
 * sigmoid and their backward nodes) as two streaming kernels per direction, csrc/ngp_head.hip.
 * h, color_in, out and their gradients are fp16 row-major ([B,16], [B,32], [B,16]); sigma, rgb, dirs fp32. */
int s3d_ngp_mid_forward(const uint16_t* h, const float* dirs, uint32_t B, float* sigma, uint16_t* color_in,
                        const int32_t* n_valid, s3d_stream_t stream);
int s3d_ngp_mid_backward(const uint16_t* grad_color_in, const float* grad_sigma /* or NULL */, const uint16_t* h,
                         uint32_t B, uint16_t* grad_h, const int32_t* n_valid, s3d_stream_t stream);
/* Two-encoder network (nerf/network.py:99-128 — the net Seal-3D trains): colour-net input [B,64] =
 * [half(SH_4(d)) | h1..h15 | encoder_color(x) (32) | 0]; enc_color and grad_enc_color (may be NULL) are level-major
 * [16][B][2] fp16, the grid kernels' own layout. */
int s3d_ngp_mid2_forward(const uint16_t* h, const float* dirs, const uint16_t* enc_color, uint32_t B, float* sigma,
                         uint16_t* color_in, const int32_t* n_valid, s3d_stream_t stream);
/* Build extension — s3d_composite_rays_train_loss with a PER-RAY background: bg [N,3] (device, fp32) replaces the 3 host floats,
 * and grad_bg [N,3] = d loss / d bg = (d loss / d pixel) * (1 - weights_sum) is written as well — the input of
 * s3d_background_backward (nerf/renderer.py:316 with `bg_color = self.background(sph, rays_d)`, :159-161).  Same launches, same
 * expressions as the constant form.  grad_bg NULL: a background that needs no gradient (the random background of RGBA
 * frames, s3d_rgba_targets); that one store is skipped. */
int s3d_composite_rays_train_loss_bg(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                     uint32_t M, uint32_t N, float T_thresh, const float* gt, const float* bg,
                                     const float* grad_loss, const float* gt_depth, float depth_weight,
                                     float* weights_sum, float* depth, float* image, float* grad_sigmas, float* grad_rgbs,
                                     float* grad_image, float* grad_weights_sum, float* grad_bg, float* loss, float* workspace,
                                     s3d_stream_t stream);

int s3d_ngp_mid2_backward(const uint16_t* grad_color_in, const float* grad_sigma /* or NULL */, const uint16_t* h,
                          uint32_t h_stride /* 16: h is the density network's [B, 16] output; 1: its first column [B] alone */,
                          uint32_t B, uint16_t* grad_h, uint16_t* grad_enc_color /* or NULL */, const int32_t* n_valid,
                          s3d_stream_t stream);
int s3d_ngp_rgb_forward(const uint16_t* out, uint32_t B, float* rgb, const int32_t* n_valid, s3d_stream_t stream);
int s3d_ngp_rgb_backward(const float* grad_rgb, const float* rgb, uint32_t B, uint16_t* grad_out,
                         const int32_t* n_valid, s3d_stream_t stream);
/* Loss head of one ray batch: loss = mean((image + (1 - weights_sum) * bg - gt)^2)  (nerf/renderer.py:316 background
 * compositing + nerf/utils.py:484 MSE); bg_rgb = 3 HOST floats; loss / grad_loss are single device floats.
 * s3d_bg_mse_forward with grad_loss != NULL also writes what s3d_bg_mse_backward would for that upstream gradient (under
 * loss scaling the loss's upstream gradient is the scale, known before the backward pass): one launch instead of two.
 * depth / gt_depth [N] (optional, both or neither) add Seal-3D's depth term depth_weight * mean(|nan_to_num(depth) - gt_depth|)
 * (nerf/utils.py:486-489) to the VALUE of the loss; like the reference's composite backward (raymarching.py:274: "grad_depth is
 * not used now") it contributes no gradient. */
int s3d_bg_mse_forward(const float* image, const float* weights_sum, const float* gt, const float* bg_rgb, uint32_t N,
                       float* loss, const float* grad_loss, float* grad_image, float* grad_weights_sum,
                       const float* depth, const float* gt_depth, float depth_weight, s3d_stream_t stream);
int s3d_bg_mse_backward(const float* image, const float* weights_sum, const float* gt, const float* bg_rgb, uint32_t N,
                        const float* grad_loss, float* grad_image, float* grad_weights_sum, s3d_stream_t stream);
/* Build extension — targets of a teacher-rendered ray batch (SealNeRF/trainer.py:506-586 `proxy_truth`): out_rgb [N,3] =
 * nan_to_num(image + (1 - weights_sum) * bg) (nerf/renderer.py:316), out_depth [N] (optional) = nan_to_num(depth), nan -> 0 and
 * +-inf -> +-FLT_MAX as torch.nan_to_num(nan=0.); bg_rgb = 3 HOST floats. */
int s3d_bg_targets(const float* image, const float* weights_sum, const float* depth, const float* bg_rgb, uint32_t N,
                   float* out_rgb, float* out_depth, s3d_stream_t stream);
/* Build extension — s3d_bg_targets with a per-ray background bg [N,3] (device, fp32): the teacher's background model. */
int s3d_bg_targets_rays(const float* image, const float* weights_sum, const float* depth, const float* bg, uint32_t N,
                        float* out_rgb, float* out_depth, s3d_stream_t stream);
/* Build extension — the NGP background model, nerf/network.py:149-163 `background(x, d)` of the reference (modules built at
 * :74-96): rgb [N,3] = sigmoid(W1 relu(W0 [SH_4(dirs) | grid(sph)])), grid = `encoder_bg`, a 4-level 2D hash grid with 2
 * features per level (GridEncoder.forward with bound = 1), W0 [64,24] and W1 [3,64] fp32 (the parameters; rounded to fp16 as they are read).  One launch: grid lookup (the
 * expressions of s3d_grid_encode_forward, D = 2: the features are bit for bit its outputs), SH degree 4, both layers (fp32
 * accumulation, fp16 rounding of each layer's output), sigmoid in fp32 rounded to fp16 (rgb holds fp16 values in fp32).
 * sph [N,2] in [-1,1] (s3d_sph_from_ray), dirs [N,3]; table [offsets[4], 2] of `dtype`; offsets [5] (device); S = log2 of the
 * per-level scale, H = base resolution; features [4,N,2] of `dtype` (optional): the grid features, level-major. */
int s3d_background_forward(const float* sph, const float* dirs, const void* table, const int32_t* offsets, uint32_t N,
                           float S, uint32_t H, int dtype, const float* w0, const float* w1, float* rgb, void* features,
                           s3d_stream_t stream);
/* Backward of s3d_background_forward from grad_rgb [N,3] (fp32) and the forward's rgb: the hidden layer is recomputed, the feature
 * gradient (fp16-rounded, like the reference's autocast backward) is ADDED into grad_table [table_rows, 2] of `dtype` (NULL: a
 * frozen table, no scatter) with the
 * grid backward's direct atomics, grad_w0 [64,24] / grad_w1 [3,64] (fp32) are overwritten.  Two launches: the per-ray pass filing
 * per-wave weight-gradient partials in `workspace` (s3d_background_backward_workspace_size(N) bytes), and their sum in wave order
 * (deterministic).  found_inf (optional): set to 1 when a weight gradient or an entry of grad_table is not finite. */
size_t s3d_background_backward_workspace_size(uint32_t N);
int s3d_background_backward(const float* grad_rgb, const float* rgb, const float* sph, const float* dirs, const void* table,
                            const int32_t* offsets, uint32_t table_rows, uint32_t N, float S, uint32_t H, int dtype,
                            const float* w0, const float* w1, void* grad_table, float* grad_w0, float* grad_w1,
                            float* found_inf, void* workspace, size_t workspace_bytes, s3d_stream_t stream);
/* Build extension — the TensoRF background model, tensoRF/network.py:201-218 `background(x, d)` of the reference (parameters
 * built at :69-96): rgb [N,3] = sigmoid(W1 relu(W0 [freq_2(dirs) | grid_sample(bg_mat, sph)])).  plane = `bg_mat` [R,H,W] fp32
 * with R = 8, H, W >= 2 (sph[:,0] runs along W, sph[:,1] along H), sampled as F.grid_sample does (bilinear, zeros padding,
 * align_corners=True; a coordinate outside [-1,1] or not finite contributes no corner); freq_2 = the 15 columns of
 * s3d_freq_encode_forward (D = 3, degree 2); W0 [64,23], W1 [3,64] fp32, rounded to fp16 as they are read.  One launch, the
 * arithmetic of s3d_background_forward's MLP.  features [N,R] fp32 (optional): the plane samples, bit for bit F.grid_sample's. */
int s3d_vm_background_forward(const float* sph, const float* dirs, const float* plane, uint32_t R, uint32_t H, uint32_t W,
                              const float* w0, const float* w1, uint32_t N, float* rgb, float* features, s3d_stream_t stream);
/* Backward of s3d_vm_background_forward from grad_rgb [N,3] (fp32) and the forward's rgb: the hidden layer is recomputed, the
 * sample gradient (fp16-rounded) times each in-range corner's weight is ADDED into grad_plane [R,H,W] fp32 with one atomic per
 * corner and rank (NULL: a frozen plane, no scatter), grad_w0 [64,23] / grad_w1 [3,64] (fp32) are overwritten.  Two launches, as
 * s3d_background_backward: per-wave partials in `workspace` (s3d_vm_background_backward_workspace_size(N) bytes), summed in wave
 * order.  found_inf (optional): set to 1 when a weight gradient or an entry of grad_plane is not finite. */
size_t s3d_vm_background_backward_workspace_size(uint32_t N);
int s3d_vm_background_backward(const float* grad_rgb, const float* rgb, const float* sph, const float* dirs, const float* plane,
                               uint32_t R, uint32_t H, uint32_t W, const float* w0, const float* w1, uint32_t N,
                               float* grad_plane, float* grad_w0, float* grad_w1, float* found_inf, void* workspace,
                               size_t workspace_bytes, s3d_stream_t stream);
/* Build extension — Seal-3D's local-pretraining loss on one point chunk (SealNeRF/trainer.py:455-469: L1Loss(sigma) +
 * L1Loss(colour), means): loss = sum|sigma - gt_sigma| / n_total + sum|color - gt_color| / (3 n_total); n_total >= n is the
 * size of the whole chunk when the call sees one rank's shard of it; sigma / color (and the gradients) hold n_rows >= n rows,
 * rows [n, n_rows) being padding of the prediction (no term, zero gradient; the targets hold n rows).  grad_loss != NULL (a device float, the loss scale):
 * grad_sigma [n] and grad_color [n,3] = sign(.) * *grad_loss / n_total resp. / (3 n_total) are written by the same launch.
 * workspace: s3d_l1_pair_workspace_size() bytes, zero-filled ONCE by the caller (the kernel leaves its ticket word zero);
 * the value is summed in a fixed order (reproducible). */
size_t s3d_l1_pair_workspace_size(void);
int s3d_l1_pair_loss(const float* sigma, const float* color, const float* gt_sigma, const float* gt_color, uint32_t n,
                     uint32_t n_rows, uint32_t n_total, float* loss, const float* grad_loss, float* grad_sigma, float* grad_color,
                     void* workspace, s3d_stream_t stream);

/* ------------------------------------------------------------------ Seal proxy mapper (bbox tool)
 * SealNeRF/seal_utils.py:132-153 (map_mask), :237-279 (map_to_origin), :630-685 (two-ray Moller-Trumbore inside test)
 * in one pass over the sample points.  points/dirs/out_* are DEVICE [M,3] f32, mask DEVICE [M] u8; everything that
 * describes the edit is HOST data (a handful of constants): triangles [n_tris,3,3], bounds [n_bounds,2,3] (min,max),
 * inv_transform [4,4] row-major, inv_rotation [3,3], inv_scale [3], center [3]; empty_bound [2,3] + map_source [3] or
 * both NULL.  out_dirs/dirs may both be NULL. */
int s3d_seal_bbox_map(const float* points, const float* dirs, uint32_t M, const float* triangles, uint32_t n_tris,
                      const float* bounds, uint32_t n_bounds, const float* inv_transform, const float* inv_rotation,
                      const float* inv_scale, const float* center, const float* empty_bound, const float* map_source,
                      float* out_points, float* out_dirs, uint8_t* mask, const int32_t* n_valid /* padded sample batch: rows past it are skipped, or NULL */,
                      s3d_stream_t stream);

/* Colour edit of the bbox tool applied to the samples the proxy moved — `rgbs[mask] = map_color(.., rgbs[mask])` of
 * SealNeRF/renderer.py:316, 396-399 with seal_utils.py:48-58 (map_color), :739-769 (modify_hsv, modify_rgb) and
 * color_utils.py:33-66 (rgb2hsv_torch / hsv2rgb_torch).  rgbs / out DEVICE [M,3] f32 or f16 (`dtype`; out may alias rgbs),
 * mask DEVICE [M] u8 (s3d_seal_bbox_map's).  hsv: HOST [3] offsets added to (h, s, v), or NULL.  rgb_target: HOST [3] target
 * colour or NULL — every moved sample takes the target's hue and saturation and the value
 * clamp(target_v + (v_i - mean_moved(v)) + light_offset, 0, 1); the mean is taken over the moved rows of THIS call (a batch
 * statistic, as in the reference) in `stats`, DEVICE 16 bytes (order-independent fixed-point sum + count; cleared by the call).
 * With both, hsv is applied first and its RGB result converted again (the reference's two steps).  Rows where mask == 0 are
 * copied. */
int s3d_seal_map_color(const void* rgbs, const uint8_t* mask, uint32_t M, int dtype, const float* hsv, const float* rgb_target,
                       float light_offset, void* out, void* stats, const int32_t* n_valid /* or NULL */, s3d_stream_t stream);

/* Texture painting of the brush tool (`imageConfig`) on the samples the proxy moved — the `image` step of map_color,
 * SealNeRF/seal_utils.py:58-79 with :753-769 (modify_rgb with a per-sample target), after the optional hsv step.  rgbs / out
 * DEVICE [M,3] f32 or f16 (`dtype`; out may alias rgbs), points DEVICE [M,3] f32 (the MAPPED sample points), mask DEVICE [M] u8.
 * hsv: HOST [3] or NULL.  texture: DEVICE [tex_h, tex_w, 4] f32, 16-byte aligned, one texel = (hue, saturation, value, alpha)
 * of the image (rgb2hsv_torch of its RGB, done once by the caller).  quad: HOST [14] = v_image_o[3], v_image_w - v_image_o [3],
 * v_image_h - v_image_o [3], v_image_norm[3], |ow|^2, |oh|^2.  A moved sample's point is projected onto the plane (o, norm);
 * its texel is (clamp(floor(v_op . oh / |oh|^2 * tex_h), 0, tex_h - 1), clamp(floor(v_op . ow / |ow|^2 * tex_w), 0, tex_w - 1)):
 * nearest texel, the edge texel outside the quad.  The sample takes the texel's hue and saturation and the value
 * clamp(texel_v + (v_i - mean_moved(v)) + light_offset, 0, 1), blended over its colour by the texel's alpha; the mean is taken
 * over the moved rows of THIS call in `stats` (DEVICE 16 bytes, cleared by the call), as in s3d_seal_map_color.  texel_out:
 * DEVICE [M,2] i32 or NULL, receives (idx_h, idx_w) of the moved rows.  Rows where mask == 0 are copied. */
int s3d_seal_map_color_image(const void* rgbs, const float* points, const uint8_t* mask, uint32_t M, int dtype, const float* hsv,
                             const float* texture, uint32_t tex_h, uint32_t tex_w, const float* quad, float light_offset, void* out,
                             void* stats, int32_t* texel_out, const int32_t* n_valid /* or NULL */, s3d_stream_t stream);

/* Seal proxy mapper, brush tool — SealNeRF/seal_utils.py:282-453 (map_to_origin :408-453) with :132-153 (map_mask) and
 * :630-685 (inside test, ray direction = the UNnormalised normal_expand).  points / out_points DEVICE [M,3] f32, mask DEVICE
 * [M] u8.  triangles DEVICE [n_tris,3,3] (12 per stroke), bounds DEVICE [n_bounds,2,3] (min,max; one per stroke), border
 * DEVICE [n_border,3] (projected border points of all strokes; may be NULL when linear == 0).  normal_expand, center: HOST [3]
 * (of the last stroke).  linear != 0: masked p -> (p - n) + (|att - d| / att) n where att > d, d = distance of p's projection
 * on the plane (center, n) to the nearest border point; linear == 0 (`dry`): p unchanged.  Unmasked rows are copied; the
 * view directions are not touched (the reference returns them unchanged). */
int s3d_seal_brush_map(const float* points, uint32_t M, const float* triangles, uint32_t n_tris, const float* bounds,
                       uint32_t n_bounds, const float* border, uint32_t n_border, const float* normal_expand, const float* center,
                       float attenuation_distance, int linear, float* out_points, uint8_t* mask,
                       const int32_t* n_valid /* or NULL */, s3d_stream_t stream);

/* Seal proxy mapper, anchor tool — SealNeRF/seal_utils.py:456-570 (map_to_origin :514-570).  points / out_points DEVICE
 * [M,3] f32, mask DEVICE [M] u8, triangles DEVICE [n_tris,3,3]; bounds HOST [2,3]; params HOST [14] = v_anchor[3],
 * v_offset[3], v_h[3], len_h, radius, scale[3].  As in the reference the decision is batch-wide: if no row passes the map
 * mask (AABB, all coordinates != 0, inside test along the fixed axis) every row is copied with mask 0; otherwise EVERY row
 * goes through the cone / plane-side map and mask = cone AND side.  flag: DEVICE 4 bytes of scratch that carries that
 * decision between the call's kernels (cleared by the call), so no host synchronisation is needed. */
int s3d_seal_anchor_map(const float* points, uint32_t M, const float* triangles, uint32_t n_tris, const float* bounds,
                        const float* params, float* out_points, uint8_t* mask, void* flag,
                        const int32_t* n_valid /* or NULL */, s3d_stream_t stream);

/* ------------------------------------------------------------------ parameter update
 * The reference's update is torch.optim.Adam(betas=(0.9, 0.99), eps=1e-15) under torch.cuda.amp.GradScaler
 * (nerf/utils.py:356-361, 495-537; main_SealNeRF.py:283-288).  These three calls are that update taken directly
 * from the gradient the backward kernels produced (fp16 for the hash tables), see csrc/optim.hip.
 * found_inf / grad_scale / step are single device floats (GradScaler's found_inf and scale, Adam's step count).
 * s3d_grads_nonfinite sets *found_inf = 1 if any element is inf/NaN (never clears it).
 * s3d_adam_step updates param / exp_avg / exp_avg_sq (fp32) with grad / *grad_scale as step number *step + 1, and
 * does nothing when *found_inf != 0; param_half (optional) receives the fp16 copy of the updated parameters.
 * s3d_adam_advance increments *step unless *found_inf != 0 (call once per optimizer step, after the tensors).
 * lr_scale (optional, device): the update uses lr * *lr_scale — the factor of a learning-rate schedule
 * (torch.optim.lr_scheduler.LambdaLR in main_SealNeRF.py:283-288), read at run time so that a step captured in a HIP graph
 * follows the schedule without being re-captured. */
int s3d_grads_nonfinite(const void* grad, size_t n, int dtype, float* found_inf, s3d_stream_t stream);
int s3d_adam_step(float* param, const void* grad, int grad_dtype, float* exp_avg, float* exp_avg_sq,
                  uint16_t* param_half, size_t n, float lr, float beta1, float beta2, float eps,
                  const float* step, const float* grad_scale, const float* found_inf, const float* lr_scale,
                  s3d_stream_t stream);
int s3d_adam_advance(float* step, const float* found_inf, s3d_stream_t stream);
/* s3d_adam_step for every tensor of the optimizer in one launch (same arithmetic per element).  consume_grads != 0: every
 * gradient is cleared behind the read — also on a skipped (*found_inf != 0) step — for producers that accumulate into it. */
typedef struct s3d_adam_tensor {
    float* param;
    void* grad; /* written only with consume_grads */
    float* exp_avg;
    float* exp_avg_sq;
    uint16_t* param_half; /* optional fp16 copy of the updated parameters */
    size_t n;
    float lr, beta1, beta2, eps;
    int grad_dtype; /* S3D_F32 or S3D_F16 */
    int consume;    /* != 0: this tensor's gradient is cleared behind the read (as consume_grads, per tensor) */
    /* pack_stride != 0: `grad` and `param_half` are views into a PACKED weight buffer — element (r, c) of the [n / pack_cols,
     * pack_cols] parameter lives at r * pack_stride + c (the nn.Linear weights of nerf/network.py inside the fused MLP
     * kernels' padded [out, in] layout); param / exp_avg / exp_avg_sq stay contiguous.  0: contiguous (the reference case). */
    uint32_t pack_cols, pack_stride;
    /* Build extension: != 0 adds the gradient of the penalty l1 * sum|param| to the (unscaled) gradient inside the update,
     * l1 * sign(param) with sign(0) = 0 — TensoRF's L1 term on the density factors (tensoRF/network.py:259-263, tensoRF/utils.py:
     * 42-49: l1 = l1_reg_weight / numel) without the sign / scale / accumulate passes over the factors. */
    float l1;
} s3d_adam_tensor;
int s3d_adam_step_multi(const s3d_adam_tensor* tensors /* host array */, int32_t n_tensors, const float* step,
                        const float* grad_scale, const float* found_inf, const float* lr_scale, int consume_grads,
                        s3d_stream_t stream);
/* GradScaler.update(): scale *= backoff on overflow, *= growth after growth_interval clean steps; clears *found_inf.
 * adam_step (optional): s3d_adam_advance of that step count folded into the same launch (before the flag is cleared). */
int s3d_scaler_update(float* scale, int32_t* growth_tracker, float* found_inf, float growth_factor,
                      float backoff_factor, int32_t growth_interval, float* adam_step, s3d_stream_t stream);
/* Build extension (graph-replayed step): the renderer keeps the marcher's {samples, rays} counters of the last 16 training
 * steps (nerf/renderer.py:106, 352-356: `step_counter[local_step % 16]`).  Device-side equivalent of that bookkeeping:
 * slot = cursor[0]; loss_ring[slot] = *loss (both optional); counter_ring[slot] = counter[0..1]; counter[0..1] = 0;
 * cursor[0] = (slot + 1) % ring; cursor[1] += 1 (running step number, the `noise_step` of s3d_near_far_from_aabb).
 * loss_slots > 0: loss_ring has loss_slots entries of its own and the loss is filed at cursor[1] % loss_slots (before the
 * increment) — a longer history than the counter ring, so that a loss handed out as a view stays valid for loss_slots steps. */
int s3d_step_ring_push(const float* loss, int32_t* counter, float* loss_ring, int32_t* counter_ring, int32_t* cursor,
                       int32_t ring, int32_t loss_slots, s3d_stream_t stream);
/* s3d_scaler_update followed by s3d_step_ring_push, one launch. */
int s3d_step_epilogue(float* scale, int32_t* growth_tracker, float* found_inf, float growth_factor, float backoff_factor,
                      int32_t growth_interval, float* adam_step, const float* loss, int32_t* counter, float* loss_ring,
                      int32_t* counter_ring, int32_t* cursor, int32_t ring, int32_t loss_slots, s3d_stream_t stream);

/* ------------------------------------------------------------------ parameter EMA (csrc/ema.hip)
 * The reference's trainers keep torch_ema's ExponentialMovingAverage of the parameters (nerf/utils.py:733,882; main_nerf.py:147
 * `ema_decay=0.95`).  tensors: HOST array of {param, shadow, n}: fp32, contiguous, DEVICE, 4-byte aligned (a view that starts
 * inside an allocation is fine), n == 0 allowed; any number of tensors (one streaming launch per 64 non-empty ones).
 * s3d_ema_update_multi: per element, three fp32 roundings and no contraction (bit-identical to torch_ema's tmp = s - p;
 * tmp.mul_(c); s.sub_(tmp)):  t = s - p;  t = t * c;  s = s - t,  with c = (float)(1.0 - d) and, in double,
 * d = min(decay, (1 + n) / (10 + n)) where n = *num_updates + 1 (use_num_updates != 0), or d = decay (use_num_updates == 0).
 * num_updates: DEVICE int64, read by the update and advanced by exactly one by a one-thread launch behind it (also with no
 * tensors at all); may be NULL when use_num_updates == 0 (nothing is counted then).  No host read: legal under stream capture,
 * and a replay uses the count of its own time.  decay must lie in [0, 1].
 * s3d_ema_exchange_multi: param[i] <-> shadow[i] for every element, in place; two calls are the identity. */
typedef struct s3d_ema_tensor {
    float* param; /* read by the update, written by the exchange */
    float* shadow;
    size_t n;
} s3d_ema_tensor;
int s3d_ema_update_multi(const s3d_ema_tensor* tensors /* host array */, int32_t n_tensors, double decay, int use_num_updates,
                         int64_t* num_updates, s3d_stream_t stream);
int s3d_ema_exchange_multi(const s3d_ema_tensor* tensors /* host array */, int32_t n_tensors, s3d_stream_t stream);

/* ------------------------------------------------------------------ training-ray sampling (build extension)
 * nerf/utils.py:92-114 `get_rays(..., N, error_map)` on the device, for one training batch in one launch.  index [B] (device
 * int64): the image of each batch row.  error_map [n_img, 128*128] (fp32, 16-byte aligned): weighted draw of N <= 16,384 cells
 * per row without replacement (an exponential race: key w / -log(u), the N largest keys; winners in ascending cell order, at the
 * threshold key the lower cell wins; when fewer than N cells are positive the rest are zero-weight cells by index, where
 * torch.multinomial raises), each jittered to a pixel with (cell * s + u * s).long().clamp(max = H|W - 1), s = H|W / 128.
 * error_map NULL: the reference's uniform randint pixels, shared by the rows.  poses [n_img,4,4]; intrinsics: 4 HOST floats
 * fx, fy, cx, cy.  Outputs [B,N,*]: rays_o, rays_d (get_rays' expression), inds (int64), inds_coarse (int64, with a map), and
 * (optional) gt [B,N,3] fp32 gathered from images [n_img,H,W,3] (images_dtype fp32 / fp16) and gt_depth [B,N] from depths
 * [n_img,H*W].  Randomness: a counter hash of (seed, ctl[0], image, cell); ctl [2] int32 on the device = {step, 0}: the last
 * workgroup advances ctl[0], so a captured launch draws fresh cells on every replay.  Test entry: u_keys [B,16384] in (0, 1]
 * and u_fine [B,N,2] in [0, 1) (both, with a map) replace the hash and leave ctl alone.  out_index [B] (optional) receives a
 * copy of index: the static index buffer a captured step's s3d_error_map_update reads. */
int s3d_sample_train_rays(const float* error_map, const int64_t* index, uint32_t B, uint32_t N, uint32_t n_img, uint32_t H,
                          uint32_t W, const float* poses, const float* intrinsics, const void* images, int images_dtype,
                          const float* depths, uint32_t seed, int32_t* ctl, const float* u_keys, const float* u_fine,
                          float* rays_o, float* rays_d, float* gt, float* gt_depth, int64_t* inds, int64_t* inds_coarse,
                          int64_t* out_index, s3d_stream_t stream);
/* s3d_sample_train_rays for RGBA frames, images [n_img,H,W,4]: the same draw (inds, inds_coarse and rays are those of
 * s3d_sample_train_rays on the same arguments), and each winner's pixel is blended onto its background as s3d_rgba_targets
 * does for row = b * N + n, in the same launch: gt [B,N,3] the blended target, bg [B,N,3] (optional) the background.  u_bg
 * [B,N,3] in [0, 1) (test entry) replaces the background's hash; ctl is left alone only when every random number of the
 * launch is explicit (u_keys, u_fine and — with random_bg — u_bg). */
int s3d_sample_train_rays_rgba(const float* error_map, const int64_t* index, uint32_t B, uint32_t N, uint32_t n_img, uint32_t H,
                               uint32_t W, const float* poses, const float* intrinsics, const void* images, int images_dtype,
                               const float* depths, uint32_t seed, int32_t* ctl, const float* u_keys, const float* u_fine,
                               int random_bg, const float* u_bg, float* rays_o, float* rays_d, float* gt, float* bg,
                               float* gt_depth, int64_t* inds, int64_t* inds_coarse, int64_t* out_index, s3d_stream_t stream);
/* Training targets of RGBA rows (nerf/utils.py:465-474; :549-554 with random_bg 0): images [R,4] fp32 / fp16 (aligned to one
 * pixel; fp16 is widened to fp32 first) -> bg [R,3] and gt [R,3] = fl(fl(rgb * a) + fl(bg * fl(1 - a))), fp32, no contraction:
 * with the same bg, bit for bit torch's expression on fp32 frames.  random_bg 0: bg = 1 (the bg pointer may be NULL).
 * random_bg 1: bg[row, c] = (float)(hash_u32(bg_key, ctl[0], 3 * row + c) >> 8) * 2^-24 — 24 bits in [0, 1) — with
 * bg_key = pcg_hash(seed ^ 0x3C6EF372), pcg_hash(v): v = v * 747796405 + 2891336453; w = ((v >> ((v >> 28) + 4)) ^ v) *
 * 277803737; (w >> 22) ^ w, and hash_u32(key, step, n) = pcg_hash(pcg_hash(key ^ (step * 0x9E3779B9)) + n), all in uint32.
 * ctl [2] int32 on the device = {step, 0}: the last workgroup advances ctl[0], so a captured launch draws a fresh
 * background on every replay.  Test entry: u_bg [R,3] in [0, 1) replaces the hash and leaves ctl alone. */
int s3d_rgba_targets(const void* images, int images_dtype, uint32_t R, int random_bg, uint32_t seed, int32_t* ctl,
                     const float* u_bg, float* gt, float* bg, s3d_stream_t stream);
/* Build extension — the error-map EMA of nerf/utils.py:506-528 after a step's loss: for ray r = (b, n) of the batch,
 * err = mean_c((image + (1 - weights_sum) * bg - gt)^2) (+ depth_weight * mean_r |nan_to_num(depth) - gt_depth|, reduced in a
 * fixed order inside the launch), then error_map[index[b], inds_coarse[r]] = 0.1 old + 0.9 err.  bg: 3 HOST floats bg_rgb or a
 * per-ray bg_rays [B*N,3] (device); weights_sum NULL (and no bg): image is the composited prediction.  Rows of `index` must be
 * distinct and every row of inds_coarse free of duplicates (as the sampler returns them): the scatter is race-free.  A
 * non-finite err leaves the old value in place (where the reference writes it and multinomial later raises). */
int s3d_error_map_update(float* error_map, uint32_t n_img, const int64_t* index, const int64_t* inds_coarse, uint32_t B, uint32_t N,
                         const float* image, const float* weights_sum, const float* gt, const float* bg_rgb, const float* bg_rays,
                         const float* depth, const float* gt_depth, float depth_weight, s3d_stream_t stream);
/* Build extension — Seal-3D's custom-pose batches (SealNeRF/provider.py:145-178): B orbit cameras looking at look_at from
 * distance radius, and every ray of each camera's rH x rW frame, in one launch.  Pose b, nerf/provider.py:57-91 `rand_poses`
 * in its expression order (fp32, no contraction): theta = u_t * fl(theta1 - theta0) + theta0, phi likewise; offset = radius *
 * (sin theta sin phi, cos theta, sin theta cos phi); forward = -offset / (|offset| + 1e-10); right = normalize(forward x
 * (0, -1, 0)); up = normalize(right x forward); poses_out [B,4,4] (optional) = columns right, up, forward, offset + look_at.
 * rays_o, rays_d [B, rH*rW, 3] (16-byte aligned), pixels in row-major order: get_rays(pose, intrinsics, rH, rW, -1), formed by
 * the code s3d_sample_train_rays forms a winner's ray with.  intrinsics: 4 HOST floats fx, fy, cx, cy of the rH x rW frame;
 * look_at: 3 HOST floats or NULL (the origin).  Randomness: u_t = (float)(hash_u32(pcg_hash(seed ^ 0x1B873593), ctl[0], b) >> 8)
 * * 2^-24, u_p the same with 0xCC9E2D51 (hash_u32, pcg_hash: s3d_rgba_targets); ctl [2] int32 on the device = {step, 0}: the
 * last workgroup advances ctl[0], so a captured launch draws fresh poses on every replay.  Test entry: u_pose [B,2] in [0, 1)
 * replaces the hash and leaves ctl alone.  B = 0 or an empty frame: nothing is launched. */
int s3d_orbit_rays(uint32_t B, uint32_t rH, uint32_t rW, const float* intrinsics, const float* look_at, float radius,
                   double theta0, double theta1, double phi0, double phi1, uint32_t seed, int32_t* ctl, const float* u_pose,
                   float* poses_out, float* rays_o, float* rays_d, s3d_stream_t stream);
/* Build extension — interactive preview (nerf/utils.py:754-820 `test_gui`, SealNeRF/gui.py `NeRFGUI.prepare_buffer`,
 * `test_step`, `get_mask_pos`); DESIGN.md §5 "Interactive preview".
 * s3d_frame_rays: rays_o, rays_d [rH*rW, 3] (16-byte aligned) of the ONE camera `pose` (16 HOST floats, a row-major 4 x 4
 * cam2world matrix; they travel in the launch's argument block) = get_rays(pose, intrinsics, rH, rW, -1), pixels in row-major
 * order, formed by the code s3d_sample_train_rays forms a winner's ray with.  intrinsics: 4 HOST floats fx, fy, cx, cy of the
 * rH x rW frame.  An empty frame: nothing is launched. */
int s3d_frame_rays(const float* pose, const float* intrinsics, uint32_t rH, uint32_t rW, float* rays_o, float* rays_d,
                   s3d_stream_t stream);
/* s3d_preview_resolve: everything between the renderer's output image [rH,rW,3], depth [rH,rW] (fp32) and the displayed
 * frame, one pass over the H x W destination (rH <= H, rW <= W).  Destination pixel (y, x) reads source pixel
 * (min((int)floorf(y * fl((float)rH / H)), rH - 1), the same for x): F.interpolate(mode='nearest').  frame_depth [H,W] =
 * nan_to_num(depth) (NaN -> 0, +-inf -> +-FLT_MAX); frame_image [H,W,3] = the colours, through linear_to_srgb (x < 0.0031308 ?
 * 12.92 x : 1.055 x^0.41666 - 0.055) when to_srgb; where that is a plain copy of image (rH == H, rW == W, no conversion)
 * frame_image may be NULL and is then not written.  pos [H,W,3] (optional; needs rays_o, rays_d [H*W,3] and rH == H, rW == W)
 * = rays_o + fl(frame_depth * rays_d).  buffer [H,W,3] (optional), the display buffer, is updated in place with the prepared
 * frame: the colours, or with depth_mode frame_depth / (max(frame_depth) + 1e-6) on all three channels (the maximum over the
 * destination frame: a first launch, into workspace — 4 bytes); where any of the K masks [K,H,W] uint8 is non-zero, fl(color *
 * fl(alpha)) + fl(prepared * fl(1 - alpha)) (color: 3 HOST floats; 1 - alpha formed in double); then with spp > 0 frames in the
 * buffer already, buffer = (fl(buffer * spp) + prepared) / (spp + 1), each operation rounded to fp32; spp == 0 stores.  All of
 * frame_image, frame_depth, pos, buffer 16-byte aligned, masks 4-byte.  Every operation but the power is individually rounded:
 * the results are the torch / numpy sequence's bits. */
int s3d_preview_resolve(const float* image, const float* depth, uint32_t rH, uint32_t rW, uint32_t H, uint32_t W, int to_srgb,
                        const float* rays_o, const float* rays_d, float* frame_image, float* frame_depth, float* pos,
                        float* buffer, int depth_mode, const uint8_t* masks, uint32_t K, const float* color, double alpha,
                        uint32_t spp, uint32_t* workspace, s3d_stream_t stream);
/* Mask positions (get_mask_pos): for each of K masks [K,H,W] uint8 the rows of pos [H*W,3] where the mask is non-zero, in
 * row-major pixel order — numpy's pos[mask > 0] — concatenated over the masks.  s3d_mask_positions_count fills the workspace
 * (s3d_mask_positions_workspace_bytes; 0 for invalid sizes) and writes offsets [K+1] int64 on the device: rows before mask k,
 * offsets[K] the total.  s3d_mask_positions_emit, given the same masks and workspace, writes out [rows,3] with rows =
 * offsets[K].  No atomics: the order is fixed.  K * H * W < 2^32. */
size_t s3d_mask_positions_workspace_bytes(uint32_t K, uint32_t H, uint32_t W);
int s3d_mask_positions_count(const uint8_t* masks, uint32_t K, uint32_t H, uint32_t W, void* workspace, int64_t* offsets,
                             s3d_stream_t stream);
int s3d_mask_positions_emit(const uint8_t* masks, uint32_t K, uint32_t H, uint32_t W, const void* workspace, const float* pos,
                            float* out, uint32_t rows, s3d_stream_t stream);

/* Build extension — mesh export: marching cubes over a dense fp32 volume u [nx,ny,nz] (C order, z fastest); DESIGN.md §8.
 * A grid point is solid iff u > iso, with NaN read as 0 and +-inf as +-FLT_MAX (u is not modified).  Point p owns its +x, +y,
 * +z edges; a crossing edge (exactly one solid end) gives one welded vertex at lo + t along its axis, t = (iso - f_lo) /
 * (f_hi - f_lo) in fp32 (kept inside [0, 1]), lo the owning point.  Vertices are ordered by the owner's linear index
 * (x ny + y) nz + z, then x-, y-, z-edge; world = v / (n_axis - 1) * (max - min) + min per axis.  Triangles are ordered by cell
 * linear index over the (nx-1)(ny-1)(nz-1) cells and by the generated case table (csrc/mc_tables.h) inside a cell, normals from
 * solid to non-solid.  Any axis < 2 or nx ny nz >= 2^31: error (s3d_mc_workspace_bytes: 0), nothing is launched.
 * s3d_mc_workspace_bytes (host): bytes of `workspace` (16-byte aligned), at most 16 per grid point.
 * s3d_mc_count: classify + count + device-wide exclusive scan into `workspace`; totals [2] uint32 on the device = {V, T}
 * (both 0xFFFFFFFF when a count does not fit).
 * s3d_mc_emit: vertices [V,3] fp32, triangles [T,3] int32 from the same u / iso and the workspace s3d_mc_count filled; bounds
 * [6] fp32 on the device = {min xyz, max xyz}.  It reads the counted totals back (one stream synchronisation) and returns an
 * error, launching nothing, unless V and T equal them; the kernel never writes at or past row V / T. */
size_t s3d_mc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int s3d_mc_count(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void* workspace, uint32_t* totals,
                 s3d_stream_t stream);
int s3d_mc_emit(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float iso, const void* workspace, const float* bounds,
                float* vertices, uint32_t V, int32_t* triangles, uint32_t T, s3d_stream_t stream);

/* ------------------------------------------------------------------ D-NeRF glue (csrc/dnerf.hip; DESIGN.md "D-NeRF")
 * The deformation backbone (dnerf/network.py:123-165 of the reference): deform = MLP_5x128([freq_10(x) | freq_6(t)])[:, :3],
 * x' = x + deform, h = MLP_2x64([grid(x') | freq_10(x) | freq_6(t)]).  Two fp16 rows per sample, padded to what s3d_ffmlp_* take:
 *   din [B, 80]  : columns 0..62 freq_10(x) in s3d_freq_encode_forward's column order, 63..75 freq_6(t), 76..79 zero
 *   sin [B, 112] : columns 0..2L-1 the grid features (level l in 2l, 2l+1), 32..94 freq_10(x), 95..107 freq_6(t), 108..111 zero
 * n_valid: the padded-batch convention above (rows at or behind round_up(*n_valid, 128) are neither read nor written).
 *
 * s3d_dnerf_encode_forward: din and columns 32..111 of sin from one launch.  x fp32 [B,3] (raw: the frequency encoder ignores
 * `bound`); t a device pointer read at t[b * t_stride], t_stride 0 (one time for all rows) or 1.  Values: the fp32 values of
 * s3d_freq_encode_forward rounded to binary16 once (the contract of s3d_freq_encode_pack_forward), i.e. bit for bit half() of that
 * kernel's output.  Columns 0..31 of sin are not touched.  No backward: neither x (marcher output) nor t takes a gradient.
 *
 * s3d_dnerf_warp_grid_forward, one launch: xw [B,3] fp32 = x + float(dout[:, 0:3]) (dout: the deformation network's fp16 [B,16]
 * output; one fp32 add), deform [B,3] fp32 = float(dout[:, 0:3]) (optional), the hash / tiled grid encoding (D = 3, C = 2, L <= 16;
 * every table dtype, gridtype, align_corners and interpolation s3d_grid_encode_forward takes) of xw written as fp16 into columns
 * 0..2L-1 of sin (an fp32 table's sums are rounded to binary16 once, an fp16 table's are stored as they are), dy_dx [B,L,3,2] in
 * the table's dtype (optional, the layout s3d_grid_encode_backward reads).  Corner rows, weights and sums are
 * s3d_grid_encode_forward's expressions: features and dy_dx equal that call's on xw bit for bit.  bound as there (> 0: raw
 * coordinates, normalised in the kernel; here WITH dy_dx, which stays the Jacobian w.r.t. the normalised coordinate).
 * reg_sum (optional): one fp32 device word = sum of |deform| over the live rows (all B without n_valid, else the rows the
 * convention above keeps: *n_valid rounded up to 128) and the three columns, summed in a fixed order (lanes by a shuffle tree,
 * waves and workgroups in index order through `workspace`, s3d_dnerf_warp_grid_workspace_size(B) bytes, 16-byte aligned) without
 * float atomics: two runs give the same bits.
 * DIVERGENCE from the reference's regulariser (dnerf/utils.py:117-119 averages |deform| over every row the marcher returned,
 * the zero-padded rows of a budgeted buffer at x = 0 included): only the live rows enter; equal whenever the marcher trims its
 * buffers, which it does to the same multiple of 128.
 *
 * s3d_dnerf_split_grad: columns 0..2L-1 of the density network's input gradient (fp16 [B,112]) as the level-major [L][B][2]
 * tensor in the table's dtype that s3d_grid_encode_backward takes as `grad` (an exact transposition; fp16 -> fp32 is exact).
 *
 * s3d_dnerf_warp_backward: grad_dout fp16 [B,16], columns 0..2 = half(fmaf(coef, sign(deform), float(grad_xw) * grad_scale)),
 * columns 3..15 zero.  grad_xw [B,3] in `dtype`: s3d_grid_encode_backward's grad_inputs; grad_scale: 1 / (2 bound) when the
 * lookup normalised in the kernel (a power of two: exact), else 1.  coef: device float, the upstream gradient of reg_sum (NULL:
 * no regulariser); sign(0) = 0 as torch's abs backward gives. */
int s3d_dnerf_encode_forward(const float* x, const float* t, uint32_t t_stride, uint32_t B, uint16_t* din, uint16_t* sin,
                             const int32_t* n_valid, s3d_stream_t stream);
size_t s3d_dnerf_warp_grid_workspace_size(uint32_t B);
int s3d_dnerf_warp_grid_forward(const float* x, const uint16_t* dout, const void* embeddings, const int32_t* offsets,
                                uint32_t B, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                uint32_t interp, int dtype, float bound, uint16_t* sin, float* xw, float* deform, void* dy_dx,
                                float* reg_sum, void* workspace, size_t workspace_bytes, const int32_t* n_valid,
                                s3d_stream_t stream);
int s3d_dnerf_split_grad(const uint16_t* grad_sin, uint32_t B, uint32_t L, int dtype, void* grad_levels,
                         const int32_t* n_valid, s3d_stream_t stream);
int s3d_dnerf_warp_backward(const void* grad_xw, int dtype, float grad_scale, const float* deform, const float* coef,
                            uint32_t B, uint16_t* grad_dout, const int32_t* n_valid, s3d_stream_t stream);

/* ------------------------------------------------------------------ D-NeRF, temporal basis: the density head
 * (csrc/dnerf_basis.hip; DESIGN.md "D-NeRF, temporal basis")
 * dnerf/network_basis.py:139-152 of the reference: sigma = trunc_exp(h[:, :32] @ sigma_basis), colour-net input =
 * cat[SH_4(d), h[:, 32:]].  h fp16 [B,64]: the density network's output; sigma_basis fp16 [32] (one call has one time); dirs fp32
 * [B,3].  One lane per row; h, sigma_basis, color_in, grad_color_in and grad_h 16-byte aligned.  n_valid: the padded-batch
 * convention above (rows at or behind round_up(*n_valid, 128) are neither read, written nor summed).
 *
 * s3d_dnerf_basis_mid_forward:
 *   acc = fmaf(float(h_k), float(sb_k), acc) for k = 0..31 ascending, acc = 0 at the start (fp32);
 *   pre = float(half(acc))  — the output of the reference's fp16 matrix-vector product;  sigma[b] = expf(pre) (fp32).
 *   color_in [B,48] fp16 (NULL: sigma alone, dirs may then be NULL): columns 0..15 the bits s3d_ngp_mid_forward writes for the
 *   same dirs (half(SH_4(d))), columns 16..47 = h[:, 32:64], copied.
 *
 * s3d_dnerf_basis_mid_backward:
 *   grad_h[:, 32:64] = grad_color_in[:, 16:48], copied;
 *   g = grad_sigma[b] * expf(clamp(pre, -15, 15)) with pre recomputed by the forward's chain (activation.py:13-16), gh = half(g);
 *   grad_h[:, k] = half(float(gh) * float(sb_k)) for k = 0..31 (the product of two halves is exact in fp32: one rounding);
 *   grad_sigma_basis[k] (fp32 [32], may be NULL) = sum over the live rows of float(gh_b) * float(h_bk), in fp32.
 *   grad_sigma == NULL: columns 0..31 of grad_h and grad_sigma_basis are zero.
 *   The sum is deterministic — the same bits on every run for the same B and the same live rows, no floating-point atomics: the
 *   launch has min(512, ceil(B / 256)) workgroups of 256 lanes; a lane adds its rows b, b + 256 G, ... in ascending order, a wave
 *   adds its lanes by a fixed exchange tree, a workgroup its four waves in index order, and the last workgroup to arrive (a ticket) adds
 *   the workgroups' partials of `workspace`: eight stripes (workgroup index mod 8) each in ascending order, then the stripes in
 *   order.  workspace: s3d_dnerf_basis_mid_workspace_size(B) bytes, 16-byte aligned; its first 16 bytes are cleared by the call. */
int s3d_dnerf_basis_mid_forward(const uint16_t* h, const float* dirs, const uint16_t* sigma_basis, uint32_t B, float* sigma,
                                uint16_t* color_in, const int32_t* n_valid, s3d_stream_t stream);
size_t s3d_dnerf_basis_mid_workspace_size(uint32_t B);
int s3d_dnerf_basis_mid_backward(const uint16_t* grad_color_in, const float* grad_sigma, const uint16_t* h,
                                 const uint16_t* sigma_basis, uint32_t B, uint16_t* grad_h, float* grad_sigma_basis,
                                 void* workspace, size_t workspace_bytes, const int32_t* n_valid, s3d_stream_t stream);

/* ------------------------------------------------------------------ D-NeRF, hyper: the 4-D grid lookup
 * (csrc/dnerf_hyper.hip; DESIGN.md "D-NeRF, hyper")
 * dnerf/network_hyper.py:126-140 of the reference: `x = cat([x, ambient.repeat(N, 1)]); x = encoder(x, bound)` with a 4-D tiled /
 * hash grid.  One call has one time, so the fourth coordinate is ONE device word for every row.  C = 2, L <= 16; every table
 * dtype, gridtype, align_corners and interpolation s3d_grid_encode_forward takes.  feat, x4, dy_da, grad_feat and grad_levels
 * 16-byte aligned.  n_valid: the padded-batch convention above (rows at or behind round_up(*n_valid, 128) are neither read,
 * written nor summed).
 *
 * s3d_dnerf_hyper_grid_forward, one launch.  x fp32 [B,3]; ambient: a DEVICE pointer to one fp32 word (no host read).  bound > 0:
 * raw coordinates, normalised in the kernel as s3d_grid_encode_forward does ((v + bound) * fl(1 / (2 bound))), the ambient word
 * as well; bound == 0: coordinates in [0,1].
 *   feat [B, 2L] fp16, row-major: bit for bit the features of s3d_grid_encode_forward with D = 4 on [x | ambient] — an fp16
 *     table's sums stored as they are, an fp32 table's sums (the fmaf chain over the 16 corners) rounded to binary16 ONCE.
 *   x4 (optional) fp32 [B,4] = [x | ambient], as given (raw when bound > 0): the `inputs` of the table backward.
 *   dy_da (optional) [B, L, 2] in the table's dtype: bit for bit that call's dy_dx[:, :, 3, :] (which it produces for
 *     pre-normalised inputs only: on the normalised coordinates as formed here), the ambient column of the Jacobian w.r.t. the
 *     NORMALISED coordinate, from the 16 corner rows the value fetched.  Rounding points as there: an fp32
 *     table adds fmaf(fl(w * diff), pos_deriv, acc) per corner pair; an fp16 table rounds diff to half (one half subtraction),
 *     fl(fl(w * diff) * pos_deriv) to half and adds in half.  pos_deriv of every dimension but 0 is the constant 0 under linear
 *     interpolation (the reference's `pos_deriv[D] = {1.0f}`): dy_da is then zero, and a caller need not ask for it.
 *   A row with any of the four normalised coordinates outside [0,1] gets zero features and zero dy_da.
 *   On a tiled level whose index does not contain the ambient coordinate (the index drops trailing coordinates once its stride
 *   exceeds the level's size) the kernel fetches eight rows and uses each twice: the same bits.
 *
 * s3d_dnerf_hyper_grid_backward, one launch.  grad_feat fp16 [B, 2L].
 *   grad_levels [L][B][2] in `dtype` (the table's): grad_feat transposed, what s3d_grid_encode_backward takes as `grad` (exact;
 *     fp16 -> fp32 is exact).
 *   grad_ambient (fp32, one word; written when dy_da and grad_ambient are both given) = fl(S * grad_scale), S = sum over the live
 *     rows of term_b, term_b = the fp32 chain acc = fmaf(float(g_bk), float(j_bk), acc) over the row's columns k = 0 .. 2L-1
 *     ascending from 0 (g = grad_feat, j = dy_da).  grad_scale: 1 / (2 bound) when the lookup normalised in the kernel (a power of
 *     two for the usual bounds: exact), else 1.
 *     DIVERGENCE from the reference, whose kernel_input_backward rounds each row's dot to the table's dtype before torch sums the
 *     [N, 1] column: the row terms stay fp32 here.
 *   The sum is deterministic — the same bits on every run for the same B and the same live rows, no floating-point atomics: the
 *   launch has G = min(512, ceil(B / 256)) workgroups of 256 lanes; a lane adds the terms of its rows b, b + 256 G, ... in ascending
 *   order, a wave adds its lanes by a fixed exchange tree (offsets 32, 16, .., 1), a workgroup its four waves in index order, and
 *   the last workgroup to arrive (a ticket) adds the workgroups' partials of `workspace`: lane i those of workgroups i, i + 256 in
 *   that order, then the tree and the waves as before.  workspace: s3d_dnerf_hyper_backward_workspace_size(B) bytes, 16-byte
 *   aligned; its first 16 bytes are cleared by the call. */
int s3d_dnerf_hyper_grid_forward(const float* x, const float* ambient, const void* embeddings, const int32_t* offsets,
                                 uint32_t B, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                 uint32_t interp, int dtype, float bound, uint16_t* feat, float* x4, void* dy_da,
                                 const int32_t* n_valid, s3d_stream_t stream);
size_t s3d_dnerf_hyper_backward_workspace_size(uint32_t B);
int s3d_dnerf_hyper_grid_backward(const uint16_t* grad_feat, const void* dy_da, uint32_t B, uint32_t L, int dtype,
                                  float grad_scale, void* grad_levels, float* grad_ambient, void* workspace,
                                  size_t workspace_bytes, const int32_t* n_valid, s3d_stream_t stream);

/* ------------------------------------------------------------------ sampling without the occupancy grid (csrc/hiersample.hip;
 * DESIGN.md "The sampling path without the grid")
 * `NeRFRenderer.run` of the reference (nerf/renderer.py:125-253) and `sample_pdf` (:12-46).  S = num_steps >= 3, U = upsample_steps,
 * K = S + U <= s3d_hier_max_samples() (2,048): above it every entry point returns S3D_ERR_UNSUPPORTED and the caller keeps its own
 * route.  All tensors fp32 and row-major unless noted; rays_o, rays_d [N,3]; aabb[6] device memory; one wave per ray, no workspace.
 * The merged row exists in depth order only as (z_sorted, order); sigma_cat, rgbs, weights, mask and the gradients are in the
 * CONCATENATED order [coarse (S) | fine (U)] in which the networks see the samples: sorted slot p belongs to column order[p].
 * order == NULL is the identity and is accepted only with U == 0.  z, new_z and the points take no gradient (:182 detaches them).
 *
 * s3d_hier_coarse_samples — :141-159.  nears, fars [N] by the expressions of s3d_near_far_from_aabb; z [N,S] = near + (far - near) *
 * lin_i with lin = torch.linspace(0, 1, S) formed as torch forms it (step = 1 / (S - 1); fma(step, i, 0) for i < S / 2, else
 * fma(-step, S - 1 - i, 1): torch's kernels contract these two), + (noise - 0.5) * sample_dist where noise [N,S] (the host's
 * torch.rand values) is given; xyz [N,S,3] = min(max(o + d z, aabb_lo), aabb_hi).  Every other operation is rounded on its own, as
 * the torch op sequence rounds it: z, nears, fars and xyz equal the torch ops on the device bit for bit.  sample_dist, here and
 * below, is (far - near) * fl(1 / S): how torch's device kernel divides by a host scalar.
 *
 * s3d_hier_upsample — :174-186 and sample_pdf :12-46, U >= 1.  Per ray: delta_i = z_{i+1} - z_i (the last (far - near) / S),
 * alpha_i = 1 - exp(-delta_i density_scale sigma_i), T_i = prod_{k<i} (1 - alpha_k + 1e-15), w_i = alpha_i T_i, bins z_mid_i =
 * z_i + delta_i / 2 (S - 1 of them), pdf = (w[1..S-2] + 1e-5) / sum, cdf = [0 | running sum of pdf]; for each u: the first cdf entry
 * above u (searchsorted right=True), its neighbour below, denom < 1e-5 -> 1, linear interpolation between the two bins.  u [N,U]
 * (training: the host's values) or NULL: torch.linspace(0.5 / U, 1 - 0.5 / U, U).  Outputs new_z [N,U], new_xyz [N,U,3] (clamped
 * like xyz), z_sorted [N,K] = sort(cat(z, new_z)) and order [N,K] int32 with cat(z, new_z)[order] == z_sorted exactly; equal depths
 * in column order.  sigma [N,S] is read, not differentiated (:174 runs under no_grad).
 *
 * s3d_hier_weights — :205-215.  weights [N,K] = alpha T of the merged row (delta from z_sorted, the last (far - near) / S; sigma of
 * sorted slot p = sigma_cat[order[p]]) and mask [N,K] (one byte per element: weights > 1e-4), both in concatenated order.
 *
 * s3d_hier_composite_forward — :222-229.  weights_sum [N] = sum w, depth [N] = sum w clamp((z - near) / (far - near), 0, 1),
 * image [N,3] = sum w rgb (rgbs [N,K,3]; the background is the caller's).  A ray that misses the box has near = far = FLT_MAX and
 * the reference's depth is 0 / 0 = NaN there: the clamp keeps a NaN (torch.clamp does, fminf / fmaxf would not).
 *
 * s3d_hier_composite_backward — the backward of s3d_hier_weights + s3d_hier_composite_forward w.r.t. sigma_cat and rgbs.  With
 * s_p = 1 - alpha_p + 1e-15 and G_p = grad_image . rgb_p + grad_weights_sum + grad_depth znorm_p (sorted slots):
 *   grad_sigma_p = delta_p density_scale exp(-delta_p density_scale sigma_p) (G_p T_p - (sum_{q>p} G_q w_q) / s_p)
 *   grad_rgb_p   = w_p grad_image
 * written at column order[p].  grad_image [N,3], grad_weights_sum [N], grad_depth [N]: each may be NULL for zero (a NULL
 * grad_depth also keeps the NaN of a missing ray's depth out of the gradients, as autograd does when depth is not used). */
int s3d_hier_max_samples(void);
int s3d_hier_coarse_samples(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near, uint32_t S,
                            const float* noise, float* nears, float* fars, float* z, float* xyz, s3d_stream_t stream);
int s3d_hier_upsample(const float* z, const float* sigma, const float* nears, const float* fars, float density_scale,
                      const float* u, const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, uint32_t S,
                      uint32_t U, float* new_z, float* new_xyz, float* z_sorted, int32_t* order, s3d_stream_t stream);
int s3d_hier_weights(const float* z_sorted, const int32_t* order, const float* sigma_cat, const float* nears, const float* fars,
                     float density_scale, uint32_t N, uint32_t S, uint32_t U, float* weights, uint8_t* mask, s3d_stream_t stream);
int s3d_hier_composite_forward(const float* weights, const float* rgbs, const float* z_sorted, const int32_t* order,
                               const float* nears, const float* fars, uint32_t N, uint32_t S, uint32_t U, float* weights_sum,
                               float* depth, float* image, s3d_stream_t stream);
int s3d_hier_composite_backward(const float* grad_image, const float* grad_weights_sum, const float* grad_depth,
                                const float* sigma_cat, const float* rgbs, const float* z_sorted, const int32_t* order,
                                const float* nears, const float* fars, float density_scale, uint32_t N, uint32_t S, uint32_t U,
                                float* grad_sigma_cat, float* grad_rgbs, s3d_stream_t stream);

/* ------------------------------------------------------------------ SDF (csrc/sdf.hip, csrc/sdf_pair.hpp; DESIGN.md "SDF")
 * The data path of the signed-distance backbone (sdf/provider.py and loss.py:7-16 of the reference).  All tensors fp32, row-major
 * and on the device unless noted; triangles [F,3,3] = F x {A, B, C} x {x, y, z}.
 *
 * s3d_mesh_sdf — sdf [N], winding [N] (optional), nearest_face [N] int32 (optional) of points [N,3] against F triangles, brute
 * force (N F pair tests, one lane per point, the triangles staged through LDS in tiles of s3d_mesh_sdf_tile() = 256).
 *   distance: min over the faces of the exact point-triangle distance = min(the three edge segments — whose end points are the
 *     three vertices — and, where the foot of the perpendicular lies inside the face, the distance to its plane).  An edge with
 *     |e|^2 <= 1e-30 is its start point, a face with |n|^2 <= 1e-30 (n = (B - A) x (C - A)) has no plane: a zero-area triangle is
 *     its segment or its point.  nearest_face: the face of the minimum, the lowest index among equals.
 *   winding:  w = (1 / 4 pi) sum_f Omega_f, Omega_f = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) with a, b, c the
 *     vertices minus the point; Omega_f = 0 for a face without area and where a.(b x c) == 0 (the point in the face's plane: also on
 *     an edge or a vertex, where atan2 would have no defined argument).
 *   sign:     sdf = -dist where w > 0.5, +dist elsewhere: negative inside a mesh whose triangles face outward (the sign of the
 *     reference's -pysdf(points)).
 * No input yields NaN or Inf from finite coordinates.  N == 0: S3D_OK, nothing launched.  F == 0: S3D_ERR_INVALID.
 *
 * s3d_sdf_sample_points — points [N,3] of one dataset item (SDFDataset.__getitem__), N % 8 == 0, N <= 2^28:
 *   rows [0, N/2)     a point on the surface
 *   rows [N/2, 7N/8)  a point on the surface + noise_std * (standard normal per axis)
 *   rows [7N/8, N)    uniform in [-1, 1)^3
 * Word j of row n is hash_u32(key, step, 8 n + j) (csrc/s3d_common.hpp); U(w) = (w >> 8) / 2^24 in [0, 1).  Surface rows: the face is
 * the first f with cdf[f] > U(word 0) (cdf [F] normalised, non-decreasing, cdf[F-1] = 1: faces in proportion to their area), the point
 * (1 - s) A + s (1 - u2) B + s u2 C with s = sqrt(U(word 1)), u2 = U(word 2).  Normals by Box-Muller: r = sqrt(-2 ln(((w >> 8) + 1) /
 * 2^24)), angle 2 pi U(next word): x, y from words 3, 4 (cosine, sine), z from words 5, 6 (cosine).  Uniform rows: 2 U(word j) - 1
 * for j = 0, 1, 2 (exact in fp32).  face [N] int32 (optional): the drawn face, -1 for the uniform rows.  An item is a pure
 * function of (key, step) and the mesh.
 *
 * s3d_sdf_mape_forward_backward — loss[0] = mean_b(|p_b - t_b| / (|t_b| + 1e-2)), p = clamp(pred, -clip, clip) (clip <= 0: none),
 * and grad = grad_scale * sign(p - t) / ((|t| + 1e-2) * B) in fp32 (sign(0) = 0; 0 where |pred| > clip), in one launch.  pred and
 * grad: S3D_F32 -> [B,1] fp32; S3D_F16 -> the [B,16] fp16 rows of the MLP's padded output, column 0 the distance, and grad's columns
 * 1..15 written as zero (grad 16-byte aligned).  target [B].  The sum runs in a fixed order (a lane's rows, lanes by a shuffle tree,
 * waves, then workgroups in index order through `workspace`, s3d_sdf_mape_workspace_size(B) bytes, 16-byte aligned) without float
 * atomics: the same inputs give the same bits.  B == 0: S3D_ERR_INVALID. */
int s3d_mesh_sdf_tile(void);
int s3d_mesh_sdf(const float* points, uint32_t N, const float* triangles, uint32_t F, float* sdf, float* winding,
                 int32_t* nearest_face, s3d_stream_t stream);
int s3d_sdf_sample_points(const float* triangles, const float* cdf, uint32_t F, uint32_t N, uint32_t key, uint32_t step,
                          float noise_std, float* points, int32_t* face, s3d_stream_t stream);
size_t s3d_sdf_mape_workspace_size(uint32_t B);
int s3d_sdf_mape_forward_backward(const void* pred, int dtype, const float* target, uint32_t B, float clip, float grad_scale,
                                  float* loss, void* grad, void* workspace, size_t workspace_bytes, s3d_stream_t stream);

/* ------------------------------------------------------------------ SDF: BVH query (csrc/sdf_bvh.hip, csrc/sdf_pair.hpp; DESIGN.md "SDF")
 * The same query as s3d_mesh_sdf over a bounding-volume hierarchy that sdf/bvh.py: MeshBVH builds once per mesh on the host.  Every
 * coordinate of points and triangles lies in [-4, 4] (the dataset normalises into [-1, 1]); the pruning slack is derived from that.
 *
 * The tree.  LEAF = s3d_mesh_bvh_leaf() = 4 faces per leaf.  The faces are sorted (stably) by the 30-bit Morton code of their
 * centroid; perm [F] int32: perm[k] is the original index of sorted face k.  L, the number of leaves, is the smallest power of two
 * with L LEAF >= F (F <= 2^26: at most 2^24 leaves, depth 24).  The 2L - 1 nodes are in heap order: the children of node i are
 * 2i + 1 and 2i + 2, the leaves are the last L nodes, and node i at depth d (i = 2^d - 1 + k) covers the sorted faces
 * [k S, (k + 1) S) below F with S = (L >> d) LEAF.  A kernel finds nodes and face ranges by this arithmetic alone and reads perm
 * only at the faces of a leaf, below F.
 *   nodes [2L-1, 16] fp32, 16-byte aligned; per node:
 *     [0..2]   lo: the lower corner of the node's (fp32) vertices, one step of nextafter towards -inf;  [3] 0
 *     [4..6]   hi: the upper corner, one step towards +inf;  [7] 0
 *     [8..10]  c: the area-weighted centroid of the faces (the mean of the vertices where the faces have no area)
 *     [11]     r: the largest |vertex - c| over the node's vertices (c as stored), rounded up
 *     [12..14] Nsum = sum_f (B - A) x (C - A) / 2, summed in float64, then rounded;  [15] 0
 *   A node without faces (padding behind F) has lo = +inf, hi = -inf, c = Nsum = 0 and r = -1.
 *   staged [F, 20] fp32, 16-byte aligned: the sorted faces as s3d_mesh_bvh_stage writes them from triangles [F,3,3] (already in
 *     sorted order) — A, B - A, C - A, the normal, the reciprocal squared lengths and dot products that s3d_mesh_sdf stages through
 *     LDS, made by the same function, so a pair test reads the same bits on either route.  F == 0: S3D_OK, nothing launched.
 *
 * s3d_mesh_sdf_bvh — sdf [N], winding [N] (optional), nearest_face [N] int32 (optional); one launch, a lane per point and walk
 * (64 points per workgroup: one wave walks for the distance, one for the winding number), no host read, no atomics: the same
 * inputs give the same bits.
 *   distance: the minimum over the visited faces of s3d_mesh_sdf's pair test.  A walk from the root, the child with the nearer box
 *     first; a subtree is skipped only where the fp32 distance to its box exceeds sqrt(best) by more than a slack of 1e-4 (csrc/
 *     sdf_pair.hpp derives it), so every face whose computed d^2 is <= the final minimum is visited.  nearest_face is the ORIGINAL
 *     index (through perm), the lowest among equal d^2.  |sdf| and nearest_face equal s3d_mesh_sdf's bit for bit.
 *   winding:  a second walk in depth-first order, left child first (a fixed summation order): a node without faces adds 0; a node
 *     with |c - p|^2 > (beta r)^2 adds Nsum.(c - p) / |c - p|^3 (the dipole term of Barill et al., "Fast winding numbers"); a leaf
 *     that is not far adds Omega_f of s3d_mesh_sdf per face; any other node is opened.  w = sum / 4 pi, sdf = -dist where w > 0.5.
 *     w differs from s3d_mesh_sdf's by the far-field approximation: at beta = 3 by at most about 1.2e-2 up to 5,120 faces (profiles/
 *     sdf_bvh.md), against the gap of 0.5 between a closed mesh's winding numbers and the sign rule's cut.
 *   Both walks are stackless over the heap indices and stop after 2 (2L - 1) iterations; a point whose walk reaches that cap gets
 *     sdf = NaN.  It is not reached on a tree of this contract (a walk visits a node at most once).
 * N == 0: S3D_OK, nothing launched.  F == 0, F > 2^26, L not a power of two, L LEAF < F, beta <= 0 or not finite, NULL points /
 * nodes / staged / perm / sdf: S3D_ERR_INVALID. */
int s3d_mesh_bvh_leaf(void);
int s3d_mesh_bvh_stage(const float* triangles, uint32_t F, float* staged, s3d_stream_t stream);
int s3d_mesh_sdf_bvh(const float* points, uint32_t N, const float* nodes, const float* staged, const int32_t* perm, uint32_t F,
                     uint32_t L, float beta, float* sdf, float* winding, int32_t* nearest_face, s3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEAL3D_HIP_H */
