// raysample.hip — error-map importance sampling of training rays (nerf/utils.py:102-114 `get_rays(error_map=...)`, the
// EMA update of nerf/utils.py:506-528) for gfx950.
//
//  * s3d_sample_train_rays: one workgroup per batch row, 1,024 threads x 16 cells = the 128 x 128 map of that row's image.
//    Weighted sampling without replacement as an exponential race: cell c gets key w_c / E_c, E_c = -log(u_c) ~ Exp(1), and
//    the N largest keys win (torch.multinomial(replacement=False) draws from the same distribution).  The keys stay in
//    VGPRs; a radix select over their bits (4 passes of 8 bits, per-wave LDS histograms) finds the N-th largest key, and one
//    block scan emits the winners in ascending cell order — at the threshold key the lower cell index wins.  Zero-weight
//    cells have key 0: when fewer than N cells are positive the rest is filled with zero-weight cells by index (where
//    torch.multinomial raises).  Each winner's thread then applies the fine perturb, forms the ray (the get_rays expression
//    and the pose rotation) and gathers its target colour / depth straight into the caller's buffers.  Without a map the
//    same launch draws the reference's uniform randint pixels.  The step number of the counter-based hash is read from
//    device memory and advanced by the last workgroup to finish, so a captured launch draws fresh cells on every replay.
//  * s3d_error_map_update: one workgroup; the depth term's batch mean is reduced first in a fixed order, then every ray's
//    error (the torch route's float expressions) is folded into its cell as 0.1 old + 0.9 err.  A non-finite error leaves the
//    cell's old value in place.
//  * s3d_rgba_targets / s3d_sample_train_rays_rgba: training targets of RGBA frames (nerf/utils.py:465-474).  Each row's
//    background is 1 or three uniforms in [0, 1), and gt = rgb * a + bg * (1 - a) in fp32 (fp16 frames are widened first).
//    Keying of the uniforms: bg_key = pcg_hash(seed ^ 0x3C6EF372), u = (float)(hash_u32(bg_key, step, 3 * row + c) >> 8) * 2^-24
//    for channel c of batch slot row = b * N + n (s3d_rgba_targets: the row itself), step = ctl[0] — a constant none of the
//    sampler's other keys uses (pixels 0x5BD1E995, rows 0x632BE5AB, fine perturb 0xA511E9B3), so what they draw for a seed
//    does not move.  The sampler's RGBA form is the same kernel body (template flag): one launch gathers four channels, blends,
//    and writes gt and bg.
//  * s3d_orbit_rays: Seal-3D's custom-pose batches (SealNeRF/provider.py:145-178) — B orbit cameras around look_at drawn as
//    nerf/provider.py:57-91 `rand_poses` draws them (theta_key = pcg_hash(seed ^ 0x1B873593), phi_key = pcg_hash(seed ^
//    0xCC9E2D51), u = (float)(hash_u32(key, step, b) >> 8) * 2^-24: two more constants of their own) and every ray of each
//    pose's rH x rW frame, formed by the sampler's own ray function.  A pose's frame spans many workgroups: each recomputes
//    the pose (one thread, handed round through LDS), and every lane stores 16 aligned bytes of the flat [B, rH rW, 3] stream.
//  * s3d_frame_rays: the rays of ONE given camera for a whole rH x rW frame (get_rays(pose, intrinsics, rH, rW, -1), the
//    first step of a preview frame: nerf/utils.py:754-763).  The pose travels in the launch's argument block; each lane stores
//    16 aligned bytes of the flat [rH rW, 3] stream, the ray formed by pixel_ray_dir like every other ray of this file.
#include "s3d_common.hpp"

#include <math.h>

#include <algorithm>
#include <cmath>

namespace s3d {
namespace {

constexpr uint32_t kCells = 128 * 128;
constexpr uint32_t kSampleBlock = 1024;
constexpr uint32_t kPerThread = kCells / kSampleBlock;  // 16
constexpr uint32_t kWaves = kSampleBlock / 64;           // 16
constexpr uint32_t kUpdateBlock = 1024;
static_assert(kPerThread == 16, "16 cells per thread");

// Exp(1) variate from a full 32-bit word: -log(u) for u in the lower half, -log1p(-(1 - u)) in the upper one, so that the
// key keeps ~24 significant bits of randomness across the whole range (a 24-bit uniform would tie often among 16,384 cells)
__device__ __forceinline__ float exp_variate(uint32_t h) {
    if (h < 0x80000000u) return 0.0f - logf(((float)h + 0.5f) * 0x1p-32f);
    return 0.0f - log1pf(0.0f - ((float)(0xFFFFFFFFu - h) + 0.5f) * 0x1p-32f);
}

// key bits of one cell: w / E (correctly rounded, -ffp-contract=off) as an unsigned word, monotone for keys >= 0; weights
// that are not positive (and a NaN key) rank as 0, below every positive key
__device__ __forceinline__ uint32_t key_bits(float w, float E) {
    if (!(w > 0.0f)) return 0u;
    const float k = w / E;
    return k >= 0.0f ? __float_as_uint(k) : 0u;
}

// block-wide exclusive scan of one word per thread (1,024 threads), total in *total
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    if (t < 64) {
        const uint32_t x = t < kWaves ? s_wave[t] : 0u;
        const uint32_t xi = wave_incl_scan(x);
        if (t < kWaves) s_wave[kWaves + t] = xi - x;
        if (t == kWaves - 1) *total = xi;
    }
    __syncthreads();
    return s_wave[kWaves + wave] + incl - v;
}

constexpr uint32_t kBgKeySalt = 0x3C6EF372u;
constexpr uint32_t kTargetsBlock = 256;

// one RGBA pixel (16-byte load of fp32 frames, 8-byte load of fp16 frames widened to fp32)
__device__ __forceinline__ float4 load_rgba(const void* __restrict__ images, size_t pix, bool f16) {
    if (f16) {
        const uint2 raw = reinterpret_cast<const uint2*>(images)[pix];
        const __half2 lo = *reinterpret_cast<const __half2*>(&raw.x), hi = *reinterpret_cast<const __half2*>(&raw.y);
        return make_float4(__low2float(lo), __high2float(lo), __low2float(hi), __high2float(hi));
    }
    return reinterpret_cast<const float4*>(images)[pix];
}

// background and blended target of one row (nerf/utils.py:465-474): bg = 1, the caller's uniforms, or the counter hash;
// gt = fl(fl(rgb * a) + fl(bg * fl(1 - a))) — torch's expression, no contraction
__device__ __forceinline__ void rgba_target(float4 px, uint32_t random_bg, const float* __restrict__ u_bg, uint32_t bg_key,
                                            uint32_t step, size_t row, float* __restrict__ gt, float* __restrict__ bg) {
    const float rgb[3] = {px.x, px.y, px.z};
    const float ia = 1.0f - px.w;
#pragma unroll
    for (uint32_t c = 0; c < 3; c++) {
        float v = 1.0f;
        if (random_bg) v = u_bg ? u_bg[row * 3 + c] : (float)(hash_u32(bg_key, step, 3u * (uint32_t)row + c) >> 8) * (1.0f / 16777216.0f);
        const float fg = rgb[c] * px.w, back = v * ia;
        gt[row * 3 + c] = fg + back;
        if (bg) bg[row * 3 + c] = v;
    }
}

// the last workgroup to finish advances the step number (every workgroup read it first); called by one thread per workgroup
// behind a __syncthreads()
__device__ __forceinline__ void advance_step(int32_t* ctl, uint32_t step) {
    __threadfence();
    const int32_t arrived = atomicAdd(&ctl[1], 1);
    if (arrived == (int32_t)gridDim.x - 1) {
        __threadfence();
        ctl[1] = 0;
        ctl[0] = (int32_t)(step + 1u);
    }
}

__global__ void __launch_bounds__(kTargetsBlock)
k_rgba_targets(const void* __restrict__ images, uint32_t f16, uint32_t R, uint32_t random_bg, uint32_t seed, int32_t* ctl,
               const float* __restrict__ u_bg, float* __restrict__ gt, float* __restrict__ bg) {
    const uint32_t step = ctl ? (uint32_t)ctl[0] : 0u;
    const uint32_t bg_key = pcg_hash(seed ^ kBgKeySalt);
    for (uint32_t r = blockIdx.x * kTargetsBlock + threadIdx.x; r < R; r += gridDim.x * kTargetsBlock)
        rgba_target(load_rgba(images, r, f16 != 0), random_bg, u_bg, bg_key, step, r, gt, bg);
    if (ctl) {
        __syncthreads();
        if (threadIdx.x == 0) advance_step(ctl, step);
    }
}

struct SampleArgs {
    const float* error_map;  // [n_img, 16384] or NULL (uniform pixels)
    const int64_t* index;    // [B] image of each batch row
    const float* poses;      // [n_img, 4, 4]
    const void* images;      // [n_img, H, W, 3] (kRgba: 4) fp32 / fp16 or NULL
    const float* depths;     // [n_img, H * W] or NULL
    const float* u_keys;     // [B, 16384] or NULL (test entry: explicit uniforms of the keys)
    const float* u_fine;     // [B, N, 2] or NULL (test entry: explicit uniforms of the fine perturb)
    int32_t* ctl;            // {step, arrivals} or NULL (explicit uniforms)
    float* rays_o;
    float* rays_d;
    float* gt;
    float* gt_depth;
    int64_t* inds;
    int64_t* inds_coarse;
    int64_t* out_index;      // [B] copy of index or NULL (the static index buffer of a captured step)
    const float* u_bg;       // kRgba: [B, N, 3] or NULL (test entry: explicit uniforms of the background)
    float* bg;               // kRgba: [B, N, 3] or NULL
    uint32_t random_bg;      // kRgba: 0 = blend onto 1
    uint32_t N, n_img, H, W, seed, img_f16;
    float fx, fy, cx, cy, sx, sy;
};

// world direction of the ray through pixel `pix` of a frame W wide (get_rays: pixel centre, normalised direction, cam2world
// rotation; pose = rows of the 4 x 4 matrix) — the one copy the sampler and the orbit-frame kernel both form their rays with
__device__ __forceinline__ void pixel_ray_dir(uint32_t pix, uint32_t W, float fx, float fy, float cx, float cy,
                                              const float* __restrict__ pose, float d[3]) {
    const float i = (float)(pix % W) + 0.5f, j = (float)(pix / W) + 0.5f;
    const float x = (i - cx) / fx * 1.0f, y = (j - cy) / fy * 1.0f, z = 1.0f;
    const float nrm = sqrtf(x * x + y * y + z * z);
    const float dx = x / nrm, dy = y / nrm, dz = z / nrm;
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = dx * pose[k * 4] + dy * pose[k * 4 + 1] + dz * pose[k * 4 + 2];
}

// the ray of pixel `pix` into row b's slot n + targets
template <bool kRgba>
__device__ __forceinline__ void emit_ray(const SampleArgs& a, uint32_t b, uint32_t img, uint32_t n, uint32_t pix,
                                         const float* __restrict__ pose, uint32_t step) {
    const size_t o = (size_t)b * a.N + n;
    float d[3];
    pixel_ray_dir(pix, a.W, a.fx, a.fy, a.cx, a.cy, pose, d);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.rays_d[o * 3 + k] = d[k];
        a.rays_o[o * 3 + k] = pose[k * 4 + 3];
    }
    a.inds[o] = (int64_t)pix;
    const size_t src = (size_t)img * a.H * a.W + pix;
    if (kRgba) {
        if (a.images && a.gt)
            rgba_target(load_rgba(a.images, src, a.img_f16 != 0), a.random_bg, a.u_bg, pcg_hash(a.seed ^ kBgKeySalt), step, o, a.gt, a.bg);
    } else if (a.images && a.gt) {
        if (a.img_f16) {
            const __half* im = reinterpret_cast<const __half*>(a.images);
#pragma unroll
            for (int k = 0; k < 3; k++) a.gt[o * 3 + k] = __half2float(im[src * 3 + k]);
        } else {
            const float* im = reinterpret_cast<const float*>(a.images);
#pragma unroll
            for (int k = 0; k < 3; k++) a.gt[o * 3 + k] = im[src * 3 + k];
        }
    }
    if (a.depths && a.gt_depth) a.gt_depth[o] = a.depths[src];
}

template <bool kRgba>
__global__ void __launch_bounds__(kSampleBlock) k_sample_train_rays(SampleArgs a) {
    __shared__ uint32_t s_hist[kWaves * 256];
    __shared__ uint32_t s_scan[2 * kWaves];
    __shared__ uint32_t s_sel[4];  // {digit, remaining k, total, step}
    const uint32_t t = threadIdx.x, b = blockIdx.x, wave = t >> 6;
    const uint32_t img = (uint32_t)a.index[b];
    if (t == 0) {
        s_sel[3] = a.ctl ? (uint32_t)a.ctl[0] : 0u;
        if (a.out_index) a.out_index[b] = (int64_t)img;
    }
    __syncthreads();
    const uint32_t step = s_sel[3];
    const float* pose = a.poses + (size_t)img * 16;

    if (img >= a.n_img) {
        // (an index outside the dataset: the row is left unwritten rather than read out of bounds)
    } else if (!a.error_map) {
        // uniform pixels (nerf/utils.py:98: randint(0, H*W, [N]) shared by the batch rows)
        const uint32_t key = pcg_hash(a.seed ^ 0x5BD1E995u), HW = a.H * a.W;
        for (uint32_t n = t; n < a.N; n += kSampleBlock) {
            const uint32_t pix = (uint32_t)(((uint64_t)hash_u32(key, step, n) * HW) >> 32);
            emit_ray<kRgba>(a, b, img, n, pix, pose, step);
        }
    } else {
        // keys of this thread's 16 consecutive cells, in registers
        const uint32_t c0 = t * kPerThread;
        const float4* w4 = reinterpret_cast<const float4*>(a.error_map + (size_t)img * kCells + c0);
        const uint32_t row_key = pcg_hash(a.seed + 0x632BE5ABu * (img + 1u));
        uint32_t key[kPerThread];
#pragma unroll
        for (uint32_t q = 0; q < kPerThread / 4; q++) {
            const float4 w = w4[q];
            const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (uint32_t r = 0; r < 4; r++) {
                const uint32_t c = c0 + q * 4 + r;
                const float E = a.u_keys ? 0.0f - logf(a.u_keys[(size_t)b * kCells + c]) : exp_variate(hash_u32(row_key, step, c));
                key[q * 4 + r] = key_bits(wv[r], E);
            }
        }
        // radix select of the N-th largest key: prefix/mask of the bits decided so far, k = how many keys matching the prefix
        // are still to be taken
        uint32_t prefix = 0, mask = 0, k = a.N;
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (uint32_t e = t; e < kWaves * 256; e += kSampleBlock) s_hist[e] = 0u;
            __syncthreads();
#pragma unroll
            for (uint32_t q = 0; q < kPerThread; q++)
                if ((key[q] & mask) == prefix) atomicAdd(&s_hist[wave * 256 + ((key[q] >> shift) & 255u)], 1u);
            __syncthreads();
            // thread t < 256 owns digit 255 - t: the inclusive scan over t counts the keys with a digit >= its own
            uint32_t cnt = 0;
            if (t < 256) {
#pragma unroll
                for (uint32_t w = 0; w < kWaves; w++) cnt += s_hist[w * 256 + (255u - t)];
            }
            uint32_t incl = 0;
            if (t < 256) {
                incl = wave_incl_scan(cnt);
                if ((t & 63u) == 63u) s_scan[t >> 6] = incl;
            }
            __syncthreads();
            if (t < 256) {
                for (uint32_t w = 0; w < (t >> 6); w++) incl += s_scan[w];
                const uint32_t excl = incl - cnt;
                if (excl < k && incl >= k) { s_sel[0] = 255u - t; s_sel[1] = k - excl; }
            }
            __syncthreads();
            prefix |= s_sel[0] << shift;
            mask |= 255u << shift;
            k = s_sel[1];
            __syncthreads();
        }
        // prefix = the threshold key, k = how many of the keys equal to it are taken (the lowest cells first)
        uint32_t n_gt = 0, n_eq = 0;
#pragma unroll
        for (uint32_t q = 0; q < kPerThread; q++) { n_gt += key[q] > prefix; n_eq += key[q] == prefix; }
        const uint32_t before = block_excl_scan((n_gt << 16) | n_eq, s_scan, &s_sel[2]);
        uint32_t gt_before = before >> 16, eq_before = before & 0xFFFFu;
        const uint32_t fine_key = pcg_hash(row_key ^ 0xA511E9B3u);
#pragma unroll
        for (uint32_t q = 0; q < kPerThread; q++) {
            const bool gt = key[q] > prefix, eq = key[q] == prefix;
            if (gt || (eq && eq_before < k)) {
                const uint32_t n = gt_before + (eq_before < k ? eq_before : k);
                if (n < a.N) {
                    const uint32_t c = c0 + q;
                    float ux, uy;
                    if (a.u_fine) {
                        ux = a.u_fine[((size_t)b * a.N + n) * 2];
                        uy = a.u_fine[((size_t)b * a.N + n) * 2 + 1];
                    } else {
                        ux = (float)(hash_u32(fine_key, step, 2u * c) >> 8) * (1.0f / 16777216.0f);
                        uy = (float)(hash_u32(fine_key, step, 2u * c + 1u) >> 8) * (1.0f / 16777216.0f);
                    }
                    // (inds_x * sx + rand * sx).long().clamp(max=H - 1), the same for y (nerf/utils.py:108-111)
                    const float fxv = (float)(c >> 7) * a.sx + ux * a.sx, fyv = (float)(c & 127u) * a.sy + uy * a.sy;
                    uint32_t px = (uint32_t)(int64_t)fxv, py = (uint32_t)(int64_t)fyv;
                    px = px < a.H - 1 ? px : a.H - 1;
                    py = py < a.W - 1 ? py : a.W - 1;
                    a.inds_coarse[(size_t)b * a.N + n] = (int64_t)c;
                    emit_ray<kRgba>(a, b, img, n, px * a.W + py, pose, step);
                }
            }
            gt_before += gt;
            eq_before += eq;
        }
    }
    // the last workgroup to finish advances the step number (every workgroup read it above)
    if (a.ctl) {
        __syncthreads();
        if (t == 0) advance_step(a.ctl, step);
    }
}

__device__ __forceinline__ float block_sum_fixed(float v, float* s_red) {
    // fixed-order tree over the 1,024 per-thread partial sums
    const uint32_t t = threadIdx.x;
    s_red[t] = v;
    __syncthreads();
    for (uint32_t h = kUpdateBlock / 2; h > 0; h >>= 1) {
        if (t < h) s_red[t] = s_red[t] + s_red[t + h];
        __syncthreads();
    }
    const float r = s_red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kUpdateBlock)
k_error_map_update(float* __restrict__ error_map, const int64_t* __restrict__ index, const int64_t* __restrict__ inds_coarse,
                   uint32_t B, uint32_t N, uint32_t n_img, const float* __restrict__ image, const float* __restrict__ weights_sum,
                   const float* __restrict__ gt, float bg0, float bg1, float bg2, const float* __restrict__ bg_rays,
                   const float* __restrict__ depth, const float* __restrict__ gt_depth, float depth_weight) {
    __shared__ float s_red[kUpdateBlock];
    const uint32_t t = threadIdx.x, R = B * N;
    float dterm = 0.0f;
    if (depth) {
        float acc = 0.0f;
        for (uint32_t r = t; r < R; r += kUpdateBlock) {
            float d = depth[r];
            d = d != d ? 0.0f : (d == INFINITY ? 3.4028234663852886e38f : (d == -INFINITY ? -3.4028234663852886e38f : d));
            acc += fabsf(d - gt_depth[r]);
        }
        dterm = depth_weight * (block_sum_fixed(acc, s_red) / (float)R);
    }
    for (uint32_t r = t; r < R; r += kUpdateBlock) {
        const uint32_t b = r / N;
        const float ws = weights_sum ? 1.0f - weights_sum[r] : 0.0f;
        float e = 0.0f;
        float sq[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float bg = bg_rays ? bg_rays[(size_t)r * 3 + k] : (k == 0 ? bg0 : (k == 1 ? bg1 : bg2));
            const float p = weights_sum ? image[(size_t)r * 3 + k] + ws * bg : image[(size_t)r * 3 + k];
            const float d = p - gt[(size_t)r * 3 + k];
            sq[k] = d * d;
        }
        e = (sq[0] + sq[1] + sq[2]) * (1.0f / 3.0f);  // (torch's mean over the channels: the sum times 1 / 3)
        if (depth) e = e + dterm;
        if (!isfinite(e)) continue;  // (documented deviation: one bad step must not poison the sampler)
        const uint64_t img = (uint64_t)index[b], c = (uint64_t)inds_coarse[r];
        if (img >= n_img || c >= kCells) continue;  // (out-of-range entries: nothing to update)
        float* cell = error_map + img * kCells + c;
        *cell = 0.1f * *cell + 0.9f * e;
    }
}

constexpr uint32_t kThetaKeySalt = 0x1B873593u, kPhiKeySalt = 0xCC9E2D51u;
constexpr uint32_t kOrbitBlock = 256;
// workgroups per pose at most; larger frames go round the item loop.  Every workgroup ends in advance_step's fence and
// arrival (about 27 ns each, one after the other): 1,875 of them made an 800 x 800 frame 60 us, 256 make it 19 us, and
// without the counter (explicit uniforms) the frame is written in 10 us either way (profiles/custom_pose.md)
constexpr uint32_t kOrbitMaxChunks = 256;

struct OrbitArgs {
    const float* u_pose;  // [B, 2] or NULL (test entry: explicit uniforms of theta, phi)
    int32_t* ctl;         // {step, arrivals} or NULL (explicit uniforms)
    float* poses_out;     // [B, 4, 4] or NULL
    float* rays_o;        // [B, HW, 3], 16-byte aligned
    float* rays_d;
    uint32_t W, HW, chunks, seed;
    float fx, fy, cx, cy;
    float radius, th_lo, th_span, ph_lo, ph_span, look[3];
};

__device__ __forceinline__ void normalize3(const float v[3], float out[3]) {
    const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-10f;
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = v[k] / n;
}

__device__ __forceinline__ void cross3(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// nerf/provider.py:57-91 `rand_poses` for one pair of uniforms, its expression order in fp32, + look_at on the centre: the
// 16 values of the cam2world matrix (columns right, up, forward, centre)
__device__ __forceinline__ void orbit_pose(const OrbitArgs& a, float u_theta, float u_phi, float* pose) {
    const float theta = u_theta * a.th_span + a.th_lo, phi = u_phi * a.ph_span + a.ph_lo;
    const float st = sinf(theta), ct = cosf(theta), sp = sinf(phi), cp = cosf(phi);
    const float off[3] = {a.radius * st * sp, a.radius * ct, a.radius * st * cp};
    const float up0[3] = {0.0f, -1.0f, 0.0f};
    float fwd[3], right[3], up[3], tmp[3];
    normalize3(off, fwd);
#pragma unroll
    for (int k = 0; k < 3; k++) fwd[k] = -fwd[k];
    cross3(fwd, up0, tmp);
    normalize3(tmp, right);
    cross3(right, fwd, tmp);
    normalize3(tmp, up);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        pose[k * 4] = right[k];
        pose[k * 4 + 1] = up[k];
        pose[k * 4 + 2] = fwd[k];
        pose[k * 4 + 3] = off[k] + a.look[k];
    }
    pose[12] = 0.0f; pose[13] = 0.0f; pose[14] = 0.0f; pose[15] = 1.0f;
}

// s3d_orbit_rays: workgroup (b, chunk) = blockIdx.x.  The rays of pose b are one stream of 3 HW floats per output; a work item
// is one 16-byte aligned group of four of them (parts of two neighbouring rays), so that a wave's store instruction covers
// 1 KiB of consecutive addresses.  The first and the last item of a pose may reach into the neighbouring pose's floats (3 HW
// need not be a multiple of 4): only there, each float inside the pose is stored on its own.
__global__ void __launch_bounds__(kOrbitBlock) k_orbit_rays(OrbitArgs a) {
    __shared__ float s_pose[16];
    __shared__ uint32_t s_step;
    const uint32_t t = threadIdx.x, b = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
    if (t == 0) {
        const uint32_t step = a.ctl ? (uint32_t)a.ctl[0] : 0u;
        s_step = step;
        float ut, up;
        if (a.u_pose) {
            ut = a.u_pose[(size_t)b * 2];
            up = a.u_pose[(size_t)b * 2 + 1];
        } else {
            ut = (float)(hash_u32(pcg_hash(a.seed ^ kThetaKeySalt), step, b) >> 8) * (1.0f / 16777216.0f);
            up = (float)(hash_u32(pcg_hash(a.seed ^ kPhiKeySalt), step, b) >> 8) * (1.0f / 16777216.0f);
        }
        orbit_pose(a, ut, up, s_pose);
        if (chunk == 0 && a.poses_out) {
#pragma unroll
            for (int k = 0; k < 16; k++) a.poses_out[(size_t)b * 16 + k] = s_pose[k];
        }
    }
    __syncthreads();
    float pose[12];
#pragma unroll
    for (int k = 0; k < 12; k++) pose[k] = s_pose[k];
    const float o[3] = {pose[3], pose[7], pose[11]};
    const uint64_t F = 3ull * a.HW, lo = (uint64_t)b * F, hi = lo + F;
    const uint64_t q1 = (hi + 3u) >> 2;  // items [lo / 4, q1) hold a float of this pose
    for (uint64_t q = (lo >> 2) + (uint64_t)chunk * kOrbitBlock + t; q < q1; q += (uint64_t)a.chunks * kOrbitBlock) {
        const uint64_t g0 = q << 2;
        const uint32_t f0 = (uint32_t)((g0 > lo ? g0 : lo) - lo);  // the item's first float inside the pose
        const uint32_t r0 = f0 / 3u;
        float d0[3], d1[3];  // the item's floats belong to rays r0 and r0 + 1 (the latter may lie past the frame: never stored)
        pixel_ray_dir(r0, a.W, a.fx, a.fy, a.cx, a.cy, pose, d0);
        pixel_ray_dir(r0 + 1u, a.W, a.fx, a.fy, a.cx, a.cy, pose, d1);
        float vd[4], vo[4];
        bool in[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t g = g0 + j;
            in[j] = g >= lo && g < hi;
            const uint32_t f = in[j] ? (uint32_t)(g - lo) : f0;
            const uint32_t r = f / 3u, c = f - 3u * r;
            const float a0 = r == r0 ? d0[0] : d1[0], a1 = r == r0 ? d0[1] : d1[1], a2 = r == r0 ? d0[2] : d1[2];
            vd[j] = c == 0u ? a0 : (c == 1u ? a1 : a2);
            vo[j] = c == 0u ? o[0] : (c == 1u ? o[1] : o[2]);
        }
        if (in[0] && in[3]) {
            *reinterpret_cast<float4*>(a.rays_d + g0) = make_float4(vd[0], vd[1], vd[2], vd[3]);
            *reinterpret_cast<float4*>(a.rays_o + g0) = make_float4(vo[0], vo[1], vo[2], vo[3]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                if (in[j]) {
                    a.rays_d[g0 + j] = vd[j];
                    a.rays_o[g0 + j] = vo[j];
                }
            }
        }
    }
    // the last workgroup to finish advances the step number (every workgroup read it above)
    if (a.ctl) {
        __syncthreads();
        if (t == 0) advance_step(a.ctl, s_step);
    }
}

struct FrameArgs {
    float pose[12];  // the cam2world matrix's first three rows
    float* rays_o;   // [HW, 3], 16-byte aligned
    float* rays_d;
    uint32_t W, HW;
    float fx, fy, cx, cy;
};

// s3d_frame_rays: a work item is one 16-byte aligned group of four floats of the 3 HW floats of either output (parts of two
// neighbouring rays); only the frame's last item can be partial
__global__ void __launch_bounds__(kOrbitBlock) k_frame_rays(FrameArgs a) {
    const uint32_t F = 3u * a.HW, items = (F + 3u) >> 2;
    for (uint32_t q = blockIdx.x * kOrbitBlock + threadIdx.x; q < items; q += gridDim.x * kOrbitBlock) {
        const uint32_t g0 = q << 2, r0 = g0 / 3u;
        float d0[3], d1[3];  // the item's floats belong to rays r0 and r0 + 1 (the latter may lie past the frame: never stored)
        pixel_ray_dir(r0, a.W, a.fx, a.fy, a.cx, a.cy, a.pose, d0);
        pixel_ray_dir(r0 + 1u, a.W, a.fx, a.fy, a.cx, a.cy, a.pose, d1);
        float vd[4], vo[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t f = g0 + j, r = f / 3u, c = f - 3u * r;
            const float a0 = r == r0 ? d0[0] : d1[0], a1 = r == r0 ? d0[1] : d1[1], a2 = r == r0 ? d0[2] : d1[2];
            vd[j] = c == 0u ? a0 : (c == 1u ? a1 : a2);
            vo[j] = c == 0u ? a.pose[3] : (c == 1u ? a.pose[7] : a.pose[11]);
        }
        if (g0 + 4u <= F) {
            *reinterpret_cast<float4*>(a.rays_d + g0) = make_float4(vd[0], vd[1], vd[2], vd[3]);
            *reinterpret_cast<float4*>(a.rays_o + g0) = make_float4(vo[0], vo[1], vo[2], vo[3]);
        } else {
            for (uint32_t j = 0; g0 + j < F; j++) {
                a.rays_d[g0 + j] = vd[j];
                a.rays_o[g0 + j] = vo[j];
            }
        }
    }
}

}  // namespace
}  // namespace s3d

using namespace s3d;

namespace s3d {
namespace {

// s3d_sample_train_rays and its RGBA form: one argument check, one launch
int launch_sample(bool rgba, const float* error_map, const int64_t* index, uint32_t B, uint32_t N, uint32_t n_img, uint32_t H,
                  uint32_t W, const float* poses, const float* intrinsics, const void* images, int images_dtype, const float* depths,
                  uint32_t seed, int32_t* ctl, const float* u_keys, const float* u_fine, int random_bg, const float* u_bg,
                  float* rays_o, float* rays_d, float* gt, float* bg, float* gt_depth, int64_t* inds, int64_t* inds_coarse,
                  int64_t* out_index, s3d_stream_t stream) {
    S3D_REQUIRE(index && poses && intrinsics && rays_o && rays_d && inds, "s3d_sample_train_rays: null argument");
    S3D_REQUIRE(B > 0 && N > 0 && n_img > 0 && H > 0 && W > 0, "s3d_sample_train_rays: empty batch or frame");
    S3D_REQUIRE(images_dtype == S3D_F32 || images_dtype == S3D_F16, "s3d_sample_train_rays: images must be fp32 or fp16");
    S3D_REQUIRE((uint64_t)H * W < (1ull << 31), "s3d_sample_train_rays: frame too large");
    if (error_map) {
        S3D_REQUIRE(N <= kCells, "s3d_sample_train_rays: N = %u exceeds the 16,384 cells of the map", N);
        S3D_REQUIRE(inds_coarse, "s3d_sample_train_rays: inds_coarse is required with an error map");
        S3D_REQUIRE((reinterpret_cast<uintptr_t>(error_map) & 15u) == 0, "s3d_sample_train_rays: error_map must be 16-byte aligned");
        S3D_REQUIRE(ctl || (u_keys && u_fine), "s3d_sample_train_rays: needs ctl or both explicit uniform arrays");
    } else {
        S3D_REQUIRE(ctl, "s3d_sample_train_rays: uniform pixels need ctl");
    }
    const bool draws_bg = rgba && images && gt && random_bg && !u_bg;
    const bool explicit_draw = error_map && u_keys && u_fine;
    if (rgba) {
        S3D_REQUIRE((uint64_t)B * N * 3 < (1ull << 32), "s3d_sample_train_rays_rgba: batch too large");
        S3D_REQUIRE((reinterpret_cast<uintptr_t>(images) & (images_dtype == S3D_F16 ? 7u : 15u)) == 0,
                    "s3d_sample_train_rays_rgba: images must be aligned to one RGBA pixel");
        S3D_REQUIRE(!bg || (images && gt), "s3d_sample_train_rays_rgba: bg is written with gt");
        S3D_REQUIRE(!draws_bg || ctl, "s3d_sample_train_rays_rgba: a random background needs ctl or u_bg");
    }
    SampleArgs a;
    a.error_map = error_map; a.index = index; a.poses = poses; a.images = images; a.depths = depths;
    a.u_keys = error_map ? u_keys : nullptr; a.u_fine = error_map ? u_fine : nullptr;
    a.ctl = (explicit_draw && !draws_bg) ? nullptr : ctl;
    a.rays_o = rays_o; a.rays_d = rays_d; a.gt = gt; a.gt_depth = gt_depth; a.inds = inds; a.inds_coarse = inds_coarse;
    a.out_index = out_index;
    a.u_bg = u_bg; a.bg = bg; a.random_bg = random_bg != 0;
    a.N = N; a.n_img = n_img; a.H = H; a.W = W; a.seed = seed; a.img_f16 = images_dtype == S3D_F16;
    a.fx = intrinsics[0]; a.fy = intrinsics[1]; a.cx = intrinsics[2]; a.cy = intrinsics[3];
    a.sx = (float)((double)H / 128.0); a.sy = (float)((double)W / 128.0);
    if (rgba) hipLaunchKernelGGL(k_sample_train_rays<true>, dim3(B), dim3(kSampleBlock), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(k_sample_train_rays<false>, dim3(B), dim3(kSampleBlock), 0, as_stream(stream), a);
    return check_launch("k_sample_train_rays");
}

}  // namespace
}  // namespace s3d

S3D_EXPORT int s3d_sample_train_rays(const float* error_map, const int64_t* index, uint32_t B, uint32_t N, uint32_t n_img,
                                     uint32_t H, uint32_t W, const float* poses, const float* intrinsics, const void* images,
                                     int images_dtype, const float* depths, uint32_t seed, int32_t* ctl, const float* u_keys,
                                     const float* u_fine, float* rays_o, float* rays_d, float* gt, float* gt_depth, int64_t* inds,
                                     int64_t* inds_coarse, int64_t* out_index, s3d_stream_t stream) {
    return launch_sample(false, error_map, index, B, N, n_img, H, W, poses, intrinsics, images, images_dtype, depths, seed, ctl, u_keys,
                         u_fine, 0, nullptr, rays_o, rays_d, gt, nullptr, gt_depth, inds, inds_coarse, out_index, stream);
}

S3D_EXPORT int s3d_sample_train_rays_rgba(const float* error_map, const int64_t* index, uint32_t B, uint32_t N, uint32_t n_img,
                                          uint32_t H, uint32_t W, const float* poses, const float* intrinsics, const void* images,
                                          int images_dtype, const float* depths, uint32_t seed, int32_t* ctl, const float* u_keys,
                                          const float* u_fine, int random_bg, const float* u_bg, float* rays_o, float* rays_d,
                                          float* gt, float* bg, float* gt_depth, int64_t* inds, int64_t* inds_coarse,
                                          int64_t* out_index, s3d_stream_t stream) {
    return launch_sample(true, error_map, index, B, N, n_img, H, W, poses, intrinsics, images, images_dtype, depths, seed, ctl, u_keys,
                         u_fine, random_bg, u_bg, rays_o, rays_d, gt, bg, gt_depth, inds, inds_coarse, out_index, stream);
}

S3D_EXPORT int s3d_rgba_targets(const void* images, int images_dtype, uint32_t R, int random_bg, uint32_t seed, int32_t* ctl,
                                const float* u_bg, float* gt, float* bg, s3d_stream_t stream) {
    if (R == 0) return S3D_OK;
    S3D_REQUIRE(images && gt, "s3d_rgba_targets: null argument");
    S3D_REQUIRE(images_dtype == S3D_F32 || images_dtype == S3D_F16, "s3d_rgba_targets: images must be fp32 or fp16");
    S3D_REQUIRE((reinterpret_cast<uintptr_t>(images) & (images_dtype == S3D_F16 ? 7u : 15u)) == 0,
                "s3d_rgba_targets: images must be aligned to one RGBA pixel");
    S3D_REQUIRE((uint64_t)R * 3 < (1ull << 32), "s3d_rgba_targets: too many rows");
    S3D_REQUIRE(!random_bg || bg, "s3d_rgba_targets: a random background is handed out in bg");
    S3D_REQUIRE(!random_bg || u_bg || ctl, "s3d_rgba_targets: a random background needs ctl or u_bg");
    int32_t* step_ctl = (random_bg && !u_bg) ? ctl : nullptr;  // (explicit uniforms, constant background: ctl is left alone)
    hipLaunchKernelGGL(k_rgba_targets, dim3(stream_grid(R, kTargetsBlock)), dim3(kTargetsBlock), 0, as_stream(stream), images,
                       (uint32_t)(images_dtype == S3D_F16), R, (uint32_t)(random_bg != 0), seed, step_ctl, random_bg ? u_bg : nullptr, gt, bg);
    return check_launch("k_rgba_targets");
}

S3D_EXPORT int s3d_error_map_update(float* error_map, uint32_t n_img, const int64_t* index, const int64_t* inds_coarse, uint32_t B,
                                    uint32_t N, const float* image, const float* weights_sum, const float* gt, const float* bg_rgb,
                                    const float* bg_rays, const float* depth, const float* gt_depth, float depth_weight,
                                    s3d_stream_t stream) {
    S3D_REQUIRE(error_map && index && inds_coarse && image && gt, "s3d_error_map_update: null argument");
    S3D_REQUIRE(B > 0 && N > 0 && N <= kCells, "s3d_error_map_update: bad batch shape");
    S3D_REQUIRE((depth == nullptr) == (gt_depth == nullptr), "s3d_error_map_update: depth and gt_depth go together");
    S3D_REQUIRE(weights_sum || (!bg_rgb && !bg_rays), "s3d_error_map_update: a background needs weights_sum");
    const float b0 = bg_rgb ? bg_rgb[0] : 0.0f, b1 = bg_rgb ? bg_rgb[1] : 0.0f, b2 = bg_rgb ? bg_rgb[2] : 0.0f;
    hipLaunchKernelGGL(k_error_map_update, dim3(1), dim3(kUpdateBlock), 0, as_stream(stream), error_map, index, inds_coarse, B, N,
                       n_img, image, weights_sum, gt, b0, b1, b2, bg_rays, depth, gt_depth, depth_weight);
    return check_launch("k_error_map_update");
}

S3D_EXPORT int s3d_orbit_rays(uint32_t B, uint32_t rH, uint32_t rW, const float* intrinsics, const float* look_at, float radius,
                              double theta0, double theta1, double phi0, double phi1, uint32_t seed, int32_t* ctl,
                              const float* u_pose, float* poses_out, float* rays_o, float* rays_d, s3d_stream_t stream) {
    if (B == 0 || rH == 0 || rW == 0) return S3D_OK;
    S3D_REQUIRE(intrinsics && rays_o && rays_d, "s3d_orbit_rays: null argument");
    S3D_REQUIRE(ctl || u_pose, "s3d_orbit_rays: needs ctl or the explicit uniforms u_pose");
    S3D_REQUIRE(((reinterpret_cast<uintptr_t>(rays_o) | reinterpret_cast<uintptr_t>(rays_d)) & 15u) == 0,
                "s3d_orbit_rays: rays_o and rays_d must be 16-byte aligned");
    S3D_REQUIRE(std::isfinite(radius) && std::isfinite(theta0) && std::isfinite(theta1) && std::isfinite(phi0) && std::isfinite(phi1),
                "s3d_orbit_rays: radius and the angle ranges must be finite");
    S3D_REQUIRE((uint64_t)rH * rW * 3 < (1ull << 32), "s3d_orbit_rays: frame too large");
    OrbitArgs a;
    a.u_pose = u_pose; a.ctl = u_pose ? nullptr : ctl;  // (explicit uniforms leave ctl alone)
    a.poses_out = poses_out; a.rays_o = rays_o; a.rays_d = rays_d;
    a.W = rW; a.HW = rH * rW; a.seed = seed;
    a.fx = intrinsics[0]; a.fy = intrinsics[1]; a.cx = intrinsics[2]; a.cy = intrinsics[3];
    a.radius = radius;
    a.th_lo = (float)theta0; a.th_span = (float)(theta1 - theta0);  // (torch: the Python difference, rounded once)
    a.ph_lo = (float)phi0; a.ph_span = (float)(phi1 - phi0);
    for (int k = 0; k < 3; k++) a.look[k] = look_at ? look_at[k] : 0.0f;
    // a pose's 3 HW floats touch at most 3 HW / 4 + 2 aligned groups of four
    a.chunks = (uint32_t)std::min<uint64_t>(div_up<uint64_t>(3ull * a.HW / 4 + 2, kOrbitBlock), kOrbitMaxChunks);
    S3D_REQUIRE((uint64_t)B * a.chunks < (1ull << 31), "s3d_orbit_rays: too many poses for one launch");
    hipLaunchKernelGGL(k_orbit_rays, dim3(B * a.chunks), dim3(kOrbitBlock), 0, as_stream(stream), a);
    return check_launch("k_orbit_rays");
}

S3D_EXPORT int s3d_frame_rays(const float* pose, const float* intrinsics, uint32_t rH, uint32_t rW, float* rays_o, float* rays_d,
                              s3d_stream_t stream) {
    if (rH == 0 || rW == 0) return S3D_OK;
    S3D_REQUIRE(pose && intrinsics && rays_o && rays_d, "s3d_frame_rays: null argument");
    S3D_REQUIRE(((reinterpret_cast<uintptr_t>(rays_o) | reinterpret_cast<uintptr_t>(rays_d)) & 15u) == 0,
                "s3d_frame_rays: rays_o and rays_d must be 16-byte aligned");
    S3D_REQUIRE((uint64_t)rH * rW * 3 + 4 < (1ull << 32), "s3d_frame_rays: frame too large");
    FrameArgs a;
    for (int k = 0; k < 12; k++) a.pose[k] = pose[k];
    a.rays_o = rays_o; a.rays_d = rays_d;
    a.W = rW; a.HW = rH * rW;
    a.fx = intrinsics[0]; a.fy = intrinsics[1]; a.cx = intrinsics[2]; a.cy = intrinsics[3];
    hipLaunchKernelGGL(k_frame_rays, dim3(stream_grid((3ull * a.HW + 3) / 4, kOrbitBlock)), dim3(kOrbitBlock), 0, as_stream(stream), a);
    return check_launch("k_frame_rays");
}
