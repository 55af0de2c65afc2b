// hiersample.hip — the sampling path without the occupancy grid (`NeRFRenderer.run`, nerf/renderer.py:125-253 of the reference, and
// `sample_pdf`, :12-46) for gfx950: stratified samples, inverse-CDF upsampling with the depth merge, weights, compositing and
// the compositing's backward.  S = num_steps, U = upsample_steps, K = S + U.
//
// One wave64 per ray, several rays per workgroup.  Lane l serves the samples l, l + 64, ... of its ray (coalesced rows); a
// scan over a ray is a shuffle ladder per 64 samples with a carry from chunk to chunk.  A workgroup's waves never exchange data;
// the kernels that use LDS keep every loop bound workgroup-uniform and let a wave without a ray repeat the last ray without
// storing, so that __syncthreads() is reached by all.  No atomics: every output element has one writer.
//
// The `order` trick: the merged row is sorted by depth only as (z_sorted, order); sigma, rgb, weights, mask and the gradients stay
// in the concatenated [coarse | fine] order in which the networks produced and consume them.  Sorted slot p reads and writes
// column order[p].
#include "s3d_common.hpp"
#include <math.h>

namespace s3d {
namespace {

constexpr uint32_t kHierCap = 2048;    // K, and the bitonic network's width
constexpr uint32_t kHierRays = 4;      // rays (waves) per workgroup, fewer where the LDS rows are long
constexpr uint32_t kHierLds = 65536;   // static + dynamic LDS a workgroup gets without an opt-in

template <bool Mul>
__device__ __forceinline__ float wave_incl(float v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v = Mul ? v * o : v + o;
    }
    return v;
}
// inclusive suffix sum: lane l gets v[l] + ... + v[63]
__device__ __forceinline__ float wave_suffix(float v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_down(v, d, 64);
        if (lane + (uint32_t)d < 64u) v = v + o;
    }
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// torch.clamp / torch.min(torch.max(.)) keep a NaN; fminf / fmaxf would drop it
__device__ __forceinline__ float clamp_keep_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// torch.linspace(start, end, steps)[i] (RangeFactories: step = (end - start) / (steps - 1), counted from the nearer end).  Torch's
// own kernels contract `start + step * i` and `end - step * k` into one fused multiply-add each, on the device and on the host, so
// the fused form is the one that reproduces its values bit for bit.
__device__ __forceinline__ float linspace_at(float start, float end, uint32_t steps, uint32_t i) {
    if (steps == 1) return start;
    const float step = (end - start) / (float)(steps - 1);
    return i < steps / 2 ? __builtin_fmaf(step, (float)i, start) : __builtin_fmaf(-step, (float)(steps - 1 - i), end);
}

// `(fars - nears) / num_steps` as torch's device kernel forms a division by a host scalar: times the rounded reciprocal
__device__ __forceinline__ float sample_dist_of(float span, uint32_t S) { return span * (1.0f / (float)S); }

// depth and column as one sortable word: the float's bits in an order-preserving unsigned form (a NaN sorts behind +inf, as
// torch.sort places it) above the column, which breaks ties (coarse before fine) and makes the order total
__device__ __forceinline__ uint64_t sort_word(float z, uint32_t col) {
    const uint32_t b = __float_as_uint(z);
    const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)k << 32) | col;
}
__device__ __forceinline__ float sort_word_z(uint64_t w) {
    const uint32_t k = (uint32_t)(w >> 32);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// alpha, the factor s = 1 - alpha + 1e-15 and exp(-delta scale sigma) of one sample (nerf/renderer.py:176-178 / :207-209)
struct Alpha { float alpha, s, e; };
__device__ __forceinline__ Alpha alpha_of(float delta, float scale, float sigma) {
    Alpha a;
    a.e = expf(-delta * scale * sigma);
    a.alpha = 1.0f - a.e;
    a.s = (1.0f - a.alpha) + 1e-15f;
    return a;
}

// one 64-sample chunk of T = exclusive product of s: returns this lane's T and advances the carry
__device__ __forceinline__ float transmittance(float s, float& carry, uint32_t lane) {
    const float incl = wave_incl<true>(s, lane);
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 1.0f;
    const float T = carry * excl;
    carry = carry * __shfl(incl, 63, 64);
    return T;
}

// ---- (a) stratified samples ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kHierRays * 64) k_hier_coarse(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                                const float* __restrict__ aabb, uint32_t N, float min_near, uint32_t S,
                                                                const float* __restrict__ noise, float* __restrict__ nears,
                                                                float* __restrict__ fars, float* __restrict__ z, float* __restrict__ xyz) {
    const uint32_t lane = threadIdx.x & 63u, n = blockIdx.x * kHierRays + (threadIdx.x >> 6);
    if (n >= N) return;
    const float a[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
    float near, far;
    near_far_of(rays_o, rays_d, n, a, min_near, near, far);
    if (lane == 0) { nears[n] = near; fars[n] = far; }
    const float o[3] = {rays_o[n * 3], rays_o[n * 3 + 1], rays_o[n * 3 + 2]};
    const float d[3] = {rays_d[n * 3], rays_d[n * 3 + 1], rays_d[n * 3 + 2]};
    const float span = far - near, sample_dist = sample_dist_of(span, S);
    const size_t row = (size_t)n * S;
    for (uint32_t i = lane; i < S; i += 64) {
        float zi = near + span * linspace_at(0.0f, 1.0f, S, i);
        if (noise) zi = zi + (noise[row + i] - 0.5f) * sample_dist;
        z[row + i] = zi;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) xyz[(row + i) * 3 + c] = clamp_keep_nan(o[c] + d[c] * zi, a[c], a[3 + c]);
    }
}

// ---- (b) inverse-CDF upsampling and the depth merge ------------------------------------------------------------------------
struct UpsampleArgs {
    const float *z, *sigma, *nears, *fars, *u, *rays_o, *rays_d, *aabb;
    float *new_z, *new_xyz, *z_sorted;
    int32_t* order;
    uint32_t N, S, U, P;  // P: K rounded up to a power of two
    float scale, u_first, u_last;
};

// LDS of one ray: words[P] (8 bytes each), cdf[S], zmid[S]
__host__ __device__ inline size_t upsample_ray_bytes(uint32_t S, uint32_t P) { return (size_t)P * 8 + (size_t)S * 8; }

__global__ void __launch_bounds__(kHierRays * 64) k_hier_upsample(UpsampleArgs a) {
    extern __shared__ __align__(16) unsigned char hier_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ray = blockIdx.x * (blockDim.x >> 6) + wave;
    const bool live = ray < a.N;
    const uint32_t n = live ? ray : a.N - 1;  // (a wave without a ray repeats the last one and stores nothing)
    const uint32_t S = a.S, U = a.U, K = S + U, P = a.P;
    uint64_t* words = reinterpret_cast<uint64_t*>(hier_lds + wave * upsample_ray_bytes(S, P));
    float* cdf = reinterpret_cast<float*>(words + P);
    float* zmid = cdf + S;

    const float near = a.nears[n], far = a.fars[n];
    const float sample_dist = sample_dist_of(far - near, S);
    const float* zr = a.z + (size_t)n * S;
    const float* sr = a.sigma + (size_t)n * S;

    // coarse weights (cdf[i] holds w_i for now), bin midpoints, and the coarse half of the sort row
    float carry = 1.0f;
    for (uint32_t base = 0; base < S; base += 64) {
        const uint32_t i = base + lane;
        const bool in = i < S;
        const float zi = in ? zr[i] : 0.0f;
        const float delta = (i + 1 < S) ? zr[i + 1] - zi : sample_dist;
        const Alpha al = alpha_of(delta, a.scale, in ? sr[i] : 0.0f);
        const float T = transmittance(in ? al.s : 1.0f, carry, lane);
        if (in) {
            cdf[i] = al.alpha * T;
            if (i + 1 < S) zmid[i] = zi + 0.5f * delta;
            words[i] = sort_word(zi, i);
        }
    }
    __syncthreads();

    // pdf over the inner weights w[1 .. S-2] and its running sum with a leading zero: cdf[0 .. S-2]
    float part = 0.0f;
    for (uint32_t i = 1 + lane; i + 1 < S; i += 64) part += cdf[i] + 1e-5f;
    const float total = wave_sum(part);
    float run = 0.0f;
    for (uint32_t base = 0; base < S; base += 64) {
        const uint32_t i = base + lane;
        const float v = (i >= 1 && i + 1 < S) ? (cdf[i] + 1e-5f) / total : 0.0f;
        const float r = run + wave_incl<false>(v, lane);
        run = __shfl(r, 63, 64);
        if (i + 1 < S) cdf[i] = r;  // (own slot: read above by this lane only)
    }
    __syncthreads();

    const float aabb[6] = {a.aabb[0], a.aabb[1], a.aabb[2], a.aabb[3], a.aabb[4], a.aabb[5]};
    const float o[3] = {a.rays_o[n * 3], a.rays_o[n * 3 + 1], a.rays_o[n * 3 + 2]};
    const float d[3] = {a.rays_d[n * 3], a.rays_d[n * 3 + 1], a.rays_d[n * 3 + 2]};
    const uint32_t bins = S - 1;  // entries of cdf and zmid
    for (uint32_t j = lane; j < U; j += 64) {
        const float uj = a.u ? a.u[(size_t)n * U + j] : linspace_at(a.u_first, a.u_last, U, j);
        uint32_t lo = 0, hi = bins;  // searchsorted(right=True): the first entry above u
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cdf[mid] <= uj) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t below = lo >= 1 ? lo - 1 : 0, above = lo < bins - 1 ? lo : bins - 1;
        const float cb = cdf[below], ca = cdf[above];
        float denom = ca - cb;
        if (denom < 1e-5f) denom = 1.0f;
        const float t = (uj - cb) / denom;
        const float zb = zmid[below];
        const float nz = zb + t * (zmid[above] - zb);
        words[S + j] = sort_word(nz, S + j);
        if (live) {
            const size_t at = (size_t)n * U + j;
            a.new_z[at] = nz;
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) a.new_xyz[at * 3 + c] = clamp_keep_nan(o[c] + d[c] * nz, aabb[c], aabb[3 + c]);
        }
    }
    for (uint32_t i = K + lane; i < P; i += 64) words[i] = ((uint64_t)0xFFFFFFFFu << 32) | i;  // padding: behind every sample
    __syncthreads();

    // bitonic network over the P words of this wave's row
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < P / 2; t += 64) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const uint64_t x = words[i], y = words[p];
                if ((x > y) == ((i & k) == 0)) { words[i] = y; words[p] = x; }
            }
            __syncthreads();
        }
    }
    if (live) {
        for (uint32_t i = lane; i < K; i += 64) {
            const uint64_t w = words[i];
            a.z_sorted[(size_t)n * K + i] = sort_word_z(w);
            a.order[(size_t)n * K + i] = (int32_t)(uint32_t)w;
        }
    }
}

// ---- (c) weights of the merged row ----------------------------------------------------------------------------------------
// column of sorted slot p (identity without `order`); a column outside the row is folded into it, so a bad `order` cannot fault
__device__ __forceinline__ uint32_t column_of(const int32_t* __restrict__ order, size_t row, uint32_t p, uint32_t K) {
    if (!order) return p;
    const uint32_t i = (uint32_t)order[row + p];
    return i < K ? i : K - 1;
}

__global__ void __launch_bounds__(kHierRays * 64) k_hier_weights(const float* __restrict__ z_sorted, const int32_t* __restrict__ order,
                                                                 const float* __restrict__ sigma_cat, const float* __restrict__ nears,
                                                                 const float* __restrict__ fars, float scale, uint32_t N, uint32_t S,
                                                                 uint32_t K, float* __restrict__ weights, uint8_t* __restrict__ mask) {
    const uint32_t lane = threadIdx.x & 63u, n = blockIdx.x * kHierRays + (threadIdx.x >> 6);
    if (n >= N) return;
    const float sample_dist = sample_dist_of(fars[n] - nears[n], S);
    const size_t row = (size_t)n * K;
    float carry = 1.0f;
    for (uint32_t base = 0; base < K; base += 64) {
        const uint32_t p = base + lane;
        const bool in = p < K;
        const uint32_t i = in ? column_of(order, row, p, K) : 0;
        const float zi = in ? z_sorted[row + p] : 0.0f;
        const float delta = (p + 1 < K) ? z_sorted[row + p + 1] - zi : sample_dist;
        const Alpha al = alpha_of(delta, scale, in ? sigma_cat[row + i] : 0.0f);
        const float T = transmittance(in ? al.s : 1.0f, carry, lane);
        if (in) {
            const float w = al.alpha * T;
            weights[row + i] = w;
            mask[row + i] = w > 1e-4f ? 1 : 0;
        }
    }
}

// ---- (d) compositing ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kHierRays * 64) k_hier_composite(const float* __restrict__ weights, const float* __restrict__ rgbs,
                                                                   const float* __restrict__ z_sorted, const int32_t* __restrict__ order,
                                                                   const float* __restrict__ nears, const float* __restrict__ fars,
                                                                   uint32_t N, uint32_t K, float* __restrict__ weights_sum,
                                                                   float* __restrict__ depth, float* __restrict__ image) {
    const uint32_t lane = threadIdx.x & 63u, n = blockIdx.x * kHierRays + (threadIdx.x >> 6);
    if (n >= N) return;
    const float near = nears[n], span = fars[n] - near;
    const size_t row = (size_t)n * K;
    float ws = 0.0f, dp = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    for (uint32_t p = lane; p < K; p += 64) {
        const uint32_t i = column_of(order, row, p, K);
        const float w = weights[row + i];
        const float zn = clamp_keep_nan((z_sorted[row + p] - near) / span, 0.0f, 1.0f);  // a miss: 0 / 0 stays NaN (:224-225)
        ws += w;
        dp += w * zn;
        c0 += w * rgbs[(row + i) * 3];
        c1 += w * rgbs[(row + i) * 3 + 1];
        c2 += w * rgbs[(row + i) * 3 + 2];
    }
    ws = wave_sum(ws); dp = wave_sum(dp); c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
    if (lane == 0) {
        weights_sum[n] = ws;
        depth[n] = dp;
        image[n * 3] = c0; image[n * 3 + 1] = c1; image[n * 3 + 2] = c2;
    }
}

// Backward.  With s_p = 1 - a_p + 1e-15, T_p = prod_{q<p} s_q, w_p = a_p T_p and G_p = g_img . rgb_p + g_ws + g_depth znorm_p the
// loss reaches a_p through w_p itself (G_p T_p) and through the factor s_p of every later weight (- sum_{q>p} G_q w_q / s_p);
// d a_p / d sigma = delta_p scale exp(-delta_p scale sigma_p).  The suffix sum is a suffix scan from the far end, not
// "total - prefix": behind an opaque sample the terms are many orders below the total, and they are divided by an s down to 1e-15.
// LDS of one ray: T[K], G[K], Gw[K], each slot written and read by the same lane.
__host__ __device__ inline size_t backward_ray_bytes(uint32_t K) { return (size_t)K * 12; }

struct BackwardArgs {
    const float *grad_image, *grad_weights_sum, *grad_depth, *sigma_cat, *rgbs, *z_sorted, *nears, *fars;
    const int32_t* order;
    float *grad_sigma, *grad_rgbs;
    uint32_t N, S, K;
    float scale;
};

__global__ void __launch_bounds__(kHierRays * 64) k_hier_composite_backward(BackwardArgs a) {
    extern __shared__ __align__(16) unsigned char hier_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n = blockIdx.x * (blockDim.x >> 6) + wave;
    if (n >= a.N) return;  // (no workgroup barrier below)
    const uint32_t K = a.K;
    float* Tb = reinterpret_cast<float*>(hier_lds + wave * backward_ray_bytes(K));
    float* Gb = Tb + K;
    float* Xb = Gb + K;
    const float near = a.nears[n], span = a.fars[n] - near;
    const float sample_dist = sample_dist_of(span, a.S);
    const size_t row = (size_t)n * K;
    const float* zr = a.z_sorted + row;
    const float gi[3] = {a.grad_image ? a.grad_image[n * 3] : 0.0f, a.grad_image ? a.grad_image[n * 3 + 1] : 0.0f,
                         a.grad_image ? a.grad_image[n * 3 + 2] : 0.0f};
    const float gws = a.grad_weights_sum ? a.grad_weights_sum[n] : 0.0f;
    const float gd = a.grad_depth ? a.grad_depth[n] : 0.0f;

    float carry = 1.0f;
    for (uint32_t base = 0; base < K; base += 64) {
        const uint32_t p = base + lane;
        const bool in = p < K;
        const uint32_t i = in ? column_of(a.order, row, p, K) : 0;
        const float zi = in ? zr[p] : 0.0f;
        const float delta = (p + 1 < K) ? zr[p + 1] - zi : sample_dist;
        const Alpha al = alpha_of(delta, a.scale, in ? a.sigma_cat[row + i] : 0.0f);
        const float T = transmittance(in ? al.s : 1.0f, carry, lane);
        if (in) {
            const float w = al.alpha * T;
            const float* c = a.rgbs + (row + i) * 3;
            float G = (gi[0] * c[0] + gi[1] * c[1]) + gi[2] * c[2] + gws;
            if (a.grad_depth) G += gd * clamp_keep_nan((zi - near) / span, 0.0f, 1.0f);  // (no 0 * NaN where depth has no gradient)
            float* g = a.grad_rgbs + (row + i) * 3;
            g[0] = w * gi[0]; g[1] = w * gi[1]; g[2] = w * gi[2];
            Tb[p] = T; Gb[p] = G; Xb[p] = G * w;
        }
    }
    float behind = 0.0f;  // sum of G w over the chunks behind this one
    for (uint32_t base = (K - 1) / 64 * 64;; base -= 64) {
        const uint32_t p = base + lane;
        const bool in = p < K;
        const float incl = wave_suffix(in ? Xb[p] : 0.0f, lane);
        float later = __shfl_down(incl, 1, 64);
        if (lane == 63) later = 0.0f;
        later += behind;
        behind += __shfl(incl, 0, 64);
        if (in) {
            const uint32_t i = column_of(a.order, row, p, K);
            const float delta = (p + 1 < K) ? zr[p + 1] - zr[p] : sample_dist;
            const Alpha al = alpha_of(delta, a.scale, a.sigma_cat[row + i]);
            a.grad_sigma[row + i] = delta * a.scale * al.e * (Gb[p] * Tb[p] - later / al.s);
        }
        if (base == 0) break;
    }
}

inline uint32_t pow2_at_least(uint32_t v) {
    uint32_t p = 2;
    while (p < v) p <<= 1;
    return p;
}
inline uint32_t rays_per_block(size_t ray_bytes) {
    const size_t fit = ray_bytes ? kHierLds / ray_bytes : kHierRays;
    return (uint32_t)(fit < kHierRays ? fit : kHierRays);
}

}  // namespace
}  // namespace s3d

using namespace s3d;

#define HIER_SHAPE(what, S, U)                                                                                                  \
    do {                                                                                                                        \
        S3D_REQUIRE((S) >= 3, what ": num_steps must be at least 3");                                                           \
        if ((uint64_t)(S) + (U) > kHierCap) {                                                                                   \
            s3d::set_error(what ": num_steps + upsample_steps = %llu exceeds %u", (unsigned long long)(S) + (U), kHierCap);    \
            return S3D_ERR_UNSUPPORTED;                                                                                         \
        }                                                                                                                       \
    } while (0)

S3D_EXPORT int s3d_hier_max_samples(void) { return (int)kHierCap; }

S3D_EXPORT int s3d_hier_coarse_samples(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near,
                                       uint32_t S, const float* noise, float* nears, float* fars, float* z, float* xyz,
                                       s3d_stream_t stream) {
    HIER_SHAPE("hier_coarse_samples", S, 0u);
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(rays_o && rays_d && aabb && nears && fars && z && xyz, "hier_coarse_samples: null pointer");
    S3D_REQUIRE(N <= (1u << 30), "hier_coarse_samples: at most 2^30 rays");
    hipLaunchKernelGGL(k_hier_coarse, dim3(div_up<uint32_t>(N, kHierRays)), dim3(kHierRays * 64), 0, as_stream(stream), rays_o, rays_d,
                       aabb, N, min_near, S, noise, nears, fars, z, xyz);
    return check_launch("hier_coarse_samples");
}

S3D_EXPORT int s3d_hier_upsample(const float* z, const float* sigma, const float* nears, const float* fars, float density_scale,
                                 const float* u, const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, uint32_t S,
                                 uint32_t U, float* new_z, float* new_xyz, float* z_sorted, int32_t* order, s3d_stream_t stream) {
    HIER_SHAPE("hier_upsample", S, U);
    S3D_REQUIRE(U >= 1, "hier_upsample: upsample_steps must be at least 1 (none: skip the call, the order is the identity)");
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(z && sigma && nears && fars && rays_o && rays_d && aabb && new_z && new_xyz && z_sorted && order,
                "hier_upsample: null pointer");
    S3D_REQUIRE(N <= (1u << 30), "hier_upsample: at most 2^30 rays");
    UpsampleArgs a{z, sigma, nears, fars, u, rays_o, rays_d, aabb, new_z, new_xyz, z_sorted, order, N, S, U, pow2_at_least(S + U),
                   density_scale, (float)(0.5 / (double)U), (float)(1.0 - 0.5 / (double)U)};
    const size_t ray_bytes = upsample_ray_bytes(S, a.P);
    const uint32_t rays = rays_per_block(ray_bytes);  // >= 2 at the cap: 2048 * 8 + 2047 * 8 bytes
    hipLaunchKernelGGL(k_hier_upsample, dim3(div_up<uint32_t>(N, rays)), dim3(rays * 64), rays * ray_bytes, as_stream(stream), a);
    return check_launch("hier_upsample");
}

S3D_EXPORT int s3d_hier_weights(const float* z_sorted, const int32_t* order, const float* sigma_cat, const float* nears,
                                const float* fars, float density_scale, uint32_t N, uint32_t S, uint32_t U, float* weights,
                                uint8_t* mask, s3d_stream_t stream) {
    HIER_SHAPE("hier_weights", S, U);
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(z_sorted && sigma_cat && nears && fars && weights && mask, "hier_weights: null pointer");
    S3D_REQUIRE(order || U == 0, "hier_weights: order may be omitted (the identity) only without upsampling");
    S3D_REQUIRE(N <= (1u << 30), "hier_weights: at most 2^30 rays");
    hipLaunchKernelGGL(k_hier_weights, dim3(div_up<uint32_t>(N, kHierRays)), dim3(kHierRays * 64), 0, as_stream(stream), z_sorted, order,
                       sigma_cat, nears, fars, density_scale, N, S, S + U, weights, mask);
    return check_launch("hier_weights");
}

S3D_EXPORT int s3d_hier_composite_forward(const float* weights, const float* rgbs, const float* z_sorted, const int32_t* order,
                                          const float* nears, const float* fars, uint32_t N, uint32_t S, uint32_t U,
                                          float* weights_sum, float* depth, float* image, s3d_stream_t stream) {
    HIER_SHAPE("hier_composite_forward", S, U);
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(weights && rgbs && z_sorted && nears && fars && weights_sum && depth && image, "hier_composite_forward: null pointer");
    S3D_REQUIRE(order || U == 0, "hier_composite_forward: order may be omitted (the identity) only without upsampling");
    S3D_REQUIRE(N <= (1u << 30), "hier_composite_forward: at most 2^30 rays");
    hipLaunchKernelGGL(k_hier_composite, dim3(div_up<uint32_t>(N, kHierRays)), dim3(kHierRays * 64), 0, as_stream(stream), weights, rgbs,
                       z_sorted, order, nears, fars, N, S + U, weights_sum, depth, image);
    return check_launch("hier_composite_forward");
}

S3D_EXPORT int s3d_hier_composite_backward(const float* grad_image, const float* grad_weights_sum, const float* grad_depth,
                                           const float* sigma_cat, const float* rgbs, const float* z_sorted, const int32_t* order,
                                           const float* nears, const float* fars, float density_scale, uint32_t N, uint32_t S,
                                           uint32_t U, float* grad_sigma_cat, float* grad_rgbs, s3d_stream_t stream) {
    HIER_SHAPE("hier_composite_backward", S, U);
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(sigma_cat && rgbs && z_sorted && nears && fars && grad_sigma_cat && grad_rgbs, "hier_composite_backward: null pointer");
    S3D_REQUIRE(order || U == 0, "hier_composite_backward: order may be omitted (the identity) only without upsampling");
    S3D_REQUIRE(N <= (1u << 30), "hier_composite_backward: at most 2^30 rays");
    BackwardArgs a{grad_image, grad_weights_sum, grad_depth, sigma_cat, rgbs, z_sorted, nears, fars, order, grad_sigma_cat, grad_rgbs,
                   N, S, S + U, density_scale};
    const size_t ray_bytes = backward_ray_bytes(a.K);
    const uint32_t rays = rays_per_block(ray_bytes);  // >= 2 at the cap: 2048 * 12 bytes
    hipLaunchKernelGGL(k_hier_composite_backward, dim3(div_up<uint32_t>(N, rays)), dim3(rays * 64), rays * ray_bytes, as_stream(stream),
                       a);
    return check_launch("hier_composite_backward");
}
