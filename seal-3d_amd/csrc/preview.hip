// preview.hip — the tail of an interactive preview frame (nerf/utils.py:782-799 `test_gui`, SealNeRF/gui.py:219-289
// `prepare_buffer`, :355-362 the accumulation of `test_step`, :300-306 `get_mask_pos`) for gfx950.  The frame stays on the
// device; the reference upsamples with two permutes around F.interpolate, copies to the host, overlays and accumulates in numpy.
//
//  * s3d_preview_resolve: one pass over the H x W destination.  A work item is one 16-byte aligned group of four consecutive
//    destination pixels of the flat frame (adjacent pixels of a row; a group may run over a row's end when W is no multiple of
//    four): per output one float4 store for the depth, three for each of the three-channel arrays, one 32-bit load per mask.
//    Only the last group of a frame whose H W is no multiple of four stores pixel by pixel.  The source pixel of each
//    destination pixel is torch's nearest rule, min((int)floorf(dst * fl(in / out)), in - 1) per axis: a gather from the small
//    rendered frame.  Everything else is one individually rounded fp32 operation per reference operation (the library is built
//    with -ffp-contract=off), so the results are the torch / numpy sequence's bit for bit — except the sRGB power, powf.
//    Depth mode divides by max(depth) + 1e-6 over the destination frame: a first launch takes that maximum with the resolve's own
//    gather (reads of the cached source, no stores), as an atomicMax on an order-preserving integer key of the float — any
//    order gives the same bits.
//  * s3d_mask_positions_count / s3d_mask_positions_emit: rows of pos [H W, 3] where mask k is non-zero, for K masks, in mask
//    then row-major pixel order.  The shape of k_mc_count / k_mc_scan / k_mc_emit (mesh.hip): workgroups of 1,024 threads x 4
//    pixels inside one mask count, one workgroup scans the workgroup sums and writes offsets [K + 1], the emit launch repeats
//    the in-workgroup scan and writes each row at its final place.  No atomics: the order is fixed.
#include "s3d_common.hpp"

#include <math.h>

namespace s3d {
namespace {

constexpr uint32_t kResolveBlock = 256;
constexpr float kFltMax = 3.402823466e+38f;

// torch.nan_to_num's defaults: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float clean_depth(float d) {
    return d != d ? 0.0f : fminf(fmaxf(d, -kFltMax), kFltMax);
}

// F.interpolate(mode='nearest'): source index of destination index `dst` (scale = fl((float)in / (float)out))
__device__ __forceinline__ uint32_t nearest_src(uint32_t dst, float scale, uint32_t in) {
    const uint32_t s = (uint32_t)(int)floorf((float)dst * scale);
    return s < in - 1u ? s : in - 1u;
}

// order-preserving key of a float that is not NaN: a < b  <=>  key(a) < key(b); key > 0 for every float
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// maximum of the cleaned depth over the destination frame -> *key (cleared before the launch): the same gather the resolve
// launch does, so a source pixel the upsampling never reads cannot count
__global__ void __launch_bounds__(kResolveBlock)
k_preview_depth_max(const float* __restrict__ depth, uint32_t rH, uint32_t rW, uint32_t H, uint32_t W, float sh, float sw,
                    uint32_t* __restrict__ key) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    uint32_t best = 0u;
    const uint32_t n = H * W;
    for (uint32_t p = blockIdx.x * kResolveBlock + threadIdx.x; p < n; p += gridDim.x * kResolveBlock) {
        const uint32_t y = p / W, x = p - y * W;
        const uint32_t k = float_key(clean_depth(depth[nearest_src(y, sh, rH) * rW + nearest_src(x, sw, rW)]));
        best = k > best ? k : best;
    }
    if (best) atomicMax(&s_max, best);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(key, s_max);
}

struct ResolveArgs {
    const float* image;    // [rH, rW, 3]
    const float* depth;    // [rH, rW]
    const float* rays_o;   // [H W, 3] or NULL (with pos)
    const float* rays_d;
    const uint8_t* masks;  // [K, H, W] or NULL
    const uint32_t* dmax;  // key of the depth maximum (depth mode)
    float* frame_image;    // [H, W, 3] or NULL (the caller keeps `image`: no upsampling, no conversion)
    float* frame_depth;    // [H, W]
    float* pos;            // [H, W, 3] or NULL
    float* buffer;         // [H, W, 3] or NULL
    uint32_t H, W, rH, rW, K, srgb, depth_mode, spp;
    float sh, sw;
    float color_a[3];      // fl(color * fl(alpha))
    float inv_alpha;       // fl(1 - alpha), the difference formed in double
};

// one destination pixel: frame colour and depth, position, and the value the display buffer takes
__device__ __forceinline__ void resolve_pixel(const ResolveArgs& a, uint32_t p, uint32_t K, float div, float rgb[3], float& d, float ps[3],
                                              float buf[3]) {
    const uint32_t y = p / a.W, x = p - y * a.W;
    const uint32_t s = nearest_src(y, a.sh, a.rH) * a.rW + nearest_src(x, a.sw, a.rW);
    d = clean_depth(a.depth[s]);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = a.image[(size_t)s * 3 + c];
        if (a.srgb) v = v < 0.0031308f ? 12.92f * v : 1.055f * powf(v, 0.41666f) - 0.055f;
        rgb[c] = v;
    }
    if (a.pos) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float t = d * a.rays_d[(size_t)p * 3 + c];  // (a product and a sum, two roundings: torch's)
            ps[c] = a.rays_o[(size_t)p * 3 + c] + t;
        }
    }
    if (!a.buffer) return;
    bool painted = false;
    for (uint32_t k = 0; k < K; k++) painted = painted || a.masks[(size_t)k * a.H * a.W + p] != 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = a.depth_mode ? d / div : rgb[c];
        if (painted) {
            const float keep = v * a.inv_alpha;
            v = a.color_a[c] + keep;
        }
        if (a.spp) {
            const float acc = buf[c] * (float)a.spp;
            v = (acc + v) / (float)(a.spp + 1u);
        }
        buf[c] = v;
    }
}

__global__ void __launch_bounds__(kResolveBlock) k_preview_resolve(ResolveArgs a) {
    const uint32_t n = a.H * a.W, groups = (n + 3u) >> 2;
    // depth mode: the divisor max + 1e-6 (an fp32 sum), the same for every pixel
    const float div = a.depth_mode ? key_float(*a.dmax) + 1e-6f : 1.0f;
    for (uint32_t g = blockIdx.x * kResolveBlock + threadIdx.x; g < groups; g += gridDim.x * kResolveBlock) {
        const uint32_t p0 = g << 2;
        const bool whole = p0 + 4u <= n;
        float rgb[12], d[4], ps[12], buf[12];
        if (a.buffer && a.spp) {
            if (whole) {
                const float4* b4 = reinterpret_cast<const float4*>(a.buffer + (size_t)p0 * 3);
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const float4 v = b4[q];
                    buf[q * 4] = v.x; buf[q * 4 + 1] = v.y; buf[q * 4 + 2] = v.z; buf[q * 4 + 3] = v.w;
                }
            } else {
                for (uint32_t e = 0; e < 12u; e++) buf[e] = p0 * 3u + e < n * 3u ? a.buffer[(size_t)p0 * 3 + e] : 0.0f;
            }
        }
        // masks of a whole group: one 32-bit load per mask says whether any of the four pixels is painted at all
        uint32_t any_mask = 0u;
        if (a.buffer && a.K) {
            if (whole && (n & 3u) == 0u) {
                for (uint32_t k = 0; k < a.K; k++) any_mask |= *reinterpret_cast<const uint32_t*>(a.masks + (size_t)k * n + p0);
            } else {
                any_mask = 1u;
            }
        }
        const uint32_t K = any_mask ? a.K : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            const uint32_t p = p0 + j < n ? p0 + j : n - 1u;
            resolve_pixel(a, p, K, div, rgb + 3 * j, d[j], ps + 3 * j, buf + 3 * j);
        }
        if (whole) {
            *reinterpret_cast<float4*>(a.frame_depth + p0) = make_float4(d[0], d[1], d[2], d[3]);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                if (a.frame_image) reinterpret_cast<float4*>(a.frame_image + (size_t)p0 * 3)[q] = make_float4(rgb[q * 4], rgb[q * 4 + 1], rgb[q * 4 + 2], rgb[q * 4 + 3]);
                if (a.pos) reinterpret_cast<float4*>(a.pos + (size_t)p0 * 3)[q] = make_float4(ps[q * 4], ps[q * 4 + 1], ps[q * 4 + 2], ps[q * 4 + 3]);
                if (a.buffer) reinterpret_cast<float4*>(a.buffer + (size_t)p0 * 3)[q] = make_float4(buf[q * 4], buf[q * 4 + 1], buf[q * 4 + 2], buf[q * 4 + 3]);
            }
        } else {
            for (uint32_t j = 0; p0 + j < n; j++) {
                a.frame_depth[p0 + j] = d[j];
                for (uint32_t c = 0; c < 3u; c++) {
                    const size_t o = (size_t)(p0 + j) * 3 + c;
                    if (a.frame_image) a.frame_image[o] = rgb[3 * j + c];
                    if (a.pos) a.pos[o] = ps[3 * j + c];
                    if (a.buffer) a.buffer[o] = buf[3 * j + c];
                }
            }
        }
    }
}

// ---- mask positions ----

constexpr uint32_t kMaskBlock = 1024;                 // threads per workgroup
constexpr uint32_t kMaskPer = 4;                      // pixels per thread
constexpr uint32_t kMaskTile = kMaskBlock * kMaskPer;  // pixels per workgroup, all of one mask

// exclusive prefix of `mine` over the 1,024 threads of the workgroup and the workgroup's sum; sh holds 16 words
__device__ __forceinline__ uint32_t mask_block_scan(uint32_t mine, uint32_t* sh, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(mine);
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kMaskBlock / 64; ++w) {
        const uint32_t s = sh[w];
        if (w < wave) base += s;
        sum += s;
    }
    __syncthreads();
    *total = sum;
    return base + incl - mine;
}

// which of this thread's four pixels of mask k are painted (bit j: pixel first + j); workgroup `tile` of the mask
__device__ __forceinline__ uint32_t mask_bits(const uint8_t* __restrict__ masks, uint32_t k, uint32_t tile, uint32_t n, uint32_t* first) {
    const uint32_t p0 = tile * kMaskTile + threadIdx.x * kMaskPer;
    *first = p0;
    const uint8_t* m = masks + (size_t)k * n;
    uint32_t bits = 0u;
    if ((n & 3u) == 0u && p0 + kMaskPer <= n) {  // (n a multiple of four: every mask starts on a 4-byte boundary)
        const uint32_t w = *reinterpret_cast<const uint32_t*>(m + p0);
#pragma unroll
        for (uint32_t j = 0; j < kMaskPer; j++) bits |= ((w >> (8u * j)) & 255u) ? 1u << j : 0u;
    } else {
        for (uint32_t j = 0; j < kMaskPer && p0 + j < n; j++) bits |= m[p0 + j] ? 1u << j : 0u;
    }
    return bits;
}

__global__ void __launch_bounds__(kMaskBlock) k_mask_count(const uint8_t* __restrict__ masks, uint32_t n, uint32_t tiles,
                                                           uint32_t* __restrict__ bsum) {
    __shared__ uint32_t sh[kMaskBlock / 64];
    uint32_t first, total;
    const uint32_t bits = mask_bits(masks, blockIdx.x / tiles, blockIdx.x % tiles, n, &first);
    mask_block_scan(__popc(bits), sh, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the nb = K tiles workgroup sums in place; offsets[k] = rows before mask k, offsets[K] = all
__global__ void __launch_bounds__(kMaskBlock) k_mask_scan(uint32_t* __restrict__ bsum, uint32_t nb, uint32_t tiles, uint32_t K,
                                                          int64_t* __restrict__ offsets) {
    __shared__ uint32_t sh[kMaskBlock / 64];
    uint64_t carry = 0;  // (K H W < 2^32 is checked on the host: the sum fits 32 bits)
    for (uint32_t b0 = 0; b0 < nb; b0 += kMaskBlock) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t mine = b < nb ? bsum[b] : 0u;
        uint32_t total;
        const uint32_t pre = (uint32_t)carry + mask_block_scan(mine, sh, &total);
        if (b < nb) {
            bsum[b] = pre;
            if (b % tiles == 0u) offsets[b / tiles] = (int64_t)pre;
        }
        carry += total;
    }
    if (threadIdx.x == 0) offsets[K] = (int64_t)carry;
}

__global__ void __launch_bounds__(kMaskBlock) k_mask_emit(const uint8_t* __restrict__ masks, uint32_t n, uint32_t tiles,
                                                          const uint32_t* __restrict__ bsum, const float* __restrict__ pos,
                                                          float* __restrict__ out, uint32_t rows) {
    __shared__ uint32_t sh[kMaskBlock / 64];
    uint32_t first, total;
    const uint32_t bits = mask_bits(masks, blockIdx.x / tiles, blockIdx.x % tiles, n, &first);
    uint32_t o = bsum[blockIdx.x] + mask_block_scan(__popc(bits), sh, &total);
#pragma unroll
    for (uint32_t j = 0; j < kMaskPer; j++) {
        if (!(bits >> j & 1u)) continue;
        if (o < rows) {  // (always, when `rows` is the counted total)
            const size_t s = (size_t)(first + j) * 3, d = (size_t)o * 3;
            out[d] = pos[s]; out[d + 1] = pos[s + 1]; out[d + 2] = pos[s + 2];
        }
        ++o;
    }
}

int mask_check(uint32_t K, uint32_t H, uint32_t W, const char* what) {
    S3D_REQUIRE(K > 0 && H > 0 && W > 0, "%s: no mask or an empty frame", what);
    S3D_REQUIRE((uint64_t)H * W * 3 < (1ull << 32) && (uint64_t)K * H * W < (1ull << 32), "%s: %u masks of %u x %u are too large", what, K, H, W);
    S3D_REQUIRE((uint64_t)K * div_up<uint64_t>((uint64_t)H * W, kMaskTile) < (1ull << 31), "%s: too many workgroups", what);
    return S3D_OK;
}

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT int s3d_preview_resolve(const float* image, const float* depth, uint32_t rH, uint32_t rW, uint32_t H, uint32_t W,
                                   int to_srgb, const float* rays_o, const float* rays_d, float* frame_image, float* frame_depth,
                                   float* pos, float* buffer, int depth_mode, const uint8_t* masks, uint32_t K, const float* color,
                                   double alpha, uint32_t spp, uint32_t* workspace, s3d_stream_t stream) {
    if (H == 0 || W == 0) return S3D_OK;
    S3D_REQUIRE(image && depth && frame_depth, "s3d_preview_resolve: null argument");
    S3D_REQUIRE(frame_image || (rH == H && rW == W && !to_srgb), "s3d_preview_resolve: frame_image may be NULL only where it would be a copy of image");
    S3D_REQUIRE(rH > 0 && rW > 0 && rH <= H && rW <= W, "s3d_preview_resolve: the rendered frame %u x %u must fit the displayed %u x %u", rH, rW, H, W);
    S3D_REQUIRE((uint64_t)H * W * 3 < (1ull << 32) && H < (1u << 22) && W < (1u << 22), "s3d_preview_resolve: frame too large");
    S3D_REQUIRE(!pos || (rays_o && rays_d && rH == H && rW == W), "s3d_preview_resolve: pos needs the rays of a frame rendered at full resolution");
    S3D_REQUIRE(K == 0 || (masks && color && buffer), "s3d_preview_resolve: an overlay needs masks, a colour and the display buffer");
    S3D_REQUIRE(!(depth_mode && buffer) || workspace, "s3d_preview_resolve: depth mode needs the 4-byte workspace");
    S3D_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "s3d_preview_resolve: alpha must lie in [0, 1]");
    const uintptr_t al = reinterpret_cast<uintptr_t>(frame_image) | reinterpret_cast<uintptr_t>(frame_depth) |
                         reinterpret_cast<uintptr_t>(pos) | reinterpret_cast<uintptr_t>(buffer);
    S3D_REQUIRE((al & 15u) == 0 && (reinterpret_cast<uintptr_t>(masks) & 3u) == 0, "s3d_preview_resolve: outputs must be 16-byte aligned, masks 4-byte");
    ResolveArgs a;
    a.image = image; a.depth = depth; a.rays_o = pos ? rays_o : nullptr; a.rays_d = pos ? rays_d : nullptr;
    a.masks = K ? masks : nullptr; a.dmax = workspace;
    a.frame_image = frame_image; a.frame_depth = frame_depth; a.pos = pos; a.buffer = buffer;
    a.H = H; a.W = W; a.rH = rH; a.rW = rW; a.K = K; a.srgb = to_srgb != 0; a.depth_mode = (depth_mode != 0 && buffer) ? 1u : 0u; a.spp = spp;
    a.sh = (float)rH / (float)H; a.sw = (float)rW / (float)W;
    const float af = (float)alpha;
    for (int c = 0; c < 3; c++) a.color_a[c] = K ? color[c] * af : 0.0f;
    a.inv_alpha = (float)(1.0 - alpha);
    if (a.depth_mode) {
        S3D_HIP(hipMemsetAsync(workspace, 0, sizeof(uint32_t), as_stream(stream)));
        hipLaunchKernelGGL(k_preview_depth_max, dim3(stream_grid((uint64_t)H * W, kResolveBlock)), dim3(kResolveBlock), 0,
                           as_stream(stream), depth, rH, rW, H, W, a.sh, a.sw, workspace);
    }
    hipLaunchKernelGGL(k_preview_resolve, dim3(stream_grid(((uint64_t)H * W + 3) / 4, kResolveBlock)), dim3(kResolveBlock), 0,
                       as_stream(stream), a);
    return check_launch("k_preview_resolve");
}

S3D_EXPORT size_t s3d_mask_positions_workspace_bytes(uint32_t K, uint32_t H, uint32_t W) {
    if (mask_check(K, H, W, "mask_positions_workspace_bytes") != S3D_OK) return 0;
    return sizeof(uint32_t) * (size_t)K * div_up<uint64_t>((uint64_t)H * W, kMaskTile);
}

S3D_EXPORT int s3d_mask_positions_count(const uint8_t* masks, uint32_t K, uint32_t H, uint32_t W, void* workspace, int64_t* offsets,
                                        s3d_stream_t stream) {
    if (int rc = mask_check(K, H, W, "mask_positions_count")) return rc;
    S3D_REQUIRE(masks && workspace && offsets, "mask_positions_count: null pointer");
    S3D_REQUIRE((reinterpret_cast<uintptr_t>(masks) & 3u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0,
                "mask_positions_count: masks and workspace must be 4-byte aligned");
    const uint32_t n = H * W, tiles = div_up<uint32_t>(n, kMaskTile), nb = K * tiles;
    hipLaunchKernelGGL(k_mask_count, dim3(nb), dim3(kMaskBlock), 0, as_stream(stream), masks, n, tiles, (uint32_t*)workspace);
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(kMaskBlock), 0, as_stream(stream), (uint32_t*)workspace, nb, tiles, K, offsets);
    return check_launch("mask_positions_count");
}

S3D_EXPORT int s3d_mask_positions_emit(const uint8_t* masks, uint32_t K, uint32_t H, uint32_t W, const void* workspace, const float* pos,
                                       float* out, uint32_t rows, s3d_stream_t stream) {
    if (int rc = mask_check(K, H, W, "mask_positions_emit")) return rc;
    S3D_REQUIRE(masks && workspace && pos, "mask_positions_emit: null pointer");
    S3D_REQUIRE((reinterpret_cast<uintptr_t>(masks) & 3u) == 0, "mask_positions_emit: masks must be 4-byte aligned");
    if (rows == 0) return S3D_OK;
    S3D_REQUIRE(out, "mask_positions_emit: null output");
    const uint32_t n = H * W, tiles = div_up<uint32_t>(n, kMaskTile), nb = K * tiles;
    hipLaunchKernelGGL(k_mask_emit, dim3(nb), dim3(kMaskBlock), 0, as_stream(stream), masks, n, tiles, (const uint32_t*)workspace, pos,
                       out, rows);
    return check_launch("mask_positions_emit");
}
