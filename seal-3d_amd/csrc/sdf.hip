// sdf.hip — the SDF backbone's data path (include/seal3d_hip.h "SDF"; DESIGN.md "SDF"): signed distance and winding number of
// points against a triangle mesh (brute force, the triangles staged through LDS), one dataset item's points in one launch, and the
// MAPE criterion with its gradient on the MLP's padded output.  The pair test itself, with its tie and sign rules, is
// csrc/sdf_pair.hpp, shared with the BVH query (csrc/sdf_bvh.hip): this file only tiles the faces and loops over them.
#include "s3d_common.hpp"
#include "sdf_pair.hpp"
#include "ordered_sum.hpp"

namespace s3d {
namespace {

using namespace sdfpair;

constexpr uint32_t kSdfBlock = 256;  // lanes per workgroup = points per workgroup
constexpr uint32_t kSdfTile = 256;   // triangles per LDS tile: one per lane to stage, 20 KiB, 8 workgroups per CU fit in 160 KiB

__global__ void __launch_bounds__(kSdfBlock) mesh_sdf_kernel(const float* __restrict__ points, uint32_t N, const float* __restrict__ triangles,
                                                            uint32_t F, float* __restrict__ sdf, float* __restrict__ winding,
                                                            int32_t* __restrict__ nearest_face) {
    __shared__ StagedTri tile[kSdfTile];
    const uint32_t n = blockIdx.x * kSdfBlock + threadIdx.x;
    const bool live = n < N;
    const size_t row = live ? (size_t)n : (size_t)(N - 1);  // (idle lanes of the last workgroup still stage and walk the tiles)
    const float px = points[row * 3], py = points[row * 3 + 1], pz = points[row * 3 + 2];
    float best = 3.402823466e+38f, omega = 0.0f;
    uint32_t best_face = 0;
    for (uint32_t base = 0; base < F; base += kSdfTile) {
        const uint32_t count = F - base < kSdfTile ? F - base : kSdfTile;
        if (threadIdx.x < count) tile[threadIdx.x] = stage_tri(triangles + (size_t)(base + threadIdx.x) * 9);
        __syncthreads();
        for (uint32_t j = 0; j < count; j++) {
            pair_accumulate(tile[j], base + j, px, py, pz, &best, &best_face, &omega);  // (one address in every lane: a broadcast read)
        }
        __syncthreads();
    }
    if (!live) return;
    float s, wn;
    pair_finish(true, best, omega, &s, &wn);
    sdf[n] = s;
    if (winding) winding[n] = wn;
    if (nearest_face) nearest_face[n] = (int32_t)best_face;
}

// ---- one dataset item ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float unit24(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }  // [0, 1)

__global__ void __launch_bounds__(256) sdf_sample_kernel(const float* __restrict__ triangles, const float* __restrict__ cdf, uint32_t F,
                                                        uint32_t N, uint32_t key, uint32_t step, float noise_std,
                                                        float* __restrict__ points, int32_t* __restrict__ face) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N) return;
    const uint32_t c = n * 8u;  // eight words of the stream belong to a row
    float x, y, z;
    int32_t f_out = -1;
    if (n >= N / 8 * 7) {
        x = unit24(hash_u32(key, step, c)) * 2.0f - 1.0f;
        y = unit24(hash_u32(key, step, c + 1)) * 2.0f - 1.0f;
        z = unit24(hash_u32(key, step, c + 2)) * 2.0f - 1.0f;
    } else {
        const float u = unit24(hash_u32(key, step, c));
        uint32_t lo = 0, hi = F - 1;  // the first f with cdf[f] > u (cdf[F - 1] = 1 > u)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cdf[mid] > u) hi = mid; else lo = mid + 1;
        }
        f_out = (int32_t)lo;
        const float* t = triangles + (size_t)lo * 9;
        const float s1 = sqrtf(unit24(hash_u32(key, step, c + 1))), u2 = unit24(hash_u32(key, step, c + 2));
        const float wa = 1.0f - s1, wb = s1 * (1.0f - u2), wc = s1 * u2;
        x = wa * t[0] + wb * t[3] + wc * t[6];
        y = wa * t[1] + wb * t[4] + wc * t[7];
        z = wa * t[2] + wb * t[5] + wc * t[8];
        if (n >= N / 2) {
            // Box-Muller: (0, 1] under the logarithm, two words per pair of normals, the second pair's sine unused
            const float r0 = sqrtf(-2.0f * logf((float)((hash_u32(key, step, c + 3) >> 8) + 1u) * (1.0f / 16777216.0f)));
            const float r1 = sqrtf(-2.0f * logf((float)((hash_u32(key, step, c + 5) >> 8) + 1u) * (1.0f / 16777216.0f)));
            const float a0 = 6.283185307179586f * unit24(hash_u32(key, step, c + 4));
            const float a1 = 6.283185307179586f * unit24(hash_u32(key, step, c + 6));
            x = x + noise_std * (r0 * cosf(a0));
            y = y + noise_std * (r0 * sinf(a0));
            z = z + noise_std * (r1 * cosf(a1));
        }
    }
    points[(size_t)n * 3] = x;
    points[(size_t)n * 3 + 1] = y;
    points[(size_t)n * 3 + 2] = z;
    if (face) face[n] = f_out;
}

// ---- MAPE with its gradient --------------------------------------------------------------------------------------------------
constexpr uint32_t kMapeBlock = kSumBlock;
constexpr uint32_t kMapeMaxBlocks = 1024;

template <bool HALF>
__global__ void __launch_bounds__(kMapeBlock) sdf_mape_kernel(const void* __restrict__ pred_, const float* __restrict__ target, uint32_t B,
                                                             float clip, float grad_scale, float* __restrict__ loss,
                                                             void* __restrict__ grad_, float* partials, uint32_t* ticket) {
    __shared__ SumShared sh;
    const float fB = (float)B;
    float s = 0.0f;
    for (uint32_t b = blockIdx.x * kMapeBlock + threadIdx.x; b < B; b += gridDim.x * kMapeBlock) {
        float raw;
        if (HALF) raw = __half2float(((const __half*)pred_)[(size_t)b * 16]);
        else raw = ((const float*)pred_)[b];
        const bool clamped = clip > 0.0f && fabsf(raw) > clip;
        const float p = clip > 0.0f ? clampf(raw, -clip, clip) : raw;
        const float t = target[b];
        const float diff = p - t, scale = fabsf(t) + 1e-2f;
        s += fabsf(diff) / scale;
        const float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
        const float g = clamped ? 0.0f : grad_scale * sgn / (scale * fB);
        if (HALF) {
            // the whole 32-byte row: column 0 the gradient, columns 1..15 zero
            uint4* row = (uint4*)((__half*)grad_ + (size_t)b * 16);
            row[0] = make_uint4((uint32_t)__half_as_ushort(__float2half(g)), 0u, 0u, 0u);
            row[1] = make_uint4(0u, 0u, 0u, 0u);
        } else {
            ((float*)grad_)[b] = g;
        }
    }
    // a lane's rows in index order, then the fixed order of csrc/ordered_sum.hpp
    float total;
    if (ordered_sum_finish(block_sum(s, sh), partials, ticket, gridDim.x, blockIdx.x, sh, total)) *loss = total / fB;
}

uint32_t mape_blocks(uint32_t B) {
    const uint32_t g = div_up<uint32_t>(B, kMapeBlock);
    return g > kMapeMaxBlocks ? kMapeMaxBlocks : (g ? g : 1u);
}

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT int s3d_mesh_sdf_tile(void) { return (int)kSdfTile; }

S3D_EXPORT int s3d_mesh_sdf(const float* points, uint32_t N, const float* triangles, uint32_t F, float* sdf, float* winding,
                            int32_t* nearest_face, s3d_stream_t stream) {
    S3D_REQUIRE(F > 0, "mesh_sdf: the mesh has no triangles");
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(points && triangles && sdf, "mesh_sdf: points, triangles and sdf must not be NULL");
    S3D_REQUIRE(F <= 0x7FFFFFFFu, "mesh_sdf: nearest_face is int32: at most 2^31 - 1 triangles");
    S3D_REQUIRE(N <= 0xFFFFFF00u, "mesh_sdf: at most 2^32 - 256 points per call");
    hipLaunchKernelGGL(mesh_sdf_kernel, dim3(div_up<uint32_t>(N, kSdfBlock)), dim3(kSdfBlock), 0, as_stream(stream), points, N,
                       triangles, F, sdf, winding, nearest_face);
    return check_launch("mesh_sdf");
}

S3D_EXPORT int s3d_sdf_sample_points(const float* triangles, const float* cdf, uint32_t F, uint32_t N, uint32_t key, uint32_t step,
                                     float noise_std, float* points, int32_t* face, s3d_stream_t stream) {
    S3D_REQUIRE(N % 8 == 0, "sdf_sample_points: num_samples must be divisible by 8, got %u", N);
    S3D_REQUIRE(N <= (1u << 28), "sdf_sample_points: at most 2^28 rows (eight words of the random stream per row)");
    S3D_REQUIRE(F > 0 && F <= 0x7FFFFFFFu, "sdf_sample_points: the mesh needs between 1 and 2^31 - 1 triangles");
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(triangles && cdf && points, "sdf_sample_points: triangles, cdf and points must not be NULL");
    hipLaunchKernelGGL(sdf_sample_kernel, dim3(div_up<uint32_t>(N, 256u)), dim3(256), 0, as_stream(stream), triangles, cdf, F, N, key,
                       step, noise_std, points, face);
    return check_launch("sdf_sample_points");
}

S3D_EXPORT size_t s3d_sdf_mape_workspace_size(uint32_t B) { return SumWorkspace::bytes(mape_blocks(B)); }

S3D_EXPORT int s3d_sdf_mape_forward_backward(const void* pred, int dtype, const float* target, uint32_t B, float clip, float grad_scale,
                                             float* loss, void* grad, void* workspace, size_t workspace_bytes, s3d_stream_t stream) {
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "sdf_mape: dtype must be S3D_F32 ([B,1]) or S3D_F16 ([B,16])");
    S3D_REQUIRE(B > 0, "sdf_mape: the mean of an empty batch is undefined");
    S3D_REQUIRE(pred && target && loss && grad, "sdf_mape: pred, target, loss and grad must not be NULL");
    S3D_REQUIRE(SumWorkspace::fits(workspace, workspace_bytes, mape_blocks(B)),
                "sdf_mape: needs a 16-byte aligned workspace of s3d_sdf_mape_workspace_size(B) bytes");
    S3D_REQUIRE(dtype == S3D_F32 || ((uintptr_t)grad % 16 == 0), "sdf_mape: the fp16 gradient rows must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    SumWorkspace ws;
    S3D_HIP(ws.arm(workspace, st));
    const uint32_t blocks = mape_blocks(B);
    if (dtype == S3D_F16)
        hipLaunchKernelGGL(sdf_mape_kernel<true>, dim3(blocks), dim3(kMapeBlock), 0, st, pred, target, B, clip, grad_scale, loss, grad,
                           ws.partials, ws.ticket);
    else
        hipLaunchKernelGGL(sdf_mape_kernel<false>, dim3(blocks), dim3(kMapeBlock), 0, st, pred, target, B, clip, grad_scale, loss, grad,
                           ws.partials, ws.ticket);
    return check_launch("sdf_mape_forward_backward");
}
