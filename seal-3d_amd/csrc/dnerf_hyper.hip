// dnerf_hyper.hip — the 4-D grid lookup of the D-NeRF hyper backbone (dnerf/network_hyper.py:126-140 of the reference:
// `ambient = tanh(ambient_net(freq_6(t))) * bound; x = cat([x, ambient.repeat(N, 1)]); x = encoder(x, bound)`) for gfx950.
// One call has one time, so the fourth coordinate of every row is the same device word.  The generic route builds [N, 4], runs
// the grid forward with dy_dx (16 gathers per level for the value and 4 x 8 x 2 for the Jacobian), stores dy_dx [N, L, 4, 2] and
// back-propagates all four columns, of which only the ambient one has a consumer.  Here:
//   forward : x [B,3] f32, ambient [1] f32 (device) -> feat [B, 2L] f16, x4 [B,4] f32 = [x | ambient], dy_da [B, L, 2] (the table's
//             dtype) = the ambient column of the Jacobian, formed from the 16 corners the value has already fetched
//   backward: grad_feat [B, 2L] f16, dy_da -> grad_levels [L][B][2] (the table's dtype, what s3d_grid_encode_backward takes),
//             grad_ambient [1] f32 = grad_scale * sum_b sum_k float(g_bk) float(j_bk)
// The forward is the four-levels-per-workgroup lookup of csrc/grid_group.hpp for D = 4: workgroup (chunk, g) serves four levels of
// 256 rows, a lane's features of those levels are one 16-byte store.  The backward's sum is the ordered sum of
// csrc/ordered_sum.hpp over a grid of fixed size (per-lane running sums over the row stride gridDim.x * 256) — no float atomics,
// the same bits on every run.
#include "s3d_common.hpp"
#include "grid_group.hpp"
#include "ordered_sum.hpp"
#include <math.h>

namespace s3d {
namespace {

constexpr uint32_t kBlock = kSumBlock, kMaxLevelsHyper = 16;
constexpr uint32_t kMaxBlocks = 512;  // workgroups of the backward (two per CU): one fp32 partial each

template <typename T>
struct HyperArgs {
    const float* x;        // [B, 3]
    const float* ambient;  // one device word
    const T* grid;
    const int32_t* offsets;
    _Float16* feat;        // [B, 2 L]
    float* x4;             // [B, 4] or NULL
    T* dy_da;              // [B, L, 2] or NULL
    uint32_t B, L, gridtype, interp;
    bool align_corners;
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_dnerf_hyper_grid(HyperArgs<T> a, LevelScales scales) {
    constexpr uint32_t D = 4, C = 2, GD = D - 1;  // GD: the ambient dimension
    const uint32_t NG = div_up<uint32_t>(a.L, kGroup);
    const uint32_t g = blockIdx.x % NG, chunk = blockIdx.x / NG;
    const uint32_t b = chunk * kBlock + threadIdx.x;
    if (b >= valid_rows(a.B, scales.n_valid)) return;
    float x01[D];
#pragma unroll
    for (uint32_t d = 0; d < GD; d++) x01[d] = a.x[(size_t)b * GD + d];
    x01[GD] = *a.ambient;
    if (g == 0 && a.x4) *reinterpret_cast<float4*>(a.x4 + (size_t)b * D) = make_float4(x01[0], x01[1], x01[2], x01[3]);
    // [-bound, bound] -> [0, 1] as load_point does it, the ambient coordinate included
    bool oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        if (scales.bound != 0.0f) x01[d] = (x01[d] + scales.bound) * scales.inv_2bound;
        if (x01[d] < 0 || x01[d] > 1) oob = true;
    }

    const uint32_t l0 = g * kGroup;
    Half8 o;  // (rows outside the box and levels past L: zeros)
    T jac[kGroup][C];
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
        o.v[k * C] = o.v[k * C + 1] = (_Float16)0.0f;
#pragma unroll
        for (uint32_t n = 0; n < C; n++) jac[k][n] = Acc<T>::zero();
    }
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
        const uint32_t level = l0 + k;
        if (level >= a.L || oob) continue;
        const LevelTable<T> lt = level_table<T>(a.grid, a.offsets, level, scales.v[level]);
        // Does the ambient coordinate enter this level's index?  (level-uniform)  get_grid_index stops adding coordinates once
        // stride > hashmap_size (gridencoder.cu:72); a tiled level past that point addresses the same row for both ambient corners
        // of a pair: eight gathers, each used twice — the same bits.  (A hash level whose strides overflow hashes all four.)
        uint32_t stride = 1;
#pragma unroll
        for (uint32_t d = 0; d < GD; d++)
            if (stride <= lt.hashmap_size) stride *= a.align_corners ? lt.resolution : (lt.resolution + 1);
        const bool shared_rows = a.gridtype == 1 && stride > lt.hashmap_size;
        float pos[D], pos_deriv[D];
        T feat[1u << D][C];
        level_value<D, T>(lt, a.gridtype, a.align_corners, a.interp, x01, shared_rows, pos, pos_deriv, feat, o, k);
        if (a.dy_da) jacobian_column<D, T>(GD, lt.scale, pos, pos_deriv, feat, jac[k][0], jac[k][1]);  // (the pair is (corner, corner | 8))
    }
    // rows of 4 L bytes: whole 16-byte words when L % 4 == 0
    store_group_features(o, a.feat + (size_t)b * a.L * C + l0 * C, a.L - l0, a.L % kGroup == 0);
    if (a.dy_da) store_group_jacobian<C, T>(jac, a.dy_da + ((size_t)b * a.L + l0) * C, a.L, l0);
}

// One lane = one row: the row's 2 L gradient columns go to the L level planes (consecutive lanes are consecutive rows, so every
// plane's stores are contiguous), and the row's term of grad_ambient is the fp32 chain over its columns in ascending order.
template <typename T>
__global__ void __launch_bounds__(kBlock) k_dnerf_hyper_backward(const _Float16* __restrict__ g_feat, const T* __restrict__ dy_da,
                                                                 uint32_t B, uint32_t L, float grad_scale, T* __restrict__ out,
                                                                 float* __restrict__ grad_ambient, float* partials, uint32_t* ticket,
                                                                 const int32_t* __restrict__ n_valid) {
    constexpr uint32_t C = 2;
    __shared__ SumShared sh;
    const uint32_t Bv = valid_rows(B, n_valid);
    const bool whole = L % kGroup == 0;  // (rows of whole 16-byte words)
    float sum = 0.0f;
    for (uint32_t b = blockIdx.x * kBlock + threadIdx.x; b < Bv; b += gridDim.x * kBlock) {
        const _Float16* grow = g_feat + (size_t)b * L * C;
        const T* jrow = dy_da ? dy_da + (size_t)b * L * C : nullptr;
        float acc = 0.0f;
        for (uint32_t l0 = 0; l0 < L; l0 += kGroup) {
            Half8 gv;
            if (whole) gv = *reinterpret_cast<const Half8*>(grow + l0 * C);
            else {
#pragma unroll
                for (uint32_t k = 0; k < kGroup; k++) {
                    uint32_t word = 0;
                    if (l0 + k < L) word = *reinterpret_cast<const uint32_t*>(grow + (l0 + k) * C);
                    __builtin_memcpy(&gv.v[k * C], &word, 4);
                }
            }
            split_row_group<T>(gv, l0, L, B, b, out);
            if (!jrow) continue;
#pragma unroll
            for (uint32_t k = 0; k < kGroup; k++) {
                if (l0 + k >= L) continue;
                T j[C];
                load_feat<T, C>(jrow + (l0 + k) * C, j);
#pragma unroll
                for (uint32_t c = 0; c < C; c++) acc = __builtin_fmaf((float)gv.v[k * C + c], Acc<T>::to_f(j[c]), acc);
            }
        }
        sum += acc;
    }
    if (!grad_ambient) return;  // (workgroup-uniform)
    float total;
    if (ordered_sum_finish(block_sum(sum, sh), partials, ticket, gridDim.x, blockIdx.x, sh, total)) *grad_ambient = total * grad_scale;
}

inline uint32_t backward_blocks(uint32_t B) { return std::min<uint32_t>(kMaxBlocks, std::max<uint32_t>(1u, div_up<uint32_t>(B, kBlock))); }

}  // namespace
}  // namespace s3d

using namespace s3d;

template <typename T>
static int launch_hyper_grid(HyperArgs<T> a, const LevelScales& sc, hipStream_t st) {
    const uint32_t NG = div_up<uint32_t>(a.L, kGroup);
    hipLaunchKernelGGL((k_dnerf_hyper_grid<T>), dim3(div_up<uint32_t>(a.B, kBlock) * NG), dim3(kBlock), 0, st, a, sc);
    return check_launch("dnerf_hyper_grid_forward");
}

S3D_EXPORT int s3d_dnerf_hyper_grid_forward(const float* x, const float* ambient, const void* embeddings, const int32_t* offsets,
                                            uint32_t B, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                            uint32_t interp, int dtype, float bound, uint16_t* feat, float* x4, void* dy_da,
                                            const int32_t* n_valid, s3d_stream_t stream) {
    if (B == 0) return S3D_OK;
    S3D_REQUIRE(x && ambient && embeddings && offsets && feat, "dnerf_hyper_grid_forward: null pointer");
    S3D_REQUIRE(L >= 1 && L <= kMaxLevelsHyper, "dnerf_hyper_grid_forward: 1 <= L <= 16 (two features per level, 32 columns)");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "dnerf_hyper_grid_forward: dtype");
    S3D_REQUIRE(gridtype <= 1 && interp <= 1, "dnerf_hyper_grid_forward: gridtype / interpolation");
    S3D_REQUIRE(bound >= 0.0f, "dnerf_hyper_grid_forward: bound > 0 (raw coordinates) or 0 (coordinates in [0, 1])");
    S3D_REQUIRE(((uintptr_t)feat | (uintptr_t)x4 | (uintptr_t)dy_da) % 16 == 0,
                "dnerf_hyper_grid_forward: feat, x4 and dy_da must be 16-byte aligned");
    LevelScales sc;
    host_scales(L, S, H, sc, bound, n_valid);
    if (dtype == S3D_F16) {
        HyperArgs<__half> a{x, ambient, (const __half*)embeddings, offsets, (_Float16*)feat, x4, (__half*)dy_da, B, L, gridtype, interp,
                            align_corners != 0};
        return launch_hyper_grid<__half>(a, sc, as_stream(stream));
    }
    HyperArgs<float> a{x, ambient, (const float*)embeddings, offsets, (_Float16*)feat, x4, (float*)dy_da, B, L, gridtype, interp,
                       align_corners != 0};
    return launch_hyper_grid<float>(a, sc, as_stream(stream));
}

S3D_EXPORT size_t s3d_dnerf_hyper_backward_workspace_size(uint32_t B) {
    return SumWorkspace::bytes(backward_blocks(B));
}

S3D_EXPORT int s3d_dnerf_hyper_grid_backward(const uint16_t* grad_feat, const void* dy_da, uint32_t B, uint32_t L, int dtype,
                                             float grad_scale, void* grad_levels, float* grad_ambient, void* workspace,
                                             size_t workspace_bytes, const int32_t* n_valid, s3d_stream_t stream) {
    hipStream_t st = as_stream(stream);
    const bool sum = dy_da && grad_ambient;
    if (B == 0) {
        if (sum) S3D_HIP(hipMemsetAsync(grad_ambient, 0, sizeof(float), st));
        return S3D_OK;
    }
    S3D_REQUIRE(grad_feat && grad_levels, "dnerf_hyper_grid_backward: null pointer");
    S3D_REQUIRE(L >= 1 && L <= kMaxLevelsHyper, "dnerf_hyper_grid_backward: 1 <= L <= 16");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "dnerf_hyper_grid_backward: dtype");
    S3D_REQUIRE(((uintptr_t)grad_feat | (uintptr_t)dy_da | (uintptr_t)grad_levels) % 16 == 0,
                "dnerf_hyper_grid_backward: grad_feat, dy_da and grad_levels must be 16-byte aligned");
    S3D_REQUIRE(!sum || SumWorkspace::fits(workspace, workspace_bytes, backward_blocks(B)),
                "dnerf_hyper_grid_backward: grad_ambient needs a workspace of s3d_dnerf_hyper_backward_workspace_size(B) bytes");
    SumWorkspace ws;
    if (sum) S3D_HIP(ws.arm(workspace, st));
    const dim3 grid(backward_blocks(B)), block(kBlock);
    if (dtype == S3D_F16)
        hipLaunchKernelGGL((k_dnerf_hyper_backward<__half>), grid, block, 0, st, (const _Float16*)grad_feat,
                           sum ? (const __half*)dy_da : nullptr, B, L, grad_scale, (__half*)grad_levels, sum ? grad_ambient : nullptr,
                           ws.partials, ws.ticket, n_valid);
    else
        hipLaunchKernelGGL((k_dnerf_hyper_backward<float>), grid, block, 0, st, (const _Float16*)grad_feat,
                           sum ? (const float*)dy_da : nullptr, B, L, grad_scale, (float*)grad_levels, sum ? grad_ambient : nullptr,
                           ws.partials, ws.ticket, n_valid);
    return check_launch("dnerf_hyper_grid_backward");
}
