// dnerf.hip — the glue kernels of the D-NeRF backbone (dnerf/network.py:123-165 of the reference) for gfx950: the two fp16 input
// rows of the deformation and the density network, the warp x' = x + deform with the hash / tiled grid lookup at x' written
// straight into the density network's row, and the two small backward steps around s3d_grid_encode_backward.
//
//   din [B, 80]  = [freq_10(x) (63) | freq_6(t) (13) | 0 (4)]
//   sin [B, 112] = [grid(x') (2 L <= 32) | freq_10(x) (63) | freq_6(t) (13) | 0 (4)]
//
// Columns 32..111 of `sin` ARE the din row: both rows are whole 16-byte words (160 B and 224 B row strides, the copy at byte 64
// of the sin row), so one lane forms eight columns once and stores the same word twice.  The seams of the layout (63, 76; 95, 108
// in the sin row) fall inside words, never across a store.
#include "s3d_common.hpp"
#include "grid_group.hpp"
#include "ordered_sum.hpp"
#include <math.h>

namespace s3d {
namespace {

constexpr uint32_t kDinCols = 80, kSinCols = 112, kGridCols = 32;
constexpr uint32_t kXDeg = 10, kTDeg = 6, kXCols = 3 + 6 * kXDeg /* 63 */, kTCols = 1 + 2 * kTDeg /* 13 */;
constexpr uint32_t kWords = kDinCols / 8;  // 16-byte words per row
static_assert(kXCols + kTCols <= kDinCols && kGridCols + kDinCols == kSinCols, "row layouts");

// column c of [freq_10(x) | freq_6(t) | 0]: k_freq_forward's expression (csrc/encoders.hip) for D = 3 and for D = 1
__device__ __forceinline__ float din_column(uint32_t c, const float (&x)[3], float t) {
    const float half_pi = 3.141592653589793f / 2;
    if (c < kXCols) {
        if (c < 3) return x[c];
        const uint32_t col = c / 3 - 1, d = c % 3, freq = col / 2;
        return sinf(ldexpf(x[d], (int)freq) + (float)(col % 2) * half_pi);
    }
    c -= kXCols;
    if (c < kTCols) {
        if (c < 1) return t;
        const uint32_t col = c - 1, freq = col / 2;
        return sinf(ldexpf(t, (int)freq) + (float)(col % 2) * half_pi);
    }
    return 0.0f;
}

// one lane per 16-byte word of the 80-column row: kWords lanes per sample
__global__ void __launch_bounds__(256) k_dnerf_encode(const float* __restrict__ x, const float* __restrict__ t, uint32_t t_stride,
                                                      uint32_t B, _Float16* __restrict__ din, _Float16* __restrict__ sin,
                                                      const int32_t* __restrict__ n_valid) {
    const uint32_t Bv = valid_rows(B, n_valid);
    const uint64_t total = (uint64_t)Bv * kWords;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t b = (uint32_t)(i / kWords), w = (uint32_t)(i - (uint64_t)b * kWords);
        const float xv[3] = {x[(size_t)b * 3], x[(size_t)b * 3 + 1], x[(size_t)b * 3 + 2]};
        const float tv = t[(size_t)b * t_stride];
        Half8 o;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) o.v[k] = (_Float16)din_column(w * 8 + k, xv, tv);
        *reinterpret_cast<Half8*>(din + (size_t)b * kDinCols + w * 8) = o;
        *reinterpret_cast<Half8*>(sin + (size_t)b * kSinCols + kGridCols + w * 8) = o;
    }
}

// ---- warp + grid lookup ---------------------------------------------------------------------------------------------------
// Workgroup (chunk, g) serves the four levels 4 g .. 4 g + 3 of 256 samples (csrc/grid_group.hpp: the level step, the Jacobian
// columns and the stores): a lane's features of those levels are eight consecutive fp16 columns of its sin row, its Jacobian entries
// 24 consecutive values of dy_dx.  blockIdx.x = chunk * NG + g, so a level group stays on the XCDs g, g + NG, ... (workgroups are
// dealt round-robin over the eight XCDs) and one XCD's L2 holds four levels' tables.
constexpr uint32_t kWarpBlock = kSumBlock;

template <typename T>
struct WarpArgs {
    const float* x;           // [B, 3]
    const _Float16* dout;     // [B, 16]: the deformation net's output, columns 0..2 = deform
    const T* grid;
    const int32_t* offsets;
    _Float16* sin;            // [B, 112]
    float* xw;                // [B, 3]
    float* deform;            // [B, 3] or NULL
    T* dy_dx;                 // [B, L, 3, 2] or NULL
    float* reg_sum;           // or NULL
    float* partials;          // [chunks] (reg_sum)
    uint32_t* ticket;         // zero at launch (reg_sum)
    uint32_t B, L, gridtype, interp;
    bool align_corners;
};

// (eight waves per SIMD asked for: the fp32 instantiation sits at the 64-register edge, where the allocator otherwise lands on either
// side of it from one small change of the source to the next)
template <typename T>
__global__ void __launch_bounds__(kWarpBlock, 8) k_dnerf_warp_grid(WarpArgs<T> a, LevelScales scales) {
    constexpr uint32_t D = 3, C = 2;
    const uint32_t NG = div_up<uint32_t>(a.L, kGroup);
    const uint32_t g = blockIdx.x % NG, chunk = blockIdx.x / NG;
    const uint32_t b = chunk * kWarpBlock + threadIdx.x;
    const uint32_t Bv = valid_rows(a.B, scales.n_valid);
    const bool valid = b < Bv;
    float dv[D] = {0.0f, 0.0f, 0.0f}, xw[D] = {0.0f, 0.0f, 0.0f};
    if (valid) {
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            dv[d] = (float)a.dout[(size_t)b * 16 + d];
            xw[d] = a.x[(size_t)b * D + d] + dv[d];
        }
    }
    if (g == 0) {
        if (valid) {
#pragma unroll
            for (uint32_t d = 0; d < D; d++) {
                a.xw[(size_t)b * D + d] = xw[d];
                if (a.deform) a.deform[(size_t)b * D + d] = dv[d];
            }
        }
        if (a.reg_sum) {  // sum of |deform| over the live rows: one row per lane, one partial per chunk (csrc/ordered_sum.hpp)
            __shared__ SumShared sh;
            const float s = block_sum(valid ? (fabsf(dv[0]) + fabsf(dv[1])) + fabsf(dv[2]) : 0.0f, sh);
            float total;
            if (ordered_sum_finish(s, a.partials, a.ticket, gridDim.x / NG, chunk, sh, total)) *a.reg_sum = total;
        }
    }
    if (!valid) return;

    // [-bound, bound] -> [0, 1] as load_point does it
    float x01[D];
    bool oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        x01[d] = xw[d];
        if (scales.bound != 0.0f) x01[d] = (x01[d] + scales.bound) * scales.inv_2bound;
        if (x01[d] < 0 || x01[d] > 1) oob = true;
    }

    const uint32_t l0 = g * kGroup;
    Half8 o;  // (rows outside the box and levels past L: zeros)
    T jac[kGroup][D * C];
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
        o.v[k * C] = o.v[k * C + 1] = (_Float16)0.0f;
#pragma unroll
        for (uint32_t n = 0; n < D * C; n++) jac[k][n] = Acc<T>::zero();
    }
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
        const uint32_t level = l0 + k;
        if (level >= a.L || oob) continue;
        const LevelTable<T> lt = level_table<T>(a.grid, a.offsets, level, scales.v[level]);
        float pos[D], pos_deriv[D];
        T feat[1u << D][C];
        level_value<D, T>(lt, a.gridtype, a.align_corners, a.interp, x01, false, pos, pos_deriv, feat, o, k);
        if (a.dy_dx) {
#pragma unroll
            for (uint32_t gd = 0; gd < D; gd++) jacobian_column<D, T>(gd, lt.scale, pos, pos_deriv, feat, jac[k][gd * C], jac[k][gd * C + 1]);
        }
    }
    // the features as the fp16 columns 2 l, 2 l + 1 of the sin row (16-byte aligned at every group), the Jacobian as [L, 3, 2]
    store_group_features(o, a.sin + (size_t)b * kSinCols + l0 * C, a.L - l0, l0 + kGroup <= a.L);
    if (a.dy_dx) store_group_jacobian<D * C, T>(jac, a.dy_dx + ((size_t)b * a.L + l0) * D * C, a.L, l0);
}

// columns 0 .. 2 L - 1 of the density network's input gradient [B, 112] -> level-major [L][B][2] in the table's dtype.  One lane
// per (four levels, sample): one 16-byte load of the row's eight columns, four stores into the four levels' planes; consecutive
// lanes are consecutive samples, so every level's stores are contiguous.
template <typename T>
__global__ void __launch_bounds__(256) k_dnerf_split_grad(const _Float16* __restrict__ g_sin, uint32_t B, uint32_t L,
                                                          T* __restrict__ out, const int32_t* __restrict__ n_valid) {
    const uint32_t Bv = valid_rows(B, n_valid);
    const uint32_t NG = div_up<uint32_t>(L, kGroup);
    const uint64_t total = (uint64_t)Bv * NG;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t q = (uint32_t)(i / Bv), b = (uint32_t)(i - (uint64_t)q * Bv);
        const Half8 w = *reinterpret_cast<const Half8*>(g_sin + (size_t)b * kSinCols + q * 2 * kGroup);  // (inside the 32 grid columns)
        split_row_group<T>(w, q * kGroup, L, B, b, out);
    }
}

// g_dout[:, 0:3] = half(fmaf(coef, sign(deform), float(g_xw) * g_scale)), columns 3..15 zero: two 16-byte stores per sample
template <typename T>
__global__ void __launch_bounds__(256) k_dnerf_warp_backward(const T* __restrict__ g_xw, float g_scale, const float* __restrict__ deform,
                                                             const float* __restrict__ coef, uint32_t B, _Float16* __restrict__ g_dout,
                                                             const int32_t* __restrict__ n_valid) {
    const uint32_t Bv = valid_rows(B, n_valid);
    const float cf = coef ? *coef : 0.0f;
    for (uint32_t b = blockIdx.x * 256 + threadIdx.x; b < Bv; b += gridDim.x * 256) {
        Half8 lo, hi;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) { lo.v[k] = (_Float16)0.0f; hi.v[k] = (_Float16)0.0f; }
#pragma unroll
        for (uint32_t d = 0; d < 3; d++) {
            const float g = Acc<T>::to_f(g_xw[(size_t)b * 3 + d]) * g_scale;
            float sg = 0.0f;
            if (coef) {
                const float v = deform[(size_t)b * 3 + d];
                sg = v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f);
            }
            lo.v[d] = (_Float16)__builtin_fmaf(cf, sg, g);
        }
        Half8* row = reinterpret_cast<Half8*>(g_dout + (size_t)b * 16);
        row[0] = lo;
        row[1] = hi;
    }
}

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT int s3d_dnerf_encode_forward(const float* x, const float* t, uint32_t t_stride, uint32_t B, uint16_t* din, uint16_t* sin,
                                        const int32_t* n_valid, s3d_stream_t stream) {
    if (B == 0) return S3D_OK;
    S3D_REQUIRE(x && t && din && sin, "dnerf_encode_forward: null pointer");
    S3D_REQUIRE(t_stride <= 1, "dnerf_encode_forward: t_stride is 0 (one time for all rows) or 1 (one per row)");
    S3D_REQUIRE(((uintptr_t)din | (uintptr_t)sin) % 16 == 0, "dnerf_encode_forward: din and sin must be 16-byte aligned");
    hipLaunchKernelGGL(k_dnerf_encode, dim3(stream_grid((uint64_t)B * kWords, 256)), dim3(256), 0, as_stream(stream), x, t, t_stride, B,
                       (_Float16*)din, (_Float16*)sin, n_valid);
    return check_launch("dnerf_encode_forward");
}

S3D_EXPORT size_t s3d_dnerf_warp_grid_workspace_size(uint32_t B) {
    return SumWorkspace::bytes(div_up<uint32_t>(B, kWarpBlock));
}

template <typename T>
static int launch_warp_grid(WarpArgs<T> a, const LevelScales& sc, hipStream_t st) {
    const uint32_t NG = div_up<uint32_t>(a.L, kGroup);
    hipLaunchKernelGGL((k_dnerf_warp_grid<T>), dim3(div_up<uint32_t>(a.B, kWarpBlock) * NG), dim3(kWarpBlock), 0, st, a, sc);
    return check_launch("dnerf_warp_grid_forward");
}

S3D_EXPORT int s3d_dnerf_warp_grid_forward(const float* x, const uint16_t* dout, const void* embeddings, const int32_t* offsets,
                                           uint32_t B, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                           uint32_t interp, int dtype, float bound, uint16_t* sin, float* xw, float* deform, void* dy_dx,
                                           float* reg_sum, void* workspace, size_t workspace_bytes, const int32_t* n_valid,
                                           s3d_stream_t stream) {
    if (B == 0) {
        if (reg_sum) S3D_HIP(hipMemsetAsync(reg_sum, 0, sizeof(float), as_stream(stream)));
        return S3D_OK;
    }
    S3D_REQUIRE(x && dout && embeddings && offsets && sin && xw, "dnerf_warp_grid_forward: null pointer");
    S3D_REQUIRE(L >= 1 && 2 * L <= kGridCols, "dnerf_warp_grid_forward: 1 <= L <= 16 (two features per level, 32 columns)");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "dnerf_warp_grid_forward: dtype");
    S3D_REQUIRE(gridtype <= 1 && interp <= 1, "dnerf_warp_grid_forward: gridtype / interpolation");
    S3D_REQUIRE(((uintptr_t)sin | (uintptr_t)dy_dx) % 16 == 0, "dnerf_warp_grid_forward: sin and dy_dx must be 16-byte aligned");
    S3D_REQUIRE(!reg_sum || SumWorkspace::fits(workspace, workspace_bytes, div_up<uint32_t>(B, kWarpBlock)),
                "dnerf_warp_grid_forward: reg_sum needs a workspace of s3d_dnerf_warp_grid_workspace_size(B) bytes");
    hipStream_t st = as_stream(stream);
    LevelScales sc;
    host_scales(L, S, H, sc, bound, n_valid);
    SumWorkspace ws;
    if (reg_sum) S3D_HIP(ws.arm(workspace, st));
    if (dtype == S3D_F16) {
        WarpArgs<__half> a{x, (const _Float16*)dout, (const __half*)embeddings, offsets, (_Float16*)sin, xw, deform, (__half*)dy_dx,
                           reg_sum, ws.partials, ws.ticket, B, L, gridtype, interp, align_corners != 0};
        return launch_warp_grid<__half>(a, sc, st);
    }
    WarpArgs<float> a{x, (const _Float16*)dout, (const float*)embeddings, offsets, (_Float16*)sin, xw, deform, (float*)dy_dx,
                      reg_sum, ws.partials, ws.ticket, B, L, gridtype, interp, align_corners != 0};
    return launch_warp_grid<float>(a, sc, st);
}

S3D_EXPORT int s3d_dnerf_split_grad(const uint16_t* grad_sin, uint32_t B, uint32_t L, int dtype, void* grad_levels,
                                    const int32_t* n_valid, s3d_stream_t stream) {
    if (B == 0) return S3D_OK;
    S3D_REQUIRE(grad_sin && grad_levels, "dnerf_split_grad: null pointer");
    S3D_REQUIRE(L >= 1 && 2 * L <= kGridCols, "dnerf_split_grad: 1 <= L <= 16");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "dnerf_split_grad: dtype");
    S3D_REQUIRE((uintptr_t)grad_sin % 16 == 0, "dnerf_split_grad: grad_sin must be 16-byte aligned");
    const dim3 grid(stream_grid((uint64_t)B * div_up<uint32_t>(L, kGroup), 256)), block(256);
    if (dtype == S3D_F16)
        hipLaunchKernelGGL((k_dnerf_split_grad<__half>), grid, block, 0, as_stream(stream), (const _Float16*)grad_sin, B, L,
                           (__half*)grad_levels, n_valid);
    else
        hipLaunchKernelGGL((k_dnerf_split_grad<float>), grid, block, 0, as_stream(stream), (const _Float16*)grad_sin, B, L,
                           (float*)grad_levels, n_valid);
    return check_launch("dnerf_split_grad");
}

S3D_EXPORT int s3d_dnerf_warp_backward(const void* grad_xw, int dtype, float grad_scale, const float* deform, const float* coef,
                                       uint32_t B, uint16_t* grad_dout, const int32_t* n_valid, s3d_stream_t stream) {
    if (B == 0) return S3D_OK;
    S3D_REQUIRE(grad_xw && grad_dout && (deform || !coef), "dnerf_warp_backward: null pointer");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "dnerf_warp_backward: dtype");
    S3D_REQUIRE((uintptr_t)grad_dout % 16 == 0, "dnerf_warp_backward: grad_dout must be 16-byte aligned");
    const dim3 grid(stream_grid(B, 256)), block(256);
    if (dtype == S3D_F16)
        hipLaunchKernelGGL((k_dnerf_warp_backward<__half>), grid, block, 0, as_stream(stream), (const __half*)grad_xw, grad_scale, deform,
                           coef, B, (_Float16*)grad_dout, n_valid);
    else
        hipLaunchKernelGGL((k_dnerf_warp_backward<float>), grid, block, 0, as_stream(stream), (const float*)grad_xw, grad_scale, deform,
                           coef, B, (_Float16*)grad_dout, n_valid);
    return check_launch("dnerf_warp_backward");
}
