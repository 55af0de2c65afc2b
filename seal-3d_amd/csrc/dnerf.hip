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
#include "grid_device.hpp"
#include <math.h>

namespace s3d {
namespace {

constexpr uint32_t kDinCols = 80, kSinCols = 112, kGridCols = 32;
constexpr uint32_t kXDeg = 10, kTDeg = 6, kXCols = 3 + 6 * kXDeg /* 63 */, kTCols = 1 + 2 * kTDeg /* 13 */;
constexpr uint32_t kWords = kDinCols / 8;  // 16-byte words per row
static_assert(kXCols + kTCols <= kDinCols && kGridCols + kDinCols == kSinCols, "row layouts");

struct alignas(16) Half8 { _Float16 v[8]; };

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
// Workgroup (chunk, g) serves the four levels 4 g .. 4 g + 3 of 256 samples: a lane's features of those levels are eight
// consecutive fp16 columns of its sin row (one 16-byte store), its Jacobian entries 24 consecutive values of dy_dx.  blockIdx.x =
// chunk * NG + g, so a level group stays on the XCDs g, g + NG, ... (workgroups are dealt round-robin over the eight XCDs) and one
// XCD's L2 holds four levels' tables.  Rows, weights and sums are k_grid_forward's (csrc/gridencoder.hip), expression by
// expression, through the helpers of grid_device.hpp.
constexpr uint32_t kWarpBlock = 256, kGroup = 4;

// The fp16 sums of grid_device.hpp's Acc<__half> with the fp32 value pinned before it is rounded to binary16: "round the fp32
// product, then round that to half" (what k_grid_forward's v_mul_f32 + v_cvt_pk_f16_f32 do) and "round the exact product to half
// once" (v_fma_mixlo_f16, which the compiler picked for the feature sums of this kernel) differ in one value in ~10^4.  An fp32
// value that exists in a register rounds to half the same way whatever instruction converts it.
__device__ __forceinline__ float pinned(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
template <typename T>
__device__ __forceinline__ T feat_fma(float w, T g, T acc) {
    if constexpr (sizeof(T) == 2) return __hadd(acc, __float2half(pinned(w * __half2float(g))));
    else return Acc<T>::fma(w, g, acc);
}

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

template <typename T>
__global__ void __launch_bounds__(kWarpBlock) k_dnerf_warp_grid(WarpArgs<T> a, LevelScales scales) {
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
        if (a.reg_sum) {
            // sum of |deform| in a fixed order: lanes by a shuffle tree, waves in order, workgroups in order by the last one to
            // arrive (one agent-scope release per workgroup, one acquire by the last) — no float atomics, the same bits every run
            __shared__ float part[kWarpBlock / 64 + 1];
            float s = valid ? (fabsf(dv[0]) + fabsf(dv[1])) + fabsf(dv[2]) : 0.0f;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) s += __shfl_down(s, o, 64);
            if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
            __syncthreads();
            const uint32_t nchunks = gridDim.x / NG;
            if (threadIdx.x == 0) {
                float v = part[0];
                for (uint32_t w = 1; w < kWarpBlock / 64; w++) v += part[w];
                a.partials[chunk] = v;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const uint32_t arrived = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool last = arrived == nchunks - 1;
                if (last) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                part[kWarpBlock / 64] = last ? 1.0f : 0.0f;
            }
            __syncthreads();
            if (part[kWarpBlock / 64] != 0.0f) {  // (workgroup-uniform)
                float v = 0.0f;
                for (uint32_t i = threadIdx.x; i < nchunks; i += kWarpBlock) v += a.partials[i];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
                __syncthreads();
                if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = v;
                __syncthreads();
                if (threadIdx.x == 0) {
                    float r = part[0];
                    for (uint32_t w = 1; w < kWarpBlock / 64; w++) r += part[w];
                    *a.reg_sum = r;
                    *a.ticket = 0u;
                }
            }
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
    T res[kGroup][C];
    T jac[kGroup][D][C];
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            res[k][c] = Acc<T>::zero();
#pragma unroll
            for (uint32_t d = 0; d < D; d++) jac[k][d][c] = Acc<T>::zero();
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
        const uint32_t level = l0 + k;
        if (level >= a.L || oob) continue;
        const uint32_t off = (uint32_t)a.offsets[level];
        const uint32_t hashmap_size = (uint32_t)a.offsets[level + 1] - off;
        const T* table = a.grid + (size_t)off * C;
        const float scale = scales.v[level];
        const uint32_t resolution = (uint32_t)ceilf(scale) + 1;
        float pos[D], pos_deriv[D];
        uint32_t pos_grid[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) pos_deriv[d] = (d == 0) ? 1.0f : 0.0f;  // `= {1.0f}`, gridencoder.cu:143
        locate<D>(x01, scale, a.align_corners, a.interp, pos, pos_deriv, pos_grid);

        T feat[1u << D][C];
        float wts[1u << D];
#pragma unroll
        for (uint32_t idx = 0; idx < (1u << D); idx++) {
            float w = 1;
            uint32_t pgl[D];
#pragma unroll
            for (uint32_t d = 0; d < D; d++) {
                if ((idx & (1u << d)) == 0) { w *= 1 - pos[d]; pgl[d] = pos_grid[d]; }
                else { w *= pos[d]; pgl[d] = pos_grid[d] + 1; }
            }
            wts[idx] = w;
            const uint32_t row = grid_row<D>(a.gridtype, a.align_corners, hashmap_size, resolution, pgl);
            load_feat<T, C>(table + (size_t)row * C, feat[idx]);
        }
#pragma unroll
        for (uint32_t idx = 0; idx < (1u << D); idx++) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) res[k][c] = feat_fma<T>(wts[idx], feat[idx][c], res[k][c]);
        }
        if (a.dy_dx) {  // gridencoder.cu:198-241; the corner rows are those gathered above (corner idx = bit d of dimension d)
#pragma unroll
            for (uint32_t gd = 0; gd < D; gd++) {
#pragma unroll
                for (uint32_t idx = 0; idx < (1u << (D - 1)); idx++) {
                    float w = scale;
                    uint32_t corner = 0;
#pragma unroll
                    for (uint32_t nd = 0; nd < D - 1; nd++) {
                        const uint32_t d = (nd >= gd) ? (nd + 1) : nd;
                        if ((idx & (1u << nd)) == 0) { w *= 1 - pos[d]; }
                        else { w *= pos[d]; corner |= 1u << d; }
                    }
#pragma unroll
                    for (uint32_t c = 0; c < C; c++) {
                        const float diff = Acc<T>::to_f(Acc<T>::sub(feat[corner | (1u << gd)][c], feat[corner][c]));
                        if constexpr (sizeof(T) == 2) jac[k][gd][c] = Acc<T>::add(jac[k][gd][c], Acc<T>::from_f(pinned(w * diff * pos_deriv[gd])));
                        else jac[k][gd][c] = Acc<T>::from_f(__builtin_fmaf(w * diff, pos_deriv[gd], Acc<T>::to_f(jac[k][gd][c])));
                    }
                }
            }
        }
    }

    // the features as the fp16 columns 2 l, 2 l + 1 of the sin row
    _Float16* srow = a.sin + (size_t)b * kSinCols + l0 * C;
    Half8 o;
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            if constexpr (sizeof(T) == 2) { __half h = res[k][c]; __builtin_memcpy(&o.v[k * C + c], &h, 2); }
            else o.v[k * C + c] = (_Float16)res[k][c];
        }
    }
    if (l0 + kGroup <= a.L) *reinterpret_cast<Half8*>(srow) = o;
    else {  // (a ragged last group; every index below is a compile-time constant: the arrays stay in registers)
#pragma unroll
        for (uint32_t k = 0; k < kGroup; k++)
            if (l0 + k < a.L) { srow[k * C] = o.v[k * C]; srow[k * C + 1] = o.v[k * C + 1]; }
    }
    if (a.dy_dx) {
        T* j = a.dy_dx + ((size_t)b * a.L + l0) * D * C;
        if (a.L % kGroup == 0) {  // whole 16-byte words: 48 B (fp16) / 96 B (fp32) per lane, rows of L * 12 / L * 24 bytes
            constexpr uint32_t NW = kGroup * D * C * sizeof(T) / 16;
            uint4 w[NW];
            __builtin_memcpy(w, jac, sizeof(w));
#pragma unroll
            for (uint32_t i = 0; i < NW; i++) reinterpret_cast<uint4*>(j)[i] = w[i];
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kGroup; k++) {
                if (l0 + k >= a.L) continue;
#pragma unroll
                for (uint32_t d = 0; d < D; d++) store_feat<T, C>(j + (k * D + d) * C, jac[k][d]);
            }
        }
    }
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
#pragma unroll
        for (uint32_t k = 0; k < kGroup; k++) {
            const uint32_t l = q * kGroup + k;
            if (l >= L) continue;
            T v[2];
            if constexpr (sizeof(T) == 2) __builtin_memcpy(v, &w.v[2 * k], 4);
            else { v[0] = (float)w.v[2 * k]; v[1] = (float)w.v[2 * k + 1]; }
            store_feat<T, 2>(out + ((size_t)l * B + b) * 2, v);
        }
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
    return 16 + sizeof(float) * (size_t)div_up<uint32_t>(B, kWarpBlock);
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
    S3D_REQUIRE(!reg_sum || (workspace && workspace_bytes >= s3d_dnerf_warp_grid_workspace_size(B) && (uintptr_t)workspace % 16 == 0),
                "dnerf_warp_grid_forward: reg_sum needs a workspace of s3d_dnerf_warp_grid_workspace_size(B) bytes");
    hipStream_t st = as_stream(stream);
    LevelScales sc;
    host_scales(L, S, H, sc, bound, n_valid);
    uint32_t* ticket = nullptr;
    float* partials = nullptr;
    if (reg_sum) {
        ticket = (uint32_t*)workspace;
        partials = (float*)((char*)workspace + 16);
        S3D_HIP(hipMemsetAsync(ticket, 0, 16, st));
    }
    if (dtype == S3D_F16) {
        WarpArgs<__half> a{x, (const _Float16*)dout, (const __half*)embeddings, offsets, (_Float16*)sin, xw, deform, (__half*)dy_dx,
                           reg_sum, partials, ticket, B, L, gridtype, interp, align_corners != 0};
        return launch_warp_grid<__half>(a, sc, st);
    }
    WarpArgs<float> a{x, (const _Float16*)dout, (const float*)embeddings, offsets, (_Float16*)sin, xw, deform, (float*)dy_dx,
                      reg_sum, partials, ticket, B, L, gridtype, interp, align_corners != 0};
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
