// dnerf_hyper.hip — the 4-D grid lookup of the D-NeRF hyper backbone (dnerf/network_hyper.py:126-140 of the reference:
// `ambient = tanh(ambient_net(freq_6(t))) * bound; x = cat([x, ambient.repeat(N, 1)]); x = encoder(x, bound)`) for gfx950.
// One call has one time, so the fourth coordinate of every row is the same device word.  The generic route builds [N, 4], runs
// the grid forward with dy_dx (16 gathers per level for the value and 4 x 8 x 2 for the Jacobian), stores dy_dx [N, L, 4, 2] and
// back-propagates all four columns, of which only the ambient one has a consumer.  Here:
//   forward : x [B,3] f32, ambient [1] f32 (device) -> feat [B, 2L] f16, x4 [B,4] f32 = [x | ambient], dy_da [B, L, 2] (the table's
//             dtype) = the ambient column of the Jacobian, formed from the 16 corners the value has already fetched
//   backward: grad_feat [B, 2L] f16, dy_da -> grad_levels [L][B][2] (the table's dtype, what s3d_grid_encode_backward takes),
//             grad_ambient [1] f32 = grad_scale * sum_b sum_k float(g_bk) float(j_bk)
// The forward is k_dnerf_warp_grid's plan (csrc/dnerf.hip) for D = 4: workgroup (chunk, g) serves four levels of 256 rows, a lane's
// features of those levels are one 16-byte store.  Rows, weights and sums are k_grid_forward's (csrc/gridencoder.hip), expression by
// expression, through grid_device.hpp.  The backward's sum is s3d_dnerf_basis_mid_backward's scheme for one column: per-lane
// running sums over the row stride, an exchange tree per wave, waves in index order, write-through partials added in a fixed order
// by the last workgroup to arrive — no float atomics, the same bits on every run.
#include "s3d_common.hpp"
#include "grid_device.hpp"
#include <math.h>

namespace s3d {
namespace {

constexpr uint32_t kBlock = 256, kGroup = 4, kMaxLevelsHyper = 16;
constexpr uint32_t kMaxBlocks = 512;  // workgroups of the backward (two per CU): one fp32 partial each

struct alignas(16) Half8 { _Float16 v[8]; };

// An fp32 value pinned in a register before it is rounded to binary16 (dnerf.hip): "round the fp32 product, then round that to
// half" is what k_grid_forward's v_mul_f32 + v_cvt_pk_f16_f32 do; without the pin the compiler may pick v_fma_mixlo_f16, which
// rounds the exact product to half once — another value in ~10^-4 of the cases.
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
    constexpr uint32_t D = 4, C = 2, NC = 1u << D, GD = D - 1;  // GD: the ambient dimension
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
    T res[kGroup][C], jac[kGroup][C];
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
#pragma unroll
        for (uint32_t c = 0; c < C; c++) { res[k][c] = Acc<T>::zero(); jac[k][c] = Acc<T>::zero(); }
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

        // Does the ambient coordinate enter this level's index?  (level-uniform)  get_grid_index stops adding coordinates once
        // stride > hashmap_size (gridencoder.cu:72); a tiled level past that point addresses the same row for both ambient corners
        // of a pair: eight gathers, each used twice — the same bits.  (A hash level whose strides overflow hashes all four.)
        uint32_t stride = 1;
#pragma unroll
        for (uint32_t d = 0; d < GD; d++)
            if (stride <= hashmap_size) stride *= a.align_corners ? resolution : (resolution + 1);
        const bool shared_rows = a.gridtype == 1 && stride > hashmap_size;

        T feat[NC][C];
        float wts[NC];
#pragma unroll
        for (uint32_t idx = 0; idx < NC; idx++) {
            float w = 1;
#pragma unroll
            for (uint32_t d = 0; d < D; d++) {
                if ((idx & (1u << d)) == 0) w *= 1 - pos[d];
                else w *= pos[d];
            }
            wts[idx] = w;
        }
        auto gather = [&](uint32_t idx) {
            uint32_t pgl[D];
#pragma unroll
            for (uint32_t d = 0; d < D; d++) pgl[d] = pos_grid[d] + ((idx >> d) & 1u);
            const uint32_t row = grid_row<D>(a.gridtype, a.align_corners, hashmap_size, resolution, pgl);
            load_feat<T, C>(table + (size_t)row * C, feat[idx]);
        };
        if (shared_rows) {
#pragma unroll
            for (uint32_t idx = 0; idx < NC / 2; idx++) gather(idx);
#pragma unroll
            for (uint32_t idx = 0; idx < NC / 2; idx++) {
#pragma unroll
                for (uint32_t c = 0; c < C; c++) feat[idx + NC / 2][c] = feat[idx][c];
            }
        } else {
#pragma unroll
            for (uint32_t idx = 0; idx < NC; idx++) gather(idx);
        }
#pragma unroll
        for (uint32_t idx = 0; idx < NC; idx++) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) res[k][c] = feat_fma<T>(wts[idx], feat[idx][c], res[k][c]);
        }
        if (a.dy_da) {  // gridencoder.cu:198-241 for gd = 3; corner idx = bit d of dimension d, so the pair is (corner, corner | 8)
#pragma unroll
            for (uint32_t idx = 0; idx < NC / 2; idx++) {
                float w = scale;
#pragma unroll
                for (uint32_t d = 0; d < GD; d++) {
                    if ((idx & (1u << d)) == 0) w *= 1 - pos[d];
                    else w *= pos[d];
                }
#pragma unroll
                for (uint32_t c = 0; c < C; c++) {
                    const float diff = Acc<T>::to_f(Acc<T>::sub(feat[idx | (1u << GD)][c], feat[idx][c]));
                    if constexpr (sizeof(T) == 2) jac[k][c] = Acc<T>::add(jac[k][c], Acc<T>::from_f(pinned(w * diff * pos_deriv[GD])));
                    else jac[k][c] = Acc<T>::from_f(__builtin_fmaf(w * diff, pos_deriv[GD], Acc<T>::to_f(jac[k][c])));
                }
            }
        }
    }

    // the features as the fp16 columns 2 l, 2 l + 1 of the row (an fp32 sum is rounded to binary16 once: pinned first)
    _Float16* frow = a.feat + (size_t)b * a.L * C + l0 * C;
    Half8 o;
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            if constexpr (sizeof(T) == 2) { __half h = res[k][c]; __builtin_memcpy(&o.v[k * C + c], &h, 2); }
            else o.v[k * C + c] = (_Float16)pinned(res[k][c]);
        }
    }
    const bool whole = a.L % kGroup == 0;  // rows of whole 16-byte words; else (a ragged last group) rows of 4 L bytes: 4-byte stores
    if (whole) *reinterpret_cast<Half8*>(frow) = o;
    else {  // (every index below is a compile-time constant: the arrays stay in registers)
#pragma unroll
        for (uint32_t k = 0; k < kGroup; k++) {
            if (l0 + k >= a.L) continue;
            uint32_t word;
            __builtin_memcpy(&word, &o.v[k * C], 4);
            *reinterpret_cast<uint32_t*>(frow + k * C) = word;
        }
    }
    if (a.dy_da) {
        T* j = a.dy_da + ((size_t)b * a.L + l0) * C;
        if (whole) {  // 16 B (fp16) / 32 B (fp32) per lane
            constexpr uint32_t NW = kGroup * C * sizeof(T) / 16;
            uint4 w[NW];
            __builtin_memcpy(w, jac, sizeof(w));
#pragma unroll
            for (uint32_t i = 0; i < NW; i++) reinterpret_cast<uint4*>(j)[i] = w[i];
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kGroup; k++)
                if (l0 + k < a.L) store_feat<T, C>(j + k * C, jac[k]);
        }
    }
}

// One lane = one row: the row's 2 L gradient columns go to the L level planes (consecutive lanes are consecutive rows, so every
// plane's stores are contiguous), and the row's term of grad_ambient is the fp32 chain over its columns in ascending order.
template <typename T>
__global__ void __launch_bounds__(kBlock) k_dnerf_hyper_backward(const _Float16* __restrict__ g_feat, const T* __restrict__ dy_da,
                                                                 uint32_t B, uint32_t L, float grad_scale, T* __restrict__ out,
                                                                 float* __restrict__ grad_ambient, float* partials, uint32_t* ticket,
                                                                 const int32_t* __restrict__ n_valid) {
    constexpr uint32_t C = 2;
    __shared__ float part[kBlock / 64];
    __shared__ uint32_t is_last;
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
#pragma unroll
            for (uint32_t k = 0; k < kGroup; k++) {
                const uint32_t l = l0 + k;
                if (l >= L) continue;
                T v[C];
                if constexpr (sizeof(T) == 2) __builtin_memcpy(v, &gv.v[k * C], 4);
                else { v[0] = (float)gv.v[k * C]; v[1] = (float)gv.v[k * C + 1]; }
                store_feat<T, C>(out + ((size_t)l * B + b) * C, v);
                if (jrow) {
                    T j[C];
                    load_feat<T, C>(jrow + l * C, j);
#pragma unroll
                    for (uint32_t c = 0; c < C; c++) acc = __builtin_fmaf((float)gv.v[k * C + c], Acc<T>::to_f(j[c]), acc);
                }
            }
        }
        sum += acc;
    }
    if (!grad_ambient) return;  // (workgroup-uniform)
    // lanes by an exchange tree, waves in index order, workgroups in a fixed order by the last one to arrive
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_down(sum, o, 64);
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        float v = part[0];
        for (uint32_t w = 1; w < kBlock / 64; w++) v += part[w];
        // The partial is a write-through (agent-scope atomic) store, drained by the lane that made it before it takes the ticket:
        // no release fence, which would write back the grad_levels rows this workgroup has just left in its XCD's L2
        // (dnerf_basis.hip).  The last workgroup acquires and reads the partials past its L1.
        __hip_atomic_store(partials + blockIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t arrived = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = arrived == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        is_last = last ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;  // (workgroup-uniform)
    // lane i: the partials of workgroups i, i + 256 in index order; then the tree, the waves in order
    float v = 0.0f;
    for (uint32_t i = threadIdx.x; i < gridDim.x; i += kBlock)
        v += __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) part[wave] = v;  // (every read of `part` above lies before the barrier in front of `is_last`)
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = part[0];
        for (uint32_t w = 1; w < kBlock / 64; w++) r += part[w];
        *grad_ambient = r * grad_scale;
        *ticket = 0u;
    }
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
    return 16 + sizeof(float) * (size_t)backward_blocks(B);
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
    S3D_REQUIRE(!sum || (workspace && workspace_bytes >= s3d_dnerf_hyper_backward_workspace_size(B) && (uintptr_t)workspace % 16 == 0),
                "dnerf_hyper_grid_backward: grad_ambient needs a workspace of s3d_dnerf_hyper_backward_workspace_size(B) bytes");
    uint32_t* ticket = nullptr;
    float* partials = nullptr;
    if (sum) {
        ticket = (uint32_t*)workspace;
        partials = (float*)((char*)workspace + 16);
        S3D_HIP(hipMemsetAsync(ticket, 0, 16, st));
    }
    const dim3 grid(backward_blocks(B)), block(kBlock);
    if (dtype == S3D_F16)
        hipLaunchKernelGGL((k_dnerf_hyper_backward<__half>), grid, block, 0, st, (const _Float16*)grad_feat,
                           sum ? (const __half*)dy_da : nullptr, B, L, grad_scale, (__half*)grad_levels, sum ? grad_ambient : nullptr,
                           partials, ticket, n_valid);
    else
        hipLaunchKernelGGL((k_dnerf_hyper_backward<float>), grid, block, 0, st, (const _Float16*)grad_feat,
                           sum ? (const float*)dy_da : nullptr, B, L, grad_scale, (float*)grad_levels, sum ? grad_ambient : nullptr,
                           partials, ticket, n_valid);
    return check_launch("dnerf_hyper_grid_backward");
}
