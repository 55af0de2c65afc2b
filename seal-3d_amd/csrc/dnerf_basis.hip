// dnerf_basis.hip — the density head of the D-NeRF temporal-basis backbone (dnerf/network_basis.py:139-152 of the reference:
// `sigma = trunc_exp(h[..., :32] @ sigma_basis); geo = h[..., 32:]; d = SH(d); colour-net input = cat[d, geo]`) for gfx950.
// In torch that is a slice, a matrix-vector product, exp, SH, cat with type promotion, a half cast and their backward nodes, each a
// pass over [M, 32..64] activations; here it is one streaming kernel per direction with the same rounding points:
//   mid forward : h [B,64] f16, dirs [B,3] f32, sb [32] f16 -> sigma [B] f32 = exp(float(half(sum_k h_k sb_k)))
//                                                             cin [B,48] f16 = [half(SH_4(d)) | h32..h63]
//   mid backward: d_cin [B,48] f16, d_sigma [B] f32, h, sb  -> d_h [B,64] f16 = [half(float(gh) sb_k) | d_cin[16..47]],
//                                                             gh = half(d_sigma exp(clamp(pre, -15, 15)))
//                                                             d_sb [32] f32 = sum_b float(gh_b) float(h_bk)
// One lane = one row; every lane reads / writes whole 16-byte pieces of its rows.  The 32-column sum of the backward runs over a
// grid of fixed size: per-lane running sums over the row stride gridDim.x * 256, one exchange tree per wave, the waves of a
// workgroup in index order, the workgroups' partials in index order by the last one to arrive (the hand-over and the workspace
// are those of csrc/ordered_sum.hpp; the 32-column fold and the striped last sum are this file's): no float atomics, the same bits
// on every run for the same B.
#include "s3d_common.hpp"
#include "sh_eval.hpp"
#include "grid_group.hpp"
#include "ordered_sum.hpp"

namespace s3d {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr uint32_t kBasis = 32, kRow = 64, kCin = 48, kBlock = kSumBlock;
constexpr uint32_t kMaxBlocks = 512;   // workgroups of the backward (two per CU): the partials are kMaxBlocks x 32 floats
constexpr uint32_t kStripes = kBlock / kBasis;  // 8 lanes per column in the last workgroup's sum
constexpr uint32_t kBatch = 16;                 // partials a lane of the last workgroup has in flight

struct Basis { float v[kBasis]; };

__device__ __forceinline__ Basis load_basis(const _Float16* __restrict__ sb) {
    Basis s;
#pragma unroll
    for (uint32_t q = 0; q < kBasis / 8; q++) {
        const h8 w = reinterpret_cast<const h8*>(sb)[q];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) s.v[8 * q + i] = (float)w[i];
    }
    return s;
}

// pre = float(half(sum)): the fp32 chain fmaf(h_k, sb_k, acc) for k = 0..31 ascending from 0, rounded to binary16 once (what an
// fp16 matmul with fp32 accumulation hands back; `pinned`, csrc/grid_group.hpp: two roundings, not one v_fma_mixlo_f16)
__device__ __forceinline__ float basis_pre(const h8 (&hv)[kBasis / 8], const Basis& s) {
    float acc = 0.0f;
#pragma unroll
    for (uint32_t q = 0; q < kBasis / 8; q++) {
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) acc = __builtin_fmaf((float)hv[q][i], s.v[8 * q + i], acc);
    }
    return (float)(_Float16)pinned(acc);
}

__global__ void __launch_bounds__(kBlock) k_basis_mid_forward(const _Float16* __restrict__ h, const float* __restrict__ dirs,
                                                              const _Float16* __restrict__ sb, uint32_t B, ShNorm K,
                                                              float* __restrict__ sigma, _Float16* __restrict__ cin,
                                                              const int32_t* __restrict__ n_valid) {
    const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= valid_rows(B, n_valid)) return;
    const Basis s = load_basis(sb);
    const h8* row = reinterpret_cast<const h8*>(h + (size_t)b * kRow);
    h8 hv[kBasis / 8];
#pragma unroll
    for (uint32_t q = 0; q < kBasis / 8; q++) hv[q] = row[q];
    sigma[b] = expf(basis_pre(hv, s));  // activation.py:8-11
    if (!cin) return;                   // (density(): sigma alone)
    const float x = dirs[(size_t)b * 3], y = dirs[(size_t)b * 3 + 1], z = dirs[(size_t)b * 3 + 2];
    float o[16], j0[1], j1[1], j2[1];
    sh_eval<4, false>(x, y, z, K, o, j0, j1, j2);
    h8 c0, c1;
#pragma unroll
    for (int i = 0; i < 8; i++) { c0[i] = (_Float16)o[i]; c1[i] = (_Float16)o[8 + i]; }
    h8* dst = reinterpret_cast<h8*>(cin + (size_t)b * kCin);
    dst[0] = c0; dst[1] = c1;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) dst[2 + q] = row[4 + q];
}

// One step of the 32-column sum across a wave: a lane keeps one half of its 2 HALF columns and hands the other half to the lane 2 HALF
// away, so that 32 sums over 64 lanes take 16 + 8 + 4 + 2 + 1 exchanges and one last add, not 32 x 6.  Behind the five steps lane l
// holds column (l >> 1) & 31, summed over the lanes that agree with it in bit 0.  The order of the additions is fixed by the lane
// numbers alone.
template <uint32_t HALF>
__device__ __forceinline__ void fold_step(float (&acc)[kBasis], uint32_t lane) {
    const bool upper = (lane & (2 * HALF)) != 0;
#pragma unroll
    for (uint32_t i = 0; i < HALF; i++) {
        const float keep = upper ? acc[i + HALF] : acc[i];
        const float send = upper ? acc[i] : acc[i + HALF];
        acc[i] = keep + __shfl_xor(send, 2 * HALF, 64);
    }
}

__global__ void __launch_bounds__(kBlock) k_basis_mid_backward(const _Float16* __restrict__ d_cin, const float* __restrict__ d_sigma,
                                                               const _Float16* __restrict__ h, const _Float16* __restrict__ sb,
                                                               uint32_t B, _Float16* __restrict__ d_h, float* __restrict__ d_sb,
                                                               float* partials, uint32_t* ticket,
                                                               const int32_t* __restrict__ n_valid) {
    __shared__ float part[kStripes][kBasis];  // (kBlock / 64 = 4 waves' sums first, then the 8 stripes of the last workgroup)
    __shared__ SumShared sh;  // (the hand-over's flag)
    const uint32_t Bv = valid_rows(B, n_valid);
    const Basis s = load_basis(sb);
    float acc[kBasis];
#pragma unroll
    for (uint32_t k = 0; k < kBasis; k++) acc[k] = 0.0f;
    for (uint32_t b = blockIdx.x * kBlock + threadIdx.x; b < Bv; b += gridDim.x * kBlock) {
        h8* dst = reinterpret_cast<h8*>(d_h + (size_t)b * kRow);
        const h8* gsrc = reinterpret_cast<const h8*>(d_cin + (size_t)b * kCin + 16);
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) dst[4 + q] = gsrc[q];
        if (!d_sigma) {
            h8 zero;
#pragma unroll
            for (int i = 0; i < 8; i++) zero[i] = (_Float16)0.0f;
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) dst[q] = zero;
            continue;
        }
        const h8* row = reinterpret_cast<const h8*>(h + (size_t)b * kRow);
        h8 hv[kBasis / 8];
#pragma unroll
        for (uint32_t q = 0; q < kBasis / 8; q++) hv[q] = row[q];
        const float pre = basis_pre(hv, s);
        const float g = d_sigma[b] * expf(fminf(15.0f, fmaxf(-15.0f, pre)));  // activation.py:13-16
        const float gh = (float)(_Float16)pinned(g);
#pragma unroll
        for (uint32_t q = 0; q < kBasis / 8; q++) {
            h8 o;
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) {
                o[i] = (_Float16)(gh * s.v[8 * q + i]);  // (a product of two halves: exact in fp32, one rounding to half)
                acc[8 * q + i] = __builtin_fmaf(gh, (float)hv[q][i], acc[8 * q + i]);
            }
            dst[q] = o;
        }
    }
    if (!d_sb) return;  // (workgroup-uniform)
    // lanes by an exchange tree, waves in index order, workgroups in a fixed order by the last one to arrive
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    fold_step<16>(acc, lane); fold_step<8>(acc, lane); fold_step<4>(acc, lane); fold_step<2>(acc, lane); fold_step<1>(acc, lane);
    acc[0] += __shfl_xor(acc[0], 1, 64);
    if ((lane & 1u) == 0) part[wave][lane >> 1] = acc[0];
    __syncthreads();
    if (threadIdx.x < kBasis) {  // (wave 0: the lanes that store the partials and the lane that takes the ticket are one wave)
        float v = part[0][threadIdx.x];
        for (uint32_t w = 1; w < kBlock / 64; w++) v += part[w][threadIdx.x];
        __hip_atomic_store(partials + (size_t)blockIdx.x * kBasis + threadIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // (write-through partials and no release fence, which would write back the 32 KB of grad_h rows this workgroup has just left
    // in its XCD's L2: profiles/dnerf_basis.md)
    if (!ordered_sum_arrive(ticket, gridDim.x, sh)) return;  // (workgroup-uniform)
    // column k = tid % 32, stripe j = tid / 32: the partials of workgroups j, j + 8, ... in index order, then the stripes in order
    const uint32_t k = threadIdx.x % kBasis, j = threadIdx.x / kBasis;
    float v = 0.0f;
    for (uint32_t i = j; i < gridDim.x; i += kStripes * kBatch) {  // (kBatch loads in flight, then their additions in index order)
        float t[kBatch];
#pragma unroll
        for (uint32_t u = 0; u < kBatch; u++) {
            const uint32_t w = i + u * kStripes;
            t[u] = w < gridDim.x ? __hip_atomic_load(partials + (size_t)w * kBasis + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
        }
#pragma unroll
        for (uint32_t u = 0; u < kBatch; u++) v += t[u];
    }
    part[j][k] = v;  // (every read of `part` above lies before the barrier of the hand-over)
    __syncthreads();
    if (threadIdx.x < kBasis) {
        float r = part[0][threadIdx.x];
        for (uint32_t q = 1; q < kStripes; q++) r += part[q][threadIdx.x];
        d_sb[threadIdx.x] = r;
    }
    if (threadIdx.x == 0) *ticket = 0u;
}

inline uint32_t backward_blocks(uint32_t B) { return std::min<uint32_t>(kMaxBlocks, std::max<uint32_t>(1u, div_up<uint32_t>(B, kBlock))); }

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT int s3d_dnerf_basis_mid_forward(const uint16_t* h, const float* dirs, const uint16_t* sigma_basis, uint32_t B, float* sigma,
                                           uint16_t* color_in, const int32_t* n_valid, s3d_stream_t stream) {
    if (B == 0) return S3D_OK;
    S3D_REQUIRE(h && sigma_basis && sigma && (dirs || !color_in), "dnerf_basis_mid_forward: null pointer");
    S3D_REQUIRE(((uintptr_t)h | (uintptr_t)sigma_basis | (uintptr_t)color_in) % 16 == 0,
                "dnerf_basis_mid_forward: h, sigma_basis and color_in must be 16-byte aligned");
    ShNorm K;
    host_sh_norm(4, K);
    hipLaunchKernelGGL(k_basis_mid_forward, dim3(div_up<uint32_t>(B, kBlock)), dim3(kBlock), 0, as_stream(stream), (const _Float16*)h, dirs,
                       (const _Float16*)sigma_basis, B, K, sigma, (_Float16*)color_in, n_valid);
    return check_launch("dnerf_basis_mid_forward");
}

S3D_EXPORT size_t s3d_dnerf_basis_mid_workspace_size(uint32_t B) {
    return SumWorkspace::bytes((size_t)kBasis * backward_blocks(B));
}

S3D_EXPORT int s3d_dnerf_basis_mid_backward(const uint16_t* grad_color_in, const float* grad_sigma, const uint16_t* h,
                                            const uint16_t* sigma_basis, uint32_t B, uint16_t* grad_h, float* grad_sigma_basis,
                                            void* workspace, size_t workspace_bytes, const int32_t* n_valid, s3d_stream_t stream) {
    hipStream_t st = as_stream(stream);
    if (B == 0 || !grad_sigma) {
        if (grad_sigma_basis) S3D_HIP(hipMemsetAsync(grad_sigma_basis, 0, kBasis * sizeof(float), st));
        if (B == 0) return S3D_OK;
    }
    S3D_REQUIRE(grad_color_in && h && sigma_basis && grad_h, "dnerf_basis_mid_backward: null pointer");
    S3D_REQUIRE(((uintptr_t)grad_color_in | (uintptr_t)h | (uintptr_t)sigma_basis | (uintptr_t)grad_h) % 16 == 0,
                "dnerf_basis_mid_backward: grad_color_in, h, sigma_basis and grad_h must be 16-byte aligned");
    const bool sum = grad_sigma && grad_sigma_basis;
    S3D_REQUIRE(!sum || SumWorkspace::fits(workspace, workspace_bytes, (size_t)kBasis * backward_blocks(B)),
                "dnerf_basis_mid_backward: grad_sigma_basis needs a workspace of s3d_dnerf_basis_mid_workspace_size(B) bytes");
    SumWorkspace ws;
    if (sum) S3D_HIP(ws.arm(workspace, st));
    hipLaunchKernelGGL(k_basis_mid_backward, dim3(backward_blocks(B)), dim3(kBlock), 0, st, (const _Float16*)grad_color_in, grad_sigma,
                       (const _Float16*)h, (const _Float16*)sigma_basis, B, (_Float16*)grad_h, sum ? grad_sigma_basis : nullptr, ws.partials,
                       ws.ticket, n_valid);
    return check_launch("dnerf_basis_mid_backward");
}
