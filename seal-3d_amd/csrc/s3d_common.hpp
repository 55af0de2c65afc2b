// s3d_common.hpp — shared device/host helpers for libseal3d_hip (gfx950 only).
//
// Arithmetic contract: the library is built with -ffp-contract=off and
// every fused multiply-add is spelled __builtin_fmaf, mirroring the CPU oracle
// expression by expression, so integer/index results (cell coordinates, hash rows,
// per-ray sample counts, span offsets) are bit-identical to the oracle.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <atomic>
#include <stdio.h>
#include <string.h>

#include "../../include/seal3d_hip.h"

#define S3D_EXPORT extern "C" __attribute__((visibility("default")))

namespace s3d {

void set_error(const char* fmt, ...);

inline hipStream_t as_stream(s3d_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return S3D_ERR_HIP;
    }
    return S3D_OK;
}

#define S3D_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            s3d::set_error(__VA_ARGS__);  \
            return S3D_ERR_INVALID;       \
        }                                 \
    } while (0)

#define S3D_HIP(call)                                                        \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) {                                             \
            s3d::set_error("%s: %s", #call, hipGetErrorString(e__));         \
            return S3D_ERR_HIP;                                              \
        }                                                                    \
    } while (0)

// One-time per-device kernel attribute setup (dynamic LDS opt-in): `flags` is a per-call-site static, one bit per device
// ordinal, so a second GPU in the same process gets its own hipFuncSetAttribute calls and concurrent host threads at worst
// repeat an idempotent call.
inline bool device_needs_setup(std::atomic<uint64_t>& flags, int* dev_out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) { *dev_out = -1; return true; }
    *dev_out = dev;
    return ((flags.load(std::memory_order_acquire) >> dev) & 1ull) == 0;
}
inline void device_setup_done(std::atomic<uint64_t>& flags, int dev) {
    if (dev >= 0) flags.fetch_or(1ull << dev, std::memory_order_release);
}

// CUs of the current device, cached per device ordinal (resident-workgroup counts of the persistent kernels)
inline uint32_t device_cus() {
    static std::atomic<uint32_t> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return 256;
    uint32_t n = cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        int v = 0;
        n = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? (uint32_t)v : 256u;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

template <typename T>
__host__ __device__ inline T div_up(T a, T b) { return (a + b - 1) / b; }

// 256 CUs x 8 resident blocks: cap for grid-stride launches of streaming kernels.
constexpr uint32_t kMaxStreamBlocks = 2048;

inline uint32_t stream_grid(uint64_t work, uint32_t block) {
    uint64_t g = div_up<uint64_t>(work, block);
    if (g > kMaxStreamBlocks) g = kMaxStreamBlocks;
    if (g == 0) g = 1;
    return (uint32_t)g;
}

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }

// raymarching.cu:near_far_from_aabb — slab test against the box, near clamped to min_near; a miss gives FLT_MAX twice
__device__ __forceinline__ void near_far_of(const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t n,
                                            const float (&a)[6], float min_near, float& near_out, float& far_out) {
    const float ox = rays_o[n * 3], oy = rays_o[n * 3 + 1], oz = rays_o[n * 3 + 2];
    const float rdx = 1 / rays_d[n * 3], rdy = 1 / rays_d[n * 3 + 1], rdz = 1 / rays_d[n * 3 + 2];
    float near = (a[0] - ox) * rdx, far = (a[3] - ox) * rdx;
    if (near > far) { float t = near; near = far; far = t; }
    float near_y = (a[1] - oy) * rdy, far_y = (a[4] - oy) * rdy;
    if (near_y > far_y) { float t = near_y; near_y = far_y; far_y = t; }
    bool miss = (near > far_y || near_y > far);
    if (!miss) {
        if (near_y > near) near = near_y;
        if (far_y < far) far = far_y;
        float near_z = (a[2] - oz) * rdz, far_z = (a[5] - oz) * rdz;
        if (near_z > far_z) { float t = near_z; near_z = far_z; far_z = t; }
        miss = (near > far_z || near_z > far);
        if (!miss) {
            if (near_z > near) near = near_z;
            if (far_z < far) far = far_z;
            if (near < min_near) near = min_near;
        }
    }
    near_out = miss ? 3.402823466e+38f : near;
    far_out = miss ? 3.402823466e+38f : far;
}

// Padded sample batches (`n_valid` of seal3d_hip.h): the ray marcher leaves the number of samples it produced in device
// memory, the buffers behind it have a static extent B.  Rows [round_up(*n_valid, 128), B) are absent for every kernel
// that takes the pointer — not read, not written — so the work follows the samples while launch geometry and strides
// (level-major layouts) stay those of B.  NULL = all B rows.
__device__ __forceinline__ uint32_t valid_rows(uint32_t B, const int32_t* n_valid) {
    if (!n_valid) return B;
    const int32_t n = *n_valid;
    const uint32_t v = n <= 0 ? 0u : (((uint32_t)n + 127u) & ~127u);
    return v < B ? v : B;
}

// lane id inside the 64-wide wavefront
__device__ __forceinline__ uint32_t lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// inclusive wave64 prefix sum (shuffle-up ladder; DPP row_shr/bcast is what hipcc lowers it to)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}

// counter-based random numbers with the step number read from device memory, so that a graph-replayed launch draws fresh
// values (torch.rand inside a captured graph costs its own kernel plus two seed/offset fills before every replay):
// hash_u32(key, step, n) is a full 32-bit word, ray_noise its top 24 bits as a uniform in [0, 1) (the marcher's per-ray jitter)
__device__ __forceinline__ uint32_t pcg_hash(uint32_t v) {
    v = v * 747796405u + 2891336453u;
    const uint32_t w = ((v >> ((v >> 28u) + 4u)) ^ v) * 277803737u;
    return (w >> 22u) ^ w;
}
__device__ __forceinline__ uint32_t hash_u32(uint32_t key, uint32_t step, uint32_t n) {
    return pcg_hash(pcg_hash(key ^ (step * 0x9E3779B9u)) + n);
}
__device__ __forceinline__ float ray_noise(uint32_t key, uint32_t step, uint32_t n) {
    return (float)(hash_u32(key, step, n) >> 8) * (1.0f / 16777216.0f);  // [0, 1)
}

}  // namespace s3d
