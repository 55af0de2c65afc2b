// grid_device.hpp — device helpers of the hash / tiled grid encoding (gridencoder.cu:23-84 of the reference: index plan,
// corner location, per-level scales, feature loads, accumulators), shared by gridencoder.hip and background.hip so that
// every kernel that reads a grid table forms its corner rows, weights and sums with the same expressions.
#pragma once
#include "s3d_common.hpp"
#include <math.h>

namespace s3d {
namespace {

constexpr uint32_t kMaxLevels = 32;
// per-level scales + the optional input normalisation of GridEncoder.forward (grid.py:146: x01 = (x + bound) / (2 bound),
// evaluated as torch's GPU kernels do: one add, one multiply by the fp32 reciprocal); bound = 0: inputs are already in [0,1]
struct LevelScales {
    float v[kMaxLevels];
    float bound, inv_2bound;
    const int32_t* n_valid;   // see valid_rows()
    const float* live;        // forward only: rows with live[b * live_stride] == 0 are written as zeros, table untouched
    uint32_t live_stride;
};

constexpr uint32_t kPrimes[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};

template <uint32_t D>
__device__ __forceinline__ uint32_t grid_row(uint32_t gridtype, bool align_corners, uint32_t hashmap_size,
                                             uint32_t resolution, const uint32_t (&pg)[D]) {
    uint32_t stride = 1, index = 0;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        if (stride <= hashmap_size) {
            index += pg[d] * stride;
            stride *= align_corners ? resolution : (resolution + 1);
        }
    }
    if (gridtype == 0 && stride > hashmap_size) {
        uint32_t r = 0;
#pragma unroll
        for (uint32_t i = 0; i < D; i++) r ^= pg[i] * kPrimes[i];
        index = r;
    }
    // `index % hashmap_size` without the ~25-instruction division by a run-time value on the paths that never need it:
    // hashed levels have power-of-two sizes (a mask), dense rows lie below the size (nothing to do); what is left (tiled
    // grids whose strides overflow the table) divides
    const uint32_t mask = hashmap_size - 1;
    if ((hashmap_size & mask) == 0) return index & mask;
    if (__builtin_expect(index >= hashmap_size, 0)) index %= hashmap_size;
    return index;
}

// Level-uniform index plan (get_grid_index, gridencoder.cu:66-84): which dimensions enter the dense index (the
// stride loop stops once stride > hashmap_size), their strides, whether the level is hashed; `% hashmap_size` is a
// mask for power-of-two sizes and a no-op for dense rows below the size.  Same rows as grid_row, fewer divisions.
template <uint32_t D>
struct LevelIndex {
    uint32_t mul[D];  // per-dimension multiplier: prime (hashed) or stride (dense; 0 = dimension dropped)
    uint32_t size, mask;
    bool hashed, pow2, need_mod;
    __device__ __forceinline__ void init(uint32_t gridtype, bool align_corners, uint32_t hashmap_size, uint32_t resolution) {
        uint32_t st = 1;
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            if (st <= hashmap_size) { mul[d] = st; st *= align_corners ? resolution : (resolution + 1); }
            else mul[d] = 0;
        }
        hashed = (gridtype == 0 && st > hashmap_size);
        if (hashed) {
#pragma unroll
            for (uint32_t d = 0; d < D; d++) mul[d] = kPrimes[d];
        }
        size = hashmap_size;
        mask = hashmap_size - 1;
        pow2 = (hashmap_size & mask) == 0;
        // can a dense index reach the table size at all?  (cell coordinates are <= resolution + 1)
        unsigned long long top = 0;
#pragma unroll
        for (uint32_t d = 0; d < D; d++) top += (unsigned long long)(resolution + 1) * mul[d];
        need_mod = hashed || top >= hashmap_size;
    }
    __device__ __forceinline__ uint32_t row(const uint32_t (&lo)[D], uint32_t idx) const {  // lo[d] = pos_grid[d] * mul[d]
        uint32_t index = 0;
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            const uint32_t t = ((idx >> d) & 1u) ? lo[d] + mul[d] : lo[d];
            index = hashed ? (index ^ t) : (index + t);
        }
        if (pow2) return index & mask;
        if (!need_mod) return index;  // (wave-uniform: dense levels skip the division by a run-time value altogether)
        return index < size ? index : index % size;
    }
};

// ---- feature vector load/store: one memory instruction per corner ----
template <typename T, uint32_t C> struct FeatVec;
template <> struct FeatVec<float, 1> { using type = float; };
template <> struct FeatVec<float, 2> { using type = float2; };
template <> struct FeatVec<float, 4> { using type = float4; };
template <> struct FeatVec<float, 8> { struct alignas(16) type { float4 a, b; }; };
template <> struct FeatVec<__half, 1> { using type = __half; };
template <> struct FeatVec<__half, 2> { using type = __half2; };
template <> struct FeatVec<__half, 4> { struct alignas(8) type { __half2 a, b; }; };
template <> struct FeatVec<__half, 8> { struct alignas(16) type { __half2 a, b, c, d; }; };

template <typename T, uint32_t C>
__device__ __forceinline__ void load_feat(const T* __restrict__ p, T (&out)[C]) {
    using V = typename FeatVec<T, C>::type;
    static_assert(sizeof(V) == sizeof(T) * C, "vector size");
    const V v = *reinterpret_cast<const V*>(p);
    __builtin_memcpy(out, &v, sizeof(V));
}
template <typename T, uint32_t C>
__device__ __forceinline__ void store_feat(T* __restrict__ p, const T (&in)[C]) {
    using V = typename FeatVec<T, C>::type;
    V v;
    __builtin_memcpy(&v, in, sizeof(V));
    *reinterpret_cast<V*>(p) = v;
}

template <typename T> struct Acc;
template <> struct Acc<float> {
    static __device__ __forceinline__ float zero() { return 0.0f; }
    // results += w * g  (fused, as nvcc contracts it)
    static __device__ __forceinline__ float fma(float w, float g, float acc) { return __builtin_fmaf(w, g, acc); }
    static __device__ __forceinline__ float sub(float a, float b) { return a - b; }
    static __device__ __forceinline__ float to_f(float a) { return a; }
    static __device__ __forceinline__ float from_f(float a) { return a; }
    static __device__ __forceinline__ float mul(float a, float b) { return a * b; }
    static __device__ __forceinline__ float add(float a, float b) { return a + b; }
};
template <> struct Acc<__half> {
    static __device__ __forceinline__ __half zero() { return __float2half(0.0f); }
    // at::Half += float : the float product is rounded to half, then a half add (gridencoder.cu:184)
    static __device__ __forceinline__ __half fma(float w, __half g, __half acc) {
        return __hadd(acc, __float2half(w * __half2float(g)));
    }
    static __device__ __forceinline__ __half sub(__half a, __half b) { return __hsub(a, b); }
    static __device__ __forceinline__ float to_f(__half a) { return __half2float(a); }
    static __device__ __forceinline__ __half from_f(float a) { return __float2half(a); }
    static __device__ __forceinline__ __half mul(__half a, __half b) { return __hmul(a, b); }
    static __device__ __forceinline__ __half add(__half a, __half b) { return __hadd(a, b); }
};

template <uint32_t D>
__device__ __forceinline__ bool load_point(const float* __restrict__ inputs, uint32_t b, const LevelScales& sc, float (&x)[D]) {
    bool oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        x[d] = inputs[(size_t)b * D + d];
        if (sc.bound != 0.0f) x[d] = (x[d] + sc.bound) * sc.inv_2bound;
        if (x[d] < 0 || x[d] > 1) oob = true;
    }
    return oob;
}

template <uint32_t D>
__device__ __forceinline__ void locate(const float (&x)[D], float scale, bool align_corners, uint32_t interp,
                                       float (&pos)[D], float (&pos_deriv)[D], uint32_t (&pos_grid)[D]) {
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        pos[d] = __builtin_fmaf(x[d], scale, align_corners ? 0.0f : 0.5f);
        pos_grid[d] = (uint32_t)floorf(pos[d]);
        pos[d] -= (float)pos_grid[d];
        if (interp == 1) {
            pos_deriv[d] = 6 * pos[d] * (1.0f - pos[d]);
            pos[d] = pos[d] * pos[d] * __builtin_fmaf(-2.0f, pos[d], 3.0f);
        }
    }
}

void host_scales(uint32_t L, float S, uint32_t H, LevelScales& out, float bound = 0.0f, const int32_t* n_valid = nullptr) {
    out.n_valid = n_valid;
    out.live = nullptr;
    out.live_stride = 0;
    out.bound = bound;
    out.inv_2bound = bound != 0.0f ? 1.0f / (2.0f * bound) : 0.0f;
    for (uint32_t l = 0; l < kMaxLevels; l++) out.v[l] = 0.0f;
    for (uint32_t l = 0; l < L; l++) out.v[l] = fmaf(exp2f((float)l * S), (float)H, -1.0f);
}

}  // namespace
}  // namespace s3d
