// grid_group.hpp — the grid lookup of the D-NeRF kernels that write fp16 network rows (csrc/dnerf.hip for D = 3, csrc/dnerf_hyper.hip
// for D = 4): a workgroup serves kGroup = 4 levels of 256 rows, so that a lane's features of those levels are eight consecutive
// fp16 columns of its row (one 16-byte store).  Rows, weights and sums are k_grid_forward's (csrc/gridencoder.hip), expression by
// expression, through grid_device.hpp; the Jacobian columns are formed from the corners the value has already fetched.  Two
// features per level.  Every array index below is a compile-time constant once the callers' loops are unrolled: the arrays stay
// in registers.
#pragma once
#include "grid_device.hpp"

namespace s3d {
namespace {

constexpr uint32_t kGroup = 4, kGroupC = 2;

struct alignas(16) Half8 { _Float16 v[8]; };

// An fp32 value pinned in a register before it is rounded to binary16: "round the fp32 result, then round that to half" (what
// k_grid_forward's v_mul_f32 + v_cvt_pk_f16_f32 do) and "round the exact result to half once" (v_fma_mixlo_f16, which the compiler
// picks when it sees both steps) differ in one value in ~10^4.  An fp32 value that exists in a register rounds to half the same
// way whatever instruction converts it.
__device__ __forceinline__ float pinned(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
// the fp16 sums of grid_device.hpp's Acc<__half> with the product pinned
template <typename T>
__device__ __forceinline__ T feat_fma(float w, T g, T acc) {
    if constexpr (sizeof(T) == 2) return __hadd(acc, __float2half(pinned(w * __half2float(g))));
    else return Acc<T>::fma(w, g, acc);
}

template <typename T>
struct LevelTable {
    const T* table;
    uint32_t hashmap_size, resolution;
    float scale;
};
template <typename T>
__device__ __forceinline__ LevelTable<T> level_table(const T* grid, const int32_t* offsets, uint32_t level, float scale) {
    const uint32_t off = (uint32_t)offsets[level];
    return {grid + (size_t)off * kGroupC, (uint32_t)offsets[level + 1] - off, (uint32_t)ceilf(scale) + 1, scale};
}

// One level at x01: pos / pos_deriv, the 2^D corner rows in `feat` (corner idx = bit d of dimension d) and the value as the fp16
// columns 2 k, 2 k + 1 of `o` (an fp32 sum is rounded to binary16 once: pinned first).  `last_shared`: the last coordinate does
// not enter this level's index, so both of its corners of a pair address one row — gather half, copy half: the same bits.
template <uint32_t D, typename T>
__device__ __forceinline__ void level_value(const LevelTable<T>& lt, uint32_t gridtype, bool align_corners, uint32_t interp,
                                            const float (&x01)[D], bool last_shared, float (&pos)[D], float (&pos_deriv)[D],
                                            T (&feat)[1u << D][kGroupC], Half8& o, uint32_t k) {
    constexpr uint32_t NC = 1u << D;
    uint32_t pos_grid[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) pos_deriv[d] = (d == 0) ? 1.0f : 0.0f;  // `= {1.0f}`, gridencoder.cu:143
    locate<D>(x01, lt.scale, align_corners, interp, pos, pos_deriv, pos_grid);
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
        const uint32_t row = grid_row<D>(gridtype, align_corners, lt.hashmap_size, lt.resolution, pgl);
        load_feat<T, kGroupC>(lt.table + (size_t)row * kGroupC, feat[idx]);
    };
    if (last_shared) {
#pragma unroll
        for (uint32_t idx = 0; idx < NC / 2; idx++) gather(idx);
#pragma unroll
        for (uint32_t idx = 0; idx < NC / 2; idx++) {
#pragma unroll
            for (uint32_t c = 0; c < kGroupC; c++) feat[idx + NC / 2][c] = feat[idx][c];
        }
    } else {
#pragma unroll
        for (uint32_t idx = 0; idx < NC; idx++) gather(idx);
    }
    T res[kGroupC] = {Acc<T>::zero(), Acc<T>::zero()};
#pragma unroll
    for (uint32_t idx = 0; idx < NC; idx++) {
#pragma unroll
        for (uint32_t c = 0; c < kGroupC; c++) res[c] = feat_fma<T>(wts[idx], feat[idx][c], res[c]);
    }
#pragma unroll
    for (uint32_t c = 0; c < kGroupC; c++) {
        if constexpr (sizeof(T) == 2) __builtin_memcpy(&o.v[k * kGroupC + c], &res[c], 2);
        else o.v[k * kGroupC + c] = (_Float16)pinned(res[c]);
    }
}

// Column `gd` of the level's Jacobian, added to (j0, j1): gridencoder.cu:198-241 on the corner rows of level_value
template <uint32_t D, typename T>
__device__ __forceinline__ void jacobian_column(uint32_t gd, float scale, const float (&pos)[D], const float (&pos_deriv)[D],
                                                const T (&feat)[1u << D][kGroupC], T& j0, T& j1) {
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
        for (uint32_t c = 0; c < kGroupC; c++) {
            T& j = c == 0 ? j0 : j1;
            const float diff = Acc<T>::to_f(Acc<T>::sub(feat[corner | (1u << gd)][c], feat[corner][c]));
            if constexpr (sizeof(T) == 2) j = Acc<T>::add(j, Acc<T>::from_f(pinned(w * diff * pos_deriv[gd])));
            else j = Acc<T>::from_f(__builtin_fmaf(w * diff, pos_deriv[gd], Acc<T>::to_f(j)));
        }
    }
}

// The group's features as the eight fp16 columns at `row`.  `whole`: all four levels exist and `row` is 16-byte aligned — one
// store; else one 4-byte store for each of the `live` levels.
__device__ __forceinline__ void store_group_features(const Half8& o, _Float16* row, uint32_t live, bool whole) {
    if (whole) *reinterpret_cast<Half8*>(row) = o;
    else {
#pragma unroll
        for (uint32_t k = 0; k < kGroup; k++) {
            if (k >= live) continue;
            uint32_t word;
            __builtin_memcpy(&word, &o.v[k * kGroupC], 4);
            *reinterpret_cast<uint32_t*>(row + k * kGroupC) = word;
        }
    }
}

// The group's N Jacobian entries per level at j = base + (b L + l0) N: rows of L N entries, whole 16-byte words when L % 4 == 0
template <uint32_t N, typename T>
__device__ __forceinline__ void store_group_jacobian(const T (&jac)[kGroup][N], T* j, uint32_t L, uint32_t l0) {
    static_assert(N % kGroupC == 0 && kGroup * N * sizeof(T) % 16 == 0, "whole feature pairs, whole words");
    if (L % kGroup == 0) {
        constexpr uint32_t NW = kGroup * N * sizeof(T) / 16;
        uint4 w[NW];
        __builtin_memcpy(w, jac, sizeof(w));
#pragma unroll
        for (uint32_t i = 0; i < NW; i++) reinterpret_cast<uint4*>(j)[i] = w[i];
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kGroup; k++) {
            if (l0 + k >= L) continue;
#pragma unroll
            for (uint32_t n = 0; n < N; n += kGroupC) {
                const T v[kGroupC] = {jac[k][n], jac[k][n + 1]};
                store_feat<T, kGroupC>(j + k * N + n, v);
            }
        }
    }
}

// Eight fp16 columns of row b (levels l0 .. l0 + 3) -> the level planes [L][B][2] in the table's dtype (fp16 -> fp32 is exact)
template <typename T>
__device__ __forceinline__ void split_row_group(const Half8& w, uint32_t l0, uint32_t L, uint32_t B, uint32_t b, T* __restrict__ out) {
#pragma unroll
    for (uint32_t k = 0; k < kGroup; k++) {
        const uint32_t l = l0 + k;
        if (l >= L) continue;
        T v[kGroupC];
        if constexpr (sizeof(T) == 2) __builtin_memcpy(v, &w.v[kGroupC * k], 4);
        else { v[0] = (float)w.v[kGroupC * k]; v[1] = (float)w.v[kGroupC * k + 1]; }
        store_feat<T, kGroupC>(out + ((size_t)l * B + b) * kGroupC, v);
    }
}

}  // namespace
}  // namespace s3d
