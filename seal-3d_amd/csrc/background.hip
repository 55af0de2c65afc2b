// background.hip — the NGP background model of nerf/network.py:149-163 (reference) for gfx950:
//   rgb = sigmoid(W1 relu(W0 [half(SH_4(d)) | encoder_bg(sph)]))
// with encoder_bg a 4-level 2D hash grid of 2 features per level (nerf/network.py:74-96: 16 + 8 = 24 inputs, 64 hidden, 3 out,
// bias-free).  One thread = one ray.
//
//  * Grid lookup: grid_device.hpp's expressions (locate, grid_row, Acc<T>) in gridencoder.hip's corner order, so the features
//    are bit for bit those of s3d_grid_encode_forward (D = 2, fp32 and fp16 tables).  The SH basis is sh_eval.hpp's.
//  * MLP on VALU: fp16 operands, fp32 accumulation in input order, fp16 rounding of every layer output, ReLU, sigmoid in fp32
//    rounded to fp16 (the `-O` contract of DESIGN §2).  24 -> 64 -> 3 is 1,728 FMAs per ray; the weights (3.4 KB) sit in LDS as
//    fp32 and every lane reads the same word (broadcast).  MFMA would need a 16-ray transpose through LDS for a layer whose
//    whole forward costs less than the four gathers in front of it.
//  * Backward: the same recomputation (no [N, 64] activation is kept), then dL/d(grid features) scattered with the direct path
//    of k_grid_backward (packed half2 / fp32 atomics into the table gradient), and the weight gradients summed per wave in LDS:
//    the wave stages its 64 rays' (input, hidden, hidden gradient, output gradient) rows as fp16 — every one of them is an fp16
//    value of the op sequence — and lane l then owns weight-gradient entries l, l + 64, ..., l + 1,664 (27 x 64 = 1,728).  Each
//    wave files its partial sums; one small launch adds them in wave order (deterministic) and, when asked, raises the loss
//    scaler's flag for a non-finite weight or table gradient.
//
// The TensoRF background model of tensoRF/network.py:69-96, :201-218 (reference) is the second pair of kernels in this file:
//   rgb = sigmoid(W1 relu(W0 [half(freq_2(d)) | grid_sample(bg_mat, sph)]))
// with bg_mat a dense plane [8, H, W] sampled bilinearly (zeros padding, align_corners) and freq_2 the frequency encoding of
// encoders.hip (15 columns): 15 + 8 = 23 inputs, 64 hidden, 3 out, bias-free.  Same MLP arithmetic, weight staging and per-wave
// weight-gradient scheme (23 x 64 + 3 x 64 = 1,664 = 26 x 64 entries); the plane gradient is fp32, one atomic per in-range
// corner and rank, the form of grid_sample's own backward.
#include "grid_device.hpp"
#include "sh_eval.hpp"

namespace s3d {
namespace {

constexpr uint32_t kBgLevels = 4, kBgC = 2, kBgIn = 24, kBgHidden = 64, kBgOut = 3;
constexpr uint32_t kBgW0 = kBgHidden * kBgIn, kBgW1 = kBgOut * kBgHidden, kBgW = kBgW0 + kBgW1;  // 1,536 + 192 = 1,728
constexpr uint32_t kBgBlock = 256;
// backward: one wave per workgroup (21.7 KB of LDS stage): a training batch of 4,096 rays spreads over 64 CUs instead of 16
constexpr uint32_t kBgBwdBlock = 64;
constexpr uint32_t kBgMaxWaves = 2048;                 // backward: partial rows at most
constexpr uint32_t kBgStage = kBgIn + 2 * kBgHidden + 4;  // fp16 per staged ray: in | h | g_h | g_o (+1 pad) = 156
static_assert(kBgW == 27 * 64, "one weight-gradient entry per lane and slot");

__device__ __forceinline__ float h16(float v) { return (float)(_Float16)v; }

// grid features of one point: the 4 levels of k_grid_forward<T, 2, 2>, corners in its order
template <typename T>
__device__ __forceinline__ void bg_features(const float (&x)[2], const T* __restrict__ grid, const int32_t* __restrict__ offsets,
                                            const LevelScales& sc, T (&feat)[kBgLevels][kBgC]) {
#pragma unroll
    for (uint32_t level = 0; level < kBgLevels; level++) {
        const uint32_t off = (uint32_t)offsets[level];
        const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off;
        const T* table = grid + (size_t)off * kBgC;
        const float scale = sc.v[level];
        const uint32_t resolution = (uint32_t)ceilf(scale) + 1;
        float pos[2], pd[2] = {1.0f, 0.0f};
        uint32_t pos_grid[2];
        locate<2>(x, scale, false, 0, pos, pd, pos_grid);
        T f[4][kBgC];
        float wts[4];
#pragma unroll
        for (uint32_t idx = 0; idx < 4; idx++) {
            float w = 1;
            uint32_t pgl[2];
#pragma unroll
            for (uint32_t d = 0; d < 2; d++) {
                if ((idx & (1u << d)) == 0) { w *= 1 - pos[d]; pgl[d] = pos_grid[d]; }
                else { w *= pos[d]; pgl[d] = pos_grid[d] + 1; }
            }
            wts[idx] = w;
            load_feat<T, kBgC>(table + (size_t)grid_row<2>(0, false, hashmap_size, resolution, pgl) * kBgC, f[idx]);
        }
#pragma unroll
        for (uint32_t c = 0; c < kBgC; c++) {
            T r = Acc<T>::zero();
#pragma unroll
            for (uint32_t idx = 0; idx < 4; idx++) r = Acc<T>::fma(wts[idx], f[idx][c], r);
            feat[level][c] = r;
        }
    }
}

// network input row [half(SH_4(d)) | features]; returns false for a point outside [0,1]^2 after normalisation (features zero,
// like the grid forward)
template <typename T>
__device__ __forceinline__ bool bg_input(const float* __restrict__ sph, const float* __restrict__ dirs, uint32_t n,
                                         const T* __restrict__ grid, const int32_t* __restrict__ offsets, const LevelScales& sc,
                                         const ShNorm& K, float (&in)[kBgIn], T (&feat)[kBgLevels][kBgC]) {
    float x[2];
    const bool oob = load_point<2>(sph, n, sc, x);
    if (oob) {
#pragma unroll
        for (uint32_t l = 0; l < kBgLevels; l++) { feat[l][0] = Acc<T>::zero(); feat[l][1] = Acc<T>::zero(); }
    } else {
        bg_features<T>(x, grid, offsets, sc, feat);
    }
    float sh[16], j0[1], j1[1], j2[1];
    sh_eval<4, false>(dirs[(size_t)n * 3], dirs[(size_t)n * 3 + 1], dirs[(size_t)n * 3 + 2], K, sh, j0, j1, j2);
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) in[i] = h16(sh[i]);
#pragma unroll
    for (uint32_t l = 0; l < kBgLevels; l++) {
        in[16 + 2 * l] = h16(Acc<T>::to_f(feat[l][0]));
        in[17 + 2 * l] = h16(Acc<T>::to_f(feat[l][1]));
    }
    return !oob;
}

// hidden unit j = half(relu(half(W0[j] . in))), fp32 accumulation in input order.  Each consumer computes the units in the loop
// that uses them, so no [64]-wide array lives in private memory.
template <uint32_t IN>
__device__ __forceinline__ float bg_hidden(const float* __restrict__ sW0, const float (&in)[IN], uint32_t j) {
    float a = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < IN; k++) a = __builtin_fmaf(sW0[j * IN + k], in[k], a);
    return fmaxf(h16(a), 0.0f);
}

// the fp32 parameters rounded to fp16 as they enter LDS (autocast's weight cast, without a cast launch)
template <uint32_t NW0 = kBgW0>
__device__ __forceinline__ void bg_load_weights(const float* __restrict__ w0, const float* __restrict__ w1, float* sW0, float* sW1) {
    for (uint32_t i = threadIdx.x; i < NW0; i += blockDim.x) sW0[i] = h16(w0[i]);
    for (uint32_t i = threadIdx.x; i < kBgW1; i += blockDim.x) sW1[i] = h16(w1[i]);
    __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(kBgBlock) k_bg_forward(const float* __restrict__ sph, const float* __restrict__ dirs,
                                                         const T* __restrict__ grid, const int32_t* __restrict__ offsets, uint32_t N,
                                                         LevelScales sc, ShNorm K, const float* __restrict__ w0,
                                                         const float* __restrict__ w1, float* __restrict__ rgb, T* __restrict__ feat_out) {
    __shared__ float sW0[kBgW0], sW1[kBgW1];
    bg_load_weights(w0, w1, sW0, sW1);
    const uint32_t n = blockIdx.x * kBgBlock + threadIdx.x;
    if (n >= N) return;
    float in[kBgIn];
    T feat[kBgLevels][kBgC];
    bg_input<T>(sph, dirs, n, grid, offsets, sc, K, in, feat);
    if (feat_out) {
#pragma unroll
        for (uint32_t l = 0; l < kBgLevels; l++) store_feat<T, kBgC>(feat_out + ((size_t)l * N + n) * kBgC, feat[l]);
    }
    float o[kBgOut] = {0.0f, 0.0f, 0.0f};  // (each output sums its 64 terms in j order, as with the whole hidden row at hand)
#pragma unroll 2
    for (uint32_t j = 0; j < kBgHidden; j++) {
        const float hj = bg_hidden(sW0, in, j);
#pragma unroll
        for (uint32_t c = 0; c < kBgOut; c++) o[c] = __builtin_fmaf(sW1[c * kBgHidden + j], hj, o[c]);
    }
#pragma unroll
    for (uint32_t c = 0; c < kBgOut; c++) rgb[(size_t)n * 3 + c] = h16(1.0f / (1.0f + expf(-h16(o[c]))));
}

template <typename T>
__global__ void __launch_bounds__(kBgBwdBlock) k_bg_backward(const float* __restrict__ grad_rgb, const float* __restrict__ rgb,
                                                          const float* __restrict__ sph, const float* __restrict__ dirs,
                                                          const T* __restrict__ grid, const int32_t* __restrict__ offsets, uint32_t N,
                                                          LevelScales sc, ShNorm K, const float* __restrict__ w0,
                                                          const float* __restrict__ w1, T* __restrict__ grad_grid,
                                                          float* __restrict__ partial) {
    __shared__ float sW0[kBgW0], sW1[kBgW1];
    __shared__ _Float16 stage[kBgBwdBlock / 64][64][kBgStage];
    bg_load_weights(w0, w1, sW0, sW1);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    _Float16 (*st)[kBgStage] = stage[wave];
    float acc[27];
#pragma unroll
    for (uint32_t i = 0; i < 27; i++) acc[i] = 0.0f;
    for (uint32_t base = blockIdx.x * kBgBwdBlock; base < N; base += gridDim.x * kBgBwdBlock) {  // (block-uniform trip count)
        const uint32_t n = base + threadIdx.x;
        _Float16* row = st[lane];
        if (n < N) {
            float in[kBgIn], go[kBgOut];
            T feat[kBgLevels][kBgC];
            const bool inside = bg_input<T>(sph, dirs, n, grid, offsets, sc, K, in, feat);
            // sigmoid backward on the fp16 output (ngp_head.hip:k_ngp_rgb_backward)
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++) {
                const float y = rgb[(size_t)n * 3 + c];
                go[c] = h16(h16(grad_rgb[(size_t)n * 3 + c]) * (y * (1.0f - y)));
            }
            // hidden gradient = half(W1^T g_o) through the ReLU (threshold on the fp16 output), then the feature gradient
            // = half(W0[:, 16:]^T g_h)
            float gf[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) gf[k] = 0.0f;
#pragma unroll 2
            for (uint32_t j = 0; j < kBgHidden; j++) {
                const float hj = bg_hidden(sW0, in, j);
                float a = 0.0f;
#pragma unroll
                for (uint32_t c = 0; c < kBgOut; c++) a = __builtin_fmaf(sW1[c * kBgHidden + j], go[c], a);
                const float gh = hj > 0.0f ? h16(a) : 0.0f;
                row[kBgIn + kBgHidden + j] = (_Float16)gh;
                row[kBgIn + j] = (_Float16)hj;
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) gf[k] = __builtin_fmaf(sW0[j * kBgIn + 16 + k], gh, gf[k]);
            }
#pragma unroll
            for (uint32_t k = 0; k < kBgIn; k++) row[k] = (_Float16)in[k];
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++) row[kBgIn + 2 * kBgHidden + c] = (_Float16)go[c];
            if (inside && grad_grid) {  // k_grid_backward<T, 2, 2> on this point's fp16-rounded feature gradient
                float x[2];
                load_point<2>(sph, n, sc, x);
#pragma unroll
                for (uint32_t level = 0; level < kBgLevels; level++) {
                    T g[kBgC];
                    g[0] = Acc<T>::from_f(h16(gf[2 * level]));
                    g[1] = Acc<T>::from_f(h16(gf[2 * level + 1]));
                    if (Acc<T>::to_f(g[0]) == 0.0f && Acc<T>::to_f(g[1]) == 0.0f) continue;
                    const uint32_t off = (uint32_t)offsets[level];
                    const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off;
                    T* table = grad_grid + (size_t)off * kBgC;
                    const float scale = sc.v[level];
                    const uint32_t resolution = (uint32_t)ceilf(scale) + 1;
                    float pos[2], pd[2];
                    uint32_t pos_grid[2];
                    locate<2>(x, scale, false, 0, pos, pd, pos_grid);
#pragma unroll
                    for (uint32_t idx = 0; idx < 4; idx++) {
                        float w = 1;
                        uint32_t pgl[2];
#pragma unroll
                        for (uint32_t d = 0; d < 2; d++) {
                            if ((idx & (1u << d)) == 0) { w *= 1 - pos[d]; pgl[d] = pos_grid[d]; }
                            else { w *= pos[d]; pgl[d] = pos_grid[d] + 1; }
                        }
                        T* dst = table + (size_t)grid_row<2>(0, false, hashmap_size, resolution, pgl) * kBgC;
                        if constexpr (sizeof(T) == 2) {
                            const __half2 v = __halves2half2(__float2half(w * __half2float(g[0])), __float2half(w * __half2float(g[1])));
                            unsafeAtomicAdd(reinterpret_cast<__half2*>(dst), v);
                        } else {
                            unsafeAtomicAdd(reinterpret_cast<float*>(dst), w * g[0]);
                            unsafeAtomicAdd(reinterpret_cast<float*>(dst) + 1, w * g[1]);
                        }
                    }
                }
            }
        } else {
            for (uint32_t k = 0; k < kBgStage; k++) row[k] = (_Float16)0.0f;  // (a ray past N adds nothing)
        }
        __syncthreads();
        // weight gradients of the wave's 64 rays: lane owns dW0 entries e = lane + 64 i (i < 24: row e / 24, column e % 24) and
        // dW1[i - 24][lane]
        for (uint32_t r = 0; r < 64; r++) {
            const _Float16* q = st[r];
#pragma unroll
            for (uint32_t i = 0; i < 24; i++) {
                const uint32_t e = lane + 64 * i;
                acc[i] = __builtin_fmaf((float)q[kBgIn + kBgHidden + e / kBgIn], (float)q[e % kBgIn], acc[i]);
            }
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++)
                acc[24 + c] = __builtin_fmaf((float)q[kBgIn + 2 * kBgHidden + c], (float)q[kBgIn + lane], acc[24 + c]);
        }
        __syncthreads();
    }
    float* out = partial + (size_t)(blockIdx.x * (kBgBwdBlock / 64) + wave) * kBgW;
#pragma unroll
    for (uint32_t i = 0; i < 27; i++) out[lane + 64 * i] = acc[i];
}

// dW0 / dW1 = sum of the wave partials in wave order; found_inf: raised for a non-finite weight gradient or table entry
template <typename T, uint32_t NW = kBgW, uint32_t NW0 = kBgW0>
__global__ void __launch_bounds__(256) k_bg_reduce(const float* __restrict__ partial, uint32_t waves, float* __restrict__ grad_w0,
                                                   float* __restrict__ grad_w1, const T* __restrict__ grad_grid, size_t table_elems,
                                                   float* __restrict__ found_inf) {
    const uint32_t wblocks = div_up<uint32_t>(NW, 256);
    bool bad = false;
    if (blockIdx.x < wblocks) {
        const uint32_t e = blockIdx.x * 256 + threadIdx.x;
        if (e < NW) {
            float s = 0.0f;
            for (uint32_t w = 0; w < waves; w++) s += partial[(size_t)w * NW + e];
            if (e < NW0) grad_w0[e] = s;
            else grad_w1[e - NW0] = s;
            bad = !(fabsf(s) <= 3.402823466e38f);
        }
    } else if (grad_grid) {
        for (size_t i = (size_t)(blockIdx.x - wblocks) * 256 + threadIdx.x; i < table_elems; i += (size_t)(gridDim.x - wblocks) * 256)
            bad |= !(fabsf(Acc<T>::to_f(grad_grid[i])) <= 3.402823466e38f);
    }
    if (found_inf && bad) *found_inf = 1.0f;
}

uint32_t bg_backward_blocks(uint32_t N) {
    const uint32_t b = div_up<uint32_t>(N, kBgBwdBlock);
    const uint32_t cap = kBgMaxWaves / (kBgBwdBlock / 64);
    return b < 1 ? 1 : (b > cap ? cap : b);
}

struct BgArgs {
    LevelScales sc;
    ShNorm K;
};

BgArgs bg_args(float S, uint32_t H) {
    BgArgs a;
    host_scales(kBgLevels, S, H, a.sc, 1.0f, nullptr);  // GridEncoder.forward(x, bound=1): x01 = (x + 1) / 2
    host_sh_norm(4, a.K);
    return a;
}

// ---- the TensoRF background model: dense plane [kVbR, H, W] + freq_2(d) -> 23 -> 64 -> 3 ----
constexpr uint32_t kVbR = 8, kVbDir = 15, kVbIn = kVbDir + kVbR;
constexpr uint32_t kVbW0 = kBgHidden * kVbIn, kVbW = kVbW0 + kBgW1;  // 1,472 + 192 = 1,664
constexpr uint32_t kVbStage = kVbIn + 2 * kBgHidden + 5;               // fp16 per staged ray: in | h | g_h | g_o (+2 pad) = 156
static_assert(kVbW == 26 * 64, "one weight-gradient entry per lane and slot");

__device__ __forceinline__ float unnormalize(float c, uint32_t size) { return ((c + 1.0f) / 2.0f) * (float)(size - 1); }

// the four corners (nw, ne, sw, se) of one ray's plane sample: tensorf.hip's expressions (torch's grid sampler: bilinear, zeros
// padding, align_corners).  `ok` is each corner's own in-range test; `cell` is made of indices clamped into the plane BEFORE they
// are combined, so that it addresses the plane whatever the coordinate was (+1 exactly: the far corner is index W or H and fails
// its test; a cell or more outside the plane: both corners of an axis fail; non-finite: x0 = y0 = -2, nothing passes).
struct VbCorners {
    float w[4];
    uint32_t cell[4];
    bool ok[4];
};

__device__ __forceinline__ VbCorners vb_corners(const float* __restrict__ sph, uint32_t n, uint32_t H, uint32_t W) {
    const float ix = unnormalize(sph[(size_t)n * 2], W), iy = unnormalize(sph[(size_t)n * 2 + 1], H);
    const float fx = floorf(ix), fy = floorf(iy);
    const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
    const bool okx = fabsf(ix) < 1e9f, oky = fabsf(iy) < 1e9f;
    const int x0 = okx ? (int)fx : -2, y0 = oky ? (int)fy : -2;
    const bool bx0 = x0 >= 0 && x0 < (int)W, bx1 = x0 + 1 >= 0 && x0 + 1 < (int)W;
    const bool by0 = y0 >= 0 && y0 < (int)H, by1 = y0 + 1 >= 0 && y0 + 1 < (int)H;
    const uint32_t cx0 = (uint32_t)min(max(x0, 0), (int)W - 1), cx1 = (uint32_t)min(max(x0 + 1, 0), (int)W - 1);
    const uint32_t cy0 = (uint32_t)min(max(y0, 0), (int)H - 1), cy1 = (uint32_t)min(max(y0 + 1, 0), (int)H - 1);
    VbCorners c;
    c.w[0] = wx0 * wy0; c.w[1] = wx1 * wy0; c.w[2] = wx0 * wy1; c.w[3] = wx1 * wy1;
    c.cell[0] = cy0 * W + cx0; c.cell[1] = cy0 * W + cx1; c.cell[2] = cy1 * W + cx0; c.cell[3] = cy1 * W + cx1;
    c.ok[0] = bx0 && by0; c.ok[1] = bx1 && by0; c.ok[2] = bx0 && by1; c.ok[3] = bx1 && by1;
    return c;
}

// network input row [half(freq_2(d)) | half(plane sample)].  The sample accumulates the in-range corners in the sampler's order
// with a fused multiply-add each — how torch's grid_sampler kernel is compiled, so `feat` is F.grid_sample's fp32 result bit for
// bit; the frequency columns are k_freq_forward's (identity, then per frequency a sine and a cosine block).
__device__ __forceinline__ void vb_input(const float* __restrict__ dirs, uint32_t n, const float* __restrict__ plane, uint32_t H,
                                         uint32_t W, const VbCorners& c, float (&in)[kVbIn], float (&feat)[kVbR]) {
    const float half_pi = 3.141592653589793f / 2;
    const size_t plane_stride = (size_t)H * W;
#pragma unroll
    for (uint32_t r = 0; r < kVbR; r++) {
        const float* pr = plane + r * plane_stride;
        float v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) v[k] = c.ok[k] ? pr[c.cell[k]] : 0.0f;
        float m = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (c.ok[k]) m = __builtin_fmaf(v[k], c.w[k], m);
        feat[r] = m;
        in[kVbDir + r] = h16(m);
    }
#pragma unroll
    for (uint32_t d = 0; d < 3; d++) {
        const float x = dirs[(size_t)n * 3 + d];
        in[d] = h16(x);
#pragma unroll
        for (uint32_t col = 0; col < 4; col++)
            in[3 + col * 3 + d] = h16(sinf(ldexpf(x, (int)(col / 2)) + (float)(col % 2) * half_pi));
    }
}

__global__ void __launch_bounds__(kBgBlock) k_vm_bg_forward(const float* __restrict__ sph, const float* __restrict__ dirs,
                                                            const float* __restrict__ plane, uint32_t H, uint32_t W, uint32_t N,
                                                            const float* __restrict__ w0, const float* __restrict__ w1,
                                                            float* __restrict__ rgb, float* __restrict__ feat_out) {
    __shared__ float sW0[kVbW0], sW1[kBgW1];
    bg_load_weights<kVbW0>(w0, w1, sW0, sW1);
    const uint32_t n = blockIdx.x * kBgBlock + threadIdx.x;
    if (n >= N) return;
    float in[kVbIn], feat[kVbR];
    vb_input(dirs, n, plane, H, W, vb_corners(sph, n, H, W), in, feat);
    if (feat_out) {
#pragma unroll
        for (uint32_t r = 0; r < kVbR; r++) feat_out[(size_t)n * kVbR + r] = feat[r];
    }
    float o[kBgOut] = {0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (uint32_t j = 0; j < kBgHidden; j++) {
        const float hj = bg_hidden(sW0, in, j);
#pragma unroll
        for (uint32_t c = 0; c < kBgOut; c++) o[c] = __builtin_fmaf(sW1[c * kBgHidden + j], hj, o[c]);
    }
#pragma unroll
    for (uint32_t c = 0; c < kBgOut; c++) rgb[(size_t)n * 3 + c] = h16(1.0f / (1.0f + expf(-h16(o[c]))));
}

__global__ void __launch_bounds__(kBgBwdBlock) k_vm_bg_backward(const float* __restrict__ grad_rgb, const float* __restrict__ rgb,
                                                                const float* __restrict__ sph, const float* __restrict__ dirs,
                                                                const float* __restrict__ plane, uint32_t H, uint32_t W, uint32_t N,
                                                                const float* __restrict__ w0, const float* __restrict__ w1,
                                                                float* __restrict__ grad_plane, float* __restrict__ partial) {
    __shared__ float sW0[kVbW0], sW1[kBgW1];
    __shared__ _Float16 stage[kBgBwdBlock / 64][64][kVbStage];
    bg_load_weights<kVbW0>(w0, w1, sW0, sW1);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    _Float16 (*st)[kVbStage] = stage[wave];
    float acc[26];
#pragma unroll
    for (uint32_t i = 0; i < 26; i++) acc[i] = 0.0f;
    for (uint32_t base = blockIdx.x * kBgBwdBlock; base < N; base += gridDim.x * kBgBwdBlock) {  // (block-uniform trip count)
        const uint32_t n = base + threadIdx.x;
        _Float16* row = st[lane];
        if (n < N) {
            float in[kVbIn], feat[kVbR], go[kBgOut];
            const VbCorners cn = vb_corners(sph, n, H, W);
            vb_input(dirs, n, plane, H, W, cn, in, feat);
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++) {  // sigmoid backward on the fp16 output
                const float y = rgb[(size_t)n * 3 + c];
                go[c] = h16(h16(grad_rgb[(size_t)n * 3 + c]) * (y * (1.0f - y)));
            }
            // hidden gradient = half(W1^T g_o) through the ReLU, then the plane-sample gradient = half(W0[:, 15:]^T g_h)
            float gf[kVbR];
#pragma unroll
            for (uint32_t k = 0; k < kVbR; k++) gf[k] = 0.0f;
#pragma unroll 2
            for (uint32_t j = 0; j < kBgHidden; j++) {
                const float hj = bg_hidden(sW0, in, j);
                float a = 0.0f;
#pragma unroll
                for (uint32_t c = 0; c < kBgOut; c++) a = __builtin_fmaf(sW1[c * kBgHidden + j], go[c], a);
                const float gh = hj > 0.0f ? h16(a) : 0.0f;
                row[kVbIn + kBgHidden + j] = (_Float16)gh;
                row[kVbIn + j] = (_Float16)hj;
#pragma unroll
                for (uint32_t k = 0; k < kVbR; k++) gf[k] = __builtin_fmaf(sW0[j * kVbIn + kVbDir + k], gh, gf[k]);
            }
#pragma unroll
            for (uint32_t k = 0; k < kVbIn; k++) row[k] = (_Float16)in[k];
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++) row[kVbIn + 2 * kBgHidden + c] = (_Float16)go[c];
            if (grad_plane) {  // grid_sample's backward: corner weight x the fp16-rounded sample gradient, in-range corners only
                const size_t plane_stride = (size_t)H * W;
#pragma unroll
                for (uint32_t r = 0; r < kVbR; r++) {
                    const float g = h16(gf[r]);
                    if (g == 0.0f) continue;
                    float* gr = grad_plane + r * plane_stride;
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++)
                        if (cn.ok[k]) unsafeAtomicAdd(gr + cn.cell[k], cn.w[k] * g);
                }
            }
        } else {
            for (uint32_t k = 0; k < kVbStage; k++) row[k] = (_Float16)0.0f;  // (a ray past N adds nothing)
        }
        __syncthreads();
        // weight gradients of the wave's 64 rays: lane owns dW0 entries e = lane + 64 i (i < 23: row e / 23, column e % 23) and
        // dW1[i - 23][lane]
        for (uint32_t r = 0; r < 64; r++) {
            const _Float16* q = st[r];
#pragma unroll
            for (uint32_t i = 0; i < kVbIn; i++) {
                const uint32_t e = lane + 64 * i;
                acc[i] = __builtin_fmaf((float)q[kVbIn + kBgHidden + e / kVbIn], (float)q[e % kVbIn], acc[i]);
            }
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++)
                acc[kVbIn + c] = __builtin_fmaf((float)q[kVbIn + 2 * kBgHidden + c], (float)q[kVbIn + lane], acc[kVbIn + c]);
        }
        __syncthreads();
    }
    float* out = partial + (size_t)(blockIdx.x * (kBgBwdBlock / 64) + wave) * kVbW;
#pragma unroll
    for (uint32_t i = 0; i < 26; i++) out[lane + 64 * i] = acc[i];
}

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT size_t s3d_background_backward_workspace_size(uint32_t N) {
    return (size_t)bg_backward_blocks(N) * (kBgBwdBlock / 64) * kBgW * sizeof(float);
}

S3D_EXPORT int s3d_background_forward(const float* sph, const float* dirs, const void* table, const int32_t* offsets, uint32_t N,
                                      float S, uint32_t H, int dtype, const float* w0, const float* w1, float* rgb, void* features,
                                      s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(sph && dirs && table && offsets && w0 && w1 && rgb, "background_forward: null pointer");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "background_forward: dtype must be f32 or f16");
    const BgArgs a = bg_args(S, H);
    const dim3 grid(div_up<uint32_t>(N, kBgBlock)), block(kBgBlock);
    if (dtype == S3D_F16)
        hipLaunchKernelGGL(k_bg_forward<__half>, grid, block, 0, as_stream(stream), sph, dirs, (const __half*)table, offsets, N, a.sc, a.K,
                           w0, w1, rgb, (__half*)features);
    else
        hipLaunchKernelGGL(k_bg_forward<float>, grid, block, 0, as_stream(stream), sph, dirs, (const float*)table, offsets, N, a.sc, a.K,
                           w0, w1, rgb, (float*)features);
    return check_launch("background_forward");
}

S3D_EXPORT int s3d_background_backward(const float* grad_rgb, const float* rgb, const float* sph, const float* dirs, const void* table,
                                       const int32_t* offsets, uint32_t table_rows, uint32_t N, float S, uint32_t H, int dtype,
                                       const float* w0, const float* w1, void* grad_table, float* grad_w0, float* grad_w1,
                                       float* found_inf, void* workspace, size_t workspace_bytes, s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(grad_rgb && rgb && sph && dirs && table && offsets && w0 && w1 && grad_w0 && grad_w1 && workspace,
                "background_backward: null pointer");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "background_backward: dtype must be f32 or f16");
    S3D_REQUIRE(workspace_bytes >= s3d_background_backward_workspace_size(N),
                "background_backward: workspace smaller than s3d_background_backward_workspace_size(N)");
    const BgArgs a = bg_args(S, H);
    const uint32_t blocks = bg_backward_blocks(N), waves = blocks * (kBgBwdBlock / 64);
    hipStream_t st = as_stream(stream);
    // (the table scan of the flag check: 256 extra workgroups, grid-stride)
    const uint32_t rblocks = div_up<uint32_t>(kBgW, 256) + (found_inf ? 256u : 0u);
    const size_t elems = (size_t)table_rows * kBgC;
    float* part = (float*)workspace;
    if (dtype == S3D_F16) {
        hipLaunchKernelGGL(k_bg_backward<__half>, dim3(blocks), dim3(kBgBwdBlock), 0, st, grad_rgb, rgb, sph, dirs, (const __half*)table,
                           offsets, N, a.sc, a.K, w0, w1, (__half*)grad_table, part);
        hipLaunchKernelGGL(k_bg_reduce<__half>, dim3(rblocks), dim3(256), 0, st, (const float*)part, waves, grad_w0, grad_w1,
                           (found_inf && grad_table) ? (const __half*)grad_table : nullptr, elems, found_inf);
    } else {
        hipLaunchKernelGGL(k_bg_backward<float>, dim3(blocks), dim3(kBgBwdBlock), 0, st, grad_rgb, rgb, sph, dirs, (const float*)table,
                           offsets, N, a.sc, a.K, w0, w1, (float*)grad_table, part);
        hipLaunchKernelGGL(k_bg_reduce<float>, dim3(rblocks), dim3(256), 0, st, (const float*)part, waves, grad_w0, grad_w1,
                           (found_inf && grad_table) ? (const float*)grad_table : nullptr, elems, found_inf);
    }
    return check_launch("background_backward");
}

S3D_EXPORT size_t s3d_vm_background_backward_workspace_size(uint32_t N) {
    return (size_t)bg_backward_blocks(N) * (kBgBwdBlock / 64) * kVbW * sizeof(float);
}

static bool vb_plane_ok(uint32_t R, uint32_t H, uint32_t W) {
    return R == kVbR && H >= 2 && W >= 2 && (uint64_t)H * W <= 0x7fffffffull;
}

S3D_EXPORT int s3d_vm_background_forward(const float* sph, const float* dirs, const float* plane, uint32_t R, uint32_t H, uint32_t W,
                                         const float* w0, const float* w1, uint32_t N, float* rgb, float* features,
                                         s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(sph && dirs && plane && w0 && w1 && rgb, "vm_background_forward: null pointer");
    S3D_REQUIRE(vb_plane_ok(R, H, W), "vm_background_forward: the plane is [8, H, W] with H, W >= 2 and H * W < 2^31");
    hipLaunchKernelGGL(k_vm_bg_forward, dim3(div_up<uint32_t>(N, kBgBlock)), dim3(kBgBlock), 0, as_stream(stream), sph, dirs, plane, H, W,
                       N, w0, w1, rgb, features);
    return check_launch("vm_background_forward");
}

S3D_EXPORT int s3d_vm_background_backward(const float* grad_rgb, const float* rgb, const float* sph, const float* dirs,
                                          const float* plane, uint32_t R, uint32_t H, uint32_t W, const float* w0, const float* w1,
                                          uint32_t N, float* grad_plane, float* grad_w0, float* grad_w1, float* found_inf,
                                          void* workspace, size_t workspace_bytes, s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(grad_rgb && rgb && sph && dirs && plane && w0 && w1 && grad_w0 && grad_w1 && workspace,
                "vm_background_backward: null pointer");
    S3D_REQUIRE(vb_plane_ok(R, H, W), "vm_background_backward: the plane is [8, H, W] with H, W >= 2 and H * W < 2^31");
    S3D_REQUIRE(workspace_bytes >= s3d_vm_background_backward_workspace_size(N),
                "vm_background_backward: workspace smaller than s3d_vm_background_backward_workspace_size(N)");
    const uint32_t blocks = bg_backward_blocks(N), waves = blocks * (kBgBwdBlock / 64);
    hipStream_t st = as_stream(stream);
    const uint32_t rblocks = div_up<uint32_t>(kVbW, 256) + (found_inf ? 256u : 0u);  // (+ the plane-gradient scan of the flag check)
    float* part = (float*)workspace;
    hipLaunchKernelGGL(k_vm_bg_backward, dim3(blocks), dim3(kBgBwdBlock), 0, st, grad_rgb, rgb, sph, dirs, plane, H, W, N, w0, w1,
                       grad_plane, part);
    hipLaunchKernelGGL((k_bg_reduce<float, kVbW, kVbW0>), dim3(rblocks), dim3(256), 0, st, (const float*)part, waves, grad_w0, grad_w1,
                       (found_inf && grad_plane) ? (const float*)grad_plane : nullptr, (size_t)R * H * W, found_inf);
    return check_launch("vm_background_backward");
}
