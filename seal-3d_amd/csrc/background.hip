// background.hip — the background head of both backbones for gfx950: one forward kernel, one backward kernel, two input sources.
//   rgb = sigmoid(W1 relu(W0 [half(direction columns) | half(features of sph)])),  IN -> 64 -> 3, bias-free.  One thread = one ray.
//
// A *source* is a small struct the kernels take by value.  It names the layout (kDir direction columns in front, kFeat = 8
// feature columns, kIn = kDir + kFeat), reads what is uniform over the launch once per workgroup (`launch`), fills one ray's
// fp16-rounded input row (`input`, which in the forward also writes the optional feature output, and returns what the scatter
// needs later) and adds the fp16-rounded feature gradient into its gradient table (`scatter`).
//  * NgpSource<T> — nerf/network.py:74-96, :149-163 (reference): SH_4(d) (16 columns) | a 4-level 2D hash grid of 2 features per
//    level, 24 inputs.  Grid lookup: grid_device.hpp's expressions (locate, grid_row, Acc<T>) in gridencoder.hip's corner order
//    (bg_level_corners, shared by the lookup and the scatter), so the features are bit for bit those of s3d_grid_encode_forward
//    (D = 2, fp32 and fp16 tables); the SH basis is sh_eval.hpp's.  Scatter: the direct path of k_grid_backward (packed half2 /
//    fp32 atomics into the table gradient), nothing for a point outside [0,1]^2 or a level whose two channels are zero.
//  * VmSource — tensoRF/network.py:69-96, :201-218 (reference): freq_2(d) of encoders.hip (15 columns) | a dense plane
//    [8, H, W] sampled bilinearly (zeros padding, align_corners), 23 inputs.  The sample accumulates the in-range corners in the
//    sampler's order with a fused multiply-add each, so it is F.grid_sample's fp32 result bit for bit.  Scatter: fp32, one atomic
//    per in-range corner and rank, the form of grid_sample's own backward.
//
// The head, written once (k_bg_forward<Source>, k_bg_backward<Source>, k_bg_reduce<Source>):
//  * MLP on VALU: fp16 operands, fp32 accumulation in input order, fp16 rounding of every layer output, ReLU, sigmoid in fp32
//    rounded to fp16 (the `-O` contract of DESIGN §2).  24 -> 64 -> 3 is 1,728 FMAs per ray; the weights (3.4 KB) sit in LDS as
//    fp32 and every lane reads the same word (broadcast).  MFMA would need a 16-ray transpose through LDS for a layer whose
//    whole forward costs less than the four gathers in front of it.
//  * Backward: the same recomputation (no [N, 64] activation is kept), then the source's scatter, and the weight gradients summed
//    per wave in LDS: the wave stages its 64 rays' (input, hidden, hidden gradient, output gradient) rows as fp16 — every one of
//    them is an fp16 value of the op sequence — and lane l then owns weight-gradient entries l, l + 64, ... of the
//    (kIn + 3) x 64 (27 x 64 = 1,728, 26 x 64 = 1,664).  Each wave files its partial sums; one small launch adds them in wave
//    order (deterministic) and, when asked, raises the loss scaler's flag for a non-finite weight or table / plane gradient.
#include "grid_device.hpp"
#include "sh_eval.hpp"

namespace s3d {
namespace {

constexpr uint32_t kBgHidden = 64, kBgOut = 3, kBgFeat = 8;
constexpr uint32_t kBgW1 = kBgOut * kBgHidden;
constexpr uint32_t kBgBlock = 256;
// backward: one wave per workgroup (21.7 KB of LDS stage): a training batch of 4,096 rays spreads over 64 CUs instead of 16
constexpr uint32_t kBgBwdBlock = 64;
constexpr uint32_t kBgMaxWaves = 2048;  // backward: partial rows at most

// everything the head sizes, from the source's layout constants
template <class Src>
struct BgLayout {
    static constexpr uint32_t kIn = Src::kIn, kDir = Src::kDir;
    static constexpr uint32_t kW0 = kBgHidden * kIn, kW = kW0 + kBgW1;  // weight-gradient entries = the partial-row stride
    static constexpr uint32_t kSlots = kIn + kBgOut;                    // accumulators per lane
    static constexpr uint32_t kStage = (kIn + 2 * kBgHidden + kBgOut + 3) / 4 * 4;  // fp16 per staged ray: in | h | g_h | g_o (+ pad)
    static_assert(Src::kFeat == kBgFeat && kDir + kBgFeat == kIn, "input row = direction columns | 8 feature columns");
    static_assert(kSlots * 64 == kW, "one weight-gradient entry per lane and slot");
    static_assert(kStage == 156, "24 and 23 inputs stage 156 halves per ray: 26,880 and 26,624 B of LDS per backward workgroup");
};

__device__ __forceinline__ float h16(float v) { return (float)(_Float16)v; }

// ---- the NGP source: 2D hash grid [rows, 2] of T + SH_4(d) ----
constexpr uint32_t kBgLevels = 4, kBgC = 2;

// one level's four corner rows (within the level, which starts at row `off`) and weights of a point: k_grid_forward<T, 2, 2>'s
struct BgLevelCorners { uint32_t off, row[4]; float w[4]; };

__device__ __forceinline__ BgLevelCorners bg_level_corners(const float (&x)[2], const uint32_t (&offsets)[kBgLevels + 1],
                                                           const LevelScales& sc, uint32_t level) {
    BgLevelCorners c;
    c.off = offsets[level];
    const uint32_t hashmap_size = offsets[level + 1] - c.off;
    const float scale = sc.v[level];
    const uint32_t resolution = (uint32_t)ceilf(scale) + 1;
    float pos[2], pd[2] = {1.0f, 0.0f};
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
        c.w[idx] = w;
        c.row[idx] = grid_row<2>(0, false, hashmap_size, resolution, pgl);
    }
    return c;
}

template <typename T>
struct NgpSource {
    static constexpr uint32_t kDir = 16, kFeat = kBgLevels * kBgC, kIn = kDir + kFeat;
    using Grad = T;
    const float *sph, *dirs;
    const T* table;
    const int32_t* offsets;
    LevelScales sc;
    ShNorm K;
    T *grad, *feat_out;  // table gradient (backward; null: frozen table), grid features [4, N, 2] (forward, optional)

    // the level offsets, read once per workgroup before anything is stored: uniform values in scalar registers, which neither the
    // lookup nor the scatter has to fetch again behind its atomics
    struct Launch { uint32_t off[kBgLevels + 1]; };
    __device__ __forceinline__ Launch launch() const {
        Launch lc;
#pragma unroll
        for (uint32_t l = 0; l <= kBgLevels; l++) lc.off[l] = (uint32_t)offsets[l];
        return lc;
    }

    struct State { float x[2]; bool inside; };

    // network input row [half(SH_4(d)) | features]; a point outside [0,1]^2 after normalisation has zero features, like the
    // grid forward
    template <bool kFeatOut>
    __device__ __forceinline__ State input(const Launch& lc, uint32_t n, uint32_t N, float (&in)[kIn]) const {
        State s;
        s.inside = !load_point<2>(sph, n, sc, s.x);
        T feat[kBgLevels][kBgC];
#pragma unroll
        for (uint32_t level = 0; level < kBgLevels; level++) feat[level][0] = feat[level][1] = Acc<T>::zero();
        if (s.inside) {
#pragma unroll
            for (uint32_t level = 0; level < kBgLevels; level++) {
                const BgLevelCorners cn = bg_level_corners(s.x, lc.off, sc, level);
                const T* lv = table + (size_t)cn.off * kBgC;
                T f[4][kBgC];
#pragma unroll
                for (uint32_t idx = 0; idx < 4; idx++) load_feat<T, kBgC>(lv + (size_t)cn.row[idx] * kBgC, f[idx]);
#pragma unroll
                for (uint32_t c = 0; c < kBgC; c++) {
                    T r = Acc<T>::zero();
#pragma unroll
                    for (uint32_t idx = 0; idx < 4; idx++) r = Acc<T>::fma(cn.w[idx], f[idx][c], r);
                    feat[level][c] = r;
                }
            }
        }
        if (kFeatOut && feat_out) {
#pragma unroll
            for (uint32_t l = 0; l < kBgLevels; l++) store_feat<T, kBgC>(feat_out + ((size_t)l * N + n) * kBgC, feat[l]);
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
        return s;
    }

    // k_grid_backward<T, 2, 2> on this point's fp16-rounded feature gradient
    __device__ __forceinline__ void scatter(const Launch& lc, const State& s, const float (&gf)[kFeat]) const {
        if (!s.inside || !grad) return;
#pragma unroll
        for (uint32_t level = 0; level < kBgLevels; level++) {
            T g[kBgC];
            g[0] = Acc<T>::from_f(h16(gf[2 * level]));
            g[1] = Acc<T>::from_f(h16(gf[2 * level + 1]));
            if (Acc<T>::to_f(g[0]) == 0.0f && Acc<T>::to_f(g[1]) == 0.0f) continue;
            const BgLevelCorners cn = bg_level_corners(s.x, lc.off, sc, level);
            T* lv = grad + (size_t)cn.off * kBgC;
#pragma unroll
            for (uint32_t idx = 0; idx < 4; idx++) {
                T* dst = lv + (size_t)cn.row[idx] * kBgC;
                const float w = cn.w[idx];
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
};

// ---- the TensoRF source: dense plane [8, H, W] + freq_2(d) ----
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

struct VmSource {
    static constexpr uint32_t kDir = 15, kFeat = kBgFeat, kIn = kDir + kFeat;
    using Grad = float;
    const float *sph, *dirs, *plane;
    uint32_t H, W;
    float *grad, *feat_out;  // plane gradient (backward; null: frozen plane), plane samples [N, 8] (forward, optional)

    struct Launch {};  // (nothing to read per workgroup)
    __device__ __forceinline__ Launch launch() const { return {}; }

    using State = VbCorners;

    // network input row [half(freq_2(d)) | half(plane sample)]; the frequency columns are k_freq_forward's (identity, then per
    // frequency a sine and a cosine block)
    template <bool kFeatOut>
    __device__ __forceinline__ State input(const Launch&, uint32_t n, uint32_t N, float (&in)[kIn]) const {
        const VbCorners c = vb_corners(sph, n, H, W);
        const float half_pi = 3.141592653589793f / 2;
        const size_t plane_stride = (size_t)H * W;
        float feat[kFeat];
#pragma unroll
        for (uint32_t r = 0; r < kFeat; r++) {
            const float* pr = plane + r * plane_stride;
            float v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) v[k] = c.ok[k] ? pr[c.cell[k]] : 0.0f;
            float m = 0.0f;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (c.ok[k]) m = __builtin_fmaf(v[k], c.w[k], m);
            feat[r] = m;
            in[kDir + r] = h16(m);
        }
        if (kFeatOut && feat_out) {
#pragma unroll
            for (uint32_t r = 0; r < kFeat; r++) feat_out[(size_t)n * kFeat + r] = feat[r];
        }
#pragma unroll
        for (uint32_t d = 0; d < 3; d++) {
            const float x = dirs[(size_t)n * 3 + d];
            in[d] = h16(x);
#pragma unroll
            for (uint32_t col = 0; col < 4; col++)
                in[3 + col * 3 + d] = h16(sinf(ldexpf(x, (int)(col / 2)) + (float)(col % 2) * half_pi));
        }
        return c;
    }

    // grid_sample's backward: corner weight x the fp16-rounded sample gradient, in-range corners only
    __device__ __forceinline__ void scatter(const Launch&, const State& c, const float (&gf)[kFeat]) const {
        if (!grad) return;
        const size_t plane_stride = (size_t)H * W;
#pragma unroll
        for (uint32_t r = 0; r < kFeat; r++) {
            const float g = h16(gf[r]);
            if (g == 0.0f) continue;
            float* gr = grad + r * plane_stride;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (c.ok[k]) unsafeAtomicAdd(gr + c.cell[k], c.w[k] * g);
        }
    }
};

// ---- the head ----
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
template <uint32_t NW0>
__device__ __forceinline__ void bg_load_weights(const float* __restrict__ w0, const float* __restrict__ w1, float* sW0, float* sW1) {
    for (uint32_t i = threadIdx.x; i < NW0; i += blockDim.x) sW0[i] = h16(w0[i]);
    for (uint32_t i = threadIdx.x; i < kBgW1; i += blockDim.x) sW1[i] = h16(w1[i]);
    __syncthreads();
}

template <class Src>
__global__ void __launch_bounds__(kBgBlock) k_bg_forward(const Src src, uint32_t N, const float* __restrict__ w0,
                                                         const float* __restrict__ w1, float* __restrict__ rgb) {
    using L = BgLayout<Src>;
    __shared__ float sW0[L::kW0], sW1[kBgW1];
    const typename Src::Launch lc = src.launch();
    bg_load_weights<L::kW0>(w0, w1, sW0, sW1);
    const uint32_t n = blockIdx.x * kBgBlock + threadIdx.x;
    if (n >= N) return;
    float in[L::kIn];
    src.template input<true>(lc, n, N, in);
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

template <class Src>
__global__ void __launch_bounds__(kBgBwdBlock) k_bg_backward(const Src src, uint32_t N, const float* __restrict__ grad_rgb,
                                                             const float* __restrict__ rgb, const float* __restrict__ w0,
                                                             const float* __restrict__ w1, float* __restrict__ partial) {
    using L = BgLayout<Src>;
    constexpr uint32_t IN = L::kIn;
    __shared__ float sW0[L::kW0], sW1[kBgW1];
    __shared__ _Float16 stage[kBgBwdBlock / 64][64][L::kStage];
    const typename Src::Launch lc = src.launch();
    bg_load_weights<L::kW0>(w0, w1, sW0, sW1);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    _Float16 (*st)[L::kStage] = stage[wave];
    float acc[L::kSlots];
#pragma unroll
    for (uint32_t i = 0; i < L::kSlots; i++) acc[i] = 0.0f;
    for (uint32_t base = blockIdx.x * kBgBwdBlock; base < N; base += gridDim.x * kBgBwdBlock) {  // (block-uniform trip count)
        const uint32_t n = base + threadIdx.x;
        _Float16* row = st[lane];
        if (n < N) {
            float in[IN], go[kBgOut];
            const typename Src::State state = src.template input<false>(lc, n, N, in);  // (no feature output here)
            // sigmoid backward on the fp16 output (ngp_head.hip:k_ngp_rgb_backward)
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++) {
                const float y = rgb[(size_t)n * 3 + c];
                go[c] = h16(h16(grad_rgb[(size_t)n * 3 + c]) * (y * (1.0f - y)));
            }
            // hidden gradient = half(W1^T g_o) through the ReLU (threshold on the fp16 output), then the feature gradient
            // = half(W0[:, kDir:]^T g_h)
            float gf[kBgFeat];
#pragma unroll
            for (uint32_t k = 0; k < kBgFeat; k++) gf[k] = 0.0f;
#pragma unroll 2
            for (uint32_t j = 0; j < kBgHidden; j++) {
                const float hj = bg_hidden(sW0, in, j);
                float a = 0.0f;
#pragma unroll
                for (uint32_t c = 0; c < kBgOut; c++) a = __builtin_fmaf(sW1[c * kBgHidden + j], go[c], a);
                const float gh = hj > 0.0f ? h16(a) : 0.0f;
                row[IN + kBgHidden + j] = (_Float16)gh;
                row[IN + j] = (_Float16)hj;
#pragma unroll
                for (uint32_t k = 0; k < kBgFeat; k++) gf[k] = __builtin_fmaf(sW0[j * IN + L::kDir + k], gh, gf[k]);
            }
#pragma unroll
            for (uint32_t k = 0; k < IN; k++) row[k] = (_Float16)in[k];
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++) row[IN + 2 * kBgHidden + c] = (_Float16)go[c];
            src.scatter(lc, state, gf);
        } else {
            for (uint32_t k = 0; k < L::kStage; k++) row[k] = (_Float16)0.0f;  // (a ray past N adds nothing)
        }
        __syncthreads();
        // weight gradients of the wave's 64 rays: lane owns dW0 entries e = lane + 64 i (i < IN: row e / IN, column e % IN) and
        // dW1[i - IN][lane]
        for (uint32_t r = 0; r < 64; r++) {
            const _Float16* q = st[r];
#pragma unroll
            for (uint32_t i = 0; i < IN; i++) {
                const uint32_t e = lane + 64 * i;
                acc[i] = __builtin_fmaf((float)q[IN + kBgHidden + e / IN], (float)q[e % IN], acc[i]);
            }
#pragma unroll
            for (uint32_t c = 0; c < kBgOut; c++)
                acc[IN + c] = __builtin_fmaf((float)q[IN + 2 * kBgHidden + c], (float)q[IN + lane], acc[IN + c]);
        }
        __syncthreads();
    }
    float* out = partial + (size_t)(blockIdx.x * (kBgBwdBlock / 64) + wave) * L::kW;
#pragma unroll
    for (uint32_t i = 0; i < L::kSlots; i++) out[lane + 64 * i] = acc[i];
}

// dW0 / dW1 = sum of the wave partials in wave order; found_inf: raised for a non-finite weight gradient or table / plane entry
template <class Src>
__global__ void __launch_bounds__(256) k_bg_reduce(const float* __restrict__ partial, uint32_t waves, float* __restrict__ grad_w0,
                                                   float* __restrict__ grad_w1, const typename Src::Grad* __restrict__ grad,
                                                   size_t grad_elems, float* __restrict__ found_inf) {
    constexpr uint32_t NW = BgLayout<Src>::kW, NW0 = BgLayout<Src>::kW0;
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
    } else if (grad) {
        for (size_t i = (size_t)(blockIdx.x - wblocks) * 256 + threadIdx.x; i < grad_elems; i += (size_t)(gridDim.x - wblocks) * 256)
            bad |= !(fabsf(Acc<typename Src::Grad>::to_f(grad[i])) <= 3.402823466e38f);
    }
    if (found_inf && bad) *found_inf = 1.0f;
}

// ---- host side ----
uint32_t bg_backward_blocks(uint32_t N) {
    const uint32_t b = div_up<uint32_t>(N, kBgBwdBlock);
    const uint32_t cap = kBgMaxWaves / (kBgBwdBlock / 64);
    return b < 1 ? 1 : (b > cap ? cap : b);
}

template <class Src>
size_t bg_workspace_size(uint32_t N) {  // one partial row per backward wave
    return (size_t)bg_backward_blocks(N) * (kBgBwdBlock / 64) * BgLayout<Src>::kW * sizeof(float);
}

template <class Src>
int bg_launch_forward(const Src& src, uint32_t N, const float* w0, const float* w1, float* rgb, s3d_stream_t stream, const char* what) {
    hipLaunchKernelGGL(k_bg_forward<Src>, dim3(div_up<uint32_t>(N, kBgBlock)), dim3(kBgBlock), 0, as_stream(stream), src, N, w0, w1, rgb);
    return check_launch(what);
}

// backward + reduce; grad_elems: entries of src.grad, which the reduce scans for the flag check (256 extra workgroups, grid-stride)
template <class Src>
int bg_launch_backward(const Src& src, uint32_t N, const float* grad_rgb, const float* rgb, const float* w0, const float* w1,
                       float* grad_w0, float* grad_w1, size_t grad_elems, float* found_inf, void* workspace, s3d_stream_t stream,
                       const char* what) {
    const uint32_t blocks = bg_backward_blocks(N), waves = blocks * (kBgBwdBlock / 64);
    const uint32_t rblocks = div_up<uint32_t>(BgLayout<Src>::kW, 256) + (found_inf ? 256u : 0u);
    hipStream_t st = as_stream(stream);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(k_bg_backward<Src>, dim3(blocks), dim3(kBgBwdBlock), 0, st, src, N, grad_rgb, rgb, w0, w1, part);
    hipLaunchKernelGGL(k_bg_reduce<Src>, dim3(rblocks), dim3(256), 0, st, (const float*)part, waves, grad_w0, grad_w1,
                       (found_inf && src.grad) ? (const typename Src::Grad*)src.grad : nullptr, grad_elems, found_inf);
    return check_launch(what);
}

template <typename T>
NgpSource<T> ngp_source(const float* sph, const float* dirs, const void* table, const int32_t* offsets, float S, uint32_t H,
                        void* grad, void* feat_out) {
    NgpSource<T> s{sph, dirs, (const T*)table, offsets, {}, {}, (T*)grad, (T*)feat_out};
    host_scales(kBgLevels, S, H, s.sc, 1.0f, nullptr);  // GridEncoder.forward(x, bound=1): x01 = (x + 1) / 2
    host_sh_norm(4, s.K);
    return s;
}

bool vb_plane_ok(uint32_t R, uint32_t H, uint32_t W) { return R == kBgFeat && H >= 2 && W >= 2 && (uint64_t)H * W <= 0x7fffffffull; }

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT size_t s3d_background_backward_workspace_size(uint32_t N) { return bg_workspace_size<NgpSource<float>>(N); }

S3D_EXPORT int s3d_background_forward(const float* sph, const float* dirs, const void* table, const int32_t* offsets, uint32_t N,
                                      float S, uint32_t H, int dtype, const float* w0, const float* w1, float* rgb, void* features,
                                      s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(sph && dirs && table && offsets && w0 && w1 && rgb, "background_forward: null pointer");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "background_forward: dtype must be f32 or f16");
    if (dtype == S3D_F16)
        return bg_launch_forward(ngp_source<__half>(sph, dirs, table, offsets, S, H, nullptr, features), N, w0, w1, rgb, stream,
                                 "background_forward");
    return bg_launch_forward(ngp_source<float>(sph, dirs, table, offsets, S, H, nullptr, features), N, w0, w1, rgb, stream,
                             "background_forward");
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
    const size_t elems = (size_t)table_rows * kBgC;
    if (dtype == S3D_F16)
        return bg_launch_backward(ngp_source<__half>(sph, dirs, table, offsets, S, H, grad_table, nullptr), N, grad_rgb, rgb, w0, w1,
                                  grad_w0, grad_w1, elems, found_inf, workspace, stream, "background_backward");
    return bg_launch_backward(ngp_source<float>(sph, dirs, table, offsets, S, H, grad_table, nullptr), N, grad_rgb, rgb, w0, w1,
                              grad_w0, grad_w1, elems, found_inf, workspace, stream, "background_backward");
}

S3D_EXPORT size_t s3d_vm_background_backward_workspace_size(uint32_t N) { return bg_workspace_size<VmSource>(N); }

S3D_EXPORT int s3d_vm_background_forward(const float* sph, const float* dirs, const float* plane, uint32_t R, uint32_t H, uint32_t W,
                                         const float* w0, const float* w1, uint32_t N, float* rgb, float* features,
                                         s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(sph && dirs && plane && w0 && w1 && rgb, "vm_background_forward: null pointer");
    S3D_REQUIRE(vb_plane_ok(R, H, W), "vm_background_forward: the plane is [8, H, W] with H, W >= 2 and H * W < 2^31");
    return bg_launch_forward(VmSource{sph, dirs, plane, H, W, nullptr, features}, N, w0, w1, rgb, stream, "vm_background_forward");
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
    return bg_launch_backward(VmSource{sph, dirs, plane, H, W, grad_plane, nullptr}, N, grad_rgb, rgb, w0, w1, grad_w0, grad_w1,
                              (size_t)R * H * W, found_inf, workspace, stream, "vm_background_backward");
}
