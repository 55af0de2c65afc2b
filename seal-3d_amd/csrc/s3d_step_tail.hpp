// s3d_step_tail.hpp — the four small bodies that end a training step, shared by the launches that own them (csrc/ffmlp.hip:
// k_ffmlp_wgrad_reduce_jobs, csrc/raymarching.hip: k_bg_mse_reduce, csrc/optim.hip: k_adam_step_multi, k_step_epilogue) and by
// the grid backward's two binned launches (csrc/gridencoder.hip), which can run them as riders (s3d_grid_encode_backward_adam_tail):
// one definition each, so both routes produce the same bits.
#pragma once
#include "s3d_common.hpp"
#include "s3d_adam.hpp"

namespace s3d {

// ------------------------------------------------------------------ (a) weight-gradient reduce of the fused MLP backward
constexpr uint32_t kMaxMlpLayers = 8;
constexpr uint32_t kWgradPad = 64;  // partial weight-gradient matrices are stored [64][64] fp32 regardless of W
// Eight lanes per matrix element: each sums every 8th workgroup partial with independent accumulators (a single chain over
// 256 partials was latency-bound: ~20 us), then a fixed xor-shuffle tree combines the eight.  Deterministic.
constexpr uint32_t kReduceSplit = 8;
struct ReduceJob {
    const float* partial;   // [nblk][64][64] planes of this layer
    _Float16* gw;           // the network's grad_weights
    float* found_inf;
    uint32_t Fo, Fi, w_off, nblk, accumulate;
};
struct ReduceJobs {
    ReduceJob job[2 * kMaxMlpLayers];
    uint32_t n;
};
// lane t of a job (t / kReduceSplit = matrix element, t % kReduceSplit = its share of the partials); whole waves call it
__device__ __forceinline__ void wgrad_reduce_job(const ReduceJob& L, uint32_t t) {
    const uint32_t e = t / kReduceSplit, part = t % kReduceSplit;
    const bool live = e < L.Fo * L.Fi;
    const uint32_t o = live ? e / L.Fi : 0, i = live ? e - o * L.Fi : 0;
    const float* p = L.partial + o * kWgradPad + i;
    constexpr size_t kPlane = (size_t)kWgradPad * kWgradPad;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (live) {
        uint32_t b = part;
        for (; b + 3 * kReduceSplit < L.nblk; b += 4 * kReduceSplit) {
            s0 += p[(size_t)(b + 0 * kReduceSplit) * kPlane];
            s1 += p[(size_t)(b + 1 * kReduceSplit) * kPlane];
            s2 += p[(size_t)(b + 2 * kReduceSplit) * kPlane];
            s3 += p[(size_t)(b + 3 * kReduceSplit) * kPlane];
        }
        for (; b < L.nblk; b += kReduceSplit) s0 += p[(size_t)b * kPlane];
    }
    float v = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int d = 1; d < (int)kReduceSplit; d <<= 1) v += __shfl_xor(v, d, 64);
    if (live && part == 0) {
        if (L.accumulate) v += (float)L.gw[L.w_off + e];
        const _Float16 h = (_Float16)v;
        L.gw[L.w_off + e] = h;
        if (L.found_inf && !(fabsf((float)h) <= 65504.0f)) *L.found_inf = 1.0f;
    }
}
// the jobs of s3d_ffmlp_wgrad_reduce_pair's arguments (csrc/ffmlp.hip); *wmax: the wider hidden width.  S3D_OK or an error code
int wgrad_reduce_pair_jobs(const void* workspace_a, uint32_t B_a, uint32_t input_dim_a, uint32_t hidden_dim_a, uint32_t num_layers_a,
                           uint16_t* grad_weights_a, int accumulate_a, float* found_inf_a, const void* workspace_b, uint32_t B_b,
                           uint32_t input_dim_b, uint32_t hidden_dim_b, uint32_t num_layers_b, uint16_t* grad_weights_b,
                           int accumulate_b, float* found_inf_b, ReduceJobs& jobs, uint32_t& wmax);
// 256-lane units per job of a launch (or a rider) that covers the widest layer
inline uint32_t wgrad_reduce_units(uint32_t wmax) { return div_up<uint32_t>(wmax * kWgradPad * kReduceSplit, 256); }

// ------------------------------------------------------------------ (b) value of the criterion from the per-ray terms
// One workgroup of 1,024 / VT threads, each carrying VT virtual threads: virtual thread t of 1,024 takes rays t, t + 1,024, ...,
// butterfly per 64, sixteen partials in sequence (ngp_head.hip: k_bg_mse_forward's order).  part / dpart: 16 floats of LDS each.
template <uint32_t VT>
__device__ __forceinline__ void loss_terms_reduce(const float* __restrict__ sq, const float* __restrict__ dabs, uint32_t N,
                                                  float depth_weight, float* __restrict__ loss, float* part, float* dpart) {
    constexpr uint32_t T = 1024 / VT;
#pragma unroll
    for (uint32_t k = 0; k < VT; k++) {
        const uint32_t vt = threadIdx.x + k * T;
        float acc = 0.0f, dacc = 0.0f;
        for (uint32_t m = vt; m < N; m += 1024) {
#pragma unroll
            for (int c = 0; c < 3; c++) acc += sq[(size_t)m * 3 + c];
        }
        if (dabs)
            for (uint32_t m = vt; m < N; m += 1024) dacc += dabs[m];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { acc += __shfl_xor(acc, d, 64); dacc += __shfl_xor(dacc, d, 64); }
        if ((vt & 63) == 0) { part[vt >> 6] = acc; dpart[vt >> 6] = dacc; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f, td = 0.0f;
        for (int w = 0; w < 16; w++) { t += part[w]; td += dpart[w]; }
        t = t / (3.0f * (float)N);
        if (dabs) t = t + depth_weight * (td / (float)N);
        *loss = t;
    }
}

// ------------------------------------------------------------------ (c) Adam over one tensor of a multi-tensor update
template <typename G> __device__ __forceinline__ float grad_to_f(G g);
template <> __device__ __forceinline__ float grad_to_f<float>(float g) { return g; }
template <> __device__ __forceinline__ float grad_to_f<__half>(__half g) { return __half2float(g); }

template <typename G> struct GradVec4;
template <> struct GradVec4<float> {
    static __device__ __forceinline__ void load(const float* g, size_t i, float (&o)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(g + i);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    }
    static __device__ __forceinline__ void zero(float* g, size_t i) { *reinterpret_cast<float4*>(g + i) = make_float4(0, 0, 0, 0); }
};
template <> struct GradVec4<__half> {
    static __device__ __forceinline__ void load(const __half* g, size_t i, float (&o)[4]) {
        const uint2 t = *reinterpret_cast<const uint2*>(g + i);
        const __half2 a = *reinterpret_cast<const __half2*>(&t.x), b = *reinterpret_cast<const __half2*>(&t.y);
        o[0] = __low2float(a); o[1] = __high2float(a); o[2] = __low2float(b); o[3] = __high2float(b);
    }
    static __device__ __forceinline__ void zero(__half* g, size_t i) { *reinterpret_cast<uint2*>(g + i) = make_uint2(0u, 0u); }
};

// `consume`: the gradient is cleared behind the read (the producers of the next step ACCUMULATE into it: saves the
// optimizer's separate zero fill); `skip`: overflow step, nothing is updated but a consumed gradient is still cleared
template <typename G>
__device__ __forceinline__ void clear_range(G* __restrict__ g, size_t n, bool vec, size_t tid, size_t nthreads) {
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t q = tid; q < n4; q += nthreads) GradVec4<G>::zero(g, q * 4);
    for (size_t i = n4 * 4 + tid; i < n; i += nthreads) g[i] = G(0.0f);
}

template <typename G>
__device__ __forceinline__ void adam_range(const AdamCoef& c, float* __restrict__ p, G* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, __half* __restrict__ p_half, size_t n, bool vec, size_t tid,
                                           size_t nthreads, bool consume) {
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t q = tid; q < n4; q += nthreads) {
        const size_t i = q * 4;
        float gi[4];
        GradVec4<G>::load(g, i, gi);
        if (consume) GradVec4<G>::zero(g, i);
        // the 24 B per element of fp32 state stream through once per step: non-temporal, so that they do not push the fp16
        // table copy (read by the next forward) and the gradient buffer out of the L2 / Infinity Cache
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v mv = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(m + i));
        const f4v vv = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(v + i));
        const f4v pv = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p + i));
        float4 mi = make_float4(mv.x, mv.y, mv.z, mv.w), vi = make_float4(vv.x, vv.y, vv.z, vv.w),
               pi = make_float4(pv.x, pv.y, pv.z, pv.w);
        adam_update(c, gi[0], mi.x, vi.x, pi.x);
        adam_update(c, gi[1], mi.y, vi.y, pi.y);
        adam_update(c, gi[2], mi.z, vi.z, pi.z);
        adam_update(c, gi[3], mi.w, vi.w, pi.w);
        __builtin_nontemporal_store(f4v{mi.x, mi.y, mi.z, mi.w}, reinterpret_cast<f4v*>(m + i));
        __builtin_nontemporal_store(f4v{vi.x, vi.y, vi.z, vi.w}, reinterpret_cast<f4v*>(v + i));
        __builtin_nontemporal_store(f4v{pi.x, pi.y, pi.z, pi.w}, reinterpret_cast<f4v*>(p + i));
        if (p_half) {
            const __half2 a = __floats2half2_rn(pi.x, pi.y), b = __floats2half2_rn(pi.z, pi.w);
            uint2 o;
            o.x = *reinterpret_cast<const uint32_t*>(&a);
            o.y = *reinterpret_cast<const uint32_t*>(&b);
            *reinterpret_cast<uint2*>(p_half + i) = o;
        }
    }
    for (size_t i = n4 * 4 + tid; i < n; i += nthreads) {
        float mi = m[i], vi = v[i], pi = p[i];
        adam_update(c, grad_to_f<G>(g[i]), mi, vi, pi);
        if (consume) g[i] = G(0.0f);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        if (p_half) p_half[i] = __float2half(pi);
    }
}

// A parameter whose fp16 gradient and fp16 copy live inside a PACKED weight buffer (the nn.Linear weights of the two-encoder
// Seal network inside the fused MLP kernels' [out, in_padded] layout): element i = (row, col) of the [rows, cols] parameter
// sits at row * stride + col of `g` and `p_half`; the fp32 state stays contiguous.  ~10 K elements per tensor: scalar accesses.
template <typename G>
__device__ __forceinline__ void adam_range_packed(const AdamCoef& c, float* __restrict__ p, G* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, __half* __restrict__ p_half, size_t n, uint32_t cols,
                                                  uint32_t stride, size_t tid, size_t nthreads, bool consume) {
    for (size_t i = tid; i < n; i += nthreads) {
        const size_t j = (i / cols) * stride + i % cols;
        float mi = m[i], vi = v[i], pi = p[i];
        adam_update(c, grad_to_f<G>(g[j]), mi, vi, pi);
        if (consume) g[j] = G(0.0f);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        if (p_half) p_half[j] = __float2half(pi);
    }
}

// one tensor of a multi-tensor update as a launch argument (stride != 0: packed layout of g / h, adam_range_packed)
struct AdamItem {
    float* p;
    void* g;
    float* m;
    float* v;
    __half* h;
    size_t n;
    float lr, beta1, beta2, eps, l1;
    uint32_t cols, stride;
    uint8_t half_grad, vec, consume;
};
// lane `tid` of `nthreads` of tensor t's update; `skip`: the step is skipped as a whole (GradScaler.step)
__device__ __forceinline__ void adam_item_run(const AdamItem& t, bool skip, const float* __restrict__ step,
                                              const float* __restrict__ grad_scale, const float* __restrict__ lr_scale, size_t tid,
                                              size_t nthreads) {
    if (skip) {  // skipped step: nothing is updated
        if (t.consume && t.stride) {
            for (size_t k = tid; k < t.n; k += nthreads) {
                const size_t j = (k / t.cols) * t.stride + k % t.cols;
                if (t.half_grad) ((__half*)t.g)[j] = __half(0.0f);
                else ((float*)t.g)[j] = 0.0f;
            }
        } else if (t.consume) {
            if (t.half_grad) clear_range<__half>((__half*)t.g, t.n, t.vec != 0, tid, nthreads);
            else clear_range<float>((float*)t.g, t.n, t.vec != 0, tid, nthreads);
        }
        return;
    }
    const AdamCoef c = adam_coef(t.lr, t.beta1, t.beta2, t.eps, t.l1, step, grad_scale, lr_scale);
    if (t.stride) {
        if (t.half_grad)
            adam_range_packed<__half>(c, t.p, (__half*)t.g, t.m, t.v, t.h, t.n, t.cols, t.stride, tid, nthreads, t.consume != 0);
        else
            adam_range_packed<float>(c, t.p, (float*)t.g, t.m, t.v, t.h, t.n, t.cols, t.stride, tid, nthreads, t.consume != 0);
    } else if (t.half_grad)
        adam_range<__half>(c, t.p, (__half*)t.g, t.m, t.v, t.h, t.n, t.vec != 0, tid, nthreads, t.consume != 0);
    else
        adam_range<float>(c, t.p, (float*)t.g, t.m, t.v, t.h, t.n, t.vec != 0, tid, nthreads, t.consume != 0);
}
// host: tensor `t` of s3d_adam_step_multi's list as an AdamItem (false + s3d_last_error: invalid)
inline bool adam_item_from(const s3d_adam_tensor& t, int consume_grads, int k, AdamItem& o) {
    if (!(t.param && t.grad && t.exp_avg && t.exp_avg_sq)) {
        set_error("adam_step_multi: null pointer in tensor %d", k);
        return false;
    }
    if (!(t.grad_dtype == S3D_F32 || t.grad_dtype == S3D_F16)) {
        set_error("adam_step_multi: grad dtype must be f32 or f16");
        return false;
    }
    if (!((t.pack_stride == 0) || (t.pack_cols > 0 && t.pack_cols <= t.pack_stride && t.n % t.pack_cols == 0))) {
        set_error("adam_step_multi: tensor %d: packed layout needs 0 < pack_cols <= pack_stride and whole rows", k);
        return false;
    }
    o.p = t.param; o.g = const_cast<void*>(static_cast<const void*>(t.grad)); o.m = t.exp_avg; o.v = t.exp_avg_sq; o.h = (__half*)t.param_half;
    o.n = t.n; o.lr = t.lr; o.beta1 = t.beta1; o.beta2 = t.beta2; o.eps = t.eps; o.l1 = t.l1;
    o.half_grad = t.grad_dtype == S3D_F16;
    o.consume = (consume_grads || t.consume) ? 1 : 0;
    o.cols = t.pack_stride ? t.pack_cols : 1u;
    o.stride = t.pack_stride;
    const uintptr_t bits = (uintptr_t)t.param | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq |
                           ((uintptr_t)t.grad << (t.grad_dtype == S3D_F16 ? 1 : 0)) | ((uintptr_t)t.param_half << 1);
    o.vec = (bits & 15) == 0;
    return true;
}

// ------------------------------------------------------------------ (d) end of the step: loss-scale schedule and the rings
// torch.amp.GradScaler.update (aten::_amp_update_scale_): back off on overflow, grow after `interval` clean steps; then
// clear the flag for the next step (saves the separate fill launch)
__device__ __forceinline__ void scaler_update(float* __restrict__ scale, int32_t* __restrict__ growth_tracker,
                                              float* __restrict__ found_inf, float growth, float backoff, int32_t interval,
                                              float* __restrict__ adam_step) {
    if (adam_step && *found_inf == 0.0f) *adam_step += 1.0f;  // (k_adam_advance folded in: one launch less per step)
    if (*found_inf != 0.0f) {
        *scale = *scale * backoff;
        *growth_tracker = 0;
    } else {
        const int32_t ok = *growth_tracker + 1;
        if (ok == interval) {
            const float grown = *scale * growth;
            if (grown <= 3.402823466e38f) *scale = grown;  // (torch keeps the scale when growing would overflow)
            *growth_tracker = 0;
        } else {
            *growth_tracker = ok;
        }
    }
    *found_inf = 0.0f;
}
// End of a graph-replayed training step: file the step's loss and the marcher's {samples, rays} counter in their 16-slot rings
// (nerf/renderer.py keeps the counters of the last 16 steps for `mean_count`), clear the counter for the next replay and
// advance the slot — what the host otherwise does with two copies and a fill per step.
__device__ __forceinline__ void step_ring_push(const float* __restrict__ loss, int32_t* __restrict__ counter,
                                               float* __restrict__ loss_ring, int32_t* __restrict__ counter_ring,
                                               int32_t* __restrict__ cursor, int32_t ring, int32_t loss_slots) {
    int32_t c = *cursor;
    if (c < 0 || c >= ring) c = 0;
    // the loss history may be longer than the counter ring: slot = running step number % loss_slots (a tensor handed to the
    // caller for step k stays valid until step k + loss_slots); loss_slots <= 0: the counter ring's slot
    if (loss && loss_ring) loss_ring[loss_slots > 0 ? (int32_t)((uint32_t)cursor[1] % (uint32_t)loss_slots) : c] = *loss;
    counter_ring[2 * c] = counter[0];
    counter_ring[2 * c + 1] = counter[1];
    counter[0] = 0;
    counter[1] = 0;
    cursor[0] = (c + 1) % ring;
    cursor[1] += 1;
}

}  // namespace s3d
