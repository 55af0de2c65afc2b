// optim.hip — the parameter update of the training step for gfx950: Adam straight from the fp16 gradients.
//
// The reference trains with torch.optim.Adam + torch.cuda.amp.GradScaler (nerf/utils.py:356-361,
// main_SealNeRF.py:283-288: betas (0.9, 0.99), eps 1e-15).  Around a 12.2 M-entry hash table that costs, per step:
// table fp32->fp16 cast for the forward (73 MB), fp16->fp32 gradient cast (73 MB), gradient accumulate (147 MB),
// non-finite check + unscale (98 MB) and the Adam pass itself (343 MB) — ~0.7 GB of HBM traffic for an update
// whose inputs are a 24.5 MB fp16 gradient.  Here the gradient is consumed where the backward kernel left it:
//   s3d_grads_nonfinite  one read of the gradient, raises the found_inf flag (GradScaler semantics)
//   s3d_adam_step        p, m, v (fp32) <- Adam(g / grad_scale), skipped as a whole when found_inf is set; optionally
//                        writes the fp16 copy of p that the next forward (autocast) reads instead of re-casting
// Update rule = torch's fused Adam functor (no amsgrad, no weight decay, maximize off), fp32 math:
//   m += (1-b1)(g - m);  v = b2 v + (1-b2) g^2;  p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// with the step count t kept on the device (graph-capturable) and advanced only by steps that are not skipped.
#include "s3d_common.hpp"
#include "s3d_adam.hpp"
#include "s3d_step_tail.hpp"

namespace s3d {
namespace {

template <typename G>
__global__ void __launch_bounds__(256) k_grads_nonfinite(const G* __restrict__ g, size_t n, float* __restrict__ found_inf) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = grad_to_f<G>(g[i]);
        bad |= !(fabsf(v) <= 3.402823466e38f);  // inf or NaN
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) *found_inf = 1.0f;  // benign race: everyone writes 1
}

// (GradVec4, clear_range, adam_range, adam_range_packed, AdamItem: s3d_step_tail.hpp — shared with the grid backward's riders)

// Four consecutive elements per lane and trip (16-byte accesses of the fp32 state, 8-byte of the fp16 gradient / copy): the
// update streams 28 B per element and is HBM-bound; `vec` is false for a tensor whose pointers are not 16-byte aligned.
template <typename G>
__global__ void __launch_bounds__(256) k_adam_step(float* __restrict__ p, const G* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, __half* __restrict__ p_half, size_t n, float lr,
                                                   float beta1, float beta2, float eps, const float* __restrict__ step,
                                                   const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                   const float* __restrict__ lr_scale, uint32_t vec) {
    if (found_inf && *found_inf != 0.0f) return;  // the whole step is skipped (GradScaler.step)
    const AdamCoef c = adam_coef(lr, beta1, beta2, eps, 0.0f, step, grad_scale, lr_scale);
    adam_range<G>(c, p, const_cast<G*>(g), m, v, p_half, n, vec != 0, (size_t)blockIdx.x * 256 + threadIdx.x,
                  (size_t)gridDim.x * 256, false);
}

// Every tensor of the optimizer in ONE launch (the hot path updates a 12 M-element hash table and two ~10 K-element MLPs: the
// small ones cost a launch each otherwise).  Blocks [first_block[i], first_block[i+1]) stride over tensor i.
constexpr int kAdamMaxTensors = 16;
struct AdamBatch {
    AdamItem t[kAdamMaxTensors];
    uint32_t first_block[kAdamMaxTensors + 1];
    int32_t count;
};

__global__ void __launch_bounds__(256) k_adam_step_multi(AdamBatch b, const float* __restrict__ step,
                                                         const float* __restrict__ grad_scale,
                                                         const float* __restrict__ found_inf,
                                                         const float* __restrict__ lr_scale) {
    int i = 0;
    while (i + 1 < b.count && blockIdx.x >= b.first_block[i + 1]) i++;
    const size_t tid = (size_t)(blockIdx.x - b.first_block[i]) * 256 + threadIdx.x;
    const size_t nthreads = (size_t)(b.first_block[i + 1] - b.first_block[i]) * 256;
    adam_item_run(b.t[i], found_inf && *found_inf != 0.0f, step, grad_scale, lr_scale, tid, nthreads);
}

__global__ void k_adam_advance(float* __restrict__ step, const float* __restrict__ found_inf) {
    if (!(found_inf && *found_inf != 0.0f)) *step += 1.0f;
}

// (scaler_update, step_ring_push: s3d_step_tail.hpp)
__global__ void k_scaler_update(float* __restrict__ scale, int32_t* __restrict__ growth_tracker, float* __restrict__ found_inf,
                                float growth, float backoff, int32_t interval, float* __restrict__ adam_step) {
    scaler_update(scale, growth_tracker, found_inf, growth, backoff, interval, adam_step);
}

__global__ void k_step_ring_push(const float* __restrict__ loss, int32_t* __restrict__ counter, float* __restrict__ loss_ring,
                                 int32_t* __restrict__ counter_ring, int32_t* __restrict__ cursor, int32_t ring, int32_t loss_slots) {
    step_ring_push(loss, counter, loss_ring, counter_ring, cursor, ring, loss_slots);
}
// both single-thread epilogues of a step in one launch
__global__ void k_step_epilogue(float* __restrict__ scale, int32_t* __restrict__ growth_tracker, float* __restrict__ found_inf,
                                float growth, float backoff, int32_t interval, float* __restrict__ adam_step,
                                const float* __restrict__ loss, int32_t* __restrict__ counter, float* __restrict__ loss_ring,
                                int32_t* __restrict__ counter_ring, int32_t* __restrict__ cursor, int32_t ring, int32_t loss_slots) {
    scaler_update(scale, growth_tracker, found_inf, growth, backoff, interval, adam_step);
    step_ring_push(loss, counter, loss_ring, counter_ring, cursor, ring, loss_slots);
}

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT int s3d_grads_nonfinite(const void* grad, size_t n, int dtype, float* found_inf, s3d_stream_t stream) {
    if (n == 0) return S3D_OK;
    S3D_REQUIRE(grad && found_inf, "grads_nonfinite: null pointer");
    S3D_REQUIRE(dtype == S3D_F32 || dtype == S3D_F16, "grads_nonfinite: dtype must be f32 or f16");
    const uint32_t grid = stream_grid(n / 8 + 1, 256);
    if (dtype == S3D_F16)
        hipLaunchKernelGGL(k_grads_nonfinite<__half>, dim3(grid), dim3(256), 0, as_stream(stream), (const __half*)grad, n, found_inf);
    else
        hipLaunchKernelGGL(k_grads_nonfinite<float>, dim3(grid), dim3(256), 0, as_stream(stream), (const float*)grad, n, found_inf);
    return check_launch("grads_nonfinite");
}

S3D_EXPORT int s3d_adam_step(float* param, const void* grad, int grad_dtype, float* exp_avg, float* exp_avg_sq,
                             uint16_t* param_half, size_t n, float lr, float beta1, float beta2, float eps,
                             const float* step, const float* grad_scale, const float* found_inf, const float* lr_scale,
                             s3d_stream_t stream) {
    if (n == 0) return S3D_OK;
    S3D_REQUIRE(param && grad && exp_avg && exp_avg_sq && step, "adam_step: null pointer");
    S3D_REQUIRE(grad_dtype == S3D_F32 || grad_dtype == S3D_F16, "adam_step: grad dtype must be f32 or f16");
    const uint32_t grid = stream_grid(n / 8 + 1, 256);
    const uintptr_t bits = (uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | ((uintptr_t)grad << (grad_dtype == S3D_F16 ? 1 : 0)) |
                           ((uintptr_t)param_half << 1);
    const uint32_t vec = (bits & 15) == 0;
    if (grad_dtype == S3D_F16)
        hipLaunchKernelGGL(k_adam_step<__half>, dim3(grid), dim3(256), 0, as_stream(stream), param, (const __half*)grad, exp_avg,
                           exp_avg_sq, (__half*)param_half, n, lr, beta1, beta2, eps, step, grad_scale, found_inf, lr_scale, vec);
    else
        hipLaunchKernelGGL(k_adam_step<float>, dim3(grid), dim3(256), 0, as_stream(stream), param, (const float*)grad, exp_avg,
                           exp_avg_sq, (__half*)param_half, n, lr, beta1, beta2, eps, step, grad_scale, found_inf, lr_scale, vec);
    return check_launch("adam_step");
}

S3D_EXPORT int s3d_adam_step_multi(const s3d_adam_tensor* tensors, int32_t n_tensors, const float* step, const float* grad_scale,
                                   const float* found_inf, const float* lr_scale, int consume_grads, s3d_stream_t stream) {
    S3D_REQUIRE(n_tensors >= 0 && (tensors || n_tensors == 0) && step, "adam_step_multi: null pointer");
    for (int32_t base = 0; base < n_tensors; base += kAdamMaxTensors) {
        AdamBatch b;
        memset(&b, 0, sizeof(b));
        uint32_t blocks = 0;
        for (int32_t k = base; k < n_tensors && k < base + kAdamMaxTensors; k++) {  // (exactly this batch's index range)
            const s3d_adam_tensor& t = tensors[k];
            if (t.n == 0) continue;
            if (!adam_item_from(t, consume_grads, k, b.t[b.count])) return S3D_ERR_INVALID;
            const int i = b.count++;
            b.first_block[i] = blocks;
            blocks += stream_grid(t.n / 8 + 1, 256);
            b.first_block[i + 1] = blocks;
        }
        if (b.count == 0) continue;
        hipLaunchKernelGGL(k_adam_step_multi, dim3(blocks), dim3(256), 0, as_stream(stream), b, step, grad_scale, found_inf, lr_scale);
    }
    return check_launch("adam_step_multi");
}

S3D_EXPORT int s3d_adam_advance(float* step, const float* found_inf, s3d_stream_t stream) {
    S3D_REQUIRE(step, "adam_advance: null pointer");
    hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, as_stream(stream), step, found_inf);
    return check_launch("adam_advance");
}

S3D_EXPORT int s3d_scaler_update(float* scale, int32_t* growth_tracker, float* found_inf, float growth_factor,
                                 float backoff_factor, int32_t growth_interval, float* adam_step, s3d_stream_t stream) {
    S3D_REQUIRE(scale && growth_tracker && found_inf, "scaler_update: null pointer");
    hipLaunchKernelGGL(k_scaler_update, dim3(1), dim3(1), 0, as_stream(stream), scale, growth_tracker, found_inf, growth_factor,
                       backoff_factor, growth_interval, adam_step);
    return check_launch("scaler_update");
}

S3D_EXPORT int s3d_step_ring_push(const float* loss, int32_t* counter, float* loss_ring, int32_t* counter_ring, int32_t* cursor,
                                  int32_t ring, int32_t loss_slots, s3d_stream_t stream) {
    S3D_REQUIRE(counter && counter_ring && cursor && ring > 0, "step_ring_push: null pointer or empty ring");
    hipLaunchKernelGGL(k_step_ring_push, dim3(1), dim3(1), 0, as_stream(stream), loss, counter, loss_ring, counter_ring, cursor, ring, loss_slots);
    return check_launch("step_ring_push");
}

S3D_EXPORT int s3d_step_epilogue(float* scale, int32_t* growth_tracker, float* found_inf, float growth_factor,
                                 float backoff_factor, int32_t growth_interval, float* adam_step, const float* loss,
                                 int32_t* counter, float* loss_ring, int32_t* counter_ring, int32_t* cursor, int32_t ring,
                                 int32_t loss_slots, s3d_stream_t stream) {
    S3D_REQUIRE(scale && growth_tracker && found_inf, "step_epilogue: null pointer (scaler)");
    S3D_REQUIRE(counter && counter_ring && cursor && ring > 0, "step_epilogue: null pointer or empty ring");
    hipLaunchKernelGGL(k_step_epilogue, dim3(1), dim3(1), 0, as_stream(stream), scale, growth_tracker, found_inf, growth_factor,
                       backoff_factor, growth_interval, adam_step, loss, counter, loss_ring, counter_ring, cursor, ring, loss_slots);
    return check_launch("step_epilogue");
}
