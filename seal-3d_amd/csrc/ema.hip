// ema.hip — exponential moving average of the parameters for gfx950 (the reference's trainers keep one through torch_ema:
// nerf/utils.py:733,882 `ema.update()` after every optimizer step, main_nerf.py:147 `ema_decay=0.95`).
//
// torch_ema's update is three torch ops per tensor (tmp = s - p; tmp.mul_(c); s.sub_(tmp)): 32 B of traffic per parameter and
// three launches per tensor.  Here every tensor of the model is updated by ONE streaming launch that reads parameter and shadow
// and writes the shadow (12 B per parameter), with the same three fp32 roundings per element (the library is built with
// -ffp-contract=off), so the shadows are bit-identical to torch_ema's:
//   t = s - p;  t = t * c;  s = s - t        c = (float)(1.0 - d),  d = min(decay, (1 + n) / (10 + n)) in double
// n is the number of updates INCLUDING this one, kept in device memory (graph-capturable: a replay reads the current count)
// and advanced by a one-thread launch behind the update (k_ema_advance) — stream order is the only synchronisation, so no
// workgroup of the update can see the advanced count.
//   s3d_ema_update_multi    the update of every tensor + the count's advance
//   s3d_ema_exchange_multi  param <-> shadow in place (evaluation on the averaged weights without a third copy)
#include "s3d_common.hpp"

namespace s3d {
namespace {

constexpr int kEmaMaxTensors = 64;  // 24 B per descriptor: 1.5 KB of the 4 KB kernel-argument block
struct EmaItem {
    float* p;
    float* s;
    size_t n;
};
struct EmaBatch {
    EmaItem t[kEmaMaxTensors];
    int32_t count;
};

template <bool kExchange>
__device__ __forceinline__ void ema_element(float& p, float& s, float c) {
    if (kExchange) {
        const float t = p;
        p = s;
        s = t;
    } else {
        float t = s - p;
        t = t * c;
        s = s - t;
    }
}

// One tensor, strided over by `nthreads` threads: 16-byte accesses over the part where parameter and shadow are 16-byte
// aligned TOGETHER (equal offsets mod 16: a scalar head of up to three elements brings both there), scalar accesses for
// that head and the tail, and for the whole tensor when the two offsets differ.
template <bool kExchange>
__device__ __forceinline__ void ema_range(float* p, float* s, size_t n, float c, size_t tid, size_t nthreads) {
    const uint32_t mp = (uint32_t)((uintptr_t)p >> 2) & 3u, ms = (uint32_t)((uintptr_t)s >> 2) & 3u;
    size_t head = n, nvec = 0;
    if (mp == ms) {
        head = (4u - mp) & 3u;
        if (head > n) head = n;
        nvec = (n - head) / 4;
    }
    const size_t tail0 = head + 4 * nvec;         // first element behind the vector body
    const size_t nscalar = head + (n - tail0);    // elements [0, head) and [tail0, n)
    for (size_t i = tid; i < nscalar; i += nthreads) {
        const size_t k = i < head ? i : tail0 + (i - head);
        float a = p[k], b = s[k];
        ema_element<kExchange>(a, b, c);
        if (kExchange) p[k] = a;
        s[k] = b;
    }
    float4* pv = reinterpret_cast<float4*>(p + head);
    float4* sv = reinterpret_cast<float4*>(s + head);
    for (size_t i = tid; i < nvec; i += nthreads) {
        float4 a = pv[i], b = sv[i];
        ema_element<kExchange>(a.x, b.x, c);
        ema_element<kExchange>(a.y, b.y, c);
        ema_element<kExchange>(a.z, b.z, c);
        ema_element<kExchange>(a.w, b.w, c);
        if (kExchange) pv[i] = a;
        sv[i] = b;
    }
}

// the whole grid strides over every tensor of the batch in turn (a 12 M-element table and a 2 K-element matrix share the
// launch; a small tensor occupies the first few workgroups for one trip)
__global__ void __launch_bounds__(256) k_ema_update_multi(EmaBatch b, double decay, int use_num_updates,
                                                          const int64_t* __restrict__ num_updates) {
    double d = decay;
    if (use_num_updates) {
        const double n = (double)(*num_updates + 1);  // this update's number
        const double warm = (1.0 + n) / (10.0 + n);
        d = warm < d ? warm : d;
    }
    const float c = (float)(1.0 - d);
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    for (int i = 0; i < b.count; i++) ema_range<false>(b.t[i].p, b.t[i].s, b.t[i].n, c, tid, nthreads);
}

__global__ void __launch_bounds__(256) k_ema_exchange_multi(EmaBatch b) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    for (int i = 0; i < b.count; i++) ema_range<true>(b.t[i].p, b.t[i].s, b.t[i].n, 0.0f, tid, nthreads);
}

__global__ void k_ema_advance(int64_t* __restrict__ num_updates) { *num_updates += 1; }

// host: the launches of one call — batches of kEmaMaxTensors non-empty tensors; nothing is launched when a tensor is invalid
template <typename Launch>
int ema_batches(const s3d_ema_tensor* tensors, int32_t n_tensors, const char* what, Launch launch) {
    for (int32_t k = 0; k < n_tensors; k++) {
        const s3d_ema_tensor& t = tensors[k];
        if (t.n == 0) continue;
        if (!t.param || !t.shadow) {
            set_error("%s: null pointer in tensor %d", what, k);
            return S3D_ERR_INVALID;
        }
        if ((((uintptr_t)t.param | (uintptr_t)t.shadow) & 3) != 0) {
            set_error("%s: tensor %d is not 4-byte aligned", what, k);
            return S3D_ERR_INVALID;
        }
    }
    EmaBatch b;
    memset(&b, 0, sizeof(b));
    uint64_t total = 0;
    for (int32_t k = 0; k < n_tensors; k++) {
        const s3d_ema_tensor& t = tensors[k];
        if (t.n == 0) continue;
        b.t[b.count].p = t.param;
        b.t[b.count].s = t.shadow;
        b.t[b.count].n = t.n;
        b.count++;
        total += t.n;
        if (b.count == kEmaMaxTensors) {
            launch(b, stream_grid(total / 8 + 1, 256));
            memset(&b, 0, sizeof(b));
            total = 0;
        }
    }
    if (b.count > 0) launch(b, stream_grid(total / 8 + 1, 256));
    return S3D_OK;
}

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT int s3d_ema_update_multi(const s3d_ema_tensor* tensors, int32_t n_tensors, double decay, int use_num_updates,
                                    int64_t* num_updates, s3d_stream_t stream) {
    S3D_REQUIRE(n_tensors >= 0 && (tensors || n_tensors == 0), "ema_update_multi: null pointer");
    S3D_REQUIRE(decay >= 0.0 && decay <= 1.0, "ema_update_multi: decay must lie in [0, 1]");
    S3D_REQUIRE(num_updates || !use_num_updates, "ema_update_multi: the warm-up schedule needs the device update count");
    const int rc = ema_batches(tensors, n_tensors, "ema_update_multi", [&](const EmaBatch& b, uint32_t blocks) {
        hipLaunchKernelGGL(k_ema_update_multi, dim3(blocks), dim3(256), 0, as_stream(stream), b, decay, use_num_updates,
                           (const int64_t*)num_updates);
    });
    if (rc != S3D_OK) return rc;
    if (num_updates) hipLaunchKernelGGL(k_ema_advance, dim3(1), dim3(1), 0, as_stream(stream), num_updates);
    return check_launch("ema_update_multi");
}

S3D_EXPORT int s3d_ema_exchange_multi(const s3d_ema_tensor* tensors, int32_t n_tensors, s3d_stream_t stream) {
    S3D_REQUIRE(n_tensors >= 0 && (tensors || n_tensors == 0), "ema_exchange_multi: null pointer");
    const int rc = ema_batches(tensors, n_tensors, "ema_exchange_multi", [&](const EmaBatch& b, uint32_t blocks) {
        hipLaunchKernelGGL(k_ema_exchange_multi, dim3(blocks), dim3(256), 0, as_stream(stream), b);
    });
    if (rc != S3D_OK) return rc;
    return check_launch("ema_exchange_multi");
}
