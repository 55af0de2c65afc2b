// ordered_sum.hpp — the deterministic fp32 sum across the workgroups of one launch: no float atomics, the same bits on every run.
//
//   a lane         its own terms in index order (the caller's loop)
//   a wave         __shfl_down by 32, 16, 8, 4, 2, 1: lane 0 holds the sum
//   a workgroup    its four waves in index order, ((p0 + p1) + p2) + p3, by thread 0: one fp32 partial per workgroup
//   the launch     the last workgroup to take a ticket: lane i adds the partials i, i + 256, ... in index order from 0, then the
//                  same wave and workgroup steps
//
// Hand-over: a partial is a write-through (agent-scope atomic) store, drained by the wave that made it before its lane 0 takes
// the ticket with a relaxed agent-scope add.  There is no release fence: it would write back every line the workgroup has just
// left in its XCD's L2 (profiles/dnerf_basis.md, profiles/ordered_sum.md).  The last workgroup acquires, reads the partials past
// its L1 and leaves the ticket at zero for the next launch.
// (k_l1_pair in ngp_head.hip is not a user: it adds its waves as (p0 + p1) + (p2 + p3) and its caller zeroes the ticket.)
#pragma once
#include "s3d_common.hpp"

namespace s3d {
namespace {

constexpr uint32_t kSumBlock = 256;  // lanes of a workgroup that sums

struct SumShared {  // one per kernel, in LDS
    float part[kSumBlock / 64];
    uint32_t is_last;
};

// every lane's v -> the workgroup's sum in thread 0 (other threads: unspecified).  All 256 threads call it.
__device__ __forceinline__ float block_sum(float v, SumShared& sh) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63u) == 0) sh.part[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.0f;
    if (threadIdx.x == 0) {
        r = sh.part[0];
        for (uint32_t w = 1; w < kSumBlock / 64; w++) r += sh.part[w];
    }
    return r;
}

// The hand-over behind the write-through stores of this workgroup's partials, all of which wave 0 has issued: wave 0 drains them,
// thread 0 takes the ticket.  All threads call it; true in every thread of the last of `n_groups` workgroups to arrive, which may
// then read every workgroup's partials with agent-scope atomic loads and must leave `*ticket = 0`.  (Reads of `sh.part` made
// before the call lie before its barrier: the last workgroup may write it again.)
__device__ __forceinline__ bool ordered_sum_arrive(uint32_t* ticket, uint32_t n_groups, SumShared& sh) {
    if (threadIdx.x < 64) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) {
            const uint32_t arrived = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool last = arrived == n_groups - 1;
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            sh.is_last = last ? 1u : 0u;
        }
    }
    __syncthreads();
    return sh.is_last != 0;  // (workgroup-uniform)
}

// `v0`: block_sum's result of workgroup `slot` of `n_groups` (thread 0's value counts).  All threads call it; true in thread 0 of
// the last workgroup to arrive, with the sum of all partials in `total`.
__device__ __forceinline__ bool ordered_sum_finish(float v0, float* partials, uint32_t* ticket, uint32_t n_groups, uint32_t slot,
                                                   SumShared& sh, float& total) {
    if (threadIdx.x == 0) __hip_atomic_store(partials + slot, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ordered_sum_arrive(ticket, n_groups, sh)) return false;
    float v = 0.0f;
    for (uint32_t i = threadIdx.x; i < n_groups; i += kSumBlock)
        v += __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    total = block_sum(v, sh);
    if (threadIdx.x != 0) return false;
    *ticket = 0u;
    return true;
}

// Host side: the caller's workspace is [ticket (16 bytes) | `floats` fp32 partials]
struct SumWorkspace {
    uint32_t* ticket = nullptr;
    float* partials = nullptr;
    static size_t bytes(size_t floats) { return 16 + sizeof(float) * floats; }
    static bool fits(const void* ws, size_t ws_bytes, size_t floats) {
        return ws && ws_bytes >= bytes(floats) && (uintptr_t)ws % 16 == 0;
    }
    hipError_t arm(void* ws, hipStream_t st) {  // split, ticket = 0
        ticket = (uint32_t*)ws;
        partials = (float*)((char*)ws + 16);
        return hipMemsetAsync(ticket, 0, 16, st);
    }
};

}  // namespace
}  // namespace s3d
