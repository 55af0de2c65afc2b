// mesh.hip — marching cubes over a dense fp32 volume u[nx, ny, nz] (z fastest), gfx950.  The contract (solid test, edge
// ownership, vertex and triangle order, world mapping, sanitising) is DESIGN.md §8 "mesh export"; tests/mc_witness.py is
// the same contract in numpy.  The case table is generated: mc_tables.h (tools/gen_mc_tables.py).
//
// Three launches, the shape of k_compact_count / k_compact_write:
//   k_mc_count   one thread per grid point, workgroups of 1,024 consecutive points.  A point is classified (solid, which of
//                its +x/+y/+z edges cross, how many triangles the cell it anchors has) and the workgroup scans both counts;
//                the point's record holds the exclusive prefixes INSIDE its workgroup, the workgroup's sums go to `bsum`.
//   k_mc_scan    one workgroup: exclusive scan of the workgroup sums in place, totals (V, T) out.
//   k_mc_emit    one thread per point: its own vertices, and the triangles of its cell.  The id of a vertex on an edge owned
//                by corner q is  bsum[q's workgroup].v + q's prefix + (crossing edges of q before this axis): one 4-byte
//                record per corner, no search and no atomics, so the output order is fixed.
// Workspace: one uint32 record per point, two uint32 per workgroup of 1,024 points, four words of totals.
//
// No fast-math flag on this file: t = (iso - f_lo) / (f_hi - f_lo) is a correctly rounded fp32 division.
#include "s3d_common.hpp"
#define MC_TABLE static __constant__ const
#include "mc_tables.h"

#include <math.h>

namespace s3d {
namespace {

constexpr uint32_t kMcBlock = 1024;  // points per workgroup = threads per workgroup

// the record of a grid point
//   bits  0..11  vertices owned by earlier points of the workgroup (<= 3 * 1,023)
//   bits 12..24  triangles of earlier cells of the workgroup       (<= MC_MAX_TRIS * 1,023)
//   bits 25..27  which of the +x, +y, +z edges cross
//   bit  28      solid
static_assert(3u * (kMcBlock - 1) < (1u << 12), "vertex prefix does not fit");
static_assert((uint32_t)MC_MAX_TRIS * (kMcBlock - 1) < (1u << 13), "triangle prefix does not fit");
constexpr uint32_t kRecVMask = 0xFFFu, kRecTShift = 12, kRecTMask = 0x1FFFu, kRecEShift = 25, kRecSolid = 1u << 28;

struct McDims {
    uint32_t nx, ny, nz, n;  // n = nx ny nz < 2^31
};

// the field as the kernels read it: NaN -> 0, +-inf -> +-FLT_MAX (the user's volume is not modified)
__device__ __forceinline__ float mc_field(const float* __restrict__ u, uint32_t i) {
    const float f = u[i];
    return f != f ? 0.0f : fminf(fmaxf(f, -3.402823466e+38f), 3.402823466e+38f);
}

// exclusive prefix of `mine` over the 1,024 threads of the workgroup and the workgroup's sum; sh holds 16 words
__device__ __forceinline__ uint32_t mc_block_scan(uint32_t mine, uint32_t* sh, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(mine);
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kMcBlock / 64; ++w) {
        const uint32_t s = sh[w];
        if (w < wave) base += s;
        sum += s;
    }
    __syncthreads();
    *total = sum;
    return base + incl - mine;
}

__global__ void __launch_bounds__(kMcBlock) k_mc_count(const float* __restrict__ u, McDims d, float iso, uint32_t* __restrict__ rec,
                                                       uint2* __restrict__ bsum) {
    __shared__ uint32_t sh[kMcBlock / 64];
    const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
    uint32_t nv = 0, nt = 0, bits = 0;
    if (i < d.n) {
        const uint32_t z = i % d.nz, y = (i / d.nz) % d.ny, x = i / (d.nz * d.ny);
        const uint32_t sx = d.ny * d.nz, sy = d.nz;
        const bool hx = x + 1 < d.nx, hy = y + 1 < d.ny, hz = z + 1 < d.nz;
        const bool s0 = mc_field(u, i) > iso;
        const bool s1 = hx && mc_field(u, i + sx) > iso, s2 = hy && mc_field(u, i + sy) > iso, s4 = hz && mc_field(u, i + 1) > iso;
        const uint32_t em = (uint32_t)(hx && s1 != s0) | (uint32_t)(hy && s2 != s0) << 1 | (uint32_t)(hz && s4 != s0) << 2;
        nv = __popc(em);
        if (hx && hy && hz) {
            const uint32_t c = (uint32_t)s0 | (uint32_t)s1 << 1 | (uint32_t)s2 << 2 | (uint32_t)(mc_field(u, i + sx + sy) > iso) << 3 |
                               (uint32_t)s4 << 4 | (uint32_t)(mc_field(u, i + sx + 1) > iso) << 5 |
                               (uint32_t)(mc_field(u, i + sy + 1) > iso) << 6 | (uint32_t)(mc_field(u, i + sx + sy + 1) > iso) << 7;
            nt = kMcTriCount[c];
        }
        bits = em << kRecEShift | (s0 ? kRecSolid : 0u);
    }
    uint32_t total;
    const uint32_t pre = mc_block_scan(nv | nt << 16, sh, &total);  // both sums stay below 2^16: one scan carries the pair
    if (i < d.n) rec[i] = (pre & 0xFFFFu) | (pre >> 16) << kRecTShift | bits;
    if (threadIdx.x == 0) bsum[blockIdx.x] = make_uint2(total & 0xFFFFu, total >> 16);
}

// totals: [0] V, [1] T, [2] 1 when either count does not fit 32 bits (then V = T = 0xFFFFFFFF), [3] unused
constexpr uint32_t kMcScanPer = 8;  // workgroup sums per thread and pass
__global__ void __launch_bounds__(kMcBlock) k_mc_scan(uint2* __restrict__ bsum, uint32_t nb, uint32_t* __restrict__ totals_ws,
                                                      uint32_t* __restrict__ totals_out) {
    __shared__ uint32_t sh[kMcBlock / 64];
    uint64_t cv = 0, ct = 0;  // (a pass adds at most 8,192 * 5,120 to either: the 32-bit scans inside a pass cannot wrap)
    for (uint64_t b0 = 0; b0 < nb; b0 += kMcBlock * kMcScanPer) {
        const uint64_t first = b0 + threadIdx.x * kMcScanPer;
        uint2 mine[kMcScanPer];
        uint32_t sv = 0, st = 0;
#pragma unroll
        for (uint32_t k = 0; k < kMcScanPer; ++k) {
            mine[k] = first + k < nb ? bsum[first + k] : make_uint2(0u, 0u);
            sv += mine[k].x;
            st += mine[k].y;
        }
        uint32_t tv, tt;
        uint32_t pv = (uint32_t)cv + mc_block_scan(sv, sh, &tv), pt = (uint32_t)ct + mc_block_scan(st, sh, &tt);
#pragma unroll
        for (uint32_t k = 0; k < kMcScanPer; ++k) {
            if (first + k < nb) bsum[first + k] = make_uint2(pv, pt);
            pv += mine[k].x;
            pt += mine[k].y;
        }
        cv += tv;
        ct += tt;
    }
    if (threadIdx.x == 0) {
        const bool over = cv >= 0xFFFFFFFFull || ct >= 0xFFFFFFFFull;
        const uint32_t V = over ? 0xFFFFFFFFu : (uint32_t)cv, T = over ? 0xFFFFFFFFu : (uint32_t)ct;
        totals_ws[0] = V; totals_ws[1] = T; totals_ws[2] = over; totals_ws[3] = 0;
        totals_out[0] = V; totals_out[1] = T;
    }
}

__global__ void __launch_bounds__(kMcBlock) k_mc_emit(const float* __restrict__ u, McDims d, float iso, const uint32_t* __restrict__ rec,
                                                      const uint2* __restrict__ bsum, const float* __restrict__ bounds,
                                                      float* __restrict__ vertices, uint32_t V, int32_t* __restrict__ triangles,
                                                      uint32_t T) {
    const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
    if (i >= d.n) return;
    const uint32_t r = rec[i];
    const uint32_t em = (r >> kRecEShift) & 7u;
    const uint32_t z = i % d.nz, y = (i / d.nz) % d.ny, x = i / (d.nz * d.ny);
    const uint32_t sx = d.ny * d.nz, sy = d.nz;
    const uint2 base = bsum[blockIdx.x];
    if (em) {
        const float f_lo = mc_field(u, i);
        const uint32_t stride[3] = {sx, sy, 1u}, dim[3] = {d.nx, d.ny, d.nz};
        uint32_t vid = base.x + (r & kRecVMask);
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) {
            if (!(em >> a & 1u)) continue;
            const float f_hi = mc_field(u, i + stride[a]);
            float t = (iso - f_lo) / (f_hi - f_lo);
            t = fminf(fmaxf(t, 0.0f), 1.0f);  // (already there unless iso - f_lo overflowed; NaN -> 0)
            float p[3] = {(float)x, (float)y, (float)z};
            p[a] = p[a] + t;
            if (vid < V) {  // (always, when V is the counted total)
#pragma unroll
                for (uint32_t k = 0; k < 3; ++k)
                    vertices[(size_t)vid * 3 + k] = p[k] / (float)(dim[k] - 1) * (bounds[3 + k] - bounds[k]) + bounds[k];
            }
            ++vid;
        }
    }
    if (x + 1 >= d.nx || y + 1 >= d.ny || z + 1 >= d.nz) return;
    // the records of the cell's eight corners: corner c = dx + 2 dy + 4 dz
    uint32_t rc[8], blk[8];
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
        const uint32_t q = i + (c & 1u) * sx + (c >> 1 & 1u) * sy + (c >> 2);
        rc[c] = c ? rec[q] : r;
        blk[c] = q / kMcBlock;
    }
    uint32_t cs = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) cs |= (rc[c] >> 28 & 1u) << c;
    const uint32_t nt = kMcTriCount[cs];
    if (!nt) return;
    uint32_t tid = base.y + ((r >> kRecTShift) & kRecTMask);
    for (uint32_t k = 0; k < nt; ++k, ++tid) {
        int32_t id[3];
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
            const uint32_t e = (uint32_t)kMcTriTable[cs][3 * k + j];
            const uint32_t a = kMcEdgeAxis[e], c = kMcEdgeOwner[e];  // the edge runs along a from corner c of the cell
            uint32_t rq = rc[0], bq = blk[0];
#pragma unroll
            for (uint32_t s = 1; s < 8; ++s)  // (select, not index: rc / blk stay in registers)
                if (s == c) { rq = rc[s]; bq = blk[s]; }
            const uint32_t before = __popc((rq >> kRecEShift) & ((1u << a) - 1u));
            id[j] = (int32_t)(bsum[bq].x + (rq & kRecVMask) + before);
        }
        if (tid < T) {  // (always, when T is the counted total)
            triangles[(size_t)tid * 3] = id[0]; triangles[(size_t)tid * 3 + 1] = id[1]; triangles[(size_t)tid * 3 + 2] = id[2];
        }
    }
}

struct McLayout {
    uint32_t nb;
    size_t rec_off, bsum_off, totals_off, bytes;
};

McLayout mc_layout(uint64_t n) {
    McLayout l;
    l.nb = (uint32_t)div_up<uint64_t>(n, kMcBlock);
    l.totals_off = 0;                                   // 4 words
    l.bsum_off = 16;                                    // uint2 [nb]
    l.rec_off = l.bsum_off + sizeof(uint2) * (size_t)l.nb;  // uint32 [n]
    l.bytes = l.rec_off + sizeof(uint32_t) * (size_t)n;
    return l;
}

int mc_check_dims(uint32_t nx, uint32_t ny, uint32_t nz, const char* what) {
    S3D_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: every axis needs at least 2 points (%u x %u x %u)", what, nx, ny, nz);
    S3D_REQUIRE(nx < (1u << 31) && ny < (1u << 31) && nz < (1u << 31) && (uint64_t)nx * ny < (1ull << 31) &&
                    (uint64_t)nx * ny * nz < (1ull << 31),
                "%s: %u x %u x %u is 2^31 points or more", what, nx, ny, nz);
    return S3D_OK;
}

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT size_t s3d_mc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (mc_check_dims(nx, ny, nz, "mc_workspace_bytes") != S3D_OK) return 0;
    return mc_layout((uint64_t)nx * ny * nz).bytes;
}

S3D_EXPORT int s3d_mc_count(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void* workspace, uint32_t* totals,
                            s3d_stream_t stream) {
    if (int rc = mc_check_dims(nx, ny, nz, "mc_count")) return rc;
    S3D_REQUIRE(u && workspace && totals, "mc_count: null pointer");
    S3D_REQUIRE(iso == iso && fabsf(iso) <= 3.402823466e+38f, "mc_count: iso must be finite");
    S3D_REQUIRE(((uintptr_t)workspace & 15u) == 0, "mc_count: the workspace must be 16-byte aligned");
    const McDims d{nx, ny, nz, nx * ny * nz};
    const McLayout l = mc_layout(d.n);
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(k_mc_count, dim3(l.nb), dim3(kMcBlock), 0, as_stream(stream), u, d, iso, (uint32_t*)(ws + l.rec_off),
                       (uint2*)(ws + l.bsum_off));
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(kMcBlock), 0, as_stream(stream), (uint2*)(ws + l.bsum_off), l.nb,
                       (uint32_t*)(ws + l.totals_off), totals);
    return check_launch("mc_count");
}

S3D_EXPORT int s3d_mc_emit(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float iso, const void* workspace, const float* bounds,
                           float* vertices, uint32_t V, int32_t* triangles, uint32_t T, s3d_stream_t stream) {
    if (int rc = mc_check_dims(nx, ny, nz, "mc_emit")) return rc;
    S3D_REQUIRE(u && workspace && bounds, "mc_emit: null pointer");
    S3D_REQUIRE((vertices || V == 0) && (triangles || T == 0), "mc_emit: null output");
    const McDims d{nx, ny, nz, nx * ny * nz};
    const McLayout l = mc_layout(d.n);
    const char* ws = (const char*)workspace;
    // the totals s3d_mc_count left in the workspace: the buffers must have exactly that many rows (one small read-back;
    // an export is not part of a training step)
    uint32_t counted[4] = {0, 0, 0, 0};
    S3D_HIP(hipMemcpyAsync(counted, ws + l.totals_off, sizeof(counted), hipMemcpyDeviceToHost, as_stream(stream)));
    S3D_HIP(hipStreamSynchronize(as_stream(stream)));
    S3D_REQUIRE(!counted[2], "mc_emit: more than 2^32 - 2 vertices or triangles");
    S3D_REQUIRE(counted[0] == V && counted[1] == T, "mc_emit: V = %u, T = %u passed, %u and %u counted", V, T, counted[0], counted[1]);
    if (V == 0 && T == 0) return S3D_OK;
    hipLaunchKernelGGL(k_mc_emit, dim3(l.nb), dim3(kMcBlock), 0, as_stream(stream), u, d, iso, (const uint32_t*)(ws + l.rec_off),
                       (const uint2*)(ws + l.bsum_off), bounds, vertices, V, triangles, T);
    return check_launch("mc_emit");
}
