// tensorf_cp.hip — TensoRF CP (CANDECOMP/PARAFAC) features: three line factors per component, no planes
// (tensoRF/network_cp.py:78-111 of the reference: get_sigma_feat / get_color_feat).
//
// The reference samples three line factors [1,R,D_i,1] with F.grid_sample (bilinear, zeros padding, align_corners=True; the
// lines as "fake 2-D" images of width 1: the x tap is column 0 with weight exactly 1), multiplies the three [R,N] results
// and sums them over R (density) or sends them through basis_mat (colour).  Line i runs along coordinate vec_ids[i] = 2 - i.
// Per point and line: p = ((u + 1) / 2) * (D - 1), i0 = floor(p), value = v[i0] * ((i0 + 1) - p) + v[i0 + 1] * (p - i0), a tap
// outside [0, D - 1] counts as zero; the product is (l0 * l1) * l2.
//
// Forward: one lane per point, the rank loop inside the lane; with the rank-fastest shadows ([D][R], s3d_cp_transpose_lines) a
// tap's channels are one contiguous run read four at a time, and the factor set (1.4 MB at the defaults) stays in L2.
// Backward: the points arrive sorted by 64-row chunk of line i (s3d_vm_backward_bins, rows 3-5).  A workgroup owns up to
// kCpPts (1,024) sorted points of ONE chunk and ONE slice of 32 rank channels; each of its four half-waves keeps a private
// [65 cells][32 ranks] fp32 tile in LDS (lane = rank channel: a lane only ever touches its own column, so the adds are plain
// read-modify-writes, no LDS atomics), the four tiles are summed in a fixed order and every cell leaves with ONE global atomic
// per workgroup.  Non-finite gradients travel through the fp32 sums as they are.  The tiles leave room for 2 waves per SIMD,
// so the point loop is a software pipeline over its dependent loads (profiles/tensorf_cp.md).
#include "s3d_common.hpp"
#include <algorithm>

namespace s3d {
namespace {

constexpr uint32_t kCpBasisPad = 32;                   // output channels of basis_mat held per lane (27 in the model)
constexpr uint32_t kCpChunk = 64;                      // rows per line chunk of the sort (tensorf.hip: kVmZChunk)
constexpr uint32_t kCpCells = kCpChunk + 1;            // a chunk's taps reach one row into the next chunk
constexpr uint32_t kCpLanes = 32;                      // rank channels per slice
constexpr uint32_t kCpGroups = 4;                      // half-waves (private tiles) per workgroup: 4 x 8,320 B = 33 KB of LDS
constexpr uint32_t kCpBwdThreads = kCpLanes * kCpGroups;
constexpr uint32_t kCpPts = 1024;                      // sorted points per workgroup

struct CpLines {
    const float* line[3];    // [R][D_i]
    const float* line_t[3];  // [D_i][R] (optional shadows), all three or none
    uint32_t D[3];           // D_i = resolution[vec_ids[i]]
    uint32_t R;
    uint32_t vec4;           // shadows present, 16-byte aligned, R % 4 == 0: the forwards read four ranks per load
};

struct CpTap {
    float w0, w1;
    int i0;
    bool b0, b1;
};

__device__ __forceinline__ float cp_unnormalize(float c, uint32_t size) { return ((c + 1.0f) / 2.0f) * (float)(size - 1); }

__device__ __forceinline__ CpTap cp_locate(float u, uint32_t D) {
    CpTap t;
    const float p = cp_unnormalize(u, D), fl = floorf(p);
    t.w1 = p - fl;
    t.w0 = (fl + 1.0f) - p;
    const bool ok = fabsf(p) < 1e9f;  // (non-finite coordinates: both taps out of range)
    t.i0 = ok ? (int)fl : -2;
    t.b0 = t.i0 >= 0 && t.i0 < (int)D;
    t.b1 = t.i0 + 1 >= 0 && t.i0 + 1 < (int)D;
    return t;
}

// line i of rank channel r at a located point, from the shadows when there are any
__device__ __forceinline__ float cp_value(const CpLines& f, uint32_t i, const CpTap& t, uint32_t r) {
    float l = 0.0f;
    if (f.line_t[i]) {
        const float* L = f.line_t[i] + r;
        if (t.b0) l += L[(size_t)t.i0 * f.R] * t.w0;
        if (t.b1) l += L[(size_t)(t.i0 + 1) * f.R] * t.w1;
    } else {
        const float* L = f.line[i] + (size_t)r * f.D[i];
        if (t.b0) l += L[t.i0] * t.w0;
        if (t.b1) l += L[t.i0 + 1] * t.w1;
    }
    return l;
}

// the products of ranks r0 .. r0 + 3 through 16-byte loads of the shadows
__device__ __forceinline__ void cp_products4(const CpLines& f, const CpTap* t, uint32_t r0, float* prod) {
    float l[3][4];
#pragma unroll
    for (uint32_t i = 0; i < 3; i++) {
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 a = t[i].b0 ? *reinterpret_cast<const float4*>(f.line_t[i] + (size_t)t[i].i0 * f.R + r0) : z;
        const float4 c = t[i].b1 ? *reinterpret_cast<const float4*>(f.line_t[i] + (size_t)(t[i].i0 + 1) * f.R + r0) : z;
        const float va[4] = {a.x, a.y, a.z, a.w}, vc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            float v = 0.0f;
            if (t[i].b0) v += va[k] * t[i].w0;
            if (t[i].b1) v += vc[k] * t[i].w1;
            l[i][k] = v;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) prod[k] = (l[0][k] * l[1][k]) * l[2][k];
}

__device__ __forceinline__ void cp_locate3(const float* __restrict__ x, uint32_t n, const CpLines& f, CpTap* t) {
#pragma unroll
    for (uint32_t i = 0; i < 3; i++) t[i] = cp_locate(x[(size_t)n * 3 + (2u - i)], f.D[i]);
}

template <bool REDUCE>
__global__ void __launch_bounds__(256) k_cp_features(const float* __restrict__ x, uint32_t N, CpLines f, float* __restrict__ out,
                                                     const int32_t* __restrict__ n_valid) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= valid_rows(N, n_valid)) return;  // (a padded sample batch: rows behind the device-side count are absent)
    CpTap t[3];
    cp_locate3(x, n, f, t);
    float total = 0.0f;
    if (f.vec4) {
        for (uint32_t r0 = 0; r0 < f.R; r0 += 4) {
            float prod[4];
            cp_products4(f, t, r0, prod);
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                if (REDUCE) total += prod[k];
                else out[(size_t)(r0 + k) * N + n] = prod[k];
            }
        }
    } else {
        for (uint32_t r = 0; r < f.R; r++) {
            const float prod = (cp_value(f, 0, t[0], r) * cp_value(f, 1, t[1], r)) * cp_value(f, 2, t[2], r);
            if (REDUCE) total += prod;
            else out[(size_t)r * N + n] = prod;
        }
    }
    if (REDUCE) out[n] = total;
}

// ---- the colour features with basis_mat applied on the spot (tensoRF/network_cp.py:105-109: basis_mat(vec_feat.T)) ----
// out[n][c] = half(sum_r half(W[c][r]) * half(prod[r])) with fp32 accumulation, the arithmetic s3d_vm_color_forward defines;
// W sits in LDS as fp32 [R][kCpBasisPad], every lane reads the same row (broadcast).  The [R, N] products are never written.
__global__ void __launch_bounds__(256) k_cp_color_basis(const float* __restrict__ x, uint32_t N, CpLines f, const _Float16* __restrict__ basis,
                                                        uint32_t Cb, _Float16* __restrict__ out, const int32_t* __restrict__ n_valid) {
    extern __shared__ float cp_smem[];  // [R][kCpBasisPad]
    if (blockIdx.x * 256 >= valid_rows(N, n_valid)) return;
    for (uint32_t e = threadIdx.x; e < f.R * kCpBasisPad; e += 256) {
        const uint32_t row = e / kCpBasisPad, c = e % kCpBasisPad;
        cp_smem[e] = c < Cb ? (float)basis[(size_t)c * f.R + row] : 0.0f;
    }
    __syncthreads();
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= valid_rows(N, n_valid)) return;
    CpTap t[3];
    cp_locate3(x, n, f, t);
    float acc[kCpBasisPad];
#pragma unroll
    for (uint32_t c = 0; c < kCpBasisPad; c++) acc[c] = 0.0f;
    auto to_basis = [&](float prod, uint32_t r) {
        const float4* wrow = reinterpret_cast<const float4*>(cp_smem + (size_t)r * kCpBasisPad);
#pragma unroll
        for (uint32_t q = 0; q < kCpBasisPad / 4; q++) {
            const float4 w = wrow[q];
            acc[4 * q] = __builtin_fmaf(prod, w.x, acc[4 * q]);
            acc[4 * q + 1] = __builtin_fmaf(prod, w.y, acc[4 * q + 1]);
            acc[4 * q + 2] = __builtin_fmaf(prod, w.z, acc[4 * q + 2]);
            acc[4 * q + 3] = __builtin_fmaf(prod, w.w, acc[4 * q + 3]);
        }
    };
    if (f.vec4) {
        for (uint32_t r0 = 0; r0 < f.R; r0 += 4) {
            float prod[4];
            cp_products4(f, t, r0, prod);
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) to_basis((float)(_Float16)prod[k], r0 + k);  // (the autocast Linear's fp16 input)
        }
    } else {
        for (uint32_t r = 0; r < f.R; r++)
            to_basis((float)(_Float16)((cp_value(f, 0, t[0], r) * cp_value(f, 1, t[1], r)) * cp_value(f, 2, t[2], r)), r);
    }
    _Float16* o = out + (size_t)n * Cb;
#pragma unroll
    for (uint32_t c = 0; c < kCpBasisPad; c++)
        if (c < Cb) o[c] = (_Float16)acc[c];
}

// [R][D] -> [D][R] for the three lines (1.4 MB at the defaults: element-wise, the reads come out of L2)
__global__ void __launch_bounds__(256) k_cp_transpose_lines(CpLines f, float* const t0, float* const t1, float* const t2) {
    const uint32_t i = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    const uint32_t D = f.D[i];
    if (e >= D * f.R) return;
    float* dst = i == 0 ? t0 : i == 1 ? t1 : t2;
    const uint32_t c = e / f.R, r = e % f.R;
    dst[e] = f.line[i][(size_t)r * D + c];
}

// ------------------------------------------------------------------ backward (parameter gradients)
struct CpBackward {
    float* d_line[3];        // [R][D_i], zero-initialised
    const float* g;          // MODE 0: [N]; MODE 1: [N][R] point-major
    const _Float16* g_out;   // MODE 2: [N][kCpBasisPad], zero-padded rows (64 bytes, 16-byte aligned)
    const _Float16* basis;   // MODE 2: [Cb][R]
    float* d_basis;          // MODE 2: [Cb][R] fp32, zero-initialised
    uint32_t Cb;
    const int32_t* perm;     // [6][N] (s3d_vm_backward_bins; rows 3-5 are read)
    const int32_t* start;    // [6][n_bounds]
    uint32_t n_bounds;
    const int32_t* n_valid;
    float* found_inf;
};

// MODE 0: sigma_feat (grad [N]); 1: the products (grad [N][R]); 2: the products behind basis_mat (grad_out fp16 [N][32])
template <int MODE>
__global__ void __launch_bounds__(kCpBwdThreads) k_cp_backward(const float* __restrict__ x, uint32_t N, CpLines f, CpBackward b) {
    __shared__ float tile[kCpGroups][kCpCells * kCpLanes];
    const uint32_t i = blockIdx.z, lane = threadIdx.x % kCpLanes, grp = threadIdx.x / kCpLanes;
    const uint32_t r = blockIdx.y * kCpLanes + lane, R = f.R, D = f.D[i];
    const bool rv = r < R;
    // this workgroup's (chunk, segment): the chunks' segment counts walked in order (at most 32 chunks)
    const int32_t* st = b.start + (size_t)(3 + i) * b.n_bounds;
    const uint32_t nchunks = div_up<uint32_t>(D, kCpChunk);
    uint32_t blk = blockIdx.x, chunk = 0, beg = 0, end = 0;
    bool found = false;
    for (; chunk < nchunks; chunk++) {
        const uint32_t s0 = (uint32_t)st[chunk], s1 = (uint32_t)st[chunk + 1];
        const uint32_t ns = s1 > s0 ? div_up<uint32_t>(s1 - s0, kCpPts) : 0u;
        if (blk < ns) {
            beg = s0 + blk * kCpPts;
            end = beg + kCpPts < s1 ? beg + kCpPts : s1;
            found = true;
            break;
        }
        blk -= ns;
    }
    if (!found || end > N) return;  // (uniform over the workgroup)
    float* my = tile[grp];
    for (uint32_t c = 0; c < kCpCells; c++) my[c * kCpLanes + lane] = 0.0f;  // (a lane's own column, like every add below)
    float wcol[MODE == 2 ? kCpBasisPad : 1], dw[MODE == 2 ? kCpBasisPad : 1];
    if constexpr (MODE == 2) {
#pragma unroll
        for (uint32_t c = 0; c < kCpBasisPad; c++) {
            wcol[c] = (c < b.Cb && rv) ? (float)b.basis[(size_t)c * R + r] : 0.0f;
            dw[c] = 0.0f;
        }
    }
    const int32_t* perm = b.perm + (size_t)(3 + i) * N;
    // Software pipeline over the three dependent loads of a point (id -> coordinates -> line values and gradient): the id is
    // read three trips ahead, the coordinates two, and the six taps and the gradient of the NEXT point are requested before
    // the current point's values are used, so a trip waits for loads that were issued one trip earlier.
    typedef _Float16 half8v __attribute__((ext_vector_type(8)));
    // (plain scalars: with arrays in it the stage was kept in scratch memory)
    struct Fetch {
        float w00, w01, w10, w11, w20, w21;  // tap weights of lines 0 .. 2
        float v00, v01, v10, v11, v20, v21;  // tap values
        float g;
        half8v gh0, gh1, gh2, gh3;
        int c;
        uint32_t flags;                      // bit 2a: tap 0 of line a in range, bit 2a + 1: tap 1; bit 6: live
    };
    auto fetch = [&](uint32_t n, const float* xc, bool in_range) {
        Fetch q;
        bool live = in_range && n < N && rv;
        const CpTap t0 = cp_locate(xc[2], f.D[0]), t1 = cp_locate(xc[1], f.D[1]), t2 = cp_locate(xc[0], f.D[2]);
        const CpTap ti = i == 0 ? t0 : i == 1 ? t1 : t2;
        q.c = ti.i0 - (int)(chunk * kCpChunk);  // first tap inside the chunk's window: -1 .. 63
        // (bins that do not belong to these points: nothing is written outside the window)
        if (q.c < -1 || q.c >= (int)kCpChunk || (q.c < 0 && ti.b0)) live = false;
        auto tap = [&](uint32_t a, const CpTap& t, int k) {
            const bool ok = live && (k ? t.b1 : t.b0);
            if (!ok) return 0.0f;
            return f.line_t[a] ? f.line_t[a][(size_t)(t.i0 + k) * R + r] : f.line[a][(size_t)r * f.D[a] + (t.i0 + k)];
        };
        q.v00 = tap(0, t0, 0); q.v01 = tap(0, t0, 1);
        q.v10 = tap(1, t1, 0); q.v11 = tap(1, t1, 1);
        q.v20 = tap(2, t2, 0); q.v21 = tap(2, t2, 1);
        q.w00 = t0.w0; q.w01 = t0.w1; q.w10 = t1.w0; q.w11 = t1.w1; q.w20 = t2.w0; q.w21 = t2.w1;
        q.flags = (t0.b0 ? 1u : 0u) | (t0.b1 ? 2u : 0u) | (t1.b0 ? 4u : 0u) | (t1.b1 ? 8u : 0u) | (t2.b0 ? 16u : 0u) | (t2.b1 ? 32u : 0u) |
                  (live ? 64u : 0u);
        q.g = 0.0f;
        if constexpr (MODE == 2) {
            const half8v* gp = reinterpret_cast<const half8v*>(b.g_out + (size_t)(live ? n : 0u) * kCpBasisPad);
            q.gh0 = gp[0]; q.gh1 = gp[1]; q.gh2 = gp[2]; q.gh3 = gp[3];
        } else if (live) {
            q.g = MODE == 0 ? b.g[n] : b.g[(size_t)n * R + r];
        }
        return q;
    };
    auto at = [&](uint32_t p) { return p < end ? (uint32_t)perm[p] : 0u; };
    auto coords = [&](uint32_t n, float* o) {
#pragma unroll
        for (uint32_t a = 0; a < 3; a++) o[a] = x[(size_t)(n < N ? n : 0u) * 3 + a];
    };
    uint32_t pos = beg + grp;
    float xa[3], xb[3];
    coords(at(pos), xa);
    Fetch nxt = fetch(at(pos), xa, pos < end);
    uint32_t n1 = at(pos + kCpGroups), n2 = at(pos + 2 * kCpGroups);
    coords(n1, xb);
    for (; pos < end; pos += kCpGroups) {
        const Fetch q = nxt;
        nxt = fetch(n1, xb, pos + kCpGroups < end);
        n1 = n2;
        n2 = at(pos + 3 * kCpGroups);
        coords(n1, xb);
        if (!(q.flags & 64u)) continue;
        float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
        if (q.flags & 1u) l0 += q.v00 * q.w00;
        if (q.flags & 2u) l0 += q.v01 * q.w01;
        if (q.flags & 4u) l1 += q.v10 * q.w10;
        if (q.flags & 8u) l1 += q.v11 * q.w11;
        if (q.flags & 16u) l2 += q.v20 * q.w20;
        if (q.flags & 32u) l2 += q.v21 * q.w21;
        const uint32_t fi = q.flags >> (2u * i);
        const bool ib0 = fi & 1u, ib1 = fi & 2u;
        const float iw0 = i == 0 ? q.w00 : i == 1 ? q.w10 : q.w20, iw1 = i == 0 ? q.w01 : i == 1 ? q.w11 : q.w21;
        const int c = q.c;
        float g = q.g;
        float go[MODE == 2 ? kCpBasisPad : 1];
        if constexpr (MODE == 2) {
            const half8v gh[4] = {q.gh0, q.gh1, q.gh2, q.gh3};
#pragma unroll
            for (uint32_t k = 0; k < kCpBasisPad / 8; k++) {
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    go[8 * k + j] = (float)gh[k][j];  // (columns behind Cb are the caller's zero padding)
                    g = __builtin_fmaf(go[8 * k + j], wcol[8 * k + j], g);
                }
            }
        }
        // autograd of (l0 * l1) * l2
        const float g01 = g * l2;
        const float gl = i == 2 ? g * (l0 * l1) : g01 * (i == 0 ? l1 : l0);
        if (ib0) my[c * (int)kCpLanes + (int)lane] += gl * iw0;
        if (ib1) my[(c + 1) * (int)kCpLanes + (int)lane] += gl * iw1;
        if constexpr (MODE == 2) {
            if (i == 0) {  // (every contributing point is in exactly one chunk of line 0: basis_mat's gradient once)
                const float prod = (float)(_Float16)((l0 * l1) * l2);
#pragma unroll
                for (uint32_t c2 = 0; c2 < kCpBasisPad; c2++) dw[c2] = __builtin_fmaf(go[c2], prod, dw[c2]);
            }
        }
    }
    __syncthreads();
    // the four private tiles in a fixed order, one global atomic per cell and workgroup (cell 64 is the next chunk's cell 0;
    // other segments of the same chunk add to the same cells)
    for (uint32_t c = grp; c < kCpCells; c += kCpGroups) {
        float v = tile[0][c * kCpLanes + lane];
#pragma unroll
        for (uint32_t q = 1; q < kCpGroups; q++) v += tile[q][c * kCpLanes + lane];
        const uint32_t d = chunk * kCpChunk + c;
        if (rv && d < D && v != 0.0f) atomicAdd(&b.d_line[i][(size_t)r * D + d], v);
    }
    if constexpr (MODE == 2) {
        if (i == 0) {
            __syncthreads();
#pragma unroll
            for (uint32_t c = 0; c < kCpBasisPad; c++) my[c * kCpLanes + lane] = dw[c];
            __syncthreads();
            for (uint32_t c = grp; c < b.Cb; c += kCpGroups) {
                float v = tile[0][c * kCpLanes + lane];
#pragma unroll
                for (uint32_t q = 1; q < kCpGroups; q++) v += tile[q][c * kCpLanes + lane];
                if (rv && v != 0.0f) atomicAdd(&b.d_basis[(size_t)c * R + r], v);
            }
        }
    }
}

// The points the sort put behind every bin (both taps of some line out of range) reach no cell, and torch's backward would
// still carry a non-finite gradient of theirs into the other lines (0 * inf): such a gradient poisons line 0 here and raises
// found_inf.  Rows behind the device-side count are absent and not read.
template <int MODE>
__global__ void __launch_bounds__(256) k_cp_check_skipped(uint32_t N, uint32_t R, CpBackward b) {
    const uint32_t s0 = (uint32_t)b.start[(size_t)3 * b.n_bounds + b.n_bounds - 1];
    const uint32_t valid = valid_rows(N, b.n_valid);
    bool bad = false;
    for (uint64_t pos = (uint64_t)s0 + blockIdx.x * 256 + threadIdx.x; pos < N; pos += (uint64_t)gridDim.x * 256) {
        const uint32_t n = (uint32_t)b.perm[(size_t)3 * N + pos];
        if (n >= valid) continue;
        if (MODE == 0) bad = bad || !isfinite(b.g[n]);
        else if (MODE == 1) for (uint32_t r = 0; r < R; r++) bad = bad || !isfinite(b.g[(size_t)n * R + r]);
        else for (uint32_t c = 0; c < kCpBasisPad; c++) bad = bad || !isfinite((float)b.g_out[(size_t)n * kCpBasisPad + c]);
    }
    if (bad) {
        atomicAdd(&b.d_line[0][0], NAN);
        if (b.found_inf) *b.found_inf = 1.0f;
    }
}

}  // namespace
}  // namespace s3d

using namespace s3d;

static int cp_fill(CpLines& f, const char* who, const float* const* lines, const uint32_t* rank, const uint32_t* resolution,
                   const float* const* lines_t) {
    static const uint32_t vec_ids[3] = {2, 1, 0};  // tensoRF/network_cp.py:35
    S3D_REQUIRE(lines && rank && resolution, "%s: null pointer", who);
    S3D_REQUIRE(rank[0] == rank[1] && rank[1] == rank[2] && rank[0] > 0,
                "%s: the three line ranks must be equal and positive (%u, %u, %u): their product runs over one rank index", who, rank[0],
                rank[1], rank[2]);
    f.R = rank[0];
    bool shadows = lines_t != nullptr;
    uintptr_t align = 0;
    for (uint32_t i = 0; i < 3; i++) {
        S3D_REQUIRE(lines[i] && resolution[i] > 0, "%s: empty line %u", who, i);
        S3D_REQUIRE((uint64_t)f.R * resolution[vec_ids[i]] < (1ull << 31), "%s: line %u too large", who, i);
        f.line[i] = lines[i];
        f.D[i] = resolution[vec_ids[i]];
        shadows = shadows && lines_t[i];
        if (shadows) align |= reinterpret_cast<uintptr_t>(lines_t[i]);
    }
    for (uint32_t i = 0; i < 3; i++) f.line_t[i] = shadows ? lines_t[i] : nullptr;
    f.vec4 = (shadows && f.R % 4 == 0 && (align & 15u) == 0) ? 1u : 0u;
    return S3D_OK;
}

S3D_EXPORT int s3d_cp_transpose_lines(const float* const* lines, const uint32_t* rank, const uint32_t* resolution, float* const* lines_t,
                                      s3d_stream_t stream) {
    S3D_REQUIRE(lines_t && lines_t[0] && lines_t[1] && lines_t[2], "cp_transpose_lines: null output");
    CpLines f;
    if (int rc = cp_fill(f, "cp_transpose_lines", lines, rank, resolution, nullptr)) return rc;
    const uint32_t dmax = std::max(f.D[0], std::max(f.D[1], f.D[2]));
    hipLaunchKernelGGL(k_cp_transpose_lines, dim3(div_up<uint32_t>(dmax * f.R, 256), 3), dim3(256), 0, as_stream(stream), f, lines_t[0],
                       lines_t[1], lines_t[2]);
    return check_launch("cp_transpose_lines");
}

S3D_EXPORT int s3d_cp_features_forward(const float* x, uint32_t N, const float* const* lines, const uint32_t* rank,
                                       const uint32_t* resolution, int reduce, float* out, const float* const* lines_t,
                                       const int32_t* n_valid, s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(x && out, "cp_features_forward: null pointer");
    CpLines f;
    if (int rc = cp_fill(f, "cp_features_forward", lines, rank, resolution, lines_t)) return rc;
    const dim3 grid(div_up<uint32_t>(N, 256)), block(256);
    if (reduce) hipLaunchKernelGGL((k_cp_features<true>), grid, block, 0, as_stream(stream), x, N, f, out, n_valid);
    else hipLaunchKernelGGL((k_cp_features<false>), grid, block, 0, as_stream(stream), x, N, f, out, n_valid);
    return check_launch("cp_features_forward");
}

S3D_EXPORT int s3d_cp_color_forward(const float* x, uint32_t N, const float* const* lines, const uint32_t* rank,
                                    const uint32_t* resolution, const uint16_t* basis, uint32_t basis_rows, uint16_t* out,
                                    const float* const* lines_t, const int32_t* n_valid, s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(x && basis && out, "cp_color_forward: null pointer");
    CpLines f;
    if (int rc = cp_fill(f, "cp_color_forward", lines, rank, resolution, lines_t)) return rc;
    S3D_REQUIRE(basis_rows >= 1 && basis_rows <= kCpBasisPad, "cp_color_forward: basis_mat with %u outputs (1 .. %u supported)", basis_rows,
                kCpBasisPad);
    S3D_REQUIRE((size_t)f.R * kCpBasisPad * sizeof(float) <= 64 * 1024, "cp_color_forward: rank %u does not fit the LDS table", f.R);
    hipLaunchKernelGGL(k_cp_color_basis, dim3(div_up<uint32_t>(N, 256)), dim3(256), f.R * kCpBasisPad * sizeof(float), as_stream(stream), x,
                       N, f, (const _Float16*)basis, basis_rows, (_Float16*)out, n_valid);
    return check_launch("cp_color_forward");
}

namespace {
struct CpBwdCall {
    const char* who;
    int mode;
    const float* x;
    uint32_t N;
    const float* const* lines;
    const uint32_t* rank;
    const uint32_t* resolution;
    const int32_t* perm;
    const int32_t* start;
    uint32_t n_bounds;
    float* const* grad_lines;
    const float* const* lines_t;
    const int32_t* n_valid;
    float* found_inf;
    hipStream_t st;
};
}  // namespace

static int cp_backward(const CpBwdCall& c, CpBackward& b) {
    S3D_REQUIRE(c.x && c.perm && c.start && c.grad_lines && c.grad_lines[0] && c.grad_lines[1] && c.grad_lines[2], "%s: null pointer", c.who);
    CpLines f;
    if (int rc = cp_fill(f, c.who, c.lines, c.rank, c.resolution, c.lines_t)) return rc;
    uint32_t nchunks = 0;
    for (uint32_t i = 0; i < 3; i++) nchunks = std::max(nchunks, div_up<uint32_t>(f.D[i], kCpChunk));
    S3D_REQUIRE(c.n_bounds >= nchunks + 2, "%s: n_bounds %u below the %u line chunks + 2", c.who, c.n_bounds, nchunks);
    S3D_REQUIRE((uint64_t)6 * c.N < (1ull << 31), "%s: batch too large", c.who);
    for (uint32_t i = 0; i < 3; i++) b.d_line[i] = c.grad_lines[i];
    b.perm = c.perm; b.start = c.start; b.n_bounds = c.n_bounds; b.n_valid = c.n_valid; b.found_inf = c.found_inf;
    // a chunk's points are cut into segments of kCpPts: at most N / kCpPts + one partial segment per chunk
    const dim3 grid(div_up<uint32_t>(c.N, kCpPts) + nchunks, div_up<uint32_t>(f.R, kCpLanes), 3), block(kCpBwdThreads);
    const dim3 cgrid(std::min<uint32_t>(div_up<uint32_t>(c.N, 256), 64u));
    if (c.mode == 0) {
        hipLaunchKernelGGL((k_cp_backward<0>), grid, block, 0, c.st, c.x, c.N, f, b);
        hipLaunchKernelGGL((k_cp_check_skipped<0>), cgrid, dim3(256), 0, c.st, c.N, f.R, b);
    } else if (c.mode == 1) {
        hipLaunchKernelGGL((k_cp_backward<1>), grid, block, 0, c.st, c.x, c.N, f, b);
        hipLaunchKernelGGL((k_cp_check_skipped<1>), cgrid, dim3(256), 0, c.st, c.N, f.R, b);
    } else {
        hipLaunchKernelGGL((k_cp_backward<2>), grid, block, 0, c.st, c.x, c.N, f, b);
        hipLaunchKernelGGL((k_cp_check_skipped<2>), cgrid, dim3(256), 0, c.st, c.N, f.R, b);
    }
    return check_launch(c.who);
}

S3D_EXPORT int s3d_cp_features_backward(const float* x, uint32_t N, const float* const* lines, const uint32_t* rank,
                                        const uint32_t* resolution, int reduce, const float* grad, const int32_t* perm,
                                        const int32_t* start, uint32_t n_bounds, float* const* grad_lines, float* found_inf,
                                        const float* const* lines_t, const int32_t* n_valid, s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(grad, "cp_features_backward: null pointer");
    CpBackward b;
    memset(&b, 0, sizeof(b));
    b.g = grad;
    const CpBwdCall c{"cp_features_backward", reduce ? 0 : 1, x, N, lines, rank, resolution, perm, start, n_bounds, grad_lines, lines_t,
                      n_valid, found_inf, as_stream(stream)};
    return cp_backward(c, b);
}

S3D_EXPORT int s3d_cp_color_backward(const float* x, uint32_t N, const float* const* lines, const uint32_t* rank,
                                     const uint32_t* resolution, const uint16_t* basis, uint32_t basis_rows, const uint16_t* grad_out,
                                     const int32_t* perm, const int32_t* start, uint32_t n_bounds, float* const* grad_lines,
                                     float* grad_basis, float* found_inf, const float* const* lines_t, const int32_t* n_valid,
                                     s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(basis && grad_out && grad_basis, "cp_color_backward: null pointer");
    S3D_REQUIRE(basis_rows >= 1 && basis_rows <= kCpBasisPad, "cp_color_backward: basis_mat with %u outputs (1 .. %u supported)", basis_rows,
                kCpBasisPad);
    S3D_REQUIRE((reinterpret_cast<uintptr_t>(grad_out) & 15u) == 0, "cp_color_backward: grad_out must be 16-byte aligned");
    CpBackward b;
    memset(&b, 0, sizeof(b));
    b.g_out = (const _Float16*)grad_out;
    b.basis = (const _Float16*)basis;
    b.d_basis = grad_basis;
    b.Cb = basis_rows;
    const CpBwdCall c{"cp_color_backward", 2, x, N, lines, rank, resolution, perm, start, n_bounds, grad_lines, lines_t, n_valid, found_inf,
                      as_stream(stream)};
    return cp_backward(c, b);
}
