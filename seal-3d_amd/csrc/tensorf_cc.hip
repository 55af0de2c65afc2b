// tensorf_cc.hip — CCNeRF (rank-residual TensoRF) features: groups of vector components (three lines, one rank index) and
// matrix components (three planes, one rank index) with a matrix S per component, summed level by level
// (tensoRF/network_cc.py:128-250 of the reference: compute_features_density / compute_features, and the SH contraction of
// forward, :287-291).  The arithmetic contract is written out in include/seal3d_hip.h.
//
// Sampling is align_corners = FALSE, unlike the vector-matrix and CP backbones: p = ((u + 1) * D - 1) / 2.
//
// Forward: one lane per point.  A group's S matrices sit in LDS as [rank][rows] (every lane reads the same row: broadcast), the
// rank loop runs inside the lane, the level's rows (1, or 3 * degree^2 <= 48) stay in registers and are contracted with the SH
// basis of the point's direction before anything is written: out [K_out, N] or [K_out, N, 3].
// Backward: one lane per point, 128 points per workgroup, the groups walked from the last to the first so that the suffix sum of
// the level gradients is one running value.  Per rank the lane recomputes the factors' values, forms the product's gradient
// from S (LDS) and the group's row gradients (registers) and adds the line / plane gradients with global fp32 atomics, one per
// run of adjacent lanes that share the cell (cc_run below).  The S
// gradient is a [rows x 128 points] x [128 points x 16 ranks] product per chunk of 16 ranks: row gradients and products are
// parked in LDS, each lane sums one rank and rows / 8 rows over the workgroup's points, one atomic per entry and workgroup.
#include "s3d_common.hpp"
#include "sh_eval.hpp"
#include <algorithm>

namespace s3d {
namespace {

constexpr uint32_t kCcMaxGroups = 8;
constexpr uint32_t kCcTable = 7168;      // floats of a group's S matrices in LDS: (rank_vec + rank_mat) * rows
constexpr uint32_t kCcFwdThreads = 256;
constexpr uint32_t kCcBwdThreads = 128;  // points per workgroup of the backward
constexpr uint32_t kCcChunk = 16;        // ranks per pass of the S gradient

struct CcGroup {
    const float* line[3];
    const float* plane[3];
    const float* s_vec;
    const float* s_mat;
    uint32_t rv, rm;
};

struct CcModel {
    CcGroup g[kCcMaxGroups];
    uint32_t K;
    uint32_t res[3];
};

struct CcGrad {
    float* line[3];
    float* plane[3];
    float* s_vec;
    float* s_mat;
};

struct CcGrads {
    CcGrad g[kCcMaxGroups];
    float* poison;  // the first S gradient: where a non-finite gradient of a point outside every factor is made visible
};

struct CcTap {
    float w0, w1;
    int i0;
    bool b0, b1;
};

__device__ __forceinline__ CcTap cc_locate(float u, uint32_t D, bool live) {
    CcTap t;
    const float p = ((u + 1.0f) * (float)D - 1.0f) / 2.0f, fl = floorf(p);
    t.w1 = p - fl;
    t.w0 = (fl + 1.0f) - p;
    const bool ok = live && fabsf(p) < 1e9f;  // (non-finite coordinates, absent rows: both taps out of range)
    t.i0 = ok ? (int)fl : -2;
    t.b0 = t.i0 >= 0 && t.i0 < (int)D;
    t.b1 = t.i0 + 1 >= 0 && t.i0 + 1 < (int)D;
    return t;
}

// line i runs along axis 2 - i; plane i spans the axes (m0, m1) = (0,1), (0,2), (1,2): m0 along the row, m1 across the rows
__device__ __forceinline__ uint32_t cc_m0(uint32_t i) { return i == 2 ? 1u : 0u; }
__device__ __forceinline__ uint32_t cc_m1(uint32_t i) { return i == 0 ? 1u : 2u; }

__device__ __forceinline__ float cc_line(const float* __restrict__ L, uint32_t D, const CcTap& t, uint32_t r) {
    const float* p = L + (size_t)r * D;
    float v = 0.0f;
    if (t.b0) v += p[t.i0] * t.w0;
    if (t.b1) v += p[t.i0 + 1] * t.w1;
    return v;
}

__device__ __forceinline__ float cc_plane(const float* __restrict__ P, uint32_t W, uint32_t H, const CcTap& tx, const CcTap& ty, uint32_t r) {
    const float* p = P + (size_t)r * W * H;
    float v = 0.0f;
    if (ty.b0 && tx.b0) v += p[(size_t)ty.i0 * W + tx.i0] * (tx.w0 * ty.w0);
    if (ty.b0 && tx.b1) v += p[(size_t)ty.i0 * W + tx.i0 + 1] * (tx.w1 * ty.w0);
    if (ty.b1 && tx.b0) v += p[(size_t)(ty.i0 + 1) * W + tx.i0] * (tx.w0 * ty.w1);
    if (ty.b1 && tx.b1) v += p[(size_t)(ty.i0 + 1) * W + tx.i0 + 1] * (tx.w1 * ty.w1);
    return v;
}

template <bool HALF>
__device__ __forceinline__ float cc_round(float v) { return HALF ? (float)(_Float16)v : v; }

// a group's S matrices [rows][rank] into LDS as [rank_vec + rank_mat][rows] (vector component first), rounded as the contract says
template <uint32_t C, bool HALF, uint32_t THREADS>
__device__ __forceinline__ void cc_stage(const CcGroup& g, float* table) {
    for (uint32_t e = threadIdx.x; e < g.rv * C; e += THREADS) {
        const uint32_t r = e / C, c = e % C;
        table[e] = cc_round<HALF>(g.s_vec[(size_t)c * g.rv + r]);
    }
    for (uint32_t e = threadIdx.x; e < g.rm * C; e += THREADS) {
        const uint32_t r = e / C, c = e % C;
        table[g.rv * C + e] = cc_round<HALF>(g.s_mat[(size_t)c * g.rm + r]);
    }
}

// DEG = 0: the density head (one row, no directions); DEG 1 .. 4: the colour head (3 DEG^2 rows contracted with the SH basis)
template <uint32_t DEG, bool HALF>
__global__ void __launch_bounds__(kCcFwdThreads) k_cc_forward(const float* __restrict__ x, const float* __restrict__ dirs, uint32_t N,
                                                              CcModel m, uint32_t residual, ShNorm Kn, float* __restrict__ out,
                                                              const int32_t* __restrict__ n_valid) {
    constexpr uint32_t C = DEG ? 3 * DEG * DEG : 1, B = DEG ? DEG * DEG : 1;
    extern __shared__ float cc_table[];
    const uint32_t valid = valid_rows(N, n_valid);
    if (blockIdx.x * kCcFwdThreads >= valid) return;  // (uniform over the workgroup)
    const uint32_t n = blockIdx.x * kCcFwdThreads + threadIdx.x;
    const bool live = n < valid;
    const uint32_t nn = live ? n : 0u;
    CcTap t[3];
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) t[a] = cc_locate(x[(size_t)nn * 3 + a], m.res[a], live);
    float sh[B];
    sh[0] = 1.0f;
    if constexpr (DEG > 0) {
        float j0[1], j1[1], j2[1];
        sh_eval<(DEG ? DEG : 1), false>(dirs[(size_t)nn * 3], dirs[(size_t)nn * 3 + 1], dirs[(size_t)nn * 3 + 2], Kn, sh, j0, j1, j2);
    }
    float last[C];
#pragma unroll
    for (uint32_t c = 0; c < C; c++) last[c] = 0.0f;
    for (uint32_t gi = 0; gi < m.K; gi++) {
        const CcGroup& g = m.g[gi];
        __syncthreads();
        cc_stage<C, HALF, kCcFwdThreads>(g, cc_table);
        __syncthreads();
        float cur[C], tmp[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) cur[c] = 0.0f;
        if (g.rv) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) tmp[c] = 0.0f;
            for (uint32_t r = 0; r < g.rv; r++) {
                float f = (cc_line(g.line[0], m.res[2], t[2], r) * cc_line(g.line[1], m.res[1], t[1], r)) * cc_line(g.line[2], m.res[0], t[0], r);
                f = cc_round<HALF>(f);
                const float* srow = cc_table + (size_t)r * C;
#pragma unroll
                for (uint32_t c = 0; c < C; c++) tmp[c] = __builtin_fmaf(srow[c], f, tmp[c]);
            }
#pragma unroll
            for (uint32_t c = 0; c < C; c++) cur[c] = cc_round<HALF>(tmp[c]);
        }
        if (g.rm) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) tmp[c] = 0.0f;
            for (uint32_t r = 0; r < g.rm; r++) {
                float f = 1.0f;
#pragma unroll
                for (uint32_t i = 0; i < 3; i++) {
                    const uint32_t a0 = cc_m0(i), a1 = cc_m1(i);
                    const float p = cc_plane(g.plane[i], m.res[a0], m.res[a1], t[a0], t[a1], r);
                    f = i == 0 ? p : f * p;
                }
                f = cc_round<HALF>(f);
                const float* srow = cc_table + (size_t)(g.rv + r) * C;
#pragma unroll
                for (uint32_t c = 0; c < C; c++) tmp[c] = __builtin_fmaf(srow[c], f, tmp[c]);
            }
#pragma unroll
            for (uint32_t c = 0; c < C; c++) cur[c] = g.rv ? cc_round<HALF>(cur[c] + cc_round<HALF>(tmp[c])) : cc_round<HALF>(tmp[c]);
        }
        if (gi > 0) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) cur[c] = cc_round<HALF>(cur[c] + last[c]);
        }
#pragma unroll
        for (uint32_t c = 0; c < C; c++) last[c] = cur[c];
        if (live && (residual || gi + 1 == m.K)) {
            const size_t row = (size_t)(residual ? gi : 0u) * N + n;
            if constexpr (DEG == 0) {
                out[row] = cur[0];
            } else {
#pragma unroll
                for (uint32_t ch = 0; ch < 3; ch++) {
                    float v = 0.0f;
#pragma unroll
                    for (uint32_t j = 0; j < B; j++) v += cur[ch * B + j] * sh[j];
                    out[row * 3 + ch] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ backward (parameter gradients)
// Consecutive samples of a ray fall into the same cell of a line (and often of a plane), and a wave holds 64 consecutive points:
// the lanes of a RUN — adjacent lanes with equal cell indices — are summed across the wave and the run's last lane issues the
// atomic.  The run structure depends on the cells only, so it is worked out once per factor and reused for every rank:
// bit s of `take` says "add the partial sum of lane - 2^s" in step s of a segmented inclusive scan, bit 6 marks the run's last lane.
__device__ __forceinline__ uint32_t cc_run(int k0, int k1) {
    const uint32_t lane = threadIdx.x & 63u;
    // (every shuffle by all lanes, outside the short-circuit operators: a lane that is masked off is read as zero)
    const int p0 = __shfl_up(k0, 1), p1 = __shfl_up(k1, 1), n0 = __shfl_down(k0, 1), n1 = __shfl_down(k1, 1);
    bool f = lane == 0 || p0 != k0 || p1 != k1;  // head of a run
    const bool tail = lane == 63 || n0 != k0 || n1 != k1;
    uint32_t take = tail ? 64u : 0u;
#pragma unroll
    for (uint32_t s = 0; s < 6; s++) {
        const bool fu = __shfl_up((int)f, 1u << s) != 0;
        if (!f) take |= 1u << s;  // (f is set on every lane below 2^s: lane 0 is a head)
        f = f || (lane >= (1u << s) && fu);
    }
    return take;
}

__device__ __forceinline__ float cc_run_sum(float v, uint32_t take) {
#pragma unroll
    for (uint32_t s = 0; s < 6; s++) {
        const float u = __shfl_up(v, 1u << s);
        if (take & (1u << s)) v += u;
    }
    return v;
}

template <uint32_t DEG, bool HALF>
__global__ void __launch_bounds__(kCcBwdThreads) k_cc_backward(const float* __restrict__ x, const float* __restrict__ dirs, uint32_t N,
                                                               CcModel m, CcGrads d, uint32_t residual, ShNorm Kn,
                                                               const float* __restrict__ grad, const int32_t* __restrict__ n_valid,
                                                               float* __restrict__ found_inf) {
    constexpr uint32_t C = DEG ? 3 * DEG * DEG : 1, B = DEG ? DEG * DEG : 1, CH = DEG ? 3 : 1;
    constexpr uint32_t CT = (C + 7) / 8;  // rows per lane of the S gradient: 8 row groups x 16 ranks = 128 lanes
    extern __shared__ float cc_table[];
    __shared__ float s_dy[kCcBwdThreads][C + 1];
    __shared__ float s_f[kCcBwdThreads][kCcChunk + 1];
    const uint32_t valid = valid_rows(N, n_valid);
    if (blockIdx.x * kCcBwdThreads >= valid) return;  // (uniform over the workgroup)
    const uint32_t tid = threadIdx.x, n = blockIdx.x * kCcBwdThreads + tid;
    const bool live = n < valid;
    const uint32_t nn = live ? n : 0u;
    CcTap t[3];
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) t[a] = cc_locate(x[(size_t)nn * 3 + a], m.res[a], live);
    float sh[B];
    sh[0] = 1.0f;
    if constexpr (DEG > 0) {
        float j0[1], j1[1], j2[1];
        sh_eval<(DEG ? DEG : 1), false>(dirs[(size_t)nn * 3], dirs[(size_t)nn * 3 + 1], dirs[(size_t)nn * 3 + 2], Kn, sh, j0, j1, j2);
    }
    uint32_t lrun[3], prun[3];  // the runs of equal cells across the wave: per axis (lines) and per plane
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) lrun[a] = cc_run(t[a].i0, 0);
#pragma unroll
    for (uint32_t i = 0; i < 3; i++) prun[i] = cc_run(t[cc_m0(i)].i0, t[cc_m1(i)].i0);
    float run[CH];  // the suffix sum of the level gradients: group g receives every level >= g
#pragma unroll
    for (uint32_t ch = 0; ch < CH; ch++) run[ch] = (live && !residual) ? grad[(size_t)n * CH + ch] : 0.0f;
    bool bad = false;
#pragma unroll
    for (uint32_t ch = 0; ch < CH; ch++) bad = bad || !isfinite(run[ch]);
    const uint32_t gj = tid % kCcChunk, gc = tid / kCcChunk;  // this lane's rank and row group in the S gradient
    for (uint32_t gi = m.K; gi-- > 0;) {
        const CcGroup& g = m.g[gi];
        const CcGrad& dg = d.g[gi];
        if (live && residual) {
#pragma unroll
            for (uint32_t ch = 0; ch < CH; ch++) {
                const float v = grad[((size_t)gi * N + n) * CH + ch];
                bad = bad || !isfinite(v);
                run[ch] += v;
            }
        }
        __syncthreads();  // (the previous group's table and row gradients have been read)
        cc_stage<C, HALF, kCcBwdThreads>(g, cc_table);
        float dy[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            dy[c] = live ? cc_round<HALF>(run[c / B] * sh[c % B]) : 0.0f;
            s_dy[tid][c] = dy[c];
        }
        __syncthreads();
        for (uint32_t comp = 0; comp < 2; comp++) {
            const uint32_t R = comp ? g.rm : g.rv, base = comp ? g.rv : 0u;
            float* dS = comp ? dg.s_mat : dg.s_vec;
            for (uint32_t r0 = 0; r0 < R; r0 += kCcChunk) {
                for (uint32_t j = 0; j < kCcChunk; j++) {
                    const uint32_t r = r0 + j;
                    float f = 0.0f;
                    if (r < R) {  // (uniform; an absent row has zero row gradients and no tap in range: it adds nothing)
                        const float* srow = cc_table + (size_t)(base + r) * C;
                        float df = 0.0f;
#pragma unroll
                        for (uint32_t c = 0; c < C; c++) df = __builtin_fmaf(srow[c], dy[c], df);
                        df = cc_round<HALF>(df);
                        float v[3];
                        if (comp == 0) {
#pragma unroll
                            for (uint32_t i = 0; i < 3; i++) v[i] = cc_line(g.line[i], m.res[2 - i], t[2 - i], r);
                        } else {
#pragma unroll
                            for (uint32_t i = 0; i < 3; i++)
                                v[i] = cc_plane(g.plane[i], m.res[cc_m0(i)], m.res[cc_m1(i)], t[cc_m0(i)], t[cc_m1(i)], r);
                        }
                        f = (v[0] * v[1]) * v[2];
                        // autograd of (v0 * v1) * v2
                        const float g01 = df * v[2];
                        const float dv[3] = {g01 * v[1], g01 * v[0], df * (v[0] * v[1])};
                        if (comp == 0) {
#pragma unroll
                            for (uint32_t i = 0; i < 3; i++) {
                                const CcTap& ta = t[2 - i];
                                const uint32_t rn = lrun[2 - i];
                                float* dl = dg.line[i] + (size_t)r * m.res[2 - i];
                                const float a0 = cc_run_sum(dv[i] * ta.w0, rn), a1 = cc_run_sum(dv[i] * ta.w1, rn);
                                if (rn & 64u) {  // (the lanes of a run share the cell, hence b0 / b1)
                                    if (ta.b0) atomicAdd(dl + ta.i0, a0);
                                    if (ta.b1) atomicAdd(dl + ta.i0 + 1, a1);
                                }
                            }
                        } else {
#pragma unroll
                            for (uint32_t i = 0; i < 3; i++) {
                                const CcTap& tx = t[cc_m0(i)];
                                const CcTap& ty = t[cc_m1(i)];
                                const uint32_t W = m.res[cc_m0(i)], H = m.res[cc_m1(i)];
                                float* dp = dg.plane[i] + (size_t)r * W * H;
                                const uint32_t rn = prun[i];
                                const float a00 = cc_run_sum(dv[i] * (tx.w0 * ty.w0), rn), a01 = cc_run_sum(dv[i] * (tx.w1 * ty.w0), rn);
                                const float a10 = cc_run_sum(dv[i] * (tx.w0 * ty.w1), rn), a11 = cc_run_sum(dv[i] * (tx.w1 * ty.w1), rn);
                                if (rn & 64u) {
                                    if (ty.b0 && tx.b0) atomicAdd(dp + (size_t)ty.i0 * W + tx.i0, a00);
                                    if (ty.b0 && tx.b1) atomicAdd(dp + (size_t)ty.i0 * W + tx.i0 + 1, a01);
                                    if (ty.b1 && tx.b0) atomicAdd(dp + (size_t)(ty.i0 + 1) * W + tx.i0, a10);
                                    if (ty.b1 && tx.b1) atomicAdd(dp + (size_t)(ty.i0 + 1) * W + tx.i0 + 1, a11);
                                }
                            }
                        }
                        f = cc_round<HALF>(f);
                    }
                    s_f[tid][j] = f;
                }
                __syncthreads();
                // dS[c][r0 + gj] += sum over the workgroup's points of dy[p][c] * f[p][gj], rows c = gc * CT .. + CT - 1
                float acc[CT];
#pragma unroll
                for (uint32_t q = 0; q < CT; q++) acc[q] = 0.0f;
                for (uint32_t p = 0; p < kCcBwdThreads; p++) {
                    const float fv = s_f[p][gj];
#pragma unroll
                    for (uint32_t q = 0; q < CT; q++) {
                        const uint32_t c = gc * CT + q;
                        if (c < C) acc[q] = __builtin_fmaf(s_dy[p][c], fv, acc[q]);
                    }
                }
                if (r0 + gj < R) {
#pragma unroll
                    for (uint32_t q = 0; q < CT; q++) {
                        const uint32_t c = gc * CT + q;
                        if (c < C && acc[q] != 0.0f) atomicAdd(dS + (size_t)c * R + r0 + gj, acc[q]);
                    }
                }
                __syncthreads();
            }
        }
    }
    if (bad) {
        atomicAdd(d.poison, NAN);
        if (found_inf) *found_inf = 1.0f;
    }
}

}  // namespace
}  // namespace s3d

using namespace s3d;

static int cc_fill(CcModel& m, const char* who, const s3d_cc_group* groups, uint32_t n_groups, const uint32_t* resolution, uint32_t rows) {
    S3D_REQUIRE(groups && resolution, "%s: null pointer", who);
    S3D_REQUIRE(n_groups >= 1 && n_groups <= kCcMaxGroups, "%s: %u groups (1 .. %u supported)", who, n_groups, kCcMaxGroups);
    memset(&m, 0, sizeof(m));
    m.K = n_groups;
    for (uint32_t a = 0; a < 3; a++) {
        S3D_REQUIRE(resolution[a] > 0 && resolution[a] < (1u << 20), "%s: resolution %u along axis %u", who, resolution[a], a);
        m.res[a] = resolution[a];
    }
    for (uint32_t k = 0; k < n_groups; k++) {
        const s3d_cc_group& s = groups[k];
        CcGroup& g = m.g[k];
        g.rv = s.rank_vec;
        g.rm = s.rank_mat;
        S3D_REQUIRE(((uint64_t)g.rv + g.rm) * rows <= kCcTable, "%s: group %u with ranks %u + %u and %u rows does not fit the LDS table (%u floats)",
                    who, k, g.rv, g.rm, rows, kCcTable);
        if (g.rv) {
            S3D_REQUIRE(s.s_vec && s.line[0] && s.line[1] && s.line[2], "%s: group %u: null vector component", who, k);
            g.s_vec = s.s_vec;
            for (uint32_t i = 0; i < 3; i++) {
                S3D_REQUIRE((uint64_t)g.rv * resolution[2 - i] < (1ull << 31), "%s: group %u: line %u too large", who, k, i);
                g.line[i] = s.line[i];
            }
        }
        if (g.rm) {
            S3D_REQUIRE(s.s_mat && s.plane[0] && s.plane[1] && s.plane[2], "%s: group %u: null matrix component", who, k);
            g.s_mat = s.s_mat;
            static const uint32_t m0[3] = {0, 0, 1}, m1[3] = {1, 2, 2};  // tensoRF/network_cc.py:55
            for (uint32_t i = 0; i < 3; i++) {
                S3D_REQUIRE((uint64_t)g.rm * resolution[m0[i]] * resolution[m1[i]] < (1ull << 31), "%s: group %u: plane %u too large", who, k, i);
                g.plane[i] = s.plane[i];
            }
        }
    }
    return S3D_OK;
}

namespace {
struct CcCall {
    const char* who;
    const float* x;
    const float* dirs;
    uint32_t N;
    const s3d_cc_group* groups;
    uint32_t n_groups;
    const uint32_t* resolution;
    uint32_t degree;  // 0: the density head
    int residual, half;
    const int32_t* n_valid;
    hipStream_t st;
};

template <uint32_t DEG>
int cc_launch_forward(const CcCall& c, const CcModel& m, size_t lds, float* out) {
    ShNorm Kn;
    host_sh_norm(DEG, Kn);
    const dim3 grid(div_up<uint32_t>(c.N, kCcFwdThreads)), block(kCcFwdThreads);
    if (c.half) hipLaunchKernelGGL((k_cc_forward<DEG, true>), grid, block, lds, c.st, c.x, c.dirs, c.N, m, (uint32_t)(c.residual != 0), Kn, out, c.n_valid);
    else hipLaunchKernelGGL((k_cc_forward<DEG, false>), grid, block, lds, c.st, c.x, c.dirs, c.N, m, (uint32_t)(c.residual != 0), Kn, out, c.n_valid);
    return check_launch(c.who);
}

template <uint32_t DEG>
int cc_launch_backward(const CcCall& c, const CcModel& m, size_t lds, const CcGrads& d, const float* grad, float* found_inf) {
    ShNorm Kn;
    host_sh_norm(DEG, Kn);
    const dim3 grid(div_up<uint32_t>(c.N, kCcBwdThreads)), block(kCcBwdThreads);
    if (c.half) hipLaunchKernelGGL((k_cc_backward<DEG, true>), grid, block, lds, c.st, c.x, c.dirs, c.N, m, d, (uint32_t)(c.residual != 0), Kn, grad, c.n_valid, found_inf);
    else hipLaunchKernelGGL((k_cc_backward<DEG, false>), grid, block, lds, c.st, c.x, c.dirs, c.N, m, d, (uint32_t)(c.residual != 0), Kn, grad, c.n_valid, found_inf);
    return check_launch(c.who);
}
}  // namespace

static int cc_prepare(const CcCall& c, CcModel& m, size_t& lds) {
    S3D_REQUIRE(c.x, "%s: null pointer", c.who);
    S3D_REQUIRE(c.degree <= 4 && (c.degree == 0) == (c.dirs == nullptr), "%s: degree %u (colour: 1 .. 4 with directions)", c.who, c.degree);
    S3D_REQUIRE((uint64_t)c.N * kCcMaxGroups * 3 < (1ull << 32), "%s: batch too large", c.who);
    const uint32_t rows = c.degree ? 3 * c.degree * c.degree : 1;
    if (int rc = cc_fill(m, c.who, c.groups, c.n_groups, c.resolution, rows)) return rc;
    uint32_t need = 1;
    for (uint32_t k = 0; k < m.K; k++) need = std::max(need, (m.g[k].rv + m.g[k].rm) * rows);
    lds = (size_t)need * sizeof(float);
    return S3D_OK;
}

static int cc_forward(const CcCall& c, float* out) {
    if (c.N == 0) return S3D_OK;
    S3D_REQUIRE(out, "%s: null output", c.who);
    CcModel m;
    size_t lds = 0;
    if (int rc = cc_prepare(c, m, lds)) return rc;
    switch (c.degree) {
        case 0: return cc_launch_forward<0>(c, m, lds, out);
        case 1: return cc_launch_forward<1>(c, m, lds, out);
        case 2: return cc_launch_forward<2>(c, m, lds, out);
        case 3: return cc_launch_forward<3>(c, m, lds, out);
        default: return cc_launch_forward<4>(c, m, lds, out);
    }
}

static int cc_backward(const CcCall& c, const float* grad, const s3d_cc_group_grad* grads, float* found_inf) {
    if (c.N == 0) return S3D_OK;
    S3D_REQUIRE(grad && grads, "%s: null pointer", c.who);
    CcModel m;
    size_t lds = 0;
    if (int rc = cc_prepare(c, m, lds)) return rc;
    CcGrads d;
    memset(&d, 0, sizeof(d));
    for (uint32_t k = 0; k < m.K; k++) {
        const s3d_cc_group_grad& s = grads[k];
        if (m.g[k].rv) {
            S3D_REQUIRE(s.s_vec && s.line[0] && s.line[1] && s.line[2], "%s: group %u: null vector gradient", c.who, k);
            d.g[k].s_vec = s.s_vec;
            for (uint32_t i = 0; i < 3; i++) d.g[k].line[i] = s.line[i];
            if (!d.poison) d.poison = s.s_vec;
        }
        if (m.g[k].rm) {
            S3D_REQUIRE(s.s_mat && s.plane[0] && s.plane[1] && s.plane[2], "%s: group %u: null matrix gradient", c.who, k);
            d.g[k].s_mat = s.s_mat;
            for (uint32_t i = 0; i < 3; i++) d.g[k].plane[i] = s.plane[i];
            if (!d.poison) d.poison = s.s_mat;
        }
    }
    S3D_REQUIRE(d.poison, "%s: no component in any group", c.who);
    switch (c.degree) {
        case 0: return cc_launch_backward<0>(c, m, lds, d, grad, found_inf);
        case 1: return cc_launch_backward<1>(c, m, lds, d, grad, found_inf);
        case 2: return cc_launch_backward<2>(c, m, lds, d, grad, found_inf);
        case 3: return cc_launch_backward<3>(c, m, lds, d, grad, found_inf);
        default: return cc_launch_backward<4>(c, m, lds, d, grad, found_inf);
    }
}

S3D_EXPORT int s3d_cc_features_forward(const float* x, uint32_t N, const s3d_cc_group* groups, uint32_t n_groups, const uint32_t* resolution,
                                       int residual, int half, float* out, const int32_t* n_valid, s3d_stream_t stream) {
    const CcCall c{"cc_features_forward", x, nullptr, N, groups, n_groups, resolution, 0, residual, half, n_valid, as_stream(stream)};
    return cc_forward(c, out);
}

S3D_EXPORT int s3d_cc_color_forward(const float* x, const float* dirs, uint32_t N, const s3d_cc_group* groups, uint32_t n_groups,
                                    const uint32_t* resolution, uint32_t degree, int residual, int half, float* out, const int32_t* n_valid,
                                    s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(dirs && degree >= 1, "cc_color_forward: directions and a degree of 1 .. 4");
    const CcCall c{"cc_color_forward", x, dirs, N, groups, n_groups, resolution, degree, residual, half, n_valid, as_stream(stream)};
    return cc_forward(c, out);
}

S3D_EXPORT int s3d_cc_features_backward(const float* x, uint32_t N, const s3d_cc_group* groups, uint32_t n_groups, const uint32_t* resolution,
                                        int residual, int half, const float* grad, const s3d_cc_group_grad* grads, float* found_inf,
                                        const int32_t* n_valid, s3d_stream_t stream) {
    const CcCall c{"cc_features_backward", x, nullptr, N, groups, n_groups, resolution, 0, residual, half, n_valid, as_stream(stream)};
    return cc_backward(c, grad, grads, found_inf);
}

S3D_EXPORT int s3d_cc_color_backward(const float* x, const float* dirs, uint32_t N, const s3d_cc_group* groups, uint32_t n_groups,
                                     const uint32_t* resolution, uint32_t degree, int residual, int half, const float* grad,
                                     const s3d_cc_group_grad* grads, float* found_inf, const int32_t* n_valid, s3d_stream_t stream) {
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(dirs && degree >= 1, "cc_color_backward: directions and a degree of 1 .. 4");
    const CcCall c{"cc_color_backward", x, dirs, N, groups, n_groups, resolution, degree, residual, half, n_valid, as_stream(stream)};
    return cc_backward(c, grad, grads, found_inf);
}
