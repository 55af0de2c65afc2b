// sdf_pair.hpp — the point-triangle pair test of the SDF backbone and the two walks of the mesh BVH (include/seal3d_hip.h "SDF",
// "SDF: BVH query"; DESIGN.md "SDF"), in plain C++ that compiles for the device and for the host.  This is the only place that
// knows the staging of a triangle, the distance and solid-angle expressions, the tie rule (pair_accumulate) and the sign rule
// (pair_finish): mesh_sdf_kernel (csrc/sdf.hip) runs pair_accumulate over its LDS tiles, csrc/sdf_bvh.hip runs each walk one lane
// per point, and tests/sdf_bvh_host.cpp runs both routes from the same text under the host sanitizers.  The library is built
// without contraction, so one text gives one set of bits wherever it is compiled.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define S3D_HD __host__ __device__ __forceinline__
#else
#define S3D_HD inline
#endif

namespace s3d {
namespace sdfpair {

constexpr uint32_t kBvhLeaf = 4;  // faces per leaf
constexpr float kTiny = 1e-30f;   // |edge|^2 or |normal|^2 below this: the edge is a point / the triangle has no area

// Slack of the distance walk's pruning test.  The contract keeps every coordinate within [-4, 4], so the vectors of a pair test
// are at most 8 sqrt(3) < 14 long and one fp32 rounding of a component is at most 14 * 2^-24 = 8.3e-7.  A pair test is a handful of
// such roundings per component (p - A, t * e, the difference, the sum of three squares; for the plane (p - A).n / |n| the same
// count relative to |p - A|): its computed distance sqrt(d2) is within about 5e-6 of the true one, whatever d2 itself.  A box holds
// its fp32 vertices exactly, so its true distance is a lower bound of every true face distance inside; its computed distance
// (three differences, three squares, a sum) is within about 2e-6 of that, and comparing squares instead of roots adds a relative
// 2^-22 of at most 14, 3e-6.  A face whose computed d2 is <= the final minimum m therefore sits in boxes of computed distance
// <= sqrt(m) + 1e-5 <= sqrt(best) + 1e-5 at every moment of the walk; kBvhSlack is ten times that, so such a face is never
// skipped, at the price of a few more visits (1e-4 is a fiftieth of an edge at 10^6 faces).  The bound takes a face's plane at its
// word: a sliver whose fp32 normal is rounding noise (open items) can report a d2 far below its true distance.
constexpr float kBvhSlack = 1e-4f;

// one staged triangle: what every pair test reads and what depends on the triangle alone (5 x 16 bytes)
struct __attribute__((aligned(16))) StagedTri {
    float ax, ay, az, inv_nn;     // A; 1 / |n|^2, 0 for a triangle without area
    float abx, aby, abz, inv_ab;  // B - A; 1 / |B - A|^2 (0: A == B)
    float acx, acy, acz, inv_ac;  // C - A; 1 / |C - A|^2
    float nx, ny, nz, inv_bc;     // n = (B - A) x (C - A); 1 / |C - B|^2
    float d00, d01, d11, pad;     // ab.ab, ab.ac, ac.ac
};

// one node of the tree (4 x 16 bytes; the layout include/seal3d_hip.h states)
struct __attribute__((aligned(16))) BvhNode {
    float lox, loy, loz, pad0;  // lower corner of the node's vertices, rounded down (+inf: no faces)
    float hix, hiy, hiz, pad1;  // upper corner, rounded up (-inf: no faces)
    float cx, cy, cz, r;        // area-weighted centroid; max |vertex - c|, rounded up (-1: no faces)
    float nx, ny, nz, pad2;     // sum over the faces of (B - A) x (C - A) / 2
};

S3D_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

S3D_HD float clamp01(float x) { return fminf(1.0f, fmaxf(0.0f, x)); }

S3D_HD float seg_dist2(float px, float py, float pz, float ex, float ey, float ez, float pe, float inv_ee) {
    // squared distance of p (relative to the segment's start) to the segment along e; pe = p.e; inv_ee = 0 collapses it to the start
    const float t = clamp01(pe * inv_ee);
    const float vx = px - t * ex, vy = py - t * ey, vz = pz - t * ez;
    return dot3(vx, vy, vz, vx, vy, vz);
}

S3D_HD StagedTri stage_tri(const float* t) {
    StagedTri s;
    s.ax = t[0]; s.ay = t[1]; s.az = t[2];
    s.abx = t[3] - s.ax; s.aby = t[4] - s.ay; s.abz = t[5] - s.az;
    s.acx = t[6] - s.ax; s.acy = t[7] - s.ay; s.acz = t[8] - s.az;
    s.nx = s.aby * s.acz - s.abz * s.acy;
    s.ny = s.abz * s.acx - s.abx * s.acz;
    s.nz = s.abx * s.acy - s.aby * s.acx;
    s.d00 = dot3(s.abx, s.aby, s.abz, s.abx, s.aby, s.abz);
    s.d01 = dot3(s.abx, s.aby, s.abz, s.acx, s.acy, s.acz);
    s.d11 = dot3(s.acx, s.acy, s.acz, s.acx, s.acy, s.acz);
    const float bcx = s.acx - s.abx, bcy = s.acy - s.aby, bcz = s.acz - s.abz;
    const float bb = dot3(bcx, bcy, bcz, bcx, bcy, bcz);
    const float nn = dot3(s.nx, s.ny, s.nz, s.nx, s.ny, s.nz);
    s.inv_ab = s.d00 > kTiny ? 1.0f / s.d00 : 0.0f;
    s.inv_ac = s.d11 > kTiny ? 1.0f / s.d11 : 0.0f;
    s.inv_bc = bb > kTiny ? 1.0f / bb : 0.0f;
    s.inv_nn = nn > kTiny ? 1.0f / nn : 0.0f;
    s.pad = 0.0f;
    return s;
}

// the point as one triangle sees it: what both halves of the pair test start from
struct PairPoint {
    float apx, apy, apz;  // p - A
    float pn;             // (p - A).n
};

S3D_HD PairPoint pair_point(const StagedTri& s, float px, float py, float pz) {
    PairPoint q;
    q.apx = px - s.ax; q.apy = py - s.ay; q.apz = pz - s.az;
    q.pn = dot3(q.apx, q.apy, q.apz, s.nx, s.ny, s.nz);
    return q;
}

// squared distance of the point to the staged triangle
S3D_HD float pair_dist2(const StagedTri& s, const PairPoint& q) {
    const float d20 = dot3(q.apx, q.apy, q.apz, s.abx, s.aby, s.abz);
    const float d21 = dot3(q.apx, q.apy, q.apz, s.acx, s.acy, s.acz);
    // the three edges (their end points are the three vertices)
    float d2 = seg_dist2(q.apx, q.apy, q.apz, s.abx, s.aby, s.abz, d20, s.inv_ab);
    d2 = fminf(d2, seg_dist2(q.apx, q.apy, q.apz, s.acx, s.acy, s.acz, d21, s.inv_ac));
    const float bpx = q.apx - s.abx, bpy = q.apy - s.aby, bpz = q.apz - s.abz;
    const float bcx = s.acx - s.abx, bcy = s.acy - s.aby, bcz = s.acz - s.abz;
    d2 = fminf(d2, seg_dist2(bpx, bpy, bpz, bcx, bcy, bcz, dot3(bpx, bpy, bpz, bcx, bcy, bcz), s.inv_bc));
    // the face: the foot of the perpendicular lies inside iff its two barycentric numerators and their complement are >= 0
    const float v = s.d11 * d20 - s.d01 * d21;
    const float w = s.d00 * d21 - s.d01 * d20;
    const float den = s.d00 * s.d11 - s.d01 * s.d01;
    if (s.inv_nn > 0.0f && v >= 0.0f && w >= 0.0f && v + w <= den) d2 = fminf(d2, q.pn * q.pn * s.inv_nn);
    return d2;
}

// whether the point sees a solid angle at all: not for a triangle without area, not from inside its plane
S3D_HD bool pair_subtends(const StagedTri& s, const PairPoint& q) { return s.inv_nn > 0.0f && q.pn != 0.0f; }

// solid angle of the staged triangle seen from a point that pair_subtends (van Oosterom & Strackee): a, b, c = vertices - point;
// a.(b x c) = a.n = -pn
S3D_HD float pair_omega(const StagedTri& s, const PairPoint& q) {
    const float ax = -q.apx, ay = -q.apy, az = -q.apz;
    const float bx = ax + s.abx, by = ay + s.aby, bz = az + s.abz;
    const float cx = ax + s.acx, cy = ay + s.acy, cz = az + s.acz;
    const float la = sqrtf(dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(dot3(bx, by, bz, bx, by, bz));
    const float lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
    const float denom = la * lb * lc + dot3(ax, ay, az, bx, by, bz) * lc + dot3(bx, by, bz, cx, cy, cz) * la
                        + dot3(cx, cy, cz, ax, ay, az) * lb;
    return 2.0f * atan2f(-q.pn, denom);
}

// the two halves for a walk, which needs one of them per visit (0 where the point sees no solid angle)
S3D_HD float pair_dist2(const StagedTri& s, float px, float py, float pz) { return pair_dist2(s, pair_point(s, px, py, pz)); }

S3D_HD float pair_omega(const StagedTri& s, float px, float py, float pz) {
    const PairPoint q = pair_point(s, px, py, pz);
    return pair_subtends(s, q) ? pair_omega(s, q) : 0.0f;
}

// One step of the brute-force loop over the faces in their order: the running minimum is strict, so among equal d2 the lowest
// face stays; the solid angles add up in face order.
S3D_HD void pair_accumulate(const StagedTri& s, uint32_t face, float px, float py, float pz, float* best_d2, uint32_t* best_face,
                            float* omega) {
    const PairPoint q = pair_point(s, px, py, pz);
    const float d2 = pair_dist2(s, q);
    if (d2 < *best_d2) { *best_d2 = d2; *best_face = face; }
    if (pair_subtends(s, q)) *omega += pair_omega(s, q);
}

// minimum and solid angle over all faces -> sdf (inside where the winding number exceeds 1/2; NaN: a walk reached its iteration
// cap, which the brute-force loop cannot) and winding number
S3D_HD void pair_finish(bool ok, float best_d2, float omega, float* sdf, float* winding) {
    const float wn = omega * 0.07957747154594767f;  // 1 / (4 pi)
    const float dist = sqrtf(best_d2);
    *sdf = ok ? (wn > 0.5f ? -dist : dist) : NAN;
    *winding = wn;
}

// squared distance of p to the node's box (+inf for a node without faces: its corners are inverted)
S3D_HD float box_dist2(const BvhNode& nd, float px, float py, float pz) {
    const float qx = fmaxf(fmaxf(nd.lox - px, 0.0f), px - nd.hix);
    const float qy = fmaxf(fmaxf(nd.loy - py, 0.0f), py - nd.hiy);
    const float qz = fmaxf(fmaxf(nd.loz - pz, 0.0f), pz - nd.hiz);
    return dot3(qx, qy, qz, qx, qy, qz);
}

// Nodes are numbered from 1 in heap order (node j is nodes[j - 1]; children 2j and 2j + 1; the L leaves are j in [L, 2L)), so a
// walk needs no stack: to leave a subtree, climb while the node was the second of its pair, then step to its sibling.  With one
// bit per level of the path, from the lowest upwards, set where the node was visited second, the climb is that word's run of
// trailing ones.  The root's leading one in j counts as "second": a walk that has left every subtree shifts j down to 0.

// Distance walk: exact minimum of pair_dist2 over the faces, the nearer child first, a subtree skipped only where its box is
// farther than sqrt(best) + kBvhSlack.  Returns false when the iteration cap was reached (it never is on a tree of the contract).
S3D_HD bool bvh_nearest(const BvhNode* nodes, const StagedTri* tris, const int32_t* perm, uint32_t F, uint32_t L, float px, float py,
                        float pz, float* best_d2, uint32_t* best_face) {
    float best = 3.402823466e+38f, reach2 = 3.402823466e+38f;
    uint32_t best_id = 0xFFFFFFFFu;
    uint32_t j = 1, trail = 0;  // trail: one bit per level of the path, set where the right child went first
    const uint32_t cap = 2u * (2u * L - 1u);
    float box2 = box_dist2(nodes[0], px, py, pz);  // of node j
    for (uint32_t step = 0; step < cap; step++) {
        if (!(box2 > reach2)) {
            if (j < L) {
                const float left2 = box_dist2(nodes[2 * j - 1], px, py, pz), right2 = box_dist2(nodes[2 * j], px, py, pz);
                const uint32_t right_first = right2 < left2 ? 1u : 0u;
                j = 2 * j + right_first;
                trail = (trail << 1) | right_first;
                box2 = right_first ? right2 : left2;
                continue;
            }
            const uint32_t base = (j - L) * kBvhLeaf;
            for (uint32_t k = 0; k < kBvhLeaf; k++) {
                const uint32_t f = base + k;
                if (f >= F) break;
                const float d2 = pair_dist2(tris[f], px, py, pz);
                if (d2 <= best) {
                    const uint32_t id = (uint32_t)perm[f];
                    if (d2 < best || id < best_id) {  // (among equal d2 the lowest original index, as the brute-force order gives)
                        best = d2;
                        best_id = id;
                        const float reach = sqrtf(best) + kBvhSlack;
                        reach2 = reach * reach;
                    }
                }
            }
        }
        const uint32_t up = (uint32_t)__builtin_ctz(~(j ^ trail));
        j >>= up;
        trail >>= up;
        if (j == 0) {
            *best_d2 = best;
            *best_face = best_id == 0xFFFFFFFFu ? 0u : best_id;
            return true;
        }
        j ^= 1u;
        box2 = box_dist2(nodes[j - 1], px, py, pz);
    }
    return false;
}

// Winding walk in depth-first order, left child first (a fixed summation order): a node without faces adds 0, a node farther
// from p than beta times its radius adds its dipole term, a near leaf adds pair_omega per face, anything else is opened.  Returns
// the solid angle (4 pi times the winding number) through *omega, false when the iteration cap was reached.
S3D_HD bool bvh_solid_angle(const BvhNode* nodes, const StagedTri* tris, uint32_t F, uint32_t L, float beta, float px, float py, float pz,
                            float* omega_out) {
    float omega = 0.0f;
    uint32_t j = 1;
    const uint32_t cap = 2u * (2u * L - 1u);
    for (uint32_t step = 0; step < cap; step++) {
        const BvhNode& nd = nodes[j - 1];
        if (nd.r >= 0.0f) {
            const float dx = nd.cx - px, dy = nd.cy - py, dz = nd.cz - pz;
            const float dist2 = dot3(dx, dy, dz, dx, dy, dz);
            const float br = beta * nd.r;
            if (dist2 > br * br) {
                omega += dot3(nd.nx, nd.ny, nd.nz, dx, dy, dz) / (dist2 * sqrtf(dist2));
            } else if (j < L) {
                j = 2 * j;
                continue;
            } else {
                const uint32_t base = (j - L) * kBvhLeaf;
                for (uint32_t k = 0; k < kBvhLeaf; k++) {
                    const uint32_t f = base + k;
                    if (f >= F) break;
                    omega += pair_omega(tris[f], px, py, pz);
                }
            }
        }
        j = (j + 1) >> __builtin_ctz(j + 1);  // past every right child on the way up, then the sibling; the root again: done
        if (j == 1) {
            *omega_out = omega;
            return true;
        }
    }
    return false;
}

// both walks for one point, one after the other (the kernel gives each walk a wave of its own)
S3D_HD void bvh_query_point(const BvhNode* nodes, const StagedTri* tris, const int32_t* perm, uint32_t F, uint32_t L, float beta, float px,
                            float py, float pz, float* sdf, float* winding, int32_t* face) {
    float best = 0.0f, omega = 0.0f;
    uint32_t best_face = 0;
    const bool ok_d = bvh_nearest(nodes, tris, perm, F, L, px, py, pz, &best, &best_face);
    const bool ok_w = bvh_solid_angle(nodes, tris, F, L, beta, px, py, pz, &omega);
    pair_finish(ok_d && ok_w, best, omega, sdf, winding);
    *face = (int32_t)best_face;
}

}  // namespace sdfpair
}  // namespace s3d
