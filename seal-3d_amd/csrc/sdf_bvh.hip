// sdf_bvh.hip — the SDF backbone's distance query over a bounding-volume hierarchy (include/seal3d_hip.h "SDF: BVH query";
// DESIGN.md "SDF"): the staging of the sorted faces and the query, one lane per point.  The tree is built on the host
// (sdf/bvh.py); the pair arithmetic and both walks are csrc/sdf_pair.hpp, which the host test compiles as well.
#include "s3d_common.hpp"
#include "sdf_pair.hpp"

namespace s3d {
namespace {

using namespace sdfpair;

constexpr uint32_t kBvhPoints = 64;  // points per workgroup; two waves: one walks for the distance, the other for the winding number

__global__ void __launch_bounds__(256) bvh_stage_kernel(const float* __restrict__ triangles, uint32_t F, StagedTri* __restrict__ staged) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < F) staged[f] = stage_tri(triangles + (size_t)f * 9);
}

// The two walks share nothing but the point, and each is a chain of dependent loads: a wave per walk doubles the waves in flight
// (an item's 2^17 points are otherwise two waves per SIMD), keeps each wave's loop to one walk's branches, and lets a point cost
// the longer of its walks instead of their sum.  Wave 1 hands the solid angle over through LDS; wave 0 signs and writes.
__global__ void __launch_bounds__(2 * kBvhPoints) mesh_sdf_bvh_kernel(const float* __restrict__ points, uint32_t N,
                                                                     const BvhNode* __restrict__ nodes, const StagedTri* __restrict__ tris,
                                                                     const int32_t* __restrict__ perm, uint32_t F, uint32_t L, float beta,
                                                                     float* __restrict__ sdf, float* __restrict__ winding,
                                                                     int32_t* __restrict__ nearest_face) {
    __shared__ float omega_of[kBvhPoints];
    __shared__ uint32_t ok_of[kBvhPoints];
    const uint32_t lane = threadIdx.x & (kBvhPoints - 1u);
    const bool winds = threadIdx.x >= kBvhPoints;  // (wave-uniform)
    const uint32_t n = blockIdx.x * kBvhPoints + lane;
    const size_t row = n < N ? (size_t)n : (size_t)(N - 1);  // (idle lanes of the last workgroup walk for the last point and write nothing)
    const float px = points[row * 3], py = points[row * 3 + 1], pz = points[row * 3 + 2];
    float best = 0.0f;
    uint32_t best_face = 0;
    bool ok = true;
    if (winds) {
        float omega = 0.0f;
        ok_of[lane] = bvh_solid_angle(nodes, tris, F, L, beta, px, py, pz, &omega) ? 1u : 0u;
        omega_of[lane] = omega;
    } else {
        ok = bvh_nearest(nodes, tris, perm, F, L, px, py, pz, &best, &best_face);
    }
    __syncthreads();
    if (winds || n >= N) return;
    float s, w;
    pair_finish(ok && ok_of[lane] != 0u, best, omega_of[lane], &s, &w);
    sdf[n] = s;
    if (winding) winding[n] = w;
    if (nearest_face) nearest_face[n] = (int32_t)best_face;
}

}  // namespace
}  // namespace s3d

using namespace s3d;

S3D_EXPORT int s3d_mesh_bvh_leaf(void) { return (int)sdfpair::kBvhLeaf; }

S3D_EXPORT int s3d_mesh_bvh_stage(const float* triangles, uint32_t F, float* staged, s3d_stream_t stream) {
    if (F == 0) return S3D_OK;
    S3D_REQUIRE(triangles && staged, "mesh_bvh_stage: triangles and staged must not be NULL");
    S3D_REQUIRE((uintptr_t)staged % 16 == 0, "mesh_bvh_stage: the staged records must be 16-byte aligned");
    S3D_REQUIRE(F <= (1u << 26), "mesh_bvh_stage: at most 2^26 triangles");
    hipLaunchKernelGGL(bvh_stage_kernel, dim3(div_up<uint32_t>(F, 256u)), dim3(256), 0, as_stream(stream), triangles, F,
                       (sdfpair::StagedTri*)staged);
    return check_launch("mesh_bvh_stage");
}

S3D_EXPORT int s3d_mesh_sdf_bvh(const float* points, uint32_t N, const float* nodes, const float* staged, const int32_t* perm, uint32_t F,
                                uint32_t L, float beta, float* sdf, float* winding, int32_t* nearest_face, s3d_stream_t stream) {
    S3D_REQUIRE(F > 0, "mesh_sdf_bvh: the mesh has no triangles");
    S3D_REQUIRE(F <= (1u << 26), "mesh_sdf_bvh: at most 2^26 triangles");
    S3D_REQUIRE(L > 0 && (L & (L - 1)) == 0, "mesh_sdf_bvh: the number of leaves must be a power of two, got %u", L);
    S3D_REQUIRE((uint64_t)L * sdfpair::kBvhLeaf >= F && L <= (1u << 24), "mesh_sdf_bvh: %u leaves of %u faces do not hold %u faces", L,
                sdfpair::kBvhLeaf, F);
    S3D_REQUIRE(beta > 0.0f && beta <= 3.402823466e+38f, "mesh_sdf_bvh: beta must be positive and finite");
    if (N == 0) return S3D_OK;
    S3D_REQUIRE(points && nodes && staged && perm && sdf, "mesh_sdf_bvh: points, nodes, staged, perm and sdf must not be NULL");
    S3D_REQUIRE((uintptr_t)nodes % 16 == 0 && (uintptr_t)staged % 16 == 0, "mesh_sdf_bvh: nodes and staged must be 16-byte aligned");
    S3D_REQUIRE(N <= 0xFFFFFF00u, "mesh_sdf_bvh: at most 2^32 - 256 points per call");
    hipLaunchKernelGGL(mesh_sdf_bvh_kernel, dim3(div_up<uint32_t>(N, kBvhPoints)), dim3(2 * kBvhPoints), 0, as_stream(stream), points, N,
                       (const sdfpair::BvhNode*)nodes, (const sdfpair::StagedTri*)staged, perm, F, L, beta, sdf, winding, nearest_face);
    return check_launch("mesh_sdf_bvh");
}
