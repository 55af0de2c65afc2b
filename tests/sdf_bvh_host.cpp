// Both routes of csrc/sdf_pair.hpp on the host, the BVH walks and the brute-force loop that mesh_sdf_kernel runs: tests/test_sdf_bvh.py
// compiles this file with the address and undefined-behaviour sanitizers and runs it on trees that sdf/bvh.py built.
//   sdf_bvh_host IN OUT
// IN:  uint32 N, F, L; float beta; points [N,3]; nodes [2L-1,16]; triangles [F,3,3] in sorted order; perm [F] int32
// OUT: per point, the BVH's sdf, winding, face [N each], then the same three from a brute-force loop over the faces in their
//      original order (pair_accumulate and pair_finish of the same header), then uint32: the points whose walk hit its cap
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sdf_pair.hpp"

using namespace s3d::sdfpair;

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t head[3];
    float beta;
    if (fread(head, 4, 3, in) != 3 || fread(&beta, 4, 1, in) != 1) return 3;
    const uint32_t N = head[0], F = head[1], L = head[2];
    if (F == 0 || F > (1u << 26) || L == 0 || (L & (L - 1)) != 0 || L > (1u << 24) || (uint64_t)L * kBvhLeaf < F || !(beta > 0.0f)) return 3;
    std::vector<float> points, tri;
    std::vector<BvhNode> nodes;
    std::vector<int32_t> perm;
    if (!read_n(in, points, (size_t)N * 3) || !read_n(in, nodes, (size_t)2 * L - 1) || !read_n(in, tri, (size_t)F * 9) || !read_n(in, perm, F))
        return 3;
    fclose(in);
    std::vector<StagedTri> staged(F), original(F);
    for (uint32_t k = 0; k < F; k++) {
        if (perm[k] < 0 || (uint32_t)perm[k] >= F) return 3;
        staged[k] = stage_tri(&tri[(size_t)k * 9]);
        original[perm[k]] = staged[k];
    }
    std::vector<float> sdf(N), w(N), bsdf(N), bw(N);
    std::vector<int32_t> face(N), bface(N);
    uint32_t capped = 0;
    for (uint32_t n = 0; n < N; n++) {
        const float px = points[(size_t)n * 3], py = points[(size_t)n * 3 + 1], pz = points[(size_t)n * 3 + 2];
        bvh_query_point(nodes.data(), staged.data(), perm.data(), F, L, beta, px, py, pz, &sdf[n], &w[n], &face[n]);
        if (std::isnan(sdf[n])) capped++;
        float best = 3.402823466e+38f, omega = 0.0f;
        uint32_t best_face = 0;
        for (uint32_t f = 0; f < F; f++) pair_accumulate(original[f], f, px, py, pz, &best, &best_face, &omega);
        pair_finish(true, best, omega, &bsdf[n], &bw[n]);
        bface[n] = (int32_t)best_face;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    bool ok = true;
    if (N) {
        ok = fwrite(sdf.data(), 4, N, out) == N && fwrite(w.data(), 4, N, out) == N && fwrite(face.data(), 4, N, out) == N &&
             fwrite(bsdf.data(), 4, N, out) == N && fwrite(bw.data(), 4, N, out) == N && fwrite(bface.data(), 4, N, out) == N;
    }
    ok = ok && fwrite(&capped, 4, 1, out) == 1;
    return fclose(out) == 0 && ok ? 0 : 4;
}
