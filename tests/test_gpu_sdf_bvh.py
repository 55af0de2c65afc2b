"""s3d_mesh_sdf_bvh on the GPU against s3d_mesh_sdf on the same points: |sdf| and nearest face bit for bit, the winding number within
a tenth of the sign rule's margin, the sign wherever brute force's winding number is off the cut; determinism, the argument checks,
and the dataset's two routes.  Meshes and points are those of tests/test_sdf_bvh.py, which runs the same traversal code on the
host first."""
import types

import numpy as np
import pytest
import torch

import sdf_bvh_witness as bw
import sdf_witness as sw

pytestmark = pytest.mark.gpu

CASES = bw.cases()
W_CAP = 0.05  # a tenth of the gap between a closed mesh's winding numbers (0 or 1) and the sign rule's cut at 0.5
SIZES = (1, 63, 64, 65, 257)


def _pool(tris):
    """(257 fp32 points, the rows placed on the mesh by construction): perturbed surface points, uniform points in the cube,
    points out to |x| = 3, and vertices / edge midpoints / centroids, interleaved so that every prefix holds each kind"""
    on = bw.surface_points(tris, 9)[:65]
    on = on[np.arange(65) % len(on)]
    near = bw.query_points(tris, 64, 64, seed=len(tris) + 1)
    far = (np.random.default_rng(len(tris) + 2).random((64, 3)) * 6 - 3).astype(np.float32)
    pts = np.empty((257, 3), np.float32)
    pts[0::4], pts[1::4], pts[2::4], pts[3::4] = on, near[:64], near[64:], far
    placed = np.zeros(257, bool)
    placed[0::4] = True
    return pts, placed


def _both(hip, bvh, tris_dev, pts, beta=3.0):
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
    brute = hip.SdfBackend.mesh_sdf(p, tris_dev, want_winding=True, want_face=True)
    tree = hip.SdfBackend.mesh_sdf_bvh(p, bvh, beta=beta, want_winding=True, want_face=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in brute], [t.cpu().numpy() for t in tree]


def _compare(brute, tree, closed, placed, label):
    (sdf0, w0, face0), (sdf1, w1, face1) = brute, tree
    assert np.isfinite(sdf1).all() and np.isfinite(w1).all(), f"{label}: NaN: a walk reached its iteration cap"
    assert np.array_equal(np.abs(sdf1).view(np.uint32), np.abs(sdf0).view(np.uint32)), label
    assert np.array_equal(face1, face0), label
    dw = float(np.abs(w1.astype(np.float64) - w0).max())
    assert dw <= W_CAP, (label, dw)
    off = np.abs(w0.astype(np.float64) - 0.5) > W_CAP
    assert np.array_equal(sdf1[off] < 0, sdf0[off] < 0), label
    if closed:  # only a point ON the mesh has a winding number near the cut
        assert int((~off & ~placed).sum()) == 0, (label, np.nonzero(~off & ~placed)[0], w0[~off & ~placed])
    return dw, int((~off).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_distance_and_face_bit_for_bit_winding_within_the_cap(hip, name):
    from sdf.bvh import MeshBVH
    tris, closed = CASES[name]
    bvh = MeshBVH(tris)
    tris_dev = torch.from_numpy(tris.astype(np.float32)).cuda()
    pts, placed = _pool(tris)
    worst, near_cut = 0.0, 0
    for N in SIZES:
        brute, tree = _both(hip, bvh, tris_dev, pts[:N])
        dw, cut = _compare(brute, tree, closed, placed[:N], f"{name} N {N}")
        worst, near_cut = max(worst, dw), cut
    print(f"[sdf bvh] {name}: F {bvh.F} L {bvh.L} max |dw| {worst:.3e}; rows within {W_CAP} of the cut at N 257: {near_cut} (placed on the mesh: {int(placed.sum())})")


def test_a_deeper_tree(hip):
    from sdf.bvh import MeshBVH
    v, f = sw.icosphere(5, 0.8)
    tris = v[f].astype(np.float32)
    bvh = MeshBVH(tris)
    assert (bvh.F, bvh.L, bvh.depth) == (20480, 8192, 13)
    pts = bw.query_points(tris, 3072, 1024, seed=5)
    brute, tree = _both(hip, bvh, torch.from_numpy(tris).cuda(), pts)
    dw, cut = _compare(brute, tree, True, np.zeros(len(pts), bool), "icosphere 20480")
    print(f"[sdf bvh] icosphere 20480: max |dw| {dw:.3e}; rows within {W_CAP} of the cut: {cut}")


def test_two_calls_give_the_same_bits(hip):
    from sdf.bvh import MeshBVH
    tris = CASES["icosphere 1280"][0]
    bvh = MeshBVH(tris)
    p = torch.from_numpy(bw.query_points(tris, 1024, 1024, seed=3)).cuda()
    a = hip.SdfBackend.mesh_sdf_bvh(p, bvh, want_winding=True, want_face=True)
    b = hip.SdfBackend.mesh_sdf_bvh(p, bvh, want_winding=True, want_face=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    only = hip.SdfBackend.mesh_sdf_bvh(p, bvh)  # (without the optional outputs)
    assert torch.equal(only.view(torch.int32), a[0].view(torch.int32))


def test_argument_checks(hip):
    from sdf.bvh import MeshBVH
    bvh = MeshBVH(CASES["shells 5"][0])
    p = torch.zeros(4, 3, device="cuda")
    arrays = bvh.device_arrays(p.device)

    def stub(F=bvh.F, L=bvh.L):
        return types.SimpleNamespace(F=F, L=L, device_arrays=lambda device: arrays)
    for beta in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="beta"):
            hip.SdfBackend.mesh_sdf_bvh(p, bvh, beta=beta)
    with pytest.raises(RuntimeError, match="no triangles"):
        hip.SdfBackend.mesh_sdf_bvh(p, stub(F=0))
    with pytest.raises(RuntimeError, match="power of two"):
        hip.SdfBackend.mesh_sdf_bvh(p, stub(L=3))
    with pytest.raises(RuntimeError, match="do not hold"):
        hip.SdfBackend.mesh_sdf_bvh(p, stub(L=1))
    assert hip.SdfBackend.mesh_sdf_bvh(p[:0], bvh).shape == (0,)  # N == 0: OK, nothing launched
    assert torch.isfinite(hip.SdfBackend.mesh_sdf_bvh(p, bvh)).all()


def test_dataset_routes(hip):
    from sdf import provider
    v, f = sw.icosphere(3, 0.8)
    brute = provider.SDFDataset((v, f), size=4, num_samples=2 ** 12, seed=1, accel="brute")
    tree = provider.SDFDataset((v, f), size=4, num_samples=2 ** 12, seed=1, accel="bvh")
    assert brute.bvh is None and tree.bvh is not None and tree.bvh.F == 1280
    for i in (0, 3):
        a, b = brute[i], tree[i]
        assert torch.equal(a["points"], b["points"])
        assert torch.equal(a["sdfs"].view(torch.int32), b["sdfs"].view(torch.int32))
        assert (a["sdfs"][2 ** 11:] != 0).any()
    for level in (0, 3, 4):
        vv, ff = sw.icosphere(level, 0.8)
        auto = provider.SDFDataset((vv, ff), size=1, num_samples=64)
        assert auto.accel == ("bvh" if len(ff) >= provider.BVH_AUTO_MIN_FACES else "brute")
        assert (auto.bvh is not None) == (auto.accel == "bvh")
    with pytest.raises(ValueError, match="accel"):
        provider.SDFDataset((v, f), num_samples=64, accel="grid")
