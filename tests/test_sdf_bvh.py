"""The mesh BVH without a GPU: what sdf/bvh.py builds against the header's tree contract (tests/sdf_bvh_witness.py states it node
by node), the witness's two walks against the brute-force witness (tests/sdf_witness.py), and the kernel's own traversal code
(csrc/sdf_pair.hpp) compiled for the host under the address and undefined-behaviour sanitizers and run on the same trees."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sdf_bvh_witness as bw
import sdf_witness as sw
from conftest import REPO

CASES = bw.cases()
NAMES = list(CASES)
W_CAP = 0.05  # a tenth of the gap between a closed mesh's winding numbers (0 or 1) and the sign rule's cut at 0.5


@pytest.fixture(scope="module")
def MeshBVH():
    import s3d_hip
    if not os.path.exists(s3d_hip.LIB_PATH):
        s3d_hip.build()
    from sdf.bvh import MeshBVH
    return MeshBVH


@pytest.fixture(scope="module")
def trees(MeshBVH):
    return {name: MeshBVH(tris) for name, (tris, _) in CASES.items()}


def _points(name):
    tris = CASES[name][0]
    return np.concatenate([bw.query_points(tris, 192, 64, seed=len(tris)), bw.surface_points(tris, 8)])


# ---- the tree ----------------------------------------------------------------------------------------------------------------
def test_leaf_size_is_the_librarys(MeshBVH):
    import s3d_hip
    assert s3d_hip.SdfBackend.bvh_leaf() == bw.LEAF == 4


@pytest.mark.parametrize("name", NAMES)
def test_tree_invariants(trees, name):
    tris = CASES[name][0]
    b, ref = trees[name], bw.build(tris)
    F, L = len(tris), bw.leaves_for(len(tris))
    assert (b.F, b.L, b.leaf) == (F, L, bw.LEAF) and 2 ** b.depth == L and b.nodes.shape == (2 * L - 1, 16)
    assert L * bw.LEAF >= F and (L == 1 or L // 2 * bw.LEAF < F)
    assert sorted(b.perm.tolist()) == list(range(F))
    assert np.array_equal(b.perm, ref["perm"])  # (Morton order, ties by the original index)
    assert np.array_equal(b.triangles_sorted, tris[b.perm].astype(np.float32))
    for i in range(2 * L - 1):
        first, last = b.node_range(i)
        assert (first, last) == bw.node_range(i, F, L)
        if i < L - 1:  # the children's ranges partition the parent's
            assert b.node_range(2 * i + 1)[0] == first and b.node_range(2 * i + 1)[1] == b.node_range(2 * i + 2)[0]
            assert b.node_range(2 * i + 2)[1] == last
        else:
            assert last - first <= bw.LEAF and first == min((i - (L - 1)) * bw.LEAF, F)
        nd = b.nodes[i].astype(np.float64)
        if first == last:  # padding: inverted bounds, the marker, no dipole
            assert np.isposinf(nd[0:3]).all() and np.isneginf(nd[4:7]).all() and nd[11] == -1 and (nd[8:11] == 0).all() and (nd[12:15] == 0).all()
            continue
        tt = tris[b.perm[first:last]]
        vv = tt.reshape(-1, 3)
        assert (nd[0:3] < vv.min(0)).all() and (nd[4:7] > vv.max(0)).all()  # one step outward
        assert (nd[0:3] >= np.nextafter(vv.min(0).astype(np.float32), np.float32(-np.inf))).all()
        assert (nd[4:7] <= np.nextafter(vv.max(0).astype(np.float32), np.float32(np.inf))).all()
        np.testing.assert_allclose(nd[8:11], ref["nodes"][i, 8:11], rtol=0, atol=1e-6)
        r64 = np.linalg.norm(vv - nd[8:11], axis=1).max()  # about the centroid AS STORED, which is what the kernel measures from
        assert r64 <= nd[11] <= r64 * (1 + 2.0 ** -22) + 1e-37
        assert abs(nd[11] - ref["nodes"][i, 11]) <= 2e-6
        # Nsum to 1e-6 of the node's summed face areas: on a closed node the sum itself cancels to rounding noise
        scale = np.linalg.norm(0.5 * np.cross(tt[:, 1] - tt[:, 0], tt[:, 2] - tt[:, 0]), axis=1).sum()
        assert np.abs(nd[12:15] - ref["nodes"][i, 12:15]).max() <= 1e-6 * scale


def test_refuses_what_it_cannot_hold(MeshBVH, monkeypatch):
    import sdf.bvh
    assert sdf.bvh.MAX_FACES == 2 ** 26
    with pytest.raises(ValueError):
        MeshBVH(np.zeros((0, 3, 3), np.float32))
    monkeypatch.setattr(sdf.bvh, "MAX_FACES", 19)  # (the limit itself needs 2.4 GB of triangles)
    with pytest.raises(ValueError, match="at most"):
        MeshBVH(CASES["icosphere 20"][0])
    monkeypatch.undo()
    b = MeshBVH(CASES["icosphere 20"][0])
    b.perm[0] = b.perm[1]
    with pytest.raises(AssertionError, match="permutation"):
        b.check()


# ---- the walks, float64, against the brute-force witness -------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_witness_walks_against_brute_force(trees, name):
    tris, closed = CASES[name]
    b, p = trees[name], _points(name).astype(np.float64)
    D2, Om = bw.pair_tables(p, tris)
    _, w_ref, face_ref, dist_ref = sw.mesh_sdf(p, tris)
    best, face, visited = bw.walk_nearest(p, b.nodes, b.perm.astype(np.int64), b.F, b.L, D2)
    assert np.array_equal(np.sqrt(best), dist_ref) and np.array_equal(face, face_ref)
    w, tests = bw.walk_winding(p, b.nodes, b.perm.astype(np.int64), b.F, b.L, Om, beta=3.0)
    dw = float(np.abs(w - w_ref).max())
    print(f"[sdf bvh witness] {name}: max |dw| {dw:.3e}; faces visited per point {visited.mean():.1f} of {b.F}, winding tests {tests.mean():.1f}")
    assert dw <= W_CAP
    if closed:
        off = np.abs(w_ref - 0.5) > W_CAP
        assert ((w > 0.5) == (w_ref > 0.5))[off].all()
    if b.F >= 255:
        assert visited.mean() < b.F / 4  # (the walk prunes: otherwise it is brute force with extra steps)


# ---- the kernel's traversal code on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the traversal code for the host"
    exe = str(tmp_path_factory.mktemp("sdf_bvh_host") / "sdf_bvh_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: it runs as it is, nothing preloaded)
                    "-I", os.path.join(REPO, "seal-3d_amd", "csrc"), os.path.join(REPO, "tests", "sdf_bvh_host.cpp"), "-o", exe],
                   check=True)
    return exe


def _run_host(exe, folder, b, points32, beta):
    src, dst = str(folder / "in.bin"), str(folder / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(points32), b.F, b.L], np.uint32).tobytes() + np.float32(beta).tobytes())
        for a in (points32.astype(np.float32), b.nodes, b.triangles_sorted, b.perm):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    N = len(points32)
    raw = open(dst, "rb").read()
    assert len(raw) == 24 * N + 4
    f32 = np.frombuffer(raw, np.float32, 6 * N).reshape(6, N)
    i32 = np.frombuffer(raw, np.int32, 6 * N).reshape(6, N)
    capped = int(np.frombuffer(raw, np.uint32, 1, 24 * N)[0])
    return (f32[0], f32[1], i32[2]), (f32[3], f32[4], i32[5]), capped


@pytest.mark.parametrize("name", NAMES)
def test_traversal_code_on_the_host_under_sanitizers(trees, host_program, tmp_path, name):
    tris, closed = CASES[name]
    b, p32 = trees[name], _points(name)
    (sdf, w, face), (bsdf, bwind, bface), capped = _run_host(host_program, tmp_path, b, p32, 3.0)
    assert capped == 0 and np.isfinite(sdf).all() and np.isfinite(w).all()
    # the same pair loop, pruned or not: the same bits and the same face
    assert np.array_equal(np.abs(sdf).view(np.uint32), np.abs(bsdf).view(np.uint32))
    assert np.array_equal(face, bface)
    assert float(np.abs(w.astype(np.float64) - bwind).max()) <= W_CAP
    # the float32 evaluation of the witness on the same tree: the far decisions are the same expressions, the sums differ by rounding
    t32 = tris.astype(np.float32)
    D2, Om = bw.pair_tables(p32, t32)
    w32, _ = bw.walk_winding(p32, b.nodes, b.perm.astype(np.int64), b.F, b.L, Om, beta=3.0)
    best32, _, _ = bw.walk_nearest(p32, b.nodes, b.perm.astype(np.int64), b.F, b.L, D2)
    # (without the rows placed ON the mesh: there the solid angle of the face that holds the point jumps by 2 pi, and whether fp32
    #  rounds the numerator to exactly 0 differs between the kernel's -(p - A).n and the witness's a.(b x c) — a property of the
    #  pair test, the same on the brute-force route, and none of the tree)
    off = slice(0, len(p32) - len(bw.surface_points(tris, 8)))
    dw = float(np.abs(w.astype(np.float64) - w32)[off].max())
    ref64 = sw.mesh_sdf(p32.astype(np.float64), tris)
    e32 = float(np.abs(np.sqrt(best32).astype(np.float64) - ref64[3]).max())
    err = float(np.abs(np.abs(sdf).astype(np.float64) - ref64[3]).max())
    print(f"[sdf bvh host] {name}: winding against the float32 witness {dw:.3e}; distance error {err:.3e} (float32 witness {e32:.3e})")
    assert dw <= 1e-5
    assert err <= 4 * e32 + 2.0 ** -22


def test_host_program_refuses_a_malformed_tree(trees, host_program, tmp_path):
    """the program under the sanitizers checks what it reads before it indexes with it"""
    b = trees["shells 5"]
    src = str(tmp_path / "bad.bin")
    with open(src, "wb") as f:
        f.write(np.array([1, b.F, 3], np.uint32).tobytes() + np.float32(3.0).tobytes())
    r = subprocess.run([host_program, src, str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 3 and not r.stderr
