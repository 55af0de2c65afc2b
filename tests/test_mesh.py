"""Mesh export without a GPU: the generated case table, the numpy witness (tests/mc_witness.py) against the surface's
invariants, extract_fields against the executed reference, PLY I/O and config_from_mesh."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

import mc_witness as w
from tools import gen_mc_tables as mct
from tools.gen_mesh_golden import golden_query

FLT_MAX = np.finfo(np.float32).max


# ------------------------------------------------------------------------------------------------ shared inputs
def random_volume(seed, shape=(24, 24, 24)):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def lattice(n=33):
    g = np.linspace(-1.0, 1.0, n, dtype=np.float32)
    return np.meshgrid(g, g, g, indexing="ij")


def sphere_volume(r=0.6):
    X, Y, Z = lattice()
    return (np.float32(r) - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)


def torus_volume(R=0.55, r=0.25):
    X, Y, Z = lattice()
    q = np.sqrt(X * X + Y * Y) - np.float32(R)
    return (np.float32(r) - np.sqrt(q * q + Z * Z)).astype(np.float32)


UNIT = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
SPHERE_R, SPHERE_H = 0.6, 2.0 / 32


def planted_volume():
    """a random 24^3 field with NaN and +-inf at 20 random points"""
    u = random_volume(7)
    rng = np.random.default_rng(8)
    idx = rng.choice(u.size, size=20, replace=False)
    u.reshape(-1)[idx] = np.array([np.nan, np.inf, -np.inf, np.nan, np.inf] * 4, dtype=np.float32)
    return u


PLANTED_BOUNDS = [-1.0, 0.0, 2.0, 1.0, 3.0, 2.5]


def one_corner_volume():
    u = np.full((2, 2, 2), -1.0, dtype=np.float32)
    u[0, 0, 0] = 1.0
    return u


def interior_edges_ok(verts_index_space, tris, shape):
    """every mesh edge that is not on the volume's boundary is in exactly two triangles, traversed in opposite directions"""
    e, fwd, bwd = w.edge_use(tris)
    ev = verts_index_space[e]  # [E, 2, 3]
    hi = np.asarray(shape, dtype=np.float32) - 1
    on_face = ((ev[:, 0] == ev[:, 1]) & ((ev[:, 0] == 0) | (ev[:, 0] == hi))).any(axis=1)  # both ends on one boundary plane
    good = (fwd == 1) & (bwd == 1)
    return bool(np.all(good | on_face)) and bool(np.all((fwd + bwd <= 2)))


def check_sphere(v, t):
    assert w.is_closed(t)
    assert w.euler(v, t) == 2
    assert w.signed_volume(v, t) > 0
    bound = SPHERE_H ** 2 / (8 * (SPHERE_R - SPHERE_H))
    dist = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - SPHERE_R)
    print("sphere: max | |v| - r | =", dist.max(), "bound", bound)
    assert dist.max() <= bound


def check_torus(v, t):
    assert w.is_closed(t)
    assert w.euler(v, t) == 0


def check_planted(v, t, bounds=PLANTED_BOUNDS):
    b = np.asarray(bounds, dtype=np.float32)
    assert len(v) > 0 and np.isfinite(v).all()
    assert (v >= b[:3]).all() and (v <= b[3:]).all()
    assert t.min() >= 0 and t.max() < len(v)


# ------------------------------------------------------------------------------------------------ table generator
def test_table_has_256_cases_and_complement_uses_the_same_edges():
    assert len(mct.TRI_TABLE) == 256 and len(mct.TRI_COUNT) == 256
    assert mct.TRI_COUNT[0] == 0 and mct.TRI_COUNT[255] == 0
    assert all(e < 0 for e in mct.TRI_TABLE[0]) and all(e < 0 for e in mct.TRI_TABLE[255])
    for c in range(256):
        row = mct.TRI_TABLE[c]
        assert len(row) == 3 * mct.MC_MAX_TRIS
        used = [e for e in row if e >= 0]
        assert len(used) == 3 * mct.TRI_COUNT[c] and all(e >= 0 for e in row[:len(used)])
        assert set(used) == {e for e in mct.TRI_TABLE[255 - c] if e >= 0}


def test_every_listed_edge_crosses_and_every_crossing_edge_is_listed():
    for c in range(256):
        crossing = {e for e, (a, b) in enumerate(mct.EDGE_ENDS) if ((c >> a) & 1) != ((c >> b) & 1)}
        assert {e for e in mct.TRI_TABLE[c] if e >= 0} == crossing, c


def test_committed_header_is_what_the_generator_prints():
    with open(os.path.join(REPO, "seal-3d_amd", "csrc", "mc_tables.h")) as f:
        assert f.read() == mct.header_text()
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_mc_tables.py"), "--print"], capture_output=True, text=True,
                         check=True).stdout
    assert out == mct.header_text()


# ------------------------------------------------------------------------------------------------ witness invariants
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_field_is_a_manifold_with_every_case_present(seed):
    u = random_volume(seed)
    hist = np.bincount(w.cell_cases(u, 0.0).reshape(-1), minlength=256)
    assert hist.min() > 0, "a case is missing from the volume"
    v, t = w.marching_cubes(u, 0.0)  # identity bounds: v is in index space
    assert interior_edges_ok(v, t, u.shape)
    _, tp = w.marching_cubes(np.pad(u, 1, constant_values=-1.0), 0.0)
    assert w.is_closed(tp)


def test_vertices_lie_on_their_edges():
    u = random_volume(0)
    v, _ = w.marching_cubes(u, 0.0)
    frac = np.abs(v - np.rint(v)) > 1e-4  # (v / 23 * 23 is v up to an ulp or two)
    assert (frac.sum(axis=1) <= 1).all()  # at most one coordinate is off the lattice
    assert (v >= 0).all() and (v <= 23).all()


# ------------------------------------------------------------------------------------------------ analytic fields
def test_sphere():
    check_sphere(*w.marching_cubes(sphere_volume(), 0.0, UNIT))


def test_torus():
    check_torus(*w.marching_cubes(torus_volume(), 0.0, UNIT))


# ------------------------------------------------------------------------------------------------ degenerate inputs
def test_all_solid_and_all_empty_volumes_are_empty_meshes():
    for value in (1.0, -1.0):
        v, t = w.marching_cubes(np.full((5, 4, 3), value, dtype=np.float32), 0.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_nan_and_inf_give_finite_vertices_inside_the_bounds():
    check_planted(*w.marching_cubes(planted_volume(), 0.0, PLANTED_BOUNDS))


def test_one_solid_corner_is_one_triangle():
    v, t = w.marching_cubes(one_corner_volume(), 0.0)
    assert v.shape == (3, 3) and t.shape == (1, 3)
    assert sorted(t[0].tolist()) == [0, 1, 2]
    n = np.cross(v[t[0, 1]] - v[t[0, 0]], v[t[0, 2]] - v[t[0, 0]])
    assert (n > 0).all()  # away from the solid corner at the origin


# ------------------------------------------------------------------------------------------------ extract_fields
def test_extract_fields_reproduces_the_reference_bit_for_bit():
    from nerf.mesh import extract_fields
    g = np.load(os.path.join(GOLDEN, "mesh_fields.npz"))
    seen = []

    def query(pts):
        seen.append(pts.clone())
        return golden_query(pts)

    u = extract_fields(torch.from_numpy(g["bound_min"]), torch.from_numpy(g["bound_max"]), int(g["resolution"]), query, S=int(g["S"]))
    assert isinstance(u, torch.Tensor) and u.dtype == torch.float32
    assert len(seen) == int(g["n_chunks"])
    assert np.array_equal(seen[-1].numpy(), g["pts_last"])
    assert np.array_equal(u.numpy(), g["u"])


# ------------------------------------------------------------------------------------------------ file I/O
def test_write_then_read_ply_is_exact(tmp_path):
    from nerf.mesh import read_ply, write_ply
    v, t = w.marching_cubes(random_volume(3, (9, 7, 5)), 0.0, [-1, 0, 1, 2, 3, 5])
    path = str(tmp_path / "m.ply")
    write_ply(path, torch.from_numpy(v), torch.from_numpy(t))
    v2, t2 = read_ply(path)
    assert v2.dtype == np.float32 and t2.dtype == np.int32
    assert np.array_equal(v, v2) and np.array_equal(t, t2)
    with open(path, "rb") as f:
        head = f.read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices" in head


def test_read_ascii_ply_with_double_vertices_and_uint_indices(tmp_path):
    from nerf.mesh import read_ply
    path = tmp_path / "hand.ply"
    path.write_text("ply\nformat ascii 1.0\ncomment written by hand\nelement vertex 4\nproperty double x\nproperty double y\n"
                    "property double z\nproperty uchar red\nelement face 2\nproperty list uchar uint vertex_indices\nend_header\n"
                    "0 0 0 255\n1 0 0.5 0\n0 1 0 7\n0.25 0.125 1 9\n3 0 1 2\n3 0 2 3\n")
    v, t = read_ply(str(path))
    assert np.array_equal(v, np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0], [0.25, 0.125, 1]], dtype=np.float32))
    assert np.array_equal(t, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))


def test_other_mesh_formats_are_refused(tmp_path):
    from nerf.mesh import read_ply, write_ply
    with pytest.raises(NotImplementedError, match=r"\.ply"):
        write_ply(str(tmp_path / "m.obj"), np.zeros((0, 3)), np.zeros((0, 3)))
    with pytest.raises(NotImplementedError, match=r"\.ply"):
        read_ply(str(tmp_path / "m.glb"))


# ------------------------------------------------------------------------------------------------ config
def test_config_from_mesh_feeds_get_seal_mapper(tmp_path):
    from nerf.mesh import write_ply
    from sealnerf import seal_utils as su
    v, t = w.marching_cubes(sphere_volume()[8:25, 8:25, 8:25], 0.3, [-0.3, -0.3, -0.3, 0.3, 0.3, 0.3])
    path = str(tmp_path / "marked.ply")
    write_ply(path, v, t)
    cfg = su.config_from_mesh(path, "bbox")
    assert cfg["type"] == "bbox" and np.array_equal(np.asarray(cfg["raw"], dtype=np.float32), v)
    assert isinstance(su.get_seal_mapper(config_dict=cfg), su.SealBBoxMapper)
    for kind in ("brush", "anchor"):
        assert su.config_from_mesh(path, kind)["type"] == kind
