"""GPU: the HIP marching cubes (csrc/mesh.hip) against the numpy witness (tests/mc_witness.py) — triangles as integers,
vertices to the rounding of the world mapping — the surface's invariants on the GPU output, the C ABI's guards, the field
extraction against the executed reference and Trainer.save_mesh end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import mc_witness as w
import test_mesh as cases
from tools.gen_mesh_golden import golden_query

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def gpu_mc(hip, u, iso, bounds):
    v, t = hip.MeshBackend.marching_cubes(torch.from_numpy(np.ascontiguousarray(u)).cuda(), iso, bounds)
    assert v.is_cuda and t.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32
    assert v.dim() == 2 and v.shape[1] == 3 and t.dim() == 2 and t.shape[1] == 3
    return v.cpu().numpy(), t.cpu().numpy()


def identity_bounds(shape):
    return [0.0, 0.0, 0.0] + [float(n - 1) for n in shape]


PARITY = {
    "random0": lambda: cases.random_volume(0),
    "random1": lambda: cases.random_volume(1),
    "random2": lambda: cases.random_volume(2),
    "odd_67x35x19": lambda: cases.random_volume(11, (67, 35, 19)),  # 44,555 points: 44 scan blocks, a partial last one
    "sliver_130x3x2": lambda: cases.random_volume(12, (130, 3, 2)),
}
ASYMMETRIC = [-1.5, 0.25, 2.0, 0.5, 3.0, 2.75]


@pytest.mark.parametrize("bounds_kind", ["identity", "asymmetric"])
@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_witness(hip, name, bounds_kind):
    u = PARITY[name]()
    bounds = identity_bounds(u.shape) if bounds_kind == "identity" else ASYMMETRIC
    v_ref, t_ref = w.marching_cubes(u, 0.0, bounds)
    v, t = gpu_mc(hip, u, 0.0, bounds)
    assert t.shape == t_ref.shape and np.array_equal(t, t_ref)
    assert v.shape == v_ref.shape
    tol = 2 * 2.0 ** -23 * max(abs(b) for b in bounds)
    err = np.abs(v.astype(np.float64) - v_ref.astype(np.float64)).max()
    print(name, bounds_kind, "V", len(v), "T", len(t), "max vertex error", err, "tolerance", tol)
    assert err <= tol


def test_volume_is_not_modified_and_a_second_call_gives_the_same_mesh(hip):
    u = torch.from_numpy(cases.planted_volume()).cuda()
    keep = u.clone()
    a = hip.MeshBackend.marching_cubes(u, 0.0, cases.PLANTED_BOUNDS)
    b = hip.MeshBackend.marching_cubes(u, 0.0, cases.PLANTED_BOUNDS)
    assert torch.equal(u.view(torch.int32), keep.view(torch.int32))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ invariants
def test_sphere_on_the_gpu(hip):
    cases.check_sphere(*gpu_mc(hip, cases.sphere_volume(), 0.0, cases.UNIT))


def test_torus_on_the_gpu(hip):
    cases.check_torus(*gpu_mc(hip, cases.torus_volume(), 0.0, cases.UNIT))


def test_padded_random_field_is_closed_on_the_gpu(hip):
    u = np.pad(cases.random_volume(0), 1, constant_values=-1.0)
    _, t = gpu_mc(hip, u, 0.0, identity_bounds(u.shape))
    assert w.is_closed(t)


def test_degenerate_inputs_on_the_gpu(hip):
    for value in (1.0, -1.0):
        v, t = gpu_mc(hip, np.full((5, 4, 3), value, dtype=np.float32), 0.0, identity_bounds((5, 4, 3)))
        assert v.shape == (0, 3) and t.shape == (0, 3)
    v, t = gpu_mc(hip, cases.planted_volume(), 0.0, cases.PLANTED_BOUNDS)
    cases.check_planted(v, t)
    v_ref, t_ref = w.marching_cubes(cases.planted_volume(), 0.0, cases.PLANTED_BOUNDS)
    assert np.array_equal(t, t_ref) and np.abs(v - v_ref).max() <= 2 * 2.0 ** -23 * 3.0
    v, t = gpu_mc(hip, cases.one_corner_volume(), 0.0, identity_bounds((2, 2, 2)))
    assert v.shape == (3, 3) and t.shape == (1, 3)
    assert (np.cross(v[t[0, 1]] - v[t[0, 0]], v[t[0, 2]] - v[t[0, 0]]) > 0).all()


# ------------------------------------------------------------------------------------------------ guards
def _abi_call(hip, u, nx, ny, nz, V_arg, T_arg, verts, tris):
    lib, u32, f32 = hip.lib(), C.c_uint32, C.c_float
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    nbytes = lib.s3d_mc_workspace_bytes(u32(nx), u32(ny), u32(nz))
    ws = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int32, device="cuda")
    bounds = torch.tensor(cases.UNIT, device="cuda")
    rc_count = lib.s3d_mc_count(p(u), u32(nx), u32(ny), u32(nz), f32(0.0), p(ws), p(totals), stream)
    torch.cuda.synchronize()
    rc_emit = lib.s3d_mc_emit(p(u), u32(nx), u32(ny), u32(nz), f32(0.0), p(ws), p(bounds), p(verts), u32(V_arg), p(tris), u32(T_arg), stream)
    torch.cuda.synchronize()
    return int(nbytes), rc_count, rc_emit, totals.cpu().numpy().view(np.uint32)


def test_wrong_totals_and_a_flat_axis_are_refused_without_a_write(hip):
    vol = cases.random_volume(5, (12, 11, 10))
    u = torch.from_numpy(vol).cuda()
    v_ref, t_ref = w.marching_cubes(vol, 0.0, cases.UNIT)
    V, T = len(v_ref), len(t_ref)
    assert hip.lib().s3d_mc_workspace_bytes(C.c_uint32(12), C.c_uint32(11), C.c_uint32(10)) <= 16 * vol.size

    def buffers():
        return (torch.full((V + 64, 3), -77.0, device="cuda"), torch.full((T + 64, 3), -77, dtype=torch.int32, device="cuda"))

    for V_arg, T_arg in ((V - 1, T), (V + 1, T), (V, T - 1), (V, T + 1), (0, 0)):
        verts, tris = buffers()
        _, rc_count, rc_emit, totals = _abi_call(hip, u, 12, 11, 10, V_arg, T_arg, verts, tris)
        assert rc_count == 0 and totals.tolist() == [V, T]
        assert rc_emit != 0 and b"counted" in hip.lib().s3d_last_error()
        assert bool((verts == -77.0).all()) and bool((tris == -77).all())
    # the right totals: rows [0, V) / [0, T) are written, the canaries behind them are not
    verts, tris = buffers()
    _, rc_count, rc_emit, _ = _abi_call(hip, u, 12, 11, 10, V, T, verts, tris)
    assert rc_count == 0 and rc_emit == 0
    assert np.array_equal(tris[:T].cpu().numpy(), t_ref) and bool((tris[T:] == -77).all()) and bool((verts[V:] == -77.0).all())
    assert np.abs(verts[:V].cpu().numpy() - v_ref).max() <= 2 * 2.0 ** -23
    # an axis of one point
    for dims in ((1, 11, 120), (12, 1, 110), (132, 10, 1)):
        verts, tris = buffers()
        nbytes, rc_count, rc_emit, totals = _abi_call(hip, u, *dims, V, T, verts, tris)
        assert nbytes == 0 and rc_count != 0 and rc_emit != 0 and totals.tolist() == [0, 0]
        assert bool((verts == -77.0).all()) and bool((tris == -77).all())
    with pytest.raises(RuntimeError):
        hip.MeshBackend.marching_cubes(torch.zeros(1, 4, 4, device="cuda"), 0.0, cases.UNIT)


def test_cpu_tensor_raises(hip):
    with pytest.raises(RuntimeError, match="GPU tensors"):
        hip.MeshBackend.marching_cubes(torch.zeros(4, 4, 4), 0.0, cases.UNIT)


def test_call_under_stream_capture_raises(hip):
    u = torch.from_numpy(cases.random_volume(0, (8, 8, 8))).cuda()
    dummy = torch.zeros(4, device="cuda")
    hip.MeshBackend.marching_cubes(u, 0.0, cases.UNIT)
    torch.cuda.synchronize()
    caught = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dummy.add_(1.0)
        try:
            hip.MeshBackend.marching_cubes(u, 0.0, cases.UNIT)
        except RuntimeError as e:
            caught = e
    assert caught is not None and "captured" in str(caught)


# ------------------------------------------------------------------------------------------------ extract_fields
def test_extract_fields_on_the_device_reproduces_the_reference(hip):
    from nerf.mesh import extract_fields
    g = np.load(os.path.join(GOLDEN, "mesh_fields.npz"))
    args = (torch.from_numpy(g["bound_min"]), torch.from_numpy(g["bound_max"]), int(g["resolution"]))
    u = extract_fields(*args, lambda pts: golden_query(pts.cuda()), S=int(g["S"]))  # host points, device query
    assert u.is_cuda and u.dtype == torch.float32 and np.array_equal(u.cpu().numpy(), g["u"])
    seen = []

    def query(pts):
        seen.append(pts)
        return golden_query(pts)

    u = extract_fields(*args, query, S=int(g["S"]), device=torch.device("cuda"))  # points built on the device
    assert u.is_cuda and all(p.is_cuda for p in seen) and len(seen) == int(g["n_chunks"])
    assert np.array_equal(seen[-1].cpu().numpy(), g["pts_last"]) and np.array_equal(u.cpu().numpy(), g["u"])


# ------------------------------------------------------------------------------------------------ Trainer.save_mesh
def _setup(n_rays=2048, n_batches=8):
    """the scene and model of tests/test_gpu_trainer.py"""
    import bench
    import s3d_hip
    from nerf import network_ff, synthetic as syn
    torch.manual_seed(0)
    model = network_ff.NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda()
    _, bits = syn.lego_like_density_grid(seed=0)
    batches, _ = bench.make_batches(n_batches, n_rays, 0, torch.device("cuda"), s3d_hip.RaymarchingBackend,
                                    torch.from_numpy(bits).cuda(), syn.lego_like_boxes(0))
    return model, batches


def _field(model, resolution, fp16=True):
    from nerf.mesh import extract_fields

    def query(pts):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
            return model.density(pts.cuda())["sigma"]
    aabb = model.aabb_infer.detach().float().cpu()
    return extract_fields(aabb[:3], aabb[3:], resolution, query, device=torch.device("cuda")), aabb.numpy()


def test_save_mesh_end_to_end(hip, tmp_path):
    from nerf.mesh import read_ply
    from nerf.trainer import Trainer
    model, batches = _setup()
    tr = Trainer(model, lr=1e-2, fp16=True)
    for i in range(6):
        tr.train_step(*batches[i])
    u, aabb = _field(model, 48)
    thr = float(u.median())
    assert bool((u > thr).any()), "the field is flat: no surface to export"
    tr.workspace, tr.name, tr.epoch = str(tmp_path), "toy", 3
    path = tr.save_mesh(resolution=48, threshold=thr)
    assert path == os.path.join(str(tmp_path), "meshes", "toy_3.ply") and os.path.exists(path)
    v, t = read_ply(path)
    assert len(v) > 0 and len(t) > 0 and t.min() >= 0 and t.max() < len(v)
    v_ref, t_ref = w.marching_cubes(u.cpu().numpy(), thr, aabb)
    assert np.array_equal(t, t_ref)
    assert v.shape == v_ref.shape and np.abs(v - v_ref).max() <= 2 * 2.0 ** -23 * float(np.abs(aabb).max())
    with pytest.raises(NotImplementedError, match=r"\.ply"):
        tr.save_mesh(save_path=str(tmp_path / "toy.obj"), resolution=8)


def test_save_mesh_leaves_a_captured_step_alone(hip, tmp_path):
    """twins from the same seed on the same batches: one exports between two replayed steps, the other does not"""
    import gc
    from nerf.trainer import GraphedTrainer
    losses = []
    for export in (True, False):
        model, batches = _setup()
        tr = GraphedTrainer(model, 2048, lr=1e-2, fp16=True)
        for i in range(24):
            tr.train_step(*batches[i % len(batches)])
        assert tr.graph is not None
        captures = tr.n_captures
        if export:
            tr.save_mesh(save_path=str(tmp_path / "twin.ply"), resolution=48, threshold=float(_field(model, 48)[0].median()))
        loss = tr.train_step(*batches[24 % len(batches)])
        assert tr.n_captures == captures  # (replayed, not re-captured)
        losses.append(float(loss))
        del tr, model
        gc.collect()
        torch.cuda.synchronize()
    print("loss after the export", losses[0], "twin", losses[1])
    assert losses[0] == losses[1]
