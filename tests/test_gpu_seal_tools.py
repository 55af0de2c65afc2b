"""GPU: the brush and anchor tools' device kernels (csrc/seal.hip: k_seal_brush_map, k_seal_anchor_flag + k_seal_anchor_map)
against the reference's executed outputs (tests/golden/seal_tools.npz) and the build's torch op sequence, under graph capture,
and through the teacher renderer and the Seal trainers."""
import numpy as np
import pytest
import torch

from test_seal_tools import ANCHOR, BRUSH, S, batches, config  # noqa: F401
from test_seal_loop_golden import G, OPT, golden_network, relmax  # noqa: F401

pytestmark = pytest.mark.gpu


def mapper(S, tag, native=True, **extra):
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(dict(config(S, tag), **extra))
    m.native = native
    return m


def around(m, n, seed):
    """n points, half of them around the edit region, a few with a zero coordinate"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, 3, generator=g) * 1.2 - 0.6
    b = m.map_data["map_bound"].reshape(-1, 2, 3).cpu()
    lo, hi = b[:, 0].min(0).values - 0.03, b[:, 1].max(0).values + 0.03
    p[n // 2:] = lo + (hi - lo) * torch.rand(n - n // 2, 3, generator=g)
    p[n // 2:n // 2 + 64, 0] = 0.0
    return p.cuda()


def agree(native, eager, max_mask_diff=0, atol=1e-5):
    """masks equal but for at most `max_mask_diff` rows right at a threshold (the two paths round differently), points within
    `atol` where the masks agree"""
    (p, _, m), (pe, _, me) = native, eager
    diff = int((m != me).sum())
    assert diff <= max_mask_diff, diff
    same = m == me
    assert (p[same] - pe[same]).abs().max().item() <= atol


@pytest.mark.parametrize("tag", BRUSH + ANCHOR)
def test_kernel_vs_reference_execution(hip, S, tag):
    """masks exact, mapped points within 1e-5, other rows untouched.  (The brush's border distance is a running minimum of
    squared differences here, torch.cdist's matmul form in the reference: the two round differently, hence no bit match.)"""
    m = mapper(S, tag)
    for b in batches(S, tag):
        pts = torch.from_numpy(S[f"{tag}_b{b}_points"]).cuda()
        for dirs in (None, torch.randn_like(pts)):
            p, d, mask = m.map_to_origin(pts, dirs)
            assert d is dirs
            want = torch.from_numpy(S[f"{tag}_b{b}_mask"])
            assert torch.equal(mask.cpu(), want), (tag, b)
            assert torch.equal(p[~mask], pts[~mask])
            if want.any():
                assert np.abs(p[mask].cpu().numpy() - S[f"{tag}_b{b}_mapped"]).max() <= 1e-5


@pytest.mark.parametrize("tag", ["brush_linear1", "brush_linear2", "brush_dry", "anchor_mixed", "anchor_scale", "anchor_axis"])
def test_kernel_vs_torch_path_random_points(hip, S, tag):
    m, e = mapper(S, tag), mapper(S, tag, native=False)
    pts = around(m, 200000, 7)
    agree(m.map_to_origin(pts), e.map_to_origin(pts), max_mask_diff=2)
    assert int(m.map_to_origin(pts)[2].sum()) > 100


def test_brush_border_larger_than_one_lds_tile(hip, S):
    """1,000 border points (4 tiles of 256) put in directly; every masked point's distance walks all tiles"""
    m, e = mapper(S, "brush_linear2"), mapper(S, "brush_linear2", native=False)
    g = torch.Generator().manual_seed(3)
    ne, c = m.map_data["normal_expand"], m.map_data["center"]
    q = c + (torch.rand(1000, 3, generator=g) - 0.5) * 0.6
    border = q - ((q - c) @ ne / (ne @ ne))[:, None] * ne  # in the plane
    for x in (m, e):
        x.map_data["border_points"] = border.clone()
    m._dev.clear()
    pts = around(m, 200000, 8)
    # (torch.cdist on the GPU takes its matmul form |a|^2 + |b|^2 - 2ab at this size: ~3e-5 off in the distance, which moves a
    #  point by up to |normal_expand| / attenuationDistance = 2/3 of that; the kernel's direct differences do not lose it)
    agree(m.map_to_origin(pts), e.map_to_origin(pts), max_mask_diff=2, atol=5e-5)
    # the last tile matters: drop it and the distances change
    m.map_data["border_points"] = border[:768].clone()
    m._dev.clear()
    p768, _, _ = m.map_to_origin(pts)
    assert not torch.equal(p768, e.map_to_origin(pts)[0])


@pytest.mark.parametrize("tag", ["brush_linear2", "anchor_mixed"])
def test_rows_behind_n_valid_are_untouched(hip, S, tag):
    import s3d_hip
    m = mapper(S, tag)
    pts = around(m, 5000, 9)
    full_p, _, full_m = m.map_to_origin(pts)
    n = 1000  # -> rows [0, 1024) (the sample count rounded up to 128, as every per-sample kernel)
    counter = torch.tensor([n], dtype=torch.int32, device="cuda")
    out = torch.full_like(pts, 7.0)
    mask = torch.full((pts.shape[0],), 2, dtype=torch.uint8, device="cuda")
    dev = m._device_constants(pts.device)
    if tag.startswith("brush"):
        s3d_hip.SealBackend.brush_map(pts, dev, out, mask, counter)
    else:
        s3d_hip.SealBackend.anchor_map(pts, dev, out, mask, torch.empty(1, dtype=torch.int32, device="cuda"), counter)
    assert torch.equal(out[:1024], full_p[:1024]) and torch.equal(mask[:1024].bool(), full_m[:1024])
    assert (out[1024:] == 7.0).all() and (mask[1024:] == 2).all()


def test_anchor_early_exit_batches_on_device(hip, S):
    m, e = mapper(S, "anchor_axis"), mapper(S, "anchor_axis", native=False)
    for b in ("0", "1"):
        pts = torch.from_numpy(S[f"anchor_axis_b{b}_points"]).cuda()
        p, _, mask = m.map_to_origin(pts)
        pe, _, me = e.map_to_origin(pts)
        assert torch.equal(mask, me) and (p - pe).abs().max().item() <= 1e-5
        assert bool(mask[:-1].all()) == (b == "1") and bool(mask.any()) == (b == "1")


@pytest.mark.parametrize("tag", ["brush_linear2", "anchor_axis"])
def test_map_to_origin_under_graph_capture(hip, S, tag):
    m = mapper(S, tag)
    a = around(m, 65536, 11)
    static = a.clone()
    m.map_to_origin(static)  # (warm-up: the constants are uploaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_p, _, out_m = m.map_to_origin(static)
    inputs = [around(m, 65536, 12)]
    if tag == "anchor_axis":  # both decisions of the batch-wide flag, replayed
        inputs.append(torch.from_numpy(np.resize(S["anchor_axis_b0_points"], (65536, 3))).cuda())
    for x in inputs:
        static.copy_(x)
        graph.replay()
        p, _, mk = m.map_to_origin(x)
        assert torch.equal(out_p, p) and torch.equal(out_m, mk)
    if tag == "anchor_axis":
        assert not out_m.any()


TOOLS = ["brush_linear1", "anchor_mixed"]


@pytest.mark.parametrize("tag", TOOLS)
def test_teacher_render_native_vs_torch_path(hip, S, G, tag):
    """SealNeRF/renderer.py:254-418 through a brush / anchor edit: the training branch and the inference loop, native mapper
    vs the torch op sequence, 1e-4 relative on image and depth"""
    from sealnerf import make_teacher
    ro, rd = torch.from_numpy(G["rays_o"]).cuda(), torch.from_numpy(G["rays_d"]).cuda()
    res = {}
    for native in (True, False):
        teacher = golden_network(make_teacher, mapper(S, tag, native=native, hsv=[0.1, 0.0, -0.05]), "cuda")
        teacher.hack_bitfield()
        out = {}
        with torch.no_grad():
            teacher.train()
            out["train"] = teacher.render(ro, rd, staged=True, bg_color=None, perturb=False, force_all_rays=True, **OPT)
            teacher.eval()
            out["eval"] = teacher.render(ro, rd, staged=True, bg_color=None, perturb=False, force_all_rays=True, **OPT)
        res[native] = out
    for branch in ("train", "eval"):
        for k in ("image", "depth"):
            assert relmax(res[True][branch][k].cpu(), res[False][branch][k].cpu()) < 1e-4, (branch, k)


@pytest.mark.parametrize("tag", TOOLS)
def test_init_pretraining_and_one_epoch(hip, S, G, tag):
    from sealnerf import SealTrainer, make_student, make_teacher, sample_points
    m = mapper(S, tag)
    teacher = golden_network(make_teacher, m, "cuda")
    student = golden_network(make_student, m, "cuda")
    tr = SealTrainer(student, teacher, lr=1e-2, fp16=False)
    n = tr.init_pretraining(batch_size=1 << 20, lr=0.05, local_point_step=0.01)
    lattice = sample_points(m.map_data["force_fill_bound"], 0.01, 45)[0].shape[0]
    if tag.startswith("anchor"):
        assert n == lattice  # `map_source`: every local lattice point is kept
    else:
        assert 0 < n < lattice
    assert np.isfinite(float(tr.pretrain_one_epoch()))


def test_graphed_seal_trainer_with_a_brush_edit(hip, S):
    from nerf import network, synthetic as syn
    from sealnerf import GraphedSealTrainer, make_student, make_teacher
    torch.manual_seed(0)
    kw = dict(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, log2_hashmap_size=15)
    teacher = make_teacher(network.NeRFNetwork, **kw).cuda()
    student = make_student(network.NeRFNetwork, **kw).cuda()
    grid, bits = syn.lego_like_density_grid(seed=0)
    for net in (teacher, student):
        net.density_grid.copy_(torch.from_numpy(grid))
        net.density_bitfield.copy_(torch.from_numpy(bits))
        net.iter_density = 100
    student.load_state_dict(teacher.state_dict())
    m = mapper(S, "brush_linear1", rgb=[0.8, 0.2, 0.1])
    teacher.init_mapper(m)
    student.init_mapper(m)
    tr = GraphedSealTrainer(student, teacher, 1024, lr=1e-2, fp16=True, update_extra_interval=16)
    poses = syn.orbit_poses(1, seed=0).cuda()
    r = syn.get_rays(poses, syn.lego_intrinsics(), 800, 800, N=1024, generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    hist = [float(tr.train_step(ro, rd)) for _ in range(40)]
    assert tr.n_captures >= 1 and np.isfinite(hist).all(), hist
