"""GPU: the brush tool's texture painting on the device (csrc/seal.hip: k_seal_color_stats + k_seal_color_image behind
s3d_seal_map_color_image) against the reference's executed outputs and texel indices (tests/golden/seal_texture.npz), against
the build's torch op sequence, under graph capture, and through the teacher renderer, the pretraining set and the graphed Seal
trainer.  Tolerances: 2e-6 (fp32) / 4e-3 (fp16) on colours as for s3d_seal_map_color (tests/test_gpu_seal_loop.py),
1e-4 relative on rendered image and depth as for the brush mapper (tests/test_gpu_seal_tools.py); texel indices exact."""
import numpy as np
import pytest
import torch

from test_seal_texture import CASES, T, texture_config  # noqa: F401
from test_seal_texture import inputs as golden_inputs
from test_seal_loop_golden import G, OPT, golden_network, relmax  # noqa: F401

pytestmark = pytest.mark.gpu


def mapper(T, tag, native=True, **extra):
    from sealnerf import get_seal_mapper
    m = get_seal_mapper(dict(texture_config(T, tag), **extra))
    m.native = native
    return m


def inputs(T, tag="image"):
    """the case's points and colours on the GPU (every kept point for `image`, the first 5,000 for the other option sets)"""
    pts, cols = golden_inputs(T, tag)[:2]
    return torch.from_numpy(pts).cuda(), torch.from_numpy(cols).cuda()


@pytest.mark.parametrize("tag", ["image", "image_hsv", "image_opaque"])
def test_kernel_vs_reference_execution(hip, T, tag):
    """every row moved: the kernel's texel of every kept point is the reference's, colours within 2e-6 (fp32) / 4e-3 (fp16)"""
    m = mapper(T, tag)
    pts, cols = inputs(T, tag)
    want_h, want_w = golden_inputs(T, tag)[2:]
    every = torch.ones(pts.shape[0], dtype=torch.uint8, device="cuda")
    k = m._image_native(pts.device)
    for c, tol in ((cols, 2e-6), (cols.half(), 4e-3)):
        out = torch.empty_like(c)
        texel = torch.full((pts.shape[0], 2), -1, dtype=torch.int32, device="cuda")
        hip.SealBackend.map_color_image(c, pts, every, k["hsv"], k["texture"], k["quad"], k["light"], out, texel_out=texel)
        wrong = int((texel[:, 0].cpu().numpy() != want_h).sum() + (texel[:, 1].cpu().numpy() != want_w).sum())
        err = float(np.abs(out.float().cpu().numpy() - T[f"{tag}_out"]).max())
        print(tag, c.dtype, "texels off:", wrong, "max |kernel - reference|:", err)
        assert wrong == 0
        assert err <= tol
        # the mapper's own route is that call
        assert torch.equal(m.map_color_masked(pts, None, c, every.bool()), out)


def test_rgb_with_texture_takes_the_torch_route_on_the_gpu(hip, T):
    tag = "image_rgb_hsv_light"
    m = mapper(T, tag)
    pts, cols = inputs(T, tag)
    want_h, want_w = golden_inputs(T, tag)[2:]
    idx_h, idx_w = m.texel_indices(pts)
    wrong = int((idx_h.cpu().numpy() != want_h).sum() + (idx_w.cpu().numpy() != want_w).sum())
    out = m.map_color_masked(pts, None, cols, torch.ones(pts.shape[0], dtype=torch.bool, device="cuda"))
    err = float(np.abs(out.cpu().numpy() - T[f"{tag}_out"]).max())
    print(tag, "texels off:", wrong, "max |torch on the GPU - reference|:", err)
    assert wrong == 0 and err <= 2e-6
    # inside an fp16 render the lookup keeps the points' precision (autocast would run its dot products in half)
    with torch.autocast("cuda", dtype=torch.float16):
        ah, aw = m.texel_indices(pts)
    assert torch.equal(ah, idx_h) and torch.equal(aw, idx_w)


@pytest.mark.parametrize("tag", ["image", "image_hsv"])
def test_partial_mask_vs_torch_route(hip, T, tag):
    """`colors[mask] = map_color(points[mask], colors[mask])`: the batch mean is the moved rows' alone; the other rows come
    back bit for bit"""
    m, e = mapper(T, tag), mapper(T, tag, native=False)
    pts, cols = inputs(T)
    part = (torch.rand(pts.shape[0], generator=torch.Generator().manual_seed(3)) < 0.4).cuda()
    a, b = m.map_color_masked(pts, None, cols, part), e.map_color_masked(pts, None, cols, part)
    assert torch.equal(a[~part], cols[~part]) and not torch.equal(a[part], cols[part])
    assert float((a - b).abs().max()) <= 2e-6
    every = torch.ones_like(part)
    assert float((a - m.map_color_masked(pts, None, cols, every))[part].abs().max()) > 1e-4  # (another batch, another mean)
    h = m.map_color_masked(pts, None, cols.half(), part)
    assert h.dtype == torch.float16 and torch.equal(h[~part], cols.half()[~part]) and float((h.float() - b).abs().max()) <= 4e-3
    none = torch.zeros_like(part)
    assert torch.equal(m.map_color_masked(pts, None, cols, none), cols)
    empty = m.map_color_masked(pts[:0], None, cols[:0], part[:0])
    assert empty.shape == (0, 3)


def test_rows_behind_n_valid_are_unwritten(hip, T):
    m = mapper(T, "image_hsv")
    pts, cols = inputs(T)
    part = (torch.rand(pts.shape[0], generator=torch.Generator().manual_seed(4)) < 0.5).cuda()
    k = m._image_native(pts.device)
    n = 1000  # -> rows [0, 1024) (the sample count rounded up to 128, as every per-sample kernel)
    counter = torch.tensor([n], dtype=torch.int32, device="cuda")
    out = torch.full_like(cols, 7.0)
    texel = torch.full((pts.shape[0], 2), -1, dtype=torch.int32, device="cuda")
    hip.SealBackend.map_color_image(cols, pts, part.view(torch.uint8), k["hsv"], k["texture"], k["quad"], k["light"], out,
                                    texel_out=texel, n_valid=counter)
    # the mean is that of the moved rows in front of the count
    want = m.map_color_masked(pts[:1024], None, cols[:1024], part[:1024])
    assert torch.equal(out[:1024], want)
    assert (out[1024:] == 7.0).all() and (texel[1024:] == -1).all() and (texel[:1024][part[:1024]] >= 0).all()
    # the renderer's announcement reaches the kernel through map_color_masked
    with hip.row_limit(counter, pts.shape[0]):
        lim = m.map_color_masked(pts, None, cols, part)
    assert torch.equal(lim[:1024], want)


def test_map_color_under_graph_capture(hip, T):
    m = mapper(T, "image_hsv")
    pts, cols = inputs(T)
    part = (torch.rand(pts.shape[0], generator=torch.Generator().manual_seed(6)) < 0.5).cuda()
    s_pts, s_cols, s_mask = pts.clone(), cols.clone(), part.clone()
    m.map_color_masked(s_pts, None, s_cols, s_mask)  # (warm-up: the texture is uploaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.map_color_masked(s_pts, None, s_cols, s_mask)
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(7)).cuda()
    for p, c, k in ((pts, cols, part), (pts[perm].contiguous(), cols.flip(0).contiguous(), ~part)):
        s_pts.copy_(p)
        s_cols.copy_(c)
        s_mask.copy_(k)
        graph.replay()
        assert torch.equal(out, m.map_color_masked(p, None, c, k))


def dry_textured_brush(T, native=True, **extra):
    return mapper(T, "image_hsv", native=native, **extra)


def test_teacher_render_native_vs_torch_path(hip, T, G):
    """both branches of the teacher's render through a dry brush with a texture: native vs the torch op sequence, 1e-4
    relative on image and depth; and the texture shows"""
    from sealnerf import get_seal_mapper, make_teacher
    ro, rd = torch.from_numpy(G["rays_o"]).cuda(), torch.from_numpy(G["rays_d"]).cuda()
    plain = get_seal_mapper({k: v for k, v in texture_config(T, "image_hsv").items() if k != "imageConfig"})
    res = {}
    for name, m in (("native", dry_textured_brush(T)), ("torch", dry_textured_brush(T, native=False)), ("plain", plain)):
        teacher = golden_network(make_teacher, m, "cuda")
        teacher.hack_bitfield()
        out = {}
        with torch.no_grad():
            teacher.train()
            out["train"] = teacher.render(ro, rd, staged=True, bg_color=None, perturb=False, force_all_rays=True, **OPT)
            teacher.eval()
            out["eval"] = teacher.render(ro, rd, staged=True, bg_color=None, perturb=False, force_all_rays=True, **OPT)
        res[name] = out
    for branch in ("train", "eval"):
        for k in ("image", "depth"):
            r = relmax(res["native"][branch][k].cpu(), res["torch"][branch][k].cpu())
            print(branch, k, "relative max difference:", r)
            assert r < 1e-4, (branch, k)
        assert relmax(res["native"][branch]["image"].cpu(), res["plain"][branch]["image"].cpu()) > 1e-2, branch


def test_graphed_seal_trainer_with_a_textured_brush(hip, T):
    """one fine-tuning step: the teacher's proxy render (texture kernel inside, fp16 autocast) is captured once, later steps
    replay it, and its targets agree with the torch route's within 1e-4 relative on image and depth, as for the brush mapper"""
    from nerf import network, synthetic as syn
    from sealnerf import GraphedSealTrainer, make_student, make_teacher
    kw = dict(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, log2_hashmap_size=15)
    poses = syn.orbit_poses(1, seed=0).cuda()
    r = syn.get_rays(poses, syn.lego_intrinsics(), 800, 800, N=1024, generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    grid, bits = syn.lego_like_density_grid(seed=0)
    got = {}
    for native in (True, False):
        torch.manual_seed(0)
        teacher = make_teacher(network.NeRFNetwork, **kw).cuda()
        student = make_student(network.NeRFNetwork, **kw).cuda()
        for net in (teacher, student):
            net.density_grid.copy_(torch.from_numpy(grid))
            net.density_bitfield.copy_(torch.from_numpy(bits))
            net.iter_density = 100
        student.load_state_dict(teacher.state_dict())
        m = dry_textured_brush(T, native=native)
        teacher.init_mapper(m)
        student.init_mapper(m)
        tr = GraphedSealTrainer(student, teacher, 1024, lr=1e-2, fp16=True, update_extra_interval=16)
        if native:
            loss = float(tr.train_step(ro, rd))
            assert tr.proxy_graph is not None and np.isfinite(loss)
            graph = tr.proxy_graph
            got[native] = (tr.s_gt.clone().cpu(), tr.s_depth.clone().cpu())
            hist = [float(tr.train_step(ro, rd)) for _ in range(24)]
            assert tr.proxy_graph is graph and tr.n_captures >= 1 and np.isfinite(hist).all(), hist
            # the replayed proxy render gives the captured call's targets again (same rays, a teacher that does not train)
            assert torch.equal(tr.s_gt.cpu(), got[native][0]) and torch.equal(tr.s_depth.cpu(), got[native][1])
        else:  # (the torch route reads masks back to the host: it cannot be captured) the same render call, eagerly
            tr.proxy_truth(ro, rd, tr.s_gt, tr.s_depth, teacher_mode="train")
            got[native] = (tr.s_gt.clone().cpu(), tr.s_depth.clone().cpu())
    image, depth = relmax(got[True][0], got[False][0]), relmax(got[True][1], got[False][1])
    print("targets, native vs torch route: relative max difference image", image, "depth", depth)
    assert image < 1e-4 and depth < 1e-4
    assert float(got[True][0].std()) > 0


def test_init_pretraining_with_a_textured_brush(hip, T, G):
    """the local pretraining targets go through map_color (torch ops, constants following the teacher's GPU tensors): they
    equal the texture step applied to the untextured edit's targets, and one pretraining epoch runs"""
    from sealnerf import SealTrainer, get_seal_mapper, make_student, make_teacher
    colors = {}
    for name in ("textured", "plain"):
        cfg = texture_config(T, "image_hsv")
        if name == "plain":
            cfg = {k: v for k, v in cfg.items() if k != "imageConfig"}
        m = get_seal_mapper(cfg)
        teacher = golden_network(make_teacher, m, "cuda")
        student = golden_network(make_student, m, "cuda")
        tr = SealTrainer(student, teacher, lr=1e-2, fp16=False)
        n = tr.init_pretraining(batch_size=1 << 20, lr=0.05, local_point_step=0.01)
        local = tr.pretraining_data["local"]
        assert n > 0 and local["color"].shape == (n, 3) and local["color"].is_cuda and torch.isfinite(local["color"]).all()
        colors[name] = (local["color"].clone(), local["points"].clone(), m)
        if name == "textured":
            assert np.isfinite(float(tr.pretrain_one_epoch()))
    (tex, pts, m), (plain, pts2, _) = colors["textured"], colors["plain"]
    assert torch.equal(pts, pts2) and not torch.equal(tex, plain)
    # a dry brush maps no point: the mapped points are the lattice points; the texture step on the hsv-edited targets
    k = m._image_twin(pts.device, pts.dtype)
    idx_h, idx_w = m.texel_indices(pts)
    from sealnerf.seal_utils import modify_rgb
    a = k["image_mask"][idx_h, idx_w][:, None]
    want = a * modify_rgb(plain, k["image"][idx_h, idx_w], 0.0) + (1 - a) * plain
    assert float((tex - want).abs().max()) <= 2e-6
