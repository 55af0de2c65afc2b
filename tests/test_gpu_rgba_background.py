"""RGBA frames on the reference's per-pixel random background, GPU: s3d_rgba_targets (explicit uniforms against torch, the
device RNG against its numpy restatement, fresh draws on graph replay), the sampler's RGBA form, the renderer's one-launch
route with a per-ray background, graph replay against its eager twin, and a TensoRF step."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_rgba_background import bg_uniforms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "rgba_background.npz"))


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _rgba(shape, seed):
    """seeded RGBA in [0, 1); every fourth alpha exactly 0, every fourth exactly 1"""
    img = _seeded(tuple(shape) + (4,), seed)
    a = img[..., 3].reshape(-1)
    a[0::4] = 0.0
    a[1::4] = 1.0
    return img.contiguous()


def _blend(images, bg):
    """the reference's expression (nerf/utils.py:474) on the CPU, in the frames' dtype"""
    images = images.cpu()
    bg = bg.cpu() if torch.is_tensor(bg) else bg
    return images[..., :3] * images[..., 3:] + bg * (1 - images[..., 3:])


def _targets(hip, images, random_bg=True, **kw):
    gt = torch.full(images.shape[:-1] + (3,), -7.0, device="cuda")
    bg = torch.full_like(gt, -7.0) if random_bg else None
    hip.RaySampleBackend.rgba_targets(images, gt, bg, random_bg=random_bg, **kw)
    torch.cuda.synchronize()
    return gt, bg


# ------------------------------------------------------------------------------------------------ 1. the streaming kernel
@pytest.mark.parametrize("rows", [4096, 100003])
def test_rgba_targets_with_explicit_uniforms_equals_torch(hip, rows):
    img = _rgba((rows,), 1)
    u = _seeded((rows, 3), 2)
    gt, bg = _targets(hip, img.cuda(), u_bg=u.cuda())
    assert torch.equal(bg.cpu(), u) and torch.equal(gt.cpu(), _blend(img, u))
    half = img.half()
    gt, bg = _targets(hip, half.cuda(), u_bg=u.cuda())  # fp16 frames: widened, then the fp32 expression
    assert torch.equal(bg.cpu(), u) and torch.equal(gt.cpu(), _blend(half.float(), u))
    gt, bg = _targets(hip, img.cuda(), random_bg=False)
    assert bg is None and torch.equal(gt.cpu(), _blend(img, 1))


def test_rgba_targets_against_the_reference_fixture(hip, G):
    img = torch.from_numpy(G["images"])
    gt, bg = _targets(hip, img.cuda(), u_bg=torch.from_numpy(G["a_bg_color"]).cuda())
    assert np.array_equal(gt.cpu().numpy(), G["a_gt_rgb"]) and np.array_equal(bg.cpu().numpy(), G["a_bg_color"])
    # fp16 frames: the reference blends in half (four half roundings of at most 2^-12 each on values in [0, 1]: rgb * a, 1 - a,
    # bg * (1 - a), the sum), the kernel in fp32 on the widened frames
    gt, bg = _targets(hip, torch.from_numpy(G["d_images"]).cuda(), u_bg=torch.from_numpy(G["d_bg_color"]).float().cuda())
    err = float((gt.cpu().double() - torch.from_numpy(G["d_gt_rgb"]).double()).abs().max())
    print("fp16 frames: max |fp32 blend - reference's half blend|", err)
    assert err <= 2.0 ** -10
    gt, _ = _targets(hip, torch.from_numpy(G["c_images"]).cuda(), random_bg=False)
    assert np.array_equal(gt.cpu().numpy(), G["c_gt_rgb"])


# ------------------------------------------------------------------------------------------------ 2. device RNG
@pytest.mark.parametrize("seed", [0, 0x9E3779B1])
def test_device_rng_equals_the_restatement_and_advances(hip, seed):
    rows = 4099
    img = _rgba((rows,), 3).cuda()
    for step in (0, 7):
        ctl = torch.tensor([step, 0], dtype=torch.int32, device="cuda")
        gt, bg = _targets(hip, img, seed=seed, ctl=ctl)
        want = bg_uniforms(seed, step, rows)
        assert np.array_equal(bg.cpu().numpy(), want)
        assert torch.equal(gt.cpu(), _blend(img, torch.from_numpy(want)))
        assert ctl.tolist() == [step + 1, 0]
        _targets(hip, img, seed=seed, ctl=ctl)
        assert ctl.tolist() == [step + 2, 0]
    ctl = torch.tensor([5, 0], dtype=torch.int32, device="cuda")
    _targets(hip, img, u_bg=torch.rand(rows, 3, device="cuda"), ctl=ctl)  # explicit uniforms leave ctl alone
    _targets(hip, img, random_bg=False, ctl=ctl)
    assert ctl.tolist() == [5, 0]


def test_captured_launch_draws_a_fresh_background_on_every_replay(hip):
    rows, seed = 4096, 11
    img = _rgba((rows,), 4).cuda()
    ctl = torch.zeros(2, dtype=torch.int32, device="cuda")
    gt, bg = torch.zeros(rows, 3, device="cuda"), torch.zeros(rows, 3, device="cuda")
    hip.RaySampleBackend.rgba_targets(img, gt, bg, seed=seed, ctl=ctl)  # warm-up: step 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.RaySampleBackend.rgba_targets(img, gt, bg, seed=seed, ctl=ctl)
    seen = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        seen.append(bg.cpu().numpy().copy())
        assert np.array_equal(seen[-1], bg_uniforms(seed, 1 + k, rows)), k
        assert torch.equal(gt.cpu(), _blend(img, bg))
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[2])
    assert ctl.tolist() == [4, 0]


# ------------------------------------------------------------------------------------------------ 3. the sampler
def _sampler_pair(hip, dtype, with_map, B=2, H=600, W=800, N=4096):
    from nerf import synthetic as syn
    from test_gpu_error_map import _peaked_map
    poses = syn.orbit_poses(B, seed=0).cuda()
    intr = syn.lego_intrinsics(H, W)
    img4 = _rgba((B, H, W), 5).to(dtype).cuda()
    img3 = img4[..., :3].contiguous()
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    u_bg = _seeded((B, N, 3), 6).cuda()
    kw = {}
    emap = None
    if with_map:
        emap = _peaked_map(B, 2).cuda()
        kw = dict(u_keys=(1.0 - _seeded((B, 128 * 128), 7)).cuda(), u_fine=_seeded((B, N, 2), 8).cuda())
    res = []
    for rgba in (False, True):
        o = {k: torch.full((B, N, 3), -7.0, device="cuda") for k in ("rays_o", "rays_d", "gt", "bg")}
        inds, coarse = (torch.full((B, N), -1, dtype=torch.int64, device="cuda") for _ in range(2))
        ctl = torch.tensor([3, 0], dtype=torch.int32, device="cuda")
        extra = dict(rgba=True, u_bg=u_bg, out_bg=o["bg"]) if rgba else {}
        hip.RaySampleBackend.sample_train_rays(emap, idx, N, H, W, poses, intr, o["rays_o"], o["rays_d"], inds, coarse if with_map else None,
                                               images=img4 if rgba else img3, gt=o["gt"], seed=9, ctl=ctl, **kw, **extra)
        torch.cuda.synchronize()
        res.append((o, inds, coarse, ctl))
    return img4, u_bg, res


@pytest.mark.parametrize("with_map", [True, False], ids=["error_map", "uniform"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_sampler_gathers_and_blends_rgba_without_changing_the_draw(hip, dtype, with_map):
    img4, u_bg, ((o3, inds3, coarse3, ctl3), (o4, inds4, coarse4, ctl4)) = _sampler_pair(hip, dtype, with_map)
    B, N = inds3.shape
    assert int(inds3.min()) >= 0
    assert torch.equal(inds3, inds4) and torch.equal(coarse3, coarse4) and ctl3.tolist() == ctl4.tolist()
    assert torch.equal(o3["rays_o"], o4["rays_o"]) and torch.equal(o3["rays_d"], o4["rays_d"])
    px = torch.gather(img4.view(B, -1, 4), 1, torch.stack(4 * [inds4], -1)).contiguous()
    assert torch.equal(o3["gt"], px[..., :3].float())  # (the 3-channel call: the gathered colours)
    gt, bg = _targets(hip, px, u_bg=u_bg)
    assert torch.equal(o4["gt"], gt) and torch.equal(o4["bg"], bg) and torch.equal(bg, u_bg)
    assert torch.equal(o4["gt"].cpu(), _blend(px.float(), u_bg))


def _dataset(channels, fp16=False, error_map=True, N=1024, seed=13, **kw):
    from nerf import synthetic as syn
    from nerf.provider import NeRFDataset
    imgs = _rgba((2, 400, 400), 5)[..., :channels].contiguous()
    return NeRFDataset(imgs, syn.orbit_poses(2, seed=0), syn.lego_intrinsics(400, 400), num_rays=N, error_map=error_map, device="cuda",
                       seed=seed, fp16=fp16, **kw)


@pytest.mark.parametrize("error_map", [True, False], ids=["error_map", "uniform"])
def test_dataset_sample_blends_rgba_frames_on_the_device_rng(hip, error_map):
    ds = _dataset(4, fp16=True, error_map=error_map)
    for step in range(2):
        b = ds.sample([1, 0])
        assert b["images"].shape == (2, 1024, 3) and b["bg_color"].shape == (2, 1024, 3) and b["images"].dtype == torch.float32
        assert np.array_equal(b["bg_color"].cpu().numpy().reshape(-1, 3), bg_uniforms(13, step, 2 * 1024))  # row = b * N + n
        px = torch.stack([ds.images[i].view(-1, 4)[b["inds"][r]] for r, i in enumerate((1, 0))])
        assert torch.equal(b["images"].cpu(), _blend(px.float(), b["bg_color"]))
    white = _dataset(4, error_map=error_map, random_bg=False)
    b = white.sample([0])
    assert "bg_color" not in b
    assert torch.equal(b["images"].cpu(), _blend(white.images[0].view(-1, 4)[b["inds"][0]][None], 1))


def test_three_channel_frames_sample_as_before(hip):
    ds = _dataset(3)
    b = ds.sample([1])
    assert set(b) == {"H", "W", "rays_o", "rays_d", "inds", "images", "index", "inds_coarse"}
    o = {k: torch.empty(1, 1024, 3, device="cuda") for k in ("rays_o", "rays_d", "gt")}
    inds, coarse = (torch.empty(1, 1024, dtype=torch.int64, device="cuda") for _ in range(2))
    hip.RaySampleBackend.sample_train_rays(ds.error_map, torch.tensor([1], device="cuda"), 1024, 400, 400, ds.poses, ds.intrinsics,
                                           o["rays_o"], o["rays_d"], inds, coarse, images=ds.images, gt=o["gt"], seed=13,
                                           ctl=torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert torch.equal(b["inds"], inds) and torch.equal(b["inds_coarse"], coarse) and torch.equal(b["images"], o["gt"])
    assert torch.equal(b["rays_o"], o["rays_o"]) and torch.equal(b["rays_d"], o["rays_d"])


# ------------------------------------------------------------------------------------------------ 4. the renderer's route
def test_loss_launch_without_grad_bg_equals_the_launch_with_it(hip):
    from test_gpu_background import _toy_batch
    sig, rgb, deltas, rays, gt, bg = _toy_batch()
    M, N = sig.shape[0], rays.shape[0]
    scale = torch.full((), 1024.0, device="cuda")
    res = []
    for with_grad in (True, False):
        ws, depth, image = torch.empty(N, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, 3, device="cuda")
        gs, gc, loss = torch.zeros(M, device="cuda"), torch.zeros(M, 3, device="cuda"), torch.empty((), device="cuda")
        gb = torch.empty(N, 3, device="cuda") if with_grad else None
        hip.RaymarchingBackend.composite_rays_train_loss_bg(sig, rgb, deltas, rays, M, N, 1e-4, gt, bg, scale, ws, depth, image, gs, gc, gb,
                                                            loss, torch.empty(4 * N, device="cuda"))
        torch.cuda.synchronize()
        res.append((loss, ws, depth, image, gs, gc))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_fused_loss_with_a_random_background_equals_unfused(hip):
    """raymarching.composite_rays_train_loss_bg with a background that takes no gradient, against composite_rays_train, the
    torch blend and F.mse_loss: the tolerances of tests/test_gpu_background.py::test_fused_per_ray_background_loss_equals_unfused"""
    import raymarching
    from test_gpu_background import _toy_batch
    sig, rgb, deltas, rays, gt, bg = _toy_batch()
    scale = torch.full((), 1024.0, device="cuda")
    s1, c1 = sig.clone().requires_grad_(), rgb.clone().requires_grad_()
    loss, ws, depth, image = raymarching.composite_rays_train_loss_bg(s1, c1, deltas, rays, 1e-4, gt, bg, scale)
    loss.backward(scale)
    s2, c2 = sig.clone().requires_grad_(), rgb.clone().requires_grad_()
    ws2, _, im2 = raymarching.composite_rays_train(s2, c2, deltas, rays, 1e-4)
    loss2 = torch.nn.functional.mse_loss(im2 + (1 - ws2).unsqueeze(-1) * bg, gt)
    loss2.backward(scale)
    print("loss", float(loss), float(loss2), "max |d grad_rgbs|", float((c1.grad - c2.grad).abs().max()),
          "max |d grad_sigmas|", float((s1.grad - s2.grad).abs().max()))
    assert bg.grad is None
    torch.testing.assert_close(loss, loss2, rtol=1e-5, atol=0)
    torch.testing.assert_close(image + (1 - ws).unsqueeze(-1) * bg, im2 + (1 - ws2).unsqueeze(-1) * bg, rtol=0, atol=0)
    torch.testing.assert_close(c1.grad, c2.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(s1.grad, s2.grad, rtol=1e-4, atol=1e-5)


def _ngp(seed=0):
    from test_gpu_error_map import _ngp as make
    return make(seed)


@pytest.fixture()
def cpu_random(monkeypatch):
    """rand / rand_like inside the marcher and the renderer drawn from the CPU generator, as the fixture's were"""
    import nerf.renderer as rend
    import raymarching.raymarching as rm
    from test_gpu_golden import _CpuRandom
    proxy = _CpuRandom()
    monkeypatch.setattr(rm, "torch", proxy)
    monkeypatch.setattr(rend, "torch", proxy)
    return proxy


def test_eager_trainer_takes_the_one_launch_form_with_a_per_ray_background(hip, monkeypatch):
    from nerf.trainer import Trainer
    ds = _dataset(4, N=4096)
    res = {}
    for fused in (True, False):
        net = _ngp()
        net.mean_count = 4096 * 40
        tr = Trainer(net, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
        tr.fused_losses = fused
        tr.global_step = 1
        tr.error_map = torch.ones_like(ds.error_map)
        ds._ctl = None  # (both runs draw the batch of step 0)
        b = ds.sample([0])
        seen = {}
        render = net.render
        monkeypatch.setattr(net, "render", lambda *a, **k: seen.setdefault("out", render(*a, **k)))
        torch.manual_seed(3)
        loss = tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], bg_color=b["bg_color"][0], index=b["index"],
                             inds_coarse=b["inds_coarse"])
        torch.cuda.synchronize()
        out = seen["out"]
        assert out["premultiplied"] and out["bg_color"].shape == (4096, 3) and ("loss" in out) == fused
        res[fused] = (float(loss), tr.error_map.clone())
    print("loss fused / unfused", res[True][0], res[False][0])
    assert np.isfinite(res[True][0]) and abs(res[True][0] - res[False][0]) <= 1e-5 * abs(res[False][0])
    assert float((res[True][1] != 1).sum()) == 4096
    torch.testing.assert_close(res[True][1], res[False][1], rtol=1e-6, atol=1e-7)


def test_one_launch_step_against_the_reference_fixture(hip, G, cpu_random):
    """fixture (a) on the HIP path in fp32 through the one-launch compositing + criterion with the fixture's background:
    loss 1e-5, every gradient within 2e-4 of its largest element (tests/test_gpu_golden.py's train-step test)"""
    from nerf.trainer import rgba_targets
    from test_gpu_golden import _check_grads, _golden_student, _relmax
    net = _golden_student()
    net.mean_count = int(G["mean_count"])
    net.train()
    torch.manual_seed(int(G["seed"]))
    gt, bg = rgba_targets(torch.from_numpy(G["images"]))  # (the CPU generator's draw, then the marcher's jitter: cpu_random)
    assert np.array_equal(bg.numpy(), G["a_bg_color"])
    one = torch.ones((), device="cuda")
    out = net.render(torch.from_numpy(G["a_rays_o"])[0].cuda(), torch.from_numpy(G["a_rays_d"])[0].cuda(), bg_color=bg[0].cuda(),
                     perturb=True, force_all_rays=False, defer_background=True, fused_loss=dict(gt=gt[0].cuda(), expected_grad=one),
                     max_steps=1024, dt_gamma=0, T_thresh=1e-4)
    assert "loss" in out and out["premultiplied"]
    assert np.array_equal(net.step_counter[0].cpu().numpy(), G["a_counter"]), "ray compaction / sample count"
    print("loss", float(out["loss"]), "reference", float(G["a_loss"]))
    assert abs(float(out["loss"]) - float(G["a_loss"])) <= 1e-5 * float(G["a_loss"])
    pred = out["image"] + (1 - out["weights_sum"]).unsqueeze(-1) * out["bg_color"]
    assert _relmax(pred, G["a_pred_rgb"][0]) < 1e-4
    net.zero_grad()
    out["loss"].backward(one)
    print("worst gradient error / largest element", _check_grads(net, G, "a_grad"))


# ------------------------------------------------------------------------------------------------ 5. graph replay
def _graphed_run(mode, steps=24, error_map=True, batches=None):
    """mode "replay": sample(out=static_batch()) + replayed steps (the batches are recorded); "eager": every step re-captured
    (the capture's eager step: same body on the stream) on the recorded batches, staged; "staged": replayed, staged"""
    from nerf.trainer import GraphedTrainer
    torch.manual_seed(0)
    net = _ngp()
    tr = GraphedTrainer(net, 4096, lr=1e-2, fp16=True, update_extra_interval=16)
    tr.global_step = 1
    net.mean_count = 4096 * 40
    ds = _dataset(4, fp16=True, N=4096, error_map=error_map)
    if error_map:
        tr.error_map = ds.error_map
    rec = []
    for k in range(steps):
        if mode == "replay":
            b = ds.sample([k % 2], out=tr.static_batch())
            assert b["bg_color"].data_ptr() == tr.s_bg.data_ptr() and b["images"].data_ptr() == tr.s_gt.data_ptr()
            rec.append({n: b[n].clone() for n in ("rays_o", "rays_d", "images", "bg_color", "index", "inds_coarse") if n in b})
        else:
            b = batches[k]
            if mode == "eager":
                tr.graph = None
        kw = dict(index=b["index"], inds_coarse=b["inds_coarse"]) if error_map else {}
        if tr.global_step % 16 == 0:
            torch.manual_seed(100)  # (the occupancy update of this step draws its cells from torch's generator)
        tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], bg_color=b["bg_color"][0], **kw)
    torch.cuda.synchronize()
    return tr, [p.detach().clone() for p in net.parameters()], ds.error_map, rec


@pytest.mark.parametrize("error_map", [False, True], ids=["plain", "error_map"])
def test_graph_replay_on_rgba_frames_and_its_eager_twin_end_alike(hip, error_map):
    """24 steps across one occupancy update (step 16).  Tolerance as test_graphed_replay_and_eager_twin_end_with_the_same_map:
    the two runs' gradients are summed by fp16 atomics in different orders; a missing, doubled or wrongly blended update moves
    a parameter by ~lr = 1e-2."""
    tr_r, p_r, m_r, rec = _graphed_run("replay", error_map=error_map)
    assert tr_r._graph_bg and 1 <= tr_r.n_captures <= 2  # (the occupancy update may move the sample budget once)
    tr_e, p_e, m_e, _ = _graphed_run("eager", error_map=error_map, batches=rec)
    assert tr_e.n_captures >= 8
    worst = max(float((a - b).abs().max()) for a, b in zip(p_r, p_e))
    print("max |parameter difference| replay vs eager", worst)
    for a, b in zip(p_r, p_e):
        assert torch.isfinite(a).all()
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3)
    if error_map:
        assert float((m_r != 1).sum()) > 0
        torch.testing.assert_close(m_r, m_e, rtol=1e-3, atol=1e-3)
    # the staged form (a bg_color tensor that is not s_bg) against the in-place form
    tr_s, p_s, m_s, _ = _graphed_run("staged", error_map=error_map, batches=rec)
    assert 1 <= tr_s.n_captures <= 2
    for a, b in zip(p_r, p_s):
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3)


def test_switching_to_a_constant_background_recaptures_once(hip):
    from nerf.trainer import GraphedTrainer
    net = _ngp()
    tr = GraphedTrainer(net, 4096, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
    tr.global_step = 1
    net.mean_count = 4096 * 40
    ds = _dataset(4, N=4096, error_map=False)
    for k in range(3):
        b = ds.sample([k % 2], out=tr.static_batch())
        tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], bg_color=b["bg_color"][0])
    assert tr.n_captures == 1
    for k in range(3):
        loss = tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], bg_color=1)
    torch.cuda.synchronize()
    assert tr.n_captures == 2 and not tr._graph_bg and bool(torch.isfinite(loss))
    with pytest.raises(ValueError, match="background"):
        tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], bg_color=0.5)
    with pytest.raises(ValueError, match="RGBA"):
        tr.train_step(b["rays_o"][0], b["rays_d"][0], torch.zeros(4096, 4, device="cuda"))


# ------------------------------------------------------------------------------------------------ 6. TensoRF
def test_tensorf_step_with_a_per_ray_background_matches_its_unfused_twin(hip, monkeypatch):
    """loss 1e-5, every gradient within 2e-4 of its largest element: the tolerances of
    tests/test_gpu_configs.py::test_tensorf_train_step_with_l1_term_vs_the_reference_trainer"""
    from nerf import synthetic as syn
    from tensoRF import network as trf
    from tensoRF.utils import Trainer
    ds = _dataset(4, N=512, error_map=False)
    b = ds.sample([0])
    res = {}
    for fused in (True, False):
        torch.manual_seed(0)  # (the network of test_tensorf_vm48_step_on_gpu, the same initial values for both twins)
        net = trf.NeRFNetwork(resolution=[128] * 3, bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10).cuda()
        grid, bits = syn.lego_like_density_grid(seed=0)
        net.density_grid.copy_(torch.from_numpy(grid))
        net.density_bitfield.copy_(torch.from_numpy(bits))
        net.iter_density = 100
        net.mean_count = 512 * 64
        tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=1e-4, fp16=True, update_extra_interval=10 ** 9)
        tr.fused_losses = fused
        tr.global_step = 1
        seen = {}
        monkeypatch.setattr(tr, "_reduce_and_step", lambda seen=seen, net=net: seen.update(
            {k: (p.grad if p.grad is not None else p._s3d.grad).detach().float().clone() for k, p in net.named_parameters()}))
        torch.manual_seed(5)
        loss = tr.train_step(b["rays_o"][0], b["rays_d"][0], b["images"][0], bg_color=b["bg_color"][0])
        torch.cuda.synchronize()
        res[fused] = (float(loss), seen)
    print("loss fused / unfused", res[True][0], res[False][0])
    assert np.isfinite(res[True][0]) and abs(res[True][0] - res[False][0]) <= 1e-5 * abs(res[False][0])
    for k, g in res[True][1].items():
        want = res[False][1][k]
        assert float((g - want).abs().max()) <= 2e-4 * float(want.abs().max()) + 1e-9, k
