"""The NGP background model on the MI355X: the fused kernels (csrc/background.hip) against the reference fixture
(tests/golden/background.npz) and against the network's own torch path, the per-ray-background loss launch against the unfused
sequence, and the background model inside the eager and graph-replayed training steps, Seal fine-tuning and rendering."""
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import REPO
from test_seal_tools import S, config  # noqa: F401

pytestmark = pytest.mark.gpu

GOLD = os.path.join(REPO, "tests", "golden", "background.npz")
NET = dict(bound=1, cuda_ray=True, log2_hashmap_size=14, bg_radius=32)


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _net(seeded=True, **kw):
    from nerf.network import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork(**dict(NET, **kw))
    if seeded:
        for k, p in net.named_parameters():
            p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
    return net.cuda()


class _Count:
    """counts the fused background launches (NgpHeadBackend.background_forward / _backward) while active"""

    def __init__(self, monkeypatch, hip):
        self.fwd = self.bwd = 0
        H = hip.NgpHeadBackend
        f, b = H.background_forward, H.background_backward

        def fwd(*a, **k):
            self.fwd += 1
            return f(*a, **k)

        def bwd(*a, **k):
            self.bwd += 1
            return b(*a, **k)
        monkeypatch.setattr(H, "background_forward", staticmethod(fwd))
        monkeypatch.setattr(H, "background_backward", staticmethod(bwd))


def _bg(net, sph, rd, fused):
    net.fused_background = fused
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            return net.background(sph, rd)
    finally:
        net.fused_background = True


def test_fused_forward_backward_vs_fixture_and_torch_path(hip, monkeypatch):
    d = np.load(GOLD)
    net = _net()
    cnt = _Count(monkeypatch, hip)
    sph, rd = torch.from_numpy(d["bg_sph"]).cuda(), torch.from_numpy(d["bg_rays_d"]).cuda()
    g = torch.from_numpy(d["bg_grad_rgb"]).cuda()
    outs = {}
    for fused in (True, False):
        net.zero_grad()
        rgb = _bg(net, sph, rd, fused)
        rgb.float().backward(g)
        outs[fused] = (rgb.detach().float(), net.bg_net[0].weight.grad.clone(), net.bg_net[1].weight.grad.clone(),
                       net.encoder_bg.embeddings.grad.float().clone())
        assert (cnt.fwd, cnt.bwd) == (1, 1), "the fused path ran exactly once, the torch path not at all"
    rgb, gw0, gw1, gt = outs[True]
    # against the torch op sequence under the same autocast: same fp16 roundings, only GEMM summation orders differ ->
    # at most one fp16 ulp of a unit, 1e-3 on the colour, 1 % of the largest weight / table gradient
    r2, w0b, w1b, tb = outs[False]
    assert (rgb - r2).abs().max().item() <= 1e-3
    for a, b in ((gw0, w0b), (gw1, w1b), (gt, tb)):
        assert (a - b).abs().max().item() <= 1e-2 * b.abs().max().item() + 1e-4
    # fp16 tolerance against the reference's fp32 run: the colour per element; the gradients as a whole (relative norm of the
    # difference) — a hidden unit within an fp16 rounding of zero switches its ReLU in one run and not in the other, which moves
    # a few single weight-gradient entries by far more than a rounding
    torch.testing.assert_close(rgb.cpu(), torch.from_numpy(d["bg_rgb"]), rtol=0, atol=4e-3)
    rows = torch.from_numpy(d["bg_grad_encoder_bg_embeddings_rows"]).cuda()
    for a, key in ((gw0, "bg_grad_bg_net_0_weight"), (gw1, "bg_grad_bg_net_1_weight"), (gt[rows], "bg_grad_encoder_bg_embeddings_at_rows")):
        ref = torch.from_numpy(d[key]).double()
        assert ((a.cpu().double() - ref).norm() / ref.norm()).item() < 2e-2, key


def test_grid_features_bit_equal_to_grid_encoder(hip):
    net = _net()
    enc = net.encoder_bg
    N = 5000
    sph = (_seeded((N, 2), 3, -1.05, 1.05)).cuda()
    rd = torch.nn.functional.normalize(_seeded((N, 3), 4, -1, 1), dim=-1).cuda()
    S = float(np.log2(enc.per_level_scale))
    for dt in (torch.float32, torch.float16):
        table = enc.embeddings.detach().to(dt).contiguous()
        feat = torch.empty(4, N, 2, dtype=dt, device="cuda")
        rgb = torch.empty(N, 3, device="cuda")
        hip.NgpHeadBackend.background_forward(sph, rd, table, enc.offsets, S, enc.base_resolution, net.bg_net[0].weight.detach(),
                                              net.bg_net[1].weight.detach(), rgb, feat)
        ref = torch.empty(4, N, 2, dtype=dt, device="cuda")
        hip.GridBackend.grid_encode_forward(sph, table, enc.offsets, ref, N, 2, 2, 4, S, enc.base_resolution, None, 0, False, 0,
                                            bound=1.0)
        torch.cuda.synchronize()
        assert torch.equal(feat, ref), dt


def _toy_batch(N=512, k=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    M = N * k
    sig = (torch.rand(M, generator=g) * 20).cuda()
    rgb = torch.rand(M, 3, generator=g).cuda()
    deltas = torch.stack([torch.full((M,), 0.01), torch.rand(M, generator=g)], 1).cuda().contiguous()
    rays = torch.stack([torch.arange(N), torch.arange(N) * k, torch.full((N,), k)], 1).int().cuda().contiguous()
    gt = torch.rand(N, 3, generator=g).cuda()
    bg = torch.rand(N, 3, generator=g).cuda()
    return sig, rgb, deltas, rays, gt, bg


def test_fused_per_ray_background_loss_equals_unfused(hip):
    import raymarching
    sig, rgb, deltas, rays, gt, bg = _toy_batch()
    scale = torch.full((), 1024.0, device="cuda")
    s1, c1, b1 = sig.clone().requires_grad_(), rgb.clone().requires_grad_(), bg.clone().requires_grad_()
    loss, ws, depth, image = raymarching.composite_rays_train_loss_bg(s1, c1, deltas, rays, 1e-4, gt, b1, scale)
    loss.backward(scale)
    s2, c2, b2 = sig.clone().requires_grad_(), rgb.clone().requires_grad_(), bg.clone().requires_grad_()
    ws2, _, im2 = raymarching.composite_rays_train(s2, c2, deltas, rays, 1e-4)
    loss2 = torch.nn.functional.mse_loss(im2 + (1 - ws2).unsqueeze(-1) * b2, gt)
    loss2.backward(scale)
    torch.testing.assert_close(loss, loss2, rtol=1e-5, atol=0)
    torch.testing.assert_close(image + (1 - ws).unsqueeze(-1) * bg, im2 + (1 - ws2).unsqueeze(-1) * bg, rtol=0, atol=0)
    torch.testing.assert_close(b1.grad, b2.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c1.grad, c2.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(s1.grad, s2.grad, rtol=1e-4, atol=1e-5)
    # per-ray targets == the constant form's expression with per-ray colours
    out = torch.empty(512, 3, device="cuda")
    hip.NgpHeadBackend.bg_targets_rays(image, ws, depth, bg, out)
    torch.testing.assert_close(out, image + (1 - ws).unsqueeze(-1) * bg, rtol=0, atol=0)


def _scene_rays(n=4096, seed=0):
    from nerf import synthetic as syn
    poses = syn.orbit_poses(2, seed=0)
    r = syn.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, N=n, generator=torch.Generator().manual_seed(seed))
    return r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous()


def _density(net):
    from nerf import synthetic as syn
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens).cuda())
    net.density_bitfield.copy_(torch.from_numpy(bits).cuda())


def _graphed_run(recapture, steps=5):
    from nerf.trainer import GraphedTrainer
    ro, rd = _scene_rays()
    gt = _seeded((4096, 3), 9).cuda()
    net = _net()
    _density(net)
    net.iter_density = 100
    tr = GraphedTrainer(net, 4096, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
    tr.global_step = 1
    net.mean_count = 4096 * 40
    losses = []
    for _ in range(steps):
        if recapture:
            tr.graph = None  # every step is the capture's eager step (the same body, run on the stream instead of replayed)
        losses.append(float(tr.train_step(ro, rd, gt)))
    torch.cuda.synchronize()
    return net, tr, losses


def test_graphed_replay_equals_the_eager_step_with_background(hip, monkeypatch):
    """GraphedTrainer with the background model: 5 steps replayed from the graph vs the same 5 steps each run eagerly (the
    capture's warm-up step: same body, same jitter from the device step counter).  Tolerance, not bit equality: the background's
    table gradient is summed by fp16 atomics, whose order differs between runs (~1 fp16 ulp on a few table rows).  A missing,
    doubled or wrongly scaled update of any parameter moves it by ~lr = 1e-2, far outside the bound."""
    cnt = _Count(monkeypatch, hip)
    net_r, tr_r, l_r = _graphed_run(False)
    assert tr_r.n_captures == 1 and cnt.fwd >= 2  # one capture, then replays (+ the eager/capture calls of the kernels)
    net_e, tr_e, l_e = _graphed_run(True)
    assert tr_e.n_captures == 5
    assert np.isfinite(l_r).all() and np.isfinite(l_e).all()
    np.testing.assert_allclose(l_r, l_e, rtol=1e-3)
    for (k, a), b in zip(net_r.named_parameters(), net_e.parameters()):
        diff = (a.detach() - b.detach()).abs()
        # (Adam moves an entry by up to ~lr whatever its gradient's size: where that gradient is at the level of the atomics'
        #  rounding, the two runs may step it differently — a few entries up to ~4e-3, measured.  Summed over the tensor the
        #  runs agree: a missing or mis-scaled update of a parameter would move its mean by ~lr)
        assert diff.max().item() <= 1.5e-2 and diff.mean().item() <= 1e-5, (k, diff.max().item(), diff.mean().item())
    tab0 = _net().encoder_bg.embeddings.detach()
    assert (net_r.encoder_bg.embeddings.detach() - tab0).abs().mean().item() > 1e-4  # (the table did move)


def test_executed_train_step_with_background_vs_fixture(hip, monkeypatch):
    """the reference's executed Trainer.train_step with bg_radius = 32 (fixture part b) on the `-O` path: loss, prediction and
    the background gradients through the fused loss-free chain (network -> composite -> background kernels) at fp16 accuracy"""
    from sealnerf import SealTrainer
    from test_gpu_golden import _CpuRandom
    import raymarching.raymarching as rm
    import nerf.renderer as rend
    proxy = _CpuRandom()
    monkeypatch.setattr(rm, "torch", proxy)
    monkeypatch.setattr(rend, "torch", proxy)
    cnt = _Count(monkeypatch, hip)
    d = np.load(GOLD)
    from nerf import synthetic as syn
    from nerf.network import NeRFNetwork
    net = NeRFNetwork(bound=1, cuda_ray=True, log2_hashmap_size=14, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=32)
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    net = net.cuda()
    net.mean_count = int(d["ts_mean_count"])
    tr = SealTrainer(net, net, lr=1e-2, fp16=True, native_optim=False)
    net.train()
    torch.manual_seed(5)
    loss, out = tr.finetune_loss(torch.from_numpy(d["ts_rays_o"]).cuda(), torch.from_numpy(d["ts_rays_d"]).cuda(),
                                 torch.from_numpy(d["ts_images"]).cuda(), torch.from_numpy(d["ts_depths"]).cuda(), bg_color=1)
    assert np.array_equal(net.step_counter[0].cpu().numpy(), d["ts_counter"])
    assert abs(float(loss.detach()) - float(d["ts_loss"])) <= 5e-3 * float(d["ts_loss"])
    pred = out["image"].detach().float().cpu().numpy().reshape(d["ts_pred"].shape)
    assert np.abs(pred - d["ts_pred"]).max() / np.abs(d["ts_pred"]).max() < 2e-2
    net.zero_grad()
    loss.backward()
    assert cnt.fwd == 1 and cnt.bwd == 1
    for k, p in net.named_parameters():
        ref = float(d[f"ts_grad_{k.replace('.', '_')}_norm"])
        assert abs(float(p.grad.double().norm()) - ref) <= 3e-2 * ref, (k, float(p.grad.double().norm()), ref)
    for name in ("bg_net_0_weight", "bg_net_1_weight"):
        g = dict(net.named_parameters())[name.replace("_net_", "_net.").replace("_weight", ".weight")].grad.cpu().double()
        ref = torch.from_numpy(d[f"ts_grad_{name}"]).double()
        assert ((g - ref).norm() / ref.norm()).item() < 3e-2, name


# measured on an MI355X: 300 steps of 4,096 rays, error on 8,192 held-out rays / error of the best constant background = 0.54
# (err 6.7e-4, constant 1.25e-3; profiles/background.md).  The bound leaves headroom for run-to-run variation of the atomics.
SMOOTH_RATIO_BOUND = 0.75


def _smooth_target(d):
    """a smooth colour of the ray direction (the scene holds nothing else: every ray misses)"""
    return torch.stack([0.5 + 0.35 * d[:, 0], 0.5 + 0.3 * d[:, 1] * d[:, 2], 0.4 + 0.4 * d[:, 2] ** 2], 1).clamp(0, 1)


def smooth_background_run(steps=300):
    from nerf import synthetic as syn
    from nerf.trainer import Trainer
    net = _net(seeded=False)
    net.density_grid.zero_()
    net.density_bitfield.zero_()  # empty scene: the pixel is the background
    tr = Trainer(net, lr=1e-2, fp16=True, update_extra_interval=10 ** 9)
    poses = syn.orbit_poses(16, seed=1)
    for it in range(steps):
        r = syn.get_rays(poses[it % 16:it % 16 + 1], syn.lego_intrinsics(), 800, 800, N=4096,
                         generator=torch.Generator().manual_seed(it))
        ro, rd = r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous()
        tr.train_step(ro, rd, _smooth_target(rd))
    r = syn.get_rays(syn.orbit_poses(1, seed=9), syn.lego_intrinsics(), 800, 800, N=8192, generator=torch.Generator().manual_seed(999))
    ro, rd = r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous()
    gt = _smooth_target(rd)
    img = tr.render_image(ro, rd)["image"].reshape(-1, 3).float()
    err = float(((img - gt) ** 2).mean())
    const = float(((gt - gt.mean(0)) ** 2).mean())
    return err, const


def test_background_model_learns_a_smooth_background(hip):
    err, const = smooth_background_run()
    assert err < SMOOTH_RATIO_BOUND * const, (err, const, err / const)


def test_render_with_background_matches_torch_path(hip, monkeypatch):
    net = _net()
    cnt = _Count(monkeypatch, hip)
    _density(net)
    net.eval()
    from nerf import synthetic as syn
    poses = syn.orbit_poses(2, seed=0)
    r = syn.get_rays(poses[1:2], syn.lego_intrinsics(), 800, 800)
    ro, rd = r["rays_o"].cuda().contiguous(), r["rays_d"].cuda().contiguous()
    imgs = []
    for fused in (True, False):
        net.fused_background = fused
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            imgs.append(net.render(ro, rd, staged=False, perturb=False, max_steps=1024)["image"].float())
    net.fused_background = True
    assert cnt.fwd == 1  # once per frame, before the march loop; the torch-path frame launched none
    assert imgs[0].shape == (1, 640000, 3)
    assert (imgs[0] - imgs[1]).abs().max().item() <= 2e-3


def test_graphed_seal_bbox_finetune_and_proxy_truth_with_background(hip, S):
    from nerf import network, synthetic as syn
    from sealnerf import GraphedSealTrainer, get_seal_mapper, make_student, make_teacher
    torch.manual_seed(0)
    kw = dict(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, log2_hashmap_size=15, bg_radius=32)
    teacher = make_teacher(network.NeRFNetwork, **kw).cuda()
    student = make_student(network.NeRFNetwork, **kw).cuda()
    grid, bits = syn.lego_like_density_grid(seed=0)
    for net in (teacher, student):
        net.density_grid.copy_(torch.from_numpy(grid))
        net.density_bitfield.copy_(torch.from_numpy(bits))
        net.iter_density = 100
    student.load_state_dict(teacher.state_dict())
    from test_seal_golden import case_config
    m = get_seal_mapper(case_config("both", np.load(os.path.join(REPO, "tests", "golden", "seal_bbox.npz"))))
    teacher.init_mapper(m)
    student.init_mapper(m)
    tr = GraphedSealTrainer(student, teacher, 1024, lr=1e-2, fp16=True, update_extra_interval=16)
    poses = syn.orbit_poses(1, seed=0).cuda()
    r = syn.get_rays(poses, syn.lego_intrinsics(), 800, 800, N=1024, generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    # proxy targets with the teacher's background model: the per-ray target kernel == the torch composite
    rgb, dep = tr.proxy_truth(ro, rd)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        teacher.train()
        out = teacher.render(ro, rd, staged=True, bg_color=None, perturb=False, force_all_rays=True, max_steps=1024)
    torch.testing.assert_close(rgb.reshape(-1, 3), torch.nan_to_num(out["image"].reshape(-1, 3).float()), rtol=0, atol=1e-6)
    bg0 = student.encoder_bg.embeddings.detach().clone()
    hist = [float(tr.train_step(ro, rd)) for _ in range(24)]
    assert tr.n_captures >= 1 and np.isfinite(hist).all(), hist
    assert not torch.equal(student.encoder_bg.embeddings.detach(), bg0)


# ------------------------------------------------------------------------------------------------ edge shapes, frozen table, stride loop
# coordinates on the border exactly (x01 = 0 or 1 is inside), at the centre, and outside [-1, 1] on one axis or both; 1.0000001
# is the fp32 neighbour of 1 whose (x + 1) rounds back to 2: inside after normalisation
_SPECIAL = [[1.0, -1.0], [-1.0, 1.0], [0.0, 0.0], [1.05, -1.02], [-1.0, -1.0], [1.0, 1.0], [1.0, 0.0], [0.0, -1.0], [1.01, 0.3],
            [-0.2, -1.05], [-1.03, 1.04], [1.0, 1.05], [-1.05, -1.0], [0.999, 1.0], [1.02, 1.0], [1.0000001, 0.5], [-3.25, 0.5]]
GUARD, GUARD_VALUE = 256, 1234.0  # (exact in fp16)


def _small_table_net(log2_hashmap_size=10):
    """the background network on a small table (the dense 17 x 17 level + three hashed levels of 2^10 rows, so rays collide on
    every level): cheap to guard, and every row is reached"""
    from encoding import get_encoder
    net = _net()
    enc, _ = get_encoder("hashgrid", input_dim=2, num_levels=4, log2_hashmap_size=log2_hashmap_size, desired_resolution=2048)
    enc.embeddings.data.copy_(_seeded(enc.embeddings.shape, 77, -0.5, 0.5))
    net.encoder_bg = enc.cuda()
    return net


def _torch_path(net, sph, rd, g, dt):
    """(rgb, dW0, dW1, d table) of background()'s torch op sequence under fp16 autocast.  fp32 table: the encoder is called
    outside autocast, where it reads the parameter itself, and the rest of the sequence under it"""
    from nerf.network import _run_mlp
    net.zero_grad()
    if dt == torch.float16:
        rgb = _bg(net, sph, rd, False)
    else:
        feat = net.encoder_bg(sph)
        with torch.autocast("cuda", dtype=torch.float16):
            rgb = torch.sigmoid(_run_mlp(net.bg_net, torch.cat([net.encoder_dir(rd), feat], dim=-1)))
    rgb.float().backward(g)
    return (rgb.detach().float(), net.bg_net[0].weight.grad.clone(), net.bg_net[1].weight.grad.clone(),
            net.encoder_bg.embeddings.grad.float().clone())


class _Guarded:
    """the table and a zeroed table gradient of dtype `dt`, each between guard words"""

    def __init__(self, net, dt):
        emb = net.encoder_bg.embeddings.detach()
        n = emb.numel()
        self.bufs = [torch.full((GUARD + n + GUARD,), GUARD_VALUE, dtype=dt, device="cuda") for _ in range(2)]
        self.table, self.grad = (b[GUARD:GUARD + n].view(emb.shape) for b in self.bufs)
        self.table.copy_(emb)
        self.grad.zero_()

    def intact(self):
        return all(bool((b[:GUARD] == GUARD_VALUE).all()) and bool((b[-GUARD:] == GUARD_VALUE).all()) for b in self.bufs)


def _fused_pair(hip, net, sph, rd, g, table, grad_table):
    """(rgb, dW0, dW1) of the two fused launches on `table`; the table gradient is ADDED into grad_table"""
    enc = net.encoder_bg
    S = float(np.log2(enc.per_level_scale))
    w0, w1 = net.bg_net[0].weight.detach(), net.bg_net[1].weight.detach()
    N = sph.shape[0]
    rgb = torch.empty(N, 3, device="cuda")
    gw0, gw1 = torch.empty(64, 24, device="cuda"), torch.empty(3, 64, device="cuda")
    hip.NgpHeadBackend.background_forward(sph, rd, table, enc.offsets, S, enc.base_resolution, w0, w1, rgb)
    hip.NgpHeadBackend.background_backward(g, rgb, sph, rd, table, enc.offsets, S, enc.base_resolution, w0, w1, grad_table, gw0, gw1)
    torch.cuda.synchronize()
    return rgb, gw0, gw1


def _assert_paths_agree(got, want, what=""):
    """the bounds of test_fused_forward_backward_vs_fixture_and_torch_path: the two paths share their fp16 roundings and differ in
    summation order only: 1e-3 on the colour, 1 % of the largest entry (+ 1e-4) on each gradient"""
    print(what, "colour max diff", (got[0] - want[0]).abs().max().item())
    for name, a, b in zip(("dW0", "dW1", "d table"), got[1:], want[1:]):
        print(what, name, "max diff", (a - b).abs().max().item(), "of max", b.abs().max().item())
    assert (got[0] - want[0]).abs().max().item() <= 1e-3
    for a, b in zip(got[1:], want[1:]):
        assert (a - b).abs().max().item() <= 1e-2 * b.abs().max().item() + 1e-4


def _outside(sph):
    """[N] mask of the rows outside [0,1]^2 after the kernels' normalisation (x + 1) * 0.5 in fp32"""
    x01 = (sph + 1.0) * 0.5
    return ((x01 < 0) | (x01 > 1)).any(1)


def _touched_rows(hip, net, sph):
    """[rows] mask of the table rows a corner of some inside ray lands on (the grid encoder's own index kernel)"""
    enc = net.encoder_bg
    N = sph.shape[0]
    cidx = torch.empty(N, 4, 4, dtype=torch.int32, device="cuda")
    hip.GridBackend.grid_corner_indices(((sph + 1.0) * 0.5).cuda().contiguous(), enc.offsets, cidx, N, 2, 2, 4,
                                        float(np.log2(enc.per_level_scale)), enc.base_resolution, 0, False)
    rows = cidx.long() + enc.offsets[:4].long().view(1, 4, 1)
    mask = torch.zeros(enc.embeddings.shape[0], dtype=torch.bool, device="cuda")
    mask[rows[~_outside(sph).cuda()].reshape(-1)] = True
    return mask


@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_edge_shapes_against_the_torch_path(hip, dt):
    """N around the wave and block sizes, coordinates on and around the border, both table dtypes: the fused pair against the
    torch path, guard words around the table and its gradient, exactly zero gradient on every row no inside ray reaches and from
    the outside rays alone, and exactly the colour of an all-zero table for a ray outside [0,1]^2 after normalisation"""
    net = _small_table_net()
    for N in (1, 63, 64, 65, 257):
        sph = _seeded((N, 2), 10 + N, -1.05, 1.05)
        k = min(N, len(_SPECIAL))
        sph[:k] = torch.tensor(_SPECIAL[:k])
        rd = torch.nn.functional.normalize(_seeded((N, 3), 20 + N, -1, 1), dim=-1).cuda()
        g = _seeded((N, 3), 30 + N, -1, 1).cuda()
        want = _torch_path(net, sph.cuda(), rd, g, dt)
        mem = _Guarded(net, dt)
        rgb, gw0, gw1 = _fused_pair(hip, net, sph.cuda(), rd, g, mem.table, mem.grad)
        assert mem.intact(), (dt, N)
        _assert_paths_agree((rgb, gw0, gw1, mem.grad.float()), want, f"table {dt} N {N}:")
        # rows no inside ray reaches: exactly zero
        mask = _touched_rows(hip, net, sph)
        assert bool((mem.grad[~mask] == 0).all()) and float(mem.grad.float().abs().sum()) > 0
        outside = _outside(sph).cuda()
        assert int(outside.sum()) >= (2 if N > len(_SPECIAL) else 0)
        # outside rows: exactly the colour of an all-zero table ...
        zero = _Guarded(net, dt)
        zero.table.zero_()
        rgb0, _, _ = _fused_pair(hip, net, sph.cuda(), rd, g, zero.table, None)
        assert zero.intact() and bool((zero.grad == 0).all())
        assert torch.equal(rgb[outside], rgb0[outside])
        assert not torch.equal(rgb[~outside], rgb0[~outside])
        # ... and, run by themselves, exactly nothing added to the gradient table
        if bool(outside.any()):
            alone = _Guarded(net, dt)
            _fused_pair(hip, net, sph.cuda()[outside].contiguous(), rd[outside].contiguous(), g[outside].contiguous(), alone.table,
                        alone.grad)
            assert alone.intact() and bool((alone.grad == 0).all())


def test_frozen_table_gets_no_scatter(hip, monkeypatch):
    net = _net()
    sph = _seeded((300, 2), 5, -1.05, 1.05).cuda()
    rd = torch.nn.functional.normalize(_seeded((300, 3), 6, -1, 1), dim=-1).cuda()
    g = _seeded((300, 3), 7, -1, 1).cuda()
    _bg(net, sph, rd, True).float().backward(g)
    want = [net.bg_net[0].weight.grad.clone(), net.bg_net[1].weight.grad.clone()]
    assert float(net.encoder_bg.embeddings.grad.abs().sum()) > 0
    net.zero_grad()
    net.encoder_bg.embeddings.requires_grad_(False)
    seen = []
    real = hip.NgpHeadBackend.background_backward
    monkeypatch.setattr(hip.NgpHeadBackend, "background_backward",
                        staticmethod(lambda *a, **k: (seen.append(a[10]), real(*a, **k))[1]))
    _bg(net, sph, rd, True).float().backward(g)
    assert seen == [None] and net.encoder_bg.embeddings.grad is None
    assert torch.equal(net.bg_net[0].weight.grad, want[0]) and torch.equal(net.bg_net[1].weight.grad, want[1])


STRIDE_N = 2048 * 64 + 65  # the backward grid is capped at 2,048 one-wave workgroups: workgroup 0 and one partial wave go round twice


def test_backward_stride_loop_second_trip(hip):
    """The backward's stride loop beyond its first trip: fused against the torch path, and against the sum of two fused calls on
    the two halves of the batch (one trip each: the same addends in another order), both within 1 % of the largest entry + 1e-4.
    On an fp32 table: 131,137 rays put ~1,800 addends on each of the 289 rows of the coarsest level, and an fp16 atomic rounds the
    running sum at every one of them — ~1,800 roundings of up to half an fp16 ulp of a sum of order 1 walk ~1e-2 away in either
    path, which is that bound; in fp32 the same walk is ~1e-6 and the bound is about the kernels."""
    net = _small_table_net()
    N, dt = STRIDE_N, torch.float32
    sph = _seeded((N, 2), 41, -1.02, 1.02).cuda()
    rd = torch.nn.functional.normalize(_seeded((N, 3), 42, -1, 1), dim=-1).cuda()
    g = _seeded((N, 3), 43, -1, 1).cuda()
    want = _torch_path(net, sph, rd, g, dt)
    mem = _Guarded(net, dt)
    rgb, gw0, gw1 = _fused_pair(hip, net, sph, rd, g, mem.table, mem.grad)
    assert mem.intact()
    _assert_paths_agree((rgb, gw0, gw1, mem.grad), want, f"N {N}:")
    halves = _Guarded(net, dt)
    h = N // 2
    parts = [_fused_pair(hip, net, sph[s].contiguous(), rd[s].contiguous(), g[s].contiguous(), halves.table, halves.grad)
             for s in (slice(0, h), slice(h, N))]
    assert torch.equal(torch.cat([p[0] for p in parts]), rgb)
    for name, a, b in (("dW0", gw0, parts[0][1] + parts[1][1]), ("dW1", gw1, parts[0][2] + parts[1][2]), ("d table", mem.grad, halves.grad)):
        print("one call vs two halves:", name, "max diff", (a - b).abs().max().item(), "of max", b.abs().max().item())
        assert (a - b).abs().max().item() <= 1e-2 * b.abs().max().item() + 1e-4
