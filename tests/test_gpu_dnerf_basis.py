"""D-NeRF temporal-basis backbone on the GPU: the two kernels of csrc/dnerf_basis.hip against the contract of include/seal3d_hip.h
(bit for bit where it says so, within bounds derived from the number formats elsewhere), the fused route of the model against its
own torch routes, the renderer's slot selection with this model, a budgeted step and a training smoke."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the bits of grad_sigma_basis recorded before the hand-over of the sum moved into csrc/ordered_sum.hpp
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordered_sum_bits.json")) as _f:
    RECORDED = json.load(_f)["basis_grad_sigma_basis"]

SENT = 12345.0  # sentinel the output buffers are pre-filled with (exact in fp16)
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]  # wave, workgroup and ragged edges of a one-lane-per-row kernel and its reduction
# ... and of the backward's sum: more than 8 workgroups (two partials in a stripe of the last workgroup's sum), more than its 512
# workgroups (a second row per lane)
CASES = [(B, None) for B in SIZES + [2305, 512 * 256 + 257]] + [(257, 0), (257, 100), (257, 262)]


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _live(B, n_valid):
    return B if n_valid is None else min(B, (max(n_valid, 0) + 127) // 128 * 128)


def _nv(n_valid):
    return None if n_valid is None else torch.tensor([n_valid, 0], dtype=torch.int32, device="cuda")


def _inputs(B):
    """h [B, 64] fp16 in [-1, 1], unit dirs, sb [32] fp16 in [-0.3, 0.3]: |h[:, :32] . sb| <= 9.6"""
    h = _seeded((B, 64), B + 1, -1, 1).half()
    d = torch.nn.functional.normalize(_seeded((B, 3), B + 2, -1, 1), dim=-1)
    sb = _seeded((32,), 3, -0.3, 0.3).half()
    return h.cuda(), d.cuda().contiguous(), sb.cuda()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- forward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n_valid", CASES)
def test_mid_forward(hip, B, n_valid):
    h, d, sb = _inputs(B)
    live = _live(B, n_valid)
    sigma = torch.full((B,), SENT, device="cuda")
    cin = torch.full((B, 48), SENT, dtype=torch.float16, device="cuda")
    hip.DnerfBasisBackend.mid_forward(h, d, sb, sigma, cin, _nv(n_valid))
    # columns 0..15: the bits of s3d_ngp_mid_forward for the same directions
    ref_sigma, ref_cin = torch.empty(B, device="cuda"), torch.empty(B, 32, dtype=torch.float16, device="cuda")
    hip.NgpHeadBackend.mid_forward(torch.zeros(B, 16, dtype=torch.float16, device="cuda"), d, ref_sigma, ref_cin)
    assert torch.equal(_bits(cin[:live, :16]), _bits(ref_cin[:live, :16]))
    assert torch.equal(_bits(cin[:live, 16:]), _bits(h[:live, 32:]))
    assert (cin[live:] == SENT).all() and (sigma[live:] == SENT).all()
    if live:
        assert bool(ref_cin[:live, 1:16].abs().sum() > 0)
        h64, sb64 = h[:live, :32].double().cpu().numpy(), sb.double().cpu().numpy()
        D = h64 @ sb64
        assert np.abs(D).max() <= 10
        # half rounding of the sum, the 32-term fp32 chain (32 fused multiply-adds + the product terms' own: 33 roundings at most),
        # expf and the fp32 store
        bound = 2.0 ** -11 * np.abs(D) + 33 * 2.0 ** -24 * (np.abs(h64) * np.abs(sb64)).sum(axis=1) + 2.0 ** -21
        err = np.abs(np.log(sigma[:live].double().cpu().numpy()) - D)
        print(f"[basis mid forward] B {B} n_valid {n_valid}: max err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), float((err / bound).max())
    # sigma alone (density()): the same bits, no colour row
    alone = torch.full((B,), SENT, device="cuda")
    hip.DnerfBasisBackend.mid_forward(h, None, sb, alone, None, _nv(n_valid))
    assert torch.equal(alone, sigma)


# ---- backward -------------------------------------------------------------------------------------------------------------------
def _backward(hip, h, sb, g_cin, g_sigma, n_valid, want_sum=True):
    B = h.shape[0]
    g_h = torch.full((B, 64), SENT, dtype=torch.float16, device="cuda")
    g_sb = torch.full((32,), SENT, device="cuda") if want_sum else None
    hip.DnerfBasisBackend.mid_backward(g_cin, g_sigma, h, sb, g_h, g_sb, _nv(n_valid))
    return g_h, g_sb


@pytest.mark.parametrize("B,n_valid", CASES)
def test_mid_backward(hip, B, n_valid):
    h, d, sb = _inputs(B)
    live = _live(B, n_valid)
    g_cin = _seeded((B, 48), B + 4, -1, 1).half().cuda()
    g_sigma = _seeded((B,), B + 5, -1, 1).cuda()
    sigma = torch.empty(B, device="cuda")
    hip.DnerfBasisBackend.mid_forward(h, None, sb, sigma)  # (|pre| <= 9.6: the clamp is the identity, exp(clamp(pre)) is the forward's sigma)
    g_h, g_sb = _backward(hip, h, sb, g_cin, g_sigma, n_valid)
    again = _backward(hip, h, sb, g_cin, g_sigma, n_valid)
    assert torch.equal(_bits(g_h[:live, 32:]), _bits(g_cin[:live, 16:]))
    assert (g_h[live:] == SENT).all()
    gh = (g_sigma.cpu().numpy().astype(np.float32) * sigma.cpu().numpy().astype(np.float32)).astype(np.float16)  # half(fl32(g sigma))
    want = (gh.astype(np.float32)[:, None] * sb.cpu().numpy().astype(np.float32)[None, :]).astype(np.float16)
    got = g_h[:, :32].cpu().numpy()
    assert np.array_equal(got[:live].view(np.int16), want[:live].view(np.int16))
    # the 32-column sum: any order of fp32 additions of n exact terms stays within n 2^-24 sum |term| of the exact sum
    terms = gh[:live].astype(np.float64)[:, None] * h[:live, :32].double().cpu().numpy()
    exact, bound = terms.sum(axis=0), B * 2.0 ** -24 * np.abs(terms).sum(axis=0)
    err = np.abs(g_sb.double().cpu().numpy() - exact)
    print(f"[basis mid backward] B {B} n_valid {n_valid}: max |sum err| {float(err.max()):.3e} (bound {float(bound.max()):.3e})")
    assert (err <= bound).all()
    assert live == 0 or bool(g_sb.abs().sum() > 0)
    assert torch.equal(g_sb.view(torch.int32), again[1].view(torch.int32))  # the same bits in two runs
    assert g_sb.view(torch.int32).cpu().tolist() == RECORDED[f"B{B}-nv{n_valid}"]
    assert torch.equal(_bits(again[0]), _bits(g_h))
    # without grad_sigma: zeros in the basis columns and in the sum, the copies as before
    z_h, z_sb = _backward(hip, h, sb, g_cin, None, n_valid)
    assert not z_h[:live, :32].any() and not z_sb.any() and torch.equal(_bits(z_h[:live, 32:]), _bits(g_cin[:live, 16:]))
    assert (z_h[live:] == SENT).all()
    # without the sum: the same rows
    only_h, _ = _backward(hip, h, sb, g_cin, g_sigma, n_valid, want_sum=False)
    assert torch.equal(_bits(only_h), _bits(g_h))


def test_mid_backward_clamps_the_exponent_at_15(hip):
    B = 65
    h = (_seeded((B, 64), 1, -1, 1) * 0.1).half()
    h[7, :32], h[9, :32] = 1.0, -1.0
    sb = torch.full((32,), 0.5).half()  # rows 7 and 9: pre = +-16 exactly
    h, sb = h.cuda(), sb.cuda()
    g_cin = torch.zeros(B, 48, dtype=torch.float16, device="cuda")
    g_sigma = torch.full((B,), 2.0 ** -12, device="cuda")
    g_sigma[9] = 2.0 ** 10  # (exp(-15) 2^10 = 3.1e-4: a normal fp16 number)
    sigma = torch.empty(B, device="cuda")
    hip.DnerfBasisBackend.mid_forward(h, None, sb, sigma)
    assert abs(float(sigma[7]) / np.exp(16.0) - 1) < 1e-6 and abs(float(sigma[9]) / np.exp(-16.0) - 1) < 1e-6  # (the value is not clamped)
    g_h, g_sb = _backward(hip, h, sb, g_cin, g_sigma, None)
    for row, e in ((7, 15.0), (9, -15.0)):
        want = float(g_sigma[row]) * np.exp(e) * 0.5  # half(g) sb_k: the product by 0.5 is exact, so one rounding, of g
        got = float(g_h[row, 0])
        ulp = float(np.spacing(np.float16(want)))
        assert want >= 2.0 ** -14 and abs(got - want) <= ulp, (row, got, want)
        assert abs(got - want * np.exp(np.sign(e))) > 100 * ulp  # (exp(+-16), the unclamped slope, is far off)
        assert torch.equal(g_h[row, :32], g_h[row, :1].expand(32))
    assert torch.isfinite(g_sb).all()


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(seed_range=0.25, time_size=2, **kw):
    from dnerf.network_basis import NeRFNetwork
    from gridencoder import GridEncoder
    net = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, time_size=time_size, **kw)
    net.encoder = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=14, desired_resolution=256,
                              gridtype="tiled")
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -seed_range, seed_range))
    return net.cuda()


def _marched_points(net, M):
    import raymarching
    from nerf import synthetic as syn
    dens, bits = syn.lego_like_density_grid(seed=0)
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=128, generator=torch.Generator().manual_seed(81))
    ro, rd = r["rays_o"][0].contiguous().cuda(), r["rays_d"][0].contiguous().cuda()
    nears, fars = raymarching.near_far_from_aabb(ro, rd, net.aabb_train, net.min_near)
    counter = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, _, _ = raymarching.march_rays_train(ro, rd, 1, torch.from_numpy(bits).cuda(), 1, 128, nears, fars, counter, 0, False, 128,
                                                    True, 0, 1024)
    assert xyzs.shape[0] >= M
    return xyzs[:M].contiguous(), dirs[:M].contiguous()


def _route(net, x, d, t, mode):
    """(outputs, parameter gradients) of one route: 'fp32' (torch ops, no autocast), 'autocast' (torch ops), 'fused'"""
    net.zero_grad()
    net.fused_mlp = mode == "fused"
    net.train()
    calls = []
    mid = net._color_fused
    net._color_fused = lambda *a: (calls.append(1), mid(*a))[1]
    try:
        with torch.autocast("cuda", dtype=torch.float16, enabled=mode != "fp32"):
            sigma, rgbs, deform = net(x, d, t)
            loss = (sigma.float() * 0.01).sum() + rgbs.float().sum() * 0.1
        loss.backward()
    finally:
        del net._color_fused
    assert deform is None and bool(calls) == (mode == "fused")
    out = dict(sigma=sigma.detach().float(), rgbs=rgbs.detach().float())
    for k, p in net.named_parameters():
        out["grad " + k] = p.grad.detach().float().clone()
    return out


def _three_routes(net, M, capsys=None):
    x, d = _marched_points(net, M)
    t = torch.tensor([[0.37]], device="cuda")
    ref = _route(net, x, d, t, "fp32")
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert 1e-3 < float(ref["sigma"].median()) < 1e3 and float(ref["sigma"].std()) > 1e-3  # (seeding: a live sigma)
    assert all(float(v.abs().max()) > 0 for v in ref.values())  # (every parameter takes a gradient, basis_net through both bases)
    auto = _route(net, x, d, t, "autocast")
    fused = _route(net, x, d, t, "fused")
    lines, bad = [], []
    for k, r in ref.items():
        scale = float(r.abs().max())
        ea, ef = float((auto[k] - r).abs().max()), float((fused[k] - r).abs().max())
        lines.append(f"{k:28s} max|ref| {scale:.3e}  autocast err {ea:.3e}  fused err {ef:.3e}")
        if not ef <= 2 * ea + 2e-3 * scale:
            bad.append(lines[-1])
    if capsys is not None:
        with capsys.disabled():
            print("\n[dnerf basis routes] " + "\n[dnerf basis routes] ".join(lines))
    assert not bad, "\n".join(bad)


def test_fused_route_against_the_models_own_torch_routes(hip, capsys):
    """the three-route criterion of tests/test_gpu_dnerf.py: for every output and parameter gradient the fused route's maximum error
    against the fp32 torch route is at most twice the autocast torch route's own, plus 2e-3 max|ref|.  1,500 marched points (no
    multiple of 128: padding rows), t = 0.37.  Figures: profiles/dnerf_basis.md."""
    net = _model()
    assert net._color_fusable()
    _three_routes(net, 1500, capsys)


def test_a_color_net_of_another_shape_stays_on_torch_inside_the_fused_route(hip):
    net = _model(hidden_dim_color=32)
    assert not net._color_fusable() and net._glue_ok()
    _three_routes(net, 300)


def test_density_on_the_fused_route(hip):
    net = _model().eval()
    x, _ = _marched_points(net, 300)
    t = torch.tensor([[0.37]], device="cuda")
    with torch.no_grad():
        ref = net.density(x, t)
        with torch.autocast("cuda", dtype=torch.float16):
            assert net._can_fuse(x)
            got = net.density(x, t)
    assert got["sigma"].shape == (300,) and got["geo_feat"].shape == (300, 32) and got["sigma"].dtype == torch.float32
    torch.testing.assert_close(got["sigma"], ref["sigma"], rtol=2e-2, atol=2e-3)
    torch.testing.assert_close(got["geo_feat"].float(), ref["geo_feat"], rtol=2e-2, atol=2e-3)


# ---- renderer, trainer ------------------------------------------------------------------------------------------------------------
def _box_bits(lo, hi):
    import raymarching
    H = 128
    c = torch.arange(H, device="cuda")
    xx, yy, zz = torch.meshgrid(c, c, c, indexing="ij")
    coords = torch.stack([xx, yy, zz], -1).reshape(-1, 3).int()
    w = 2 * coords.float() / (H - 1) - 1
    inside = ((w >= torch.tensor(lo, device="cuda")) & (w <= torch.tensor(hi, device="cuda"))).all(-1)
    grid = torch.zeros(1, H ** 3, device="cuda")
    grid[0, raymarching.morton3D(coords).long()] = inside.float()
    return raymarching.packbits(grid, 0.5)


@pytest.mark.parametrize("train", [True, False])
def test_run_cuda_marches_the_slot_of_its_time(hip, train):
    """two slots holding two different boxes: a rendering at t = 0.2 / 0.8 equals, bit for bit, the rendering of a one-slot model with
    the same parameters whose only slot holds that time's box"""
    from nerf import synthetic as syn
    model = _model(time_size=2)
    boxes = (_box_bits([-0.6, -0.6, -0.6], [-0.1, 0.6, 0.6]), _box_bits([0.1, -0.6, -0.6], [0.6, 0.6, 0.6]))
    model.density_bitfield[0].copy_(boxes[0])
    model.density_bitfield[1].copy_(boxes[1])
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=512, generator=torch.Generator().manual_seed(3))
    ro, rd = r["rays_o"][0].contiguous().cuda(), r["rays_d"][0].contiguous().cuda()
    images = []
    for time, slot in ((0.2, 0), (0.8, 1)):
        base = _model(time_size=1)
        base.density_bitfield[0].copy_(boxes[slot])
        model.train(train)
        base.train(train)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            got = model.run_cuda(ro, rd, time, bg_color=1, perturb=False, max_steps=256)
            want = base.run_cuda(ro, rd, time, bg_color=1, perturb=False, max_steps=256)
        assert torch.equal(got["image"], want["image"]) and torch.equal(got["depth"], want["depth"])
        assert ("deform" in got) == train and got.get("deform") is None
        assert model.density_bitfield.shape == (2, 128 ** 3 // 8)
        images.append(got["image"])
    assert not torch.equal(images[0], images[1]) and float((images[0] - 1).abs().max()) > 0.05


def test_a_budgeted_step_equals_the_trimmed_one(hip):
    """mean_count > 0: the marcher hands back zero-padded buffers, forward reads the count back once and runs on the live rows — the
    rows the marcher keeps when it trims (mean_count 0): the same samples through the same kernels."""
    from dnerf.utils import Trainer
    from nerf import synthetic as syn
    dens, bits = syn.lego_like_density_grid(seed=0)
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=256, generator=torch.Generator().manual_seed(81))
    ro, rd = r["rays_o"][0].contiguous().cuda(), r["rays_d"][0].contiguous().cuda()
    gt = _seeded((256, 3), 82).cuda()
    runs = {}
    for budget in (0, 32768):
        net = _model()
        net.density_bitfield[0].copy_(torch.from_numpy(bits))
        net.mean_count = budget
        tr = Trainer(net, fp16=True, native_optim=False, update_extra_interval=10 ** 9)
        tr.global_step = 1
        seen, shapes, ran = {}, [], []
        tr._reduce_and_step = lambda seen=seen, net=net: seen.update({k: p.grad.clone() for k, p in net.named_parameters()})
        fwd, dens_of = net.forward, net._density_fused
        net.forward = lambda x, d, t=None, fwd=fwd, shapes=shapes: (shapes.append(x.shape[0]), fwd(x, d, t))[1]
        net._density_fused = lambda x, t, dens_of=dens_of, ran=ran: (ran.append(x.shape[0]), dens_of(x, t))[1]
        torch.manual_seed(5)  # (the marcher's per-ray jitter: the same samples in both steps)
        loss = tr.train_step(ro, rd, gt, 0.2)
        runs[budget] = (loss.float(), seen, shapes[0], ran[0], int(net.step_counter[0, 0]))
    count = runs[0][4]
    live = (count + 127) // 128 * 128
    assert runs[32768][4] == count and 0 < live < 32768
    assert runs[0][2] == live and runs[32768][2] == 32768 + 128 - 32768 % 128  # (what the marcher handed over)
    assert runs[0][3] == runs[32768][3] == live  # (what the networks ran on)
    torch.testing.assert_close(runs[32768][0], runs[0][0], rtol=1e-6, atol=0)
    for k, g in runs[0][1].items():
        other = runs[32768][1][k]
        assert torch.isfinite(other).all() and bool(other.abs().sum() > 0), k
        if k == "encoder.embeddings":
            # (the fp16 table gradient of a batch this small is summed by atomics: tests/test_gpu_dnerf.py, the same step)
            assert torch.equal((other != 0).any(1).view(-1)[:4096], (g != 0).any(1).view(-1)[:4096])
            continue
        # the same rows through the same kernels; the Linear layers' GEMMs may add in another order from run to run, which moves an
        # fp16 result by an ulp of its size: 2^-10 of the largest entry
        torch.testing.assert_close(other, g, rtol=0, atol=2.0 ** -10 * float(g.abs().max()), msg=k)


def test_training_smoke_on_two_flat_colours(hip):
    """64 x 64 frames at eight times, one flat colour before t = 0.5 and another from there on: 30 eager steps of 1,024 rays; the loss
    stays finite and the mean of the last 8 steps (every frame once) lies below the mean of the first 8 (a direction, not a magnitude)"""
    from dnerf.network_basis import NeRFNetwork
    from dnerf.provider import DNeRFDataset
    from dnerf.utils import Trainer
    from nerf import synthetic as syn
    torch.manual_seed(0)
    times = (torch.arange(8, dtype=torch.float32) + 0.5) / 8
    colours = torch.tensor([[0.9, 0.2, 0.1], [0.1, 0.3, 0.9]])
    images = colours[(times >= 0.5).long()].view(8, 1, 1, 3).expand(8, 64, 64, 3).contiguous()
    poses = syn.orbit_poses(8, seed=0)
    f = 64 / 800
    fx, fy, cx, cy = syn.lego_intrinsics()
    ds = DNeRFDataset(images, poses, (fx * f, fy * f, cx * f, cy * f), times, num_rays=1024, device="cuda")
    net = NeRFNetwork(bound=1, cuda_ray=True, time_size=2, density_thresh=0.01).cuda()
    tr = Trainer(net, fp16=True, update_extra_interval=16)
    fused = []
    mid = net._color_fused
    net._color_fused = lambda *a: (fused.append(1), mid(*a))[1]
    losses = []
    for step in range(30):
        batch = ds.collate([step % 8])
        losses.append(tr.train_step(batch["rays_o"][0], batch["rays_d"][0], batch["images"][0], batch["time"]))
    losses = torch.stack(losses).float().cpu()
    assert torch.isfinite(losses).all() and fused
    first, last = float(losses[:8].mean()), float(losses[-8:].mean())
    print(f"[dnerf basis smoke] first 8: {first:.5f}  last 8: {last:.5f}")
    assert last < first
