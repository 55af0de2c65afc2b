"""D-NeRF backbone on the GPU: the four glue kernels of csrc/dnerf.hip against the kernels and torch ops they stand for (bit for
bit where the header says so), the two new MLP shapes through the existing entry points, the fused route of the model against its
own torch routes, the gradient path through dy_dx, the renderer's slot selection, the occupancy update and a training smoke."""
import math

import numpy as np
import pytest
import torch

import ordered_sum_witness as ow

pytestmark = pytest.mark.gpu

SENT = 12345.0  # sentinel the output buffers are pre-filled with (exact in fp16)


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _freq_half(hip, v, deg):
    v = v.contiguous()
    C = v.shape[1] * (1 + 2 * deg)
    out = torch.empty(v.shape[0], C, device="cuda")
    hip.FreqBackend.freq_encode_forward(v, v.shape[0], v.shape[1], deg, C, out)
    return out.half()


# ---- encode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 127, 129, 1500])
@pytest.mark.parametrize("n_valid", [None, 0, 77])
@pytest.mark.parametrize("per_row", [False, True])
def test_encode_rows_are_half_of_the_frequency_encoder(hip, B, n_valid, per_row):
    for bound, tv in ((1.0, 0.0), (2.0, 0.37), (1.0, 1.0)):
        x = _seeded((B, 3), B + 1, -bound, bound)
        x[0] = 0.0
        if B > 2:
            x[1], x[2] = bound, -bound
        x = x.cuda()
        t = (_seeded((B, 1), 7).cuda() if per_row else torch.full((1, 1), tv, device="cuda"))
        if per_row:
            t[0] = tv
        din = torch.full((B, 80), SENT, dtype=torch.float16, device="cuda")
        sin = torch.full((B, 112), SENT, dtype=torch.float16, device="cuda")
        nv = None if n_valid is None else torch.tensor([n_valid, 0], dtype=torch.int32, device="cuda")
        hip.DnerfBackend.encode_forward(x, t.reshape(-1), din, sin, nv)
        live = B if n_valid is None else min(B, (n_valid + 127) // 128 * 128)
        tt = t if per_row else t.expand(B, 1)
        want = torch.cat([_freq_half(hip, x, 10), _freq_half(hip, tt.contiguous(), 6),
                          torch.zeros(B, 4, dtype=torch.float16, device="cuda")], dim=1)
        assert torch.equal(din[:live], want[:live])
        assert torch.equal(sin[:live, 32:], want[:live])
        assert not din[:live, 76:].any() and not sin[:live, 108:].any()
        assert (sin[:, :32] == SENT).all() and (din[live:] == SENT).all() and (sin[live:] == SENT).all()


# ---- warp + grid --------------------------------------------------------------------------------------------------------------
def _encoder(gridtype, log2=14):
    from gridencoder import GridEncoder
    enc = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=log2, desired_resolution=256,
                      gridtype=gridtype).cuda()
    enc.embeddings.data.copy_(_seeded(enc.embeddings.shape, 11, -1, 1))
    rows = (enc.offsets[1:] - enc.offsets[:-1]).tolist()
    res = [int(np.ceil(16 * enc.per_level_scale ** l)) for l in range(16)]
    dense = sum((r + 1) ** 3 <= 2 ** log2 for r in res)
    assert dense >= 2 and 16 - dense >= 4, (dense, rows)
    return enc


@pytest.mark.parametrize("gridtype", ["hash", "tiled"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("B", [1, 129, 1500, 65795])  # (65,795: 258 chunks — a second partial for lane 0 of the last sum, three rows in the last chunk)
def test_warp_grid_forward_is_the_add_and_the_grid_encoder(hip, gridtype, dtype, B):
    enc = _encoder(gridtype)
    table = enc.embeddings.detach().to(dtype).contiguous()
    S, H = float(np.log2(enc.per_level_scale)), enc.base_resolution
    x = _seeded((B, 3), B, -1, 1).cuda()
    dout = (_seeded((B, 16), B + 3, -0.05, 0.05)).half().cuda()
    dout[0::5] = 0  # rows of zeros: xw == x exactly
    if B > 4:
        x[3] = torch.tensor([0.99, -0.99, 0.5])
        dout[3, :3] = torch.tensor([0.05, -0.05, 0.0])  # pushed outside the box
        x[4], dout[4, :3] = torch.tensor([1.0, 1.0, -1.0]), 0  # on the box
    sin = torch.full((B, 112), SENT, dtype=torch.float16, device="cuda")
    xw, deform = torch.empty(B, 3, device="cuda"), torch.empty(B, 3, device="cuda")
    dy_dx = torch.empty(B, 16 * 6, dtype=dtype, device="cuda")
    regs = []
    for _ in range(2):
        reg = torch.zeros((), device="cuda")
        hip.DnerfBackend.warp_grid_forward(x, dout, table, enc.offsets, S, H, enc.gridtype_id, False, 0, 1.0, sin, xw, deform, dy_dx, reg)
        regs.append(reg.clone())
    want_xw = x + dout[:, :3].float()
    assert torch.equal(xw, want_xw) and torch.equal(deform, dout[:, :3].float())
    assert torch.equal(xw[0], x[0])
    if B > 4:
        assert (xw[3].abs() > 1).any()
    ref = torch.empty(16, B, 2, dtype=dtype, device="cuda")
    ref_j = torch.empty(B, 16 * 6, dtype=dtype, device="cuda")
    hip.GridBackend.grid_encode_forward(((want_xw + 1) / 2).contiguous(), table, enc.offsets, ref, B, 3, 2, 16, S, H, ref_j, enc.gridtype_id,
                                        False, 0)
    want = ref.permute(1, 0, 2).reshape(B, 32).half()
    wrong = sin[:, :32] != want
    assert not wrong.any(), (f"{int(wrong.sum())} features differ: rows {wrong.any(1).nonzero().reshape(-1)[:8].tolist()} columns "
                             f"{wrong.any(0).nonzero().reshape(-1).tolist()} got {sin[:, :32][wrong][:4].tolist()} want {want[wrong][:4].tolist()}")
    wrong = (dy_dx != ref_j).view(B, 16, 6)
    assert not wrong.any(), (f"{int(wrong.sum())} dy_dx entries differ: rows {wrong.any(2).any(1).nonzero().reshape(-1)[:8].tolist()} levels "
                             f"{wrong.any(2).any(0).nonzero().reshape(-1).tolist()}")
    assert ref.abs().sum() > 0 and (B <= 4 or not sin[3, :32].any())
    assert (sin[:, 32:] == SENT).all()
    total = float(dout[:, :3].double().abs().sum())
    assert abs(float(regs[0]) - total) <= 1e-6 * total + 1e-12
    assert torch.equal(regs[0], regs[1])  # the same bits in two runs
    # ... and the bits of the documented order (csrc/ordered_sum.hpp): one row per lane, one partial per chunk of 256 rows
    d = dout[:, :3].float().abs().cpu().numpy()
    want_reg = ow.ordered_sum((d[:, 0] + d[:, 1]) + d[:, 2], (B + 255) // 256, strided=False)
    assert regs[0].cpu().numpy().view(np.uint32) == want_reg.view(np.uint32), (float(regs[0]), float(want_reg))
    # through the module (the table the kernels read under autocast is its fp16 cast): GridEncoder's forward at xw
    if dtype == torch.float16:
        enc.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert torch.equal(sin[:, :32], enc(want_xw, bound=1))


def test_warp_grid_smoothstep_align_corners_ragged_levels_and_row_limit(hip):
    from gridencoder import GridEncoder
    enc = GridEncoder(input_dim=3, num_levels=6, level_dim=2, base_resolution=8, log2_hashmap_size=10, desired_resolution=64,
                      gridtype="tiled", align_corners=True, interpolation="smoothstep").cuda()
    enc.embeddings.data.copy_(_seeded(enc.embeddings.shape, 12, -1, 1))
    table = enc.embeddings.detach().half().contiguous()
    S, H, B, L = float(np.log2(enc.per_level_scale)), enc.base_resolution, 300, 6
    x = _seeded((B, 3), 1, -2, 2).cuda()
    dout = _seeded((B, 16), 2, -0.05, 0.05).half().cuda()
    sin = torch.full((B, 112), SENT, dtype=torch.float16, device="cuda")
    xw = torch.full((B, 3), SENT, device="cuda")
    dy_dx = torch.full((B, L * 6), SENT, dtype=torch.float16, device="cuda")
    nv = torch.tensor([130, 0], dtype=torch.int32, device="cuda")
    reg = torch.zeros((), device="cuda")
    hip.DnerfBackend.warp_grid_forward(x, dout, table, enc.offsets, S, H, 1, True, 1, 2.0, sin, xw, None, dy_dx, reg, nv)
    live = 256
    want_xw = x + dout[:, :3].float()
    ref = torch.empty(L, B, 2, dtype=torch.float16, device="cuda")
    ref_j = torch.empty(B, L * 6, dtype=torch.float16, device="cuda")
    hip.GridBackend.grid_encode_forward(((want_xw + 2) / 4).contiguous(), table, enc.offsets, ref, B, 3, 2, L, S, H, ref_j, 1, True, 1)
    assert torch.equal(xw[:live], want_xw[:live]) and (xw[live:] == SENT).all()
    assert torch.equal(sin[:live, :2 * L], ref.permute(1, 0, 2).reshape(B, 2 * L)[:live])
    wrong = (dy_dx[:live] != ref_j[:live]).view(live, L, 3, 2)
    assert not wrong.any(), f"dy_dx differs at (level, dim) {wrong.any(0).any(-1).nonzero().tolist()} in {int(wrong.any(-1).any(-1).any(-1).sum())} rows"
    assert (dy_dx[live:] == SENT).all()
    assert (sin[:, 2 * L:] == SENT).all() and (sin[live:] == SENT).all()
    total = float(dout[:live, :3].double().abs().sum())  # the regulariser's rows: the live ones
    assert abs(float(reg) - total) <= 1e-6 * total


# ---- the two backward steps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("B", [1, 129, 1500])
def test_split_grad_and_warp_backward(hip, dtype, B):
    g_sin = _seeded((B, 112), 5, -1, 1).half().cuda()
    out = torch.full((16, B, 2), SENT, dtype=dtype, device="cuda")
    hip.DnerfBackend.split_grad(g_sin, out)
    assert torch.equal(out, g_sin[:, :32].reshape(B, 16, 2).permute(1, 0, 2).to(dtype))
    for L in (6, 1):  # a ragged last group of levels; one level; rows behind the limit stay as they were
        out = torch.full((L, B, 2), SENT, dtype=dtype, device="cuda")
        nv = torch.tensor([130, 0], dtype=torch.int32, device="cuda")
        hip.DnerfBackend.split_grad(g_sin, out, nv)
        live = min(B, 256)
        assert torch.equal(out[:, :live], g_sin[:live, :2 * L].reshape(live, L, 2).permute(1, 0, 2).to(dtype))
        assert (out[:, live:] == SENT).all()
    g_xw = _seeded((B, 3), 6, -1, 1).to(dtype).cuda()
    deform = _seeded((B, 3), 7, -0.05, 0.05).cuda()
    deform[0] = 0.0
    coef = torch.tensor([0.4375], device="cuda")
    for c in (None, coef):
        for scale in (1.0, 0.5):
            g_dout = torch.full((B, 16), SENT, dtype=torch.float16, device="cuda")
            hip.DnerfBackend.warp_backward(g_xw, scale, deform, c, g_dout)
            want = g_xw.float() * scale if c is None else (c * torch.sign(deform) + g_xw.float() * scale)
            # (coef * sign is exact and the product by a power of two too: the sum rounds once in fp32, as the kernel's fmaf does)
            assert torch.equal(g_dout[:, :3], want.half())
            assert not g_dout[:, 3:].any()
            assert c is None or torch.equal(g_dout[0, :3], (g_xw[0].float() * scale).half())


# ---- the two MLP shapes through the existing entry points ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(80, 128, 4), (112, 64, 2)])
@pytest.mark.parametrize("n_valid", [None, 200])
def test_the_two_mlp_shapes_through_ffmlp(hip, shape, n_valid):
    """80 -> 128 x 4 -> 16 and 112 -> 64 (-> I_64) -> 16 against torch's fp16 Linears, at the tolerances tests/test_gpu_ffmlp.py uses
    for its layer-by-layer shapes.  n_valid = 200: 200 live rows in a batch of 256 whose other rows are zero (what the fused route
    hands these networks: the renderer trims the marcher's rows for this backbone and the route pads with zero rows).  The 128-wide
    network also takes the device-side count itself; the 112-wide one runs on the layer-by-layer kernels, which refuse it."""
    from ffmlp.ffmlp import ffmlp_forward
    in_dim, W, n = shape
    B = 256
    live = B if n_valid is None else n_valid
    torch.manual_seed(in_dim)
    dims = [in_dim] + [W] * n + [16]
    mats = [(torch.randn(o, i, device="cuda") * math.sqrt(2.0 / i)).half() for i, o in zip(dims[:-1], dims[1:])]
    if shape == (112, 64, 2):
        mats[1] = torch.eye(64, device="cuda").half()
    flat = torch.cat([m.reshape(-1) for m in mats]).float().requires_grad_(True)
    x = (torch.randn(B, in_dim, device="cuda") * 0.5).half()
    x[live:] = 0
    xg = x.clone().requires_grad_(True)
    nv = None if n_valid is None else torch.tensor([n_valid, 0], dtype=torch.int32, device="cuda")
    if nv is not None and W == 64:
        with pytest.raises(RuntimeError, match="n_valid"), torch.autocast("cuda", dtype=torch.float16):
            ffmlp_forward(xg, flat, in_dim, 16, W, n, 0, 6, False, True, None, None, 0, nv)
        nv = None
    with torch.autocast("cuda", dtype=torch.float16):
        y = ffmlp_forward(xg, flat, in_dim, 16, W, n, 0, 6, False, True, None, None, 0, nv)
    go = torch.randn(B, 16, device="cuda") * 0.1
    go[live:] = 0
    y.float().backward(go)
    xr = x.float().requires_grad_(True)
    wr = [m.float().requires_grad_(True) for m in mats]
    h = xr
    for i, m in enumerate(wr):
        h = h @ m.t()
        if i != n:
            h = torch.relu(h)
    h.backward(go)
    torch.testing.assert_close(y.float(), h.detach(), rtol=3e-2, atol=3e-2)
    assert not y[live:].any()
    assert (xg.grad.float() - xr.grad).norm() / xr.grad.norm() < 3e-2
    gw_ref = torch.cat([m.grad.reshape(-1) for m in wr])
    assert (flat.grad - gw_ref).abs().max() / gw_ref.abs().max() < 3e-2
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        yi = ffmlp_forward(x, flat.detach(), in_dim, 16, W, n, 0, 6, True, False, None, None, 0, None)
    torch.testing.assert_close(yi.float(), y.detach().float(), rtol=1e-3, atol=1e-3)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(seed_range=0.09, **kw):  # (|deform| stays below 0.05 on the marched points; checked where it matters)
    import zlib
    from dnerf.network import NeRFNetwork
    from gridencoder import GridEncoder
    net = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, time_size=2, **kw)
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
    with torch.autocast("cuda", dtype=torch.float16, enabled=mode != "fp32"):
        sigma, rgbs, deform = net(x, d, t)
        used = net._deform_reg is not None
        assert used == (mode == "fused")
        reg = net._deform_reg[0] / (3 * x.shape[0]) if used else deform.float().abs().mean()
        loss = (sigma.float() * 0.01).sum() + rgbs.float().sum() * 0.1 + reg * 10.0
    loss.backward()
    out = dict(sigma=sigma.detach().float(), rgbs=rgbs.detach().float(), deform=deform.detach().float())
    for k, p in net.named_parameters():
        out["grad " + k] = p.grad.detach().float().clone()
    return out


def test_fused_route_against_the_models_own_torch_routes(hip, capsys):
    """Because x' feeds the finest grid level, one fp16 ulp of `deform` moves features visibly: no fixed fp16 tolerance against the
    autocast route is derivable.  Measured instead: for every output and parameter gradient, the fused route's maximum error against
    the fp32 torch route may be at most twice the autocast torch route's own, plus 2e-3 max|ref| (the project's fp16 atol,
    tests/test_gpu_tensorf_cp.py).  Figures: profiles/dnerf.md."""
    net = _model()
    x, d = _marched_points(net, 1500)
    t = torch.tensor([[0.37]], device="cuda")
    ref = _route(net, x, d, t, "fp32")
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert float(ref["deform"].abs().max()) < 0.05 and 1e-3 < float(ref["sigma"].median()) < 1e3  # (seeding: small warp, live sigma)
    auto = _route(net, x, d, t, "autocast")
    fused = _route(net, x, d, t, "fused")
    lines, bad = [], []
    for k, r in ref.items():
        scale = float(r.abs().max())
        ea, ef = float((auto[k] - r).abs().max()), float((fused[k] - r).abs().max())
        lines.append(f"{k:28s} max|ref| {scale:.3e}  autocast err {ea:.3e}  fused err {ef:.3e}")
        if not ef <= 2 * ea + 2e-3 * scale:
            bad.append(lines[-1])
    with capsys.disabled():
        print("\n[dnerf routes] " + "\n[dnerf routes] ".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kw", [dict(hidden_dim_deform=64), dict(num_layers_deform=3), dict(num_layers=3), dict(geo_feat_dim=7),
                                dict(hidden_dim_color=32)])
def test_a_network_of_another_shape_stays_on_torch_inside_the_fused_route(hip, kw):
    """a shape the fused MLP entry points do not take keeps THAT network on torch's Linear; the glue kernels and the other networks
    still run (the regulariser's sum comes from the warp kernel) — same criterion as the three-route test"""
    net = _model(**kw)
    x, d = _marched_points(net, 300)
    t = torch.tensor([[0.37]], device="cuda")
    assert net._deform_fusable() == ("hidden_dim_deform" not in kw and "num_layers_deform" not in kw)
    assert net._sigma_fusable() == ("num_layers" not in kw and "geo_feat_dim" not in kw)
    assert net._color_fusable() == ("geo_feat_dim" not in kw and "hidden_dim_color" not in kw)
    ref = _route(net, x, d, t, "fp32")
    auto = _route(net, x, d, t, "autocast")
    fused = _route(net, x, d, t, "fused")
    for k, r in ref.items():
        scale = float(r.abs().max())
        ea, ef = float((auto[k] - r).abs().max()), float((fused[k] - r).abs().max())
        assert ef <= 2 * ea + 2e-3 * scale, f"{k}: max|ref| {scale:.3e} autocast err {ea:.3e} fused err {ef:.3e}"


def test_gradient_reaches_the_deformation_net_through_dy_dx(hip):
    from dnerf.utils import Trainer
    from nerf import synthetic as syn
    dens, bits = syn.lego_like_density_grid(seed=0)
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=256, generator=torch.Generator().manual_seed(81))
    ro, rd = r["rays_o"][0].contiguous().cuda(), r["rays_d"][0].contiguous().cuda()
    gt = _seeded((256, 3), 82).cuda()
    for weight in (1e-3, 0.0):
        net = _model()
        net.density_bitfield[0].copy_(torch.from_numpy(bits))
        tr = Trainer(net, fp16=True, native_optim=False, deform_reg_weight=weight, update_extra_interval=10 ** 9)
        tr.global_step = 1
        seen = {}
        tr._reduce_and_step = lambda: seen.update({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
        fused_calls = []
        orig = net._density_fused
        net._density_fused = lambda *a: (fused_calls.append(1), orig(*a))[1]
        loss = tr.train_step(ro, rd, gt, 0.2)
        assert torch.isfinite(loss) and fused_calls
        grads = [seen[f"deform_net.{i}.weight"] for i in range(5)]
        assert all(torch.isfinite(g).all() for g in grads)
        assert any(bool(g.abs().sum() > 0) for g in grads), weight  # (weight 0: the gradient comes through dy_dx alone)
        assert bool(seen["encoder.embeddings"].abs().sum() > 0)


def test_under_a_sample_budget_the_fused_step_runs_on_the_live_rows(hip):
    """mean_count > 0: the marcher hands back zero-padded buffers.  The networks, the warp kernel's sum and warp_backward's
    coefficient see the rows that hold a sample: the regulariser is 1e-3 reg_sum / (3 live rows), and loss and gradients are those of
    the trimmed step (mean_count 0) — the padded rows at x = 0 add nothing to either."""
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
        seen, regs, shapes = {}, [], []
        tr._reduce_and_step = lambda seen=seen, net=net: seen.update({k: p.grad.clone() for k, p in net.named_parameters()})
        fwd, reg_of = net.forward, tr._regularizer
        net.forward = lambda x, d, t=None, fwd=fwd, shapes=shapes: (shapes.append(x.shape[0]), fwd(x, d, t))[1]
        tr._regularizer = lambda reg_of=reg_of, regs=regs, net=net: (regs.append((net._deform_reg[0].detach().clone(), net._deform_reg[1],
                                                                                    net._last_deform.detach().clone())), reg_of())[1]
        torch.manual_seed(5)  # (the marcher's per-ray jitter: the same samples in both steps)
        loss = tr.train_step(ro, rd, gt, 0.2)
        runs[budget] = (loss.float(), seen, shapes[0], regs[0], int(net.step_counter[0, 0]))
    count = runs[0][4]
    live = (count + 127) // 128 * 128  # (the project's row-limit convention, and what the marcher keeps when it trims)
    assert runs[32768][4] == count and 0 < live < 32768
    assert runs[0][2] == live and runs[32768][2] == 32768 + 128 - 32768 % 128  # (what the marcher handed over)
    for budget in runs:
        reg_sum, rows, deform = runs[budget][3]
        assert rows == live and deform.shape == (live, 3)
        total = float(deform.double().abs().sum())
        assert abs(float(reg_sum) - total) <= 1e-6 * total
    assert torch.equal(runs[0][3][0], runs[32768][3][0]) and torch.equal(runs[0][3][2], runs[32768][3][2])
    torch.testing.assert_close(runs[32768][0], runs[0][0], rtol=1e-6, atol=0)
    for k, g in runs[0][1].items():
        other = runs[32768][1][k]
        if k == "encoder.embeddings":
            # the fp16 table gradient of a batch this small is summed by atomics: two runs of the SAME step differ by the roundings
            # of another order of additions (up to hundreds of terms per coarse cell), for which no tight bound follows from the
            # format.  The table gradient of the budgeted step is compared exactly where sums have a fixed order: on the CPU
            # (tests/test_dnerf.py).  Here: the same cells are touched, finite values.
            assert torch.isfinite(other).all() and bool(other.abs().sum() > 0)
            assert torch.equal((other != 0).any(1).view(-1)[:4096], (g != 0).any(1).view(-1)[:4096])  # (the dense coarsest level)
            continue
        # every other gradient is a fixed-order sum over the same rows, fed by the per-sample (atomic-free) input gradient
        assert torch.equal(other, g), k


# ---- renderer -----------------------------------------------------------------------------------------------------------------
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
    from dnerf.renderer import NeRFRenderer
    from nerf import synthetic as syn
    from nerf.renderer import NeRFRenderer as Ngp

    class Stub(NeRFRenderer):
        def forward(self, x, d, t=None):
            self.seen_t = self._bound_time if t is None else t
            self._deform_out = torch.zeros_like(x)
            return torch.full((x.shape[0],), 3.0, device=x.device), (d * 0.25 + 0.5)

    class NgpStub(Ngp):
        def forward(self, x, d):
            return torch.full((x.shape[0],), 3.0, device=x.device), (d * 0.25 + 0.5)
    model = Stub(bound=1, cuda_ray=True, time_size=2).cuda()
    boxes = (_box_bits([-0.6, -0.6, -0.6], [-0.1, 0.6, 0.6]), _box_bits([0.1, -0.6, -0.6], [0.6, 0.6, 0.6]))
    model.density_bitfield[0].copy_(boxes[0])
    model.density_bitfield[1].copy_(boxes[1])
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=512, generator=torch.Generator().manual_seed(3))
    ro, rd = r["rays_o"][0].contiguous().cuda(), r["rays_d"][0].contiguous().cuda()
    images = []
    for time, slot in ((0.2, 0), (0.8, 1)):
        base = NgpStub(bound=1, cuda_ray=True).cuda()
        base.density_bitfield.copy_(boxes[slot])
        model.train(train)
        base.train(train)
        with torch.no_grad():
            got = model.run_cuda(ro, rd, time, bg_color=1, perturb=False, max_steps=256)
            want = base.run_cuda(ro, rd, bg_color=1, perturb=False, max_steps=256)
        assert torch.equal(got["image"], want["image"]) and torch.equal(got["depth"], want["depth"])
        assert float(model.seen_t) == pytest.approx(time) and ("deform" in got) == train
        assert model.density_bitfield.shape == (2, 128 ** 3 // 8)
        images.append(got["image"])
    assert not torch.equal(images[0], images[1]) and float((images[0] - 1).abs().max()) > 0.1


def test_occupancy_update_follows_the_moving_box(hip):
    import raymarching
    from dnerf.renderer import NeRFRenderer

    class Stub(NeRFRenderer):
        def density(self, x, t=None):
            c = torch.stack([-0.6 + 1.2 * t.reshape(()), t.new_zeros(()), t.new_zeros(())])
            return {"sigma": ((x - c).abs().max(dim=-1).values < 0.2).float() * 100.0}

    def centre_cell(slot):
        w = torch.tensor([[-0.6 + 1.2 * (slot + 0.5) / 4, 0.0, 0.0]])
        coords = torch.round((w / (1 - 1 / 128) + 1) * 63.5).int().cuda()
        return int(raymarching.morton3D(coords)[0])

    def bit(model, slot, cell):
        return (int(model.density_bitfield[slot, cell // 8]) >> (cell % 8)) & 1
    a = Stub(bound=1, cuda_ray=True, time_size=4, density_thresh=10).cuda()
    b = Stub(bound=1, cuda_ray=True, time_size=4, density_thresh=10).cuda()
    torch.rand(5, device="cuda")  # (another consumer of torch's global stream between the two models' draws)
    for _ in range(16):
        b.update_extra_state()
    for _ in range(16):
        a.update_extra_state()
    assert torch.equal(a.density_grid, b.density_grid) and torch.equal(a.density_bitfield, b.density_bitfield)  # same seed, same buffers
    assert a.iter_density == 16 and float(a.density_grid.max()) == 100.0
    thresh = min(a.mean_density, a.density_thresh)
    for slot in range(4):
        assert torch.equal(a.density_bitfield[slot], raymarching.packbits(a.density_grid[slot], thresh))
        cell = centre_cell(slot)
        assert bit(a, slot, cell) == 1, slot
        # two slots on, the box has moved away by 0.6: further than its half size 0.2 plus the time jitter's 0.15
        assert bit(a, (slot + 2) % 4, cell) == 0, slot
    assert not torch.equal(a.density_bitfield[0], a.density_bitfield[3])


def test_training_smoke_on_two_flat_colours(hip):
    """64 x 64 frames at eight times, one flat colour before t = 0.5 and another from there on: 150 eager steps of 1,024 rays; the
    loss stays finite and the mean of the last 20 steps lies below the mean of the first 20 (a direction, not a magnitude)."""
    from dnerf.network import NeRFNetwork
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
    losses = []
    for step in range(150):
        batch = ds.collate([step % 8])
        losses.append(tr.train_step(batch["rays_o"][0], batch["rays_d"][0], batch["images"][0], batch["time"]))
    losses = torch.stack(losses).float().cpu()
    assert torch.isfinite(losses).all()
    first, last = float(losses[:20].mean()), float(losses[-20:].mean())
    print(f"[dnerf smoke] first 20: {first:.5f}  last 20: {last:.5f}")
    assert last < first
