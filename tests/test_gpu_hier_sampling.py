"""GPU: the kernels of csrc/hiersample.hip — the sampling path without the occupancy grid — stage by stage against the torch ops
(bit for bit where the arithmetic is elementwise) and the float64 witness (tests/hier_witness.py), and `NeRFRenderer.run` on the
native route against its torch route on the same GPU.  Inputs, the witness tolerances and their provenance: tests/hier_cases.py."""
import os

import numpy as np
import pytest
import torch

import hier_cases as C
import hier_witness as W
from conftest import GOLDEN
from hier_cases import gauss_renderer

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def dev(a, dtype=None):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype).cuda()


def filled(*shape, dtype=torch.float32):
    """an output buffer pre-filled with a sentinel: a slot no lane wrote shows"""
    if dtype == torch.bool:
        return torch.ones(shape, dtype=torch.uint8, device="cuda") * 7
    return torch.full(shape, SENTINEL if dtype == torch.float32 else -7, dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def points(o, d, z, aabb):
    x = o.unsqueeze(-2) + d.unsqueeze(-2) * z.unsqueeze(-1)
    return torch.min(torch.max(x, aabb[:3]), aabb[3:])


COARSE_CASES = sorted({(n, s, kind) for (n, s, _, kind) in C.CASES})


@pytest.mark.parametrize("perturb", [False, True], ids=["plain", "jitter"])
@pytest.mark.parametrize("case", COARSE_CASES, ids=lambda c: f"N{c[0]}-S{c[1]}-{c[2]}")
def test_coarse_samples_equal_the_torch_ops_bit_for_bit(hip, case, perturb):
    """(a): nears, fars, z and xyz against near_far_from_aabb + the torch ops of `_run_torch` on the GPU, every bit: the kernel
    rounds each operation on its own, as the op sequence does, and forms torch.linspace's values the way torch does"""
    import raymarching
    N, S, kind = case
    o, d = (dev(v) for v in C.rays(N, kind))
    aabb = dev(C.AABB)
    noise = torch.rand(N, S, generator=torch.Generator().manual_seed(S)).cuda() if perturb else None
    nears, fars, z, xyz = filled(N), filled(N), filled(N, S), filled(N, S, 3)
    hip.HierBackend.coarse_samples(o, d, aabb, C.MIN_NEAR, S, nears, fars, z, xyz, noise)
    want_near, want_far = raymarching.near_far_from_aabb(o, d, aabb, C.MIN_NEAR)
    wn, wf = want_near.unsqueeze(-1), want_far.unsqueeze(-1)
    want_z = wn + (wf - wn) * torch.linspace(0.0, 1.0, S, device="cuda").unsqueeze(0).expand((N, S))
    if perturb:
        want_z = want_z + (noise - 0.5) * ((wf - wn) / S)
    assert torch.equal(nears, want_near) and torch.equal(fars, want_far)
    assert torch.equal(z, want_z), float((z - want_z).abs().max())
    assert torch.equal(xyz, points(o, d, want_z, aabb))
    miss = host(want_near) == np.float32(C.FLT_MAX)
    assert miss.any() == (kind != "inside") and (not miss[1:].any() or kind == "miss")


@pytest.mark.parametrize("given_u", [False, True], ids=["deterministic", "given-u"])
@pytest.mark.parametrize("case", C.UPSAMPLE_CASES, ids=C.case_id)
def test_upsample_matches_the_witness_and_merges_exactly(hip, case, given_u):
    """(b) on well-conditioned input: new_z within KERNEL_MARGIN x the torch fp32 ops' own error of the float64 witness (in units
    of the ray's length); new_xyz the clamped points of new_z bit for bit; z_sorted non-decreasing; order a permutation with
    cat(z, new_z)[order] == z_sorted exactly; no slot left unwritten"""
    N, S, U, kind = case
    K = S + U
    inp = C.upsample_inputs(N, S, U, kind)
    t = {k: dev(v) for k, v in inp.items()}
    aabb = dev(C.AABB)
    new_z, new_xyz, z_sorted, order = filled(N, U), filled(N, U, 3), filled(N, K), filled(N, K, dtype=torch.int32)
    hip.HierBackend.upsample(t["z"], t["sigma"], t["nears"], t["fars"], C.SCALE, t["u"] if given_u else None, t["rays_o"], t["rays_d"],
                             aabb, U, new_z, new_xyz, z_sorted, order)
    ref = W.upsample(inp["z"], inp["sigma"], inp["nears"], inp["fars"], C.SCALE, inp["u"] if given_u else None, U, inp["rays_o"],
                     inp["rays_d"], C.AABB)[0]
    err = C.err_new_z(host(new_z), ref, inp)
    print(f"new_z: error {err:.3e} of the ray's length, bound {C.bound('new_z'):.3e}")
    assert err <= C.bound("new_z")
    assert torch.equal(new_xyz, points(t["rays_o"], t["rays_d"], new_z, aabb))
    assert bool((z_sorted[:, 1:] >= z_sorted[:, :-1]).all())
    assert torch.equal(torch.sort(order.long(), dim=1).values, torch.arange(K, device="cuda").expand(N, K))
    assert torch.equal(torch.gather(torch.cat([t["z"], new_z], dim=1), 1, order.long()), z_sorted)
    if not given_u:  # (the deterministic row gives sorted fine samples)
        assert bool((new_z[:, 1:] >= new_z[:, :-1]).all())


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_weights_compositing_and_backward_match_the_witness(hip, case):
    """(c), (d) and the backward on given merged rows, sigma from empty to opaque (s reaches 1e-15): each within KERNEL_MARGIN x
    the torch fp32 ops' own error of the float64 witness.  The ray that misses the box has a NaN depth and (with a depth
    gradient) NaN sigma gradients, as autograd gives; everything else is finite."""
    N, S, U, kind = case
    K = S + U
    inp = C.composite_inputs(N, S, U, kind)
    ref = C.witness_composite(inp, S)
    t = {k: dev(v) for k, v in inp.items()}
    H = hip.HierBackend
    weights, mask = filled(N, K), filled(N, K, dtype=torch.bool)
    H.weights(t["z_sorted"], t["order"], t["sigma_cat"], t["nears"], t["fars"], C.SCALE, S, weights, mask)
    err = C.err_abs(host(weights), ref["weights"])
    print(f"weights: error {err:.3e}, bound {C.bound('weights'):.3e}")
    assert err <= C.bound("weights")
    assert torch.equal(mask, (weights > 1e-4).to(torch.uint8))
    clear = np.abs(ref["weights"] - 1e-4) > C.bound("weights")
    assert np.array_equal(host(mask).astype(bool)[clear], ref["mask"][clear])
    ws, depth, image = filled(N), filled(N), filled(N, 3)
    H.composite_forward(weights, t["rgbs"], t["z_sorted"], t["order"], t["nears"], t["fars"], S, ws, depth, image)
    hit = inp["nears"] < C.FLT_MAX
    assert np.isnan(host(depth)[~hit]).all() and np.isfinite(host(image)).all() and np.isfinite(host(ws)).all()
    for key, got in (("weights_sum", ws), ("depth", depth), ("image", image)):
        err = C.err_abs(host(got), ref[key])
        print(f"{key}: error {err:.3e}, bound {C.bound('composite'):.3e}")
        assert err <= C.bound("composite"), key
    g_sigma, g_rgbs = filled(N, K), filled(N, K, 3)
    H.composite_backward(t["grad_image"], t["grad_weights_sum"], t["grad_depth"], t["sigma_cat"], t["rgbs"], t["z_sorted"], t["order"],
                         t["nears"], t["fars"], C.SCALE, S, g_sigma, g_rgbs)
    assert np.isfinite(host(g_sigma)[hit]).all() and np.isfinite(host(g_rgbs)).all()
    for key, got in (("grad_sigma", g_sigma), ("grad_rgbs", g_rgbs)):
        err = C.err_rel(host(got), ref[key])
        print(f"{key}: relative error {err:.3e}, bound {C.bound(key):.3e}")
        assert err <= C.bound(key), key
    # the image's gradient alone (what a colour loss sends): the other two absent, and no NaN on the missing ray
    g_sigma, g_rgbs = filled(N, K), filled(N, K, 3)
    H.composite_backward(t["grad_image"], None, None, t["sigma_cat"], t["rgbs"], t["z_sorted"], t["order"], t["nears"], t["fars"],
                         C.SCALE, S, g_sigma, g_rgbs)
    want = W.composite_backward(inp["grad_image"], None, None, inp["sigma_cat"], inp["rgbs"], inp["z_sorted"], inp["order"],
                                inp["nears"], inp["fars"], C.SCALE, S)
    assert np.isfinite(host(g_sigma)).all()
    assert C.err_rel(host(g_sigma), want[0]) <= C.bound("grad_sigma") and C.err_rel(host(g_rgbs), want[1]) <= C.bound("grad_rgbs")


def test_entry_points_refuse_rows_above_the_cap(hip):
    import ctypes as ct
    lib = hip.lib()
    cap = hip.HierBackend.max_samples()
    x = torch.zeros(8, device="cuda")
    p = ct.c_void_p(x.data_ptr())
    rc = lib.s3d_hier_weights(p, p, p, p, p, ct.c_float(1.0), ct.c_uint32(1), ct.c_uint32(cap), ct.c_uint32(1), p, p, None)
    assert rc == 3 and b"hier_weights" in lib.s3d_last_error() and b"exceeds" in lib.s3d_last_error()  # S3D_ERR_UNSUPPORTED
    rc = lib.s3d_hier_coarse_samples(p, p, p, ct.c_uint32(1), ct.c_float(0.2), ct.c_uint32(2), None, p, p, p, p, None)
    assert rc == 1  # S3D_ERR_INVALID: fewer than three steps


# ---- the whole route ------------------------------------------------------------------------------------------------------
def both_routes(model, call):
    """`call(model)` on the native and on the torch route, same seed: the jitter is drawn on the device and the pdf's uniforms on
    the host by both, in the same order"""
    out = {}
    for route, native in (("native", True), ("torch", False)):
        model.native_sampling = native
        torch.manual_seed(11)
        out[route] = call(model)
        assert model.last_sampling_route == route
    model.native_sampling = True
    return out["native"], out["torch"]


def assert_every_pixel(got, ref, key):
    got, ref = host(got.float()), host(ref.float())
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), key
    scale = max(float(np.nanmax(np.abs(ref))), 1e-30)
    worst = float(np.nanmax(np.abs(got - ref))) / scale
    print(f"{key}: worst pixel {worst:.3e} of the range")
    assert worst <= 1e-4, (key, worst)


def assert_opaque_allowance(got, ref, key):
    """tests/test_gpu_golden.py::test_sampling_path_without_occupancy_grid_vs_reference_fixture's allowance: at most 0.2 % of the
    entries beyond 1e-4 of the range (a sample on the other side of a near-empty pdf bin), none beyond 2e-2"""
    got, ref = host(got.float()), host(ref.float())
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), key
    d = np.abs(np.nan_to_num(got) - np.nan_to_num(ref))
    scale = max(float(np.nanmax(np.abs(ref))), 1e-30)
    print(f"{key}: {float((d > 1e-4 * scale).mean()):.5f} of the entries beyond 1e-4, worst {float(d.max()) / scale:.3e}")
    assert float((d > 1e-4 * scale).mean()) <= 2e-3, (key, float((d > 1e-4 * scale).mean()), float(d.max()))
    assert float(d.max()) <= 2e-2 * scale, (key, float(d.max()))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_run_native_equals_torch_route_on_the_semi_transparent_scene(hip, train):
    """sigma(x) = 2.5 exp(-|x|^2 / (2 0.3^2)): no ray above weights_sum 0.9 (checked on the CPU in tests/test_hier_sampling.py and
    here), so no pdf bin falls under the 1e-5 rule and the sampling is continuous in rounding — EVERY pixel of image, depth and
    weights_sum within 1e-4 of the value range, the missing ray's depth NaN on both routes"""
    N, S, U = 1500, 64, 48
    o, d = (dev(v) for v in C.rays(N, "mixed"))
    R = gauss_renderer().cuda()
    R.train(train)
    with torch.no_grad():
        got, ref = both_routes(R, lambda m: m.run(o, d, num_steps=S, upsample_steps=U, bg_color=1, perturb=train))
    assert 0.5 < float(ref["weights_sum"].max()) <= 0.9
    assert bool(torch.isnan(ref["depth"][0])) and bool(torch.isfinite(got["image"]).all())
    for key in ("image", "depth", "weights_sum"):
        assert_every_pixel(got[key], ref[key], key)


def test_run_native_equals_torch_route_on_the_opaque_scene(hip):
    """the opaque boxes of the reference fixture (sigma 40; the rays and the seed of tests/test_gpu_golden.py, for which the torch
    route on the CPU equals the fixture bit for bit: tests/test_golden_wrappers.py), eval staged in 1,500-ray chunks and a
    perturbed training batch: the allowance the project already uses for this path"""
    from nerf import renderer, synthetic as syn
    lo, hi = syn.lego_like_boxes(0)

    class AnalyticRun(renderer.NeRFRenderer):
        def density(self, x):
            return {"sigma": syn.box_density(x, lo, hi, sigma=40.0)}

        def color(self, x, dd, mask=None, **kw):
            rgb = (x * 0.5 + 0.5).clamp(0, 1) * (0.5 + 0.5 * dd.abs())
            if mask is None:
                return rgb
            out = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            out[mask] = rgb[mask]
            return out
    G = np.load(os.path.join(GOLDEN, "wrappers.npz"))
    ro, rd = torch.from_numpy(G["march_ro"]).cuda(), torch.from_numpy(G["march_rd"]).cuda()
    R = AnalyticRun(bound=1, cuda_ray=False, density_scale=1, min_near=0.2).cuda()
    R.eval()
    with torch.no_grad():
        got, ref = both_routes(R, lambda m: m.render(ro[None], rd[None], staged=True, max_ray_batch=1500, bg_color=1, perturb=False,
                                                     num_steps=64, upsample_steps=48))
    assert float(torch.nan_to_num(ref["image"]).std()) > 0.05
    for key in ("image", "depth"):
        assert_opaque_allowance(got[key][0], ref[key][0], "eval " + key)
    R.train()
    with torch.no_grad():
        got, ref = both_routes(R, lambda m: m.render(ro[None, :1024], rd[None, :1024], bg_color=1, perturb=True, num_steps=64,
                                                     upsample_steps=48))
    assert float(ref["weights_sum"].max()) > 0.5
    for key in ("image", "depth", "weights_sum"):
        assert_opaque_allowance(got[key], ref[key], "train " + key)


def small_ngp():
    from nerf.network import NeRFNetwork
    torch.manual_seed(3)
    return NeRFNetwork(bound=1, cuda_ray=False, log2_hashmap_size=14, density_scale=1, min_near=0.2).cuda()


class _GivenRandom:
    """stand-in for the `torch` name inside nerf.renderer: `rand` hands out the given tensors in turn (the jitter, then the pdf's
    uniforms), so that every run of a comparison gets the same draws, in the dtype it computes in"""

    def __init__(self, draws):
        self.draws = list(draws)

    def __getattr__(self, k):
        return getattr(torch, k)

    def rand(self, *a, **kw):
        t = self.draws.pop(0)
        assert tuple(t.shape) == tuple(a[0])
        return t.to(kw["device"]) if kw.get("device") is not None else t


class _Float64Sampling:
    """Runs a model's torch route with the SAMPLING arithmetic in float64 — depths, weights, pdf, inverse CDF, sort, compositing —
    around networks that stay what they are: rays and draws go in as float64, the slab test and the networks get fp32 inputs
    and hand float64 back (the hash-grid kernels have no float64; autograd passes through the casts)."""

    def __init__(self, rend, net):
        self.rend, self.net, self.raymarching = rend, net, rend.raymarching

    def __enter__(self):
        import types
        rm, net = self.raymarching, self.net
        density, color = net.density, net.color

        def near_far(o, d, aabb, min_near):
            return tuple(t.double() for t in rm.near_far_from_aabb(o.float(), d.float(), aabb, min_near))
        self.rend.raymarching = types.SimpleNamespace(near_far_from_aabb=near_far, sph_from_ray=rm.sph_from_ray)
        net.density = lambda x: {k: v.double() for k, v in density(x.float()).items()}
        net.color = lambda x, d, mask=None, **dens: color(x.float(), d.float(), mask=mask, **{k: v.float() for k, v in dens.items()}).double()
        return self

    def __exit__(self, *exc):
        del self.net.density, self.net.color
        self.rend.raymarching = self.raymarching


def test_parameter_gradients_through_the_whole_route(hip, monkeypatch):
    """a small NGP network under fp16 autocast, 256 rays at (S, U) = (32, 16), training mode with jitter: loss.backward() on the
    native route against the torch route, same draws.  Tolerance, measured in the test itself on the reference: the torch route in
    fp32 against the same route with its sampling arithmetic in float64 (`_Float64Sampling`; the networks cannot run in float64,
    the hash-grid kernels have none).  That is the error fp32 sampling has anyway — above all the last bits of the new depths,
    which the finest hash level (resolution 2,048) turns into 1e-3 of a sample's share of a table cell — and the native route is
    allowed KERNEL_MARGIN times it, per tensor, relative to nothing but that.  (Measured on an MI355X: the routes' sigma and
    geo_feat gradients agree per sample to 7e-6 of the largest, their new points to 1.2e-6; the density table's gradient then
    differs by 0.9 % of its largest entry on either route against the other.)  The loss is scaled by 2^16, GradScaler's initial
    scale, as every fp16 training step of the project is: unscaled, the fp16 gradients (3e-6 at most here) sit in binary16's
    subnormal range and the first density layer's gradient is zero outright."""
    import nerf.renderer as rend
    LOSS_SCALE = 65536.0
    N, S, U = 256, 32, 16
    o, d = (dev(v) for v in C.rays(N, "mixed"))
    g = torch.Generator().manual_seed(9)
    target, noise, u = torch.rand(N, 3, generator=g).cuda(), torch.rand(N, S, generator=g), torch.rand(N, U, generator=g)
    net = small_ngp().train()

    def step(native, dtype=torch.float32):
        net.native_sampling = native
        net.zero_grad(set_to_none=True)
        with monkeypatch.context() as m:
            m.setattr(rend, "torch", _GivenRandom([noise.to(dtype), u.to(dtype)]))
            with torch.autocast("cuda", dtype=torch.float16):
                out = net.run(o.to(dtype), d.to(dtype), num_steps=S, upsample_steps=U, bg_color=1, perturb=True)
                loss = ((out["image"].float() - target) ** 2).mean()
            (loss * LOSS_SCALE).backward()
        assert net.last_sampling_route == ("native" if native else "torch")
        return float(loss.detach()), {k: p.grad.detach().float().clone() for k, p in net.named_parameters() if p.grad is not None}
    loss_t, grads_t = step(False)
    with _Float64Sampling(rend, net):
        loss_64, grads_64 = step(False, torch.float64)
    loss_n, grads_n = step(True)
    net.native_sampling = True
    print(f"loss: native {loss_n:.8f}, torch {loss_t:.8f}, torch with float64 sampling {loss_64:.8f}")
    assert abs(loss_n - loss_t) <= 1e-4 * abs(loss_t) and abs(loss_64 - loss_t) <= 1e-4 * abs(loss_t)
    assert set(grads_n) == set(grads_t) == set(grads_64)
    assert any("encoder.embeddings" in k for k in grads_t) and any("color_net" in k for k in grads_t)
    failed = []
    for k, ref in grads_t.items():
        top = float(ref.abs().max())
        own = float((grads_64[k] - ref).abs().max())
        err = float((grads_n[k] - ref).abs().max())
        print(f"{k}: max |ref| {top:.3e}, torch fp32 against float64 sampling {own:.3e}, native against torch {err:.3e}, "
              f"allowed {C.KERNEL_MARGIN * own:.3e}")
        assert top > 0 and bool(torch.isfinite(grads_n[k]).all()), k
        if err > C.KERNEL_MARGIN * own:
            failed.append(k)
    assert not failed, failed


def test_eager_trainer_learns_through_the_native_route(hip):
    """30 eager steps of the Trainer on the synthetic scene with cuda_ray off: the loss is finite and lower at the end, and the
    native route is the one that ran"""
    from nerf import synthetic as syn
    from nerf.trainer import Trainer
    net = small_ngp()
    tr = Trainer(net, lr=1e-2, fp16=True)
    lo, hi = syn.lego_like_boxes(0)
    r = syn.get_rays(syn.orbit_poses(1, seed=0).cuda(), syn.lego_intrinsics(), 800, 800, N=1024, generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    with torch.no_grad():  # targets: the opaque boxes rendered by the analytic scene's torch route would do; a flat colour is enough
        gt = (0.5 + 0.5 * rd.abs()).clamp(0, 1) * 0.3
    losses = [float(tr.train_step(ro, rd, gt)) for _ in range(30)]
    assert net.last_sampling_route == "native"
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < losses[0], losses


def test_dnerf_render_native_equals_torch_route(hip):
    """the D-NeRF renderer reaches the route through super().run: render(..., num_steps=16, upsample_steps=16) native against the
    torch route, the allowance of the opaque scene; `deform` comes back for every sample on both routes"""
    from dnerf.network import NeRFNetwork
    from gridencoder import GridEncoder
    torch.manual_seed(4)
    net = NeRFNetwork(bound=1, cuda_ray=False, density_scale=1, min_near=0.2)
    net.encoder = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=14, desired_resolution=256,
                              gridtype="tiled")  # (a small table: the test is about the route, not the backbone)
    net = net.cuda().eval()
    N = 512
    o, d = (dev(v) for v in C.rays(N, "mixed"))
    time = torch.tensor([[0.4]], device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        got, ref = both_routes(net, lambda m: m.render(o[None], d[None], time, bg_color=1, perturb=False, num_steps=16, upsample_steps=16))
    for key in ("image", "depth"):
        assert_opaque_allowance(got[key][0], ref[key][0], key)
    assert got["deform"].shape == ref["deform"].shape and got["deform"].shape[0] == N * 32
