"""GPU: the TensoRF CP backbone on the HIP path (csrc/tensorf_cp.hip, tensoRF/network_cp.py).

fp32 kernels against the float64 witness (tests/cp_witness.py): rtol 1e-4, atol 2e-5 * max |ref| (the numbers of
test_tensorf_vm_kernels_match_cpu_oracle); the fp16-basis path against the torch autocast sequence: rtol 2e-2,
atol 2e-3 * max |ref| (test_tensorf_color_features_with_basis_mat_in_the_kernel)."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import cp_witness as cw
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EDGE = [-1.0, 1.0, 0.0, -1.0001, 1.0001, -1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, 3.0]


def _points(N, res, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "one_cell":  # every point inside one cell of every line (maximum collision)
        lo = torch.tensor([-1 + 2 * (0.4 * (res[a] - 1) // 1) / max(res[a] - 1, 1) for a in range(3)])
        width = torch.tensor([2.0 / max(res[a] - 1, 1) for a in range(3)])
        return (lo + (0.05 + 0.9 * torch.rand(N, 3, generator=g)) * width).float()
    if kind == "spread":  # every point in a different 64-row chunk of every line
        n = min(N, min((r + 63) // 64 for r in res))
        k = torch.arange(n, dtype=torch.float32)
        return torch.stack([-1 + 2 * (64 * k + 5.3 + a) / (res[a] - 1) for a in range(3)], dim=1)
    x = torch.rand(N, 3, generator=g) * 2.1 - 1.05
    if N >= 40:  # rows exactly on u = +-1 / 0, just outside, far outside
        e = torch.tensor(EDGE)
        for a in range(3):
            x[a * 8:(a + 1) * 8, a] = e
        x[24:32] = e[:, None]
    return x


CASES = {
    "r8": ((20, 17, 13), 8, 300, "random"),
    "r24": ((20, 17, 13), 24, 300, "random"),
    "tiny": ((2, 3, 65), 4, 300, "random"),
    "default96": ((300, 299, 301), 96, 4096, "random"),
    "default288": ((300, 299, 301), 288, 4096, "random"),
    "n1": ((20, 17, 13), 8, 1, "random"),
    "n63": ((20, 17, 13), 8, 63, "random"),
    "n129": ((20, 17, 13), 8, 129, "random"),
    "one_cell": ((300, 299, 301), 24, 1000, "one_cell"),
    "spread": ((300, 299, 301), 24, 5, "spread"),
    "rank5": ((20, 17, 13), 5, 300, "random"),  # (not a multiple of four: the scalar reads of the forwards)
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs and the witness' results of a case, computed once"""
    res, R, N, kind = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000)
    lines = [(0.2 * torch.randn(1, R, res[a], 1, generator=g)) for a in cw.VEC_IDS]
    x = _points(N, res, kind, 11)
    N = x.shape[0]
    g1, gR = torch.randn(N, generator=g), torch.randn(N, R, generator=g)
    ln = [v[0, :, :, 0].numpy() for v in lines]
    ref = dict(feat=cw.features(x.numpy(), ln), prod=cw.products(x.numpy(), ln),
               g1=cw.line_grads(x.numpy(), ln, g1.numpy())[0], gR=cw.line_grads(x.numpy(), ln, gR.numpy().T)[0])
    return res, lines, x, g1, gR, ref


def _close(got, want, what):
    want = np.asarray(want)
    np.testing.assert_allclose(got.double().cpu().numpy().reshape(want.shape), want, rtol=1e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-30,
                               err_msg=what)


@pytest.mark.parametrize("shadows", [True, False], ids=["shadows", "plain"])
@pytest.mark.parametrize("name", list(CASES))
def test_cp_kernels_through_the_c_abi_match_the_witness(hip, name, shadows):
    be = hip.CpBackend
    res, lines, x, g1, gR, ref = _case(name)
    lines = [v.cuda() for v in lines]
    x, N, R = x.cuda(), x.shape[0], lines[0].shape[1]
    sh = be.transpose_lines(lines, res) if shadows else None
    if sh is not None:
        for a, t in zip(lines, sh):
            assert torch.equal(t, a[0, :, :, 0].t().contiguous())
    out1, outR = torch.full((N,), 7.0, device="cuda"), torch.full((R, N), 7.0, device="cuda")
    be.features_forward(x, lines, res, True, out1, shadows=sh)
    be.features_forward(x, lines, res, False, outR, shadows=sh)
    _close(out1, ref["feat"], "sigma_feat")
    _close(outR, ref["prod"], "products")
    bins = be.backward_bins(x, res)
    for reduce, g, key in ((True, g1, "g1"), (False, gR, "gR")):
        gl = be.features_backward(x, lines, res, reduce, g.cuda().contiguous(), bins=bins, shadows=sh)
        for i in range(3):
            assert gl[i].shape == lines[i].shape
            _close(gl[i], ref[key][i], f"{key} line {i}")
    gl2 = be.features_backward(x, lines, res, True, g1.cuda())  # (takes the bins itself)
    for a, b in zip(gl2, ref["g1"]):
        _close(a, b, "own bins")


def test_cp_binding_refuses_unequal_ranks_and_cpu_tensors(hip):
    be = hip.CpBackend
    res = (6, 5, 4)
    lines = [torch.randn(1, r, res[a], 1, device="cuda") for r, a in zip((4, 4, 8), cw.VEC_IDS)]
    x = torch.zeros(3, 3, device="cuda")
    with pytest.raises(RuntimeError, match="cp features_forward.*equal rank"):
        be.features_forward(x, lines, res, True, torch.empty(3, device="cuda"))
    import ctypes as C
    lib = hip.lib()
    ptr3, u3 = C.c_void_p * 3, C.c_uint32 * 3
    rc = lib.s3d_cp_features_forward(C.c_void_p(x.data_ptr()), C.c_uint32(3), ptr3(*[t.data_ptr() for t in lines]), u3(4, 4, 8), u3(*res),
                                     C.c_int(1), C.c_void_p(x.data_ptr()), None, None, None)
    assert rc != 0 and b"cp_features_forward" in lib.s3d_last_error() and b"equal" in lib.s3d_last_error()
    ok = [torch.randn(1, 4, res[a], 1) for a in cw.VEC_IDS]
    with pytest.raises(RuntimeError):
        be.features_forward(x.cpu(), ok, res, True, torch.empty(3))


@pytest.mark.parametrize("R,N", [(24, 300), (288, 1024)])
def test_cp_color_kernels_match_the_autocast_linear(hip, R, N):
    """s3d_cp_color_forward / _backward against the torch sequence under fp16 autocast (products in fp32, basis_mat as the
    autocast nn.Linear): rtol 2e-2, atol 2e-3 * max |ref|"""
    from tensoRF import network_cp as cp
    torch.manual_seed(R)
    res = [20, 17, 13] if R == 24 else [300, 299, 301]
    net = cp.NeRFNetwork(resolution=res, sigma_rank=[8] * 3, color_rank=[R] * 3, bound=1, cuda_ray=False).cuda()
    x = _points(N, res, "random", 5).cuda()
    go = (torch.randn(N, 27, generator=torch.Generator().manual_seed(6)) * 0.1).cuda()
    out = {}
    for fused in (True, False):
        net.fused_cp = fused
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            cf = net.get_color_feat(x)
        assert cf.dtype == torch.float16 and (type(cf.grad_fn).__name__ == "_CpColorBasisBackward") == fused
        (cf.float() * go).sum().backward()
        out[fused] = [cf.detach().float()] + [p.grad.float().clone() for p in list(net.color_vec) + [net.basis_mat.weight]]
    net.fused_cp = True
    for a, b, what in zip(out[True], out[False], ("features", "line 0", "line 1", "line 2", "basis_mat")):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-2, atol=2e-3 * float(b.abs().max()), err_msg=what)


@pytest.mark.parametrize("reduce", [True, False], ids=["sigma", "products"])
def test_cp_backward_keeps_gradients_far_below_the_batch_maximum(hip, reduce):
    """Each gradient cell within (n_cell + 8) * 2^-23 * sum |term| of the witness: the worst case of fp32 products and an fp32
    sum in ANY order.  `grad` is 2^-20 for the points of one cell of line 0 and O(1) elsewhere — what an accumulator scaled by
    the batch maximum loses.  The line values are positive (uniform in [0.5, 1.5]): a line value is itself an fp32 sum of two
    products, and only without cancellation INSIDE it is a term's rounding error proportional to the term, which is what the
    bound assumes; the gradients keep both signs, so the cells' sums cancel as they do in training."""
    be = hip.CpBackend
    res, R, N = (40, 33, 70), 24, 6000
    g = torch.Generator().manual_seed(17)
    lines = [0.5 + torch.rand(1, R, res[a], 1, generator=g) for a in cw.VEC_IDS]
    x = torch.rand(N, 3, generator=g) * 2.04 - 1.02
    grad = torch.randn(N, generator=g) if reduce else torch.randn(N, R, generator=g)
    i0 = cw.locate(x[:, 2].numpy(), res[2])[0]
    cell = 37
    small = torch.from_numpy(i0 == cell)
    assert 20 < int(small.sum()) < 400
    grad[small] = 2.0 ** -20
    ln = [v[0, :, :, 0].numpy() for v in lines]
    want, n_cell, abs_sum = cw.line_grads(x.numpy(), ln, grad.numpy() if reduce else grad.numpy().T)
    got = be.features_backward(x.cuda(), [v.cuda() for v in lines], res, reduce, grad.cuda().contiguous())
    for i in range(3):
        err = np.abs(got[i].double().cpu().numpy()[0, :, :, 0] - want[i])
        bound = (n_cell[i][None] + 8) * 2.0 ** -23 * abs_sum[i]
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"line {i}: worst error / bound {worst:.3f}")
        assert (err <= bound).all(), (i, worst)
    # (the batch is what it claims to be: the cell's own points add a share far below the cells' totals)
    only_small = cw.line_grads(x.numpy()[small.numpy()], ln, grad.numpy()[small.numpy()] if reduce else grad.numpy()[small.numpy()].T)[0][0]
    assert float(np.abs(only_small[:, cell]).min()) > 0 and float(np.abs(only_small).max()) < 2.0 ** -10 * float(np.abs(want[0]).max())


def _small_net(seed=1, res=32, **kw):
    from nerf import synthetic as syn
    from tensoRF import network_cp as cp
    torch.manual_seed(seed)
    net = cp.NeRFNetwork(resolution=[res] * 3, sigma_rank=[8] * 3, color_rank=[24] * 3, bound=1, cuda_ray=True, density_scale=1,
                         min_near=0.2, density_thresh=10, **kw).cuda()
    grid, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(grid))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    net.iter_density = 100
    net.mean_density = 5.0
    with torch.no_grad():
        for l in net.color_net:
            l.weight.mul_(3.0)  # (default init leaves the colours near 0.5: make the network matter)
    return net


def _graph_nodes(t):
    """names of the autograd nodes behind a tensor"""
    seen, todo = set(), [t.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        todo.extend(f for f, _ in n.next_functions)
    return {type(n).__name__ for n in seen}


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "fp16"])
def test_cp_network_fused_route_equals_the_grid_sample_route(hip, autocast):
    net = _small_net()
    N = 128 * 10
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(N, 3, generator=g) * 1.9 - 0.95).cuda()
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).cuda()
    ws, wr = torch.randn(N, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda()
    out = {}
    for fused in (True, False):
        net.fused_cp = fused
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            x_n = net._normalize(x)
            sf, cf = net.get_sigma_feat(x_n), net.get_color_feat(x_n)
            names = _graph_nodes(sf) | _graph_nodes(cf)
            if fused:
                assert type(sf.grad_fn).__name__ == "_CpFeaturesBackward"
                assert type(cf.grad_fn).__name__ == "_CpColorBasisBackward" if autocast else "_CpFeaturesBackward" in _graph_nodes(cf)
            else:
                assert not any(n.startswith("_Cp") for n in names), names
            sigma, rgb = net(x, d)
        ((sigma.float() * ws).sum() + (rgb.float() * wr).sum()).backward()
        out[fused] = (sigma.detach().float(), rgb.detach().float(), {k: p.grad.float().clone() for k, p in net.named_parameters()})
    net.fused_cp = True
    rtol, atol = (2e-2, 2e-3) if autocast else (1e-4, 2e-5)
    for a, b, what in ((out[True][0], out[False][0], "sigma"), (out[True][1], out[False][1], "rgb")):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=rtol, atol=atol * float(b.abs().max()), err_msg=what)
    assert set(out[True][2]) == set(out[False][2]) == {k for k, _ in net.named_parameters()}
    for k, b in out[False][2].items():
        np.testing.assert_allclose(out[True][2][k].cpu().numpy(), b.cpu().numpy(), rtol=rtol, atol=atol * float(b.abs().max()), err_msg=k)


def test_cp_coordinate_gradient_falls_back_to_the_torch_sequence(hip):
    net = _small_net()
    x = (torch.rand(256, 3, generator=torch.Generator().manual_seed(3)) * 1.8 - 0.9).cuda()
    res = {}
    for fused in (True, False):
        net.fused_cp = fused
        net.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        net.get_sigma_feat(xi).sum().backward()
        res[fused] = (xi.grad.clone(), [p.grad.clone() for p in net.sigma_vec])
    net.fused_cp = True
    torch.testing.assert_close(res[True][0], res[False][0], rtol=1e-4, atol=1e-6)
    for a, b in zip(res[True][1], res[False][1]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


def test_cp_padded_sample_batch_follows_the_device_side_count(hip):
    """s3d_hip.row_limit -> n_valid on the CP sample path: rows behind round_up(count, 128) are not written by the forwards
    (sentinel kept), the live rows equal the unpadded call bit for bit and the gradients equal those of the truncated batch"""
    import s3d_hip
    be = hip.CpBackend
    net = _small_net()
    g = torch.Generator().manual_seed(3)
    n0, live, M = 1000, 1024, 1024 + 640
    x = (torch.rand(live, 3, generator=g) * 1.9 - 0.95).cuda()
    d = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=-1).cuda()
    ws, wr = torch.randn(live, generator=g).cuda(), torch.randn(live, 3, generator=g).cuda()
    xp = torch.full((M, 3), float("nan"), device="cuda")
    xp[:live] = x
    counter = torch.tensor([n0, 0], dtype=torch.int32, device="cuda")
    # the forwards through the binding: a sentinel behind the live rows survives
    lines, cl = [p.detach() for p in net.sigma_vec], [p.detach() for p in net.color_vec]
    s1, sR = torch.full((M,), 7.0, device="cuda"), torch.full((8, M), 7.0, device="cuda")
    c16 = torch.full((M, 27), 7.0, dtype=torch.float16, device="cuda")
    xn = net._normalize(xp)
    be.features_forward(xn, lines, net.resolution, True, s1, n_valid=counter)
    be.features_forward(xn, lines, net.resolution, False, sR, n_valid=counter)
    be.color_forward(xn, cl, net.resolution, net.basis_mat.weight.detach().half(), c16, n_valid=counter)
    assert bool((s1[live:] == 7).all()) and bool((sR[:, live:] == 7).all()) and bool((c16[live:] == 7).all())
    assert bool(torch.isfinite(s1[:live]).all()) and bool(torch.isfinite(c16[:live].float()).all())
    res = {}
    for tag in ("plain", "padded"):
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            if tag == "plain":
                sigma, rgb = net(x, d[:live].contiguous())
            else:
                with s3d_hip.row_limit(counter, M):
                    sigma, rgb = net(xp, d)
        ((sigma[:live].float() * ws).sum() + (rgb[:live].float() * wr).sum()).backward()
        res[tag] = (sigma[:live].detach().float().clone(), rgb[:live].detach().float().clone(),
                    {n: p.grad.float().clone() for n, p in net.named_parameters() if p.grad is not None})
    assert torch.equal(res["plain"][0], res["padded"][0]) and torch.equal(res["plain"][1], res["padded"][1])
    assert set(res["plain"][2]) == set(res["padded"][2]) == {k for k, _ in net.named_parameters()}
    for n, a in res["plain"][2].items():
        b = res["padded"][2][n]
        assert bool(torch.isfinite(b).all()), n
        tol = (2e-3 if n.startswith("color_net") else 1e-5) * float(a.abs().max()) + 1e-12
        assert float((a - b).abs().max()) <= tol, (n, float((a - b).abs().max()), float(a.abs().max()))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["inside", "outside"])
def test_cp_backward_does_not_swallow_non_finite_gradients(hip, bad, where):
    """a NaN / inf in `grad`: the line gradient is non-finite or found_inf is raised — also for a point outside every line's
    range, which reaches no cell (torch's backward carries 0 * inf = NaN into the other lines there)"""
    be = hip.CpBackend
    res, lines, x, g1, gR, _ = _case("r8")
    lines, x = [v.cuda() for v in lines], x.clone()
    x[40] = torch.tensor([0.1, -0.2, 0.3]) if where == "inside" else torch.tensor([0.1, 5.0, 0.3])
    x = x.cuda()
    N = x.shape[0]
    for reduce, g in ((True, g1.clone()), (False, gR.clone())):
        g[40] = bad
        flag = torch.zeros(1, device="cuda")
        gl = be.features_backward(x, lines, res, reduce, g.cuda().contiguous(), found_inf=flag)
        assert float(flag) == 1.0 or not all(bool(torch.isfinite(t).all()) for t in gl)
    go = torch.zeros(N, 27, dtype=torch.float16, device="cuda")
    go[40, 3] = bad
    flag = torch.zeros(1, device="cuda")
    w = torch.randn(27, 8, device="cuda").half()
    gl, gw = be.color_backward(x, lines, res, w, go, found_inf=flag)
    assert float(flag) == 1.0 or not all(bool(torch.isfinite(t).all()) for t in list(gl) + [gw])


def _rays(n, seed=0):
    from nerf import synthetic as syn
    poses = syn.orbit_poses(2, seed=0)
    r = syn.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, N=n, generator=torch.Generator().manual_seed(seed))
    return r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous()


def test_cp_trainer_skips_the_step_on_a_non_finite_gradient(hip):
    """NativeGradScaler on a CP trainer: the factor gradients are not marked as checked, the scaler reads them itself; a
    non-finite colour line makes the step's gradients non-finite: no parameter moves, the scale backs off"""
    from tensoRF.utils import Trainer
    net = _small_net(seed=3)
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=1e-4, fp16=True, update_extra_interval=10 ** 9, native_optim=True)
    tr.global_step = 1
    ro, rd = _rays(512)
    gt = torch.rand(512, 3, generator=torch.Generator().manual_seed(1)).cuda()
    before = [p.detach().clone() for p in net.parameters()]
    tr.train_step(ro, rd, gt)
    assert any(not torch.equal(a.detach(), b) for a, b in zip(net.parameters(), before))  # (a finite step moves them)
    assert all("_s3d_grad_checked" not in p.__dict__ for p in net.parameters())
    with torch.no_grad():
        net.color_vec[1][0, 3, 7, 0] = float("inf")
    before = [p.detach().clone() for p in net.parameters()]
    scale0 = float(tr.scaler.get_scale())
    tr.train_step(ro, rd, gt)
    for a, b in zip(net.parameters(), before):
        assert torch.equal(a.detach(), b)
    assert float(tr.scaler.get_scale()) < scale0


def test_cp_train_step_with_l1_term_vs_the_reference_trainer(hip, monkeypatch):
    """tests/golden/tensorf_cp.npz: tensoRF/utils.py `Trainer.train_step` EXECUTED on the reference's CP network; here the
    build's trainer on the HIP path in fp32 — tolerances of test_tensorf_train_step_with_l1_term_vs_the_reference_trainer"""
    import raymarching.raymarching as rm
    import nerf.renderer as rend
    from nerf import synthetic as syn
    from tensoRF import network_cp as cp
    from tensoRF.utils import Trainer
    from test_gpu_golden import _CpuRandom   # the marcher's jitter drawn from the CPU generator, as the fixture's was
    T = np.load(os.path.join(GOLDEN, "tensorf_cp.npz"))
    net = cp.NeRFNetwork(resolution=[20, 17, 13], sigma_rank=[8] * 3, color_rank=[24] * 3, bound=1, cuda_ray=True, density_scale=1,
                         min_near=0.2, density_thresh=10)
    for k, p in net.named_parameters():
        g = torch.Generator().manual_seed(zlib.crc32(k.encode()) % 1000)
        p.data.copy_(torch.rand(*p.shape, generator=g) - 0.5)
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    net = net.cuda()
    with torch.no_grad():
        sg, cl = net(torch.from_numpy(T["fw_x"]).cuda(), torch.from_numpy(T["fw_d"]).cuda())
    np.testing.assert_allclose(sg.cpu().numpy(), T["fw_sigma"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(cl.cpu().numpy(), T["fw_color"], rtol=2e-5, atol=1e-6)
    assert abs(float(net.density_loss()) - float(T["density_loss"])) <= 1e-6 * float(T["density_loss"])
    net.mean_count = 32768
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=float(T["ts_l1_weight"]), fp16=False, update_extra_interval=10 ** 9)
    tr.global_step = 1
    net.train()
    proxy = _CpuRandom()
    monkeypatch.setattr(rm, "torch", proxy)
    monkeypatch.setattr(rend, "torch", proxy)
    torch.manual_seed(5)
    seen = {}
    monkeypatch.setattr(tr, "_reduce_and_step", lambda: seen.update(
        {k: (p.grad if p.grad is not None else p._s3d.grad).detach().float().clone() for k, p in net.named_parameters()}))
    ro, rd, gt = (torch.from_numpy(T[k]).cuda() for k in ("ts_rays_o", "ts_rays_d", "ts_images"))
    loss = tr.train_step(ro[0].contiguous(), rd[0].contiguous(), gt[0].contiguous())
    assert np.array_equal(net.step_counter[0].cpu().numpy(), T["ts_counter"])
    assert abs(float(loss) - float(T["ts_loss"])) <= 1e-5 * float(T["ts_loss"])
    scale = float(tr.scaler.get_scale()) if hasattr(tr.scaler, "get_scale") else 1.0
    assert set(seen) == set(T["param_names"].tolist())
    for k, g in seen.items():
        key = "ts_grad_" + k.replace(".", "_")
        g = (g / scale).reshape(-1).cpu()
        if key in T.files:
            want = torch.from_numpy(T[key])
        else:
            want, g = torch.from_numpy(T[key + "_at_values"]), g[torch.from_numpy(T[key + "_at"])]
        assert float((g - want).abs().max()) <= 2e-4 * float(want.abs().max()) + 1e-9, k


def _trained(kind, steps=12, n=256):
    """12 steps on a small CP model with one scheduled shrink + upsample after step 6.  kind: 'graph' (replayed), 'recapture'
    (the graphed trainer's step body run eagerly every time: the same jitter from the device step counter) or 'eager' (Trainer)"""
    from tensoRF.utils import GraphedTrainer, Trainer
    ro, rd = _rays(n)
    gt = torch.rand(n, 3, generator=torch.Generator().manual_seed(9)).cuda()
    net = _small_net(seed=7)
    kw = dict(lr0=2e-2, lr1=1e-3, l1_reg_weight=1e-4, fp16=True, update_extra_interval=10 ** 9, upsample_model_steps=[7],
              upsample_resolutions=[40])
    tr = Trainer(net, **kw) if kind == "eager" else GraphedTrainer(net, n, **kw)
    tr.global_step = 1
    net.mean_count = n * 40
    torch.manual_seed(4)
    losses, shapes = [], []
    for _ in range(steps):
        if kind == "recapture":
            tr.graph = None
        losses.append(float(tr.train_step(ro, rd, gt)))
        shapes.append(tuple(net.resolution))
    torch.cuda.synchronize()
    return net, tr, losses, shapes


def test_cp_graphed_trainer_with_a_scheduled_upsample(hip):
    net_g, tr_g, l_g, s_g = _trained("graph")
    assert tr_g.n_captures == 2 and tr_g.graph is not None  # (captured, dropped by the upsampling, captured again)
    assert s_g[4] == (32, 32, 32) and s_g[5] != (32, 32, 32) and s_g[-1] == s_g[5]  # (after the sixth step)
    assert [v.shape[2] for v in net_g.sigma_vec] == [net_g.resolution[a] for a in (2, 1, 0)]
    assert [id(p) for grp in tr_g.optimizer.param_groups for p in grp["params"]] == [id(p) for p in net_g.parameters()]
    assert np.isfinite(l_g).all()
    # the same steps, each run eagerly on the stream with the replay's jitter (tolerance of
    # test_graphed_replay_equals_the_eager_step_with_background)
    _, tr_r, l_r, s_r = _trained("recapture")
    assert tr_r.n_captures == 12 and s_r == s_g
    print("graphed", l_g, "\nrecapture", l_r)
    np.testing.assert_allclose(l_g, l_r, rtol=1e-3)
    # the eager Trainer from the same seed: the same schedule, the same losses
    _, _, l_e, s_e = _trained("eager")
    print("eager", l_e)
    assert s_e == s_g and np.isfinite(l_e).all()
    np.testing.assert_allclose(l_g, l_e, rtol=1e-3)


def test_cp_save_mesh_writes_a_ply(hip, tmp_path):
    from nerf.mesh import read_ply
    from tensoRF.utils import Trainer
    net = _small_net(seed=7)
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, fp16=True, update_extra_interval=10 ** 9)
    path = tr.save_mesh(save_path=str(tmp_path / "cp.ply"), resolution=32, threshold=1.0)  # sigma = exp(feat): the feat > 0 region
    v, t = read_ply(path)
    assert len(v) > 0 and len(t) > 0 and t.min() >= 0 and t.max() < len(v)
    assert np.isfinite(v).all() and float(np.abs(v).max()) <= 1.0 + 1e-6


@pytest.mark.parametrize("kind", ["vm", "cp"])
def test_tensorf_backbones_take_one_sort_and_one_shadow_set_per_factor_set_and_step(hip, kind):
    """what the shared host path of the two backbones (tensoRF/network.py: TensoRFCommon) shares within a step, counted at the
    backend classes — replaced on the class, so the networks must look the backend up at call time: the density and the colour
    backward use ONE sort of the points, each factor set's shadows are taken once (in the forward, reused by the backward), and
    the sorted-point cache on the network is empty when both consumers have run.  Numbers cannot show any of this."""
    import s3d_hip
    from tensoRF import network as vm, network_cp as cp
    key = vm.BINS
    torch.manual_seed(5)
    if kind == "vm":
        net = vm.NeRFNetwork(resolution=[24, 20, 16], sigma_rank=[8] * 3, color_rank=[16] * 3, bound=1, cuda_ray=True).cuda()
        be, transpose = hip.VmBackend, "transpose_factors"
    else:
        net = cp.NeRFNetwork(resolution=[24, 20, 16], sigma_rank=[8] * 3, color_rank=[32] * 3, bound=1, cuda_ray=True).cuda()
        be, transpose = hip.CpBackend, "transpose_lines"
    N, live = 384, 256
    g = torch.Generator().manual_seed(6)
    xs = [(torch.rand(N, 3, generator=g) * 2 - 1).cuda() for _ in range(2)]
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).cuda()
    ws, wr = torch.randn(N, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda()
    counts, saved = {"backward_bins": 0, transpose: 0}, {n: be.__dict__[n] for n in ("backward_bins", transpose)}

    def counting(name, fn):
        def wrapper(*a, **kw):
            counts[name] += 1
            return fn(*a, **kw)
        return staticmethod(wrapper)

    def step(x, dirs, rows=N, sigma_only=False):
        """(sorts, transposes) of one forward + backward on the first `rows` rows"""
        net.zero_grad(set_to_none=True)
        before = dict(counts)
        with torch.autocast("cuda", dtype=torch.float16):
            sigma, rgb = net(x, dirs)
        prefix = "_Vm" if kind == "vm" else "_Cp"  # (the fused routes: the density features and the basis_mat Function)
        assert prefix + "FeaturesBackward" in _graph_nodes(sigma) and prefix + "ColorBasisBackward" in _graph_nodes(rgb)
        loss = (sigma[:rows].float() * ws[:rows]).sum()
        (loss if sigma_only else loss + (rgb[:rows].float() * wr[:rows]).sum()).backward()
        return counts["backward_bins"] - before["backward_bins"], counts[transpose] - before[transpose]

    try:
        for name, fn in saved.items():
            setattr(be, name, counting(name, getattr(be, name)))
        for x in xs:  # (new points the second time: another cache entry, the first one let go)
            assert step(x, d) == (1, 2)
            assert net.__dict__[key] == {}
        before = dict(counts)
        with torch.no_grad():
            net.density(xs[0])
        assert (counts["backward_bins"] - before["backward_bins"], counts[transpose] - before[transpose]) == (0, 1)
        # the density's backward alone: one consumer of two, the entry waits for the second and the next forward drops it
        assert step(xs[0], d, sigma_only=True) == (1, 2)
        assert [e[2] for e in net.__dict__[key].values()] == [1]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            net(xs[1], d)
        assert net.__dict__[key] == {}
        # a padded batch (s3d_hip.row_limit): still one sort, and the gradients of the rows in front of round_up(count, 128)
        xp = xs[0].clone()
        xp[live:] = float("nan")
        with s3d_hip.row_limit(torch.tensor([200, 0], dtype=torch.int32, device="cuda"), N):
            assert step(xp, d, rows=live)[0] == 1
        padded = {n: p.grad.float().clone() for n, p in net.named_parameters() if p.grad is not None}
        step(xs[0][:live].contiguous(), d[:live].contiguous(), rows=live)
        plain = {n: p.grad.float().clone() for n, p in net.named_parameters() if p.grad is not None}
    finally:
        for name, fn in saved.items():
            setattr(be, name, fn)
    assert set(plain) == set(padded) == {n for n, _ in net.named_parameters()}
    for n, a in plain.items():  # (tolerances of test_cp_padded_sample_batch_follows_the_device_side_count)
        b = padded[n]
        assert bool(torch.isfinite(b).all()), n
        tol = (2e-3 if n.startswith("color_net") else 1e-5) * float(a.abs().max()) + 1e-12
        assert float((a - b).abs().max()) <= tol, (n, float((a - b).abs().max()), float(a.abs().max()))
