"""GPU: the CCNeRF backbone on the HIP path (csrc/tensorf_cc.hip, tensoRF/network_cc.py).

fp32 kernels through the C ABI against the float64 witness (tests/cc_witness.py): rtol 1e-4, atol 2e-5 * max |ref|; the fp16 path
against the torch autocast sequence: rtol 2e-2, atol 2e-3 * max |ref| — both pairs are the numbers of tests/test_gpu_tensorf_cp.py."""
import copy
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import cc_witness as cw
from conftest import GOLDEN
from test_ccnerf import NET, _net, compose_scene, edge_points, witness_groups

pytestmark = pytest.mark.gpu

# group sizes (vector, matrix) per level
LAYOUTS = {
    "k1": ([8], [5]),                                    # one group: a finalized model
    "k3": ([2, 0, 3], [0, 3, 0]),                        # no matrix group at level 0, no vector group at level 1
    "ranks": ([2, 3, 5, 8, 40], [3, 2, 8, 2, 35]),       # group ranks 2, 3, 5, 8 and two above 32
}
# name: (resolution, layout, N, degree)
CASES = {
    "k3_d4": ((20, 17, 13), "k3", 300, 4),
    "k3_d1": ((20, 17, 13), "k3", 300, 1),
    "k1_d4": ((20, 17, 13), "k1", 300, 4),
    "ranks_d4": ((12, 20, 16), "ranks", 300, 4),
    "ranks_d1": ((12, 20, 16), "ranks", 129, 1),
    "flat_a": ((1, 2, 65), "k3", 300, 4),
    "flat_b": ((65, 1, 2), "k3", 300, 1),
    "flat_c": ((2, 65, 1), "k1", 300, 4),
    "n1": ((20, 17, 13), "k3", 1, 4),
    "n127": ((20, 17, 13), "k3", 127, 4),
    "n129": ((12, 20, 16), "k1", 129, 1),
    "n1500": ((12, 20, 16), "k3", 1500, 4),
    # consecutive samples of a few rays: adjacent lanes share cells, the backward sums such runs across the wave before its atomics
    "rays_d4": ((20, 17, 13), "k3", 700, 4),
    "rays_d1": ((12, 20, 16), "ranks", 300, 1),
}


def ray_points(N, gen, per_ray=37):
    """samples marched along rays through the box (37 per ray: the rays do not line up with the waves), steps of 1 / 64"""
    n_rays = (N + per_ray - 1) // per_ray
    o = torch.rand(n_rays, 3, generator=gen) * 2.0 - 1.0
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1)
    t = (torch.arange(per_ray, dtype=torch.float32) - per_ray / 2) / 64.0
    return (o[:, None, :] + t[None, :, None] * d[:, None, :]).reshape(-1, 3)[:N].contiguous()


def make_groups(res, layout, rows, gen):
    groups = []
    for rv, rm in zip(*LAYOUTS[layout]):
        lines = planes = s_vec = s_mat = None
        if rv:
            lines = [0.5 * torch.randn(1, rv, res[a], 1, generator=gen) for a in cw.VEC_IDS]
            s_vec = torch.randn(rows, rv, generator=gen)
        if rm:
            planes = [0.5 * torch.randn(1, rm, res[m1], res[m0], generator=gen) for m0, m1 in cw.MAT_IDS]
            s_mat = torch.randn(rows, rm, generator=gen)
        groups.append((lines, planes, s_vec, s_mat))
    return groups


def to_cuda(groups):
    return [tuple(None if t is None else (t.cuda() if torch.is_tensor(t) else [u.cuda() for u in t]) for t in g) for g in groups]


def flat(groups):
    """the tensors of a group list (or of the gradients shaped like it) in one order"""
    out = []
    for lines, planes, s_vec, s_mat in groups:
        out += list(lines or ()) + ([s_vec] if s_vec is not None else []) + list(planes or ()) + ([s_mat] if s_mat is not None else [])
    return out


def flat_witness(grads):
    out = []
    for w in grads:
        out += list(w["lines"] or ()) + ([w["s_vec"]] if w["s_vec"] is not None else []) + list(w["planes"] or ()) + \
            ([w["s_mat"]] if w["s_mat"] is not None else [])
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs and the witness' results of a case, computed once"""
    res, layout, N, degree = CASES[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000)
    dens, col = make_groups(res, layout, 1, gen), make_groups(res, layout, 3 * degree * degree, gen)
    if name.startswith("rays"):
        x = ray_points(N, gen)
        i0 = torch.from_numpy(cw.locate(x[:, 0].numpy(), res[0])[0])
        assert 0.3 < float((i0[1:] == i0[:-1]).float().mean()) < 0.98  # (there are runs, and they end)
    else:
        x = edge_points(N, res, 11) if N >= 40 else torch.rand(N, 3, generator=gen) * 2.6 - 1.3
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    K = len(dens)
    g_s, g_c = torch.randn(K, N, generator=gen), torch.randn(K, N, 3, generator=gen)
    wd, wc = witness_groups(dens), witness_groups(col)
    xs, ds = x.numpy(), d.numpy()
    ref = {}
    for residual in (True, False):
        ko = K if residual else 1
        ref[residual] = dict(feat=cw.features(xs, wd, residual), col=cw.color(xs, ds, wc, degree, residual),
                             g_feat=flat_witness(cw.grads(xs, wd, g_s[:ko].numpy(), residual)),
                             g_col=flat_witness(cw.grads(xs, wc, g_c[:ko].numpy(), residual, ds, degree)))
    return res, degree, dens, col, x, d, g_s, g_c, ref


def _close(got, want, what):
    want = np.asarray(want)
    np.testing.assert_allclose(got.double().cpu().numpy().reshape(want.shape), want, rtol=1e-4, atol=2e-5 * float(np.abs(want).max()) + 1e-30,
                               err_msg=what)


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "last"])
@pytest.mark.parametrize("name", list(CASES))
def test_cc_kernels_through_the_c_abi_match_the_witness(hip, name, residual):
    be = hip.CcBackend
    res, degree, dens, col, x, d, g_s, g_c, ref = _case(name)
    ref = ref[residual]
    dens, col, x, d = to_cuda(dens), to_cuda(col), x.cuda(), d.cuda()
    N, K = x.shape[0], len(dens)
    ko = K if residual else 1
    out_s, out_c = torch.full((ko, N), 7.0, device="cuda"), torch.full((ko, N, 3), 7.0, device="cuda")
    be.forward(x, None, dens, res, 0, residual, False, out_s)
    be.forward(x, d, col, res, degree, residual, False, out_c)
    _close(out_s, ref["feat"], "features")
    _close(out_c, ref["col"], "colour")
    if N >= 40 and not name.startswith("rays"):  # (the align_corners=False property: the rows just outside [-1, 1] read a value)
        outside = (x.abs() > 1).any(1) & (x.abs() < 1.06).all(1)
        assert bool(outside.any()) and float(out_s[:, outside].abs().max()) > 0
    gs = be.backward(x, None, dens, res, 0, residual, False, g_s[:ko].cuda().contiguous())
    gc = be.backward(x, d, col, res, degree, residual, False, g_c[:ko].cuda().contiguous())
    for got, want, params, tag in ((flat(gs), ref["g_feat"], flat(dens), "features"), (flat(gc), ref["g_col"], flat(col), "colour")):
        assert len(got) == len(want) == len(params)
        for i, (a, b, p) in enumerate(zip(got, want, params)):
            assert a.shape == p.shape
            _close(a, b, f"{tag} gradient {i} {tuple(p.shape)}")


def _autocast_reference(groups, x, d, degree, residual, g):
    """the torch sequence under fp16 autocast (tensoRF/network_cc.py: `_levels_torch` + the SH contraction) on copies of the
    factors: (head output fp32, gradients in the order of `flat`)"""
    from encoding import get_encoder
    from tensoRF import network_cc as cc
    leaves = [tuple(None if t is None else (t.clone().requires_grad_(True) if torch.is_tensor(t) else [u.clone().requires_grad_(True) for u in t])
                    for t in grp) for grp in groups]
    with torch.autocast("cuda", dtype=torch.float16):
        h = cc.NeRFNetwork._levels_torch(x, leaves, residual)
        assert h.dtype == torch.float16  # (the S @ f products and the level sums are half precision in this sequence)
        h = h if residual else h.unsqueeze(0)
        if degree == 0:
            out = h.squeeze(-1).float()
        else:
            enc, _ = get_encoder("sphere_harmonics", degree=degree)
            out = (h.view(h.shape[0], x.shape[0], 3, degree * degree) * enc(d).unsqueeze(1)).sum(-1)
            assert out.dtype == torch.float32
    (out * g).sum().backward()
    return out.detach(), [t.grad for t in flat(leaves)]


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "last"])
@pytest.mark.parametrize("name", list(CASES))
def test_cc_fp16_kernels_through_the_c_abi_match_the_autocast_sequence(hip, name, residual):
    """half = 1 of s3d_cc_* (both heads, forward and backward) over the same cases — degrees 1 and 4, K = 1 / 3 / 5, groups with
    one or both components, ranks above 32, flat resolutions, the edge rows, ray-ordered points — against the torch sequence under
    fp16 autocast: rtol 2e-2, atol 2e-3 * max |ref|"""
    be = hip.CcBackend
    res, degree, dens, col, x, d, g_s, g_c, _ = _case(name)
    dens, col, x, d = to_cuda(dens), to_cuda(col), x.cuda(), d.cuda()
    N, K = x.shape[0], len(dens)
    ko = K if residual else 1
    for groups, dirs, deg, g, tag in ((dens, None, 0, g_s[:ko].cuda().contiguous(), "features"), (col, d, degree, g_c[:ko].cuda().contiguous(), "colour")):
        want, want_grads = _autocast_reference(groups, x, dirs, deg, residual, g)
        out = torch.full((ko, N) + ((3,) if deg else ()), 7.0, device="cuda")
        be.forward(x, dirs, groups, res, deg, residual, True, out)
        got_grads = flat(be.backward(x, dirs, groups, res, deg, residual, True, g))
        pairs = [(out, want, tag)] + [(a, b, f"{tag} gradient {i} {tuple(b.shape)}") for i, (a, b) in enumerate(zip(got_grads, want_grads))]
        assert len(got_grads) == len(want_grads) == len(flat(groups))
        for a, b, what in pairs:
            assert a.shape == b.shape and bool(torch.isfinite(b).all()), what
            np.testing.assert_allclose(a.float().cpu().numpy(), b.float().cpu().numpy(), rtol=2e-2, atol=2e-3 * float(b.abs().max()) + 1e-30,
                                       err_msg=what)


def test_cc_binding_refuses_what_the_kernels_do_not_cover(hip):
    import ctypes as C
    be = hip.CcBackend
    gen = torch.Generator().manual_seed(1)
    res = (6, 5, 4)
    x, d = torch.zeros(4, 3, device="cuda"), torch.ones(4, 3, device="cuda")
    ok = to_cuda(make_groups(res, "k1", 1, gen))
    with pytest.raises(RuntimeError, match="degree 5"):
        be.forward(x, d, ok, res, 5, True, False, torch.empty(1, 4, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="fp32 GPU tensors"):
        be.forward(x, None, make_groups(res, "k1", 1, gen), res, 0, True, False, torch.empty(1, 4, device="cuda"))
    big = [([torch.zeros(1, 160, res[a], 1, device="cuda") for a in cw.VEC_IDS], None, torch.zeros(48, 160, device="cuda"), None)]
    with pytest.raises(RuntimeError, match="table"):
        be.forward(x, d, big, res, 4, True, False, torch.empty(1, 4, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="line 0"):
        be.forward(x, None, ok, (6, 5, 7), 0, True, False, torch.empty(1, 4, device="cuda"))
    # the C entry points check for themselves
    lib = hip.lib()
    arr, r3 = be._groups(ok, res, 0, "test")
    rc = lib.s3d_cc_features_forward(C.c_void_p(x.data_ptr()), C.c_uint32(4), arr, C.c_uint32(9), r3, C.c_int(1), C.c_int(0),
                                     C.c_void_p(x.data_ptr()), None, None)
    assert rc != 0 and b"cc_features_forward" in lib.s3d_last_error() and b"groups" in lib.s3d_last_error()
    rc = lib.s3d_cc_color_forward(C.c_void_p(x.data_ptr()), C.c_void_p(d.data_ptr()), C.c_uint32(4), arr, C.c_uint32(1), r3, C.c_uint32(5),
                                  C.c_int(1), C.c_int(0), C.c_void_p(x.data_ptr()), None, None)
    assert rc != 0 and b"degree" in lib.s3d_last_error()


def test_cc_padded_batch_rows_behind_the_count_are_neither_written_nor_read(hip):
    be = hip.CcBackend
    res, degree, dens, col, x, d, g_s, g_c, _ = _case("n1500")
    dens, col = to_cuda(dens), to_cuda(col)
    K, n0, live, M = len(dens), 1000, 1024, 1500
    counter = torch.tensor([n0, 0], dtype=torch.int32, device="cuda")
    xp, dp, gsp, gcp = x.clone().cuda(), d.clone().cuda(), g_s.clone().cuda(), g_c.clone().cuda()
    xp[live:], dp[live:], gsp[:, live:], gcp[:, live:] = float("nan"), float("nan"), float("nan"), float("nan")
    out_s, out_c = torch.full((K, M), 7.0, device="cuda"), torch.full((K, M, 3), 7.0, device="cuda")
    be.forward(xp, None, dens, res, 0, True, False, out_s, n_valid=counter)
    be.forward(xp, dp, col, res, degree, True, False, out_c, n_valid=counter)
    assert bool((out_s[:, live:] == 7).all()) and bool((out_c[:, live:] == 7).all())
    xt, dt = x[:live].cuda().contiguous(), d[:live].cuda().contiguous()
    ref_s, ref_c = torch.empty(K, live, device="cuda"), torch.empty(K, live, 3, device="cuda")
    be.forward(xt, None, dens, res, 0, True, False, ref_s)
    be.forward(xt, dt, col, res, degree, True, False, ref_c)
    assert torch.equal(out_s[:, :live], ref_s) and torch.equal(out_c[:, :live], ref_c)
    flag = torch.zeros(1, device="cuda")
    got = flat(be.backward(xp, None, dens, res, 0, True, False, gsp, found_inf=flag, n_valid=counter)) + \
        flat(be.backward(xp, dp, col, res, degree, True, False, gcp, found_inf=flag, n_valid=counter))
    want = flat(be.backward(xt, None, dens, res, 0, True, False, g_s[:, :live].cuda().contiguous())) + \
        flat(be.backward(xt, dt, col, res, degree, True, False, g_c[:, :live].cuda().contiguous()))
    assert float(flag) == 0.0
    for a, b in zip(got, want):  # (fp32 atomics: the order of the adds is all that differs)
        assert bool(torch.isfinite(a).all())
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["inside", "outside"])
def test_cc_backward_does_not_swallow_non_finite_gradients(hip, bad, where):
    """a NaN / inf level gradient raises found_inf and reaches the gradients — also for a point outside every factor, which
    reaches no cell (torch's backward carries 0 * inf = NaN into S there)"""
    be = hip.CcBackend
    res, degree, dens, col, x, d, g_s, g_c, _ = _case("k3_d4")
    dens, col, x = to_cuda(dens), to_cuda(col), x.clone()
    # (outside along all three axes: no tap of any line or plane is in range, the poison write is the only way in)
    x[40] = torch.tensor([0.1, -0.2, 0.3]) if where == "inside" else torch.tensor([5.0, 5.0, 5.0])
    x, d = x.cuda(), d.cuda()
    for groups, dirs, deg, g in ((dens, None, 0, g_s.clone()), (col, d, degree, g_c.clone())):
        g[1, 40] = bad
        flag = torch.zeros(1, device="cuda")
        grads = flat(be.backward(x, dirs, groups, res, deg, True, False, g.cuda().contiguous(), found_inf=flag))
        assert float(flag) == 1.0 and not all(bool(torch.isfinite(t).all()) for t in grads)
        flag.zero_()
        g[1, 40] = 0.5
        grads = flat(be.backward(x, dirs, groups, res, deg, True, False, g.cuda().contiguous(), found_inf=flag))
        assert float(flag) == 0.0 and all(bool(torch.isfinite(t).all()) for t in grads)


def _graph_nodes(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        todo.extend(f for f, _ in n.next_functions)
    return {type(n).__name__ for n in seen}


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_cc_network_fused_route_equals_the_grid_sample_route(hip, autocast, training):
    net = _net(grid=False).cuda().train(training)
    N = 1280
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(N, 3, generator=g) * 2.2 - 1.1).cuda()
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).cuda()
    K = 3 if training else 1
    ws, wr = torch.randn(K, N, generator=g).cuda(), torch.randn(K, N, 3, generator=g).cuda()
    out = {}
    for fused in (True, False):
        net.fused_cc = fused
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            sigma, rgb = net(x, d)
        assert sigma.shape == ((K, N) if training else (N,)) and rgb.shape == (K, N, 3)
        assert ("_CcHeadBackward" in _graph_nodes(sigma) and "_CcHeadBackward" in _graph_nodes(rgb)) == fused
        ((sigma.float().reshape(K, N) * ws).sum() + (rgb.float() * wr).sum()).backward()
        out[fused] = (sigma.detach().float(), rgb.detach().float(), {k: p.grad.float().clone() for k, p in net.named_parameters()})
    rtol, atol = (2e-2, 2e-3) if autocast else (1e-4, 2e-5)
    for a, b, what in ((out[True][0], out[False][0], "sigma"), (out[True][1], out[False][1], "rgb")):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=rtol, atol=atol * float(b.abs().max()), err_msg=what)
    assert set(out[True][2]) == set(out[False][2]) == {k for k, _ in net.named_parameters()}
    for k, b in out[False][2].items():
        np.testing.assert_allclose(out[True][2][k].cpu().numpy(), b.cpu().numpy(), rtol=rtol, atol=atol * float(b.abs().max()), err_msg=k)


def test_cc_coordinate_gradient_falls_back_to_the_torch_sequence(hip):
    net = _net(grid=False).cuda().train()
    x = (torch.rand(256, 3, generator=torch.Generator().manual_seed(3)) * 1.8 - 0.9).cuda().requires_grad_(True)
    d = torch.nn.functional.normalize(torch.ones(256, 3), dim=-1).cuda()
    sigma, rgb = net(x, d)
    assert "_CcHeadBackward" not in _graph_nodes(sigma) | _graph_nodes(rgb)
    (sigma.sum() + rgb.sum()).backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


def test_cc_train_step_vs_the_reference_trainer(hip, monkeypatch):
    """tests/golden/ccnerf.npz: tensoRF/utils.py `Trainer.train_step` EXECUTED on the reference's CCNeRF network; here the build's
    trainer on the HIP path in fp32 — tolerances of test_cp_train_step_with_l1_term_vs_the_reference_trainer"""
    import raymarching.raymarching as rm
    import nerf.renderer as rend
    from tensoRF.utils import Trainer
    from test_gpu_golden import _CpuRandom   # the marcher's jitter drawn from the CPU generator, as the fixture's was
    T = np.load(os.path.join(GOLDEN, "ccnerf.npz"))
    net = _net().cuda().train()
    with torch.no_grad():
        sg, cl = net(torch.from_numpy(T["fw_x"]).cuda(), torch.from_numpy(T["fw_d"]).cuda())
    assert "_CcHead" in str(type(net._head(torch.zeros(4, 3, device="cuda"), None, net._groups(True), True).grad_fn))
    np.testing.assert_allclose(sg.cpu().numpy(), T["train_sigma"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(cl.cpu().numpy(), T["train_color"], rtol=2e-5, atol=1e-6)
    net.mean_count = 32768
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=float(T["ts_l1_weight"]), fp16=False, update_extra_interval=10 ** 9)
    tr.global_step = 1
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


def test_cc_fp16_trainer_steps_and_the_graphed_trainer_refuses(hip):
    from nerf import synthetic as syn
    from tensoRF.utils import GraphedTrainer, Trainer
    net = _net().cuda()
    net.iter_density, net.mean_density, net.mean_count = 100, 5.0, 256 * 40
    with pytest.raises(NotImplementedError, match="rank-residual"):
        GraphedTrainer(net, 256)
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=1e-4, fp16=True, update_extra_interval=10 ** 9, upsample_model_steps=[3],
                 upsample_resolutions=[24])
    tr.global_step = 1
    r = syn.get_rays(syn.orbit_poses(2, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=256, generator=torch.Generator().manual_seed(0))
    ro, rd = r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous()
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(9)).cuda()
    before = [p.detach().clone() for p in net.parameters()]
    losses = [float(tr.train_step(ro, rd, gt)) for _ in range(2)]
    assert np.isfinite(losses).all() and any(not torch.equal(a.detach(), b) for a, b in zip(net.parameters(), before))
    assert net.resolution != NET["resolution"]  # (the scheduled shrink + upsample after the second step)
    assert [id(p) for grp in tr.optimizer.param_groups for p in grp["params"]] == [id(p) for p in net.parameters()]
    assert np.isfinite(float(tr.train_step(ro, rd, gt)))


def test_cc_finalize_and_compress_render_what_forward_k_rendered(hip):
    net = _net(grid=False).cuda().eval()
    g = torch.Generator().manual_seed(4)
    x = (torch.rand(640, 3, generator=g) * 2.2 - 1.1).cuda()
    d = torch.nn.functional.normalize(torch.randn(640, 3, generator=g), dim=-1).cuda()
    with torch.no_grad():
        for k in (3, 2, 1):
            want_s, want_c = net(x, d, K=k)
            cut = copy.deepcopy(net)
            cut.finalize()
            cut.compress(tuple(NET[name][k - 1] for name in ("rank_vec_density", "rank_mat_density", "rank_vec", "rank_mat")))
            got_s, got_c = cut(x, d)
            np.testing.assert_allclose(got_s.cpu().numpy(), want_s.cpu().numpy(), rtol=1e-4, atol=2e-5 * float(want_s.abs().max()))
            np.testing.assert_allclose(got_c.cpu().numpy(), want_c.cpu().numpy(), rtol=1e-4, atol=2e-5)


def test_cc_composed_scene_renders_and_equals_the_reference(hip):
    from nerf import synthetic as syn
    T = np.load(os.path.join(GOLDEN, "ccnerf.npz"))
    scene = compose_scene("cuda")
    with torch.no_grad():
        sg, cl = scene(torch.from_numpy(T["cmp_x"]).cuda(), torch.from_numpy(T["fw_d"]).cuda())
        np.testing.assert_allclose(sg.cpu().numpy(), T["cmp_sigma"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(cl.cpu().numpy(), T["cmp_color"], rtol=1e-4, atol=1e-5)
        del scene.update_extra_state  # (the instance's no-op: now the real sweeps, object by object through the kernels)
        scene.update_extra_state()
        assert scene.mean_density > 0
        r = syn.get_rays(syn.orbit_poses(2, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=64, generator=torch.Generator().manual_seed(0))
        out = scene.render(r["rays_o"][0].cuda().contiguous(), r["rays_d"][0].cuda().contiguous(), bg_color=1, perturb=False, max_steps=256)
    assert out["image"].shape == (64, 3) and bool(torch.isfinite(out["image"]).all()) and bool(torch.isfinite(out["depth"]).all())
    assert float(out["image"].min()) >= 0 and float(out["image"].max()) <= 1 + 1e-5
