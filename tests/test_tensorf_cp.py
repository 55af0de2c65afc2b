"""CPU: the TensoRF CP backbone (tensoRF/network_cp.py).

1. tests/cp_witness.py (float64 numpy statement of the line-factor contract) against torch's CPU grid_sample sequence and its
   autograd, at the tolerances tests/test_vm_oracle.py uses for the VM witness;
2. the build's network on the torch route against the REFERENCE's, executed (tests/golden/tensorf_cp.npz from
   tools/gen_tensorf_cp_golden.py), at the tolerances of tests/test_tensorf_golden.py;
3. tensoRF.utils.Trainer on a CP model: the L1 term, the scheduled upsampling; the VM model's term unchanged;
4. a reference-named state dict loads strictly."""
import os
import zlib

import numpy as np
import pytest
import torch

import cp_witness as cw
from conftest import GOLDEN

NET = dict(resolution=[20, 17, 13], sigma_rank=[8, 8, 8], color_rank=[24, 24, 24], bound=1, cuda_ray=True, density_scale=1,
           min_near=0.2, density_thresh=10)


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


@pytest.fixture(scope="module")
def T():
    return np.load(os.path.join(GOLDEN, "tensorf_cp.npz"))


def _net(**over):
    from nerf import synthetic as syn
    from tensoRF import network_cp as cp
    net = cp.NeRFNetwork(**{**NET, **over})
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    return net, dens


def _np(vecs):
    return [v.detach().numpy()[0, :, :, 0] for v in vecs]


def _edge_points(n, seed):
    """random points in [-1.3, 1.3]^3 with rows exactly on u = +-1, 0 and just outside +-1"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 2.6 - 1.3
    edge = torch.tensor([-1.0, 1.0, 0.0, -1.0001, 1.0001, -1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, 3.0])
    k = edge.numel()
    for a in range(3):
        x[a * k:(a + 1) * k, a] = edge
    x[3 * k:4 * k] = edge[:, None]
    return x


@pytest.mark.parametrize("res,R", [((12, 20, 16), 5), ((1, 2, 65), 3), ((65, 1, 2), 2), ((2, 65, 1), 4)])
def test_witness_matches_the_grid_sample_sequence_and_its_autograd(res, R):
    from tensoRF import network_cp as cp
    torch.manual_seed(5)
    net = cp.NeRFNetwork(resolution=list(res), sigma_rank=[R] * 3, color_rank=[R + 1] * 3, bound=1, cuda_ray=False)
    x = _edge_points(1500, 6)
    xs = x.numpy()
    s_ref = net._sigma_feat_torch(x, net.sigma_vec)
    c_ref = net._color_prod_torch(x, net.color_vec)
    np.testing.assert_allclose(cw.features(xs, _np(net.sigma_vec)), s_ref.detach().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(cw.products(xs, _np(net.color_vec)), c_ref.detach().numpy(), rtol=1e-5, atol=1e-7)
    if min(res) > 1:  # (a one-cell line is a constant: every point sees it, inside or not)
        inside = (x.abs() <= 1).all(1).numpy()
        assert 0.2 < inside.mean() < 0.8 and np.abs(cw.products(xs, _np(net.color_vec))[:, ~inside]).max() > 0
    w = torch.linspace(-1, 1, x.shape[0])
    s_ref.mul(w).sum().backward()
    gl, nc, sa = cw.line_grads(xs, _np(net.sigma_vec), w.numpy())
    for p, g, n, s in zip(net.sigma_vec, gl, nc, sa):
        np.testing.assert_allclose(g.reshape(p.grad.shape), p.grad.numpy(), rtol=2e-4, atol=1e-6)
        assert n.sum() > 0 and (s >= np.abs(g) - 1e-12).all()
    gc = torch.randn(c_ref.shape, generator=torch.Generator().manual_seed(7))
    c_ref.mul(gc).sum().backward()
    gl, _, _ = cw.line_grads(xs, _np(net.color_vec), gc.numpy())
    for p, g in zip(net.color_vec, gl):
        np.testing.assert_allclose(g.reshape(p.grad.shape), p.grad.numpy(), rtol=2e-4, atol=1e-6)
    # basis_mat behind the products
    net.zero_grad()
    go = torch.randn(x.shape[0], 27, generator=torch.Generator().manual_seed(8))
    out = net.get_color_feat(x)
    np.testing.assert_allclose(cw.basis_features(xs, _np(net.color_vec), net.basis_mat.weight.detach().numpy()), out.detach().numpy(),
                               rtol=1e-5, atol=1e-6)
    out.mul(go).sum().backward()
    gl, _, _, gw = cw.basis_grads(xs, _np(net.color_vec), net.basis_mat.weight.detach().numpy(), go.numpy())
    np.testing.assert_allclose(gw, net.basis_mat.weight.grad.numpy(), rtol=2e-4, atol=1e-5)
    for p, g in zip(net.color_vec, gl):
        np.testing.assert_allclose(g.reshape(p.grad.shape), p.grad.numpy(), rtol=2e-4, atol=1e-5)


def test_witness_counts_the_terms_of_a_cell():
    """one line cell hit by a known number of taps: n_cell and sum |term| are what the fp32 bound of the GPU tests is made of"""
    lines = [np.ones((2, 5)), np.ones((2, 3)), np.ones((2, 4))]
    x = np.zeros((7, 3), dtype=np.float32)
    x[:, 2] = -1.0 + 2.0 * 1.25 / 4.0  # line 0 (axis 2, D = 5): p = 1.25 -> cells 1 and 2 with weights 0.75 / 0.25
    gl, nc, sa = cw.line_grads(x, lines, np.full(7, -2.0))
    assert nc[0].tolist() == [0, 7, 7, 0, 0]
    np.testing.assert_allclose(gl[0][0], [0, -10.5, -3.5, 0, 0], rtol=1e-12)
    np.testing.assert_allclose(sa[0][1], [0, 10.5, 3.5, 0, 0], rtol=1e-12)


def _check_grads(net, T, prefix, rtol=1e-6):
    for k, p in net.named_parameters():
        key = f"{prefix}_{k.replace('.', '_')}"
        g = p.grad.detach().reshape(-1)
        assert abs(float(g.double().norm()) - float(T[key + "_norm"])) <= rtol * max(float(T[key + "_norm"]), 1e-12), k
        if key in T.files:
            np.testing.assert_allclose(g.numpy(), T[key], rtol=1e-5, atol=rtol * float(np.abs(T[key]).max()), err_msg=k)
        else:
            np.testing.assert_allclose(g[torch.from_numpy(T[key + "_at"])].numpy(), T[key + "_at_values"], rtol=1e-5,
                                       atol=rtol * float(np.abs(T[key + "_at_values"]).max()), err_msg=k)


def test_parameters_groups_forward_and_density_loss(oracle_wrappers, T):
    net, _ = _net()
    assert [k for k, _ in net.named_parameters()] == T["param_names"].tolist()
    assert [str(tuple(p.shape)) for _, p in net.named_parameters()] == T["param_shapes"].tolist()
    names = {id(p): k for k, p in net.named_parameters()}
    groups = net.get_params(2e-2, 1e-3)
    assert [g["lr"] for g in groups] == T["group_lrs"].tolist() == [2e-2, 2e-2, 1e-3, 1e-3]
    assert [",".join(names[id(p)] for p in g["params"]) for g in groups] == T["group_members"].tolist()
    x, d = torch.from_numpy(T["fw_x"]), torch.from_numpy(T["fw_d"])
    with torch.no_grad():
        sg, cl = net(x, d)
        np.testing.assert_allclose(sg.numpy(), T["fw_sigma"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(cl.numpy(), T["fw_color"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(net.density(x)["sigma"].numpy(), T["fw_density"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(net.color(x, d).numpy(), T["fw_color"], rtol=1e-6, atol=1e-7)
        mask = torch.arange(x.shape[0]) % 3 == 0
        masked = net.color(x, d, mask=mask)
        np.testing.assert_allclose(masked[mask].numpy(), T["fw_color"][mask.numpy()], rtol=1e-6, atol=1e-7)
        assert not masked[~mask].any() and not net.color(x, d, mask=torch.zeros_like(mask)).any()
        for fused in (True, False):
            net.fused_l1 = fused
            assert abs(float(net.density_loss()) - float(T["density_loss"])) <= 1e-6 * float(T["density_loss"])
        assert abs(float(net.density_loss_value()) - float(T["density_loss"])) <= 1e-6 * float(T["density_loss"])
    # the witness on the fixture's own numbers (the reference's get_sigma_feat / get_color_feat)
    np.testing.assert_allclose(cw.features(T["fw_x"], _np(net.sigma_vec)), T["fw_sigma_feat"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cw.basis_features(T["fw_x"], _np(net.color_vec), net.basis_mat.weight.detach().numpy()),
                               T["fw_color_feat"], rtol=1e-5, atol=1e-5)


def test_train_step_with_the_l1_term_matches_the_reference_trainer(oracle_wrappers, T, monkeypatch):
    from tensoRF.utils import Trainer
    net, _ = _net()
    net.mean_count = 32768
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=float(T["ts_l1_weight"]), fp16=False, update_extra_interval=10 ** 9)
    assert [g["lr"] for g in tr.optimizer.param_groups] == T["group_lrs"].tolist()
    tr.global_step = 1
    net.train()
    torch.manual_seed(5)
    ro, rd, gt = (torch.from_numpy(T[k]) for k in ("ts_rays_o", "ts_rays_d", "ts_images"))
    seen = {}
    monkeypatch.setattr(tr, "_reduce_and_step", lambda: seen.update({k: p.grad.clone() for k, p in net.named_parameters()}))
    loss = tr.train_step(ro[0], rd[0], gt[0])
    assert abs(float(loss) - float(T["ts_loss"])) <= 1e-6 * float(T["ts_loss"])
    assert np.array_equal(net.step_counter[0].numpy(), T["ts_counter"])
    for k, p in net.named_parameters():
        p.grad = seen[k]
    _check_grads(net, T, "ts_grad")


def test_shrink_and_upsample_follow_the_reference(oracle_wrappers, T):
    net, dens = _net()
    net.mean_density = 5.0
    tl, br = net.shrink_model()
    np.testing.assert_allclose(net.aabb_train.numpy(), T["shrink_aabb"], rtol=0, atol=1e-7)
    assert [str(tuple(p.shape)) for _, p in net.named_parameters()] == T["shrink_shapes"].tolist()
    assert net.resolution == [b - a for a, b in zip(tl, br)]  # (follows the crop)
    net.upsample_model([30, 26, 22])
    assert [str(tuple(p.shape)) for _, p in net.named_parameters()] == T["up_shapes"].tolist()
    with torch.no_grad():
        sg, cl = net(torch.from_numpy(T["up_x"]), torch.from_numpy(T["fw_d"][:200]))
    np.testing.assert_allclose(sg.numpy(), T["up_sigma"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(cl.numpy(), T["up_color"], rtol=1e-5, atol=1e-7)
    net.density_grid.zero_()
    with pytest.raises(RuntimeError, match="no cell"):
        net.shrink_model()


def test_constructor_defaults_and_refusals():
    from tensoRF import network_cp as cp
    net = cp.NeRFNetwork(resolution=[4, 5, 6])
    assert net.sigma_rank == [96] * 3 and net.color_rank == [288] * 3 and net.color_feat_dim == 27 and net.in_dim == 150
    assert [tuple(v.shape) for v in net.sigma_vec] == [(1, 96, 6, 1), (1, 96, 5, 1), (1, 96, 4, 1)]
    assert tuple(net.basis_mat.weight.shape) == (27, 288) and [tuple(l.weight.shape) for l in net.color_net] == [(128, 150), (128, 128), (3, 128)]
    assert 0.17 < float(torch.cat([v.detach().reshape(-1) for v in net.color_vec]).std()) < 0.23  # (init scale 0.2)
    with pytest.raises(AssertionError, match="background model is not implemented for --cp"):
        cp.NeRFNetwork(resolution=[4, 5, 6], bg_radius=2.0)
    with pytest.raises(ValueError, match="must be equal"):
        cp.NeRFNetwork(resolution=[4, 5, 6], color_rank=[8, 8, 12])


def test_trainer_takes_a_cp_model_and_the_vm_term_is_unchanged(oracle_wrappers):
    from tensoRF import network as trf
    from tensoRF.utils import Trainer
    net, _ = _net()
    net.mean_count = 32768
    net.mean_density = 5.0
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=3e-3, fp16=False, update_extra_interval=10 ** 9,
                 upsample_model_steps=[2], upsample_resolutions=[24])
    want = 3e-3 * sum(float(v.abs().mean()) for v in net.sigma_vec)
    assert abs(float(tr._regularizer()) - want) <= 1e-6 * want
    assert [id(p) for p in net.density_factors()] == [id(p) for p in net.sigma_vec]
    g = torch.Generator().manual_seed(81)
    from nerf import synthetic as syn
    r = syn.get_rays(syn.orbit_poses(1, seed=0)[:1], syn.lego_intrinsics(), 800, 800, N=64, generator=g)
    ro, rd, gt = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous(), _seeded((64, 3), 82)
    tr.train_step(ro, rd, gt)
    old = [id(p) for grp in tr.optimizer.param_groups for p in grp["params"]]
    assert net.resolution == NET["resolution"]
    tr.train_step(ro, rd, gt)  # global_step 2: shrink + upsample + a new optimizer over the new lines
    assert net.resolution != NET["resolution"] and [v.shape[2] for v in net.sigma_vec] == [net.resolution[a] for a in (2, 1, 0)]
    new = [id(p) for grp in tr.optimizer.param_groups for p in grp["params"]]
    assert new == [id(p) for p in net.parameters()] and new[:6] != old[:6] and new[6:] == old[6:]
    assert [grp["lr"] for grp in tr.optimizer.param_groups] == [2e-2, 2e-2, 1e-3, 1e-3]
    assert np.isfinite(float(tr.train_step(ro, rd, gt)))
    # the VM model's term: the value density_loss() gives
    vm = trf.NeRFNetwork(resolution=[8, 9, 10], sigma_rank=[2, 3, 4], color_rank=[2, 2, 2], bound=1, cuda_ray=True)
    tv = Trainer(vm, lr0=2e-2, lr1=1e-3, l1_reg_weight=3e-3, fp16=False, update_extra_interval=10 ** 9)
    assert float(tv._regularizer()) == float(vm.density_loss() * 3e-3)
    assert [id(p) for p in vm.density_factors()] == [id(p) for p in list(vm.sigma_mat) + list(vm.sigma_vec)]
    assert abs(float(vm.density_loss_value()) - float(vm.density_loss())) <= 1e-6 * float(vm.density_loss())


def test_reference_named_state_dict_loads_strictly(T):
    from tensoRF import network_cp as cp
    net = cp.NeRFNetwork(**NET)
    state = {k: _seeded(eval(s), zlib.crc32(k.encode()) % 1000, -0.5, 0.5) for k, s in zip(T["param_names"].tolist(), T["param_shapes"].tolist())}
    for k, v in net.state_dict().items():  # (buffers of the renderer: not parameters of the reference's class either)
        state.setdefault(k, v.clone())
    net.load_state_dict(state, strict=True)
    with torch.no_grad():
        sf = net.get_sigma_feat(torch.from_numpy(T["fw_x"]))
    np.testing.assert_allclose(sf.numpy(), T["fw_sigma_feat"], rtol=1e-6, atol=1e-7)
