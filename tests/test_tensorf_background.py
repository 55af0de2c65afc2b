"""The TensoRF background model (bg_radius > 0, tensoRF/network.py:69-96 / :201-218 of the reference) on CPU: construction, seeded
init and checkpoint keys, `background` and one trainer step on the oracle backends against tests/golden/tensorf_background.npz
(written by tools/gen_tensorf_background_golden.py from the reference's own network and trainer)."""
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NET = dict(resolution=[24, 28, 32], sigma_rank=[4, 5, 6], color_rank=[6, 7, 8], bound=1, cuda_ray=True, density_scale=1,
           min_near=0.2, density_thresh=10)
BG = dict(bg_radius=32, bg_resolution=[20, 12])       # fixture parts (a), (c): a plane that is not square
TS_BG = dict(bg_radius=32, bg_resolution=[32, 32])    # fixture part (b)


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "tensorf_background.npz"))


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _seed_params(net):
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
    return net


def _net(seed=None, **kw):
    from tensoRF.network import NeRFNetwork
    if seed is not None:
        torch.manual_seed(seed)
    return NeRFNetwork(**dict(NET, **kw))


def test_parameters_and_seeded_init_match_reference(G):
    net = _net(int(G["init_seed"]), **BG)
    params = list(net.named_parameters())
    assert [k for k, _ in params] == G["init_names"].tolist()
    assert [str(tuple(p.shape)) for _, p in params] == G["init_shapes"].tolist()
    for (k, p), s, s2 in zip(params, G["init_sum"], G["init_sumsq"]):
        assert p.detach().double().sum().item() == pytest.approx(float(s), rel=1e-12, abs=1e-12), k
        assert (p.detach().double() ** 2).sum().item() == pytest.approx(float(s2), rel=1e-12), k
    assert net.bg_mat.shape == (1, 8, 20, 12) and net.bg_net[0].weight.shape == (64, 23) and net.bg_net[1].weight.shape == (3, 64)
    groups = net.get_params(2e-2, 1e-3)
    assert [sum(p.numel() for p in g["params"]) for g in groups] == G["get_params_sizes"].tolist()
    assert [g["lr"] for g in groups] == G["get_params_lrs"].tolist()
    assert groups[-2]["params"] is net.bg_mat and groups[-2]["lr"] == 2e-2 and groups[-1]["lr"] == 1e-3


def test_default_constructor_arguments_are_the_references():
    net = _net(**dict(bg_radius=32))
    assert net.bg_mat.shape == (1, 8, 512, 512) and net.num_layers_bg == 2 and net.hidden_dim_bg == 64


def test_reference_state_dict_loads_strict(G):
    ref = _net(1, **BG)
    sd = {k: torch.randn_like(v) if v.is_floating_point() else v.clone() for k, v in ref.state_dict().items()}
    assert {k for k in sd if not k.startswith(("aabb_", "density_", "step_counter"))} == set(G["init_names"].tolist())
    net = _net(2, **BG)
    net.load_state_dict(sd, strict=True)
    assert torch.equal(net.bg_mat, sd["bg_mat"]) and torch.equal(net.bg_net[1].weight, sd["bg_net.1.weight"])


def test_no_background_model_is_unchanged(G):
    torch.manual_seed(int(G["init_seed"]))
    net = _net()
    assert net.bg_net is None and not hasattr(net, "bg_mat")
    names = [k for k, _ in net.named_parameters()]
    assert names == [k for k in G["init_names"].tolist() if not k.startswith("bg_")]
    assert len(net.get_params(2e-2, 1e-3)) == 6
    # the draws in front of the background's are the same with and without it
    sums = dict(zip(G["init_names"].tolist(), G["init_sum"]))
    for k, p in net.named_parameters():
        assert p.detach().double().sum().item() == pytest.approx(float(sums[k]), rel=1e-12, abs=1e-12), k


def test_deepcopy_keeps_the_background_model():
    import copy
    net = _net(0, **BG)
    twin = copy.deepcopy(net)
    assert torch.equal(twin.bg_mat, net.bg_mat) and twin.bg_mat is not net.bg_mat
    assert torch.equal(twin.bg_net[0].weight, net.bg_net[0].weight)


def test_background_forward_backward_match_reference(oracle_wrappers, G):
    net = _seed_params(_net(0, **BG))
    sph, rd = torch.from_numpy(G["bg_sph"]), torch.from_numpy(G["bg_rays_d"])
    n = int(G["bg_n_marched"])
    sph2 = oracle_wrappers.rm.sph_from_ray(torch.from_numpy(G["bg_rays_o"])[:n], rd[:n], BG["bg_radius"])
    assert torch.equal(sph2, sph[:n])
    assert sph.shape[0] == n + 16 and float(sph[n:].abs().max()) == pytest.approx(1.05)
    rgb = net.background(sph, rd)
    torch.testing.assert_close(rgb.detach(), torch.from_numpy(G["bg_rgb"]), rtol=0, atol=2e-6)
    rgb.backward(torch.from_numpy(G["bg_grad_rgb"]))
    assert net.bg_mat.grad.shape == (1, 8, 20, 12)
    for p, key in ((net.bg_mat, "bg_mat"), (net.bg_net[0].weight, "bg_net_0_weight"), (net.bg_net[1].weight, "bg_net_1_weight")):
        torch.testing.assert_close(p.grad, torch.from_numpy(G[f"bg_grad_{key}"]), rtol=1e-5, atol=1e-5)


def _ts_net():
    from nerf import synthetic as syn
    net = _seed_params(_net(**TS_BG))
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    return net


def test_train_step_with_background_matches_reference_train_step(oracle_wrappers, G, monkeypatch):
    """the reference's executed tensoRF Trainer.train_step with bg_radius = 32 (fixture part b): loss, prediction, sample count,
    the gradients of the background parameters and every other parameter's gradient norm, on the oracle backends"""
    from tensoRF.utils import Trainer
    net = _ts_net()
    net.mean_count = int(G["ts_mean_count"])
    tr = Trainer(net, lr0=2e-2, lr1=1e-3, l1_reg_weight=float(G["ts_l1_weight"]), fp16=False, update_extra_interval=10 ** 9)
    assert [g["lr"] for g in tr.optimizer.param_groups] == [2e-2] * 4 + [1e-3] * 2 + [2e-2, 1e-3]
    tr.global_step = 1
    net.train()
    torch.manual_seed(5)
    ro, rd, gt = (torch.from_numpy(G[k]) for k in ("ts_rays_o", "ts_rays_d", "ts_images"))
    seen = {}
    monkeypatch.setattr(tr, "_reduce_and_step", lambda: seen.update({k: p.grad.clone() for k, p in net.named_parameters()}))
    pred = {}
    render = net.render
    monkeypatch.setattr(net, "render", lambda *a, **k: pred.setdefault("out", render(*a, **k)))
    loss = tr.train_step(ro[0], rd[0], gt[0])
    assert abs(float(loss) - float(G["ts_loss"])) <= 1e-6 * float(G["ts_loss"])
    assert np.array_equal(net.step_counter[0].numpy(), G["ts_counter"])
    np.testing.assert_allclose(pred["out"]["image"].detach().numpy().reshape(G["ts_pred"].shape), G["ts_pred"], rtol=1e-6, atol=1e-7)
    for k, g in seen.items():
        key = "ts_grad_" + k.replace(".", "_")
        ref = float(G[key + "_norm"])
        assert abs(float(g.double().norm()) - ref) <= 1e-6 * ref, k
        if key in G.files:
            np.testing.assert_allclose(g.reshape(-1).numpy(), G[key], rtol=1e-5, atol=1e-6 * float(np.abs(G[key]).max()), err_msg=k)
    assert {"ts_grad_bg_mat", "ts_grad_bg_net_0_weight", "ts_grad_bg_net_1_weight"} <= set(G.files)


@pytest.mark.parametrize("kw", [dict(bg_rank=4), dict(hidden_dim_bg=32), dict(num_layers_bg=3)], ids=["rank4", "hidden32", "layers3"])
def test_other_shapes_construct_and_run_on_the_torch_path(oracle_wrappers, kw):
    net = _net(0, **dict(BG, **kw))
    R, Hd = kw.get("bg_rank", 8), kw.get("hidden_dim_bg", 64)
    assert net.bg_mat.shape == (1, R, 20, 12) and net.bg_net[0].weight.shape == (Hd, R + 15) and len(net.bg_net) == kw.get("num_layers_bg", 2)
    sph = _seeded((33, 2), 1, -1.05, 1.05)
    rd = torch.nn.functional.normalize(_seeded((33, 3), 2, -1, 1), dim=-1)
    rgb = net.background(sph, rd)
    assert rgb.shape == (33, 3) and bool(((rgb > 0) & (rgb < 1)).all())
    rgb.sum().backward()
    assert net.bg_mat.grad is not None and float(net.bg_mat.grad.abs().sum()) > 0
