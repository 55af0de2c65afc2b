"""The NGP background model (bg_radius > 0, nerf/network.py:74-96 / :149-163 of the reference) on CPU: construction, seeded
init and checkpoint keys, and the torch path on the oracle backends against tests/golden/background.npz (written by
tools/gen_background_golden.py from the reference's own network)."""
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import REPO

GOLD = os.path.join(REPO, "tests", "golden", "background.npz")
NET = dict(bound=1, cuda_ray=True, log2_hashmap_size=14, bg_radius=32)


def _gold():
    return np.load(GOLD)


def _seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _net(seed=None):
    from nerf.network import NeRFNetwork
    if seed is not None:
        torch.manual_seed(seed)
    return NeRFNetwork(**NET)


def test_parameters_and_seeded_init_match_reference():
    d = _gold()
    net = _net(int(d["init_seed"]))
    params = list(net.named_parameters())
    assert [k for k, _ in params] == [str(s) for s in d["init_names"]]
    for (k, p), shp, s, s2 in zip(params, d["init_shapes"], d["init_sum"], d["init_sumsq"]):
        assert list(p.shape) == [int(v) for v in shp[:p.dim()]], k
        assert p.detach().double().sum().item() == pytest.approx(float(s), rel=1e-12, abs=1e-12), k
        assert (p.detach().double() ** 2).sum().item() == pytest.approx(float(s2), rel=1e-12), k
    assert net.encoder_bg.embeddings.numel() == 1395552 and net.bg_net[0].weight.shape == (64, 24)
    sizes = [sum(p.numel() for p in g["params"]) for g in net.get_params(1e-2)]
    assert sizes == [int(v) for v in d["get_params_sizes"]]


def test_reference_state_dict_loads_strict():
    d = _gold()
    ref = _net(1)
    # a reference-format state dict: the reference's parameter names + the renderer's buffers
    sd = {k: torch.randn_like(v) if v.is_floating_point() else v.clone() for k, v in ref.state_dict().items()}
    assert {k for k in sd if not k.startswith(("aabb_", "density_", "step_counter")) and "offsets" not in k} == \
        {str(s) for s in d["init_names"]}
    net = _net(2)
    net.load_state_dict(sd, strict=True)
    assert torch.equal(net.encoder_bg.embeddings, sd["encoder_bg.embeddings"])
    assert torch.equal(net.bg_net[1].weight, sd["bg_net.1.weight"])


def test_no_background_model_is_unchanged():
    from nerf.network import NeRFNetwork
    net = NeRFNetwork(bound=1, cuda_ray=True, log2_hashmap_size=14)
    assert not hasattr(net, "encoder_bg") and not hasattr(net, "bg_net")
    assert len(net.get_params(1e-2)) == 5


def test_network_ff_refuses_background():
    from nerf.network_ff import NeRFNetwork as FF
    with pytest.raises(NotImplementedError):
        FF(bound=1, cuda_ray=True, bg_radius=32)


def test_background_forward_backward_match_reference(oracle_wrappers):
    d = _gold()
    net = _net(0)
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
    sph, rd = torch.from_numpy(d["bg_sph"]), torch.from_numpy(d["bg_rays_d"])
    ro = torch.from_numpy(d["bg_rays_o"])
    sph2 = oracle_wrappers.rm.sph_from_ray(ro, rd, NET["bg_radius"])
    assert torch.equal(sph2, sph)
    rgb = net.background(sph, rd)
    torch.testing.assert_close(rgb.detach(), torch.from_numpy(d["bg_rgb"]), rtol=0, atol=2e-6)
    rgb.backward(torch.from_numpy(d["bg_grad_rgb"]))
    for name in ("bg_net_0_weight", "bg_net_1_weight"):
        p = dict(net.named_parameters())[name.replace("_net_", "_net.").replace("_weight", ".weight")]
        torch.testing.assert_close(p.grad, torch.from_numpy(d[f"bg_grad_{name}"]), rtol=1e-5, atol=1e-5)
    g = net.encoder_bg.embeddings.grad
    rows = torch.from_numpy(d["bg_grad_encoder_bg_embeddings_rows"])
    torch.testing.assert_close(g[rows], torch.from_numpy(d["bg_grad_encoder_bg_embeddings_at_rows"]), rtol=1e-5, atol=1e-6)
    assert g.double().norm().item() == pytest.approx(float(d["bg_grad_encoder_bg_embeddings_norm"]), rel=1e-5)


def _ts_student():
    from nerf import synthetic as syn
    from nerf.network import NeRFNetwork
    net = NeRFNetwork(bound=1, cuda_ray=True, log2_hashmap_size=14, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=32)
    for k, p in net.named_parameters():
        p.data.copy_(_seeded(p.shape, zlib.crc32(k.encode()) % 1000, -0.5, 0.5))
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    return net


def test_train_step_with_background_matches_reference_train_step(oracle_wrappers):
    """the reference's executed Trainer.train_step with bg_radius = 32 (fixture part b): loss, prediction, sample count and the
    gradients of the background parameters (every other parameter: gradient norm) on the oracle backends"""
    from sealnerf import SealTrainer
    d = _gold()
    net = _ts_student()
    net.mean_count = int(d["ts_mean_count"])
    tr = SealTrainer(net, net, lr=1e-2, fp16=False)
    net.train()
    torch.manual_seed(5)
    loss, out = tr.finetune_loss(torch.from_numpy(d["ts_rays_o"]), torch.from_numpy(d["ts_rays_d"]), torch.from_numpy(d["ts_images"]),
                                 torch.from_numpy(d["ts_depths"]), bg_color=1)
    assert np.array_equal(net.step_counter[0].numpy(), d["ts_counter"])
    assert abs(float(loss) - float(d["ts_loss"])) <= 1e-6 * float(d["ts_loss"])
    np.testing.assert_allclose(out["image"].detach().numpy(), d["ts_pred"], rtol=1e-6, atol=1e-7)
    net.zero_grad()
    loss.backward()
    for k, p in net.named_parameters():
        key = "ts_grad_" + k.replace(".", "_")
        g = p.grad.detach()
        assert abs(float(g.double().norm()) - float(d[key + "_norm"])) <= 1e-6 * float(d[key + "_norm"]), k
        if key in d.files:
            np.testing.assert_allclose(g.numpy(), d[key], rtol=1e-5, atol=1e-6 * float(np.abs(d[key]).max()), err_msg=k)
        elif key + "_rows" in d.files:
            np.testing.assert_allclose(g[torch.from_numpy(d[key + "_rows"])].numpy(), d[key + "_at_rows"], rtol=1e-5,
                                       atol=1e-6 * float(np.abs(d[key + "_at_rows"]).max()), err_msg=k)


_DP_SCRIPT = r'''
import os, sys, torch, torch.distributed as dist
repo = os.environ["S3D_REPO"]
sys.path.insert(0, repo); sys.path.insert(0, os.path.join(repo, "seal-3d_amd")); sys.path.insert(0, os.path.join(repo, "tests"))
from parallel import RayShardedDP, init_from_env
rank, world, _ = init_from_env("gloo")
from oracle import oracle_backend as ob
import raymarching.raymarching as rm, gridencoder.grid as gg, shencoder.sphere_harmonics as sh
rm._backend, gg._backend, sh._backend = ob.RaymarchingBackend, ob.GridBackend, ob.SHBackend
ob.set_threads(1)
from nerf import synthetic as syn
import test_background as tb
torch.manual_seed(100 + rank)
net = tb._ts_student()
dp = RayShardedDP().register(net)
bg = [net.encoder_bg.embeddings, net.bg_net[0].weight, net.bg_net[1].weight]
assert all(any(p is q for q in dp.params) for p in bg)
net.train()
net.mean_count = 32768
poses = syn.orbit_poses(2, seed=0)
r = syn.get_rays(poses[rank:rank + 1], syn.lego_intrinsics(), 800, 800, N=256, generator=torch.Generator().manual_seed(7 + rank))
dp.flat.zero_()
out = net.render(r["rays_o"][0], r["rays_d"][0], bg_color=1, perturb=False, force_all_rays=True, max_steps=1024)
loss = torch.nn.functional.mse_loss(out["image"], torch.full_like(out["image"], 0.3))
loss.backward()
local = [p.grad.detach().clone() for p in bg]
dp.allreduce_grads()
ok = True
for p, g in zip(bg, local):
    every = [torch.empty_like(g) for _ in range(world)]
    dist.all_gather(every, g)
    mean = sum(every) / world
    ok &= bool(torch.allclose(p.grad, mean, rtol=1e-6, atol=1e-9)) and float(g.abs().sum()) > 0
    ok &= not torch.equal(every[0], every[1])
print(f"RANK{rank} averaged={ok}")
dist.destroy_process_group()
'''


def test_background_gradients_are_averaged_over_two_gloo_ranks(tmp_path):
    import subprocess
    import sys
    script = tmp_path / "bg_dp.py"
    script.write_text(_DP_SCRIPT)
    env = dict(os.environ, S3D_REPO=REPO, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29563", str(script)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    for r in range(2):
        assert f"RANK{r} averaged=True" in res.stdout, res.stdout + res.stderr[-1500:]
