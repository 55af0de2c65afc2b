#!/usr/bin/env python3
"""Generate tests/golden/tensorf_cp.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the CP backbone the way oracle/gen_golden.py `tensorf` pins the vector-matrix one: the reference's
tensoRF/network_cp.py `NeRFNetwork` (line factors only) with seeded parameters is EXECUTED on the CPU oracle stack —
forward / density on seeded points, `density_loss()`, the `get_params` group layout, tensoRF/utils.py `Trainer.train_step`
(the NGP step + `density_loss() * l1_reg_weight`) with every parameter gradient, `shrink_model` + `upsample_model` and a
forward on the re-sampled lines.  Only recorded arrays are stored.

    python tools/gen_tensorf_cp_golden.py     (re-running reproduces the file bit for bit)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle.gen_golden import (_assert_reference, _grad_record_flat, _install_reference_stack, _load_synthetic, _seed_params,  # noqa: E402
                               _seeded, _stub_training_imports)

OUT = os.path.join(REPO, "tests", "golden", "tensorf_cp.npz")
CP_NET = dict(resolution=[20, 17, 13], sigma_rank=[8, 8, 8], color_rank=[24, 24, 24], bound=1, cuda_ray=True, density_scale=1,
              min_near=0.2, density_thresh=10)


def main():
    _install_reference_stack()
    _stub_training_imports()
    cp = importlib.import_module("tensoRF.network_cp")
    tu = importlib.import_module("tensoRF.utils")
    strainer = importlib.import_module("SealNeRF.trainer")
    for m_ in (cp, tu, strainer):
        _assert_reference(m_)
    syn = _load_synthetic()
    out = {}
    torch.manual_seed(3)
    net = cp.NeRFNetwork(**CP_NET)
    _seed_params(net)
    out.update(param_names=np.array([k for k, _ in net.named_parameters()]),
               param_shapes=np.array([str(tuple(p.shape)) for _, p in net.named_parameters()]))
    groups = net.get_params(2e-2, 1e-3)
    names = {id(p): k for k, p in net.named_parameters()}
    out["group_lrs"] = np.array([g["lr"] for g in groups])
    out["group_members"] = np.array([",".join(names[id(p)] for p in g["params"]) for g in groups])
    x = _seeded((300, 3), 71, -1, 1)
    d = torch.nn.functional.normalize(_seeded((300, 3), 72, -1, 1), dim=-1)
    sg, cl = net(x, d)
    dl = net.density_loss()
    out.update(fw_x=x.numpy(), fw_d=d.numpy(), fw_sigma=sg.detach().numpy(), fw_color=cl.detach().numpy(),
               fw_sigma_feat=net.get_sigma_feat(x).detach().numpy(), fw_color_feat=net.get_color_feat(x).detach().numpy(),
               fw_density=net.density(x)["sigma"].detach().numpy(), density_loss=np.float64(dl.item()))
    # -- Trainer.train_step (tensoRF/utils.py:42-49) on an instance made without __init__
    dens, bits = syn.lego_like_density_grid(seed=0)
    net.density_grid.copy_(torch.from_numpy(dens))
    net.density_bitfield.copy_(torch.from_numpy(bits))
    net.mean_count = 32768
    poses = syn.orbit_poses(1, seed=0)
    r = syn.get_rays(poses[:1], syn.lego_intrinsics(), 800, 800, N=256, generator=torch.Generator().manual_seed(81))
    ro, rd = r["rays_o"].contiguous(), r["rays_d"].contiguous()
    images = _seeded((1, 256, 3), 82)
    opt = types.SimpleNamespace(color_space="srgb", patch_size=1, dt_gamma=0, max_steps=1024, T_thresh=1e-4, l1_reg_weight=1e-4)
    me = object.__new__(tu.Trainer)
    me.model, me.opt, me.criterion, me.error_map = net, opt, torch.nn.MSELoss(reduction="none"), None
    me._backbone, me.log_ptr = strainer.BackBoneTypes.TensoRF, None
    net.train()
    torch.manual_seed(5)
    noises = torch.rand(256)
    torch.manual_seed(5)
    pred, gt, loss = tu.Trainer.train_step(me, {"rays_o": ro, "rays_d": rd, "images": images.clone()})
    net.zero_grad()
    loss.backward()
    out.update(ts_rays_o=ro.numpy(), ts_rays_d=rd.numpy(), ts_images=images.numpy(), ts_noises=noises.numpy(),
               ts_loss=np.float64(loss.item()), ts_pred=pred.detach().numpy(), ts_counter=net.step_counter[0].numpy().copy(),
               ts_l1_weight=np.float64(opt.l1_reg_weight))
    _grad_record_flat(net, "ts_grad", out)
    # -- shrink_model + upsample_model (parameter shapes, aabb, a forward on the re-sampled lines)
    net.mean_density = 5.0
    net.density_grid.copy_(torch.from_numpy(dens))
    with torch.no_grad():
        net.shrink_model()
        out.update(shrink_aabb=net.aabb_train.numpy().copy(),
                   shrink_shapes=np.array([str(tuple(p.shape)) for _, p in net.named_parameters()]))
        net.upsample_model([30, 26, 22])
        out["up_shapes"] = np.array([str(tuple(p.shape)) for _, p in net.named_parameters()])
        xs = _seeded((200, 3), 95, -0.5, 0.5)
        sg2, cl2 = net(xs, d[:200])
        out.update(up_x=xs.numpy(), up_sigma=sg2.numpy(), up_color=cl2.numpy())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays); train loss {loss.item()} density_loss {dl.item()}")


if __name__ == "__main__":
    main()
