#!/usr/bin/env python3
"""Generate tests/golden/ccnerf.npz from the reference (AUTHORING CONTAINER ONLY, beside the reference checkout).

Pins the CCNeRF backbone the way tools/gen_tensorf_cp_golden.py pins the CP one: the reference's tensoRF/network_cc.py
`NeRFNetwork` (rank-residual groups of vector and matrix components) with seeded parameters is EXECUTED on the CPU oracle stack —
train-mode and eval-mode forward / density on seeded points (some of them outside [-1, 1]: align_corners=False reads a value
there), train mode with K = 2, `density_loss()`, the `get_params` group layout, tensoRF/utils.py `Trainer.train_step` with the
per-level prediction and every parameter gradient, `shrink_model` + `upsample_model`, `finalize()`, `compress((4, 2, 4, 2))`
and `compose` of two finalized models into an empty scene.  Only recorded arrays are stored.

`compose` updates the density grid three times with random offsets; the grid is not recorded (the forward does not read it), so
the generator skips those sweeps of 128^3 CPU queries.

    python tools/gen_ccnerf_golden.py     (re-running reproduces the file bit for bit)
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

OUT = os.path.join(REPO, "tests", "golden", "ccnerf.npz")
CC_NET = dict(resolution=[20, 17, 13], rank_vec_density=[8, 8, 8], rank_mat_density=[0, 2, 5], rank_vec=[8, 8, 12], rank_mat=[0, 4, 4],
              bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
CC_OTHER = dict(resolution=[9, 14, 11], rank_vec_density=[3, 5], rank_mat_density=[2, 3], rank_vec=[4, 6], rank_mat=[1, 3],
                bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
CC_EMPTY = dict(resolution=[1, 1, 1], rank_vec_density=[1], rank_mat_density=[1], rank_vec=[1], rank_mat=[1],
                bound=2, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10)
COMPOSE = (dict(s=0.4, t=np.array([0.0, 0.2, 0.0])),
           dict(s=0.6, t=np.array([0.3, -0.1, -0.5]),
                R=np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]) @ np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])))


def _shapes(net):
    return np.array([str(tuple(p.shape)) for _, p in net.named_parameters()])


def main():
    _install_reference_stack()
    _stub_training_imports()
    cc = importlib.import_module("tensoRF.network_cc")
    tu = importlib.import_module("tensoRF.utils")
    strainer = importlib.import_module("SealNeRF.trainer")
    for m_ in (cc, tu, strainer):
        _assert_reference(m_)
    syn = _load_synthetic()
    out = {}

    def make(cfg, lo=-0.5, hi=0.5):
        torch.manual_seed(3)
        net = cc.NeRFNetwork(**cfg)
        _seed_params(net, lo, hi)
        return net
    net = make(CC_NET)
    out.update(param_names=np.array([k for k, _ in net.named_parameters()]), param_shapes=_shapes(net))
    groups = net.get_params(2e-2, 1e-3)
    names = {id(p): k for k, p in net.named_parameters()}
    out["group_lrs"] = np.array([g["lr"] for g in groups])
    out["group_members"] = np.array([",".join(names[id(p)] for p in g["params"]) for g in groups])
    x = _seeded((300, 3), 71, -1.12, 1.12)
    d = torch.nn.functional.normalize(_seeded((300, 3), 72, -1, 1), dim=-1)
    net.train()
    sg, cl = net(x, d)
    sg2, cl2 = net(x, d, K=2)
    dl = net.density_loss()
    out.update(fw_x=x.numpy(), fw_d=d.numpy(), train_sigma=sg.detach().numpy(), train_color=cl.detach().numpy(),
               train_k2_sigma=sg2.detach().numpy(), train_k2_color=cl2.detach().numpy(),
               train_density=net.density(x)["sigma"].detach().numpy(), density_loss=np.float64(dl.item()))
    net.eval()
    sg, cl = net(x, d)
    out.update(eval_sigma=sg.detach().numpy(), eval_color=cl.detach().numpy(), eval_density=net.density(x)["sigma"].detach().numpy())
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
    # -- shrink_model + upsample_model (parameter shapes, aabb, a forward on the re-sampled factors)
    net.mean_density = 5.0
    net.density_grid.copy_(torch.from_numpy(dens))
    net.eval()
    with torch.no_grad():
        net.shrink_model()
        out.update(shrink_aabb=net.aabb_train.numpy().copy(), shrink_shapes=_shapes(net))
        net.upsample_model([30, 26, 22])
        out["up_shapes"] = _shapes(net)
        xs = _seeded((200, 3), 95, -0.5, 0.5)
        sg, cl = net(xs, d[:200])
        out.update(up_x=xs.numpy(), up_sigma=sg.numpy(), up_color=cl.numpy())
    # -- finalize() and compress() on a fresh seeded model
    with torch.no_grad():
        net = make(CC_NET).eval()
        net.finalize()
        sg, cl = net(x, d)
        out.update(fin_names=np.array([k for k, _ in net.named_parameters()]), fin_shapes=_shapes(net), fin_sigma=sg.numpy(), fin_color=cl.numpy())
        for k, p in net.named_parameters():
            out["fin_param_" + k.replace(".", "_")] = p.detach().numpy().copy()
        net.compress((4, 2, 4, 2))
        sg, cl = net(x, d)
        out.update(comp_shapes=_shapes(net), comp_sigma=sg.numpy(), comp_color=cl.numpy())
    # -- compose: two finalized seeded models, one of them rotated, into an empty scene
    with torch.no_grad():
        scene = make(CC_EMPTY).eval()
        scene.update_extra_state = lambda *a, **k: None  # (see the module docstring)
        objs = [make(CC_NET).eval(), make(CC_OTHER, -0.6, 0.4).eval()]
        for obj, how in zip(objs, COMPOSE):
            scene.compose(obj, **how)
        xc = _seeded((300, 3), 97, -1.0, 1.0)
        sg, cl = scene(xc, d)
        out.update(cmp_x=xc.numpy(), cmp_sigma=sg.numpy(), cmp_color=cl.numpy(), cmp_density=scene.density(xc)["sigma"].numpy(),
                   cmp_buffers=np.array([k for k, _ in scene.named_buffers()]))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays); train loss {loss.item()} density_loss {dl.item()}")


if __name__ == "__main__":
    main()
